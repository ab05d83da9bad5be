"""Hub-chain hops that stay in chain_hop's lean critical section (k_stream, zebra_amd/csrc/tppr_chain.hpp) where they used to
leave it: a self-loop of the hub (every key meets itself: weight (w * scale_s1) + (w * scale_s2), one new candidate), the hop
behind a hop of the general code (process_edge publishes a pruned row as the sorted arrangement it is), and a hop that only
lacks the identities of a straddling run's members (it waits for the predecessor's order and carries on).  Star-shaped streams
as in test_chain_head_gpu.py: N = 512, one or two hubs, B = L + 300 (the fused prepass) and B = 1500 (the eleven launches),
two launches per case (a fresh handle, then the warm state), k = 20 and k = 5, both models (beta 0.5 and 0.95).  Emitted rows
and the exported state of every touched node must equal ``oracle/pyoracle.py::TpprOracle`` under ``np.array_equal``.

Which way the hops of these streams went, counted once with the critical-section diagnostic build (tools/build_variant.sh crit
-DZT_CRIT; the LEANC counters of chain_hop, model 0 = beta 0.5 only) over this whole file:
    lean hops 38 980, of them: self-loops 1 969, hops right behind a self-loop 1 863, carried on after the wait for the
    predecessor's order 112 (an alternate may be in the row 72, a picked member is kept 40);
    left to the general code: row not a sorted arrangement / norm 1 061 (the fresh hubs' rows while they fill), key match or
    NaN 1 098, both slot functions clash 45.
The tests compare results only, and every new path has a bit-identical fallback in the general code: the counts above are a
record of one run, not something a later run asserts (the counters exist in the diagnostic build only).
"""
import numpy as np
import pytest

from test_chain_head_gpu import BIG_B, FUSED_FILL, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd import tppr
    return tppr


def loop_sets(L):
    """Self-loops at positions {1}, {1, 2}, {L-2, L-1}, every second position, every third position (position 0 is
    process_edge's in any case)."""
    return [(1,), (1, 2), (L - 2, L - 1), tuple(range(1, L, 2)), tuple(range(1, L, 3))]


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("B", [FUSED_FILL, BIG_B])
@pytest.mark.parametrize("L", [24, 65, 130])
def test_self_loops_stay_lean(zt, oracle, k, B, L):
    """The warm launch finds the hub's row full: its self-loops take the lean section, singly, in pairs (the second one behind a
    lean self-loop), at the chain's end (the last hop also stores to memory), and densely (every second / third position)."""
    Bt = B + L if B == FUSED_FILL else B
    for n, loops in enumerate(loop_sets(L)):
        spec = dict(B=Bt, hubs=[(0, L)], loops=loops)
        run_case(zt, oracle, k, 6000 + 10 * L + n, [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("B", [FUSED_FILL, BIG_B])
def test_fresh_hub_loops_while_the_row_fills(zt, oracle, k, B):
    """Self-loops at every position from 1 to k + 2 of a fresh hub: the row is not full there (a self-loop adds one entry per
    hop), nothing is pruned, process_edge publishes `sorted = 0` and keeps those hops; the first pruned row switches over.
    (What is checked is the result: a wrong `sorted = 1` on such a row would be caught by the lean section's own "no prune" exit
    and fall back, bit for bit the same.)"""
    L = 40
    Bt = B + L if B == FUSED_FILL else B
    spec = dict(B=Bt, hubs=[(0, L)], loops=tuple(range(1, k + 3)))
    run_case(zt, oracle, k, 7000 + k, [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("B", [FUSED_FILL, BIG_B])
@pytest.mark.parametrize("L0,L1,joins", [(40, 30, 6), (100, 70, 25)])
def test_two_hubs_joined_with_loops(zt, oracle, k, B, L0, L1, joins):
    """Two joined hubs, self-loops on the first (every second position that is not a join), the first hub as a negative sample
    around them: the other chain and the negatives read the versions the lean self-loops store."""
    Bt = B + L0 + L1 if B == FUSED_FILL else B
    spec = dict(B=Bt, hubs=[(0, L0), (1, L1)], joins=joins, hub_negs=8, loops=tuple(range(1, L0, 2)))
    run_case(zt, oracle, k, 8000 + L0, [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("seed", range(10))
def test_straddling_runs_carry_on_after_the_order(zt, oracle, k, seed):
    """L = 200: on the beta = 0.5 model many weights are equal (powers of two times the same factors), runs of equal weights
    straddle the cut and their picked members are kept one hop later: those hops wait for the predecessor's order and go on."""
    L = 200
    spec = dict(B=(L + FUSED_FILL) if seed % 2 == 0 else BIG_B, hubs=[(0, L)], loops=(50, 51, 120) if seed >= 5 else ())
    run_case(zt, oracle, k, 9000 + seed, [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("seed", range(4))
def test_long_chain_keeps_picked_members(zt, oracle, k, seed):
    """L = 1400 of B = 1500: the partners come back every few hundred hops with rows made of the hub's own old entries, small
    against the hub's; many of their candidates fall below the cut and the PICKED members of a straddling run are kept one hop
    later -- the second way into the order wait (the key tests are made again on the final keys)."""
    spec = dict(B=BIG_B, hubs=[(0, 1400)])
    run_case(zt, oracle, k, 9300 + seed, [spec, spec])
