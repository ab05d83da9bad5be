"""The head of a hub chain (k_stream's chain workgroups): hop records packed by the prepass, the hub's scale table filled
block by block ahead of the hops.  The streaming update against ``oracle/pyoracle.py::TpprOracle`` on star-shaped streams:
ONE node takes L edges of ONE launch, the rest of the launch is filler among the other nodes (in the small launches nobody
else reaches HOT_MIN = 24 accesses).  Emitted rows and the dictionaries of every touched node must be the oracle's bit for bit
(reference utils/util.py:473-576), on a fresh handle (hub row empty, versions and scale table just allocated) and on the
warm state a second launch finds.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 512
AL, BE = [0.1, 0.1], [0.5, 0.95]
FUSED_FILL, BIG_B = 300, 1500        # 3 (L + 300) <= 4096 accesses: the single-workgroup prepass; 3 * 1500: the eleven launches


@pytest.fixture(scope="module")
def zt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd import tppr
    return tppr


def star_launch(rng, B, hubs, first_eidx, t0, loops=(), joins=0, hub_negs=0):
    """One launch of B edges.  hubs = [(node, L), ..]: node takes L edges at random places of the launch, alternately as source
    and destination, partners drawn from the filler nodes; ``loops``: chain positions of hubs[0] that are self-loops;
    ``joins``: that many of hubs[0]'s edges (and of hubs[1]'s) are edges between the two; ``hub_negs``: negatives equal to
    hubs[0] (readers of its versions).  Filler edges walk round the other nodes so that each gets ~3 B / N accesses."""
    hub_ids = [h for h, _ in hubs]
    others = np.array([x for x in range(N) if x not in hub_ids], np.int32)
    n_hub = sum(L for _, L in hubs) - joins
    assert n_hub <= B
    src = np.empty(B, np.int32)
    dst = np.empty(B, np.int32)
    places = np.sort(rng.choice(B, n_hub, replace=False))
    # which hub each hub place belongs to, in random order; a join serves both
    owner = np.concatenate([[0] * (hubs[0][1] - joins)] + [[q] * (L - (joins if q == 1 else 0)) for q, (_, L) in list(enumerate(hubs))[1:]]
                           + [[-1] * joins]).astype(np.int64)
    rng.shuffle(owner)
    is_hub = np.zeros(B, bool)
    is_hub[places] = True
    pos0 = 0                                          # chain position of hubs[0] at the edge being made
    fill_i = 0
    oi = 0
    for i in range(B):
        if not is_hub[i]:
            src[i] = others[(2 * fill_i) % len(others)]
            dst[i] = others[(2 * fill_i + 1) % len(others)]
            fill_i += 1
            continue
        o = owner[oi]
        oi += 1
        if o == -1:
            a, b = hub_ids[0], hub_ids[1]
        else:
            a = hub_ids[o]
            b = a if (o == 0 and pos0 in loops) else int(others[rng.integers(len(others))])
        if o in (0, -1):
            pos0 += 1
        src[i], dst[i] = (a, b) if i % 2 == 0 else (b, a)
    neg = others[rng.integers(len(others), size=B)].astype(np.int32)
    if hub_negs:
        neg[rng.choice(B, hub_negs, replace=False)] = hub_ids[0]
    ts = t0 + np.cumsum(rng.integers(1, 4, size=B)).astype(np.float64)
    eidx = np.arange(first_eidx, first_eidx + B, dtype=np.int64)
    return src, dst, neg, ts, eidx


def run_case(zt, oracle, k, seed, launches, al=None, be=None):
    """launches: list of dicts for star_launch (B, hubs, ..).  A fresh finder; every launch compared.  al, be: the models'
    alpha / beta lists (AL, BE where not given)."""
    al, be = AL if al is None else al, BE if be is None else be
    rng = np.random.default_rng(seed)
    f = zt.tppr_finder(N, k, len(al), al, be)
    o = oracle.TpprOracle(N, k, len(al), al, be)
    e0, t0 = 1, 0.0
    for n, spec in enumerate(launches):
        src, dst, neg, ts, eidx = star_launch(rng, first_eidx=e0, t0=t0, **spec)
        e0, t0 = e0 + len(src), float(ts[-1])
        nodes = np.concatenate([src, dst, neg])
        a = f.streaming_topk(nodes, ts, eidx)
        f.check_status()
        b = o.streaming_topk(nodes, ts, eidx)
        what = "k %d seed %d launch %d %r" % (k, seed, n, spec)
        for x, y, nm in zip(a, b, ("nodes", "eidx", "dt", "w")):
            assert np.array_equal(np.stack(x), np.stack(y)), "emitted %s differs: %s" % (nm, what)
        ids = np.unique(nodes).astype(np.int64)
        for m in range(len(al)):
            sa, sb = f.export_rows(m, ids), o.export_rows(m, ids)
            for kk in ("len", "norm", "eidx", "node", "ts", "w"):
                assert np.array_equal(sa[kk], sb[kk]), "state %s of model %d differs: %s" % (kk, m, what)


SWEEP = [(24, 67), (68, 111), (112, 155), (156, 200)]


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("lo,hi", SWEEP)
def test_every_chain_length(zt, oracle, k, lo, hi):
    """Every L from 24 to 200 (the first block of the scale table, its edge and the blocks behind it), the hub at node 0,
    two launches each: the first on a fresh handle, the second on the state it left.  L = 23 -- no chain -- runs the same
    stream as the control."""
    for L in ([23] if lo == 24 else []) + list(range(lo, hi + 1)):
        spec = dict(B=L + FUSED_FILL, hubs=[(0, L)])
        run_case(zt, oracle, k, 1000 + L, [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("L", [24, 63, 64, 65, 127, 128, 129, 200])
def test_chain_lengths_eleven_launch_prepass(zt, oracle, k, L):
    """The prepass as eleven launches (more than 4096 accesses) writes the same records."""
    spec = dict(B=BIG_B, hubs=[(0, L)])
    run_case(zt, oracle, k, 2000 + L, [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("L", [2047, 2048, 2049])
def test_chain_lengths_around_ch_max(zt, oracle, k, L):
    """A chain holds CH_MAX = 2048 positions; the hub's later edges go through the general queue."""
    spec = dict(B=L + 1000, hubs=[(0, L)])
    run_case(zt, oracle, k, 3000 + L, [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("B", [FUSED_FILL, BIG_B])
@pytest.mark.parametrize("L", [24, 65, 130])
def test_self_loops_of_the_hub(zt, oracle, k, B, L):
    """A self-loop of the hub at chain position 0, at a middle position, at both (process_edge takes those hops)."""
    Bt = B + L if B == FUSED_FILL else B
    for loops in ((0,), (L // 2,), (0, L // 2, L - 1)):
        spec = dict(B=Bt, hubs=[(0, L)], loops=loops)
        run_case(zt, oracle, k, 4000 + L + loops[0], [spec, spec])


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("B", [FUSED_FILL, BIG_B])
@pytest.mark.parametrize("L0,L1,joins", [(40, 30, 6), (100, 70, 25), (150, 24, 24)])
def test_two_hubs_joined(zt, oracle, k, B, L0, L1, joins):
    """Two hubs with edges between them: both chains hold those edges (HopRec::pchain), each reads the other's row by
    version; negatives equal to the first hub read its versions too."""
    Bt = B + L0 + L1 if B == FUSED_FILL else B
    spec = dict(B=Bt, hubs=[(0, L0), (1, L1)], joins=joins, hub_negs=5)
    run_case(zt, oracle, k, 5000 + L0, [spec, spec])
