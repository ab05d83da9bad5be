"""The pruning query's plan without a GPU (csrc/tppr_prune.hip: prune_plan through zt_prune_plan, host code only): which
walks stay in LDS and with what launch, which take the workspace form, what a slab costs, how many fit a budget, what is
refused -- and the CPU oracle held to the fixtures the reference itself produced for two walks beyond the LDS form."""
import types

import numpy as np
import pytest

import inputs as I
from conftest import golden

MAX_CAND, MAX_FRONT, PR_WAVES, PR_MAX_MODELS = 1280, 512, 4, 4
SORT_LDS = 4 * (128 + 128 + 130 + 130 + 96) + 8 * 128 + 2 * (128 + 128)      # sizeof(SortLds), numba_sort.hpp
WS_MAX_STATES, WS_MAX_SLABS = 1 << 18, 768


@pytest.fixture(scope="module")
def plan():
    from zebra_amd import build
    build.build()
    from zebra_amd.tppr import NeighborFinder
    return NeighborFinder.pruning_plan


def states(width, depth):
    return sum(width ** d for d in range(1, depth + 1))


def a16(x):
    return (x + 15) & ~15


def lds_form_bytes(cap_c, cap_f, M, k):
    """prune_lds_bytes x PR_WAVES with the models per launch pruned_launch has always picked"""
    one = lambda m: ((2 + m) * a16(cap_c * 8) + a16(cap_c * 4) + a16((64 if k <= 64 else 256) * 4) + a16(96 * 4) +
                     3 * a16(cap_f * 4) + (1 + m) * a16(cap_f * 8) + a16(SORT_LDS))
    mm = min(M, PR_MAX_MODELS)
    while mm > 1 and one(mm) * PR_WAVES > 64 * 1024:
        mm -= 1
    return mm, one(mm) * PR_WAVES


@pytest.mark.parametrize("width,depth,M,k", [(10, 2, 2, 40), (10, 2, 1, 20), (20, 2, 2, 20), (10, 3, 2, 20), (35, 2, 1, 20),
                                             (35, 2, 4, 255), (30, 2, 1, 255), (1280, 1, 1, 20), (8, 3, 5, 63)])
def test_lds_shapes_keep_their_launch(plan, width, depth, M, k):
    p = plan(width, depth, M, k)
    assert p["form"] == "lds"
    assert p["cap_c"] == states(width, depth) <= MAX_CAND and p["cap_f"] == width ** (depth - 1) <= MAX_FRONT
    mm, lds = lds_form_bytes(p["cap_c"], p["cap_f"], M, k)
    assert (p["models_per_launch"], p["lds_bytes"], p["threads"]) == (mm, lds, 64 * PR_WAVES)
    assert p["slab_bytes"] == 0 and p["slabs"] == 0
    assert plan(width, depth, M, k, 0)["form"] == "lds"            # no budget needed


@pytest.mark.parametrize("width,depth,n", [(36, 2, 1332), (11, 3, 1463), (1281, 1, 1281), (23, 3, 12719), (40, 2, 1640),
                                           (50, 2, 2550), (20, 3, 8420), (10, 4, 11110), (6, 5, 9330), (3000, 1, 3000),
                                           (50, 3, 127550), (10, 5, 111110)])
def test_wider_walks_take_the_workspace(plan, width, depth, n):
    p = plan(width, depth, 2, 20)
    assert p["form"] == "workspace" and p["cap_c"] == p["states"] == n == states(width, depth)
    assert p["cap_f"] == width ** (depth - 1)
    assert p["threads"] == 256 and p["grid"] == p["slabs"] >= 1 and p["models_per_launch"] == 2
    # a slab holds at least the LDS form's arrays at that size (keys, times, one weight column per model, first occurrences)
    assert p["slab_bytes"] >= n * (8 + 8 + 2 * 8 + 4) and p["slab_bytes"] % 256 == 0


def test_frontier_alone_sends_a_walk_to_the_workspace(plan):
    # 23 x 3's frontier (529 entries) is beyond the LDS form's 512
    p = plan(23, 3, 1, 20)
    assert p["form"] == "workspace" and p["cap_f"] == 529 > MAX_FRONT


def test_slab_bytes_monotone_in_states_and_models(plan):
    shapes = sorted([(36, 2), (11, 3), (40, 2), (50, 2), (3000, 1), (20, 3), (6, 5), (10, 4), (10, 5), (50, 3)],
                    key=lambda s: states(*s))
    for M in (1, 2, 3, 4):
        b = [plan(w, d, M, 20)["slab_bytes"] for w, d in shapes]
        assert all(x <= y for x, y in zip(b, b[1:])), b
    for w, d in shapes:
        b = [plan(w, d, M, 20)["slab_bytes"] for M in (1, 2, 3, 4)]
        assert all(x < y for x, y in zip(b, b[1:])), b
        assert plan(w, d, 7, 20)["slab_bytes"] == b[3] and plan(w, d, 7, 20)["models_per_launch"] == PR_MAX_MODELS


def test_slabs_fill_the_budget_up_to_the_cap(plan):
    one = plan(20, 3, 2, 20)["slab_bytes"]
    for budget in (one, 3 * one, 3 * one + one - 1, 17 * one + 5, 1 << 30):
        p = plan(20, 3, 2, 20, budget)
        assert p["slabs"] == min(budget // one, WS_MAX_SLABS) and p["form"] == "workspace"
    assert plan(20, 3, 2, 20, 1 << 40)["slabs"] == WS_MAX_SLABS    # capped by what the device keeps resident
    p = plan(20, 3, 2, 20, one - 1)
    assert p["form"] == "refused" and p["slabs"] == 0 and p["slab_bytes"] == one
    from zebra_amd import _capi
    assert str(one).encode() in _capi.lib().zt_last_error()          # the message names the bytes one slab needs


def test_beyond_the_bound_is_refused(plan):
    assert WS_MAX_STATES >= 1 << 17
    for width, depth in ((100, 3), (64, 3), (512, 2), (10, 6), (WS_MAX_STATES + 1, 1), (2, 40)):
        assert states(width, depth) > WS_MAX_STATES
        assert plan(width, depth, 1, 20)["form"] == "refused"
    assert plan(WS_MAX_STATES, 1, 1, 20)["form"] == "workspace"
    assert plan(10, 2, 1, 256)["form"] == "refused" and plan(20, 3, 1, 256)["form"] == "refused"   # k beyond ZT_MAX_K_WIDE
    with pytest.raises(ValueError):
        plan(0, 2, 1, 20)
    with pytest.raises(ValueError):
        plan(10, 2, 1, 20, -1)


@pytest.mark.parametrize("name,width,depth", [("w36d2_k20", 36, 2), ("w11d3_k20", 11, 3)])
def test_oracle_matches_the_reference_on_wide_walks(oracle, name, width, depth):
    """The CPU oracle against the reference's own get_pruned_topk beyond the LDS form (gen_golden_wide_prune.py)."""
    g = golden("g13_prune_" + name)
    src, dst, neg, ts, eidx = I.make_stream("hub", 400, 24000, 305)
    csr = oracle.CsrOracle(src, dst, eidx, ts, int(max(src.max(), dst.max())) + 1)
    nq, k = g["nodes"].shape
    assert (nq, k) == (24, 20)
    outs = [np.zeros((nq, k), dt) for dt in (np.int32, np.int32, np.float32, np.float32)]
    csr.get_pruned_topk(g["q_nodes"], g["q_ts"], width, depth, 0.1, 0.5, k, *outs)
    for x, nm in zip(outs, ("nodes", "eidx", "dt", "w")):
        assert np.array_equal(x, g[nm]), nm
    assert (np.count_nonzero(g["w"], axis=1) == k).any()
