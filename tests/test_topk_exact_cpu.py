"""The planted top-K cases without a GPU (tests/helpers_topk_planted.py): the dialled MergeLayer gives sigmoid(+-u) exactly on
the CPU, a host model of the kernel's list shows which list positions a case's inserts reach, every case reaches the plan its id
names (_capi.topk_plan), and the plan's bounds hold over the cross of its edges."""
import itertools

import numpy as np
import pytest
import torch

import helpers_topk_planted as P


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def _merge_layer(H, dtype):
    from zebra_amd.modules import MergeLayer
    m = MergeLayer(H, H, H, 1)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), P.scorer_weights(H)):
            p.copy_(torch.from_numpy(w))
    return m.to(dtype)


def _ordered_like(values, S):
    """distinct scores give strictly ordered values, equal scores equal values (along the last axis of one row)"""
    order = np.argsort(S, kind="stable")
    s, v = S[order], values[order]
    up = s[1:] > s[:-1]
    return bool((v[1:][up] > v[:-1][up]).all() and (v[1:][~up] == v[:-1][~up]).all())


# ---- 1. the dial --------------------------------------------------------------------------------------------------------
def test_float32_sigmoid_orders_every_level():
    """all levels and the special values: strictly increasing in float32, 1.0f at U_ONE, +0.0f at -U_ZERO, 0.5f at 0"""
    u = np.concatenate([-P.lev(np.arange(P.MAX_LEVEL, 0, -1)), P.lev(np.arange(P.MAX_LEVEL + 1))])
    s = torch.sigmoid(torch.from_numpy(u.astype(np.float32))).numpy()
    assert (np.diff(s.view(np.uint32).astype(np.int64)) > 0).all()
    fine = np.arange(16385, dtype=np.float64) * (6.0 / 16384)          # the grid the levels are 15 apart on
    sf = torch.sigmoid(torch.from_numpy(fine.astype(np.float32))).numpy()
    assert np.diff(sf.view(np.uint32).astype(np.int64)).min() >= 1
    edge = torch.sigmoid(torch.tensor([P.U_ONE, -P.U_ZERO, 0.0], dtype=torch.float32)).numpy()
    assert edge.view(np.uint32).tolist() == np.array([1.0, 0.0, 0.5], np.float32).view(np.uint32).tolist()
    assert s.max() < 1.0 and s.min() > 0.0


DIAL_CASES = ["ladder-shared-K256", "ladder-indexed-K65", "tiles-shared-Q9", "tiles-indexed-Q5", "extreme-ones-shared-K10",
              "extreme-fewabovezero-indexed-K65", "extreme-H1028-coord1027-shared-K65", "accumulate-ones-shared-K64",
              "orders-shared-K65-C131"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("cid", DIAL_CASES)
def test_the_dial_gives_sigmoid_of_the_planted_score(cid, dtype):
    case = P.BY_ID[cid]
    d = case.data()
    m = _merge_layer(case.H, dtype)
    eq, ec = torch.from_numpy(d["emb_q"]).to(dtype), torch.from_numpy(d["emb_c"]).to(dtype)
    for q in range(case.Q):
        S = d["S"][d["dial_of"][q]]
        live = ~np.isnan(S)
        rows = np.arange(case.C) if d["idx"] is None else d["idx"][q]
        with torch.no_grad():
            logit = m(eq[q:q + 1].expand(int(live.sum()), -1), ec[rows[live]]).squeeze(1)
        assert np.array_equal(logit.numpy().astype(np.float64), S[live]), (cid, q)        # the score itself, exactly
        # (torch's CPU sigmoid rounds the vector body and the scalar tail of an array differently: whole vectors only)
        n = logit.numel()
        pad = torch.cat([logit, logit[-1:].expand(-n % 64)])
        prob = torch.sigmoid(pad).numpy()[:n]
        want = torch.sigmoid(torch.from_numpy(np.concatenate([S[live], np.repeat(S[live][-1:], -n % 64)])).to(dtype)).numpy()[:n]
        assert np.array_equal(prob, want)
        assert _ordered_like(prob, S[live]), (cid, q)


# ---- 2. the host model of the list ---------------------------------------------------------------------------------------
def _edges(K):
    return sorted(set(p for p in (0, 63, 64, 127, 128, 191, 192, 255) if p < K) | {K - 1})


def test_model_list_on_hand_made_batches():
    m = P.ModelList(3)
    m.offer([(-1.0, 0), (-3.0, 1), None, (-2.0, 2)])                   # scores 1, 3, 2: positions 0, 0, 1
    assert m.log == [0, 0, 1] and [k[1] for k in m.keys] == [1, 2, 0]
    m.offer([(-1.0, 5), (-2.0, 1)])                                    # 1.0 again, larger index: out; 2.0 with index 1: before 2
    assert m.log == [0, 0, 1, 1] and [k[1] for k in m.keys] == [1, 1, 2]
    m.offer([(-0.5, 9)])
    assert len(m.log) == 4


POSITION_CASES = [c for c in P.CASES if c.positions]


@pytest.mark.parametrize("case", POSITION_CASES, ids=repr)
def test_ladder_inserts_land_on_every_edge_of_the_list(case, capi):
    """the pair kernel's own running list (the wave that sees the ladder; the query's wave in the indexed form) takes an insert
    at positions 0, 63, 64, 127, 128, 191, 192, 255 (those below K) and K - 1 -- at every position, in fact, and the second half
    of the ladder at K-1, K-2, .. in that order -- and the model's result is the host expectation"""
    d, K = case.data(), case.K
    pl = case.plan(capi)
    assert pl["n_spans"] == 1 and pl["n_slabs"] == 1
    want, _ = P.expected(d["S"], K)
    for q in range(case.Q):
        dial = d["dial_of"][q]
        keys, stages = P.model_query(d["S"][dial], None, K, case.shared, pl["span_cols"], pl["n_spans"])
        log = stages["wave%d" % (q % 3)] if case.shared else stages["pairs"]
        assert set(_edges(K)) <= set(log), (case.id, q)
        n = P.ladder_shape(K, case.shared)[1]
        assert log[:K] == list(range(K)) and log[K:] == list(range(K - 1, 2 * K - 1 - n, -1)), (case.id, q)
        got = [k[1] for k in keys] + [-1] * (K - len(keys))
        assert got == want[dial].tolist(), (case.id, q)


@pytest.mark.parametrize("cid", ["tie-span-shared-K65", "tie-span-indexed-K10", "spans-shared-Nc2500-partial-K100-laststep",
                                 "spans-indexed-C512-K65-lastspan", "orders-shared-K64-C129", "orders-indexed-K129-C1000",
                                 "masked-winners-ladder-shared-K129", "accumulate-smaller-shared-K65",
                                 "accumulate-ones-shared-K129"])
def test_model_agrees_with_the_host_expectation(cid, capi):
    """whatever the spans, the waves and the merges: the model's list ends as lexsort(-level, column)[:K]"""
    case = P.BY_ID[cid]
    d, K = case.data(), case.K
    pl = case.plan(capi)
    base = P.IDX_BASE_ACC if d["incoming"] is not None else 0
    want, _ = P.expected(d["S"], K, d["mask"], base, d["incoming"])
    for dial in range(d["D"]):
        inc = None if d["incoming"] is None else (d["incoming"]["idx"][dial], d["incoming"]["s"][dial])
        keys, _ = P.model_query(d["S"][dial], None if d["mask"] is None else d["mask"][dial], K, case.shared, pl["span_cols"],
                                pl["n_spans"], incoming=inc, idx_base=base)
        assert [k[1] for k in keys] + [-1] * (K - len(keys)) == want[dial].tolist(), (cid, dial)


@pytest.mark.parametrize("case", [c for c in P.CASES if c.id.startswith("lastslot-")], ids=repr)
def test_lastslot_inserts_at_the_end_of_a_merged_list(case, capi):
    """the merge of the four waves' lists (wave) or of the spans' lists (span) begins with the K-1 best in place: whatever it
    inserts lands at position K-1, and the planted K-th best is what stays there"""
    d, K = case.data(), case.K
    pl = case.plan(capi)
    want, _ = P.expected(d["S"], K)
    for dial in range(d["D"]):
        keys, stages = P.model_query(d["S"][dial], None, K, case.shared, pl["span_cols"], pl["n_spans"])
        log = stages["wave_merge"] if "-wave-" in case.id else stages["merge"][K:]
        assert len(log) > 0 and set(log) == {K - 1}, (case.id, dial, log)
        assert [k[1] for k in keys] == want[dial].tolist() and d["u"][dial, keys[-1][1]] == P.lev(500)


# ---- 3. every case reaches the seam its id names ---------------------------------------------------------------------------
NAMED = ("ladder-", "tie-span-", "tie-slab", "spans-", "tiles-", "masked-winners-", "lastslot-")


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_case_reaches_the_plan_its_id_names(case, capi):
    pl = case.plan(capi)
    assert pl["form"] == (capi.TOPK_FORM_LANE if case.K <= 64 else capi.TOPK_FORM_LANE4)
    assert pl["wave_queries"] == (4 if case.shared else 1)
    if case.id.startswith(NAMED):
        assert case.reach, case.id
    for name, want in case.reach.items():
        assert pl[name] == want, (case.id, name, pl[name], want)
    if case.ws_rows is not None:
        assert pl["slab_rows"] == case.ws_rows and pl["n_slabs"] > 1
    else:
        assert pl["n_slabs"] == 1
    # the boundary a tie case names lies where the plan puts it
    d = None
    if case.id.startswith("tie-span-"):
        d, b = case.data(), pl["span_cols"]
    elif case.id.startswith("tie-slab"):
        d, b = case.data(), 2 * pl["slab_rows"]
    if d is not None:
        for dial in range(d["D"]):
            S = d["S"][dial]
            tie = S[b - 2:b + 2]
            assert (tie == tie[0]).all() and (S > tie[0]).sum() == case.K - 2 and (S == tie[0]).sum() == 4
    if case.pieces is not None:
        assert sorted(case.pieces) == [(0, 100), (100, case.C)]
    if "laststep" in case.id:
        assert case.C % P.STEP[case.shared] != 0 or case.C == pl["n_spans"] * pl["span_cols"]
    if case.id.startswith("spans-cap-"):
        assert pl["n_spans"] == 2 and case.C // (P.STEP[case.shared] * 8) == 4       # 4 spans would fit; the cap says 2
        assert pl["n_spans"] == -(-2048 // pl["q_tiles"])


def test_the_planted_cases_cover_their_families():
    ids = set(P.BY_ID)
    for K in P.LADDER_K:
        assert {"ladder-shared-K%d" % K, "ladder-indexed-K%d" % K} <= ids
    for K in P.ORDER_K:
        for C_ in (K - 1, K, K + 1, 2 * K + 1, 1000):
            assert {"orders-shared-K%d-C%d" % (K, C_), "orders-indexed-K%d-C%d" % (K, C_)} <= ids
    for Q in (1, 2, 3, 4, 5, 7, 8, 9):
        assert {"tiles-shared-Q%d" % Q, "tiles-indexed-Q%d" % Q} <= ids
    assert max(c.Q * c.C for c in P.CASES) == 4096 * 4096
    assert all(c.K <= 256 and 4 * c.K + 2 <= P.MAX_LEVEL for c in P.CASES)


# ---- 4. the plan's bounds ------------------------------------------------------------------------------------------------
PLAN_Q = (1, 4, 5, 2047, 2048, 8191, 8192, 8193, 100000)
PLAN_H = (4, 300, 4352)
PLAN_K = (1, 64, 65, 256)
PLAN_C = (1, 255, 256, 257, 2047, 2048, 10 ** 6)


@pytest.mark.parametrize("indexed", [False, True], ids=["shared", "indexed"])
@pytest.mark.parametrize("H", PLAN_H)
def test_topk_plan_bounds(H, indexed, capi):
    import ctypes as C
    ws = capi.lib().zt_affinity_topk_workspace_bytes
    for Q, K, C_ in itertools.product(PLAN_Q, PLAN_K, PLAN_C):
        Nc = C_
        full = int(ws(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H), C.c_int32(K)))
        least = int(ws(C.c_int64(Q), C.c_int64(32), C.c_int32(H), C.c_int32(K)))
        for bytes_ in (full, least):
            pl = capi.topk_plan(Q, Nc, C_, H, K, indexed, bytes_)
            what = (Q, H, K, C_, indexed, bytes_ == full, pl)
            cols = C_ if indexed else min(pl["slab_rows"], max(Nc, 1))
            step = 32 if indexed else 128
            assert pl["q_tiles"] == (Q + 3) // 4, what
            assert pl["lists_offset"] + Q * pl["n_spans"] * K * 8 <= pl["pc_offset"], what      # the lists fit their region
            assert pl["pc_offset"] + pl["slab_rows"] * H * 4 <= bytes_, what                    # ... and the slab the rest
            assert 1 <= pl["n_spans"] <= -(-2048 // pl["q_tiles"]), what
            assert pl["n_spans"] * pl["span_cols"] >= cols, what
            assert (pl["n_spans"] - 1) * pl["span_cols"] < cols, what
            assert pl["span_cols"] > 0 and pl["span_cols"] % step == 0, what
            assert pl["slab_rows"] >= 32 and pl["slab_rows"] % 32 == 0, what
            assert pl["n_slabs"] * pl["slab_rows"] >= Nc and (pl["n_slabs"] - 1) * pl["slab_rows"] < max(Nc, 1), what
            assert pl["grid_pairs"] == pl["q_tiles"] * pl["n_spans"] and pl["grid_merge"] == (Q + 3) // 4, what
            if bytes_ == least:
                assert pl["slab_rows"] == 32 and pl["min_bytes"] == least, what
