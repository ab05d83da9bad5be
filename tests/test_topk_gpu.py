"""Top-K link scoring on the GPU: zt_affinity_topk (TGN.topk_scores) against the numpy selection over zt_affinity_rank's own
probabilities, bit for bit -- ties, slabs and spans, accumulate, skip / NaN / range --, against a float64 MergeLayer, and
TGN.recommend against rank_candidates."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn
from helpers_query import merge_f64
from helpers_topk import select_topk

pytestmark = pytest.mark.gpu
TOL = 1e-4            # the project's tolerance for a probability (tests/test_query_gpu.py)
# hidden width H = D (n_tppr + 1) -> (D, n_tppr) of the weight generator; 1028 is the smallest width above one LDS chunk
WIDTHS = {4: (2, 1), 20: (10, 1), 300: (100, 2), 1028: (257, 3)}


@functools.lru_cache(maxsize=None)
def _weights(H):
    D, M = WIDTHS[H]
    return I.model_weights(D, 1, 20, M, 7 + H)


@functools.lru_cache(maxsize=None)
def _ranker(H):
    """TGN.rank_scores / topk_scores on a MergeLayer of width H alone (some widths have no (D, M) a TGN takes)"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN
    m = MergeLayer(H, H, H, 1)
    w = _weights(H)
    with torch.no_grad():
        for p, key in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), ("aff1_w", "aff1_b", "aff2_w", "aff2_b")):
            p.copy_(torch.from_numpy(w[key]))
    holder = types.SimpleNamespace(affinity_score=m.to("cuda"), device=torch.device("cuda"))
    for name in ("rank_scores", "topk_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    return holder


@functools.lru_cache(maxsize=None)
def _inputs(Q, C_, H, shared, Nc=None, scale=1.0):
    """(emb_q, emb_c, cand_idx or None) as CUDA tensors plus the numpy cand_idx, and zt_affinity_rank's own prob [Q, C] on
    the host -- computed once per shape and left unchanged.  Indexed: repeats, 15 % absent, the last row all absent (Q > 1),
    Nc != C."""
    rng = np.random.RandomState(1000 * Q + 10 * C_ + H + (1 if shared else 0))
    if Nc is None:
        Nc = C_ if shared else max(2, C_ // 2 + 3)
    emb_q = (rng.standard_normal((Q, H)) * 0.7).astype(np.float32)
    emb_c = (rng.standard_normal((Nc, H)) * 0.7 * scale).astype(np.float32)
    idx = None
    if not shared:
        idx = rng.randint(0, Nc, (Q, C_)).astype(np.int32)
        idx[rng.random_sample((Q, C_)) < 0.15] = -1
        if Q > 1:
            idx[-1] = -1
    eq, ec = torch.from_numpy(emb_q).cuda(), torch.from_numpy(emb_c).cuda()
    ix = None if shared else torch.from_numpy(idx).cuda()
    prob = _ranker(H).rank_scores(eq, ec, ix).cpu().numpy()
    return eq, ec, ix, idx, prob


def _same(got, want, what=""):
    gi, gp = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gi.dtype == np.int32 and gp.dtype == np.float32 and gi.shape == want[0].shape and gp.shape == want[1].shape
    assert np.array_equal(gi, want[0]), "indices differ %s" % (what,)
    assert np.array_equal(gp.view(np.uint32), want[1].view(np.uint32)), "probabilities differ %s" % (what,)


def _ws_bytes(Q, Nc, H, K):
    from zebra_amd._capi import lib
    return int(lib().zt_affinity_topk_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H), C.c_int32(K)))


# ---- 1. exact against the parent's scorer ---------------------------------------------------------------------------------
# every Q in {1, 5, 17}, C in {1, 31, 33, 64, 65, 300, 2500}, K in {1, 10, 64, 65, 256}, H in {4, 300, 1028}; C < K; 2500 with
# K = 64 and K = 65 (the two forms over several spans)
EXACT = [(1, 1, 1, 4), (5, 31, 64, 300), (17, 33, 10, 4), (5, 64, 65, 300), (17, 65, 256, 1028), (5, 300, 256, 300),
         (17, 2500, 64, 300), (17, 2500, 65, 300), (1, 300, 10, 1028), (5, 2500, 10, 4)]


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "indexed"])
@pytest.mark.parametrize("Q,C_,K,H", EXACT)
def test_topk_equals_the_selection_over_the_rank_scorer(Q, C_, K, H, shared):
    eq, ec, ix, idx, prob = _inputs(Q, C_, H, shared)
    want = select_topk(prob, idx, K)
    rk = _ranker(H)
    got = rk.topk_scores(eq, ec, K, cand_idx=ix)
    again = rk.topk_scores(eq, ec, K, cand_idx=ix)
    _same(got, want, (Q, C_, K, H, shared))
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    if not shared and Q > 1:
        assert (want[0][-1] == -1).all() and not want[1][-1].any()           # the all-absent row: -1 and 0
    if C_ < K:
        assert (want[0][0, C_:] == -1).all()


# ---- 2. ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 65])
def test_topk_ties_between_repeated_candidates(K):
    """indices drawn from three rows: whole groups of candidates share their bits, the index alone orders them"""
    eq, ec, ix, idx, prob = _inputs(17, 300, 300, False, Nc=3)
    assert len(np.unique(prob[0][idx[0] >= 0])) <= 3
    _same(_ranker(300).topk_scores(eq, ec, K, cand_idx=ix), select_topk(prob, idx, K), K)


def test_topk_ties_at_saturation():
    """emb_c scaled by 40: above s ~ 17.4 float32's sigmoid is exactly 1.0f, so many candidates tie at the top"""
    K = 10
    eq, ec, ix, idx, prob = _inputs(5, 300, 300, True, scale=40.0)
    ones = (prob == np.float32(1.0)).sum(axis=1)
    print("candidates at exactly 1.0f per query:", ones.tolist())
    if ones.max() < K + 5:
        pytest.skip("THE DRAW GIVES NO SATURATED TIES (%s at 1.0f): this test checked nothing" % ones.tolist())
    _same(_ranker(300).topk_scores(eq, ec, K), select_topk(prob, None, K))


# ---- 3. slabs and spans do not show -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "indexed"])
@pytest.mark.parametrize("Q,C_,K", [(17, 300, 10), (17, 2500, 65), (5, 2500, 10)])
def test_topk_is_the_same_from_the_smallest_workspace(Q, C_, K, shared):
    from zebra_amd import _capi
    H = 300
    eq, ec, ix, idx, prob = _inputs(Q, C_, H, shared)
    Nc = ec.shape[0]
    least, full = _ws_bytes(Q, 32, H, K), _ws_bytes(Q, Nc, H, K)
    small_plan = _capi.topk_plan(Q, Nc, C_, H, K, not shared, least)
    assert least < full and small_plan["slab_rows"] == 32 and small_plan["n_slabs"] == (Nc + 31) // 32 > 1
    rk = _ranker(H)
    small = rk.topk_scores(eq, ec, K, cand_idx=ix, workspace_bytes=least)
    big = rk.topk_scores(eq, ec, K, cand_idx=ix)
    assert torch.equal(small[0], big[0]) and torch.equal(small[1].view(torch.int32), big[1].view(torch.int32))
    _same(small, select_topk(prob, idx, K))


# ---- 4. accumulate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 100])
def test_topk_accumulates_a_pool_given_in_pieces(K):
    Q, H, N = 17, 300, 700
    eq, ec, _, _, prob = _inputs(Q, N, H, True)
    want = select_topk(prob, None, K)
    rk = _ranker(H)
    _same(rk.topk_scores(eq, ec, K), want)
    pieces = [(0, 100), (100, 450), (450, 700)]
    for order in ((0, 1, 2), (2, 0, 1)):
        out = None
        for i in order:
            s, e = pieces[i]
            out = rk.topk_scores(eq, ec[s:e].contiguous(), K, idx_base=s, out=out)
        _same(out, want, order)
    # an incoming list that is all empty: as without accumulate
    empty = (torch.full((Q, K), -1, dtype=torch.int32, device="cuda"), torch.full((Q, K), 0.75, dtype=torch.float32, device="cuda"))
    got = rk.topk_scores(eq, ec, K, out=empty)
    assert got[0] is empty[0] and got[1] is empty[1]
    _same(got, want)


# ---- 5. skip, NaN, range ------------------------------------------------------------------------------------------------
def test_topk_skip_nan_and_range():
    Q, C_, H, K = 17, 300, 300, 10
    rk = _ranker(H)
    eq, ec, _, _, prob = _inputs(Q, C_, H, True)
    base = select_topk(prob, None, K)
    # skip: each query leaves out its best column (queries 3 and 4: none, and a column that is not in the pool)
    skip = base[0][:, 0].copy()
    skip[3], skip[4] = -1, C_ + 5
    want = select_topk(prob, None, K, skip=skip)
    got = rk.topk_scores(eq, ec, K, skip=torch.from_numpy(skip).cuda())
    _same(got, want)
    gi = got[0].cpu().numpy()
    for q in range(Q):
        if q in (3, 4):
            assert np.array_equal(gi[q], base[0][q])
        else:
            assert skip[q] not in gi[q] and np.array_equal(gi[q][:K - 1], base[0][q][1:])     # exactly that column is gone
    # with idx_base the skipped column is the global one
    got = rk.topk_scores(eq, ec, K, skip=torch.from_numpy(skip + 1000).cuda(), idx_base=1000)
    _same(got, select_topk(prob, None, K, skip=skip + 1000, idx_base=1000))
    # a NaN row of emb_c is never returned.  (The pair sum's relu drops the NaN, so zt_affinity_rank writes a finite number
    # for that column; the selection's reference reads NaN there.)
    bad_col = int(base[0][0, 0])
    ec_nan = ec.clone()
    ec_nan[bad_col, 5] = float("nan")
    p_nan = rk.rank_scores(eq, ec_nan).cpu().numpy()
    keep = np.ones(C_, bool)
    keep[bad_col] = False
    assert np.array_equal(p_nan[:, keep].view(np.uint32), prob[:, keep].view(np.uint32))
    p_nan[:, bad_col] = np.nan
    got = rk.topk_scores(eq, ec_nan, K)
    _same(got, select_topk(p_nan, None, K))
    assert bad_col not in got[0].cpu().numpy()
    # an index == Nc: skipped, the status word set, IndexError under check_status, the next call clean
    eq, ec, ix, idx, prob = _inputs(Q, 65, H, False)
    Nc = ec.shape[0]
    q_hit = 2
    col = int(select_topk(prob, idx, K)[0][q_hit, 0])
    bad = idx.copy()
    bad[q_hit, col] = Nc
    gone = idx.copy()
    gone[q_hit, col] = -1
    got = rk.topk_scores(eq, ec, K, cand_idx=torch.from_numpy(bad).cuda(), check_status=False)
    _same(got, select_topk(prob, gone, K))
    with pytest.raises(IndexError):
        rk.topk_scores(eq, ec, K, cand_idx=torch.from_numpy(bad).cuda())
    _same(rk.topk_scores(eq, ec, K, cand_idx=ix), select_topk(prob, idx, K))


# ---- 6. float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "indexed"])
@pytest.mark.parametrize("Q,C_,K,H", [(17, 2500, 64, 300), (17, 65, 256, 1028), (5, 300, 10, 4), (17, 2500, 65, 300)])
def test_topk_against_a_float64_merge_layer(Q, C_, K, H, shared):
    """every returned probability within 1e-4 of the float64 MergeLayer for its pair; no present candidate left out whose float64
    probability is above the smallest selected one's by more than 2e-4 (each side's 1e-4, nothing else)"""
    eq, ec, ix, idx, _ = _inputs(Q, C_, H, shared)
    full_idx = np.tile(np.arange(C_, dtype=np.int32), (Q, 1)) if shared else idx
    ref = merge_f64(eq.cpu().numpy(), ec.cpu().numpy(), full_idx, _weights(H))
    gi, gp = [x.cpu().numpy() for x in _ranker(H).topk_scores(eq, ec, K, cand_idx=ix)]
    worst, over = 0.0, -np.inf
    for q in range(Q):
        sel = gi[q][gi[q] >= 0]
        present = np.nonzero(full_idx[q] >= 0)[0]
        assert len(sel) == min(K, len(present)) and len(set(sel.tolist())) == len(sel) and (full_idx[q][sel] >= 0).all()
        if len(sel) == 0:
            continue
        worst = max(worst, float(np.abs(gp[q][:len(sel)].astype(np.float64) - ref[q][sel]).max()))
        rest = np.setdiff1d(present, sel)
        if len(rest):
            over = max(over, float(ref[q][rest].max() - ref[q][sel].min()))
    print("Q=%d C=%d K=%d H=%d %s: max |prob - float64| = %.3g, best left out above the smallest selected by %.3g"
          % (Q, C_, K, H, "shared" if shared else "indexed", worst, over))
    assert worst <= TOL and over <= 2 * TOL


# ---- 7. TGN.recommend ---------------------------------------------------------------------------------------------------
def _model_state(tgn):
    m = tgn.memory
    st = {kk: getattr(m, kk).cpu().numpy().copy() for kk in ("memory", "last_update", "messages", "timestamps", "_flag_buf")}
    em = tgn.embedding_module
    if em.tppr_strategy == "streaming":
        for mi in range(em.n_tppr):
            for kk, v in em.tppr_finder.export_state(mi).items():
                st["tppr%d_%s" % (mi, kk)] = v
    st["batch_counter"] = np.int64(tgn.batch_counter)
    return st


@pytest.mark.parametrize("strategy", ["streaming", "pruning"])
def test_recommend_matches_rank_candidates(strategy):
    from zebra_amd.tppr import get_neighbor_finder
    D, F, T, k, al, be = 20, 7, 20, 5, [0.2, 0.1], [0.8, 0.5]
    N, E, bs, seed, K = 80, 250, 50, 61, 7
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    N = int(max(src.max(), dst.max())) + 1      # the node count of the model: the ids the pruning finder's data holds, and 0
    assert 64 < N <= 80 and neg.max() < N
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    nf = None
    if strategy == "pruning":
        nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat, strategy=strategy, nf=nf).eval()
    dev = torch.device("cuda")
    t = [torch.from_numpy(x).to(dev) for x in (src, dst, neg, ts, eidx)]
    for b in range(3):
        tgn.step_device(*[x[b * bs:(b + 1) * bs] for x in t], check_status=True)
    s = 3 * bs
    Q = 9
    sources, t0 = src[s:s + Q], float(ts[s])
    before = _model_state(tgn)
    # every node id 1 .. N - 1 in chunks smaller than the node count, the source's own id left out
    nodes, prob = tgn.recommend(sources, t0, K, pool_chunk=32)
    pool = np.arange(1, N, dtype=np.int32)
    full = tgn.rank_candidates(sources, np.full(Q, t0), pool).cpu().numpy()
    wi, wp = select_topk(full, None, K, skip=sources.astype(np.int64) - 1)
    _same((nodes, prob), (np.where(wi >= 0, wi + 1, -1).astype(np.int32), wp), "all nodes")
    for q in range(Q):
        assert int(sources[q]) not in nodes[q].cpu().numpy()
    same_t = tgn.recommend(sources, np.full(Q, t0), K, pool_chunk=1000)          # equal times as an array; one chunk
    assert torch.equal(same_t[0], nodes) and torch.equal(same_t[1], prob)
    with_self = tgn.recommend(sources, t0, K, exclude_self=False, pool_chunk=32)
    wi, wp = select_topk(full, None, K)
    _same(with_self, (wi + 1, wp), "exclude_self=False")
    # a shared 1-D pool with an absent entry, mapped back to node ids
    shared = np.array([5, 9, -1, 3, 40, 41, 17, 2, 60], np.int32)
    got = tgn.recommend(sources, t0, 4, candidates=shared, pool_chunk=4)
    ps = tgn.rank_candidates(sources, np.full(Q, t0), shared).cpu().numpy()
    wi, wp = select_topk(ps, np.tile(shared, (Q, 1)), 4)
    _same(got, (np.where(wi >= 0, shared[np.maximum(wi, 0)], -1).astype(np.int32), wp), "shared list")
    # [Q, C] with per-query times
    rng = np.random.RandomState(3)
    cands = rng.randint(1, N, (Q, 12)).astype(np.int32)
    cands[rng.random_sample(cands.shape) < 0.2] = -1
    tq = ts[s:s + Q]
    got = tgn.recommend(sources, tq, K, candidates=cands)
    pq = tgn.rank_candidates(sources, tq, cands).cpu().numpy()
    wi, wp = select_topk(pq, cands, K)
    _same(got, (np.where(wi >= 0, np.take_along_axis(cands, np.maximum(wi, 0), axis=1), -1).astype(np.int32), wp), "[Q, C]")
    after = _model_state(tgn)
    for kk in before:
        assert np.array_equal(before[kk], after[kk]), "recommend changed %s" % kk
    # unequal times with a shared pool; training messages pending; the pipeline enabled
    with pytest.raises(ValueError, match="time"):
        tgn.recommend(sources, tq, K)
    with pytest.raises(ValueError, match="time"):
        tgn.recommend(sources, tq, K, candidates=shared)
    tgn.test_mode = False
    with pytest.raises(RuntimeError):
        tgn.recommend(sources, t0, K)
    tgn.test_mode = True
    tgn.enable_pipeline(max_batch=64)
    try:
        with pytest.raises(RuntimeError, match="pipeline"):
            tgn.recommend(sources, t0, K)
        with pytest.raises(RuntimeError, match="pipeline"):
            tgn.recommend(sources, tq, K, candidates=cands)
    finally:
        tgn.enable_pipeline(False)


# ---- 8. fallback --------------------------------------------------------------------------------------------------------
def test_topk_scores_falls_back_to_torch_off_the_bound():
    """CPU tensors and k = 300 go through rank_scores and stable sorts: the same selection"""
    from zebra_amd.tgn import TGN
    rk = _ranker(20)
    eq, ec, ix, idx, _ = _inputs(17, 63, 20, False)
    cpu = types.SimpleNamespace(affinity_score=type(rk.affinity_score)(20, 20, 20, 1), device=torch.device("cpu"))
    cpu.affinity_score.load_state_dict(rk.affinity_score.state_dict())
    cpu.rank_scores = types.MethodType(TGN.rank_scores, cpu)
    p_cpu = cpu.rank_scores(eq.cpu(), ec.cpu(), ix.cpu()).numpy()
    skip = np.arange(17, dtype=np.int32) + 100
    got = TGN.topk_scores(cpu, eq.cpu(), ec.cpu(), 10, cand_idx=ix.cpu(), skip=torch.from_numpy(skip), idx_base=100)
    assert not got[0].is_cuda
    _same(got, select_topk(p_cpu, idx, 10, skip=skip, idx_base=100), "cpu")
    more = TGN.topk_scores(cpu, eq.cpu(), ec.cpu(), 10, cand_idx=ix.cpu(), idx_base=1000, out=got)     # the same pool again
    merged_p = np.concatenate([p_cpu, p_cpu], axis=1)
    merged_i = np.concatenate([idx, idx], axis=1)
    wi, wp = select_topk(merged_p, merged_i, 10, skip=np.arange(17))             # (the first copy's skipped columns)
    wi = np.where(wi >= 0, np.where(wi < 63, wi + 100, wi - 63 + 1000), -1).astype(np.int32)
    _same(more, (wi, wp), "cpu, accumulate")
    # k = 300 on the GPU: beyond the kernel's K, the same rule (C < k too)
    for shared in (True, False):
        eq, ec, ix, idx, prob = _inputs(17, 2500, 300, shared)
        _same(_ranker(300).topk_scores(eq, ec, 300, cand_idx=ix), select_topk(prob, idx, 300), "k=300")
    eq, ec, ix, idx, prob = _inputs(5, 64, 300, True)
    _same(_ranker(300).topk_scores(eq, ec, 300), select_topk(prob, None, 300), "k=300, C=64")
