"""Filtered top-K on the GPU, everything exact (integers and bit patterns): zt_csr_seen_ranges on a hand-made adjacency,
zt_exclude_mark against numpy in its three modes, zt_affinity_topk_masked (TGN.topk_scores(absent=...)) against the numpy
selection with the absent columns turned into -1 -- slabs, spans, accumulate, skip and NaN --, and TGN.recommend(exclude=...)
and evaluation.eval_edge_ranking(filtered=True) against restatements."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn
from helpers_filtered import add_rank_sums, adjacency, bits_to_mask, mark_bits, mask_to_bits, masked_idx, seen_ranges
from helpers_query import rank_of_positive
from helpers_topk import select_topk
from test_topk_gpu import _inputs, _model_state, _ranker, _same, _ws_bytes      # the shapes and references of the plain top-K

pytestmark = pytest.mark.gpu


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---- 1. seen ranges -----------------------------------------------------------------------------------------------------
def test_seen_ranges_on_a_hand_made_adjacency():
    from zebra_amd.tppr import NeighborFinder
    nbrs = [[3, 3, 1, 2], [], [0, 0, 0, 3, 3, 1], [2]]
    times = [[1.0, 2.0, 2.0, 7.5], [], [1.0, 3.0, 3.0, 3.0, 3.0, 9.0], [4.0]]
    nf = NeighborFinder([np.array(a, np.int32) for a in nbrs], [np.arange(len(a), dtype=np.int32) for a in nbrs],
                        [np.array(a, np.float64) for a in times])
    indptr = np.concatenate([[0], np.cumsum([len(a) for a in nbrs])])
    # (node, t, len): node 0; no entries; below all, above all; AT an entry inside a run of equal timestamps (the run is
    # excluded whole), just above it; the last node
    cases = [(0, 0.5, 0), (0, 1.0, 0), (0, 2.0, 1), (0, 2.5, 3), (0, 7.5, 3), (0, 100.0, 4), (1, 5.0, 0), (2, 0.0, 0),
             (2, 3.0, 1), (2, np.nextafter(3.0, 4.0), 5), (2, 9.0, 5), (2, 9.5, 6), (3, 4.0, 0), (3, 4.5, 1)]
    for v, t, want in cases:                                              # one query per case
        b, n = nf.seen_ranges_device(_cuda([v], np.int32), _cuda([t], np.float64))
        assert b.dtype == n.dtype == torch.int64 and b.is_cuda and n.is_cuda
        assert (int(b[0]), int(n[0])) == (int(indptr[v]), want), (v, t)
        assert len(nf.find_before(v, t)[0]) == want
    v, t, want = [np.array(x) for x in zip(*cases)]
    b, n = nf.seen_ranges_device(_cuda(v, np.int32), _cuda(t, np.float64))                # all at once
    assert np.array_equal(b.cpu().numpy(), indptr[v]) and np.array_equal(n.cpu().numpy(), want)
    b, n = nf.seen_ranges_device(_cuda([], np.int32), _cuda([], np.float64))
    assert b.shape == n.shape == (0,)
    # an id >= N (and a negative one): IndexError; without the check the other queries are still right; the next call is clean
    bad_v = np.array([0, 4, 2, -1, 3], np.int32)
    bad_t = np.array([2.5, 5.0, 9.5, 5.0, 4.5])
    with pytest.raises(IndexError):
        nf.seen_ranges_device(_cuda(bad_v), _cuda(bad_t))
    b, n = nf.seen_ranges_device(_cuda(bad_v), _cuda(bad_t), check_status=False)
    assert n.cpu().numpy().tolist() == [3, 0, 6, 0, 1] and b.cpu().numpy()[[0, 2, 4]].tolist() == indptr[[0, 2, 3]].tolist()
    with pytest.raises(IndexError):                                       # (the status latched by the unchecked call)
        nf.seen_ranges_device(_cuda([0], np.int32), _cuda([1.0]))
    nf.seen_ranges_device(_cuda([0], np.int32), _cuda([1.0]))


# ---- 2. the mark kernel -------------------------------------------------------------------------------------------------
LENS = (0, 1, 255, 256, 257, 5000)        # around one stride of the workgroup (256), and many strides
N_IDS = 3000
ID_LO = 7


@functools.lru_cache(maxsize=None)
def _lists():
    """a finder whose node v < 6 holds a list of LENS[v] ids in [0, N_IDS) with duplicates, in no order (the handle's own
    array), and the same lists with negative and far ids mixed in as a caller's array"""
    from zebra_amd.tppr import NeighborFinder
    rng = np.random.RandomState(21)
    lists = [rng.randint(0, N_IDS, n).astype(np.int32) for n in LENS] + [np.zeros(0, np.int32)] * (N_IDS - len(LENS))
    lists[2][:40] = lists[2][40:80]                                       # duplicates for certain
    nf = NeighborFinder(lists, [np.zeros(len(a), np.int32) for a in lists], [np.sort(rng.random_sample(len(a))) for a in lists])
    begin = np.concatenate([[0], np.cumsum(LENS)])[:-1].astype(np.int64)
    own = np.concatenate(lists[:len(LENS)])
    assert np.array_equal(nf._nbr, own)
    far = own.copy()
    far[::7] = np.array([-1, -5, 10 ** 6, 2 ** 31 - 1, ID_LO - 1, 0, N_IDS])[np.arange(len(far[::7])) % 7]
    return nf, own, far, begin, np.array(LENS, np.int64)


def _mark(handle, ids, begin, length, C_, W, id_lo=0, cand=None):
    """zt_exclude_mark into a buffer pre-filled with ones: uint32 [Q, W] on the host"""
    from zebra_amd._capi import check, lib, ptr, stream_ptr
    Q = len(begin)
    out = torch.full((max(Q, 1), W), -1, dtype=torch.int32, device="cuda")           # (Q = 0: still an address to hand over)
    srt = col = None
    stride = 0
    if cand is not None:
        srt, order = torch.sort(_cuda(cand, np.int32), dim=-1)
        srt, col = srt.contiguous(), order.to(torch.int32).contiguous()
        stride = C_ if np.ndim(cand) == 2 else 0
    b = _cuda(begin, np.int64) if Q else torch.zeros(1, dtype=torch.int64, device="cuda")
    n = _cuda(length, np.int64) if Q else torch.zeros(1, dtype=torch.int64, device="cuda")
    check(lib().zt_exclude_mark(handle, ptr(ids), ptr(b), ptr(n), C.c_int64(Q), C.c_int64(id_lo), ptr(srt), ptr(col),
                                C.c_int64(stride), C.c_int64(C_), ptr(out), C.c_int64(W), stream_ptr()), "zt_exclude_mark")
    return out[:Q].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("mode", ["range", "shared", "per_query"])
def test_exclude_mark_against_numpy(mode):
    nf, own, far, begin, lens = _lists()
    far_d = _cuda(far)
    rng = np.random.RandomState(5)
    hits = 0
    for C_ in (1, 31, 32, 33, 64, 65, 2500):
        for rows in ([], [5], [0, 1, 2, 3, 4], [5, 0, 3, 1, 4, 2]):                       # Q = 0, 1, 5, 6
            Q = len(rows)
            b, n = begin[rows], lens[rows]
            cand = None
            if mode != "range":                                           # repeated ids (all their columns set) and -1 entries
                cand = rng.randint(0, N_IDS, (Q, C_) if mode == "per_query" else C_).astype(np.int32)
                cand[..., ::5] = cand[..., :1]
                cand[rng.random_sample(cand.shape) < 0.1] = -1
            W = (C_ + 31) // 32 + 2                                       # spare words and trailing bits must read 0
            for handle, ids_d, ids in ((nf._h, None, own), (None, far_d, far), (nf._h, far_d, far)):
                got = _mark(handle, ids_d, b, n, C_, W, ID_LO, cand)
                want = mark_bits(ids, b, n, C_, W, ID_LO if cand is None else 0, cand)
                assert got.shape == want.shape and np.array_equal(got, want), (mode, C_, Q, ids is own)
                assert not got[:, (C_ + 31) // 32:].any() and not bits_to_mask(got, W * 32)[:, C_:].any()
                hits += int(want.any())
            # the exact width too
            got = _mark(nf._h, None, b, n, C_, (C_ + 31) // 32, ID_LO, cand)
            assert np.array_equal(got, mark_bits(own, b, n, C_, (C_ + 31) // 32, ID_LO if cand is None else 0, cand))
    assert hits > 30                                                       # (the draws do mark something)
    # ranges of the handle's array are clipped to it
    e2 = len(own)
    got = _mark(nf._h, None, np.array([e2 - 3, e2, -4]), np.array([10, 5, 2]), 2500, 79, ID_LO, None)
    assert np.array_equal(got, mark_bits(own, np.array([e2 - 3, 0, 0]), np.array([3, 0, 0]), 2500, 79, ID_LO))


def test_exclude_mark_over_more_than_one_tile_of_words():
    """C beyond 65 536 columns: two workgroups per query, each with its own part of the bits"""
    C_, Q = 65536 + 40, 2
    rng = np.random.RandomState(8)
    ids = rng.randint(0, 70000, 6000).astype(np.int32)
    ids[:4] = [0, 65535, 65536, C_ - 1]
    begin, length = np.array([0, 3000]), np.array([3000, 3000])
    W = (C_ + 31) // 32
    got = _mark(None, _cuda(ids), begin, length, C_, W, 0, None)
    want = np.zeros((Q, C_), bool)
    for q in range(Q):
        own = ids[begin[q]:begin[q] + length[q]]
        want[q, own[own < C_]] = True
    assert np.array_equal(bits_to_mask(got, C_), want) and not bits_to_mask(got, W * 32)[:, C_:].any()
    assert want[0, 65535] and want[0, 65536] and want[:, 65536:].sum() > 0
    cand = rng.permutation(C_).astype(np.int32)                            # a shared list: column c holds id cand[c]
    got = _mark(None, _cuda(ids), begin, length, C_, W, 0, cand)
    assert np.array_equal(bits_to_mask(got, C_), want[:, cand])


# ---- 3. the masked top-K ------------------------------------------------------------------------------------------------
def _absent(mask, W=None):
    return _cuda(mask_to_bits(mask, W).view(np.int32))


def _masks(Q, C_, seed):
    """mask densities 0, ~30 % and all ones"""
    rng = np.random.RandomState(seed)
    return [np.zeros((Q, C_), bool), rng.random_sample((Q, C_)) < 0.3, np.ones((Q, C_), bool)]


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "indexed"])
@pytest.mark.parametrize("Q,K", [(5, 10), (17, 64), (17, 65), (5, 256)])
def test_masked_topk_equals_the_selection_with_absent_columns(Q, K, shared):
    """C = 2500 from the smallest workspace -- slabs of 32 rows: all but the first have r0 != 0 -- and from the default one
    (several spans); Q is no multiple of 4: a tile has idle query slots"""
    from zebra_amd import _capi
    C_, H = 2500, 300
    eq, ec, ix, idx, prob = _inputs(Q, C_, H, shared)
    Nc = ec.shape[0]
    least = _ws_bytes(Q, 32, H, K)
    assert _capi.topk_plan(Q, Nc, C_, H, K, not shared, least)["n_slabs"] == (Nc + 31) // 32 > 1
    assert _capi.topk_plan(Q, Nc, C_, H, K, not shared, _ws_bytes(Q, Nc, H, K))["n_spans"] > 1
    rk = _ranker(H)
    plain = rk.topk_scores(eq, ec, K, cand_idx=ix)
    for d, mask in enumerate(_masks(Q, C_, 100 * Q + K)):
        want = select_topk(prob, masked_idx(idx, mask), K)
        for ws in (least, None):
            got = rk.topk_scores(eq, ec, K, cand_idx=ix, workspace_bytes=ws, absent=_absent(mask))
            _same(got, want, (Q, K, shared, d, ws))
        if d == 0:                                                        # no bit set: zt_affinity_topk's bits
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1].view(torch.int32), plain[1].view(torch.int32))
        if d == 1:
            assert not np.array_equal(want[0], plain[0].cpu().numpy())    # the mask took something out of the top K
            wide = rk.topk_scores(eq, ec, K, cand_idx=ix, absent=_absent(mask, 90))      # a row stride above ceil(C / 32)
            _same(wide, want, "W = 90")
        if d == 2:                                                        # a fully masked query: -1 and 0 in every slot
            assert (want[0] == -1).all() and not want[1].any()
    _same(rk.topk_scores(eq, ec, K, cand_idx=ix, absent=None), (plain[0].cpu().numpy(), plain[1].cpu().numpy()))


def test_masked_topk_at_small_sizes():
    """C below, at and just above a word; C < K; one query; the last words' unused bits"""
    H = 300
    rk = _ranker(H)
    for Q, C_, K in ((1, 1, 1), (5, 31, 64), (17, 33, 10), (5, 64, 65), (5, 65, 256)):
        for shared in (True, False):
            eq, ec, ix, idx, prob = _inputs(Q, C_, H, shared)
            for d, mask in enumerate(_masks(Q, C_, C_)):
                got = rk.topk_scores(eq, ec, K, cand_idx=ix, absent=_absent(mask))
                _same(got, select_topk(prob, masked_idx(idx, mask), K), (Q, C_, K, shared, d))


def test_masked_topk_with_skip_and_nan():
    Q, C_, H, K = 17, 300, 300, 10
    rk = _ranker(H)
    eq, ec, _, _, prob = _inputs(Q, C_, H, True)
    base = select_topk(prob, None, K)
    mask = np.random.RandomState(4).random_sample((Q, C_)) < 0.3
    skip = base[0][:, 0].copy()
    mask[:8, :][np.arange(8), skip[:8]] = True               # the bit set ON the skip column for half the queries, ...
    mask[8:, :][np.arange(Q - 8), skip[8:]] = False          # ... clear for the others: the column is gone either way
    got = rk.topk_scores(eq, ec, K, skip=_cuda(skip), absent=_absent(mask))
    _same(got, select_topk(prob, masked_idx(None, mask), K, skip=skip))
    assert all(skip[q] not in got[0][q].cpu().numpy() for q in range(Q))
    got = rk.topk_scores(eq, ec, K, skip=_cuda(skip + 1000), idx_base=1000, absent=_absent(mask))     # bits are LOCAL columns
    _same(got, select_topk(prob, masked_idx(None, mask), K, skip=skip + 1000, idx_base=1000))
    # a NaN candidate with its bit set for some queries and clear for others: never returned
    bad_col = int(base[0][0, 0])
    ec_nan = ec.clone()
    ec_nan[bad_col, 5] = float("nan")
    p_nan = prob.copy()
    p_nan[:, bad_col] = np.nan
    mask[::2, bad_col], mask[1::2, bad_col] = True, False
    got = rk.topk_scores(eq, ec_nan, K, absent=_absent(mask))
    _same(got, select_topk(p_nan, masked_idx(None, mask), K))
    assert bad_col not in got[0].cpu().numpy()


@pytest.mark.parametrize("K", [10, 100])
def test_masked_topk_accumulates_pieces_with_their_own_local_masks(K):
    """the pieces' seams at 100 and 450 cut words of the whole pool's mask: each piece brings bits of its OWN columns"""
    Q, H, N = 17, 300, 700
    eq, ec, _, _, prob = _inputs(Q, N, H, True)
    mask = np.random.RandomState(K).random_sample((Q, N)) < 0.3
    want = select_topk(prob, masked_idx(None, mask), K)
    rk = _ranker(H)
    _same(rk.topk_scores(eq, ec, K, absent=_absent(mask)), want, "one call")
    pieces = [(0, 100), (100, 450), (450, 700)]
    for order in ((0, 1, 2), (2, 0, 1)):
        out = None
        for i in order:
            s, e = pieces[i]
            out = rk.topk_scores(eq, ec[s:e].contiguous(), K, idx_base=s, out=out, absent=_absent(mask[:, s:e]))
        _same(out, want, order)


# ---- 4. TGN.recommend(exclude=...) and eval_edge_ranking(filtered=True) ---------------------------------------------------
def _stepped_model(strategy):
    """the set-up of test_recommend_matches_rank_candidates: three batches of 50 stepped; (tgn, finder over the whole stream,
    the stream, N)"""
    from zebra_amd.tppr import get_neighbor_finder
    D, F, T, k, al, be = 20, 7, 20, 5, [0.2, 0.1], [0.8, 0.5]
    N, E, bs, seed = 80, 250, 50, 61
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    N = int(max(src.max(), dst.max())) + 1
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat, strategy=strategy, nf=nf if strategy == "pruning" else None).eval()
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    for b in range(3):
        tgn.step_device(*[x[b * bs:(b + 1) * bs] for x in t], check_status=True)
    return tgn, nf, (src, dst, neg, ts, eidx), N


def _check_recommend(got, full, gone, K, skip, ids_of, what):
    """``got`` against the selection over ``full`` [Q, C] with the ``gone`` [Q, C] columns absent; ids_of maps columns to ids"""
    wi, wp = select_topk(full, masked_idx(None, gone), K, skip=skip)
    _same(got, (ids_of(wi), wp), what)


@pytest.mark.parametrize("strategy", ["streaming", "pruning"])
def test_recommend_leaves_out_seen_partners(strategy):
    tgn, nf, (src, dst, neg, ts, eidx), N = _stepped_model(strategy)
    s, Q = 150, 9
    sources, t0 = src[s:s + Q], float(ts[s])
    # the draw: what the adjacency holds before t0 for these sources
    indptr, nbr, ats = adjacency(src, dst, ts, N)
    assert np.array_equal(nf._indptr, indptr) and np.array_equal(nf._nbr, nbr) and np.array_equal(nf._ts, ats)
    assert len(ts) - len(np.unique(ts)) == 24                              # timestamp ties in the stream
    begin, length = seen_ranges(indptr, ats, sources, np.full(Q, t0))
    seen = [set(nbr[begin[q]:begin[q] + length[q]].tolist()) for q in range(Q)]
    assert [len(x) for x in seen] == [8, 0, 1, 23, 3, 1, 12, 16, 3] and sources[1] == 77        # a source with nothing to exclude
    assert length.tolist() == [9, 0, 1, 39, 3, 1, 15, 31, 3]               # lists with duplicates (a self-loop is two entries)
    assert sources[3] == 1 and 1 in seen[3]                                # a source whose list contains itself
    gb, gl = nf.seen_ranges_device(_cuda(sources, np.int32), _cuda(np.full(Q, t0)))
    assert np.array_equal(gb.cpu().numpy(), begin) and np.array_equal(gl.cpu().numpy(), length)

    before = _model_state(tgn)
    pool = np.arange(1, N, dtype=np.int32)
    full = tgn.rank_candidates(sources, np.full(Q, t0), pool).cpu().numpy()
    gone = np.array([[int(v) in seen[q] for v in pool] for q in range(Q)])
    skip = sources.astype(np.int64) - 1
    to_ids = lambda wi: np.where(wi >= 0, wi + 1, -1).astype(np.int32)
    exclude = "seen" if strategy == "pruning" else nf                      # (the streaming model holds no finder)
    if strategy == "streaming":
        with pytest.raises(ValueError, match="neighbor_finder"):
            tgn.recommend(sources, t0, 7, exclude="seen")
    # K = N - 1: every node that is not excluded comes back, in select_topk's order, with rank_candidates' bits
    nodes, prob = tgn.recommend(sources, t0, N - 1, exclude=exclude, pool_chunk=48)       # a chunk that is no multiple of 32
    _check_recommend((nodes, prob), full, gone, N - 1, skip, to_ids, "K = N - 1")
    for q in range(Q):
        back = nodes[q].cpu().numpy()
        assert set(back[back >= 0].tolist()) == set(range(1, N)) - {int(sources[q])} - seen[q], q
    for K, chunk in ((7, 48), (7, 65536), (7, 32)):
        _check_recommend(tgn.recommend(sources, t0, K, exclude=exclude, pool_chunk=chunk), full, gone, K, skip, to_ids, (K, chunk))
    _check_recommend(tgn.recommend(sources, t0, 7, exclude=exclude, exclude_self=False, pool_chunk=48), full, gone, 7, None, to_ids,
                     "exclude_self=False")
    # the caller's own lists, equal to the seen sets (in another order, with an id outside the pool): the same answer
    lists = [np.array(sorted(x, reverse=True) + [N + 50], np.int32) for x in seen]
    lptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    own = tgn.recommend(sources, t0, 7, exclude=(lptr, np.concatenate(lists)), pool_chunk=48)
    _check_recommend(own, full, gone, 7, skip, to_ids, "(ptr, ids)")
    bits = tgn.absent_bits(sources, t0, exclude, id_lo=1, n_cols=N - 1)
    assert bits.dtype == torch.int32 and bits.shape == (Q, (N - 1 + 31) // 32)
    assert np.array_equal(bits_to_mask(bits.cpu().numpy(), N - 1), gone)
    assert torch.equal(bits, tgn.absent_bits(sources, np.full(Q, t0), (lptr, np.concatenate(lists)), id_lo=1, n_cols=N - 1))
    # exclude=None is today's call
    a, b = tgn.recommend(sources, t0, 7, pool_chunk=48), tgn.recommend(sources, t0, 7, pool_chunk=48, exclude=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _check_recommend(a, full, np.zeros_like(gone), 7, skip, to_ids, "exclude=None")
    # a shared list holding a repeat and a -1
    shared = np.array([5, 9, -1, 3, 40, 41, 17, 2, 60, 9, 1, 4, 32, 53, 29], np.int32)
    ps = tgn.rank_candidates(sources, np.full(Q, t0), shared).cpu().numpy()
    gone_s = np.array([[int(v) in seen[q] for v in shared] for q in range(Q)]) | (shared < 0)[None, :]
    assert gone_s[:, shared >= 0].any() and gone_s[0, 1] == gone_s[0, 9]
    got = tgn.recommend(sources, t0, 6, candidates=shared, pool_chunk=4, exclude=exclude)
    _check_recommend(got, ps, gone_s, 6, None, lambda wi: np.where(wi >= 0, shared[np.maximum(wi, 0)], -1).astype(np.int32), "shared list")
    # [Q, C] candidates with per-query times: seen is taken at each query's own time
    rng = np.random.RandomState(3)
    cands = rng.randint(1, N, (Q, 40)).astype(np.int32)
    cands[rng.random_sample(cands.shape) < 0.2] = -1
    tq = ts[s:s + Q]
    bq, lq = seen_ranges(indptr, ats, sources, tq)
    assert lq.tolist() != length.tolist()
    seen_q = [set(nbr[bq[q]:bq[q] + lq[q]].tolist()) for q in range(Q)]
    gone_q = np.array([[int(v) in seen_q[q] for v in cands[q]] for q in range(Q)]) | (cands < 0)
    assert gone_q[cands >= 0].any()
    pq = tgn.rank_candidates(sources, tq, cands).cpu().numpy()
    got = tgn.recommend(sources, tq, 7, candidates=cands, exclude=exclude)
    _check_recommend(got, pq, gone_q, 7, None,
                     lambda wi: np.where(wi >= 0, np.take_along_axis(cands, np.maximum(wi, 0), axis=1), -1).astype(np.int32), "[Q, C]")
    # read-only
    after = _model_state(tgn)
    for kk in before:
        assert np.array_equal(before[kk], after[kk]), "recommend(exclude=...) changed %s" % kk
    # refusals: a source outside the finder; outside test mode; under the pipeline -- as recommend refuses
    with pytest.raises(ValueError):
        tgn.recommend(sources, t0, 7, exclude="partners")
    with pytest.raises(ValueError, match="ptr"):
        tgn.recommend(sources, t0, 7, exclude=(lptr[:-1], np.concatenate(lists)))
    with pytest.raises(ValueError, match="time"):
        tgn.recommend(sources, tq, 7, exclude=exclude)
    tgn.test_mode = False
    with pytest.raises(RuntimeError):
        tgn.recommend(sources, t0, 7, exclude=exclude)
    tgn.test_mode = True
    tgn.enable_pipeline(max_batch=64)
    try:
        with pytest.raises(RuntimeError, match="pipeline"):
            tgn.recommend(sources, t0, 7, exclude=exclude)
        with pytest.raises(RuntimeError, match="pipeline"):
            tgn.recommend(sources, tq, 7, candidates=cands, exclude=exclude)
    finally:
        tgn.enable_pipeline(False)


class _Sampler:
    def __init__(self, dst_list, seed):
        self.dst_list, self.seed = np.unique(dst_list), seed
        self.random_state = np.random.RandomState(seed)

    def reset_random_state(self):
        self.random_state = np.random.RandomState(self.seed)

    def sample(self, size):
        i = self.random_state.randint(0, len(self.dst_list), size)
        return self.dst_list[i], self.dst_list[self.random_state.randint(0, len(self.dst_list), size)]


def test_filtered_edge_ranking_matches_a_restatement():
    from zebra_amd import evaluation as ev
    from zebra_amd.tppr import get_neighbor_finder
    N, E, D, F, T, k, al, be, seed, bs, n_neg = 80, 250, 20, 7, 20, 5, [0.2, 0.1], [0.8, 0.5], 61, 50, 20
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    N = int(max(src.max(), dst.max())) + 1
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    data = types.SimpleNamespace(sources=src, destinations=dst, timestamps=ts, edge_idxs=eidx, n_interactions=E)
    nf = get_neighbor_finder(data)
    got = ev.eval_edge_ranking(build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat), _Sampler(dst, 9), data, 10, batch_size=bs,
                               n_negatives=n_neg, filtered=True, finder=nf)
    plain = ev.eval_edge_ranking(build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat), _Sampler(dst, 9), data, 10, batch_size=bs,
                                 n_negatives=n_neg, filtered=False, finder=nf)       # today's numbers: the restatement below
    with pytest.raises(ValueError, match="finder"):                        # (the streaming model holds no finder)
        ev.eval_edge_ranking(build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat), _Sampler(dst, 9), data, 10, filtered=True)
    # the restatement: rank_candidates' probabilities, numpy masks from the numpy adjacency, helpers_query's rank, the kernel's
    # additions in its order; the state advances by plain eval steps over the first-column negatives
    indptr, nbr, ats = adjacency(src, dst, ts, N)
    model = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()
    smp = _Sampler(dst, 9)
    smp.reset_random_state()
    model.update_memory_in_test(model.memory)
    model.test_mode = True
    sums = {True: np.zeros(5), False: np.zeros(5)}
    masked = 0
    for s in range(0, E, bs):
        e = s + bs
        negs = smp.sample(bs * n_neg)[1].reshape(bs, n_neg)
        cands = np.concatenate([dst[s:e, None], negs], axis=1)
        prob = model.rank_candidates(src[s:e], ts[s:e], cands).cpu().numpy()
        begin, length = seen_ranges(indptr, ats, src[s:e], ts[s:e])
        gone = np.zeros(cands.shape, bool)
        for q in range(bs):
            seen = set(nbr[begin[q]:begin[q] + length[q]].tolist()) | {int(dst[s + q])}
            gone[q, 1:] = [int(v) in seen for v in cands[q, 1:]]           # column 0, the positive, is never masked
        masked += int(gone.sum())
        sums[True] = add_rank_sums(sums[True], rank_of_positive(prob, masked_idx(None, gone)))
        sums[False] = add_rank_sums(sums[False], rank_of_positive(prob))
        model.compute_temporal_embeddings(src[s:e], dst[s:e], negs[:, 0], ts[s:e], eidx[s:e], 10, False)
    assert masked > 0                                                      # the filter did something
    for res, a in ((got, sums[True]), (plain, sums[False])):
        assert a[4] == E
        assert res == dict(mrr=float(a[0] / E), hits1=float(a[1] / E), hits3=float(a[2] / E), hits10=float(a[3] / E))
    print("filtered:", got, "unfiltered:", plain, "negatives masked:", masked)
    assert got != plain and got["mrr"] >= plain["mrr"]                     # a rank can only improve when negatives leave
