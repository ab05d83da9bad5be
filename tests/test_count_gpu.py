"""The full-pool rank on the GPU: TGN.count_scores (csrc/rank_count.hip) against the counts taken from rank_scores' own
prob [Q, C] -- integer equality, the bits are shared --, its torch fallback, zt_rank_metrics_counts against zt_rank_metrics,
TGN.rank_of on a stepped model against rank_candidates + rank_metrics, and eval_edge_ranking_full against a loop written here."""
import functools
import types

import numpy as np
import pytest
import torch

import helpers_count_planted as K
import helpers_topk_planted as P
import inputs as I
from helpers import build_tgn
from helpers_filtered import adjacency, seen_ranges

pytestmark = pytest.mark.gpu


def _holder(H, weights, device):
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN
    m = MergeLayer(H, H, H, 1)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), weights):
            p.copy_(torch.from_numpy(w))
    holder = types.SimpleNamespace(affinity_score=m.to(device), device=torch.device(device))
    for name in ("rank_scores", "count_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    return holder


@functools.lru_cache(maxsize=None)
def _random_ranker(H):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    rng = np.random.RandomState(700 + H)
    w = ((rng.standard_normal((H, 2 * H)) / np.sqrt(2 * H)).astype(np.float32), (rng.standard_normal(H) * 0.1).astype(np.float32),
         (rng.standard_normal((1, H)) / np.sqrt(H)).astype(np.float32), (rng.standard_normal(1) * 0.1).astype(np.float32))
    return _holder(H, w, "cuda")


# ---- 1. random weights and embeddings: the counts of rank_scores' own probabilities ---------------------------------------
@pytest.mark.parametrize("H", [20, 200, 344])
def test_count_equals_the_counts_over_the_rank_scorer(H):
    Q, C_ = 7, 1000
    rk = _random_ranker(H)
    rng = np.random.RandomState(H)
    eq = torch.from_numpy((rng.standard_normal((Q, H)) * 0.7).astype(np.float32)).cuda()
    emb_c = (rng.standard_normal((C_, H)) * 0.7).astype(np.float32)
    emb_c[500:520] = emb_c[3]                                  # ties: twenty copies of the row query 3's threshold comes from
    emb_c[77, 5] = np.nan                                      # a NaN candidate
    ec = torch.from_numpy(emb_c).cuda()
    prob = rk.rank_scores(eq, ec).cpu().numpy()
    thr_h = prob[np.arange(Q), np.arange(Q)].copy()            # query q's threshold: its probability at column q
    thr_h[5] = np.nan
    thr = torch.from_numpy(thr_h).cuda()
    nan_col = np.isnan(emb_c).any(axis=1)
    mask = rng.random_sample((Q, C_)) < 0.3
    mask[2] = True
    skip = np.stack([np.arange(Q), rng.randint(0, C_, Q), np.full(Q, -1)], axis=1).astype(np.int32)
    col = np.arange(C_)

    def want(live):
        with np.errstate(invalid="ignore"):
            return (live & (prob > thr_h[:, None])).sum(axis=1), (live & (prob == thr_h[:, None])).sum(axis=1)

    base = np.broadcast_to(~nan_col, (Q, C_)) & ~np.isnan(prob)
    skipped = np.zeros((Q, C_), bool)
    for j in range(skip.shape[1]):
        skipped |= col[None, :] == skip[:, j:j + 1]
    bits = torch.from_numpy(K.pack_bits(mask).view(np.int32)).cuda()
    for name, live, kw in (("plain", base, {}), ("bits", base & ~mask, dict(absent=bits)),
                           ("skip", base & ~skipped, dict(skip=torch.from_numpy(skip).cuda())),
                           ("skip1", base & (col[None, :] != skip[:, :1]), dict(skip=torch.from_numpy(skip[:, 0].copy()).cuda())),
                           ("both", base & ~mask & ~skipped, dict(absent=bits, skip=torch.from_numpy(skip).cuda()))):
        a, e = rk.count_scores(eq, ec, thr, **kw)
        wa, we = want(live)
        assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(e.cpu().numpy(), we), (H, name)
    wa, we = want(base)
    assert we[3] >= 21 and we[0] >= 1 and wa[5] == we[5] == 0 and wa.max() > 100


# ---- 2. the torch fallback ------------------------------------------------------------------------------------------------
def test_fallback_equals_the_hip_path():
    """the dialled scorer: a pair scores exactly its level in any summation order, and the threshold 0.5f is the sigmoid of
    score 0 on every path -- levels 0 are the equal columns, rising levels above, falling ones below"""
    Q, C_ = 6, 333
    case = K.CountCase("fallback", Q, C_, lambda: dict(
        u=np.stack([P.lev(np.random.RandomState(q).randint(0, 4, C_)) for q in range(Q)]), falling=(1, 4),
        thr=[("const", "half")] * Q, nan_cols=(9, 40),
        mask=np.random.RandomState(3).random_sample((Q, C_)) < 0.25,
        skip=np.stack([np.arange(Q) * 7, np.full(Q, -1)], axis=1)))
    d = case.data()
    wa, we = K.expected(case, d)
    assert (we > 30).all() and wa[0] > 100 and wa[1] == 0
    thr = torch.full((Q,), 0.5)
    bits = torch.from_numpy(K.pack_bits(d["mask"]).view(np.int32))
    skip = torch.from_numpy(d["skip"])
    eq, ec = torch.from_numpy(d["emb_q"]), torch.from_numpy(d["emb_c"])
    hip = _holder(20, P.scorer_weights(20), "cuda").count_scores(eq.cuda(), ec.cuda(), thr.cuda(), skip=skip.cuda(), absent=bits.cuda())
    cpu = _holder(20, P.scorer_weights(20), "cpu").count_scores(eq, ec, thr, skip=skip, absent=bits)
    assert not cpu[0].is_cuda and cpu[0].dtype == torch.int32
    for got in (hip, cpu):
        assert np.array_equal(got[0].cpu().numpy(), wa) and np.array_equal(got[1].cpu().numpy(), we)
    # a width the kernels do not take: H = 22 (H % 4 != 0), CUDA tensors, the same pool on the first 20 coordinates
    pad = lambda x: np.concatenate([x, np.full((x.shape[0], 2), x.min() if x.min() < 0 else 0.0, np.float32)], axis=1)
    w22 = P.scorer_weights(22)
    got = _holder(22, w22, "cuda").count_scores(torch.from_numpy(pad(d["emb_q"])).cuda(), torch.from_numpy(pad(d["emb_c"])).cuda(),
                                                thr.cuda(), skip=skip.cuda(), absent=bits.cuda())
    assert np.array_equal(got[0].cpu().numpy(), wa) and np.array_equal(got[1].cpu().numpy(), we)
    # accumulate in the fallback
    out = (torch.full((Q,), 5, dtype=torch.int32), torch.full((Q,), 9, dtype=torch.int32))
    _holder(20, P.scorer_weights(20), "cpu").count_scores(eq, ec, thr, skip=skip, absent=bits, out=out)
    assert np.array_equal(out[0].numpy(), wa + 5) and np.array_equal(out[1].numpy(), we + 9)


# ---- 3. zt_rank_metrics_counts --------------------------------------------------------------------------------------------
def test_rank_metrics_counts_has_rank_metrics_bits():
    from zebra_amd import evaluation as ev
    rng = np.random.RandomState(11)
    Q, C_ = 1500, 40                                            # more than one chunk of 1024 queries
    prob = (rng.randint(0, 12, (Q, C_)) / 16.0).astype(np.float32)          # ties
    idx = np.where(rng.random_sample((Q, C_)) < 0.2, -1, 0).astype(np.int32)
    idx[:, 0] = 0
    idx[::50, 0] = -1                                           # absent positives: skipped queries
    prob[1, 1:] = 0.0
    prob[1, 0] = 0.5                                            # a rank of exactly 1
    live = idx[:, 1:] >= 0
    above = (live & (prob[:, 1:] > prob[:, :1])).sum(axis=1).astype(np.int32)
    equal = (live & (prob[:, 1:] == prob[:, :1])).sum(axis=1).astype(np.int32)
    thr = np.where(idx[:, 0] >= 0, prob[:, 0], np.float32(np.nan)).astype(np.float32)
    pd, ixd = torch.from_numpy(prob).cuda(), torch.from_numpy(idx).cuda()
    td, ad, ed = torch.from_numpy(thr).cuda(), torch.from_numpy(above).cuda(), torch.from_numpy(equal).cuda()
    want_acc, want_rank = ev.rank_metrics(pd, ixd, ranks=True)
    got_acc, got_rank = ev.rank_metrics_counts(td, ad, ed, ranks=True)
    assert got_rank.dtype == torch.float64 and got_acc.dtype == torch.float64
    assert torch.equal(got_rank, want_rank.double()) and (got_rank == 0).sum() == 30 and got_rank[1] == 1.0
    assert torch.equal(got_acc.view(torch.int64), want_acc.view(torch.int64)), (got_acc, want_acc)
    # acc accumulates over two calls: the halves, in order, onto the first half's sums
    h = 700
    acc = ev.rank_metrics_counts(td[:h], ad[:h], ed[:h])
    back = ev.rank_metrics_counts(td[h:], ad[h:], ed[h:], out=acc)
    ref = ev.rank_metrics(pd[h:], ixd[h:], out=ev.rank_metrics(pd[:h], ixd[:h]))
    assert back is acc and torch.equal(acc.view(torch.int64), ref.view(torch.int64)) and acc[4] == Q - 30
    # ranks beyond float32: exact in the float64 output
    big_a = torch.tensor([2 ** 24 + 1, 2 ** 31 - 1, 0, 9], dtype=torch.int32, device="cuda")
    big_e = torch.tensor([1, 2 ** 31 - 1, 0, 0], dtype=torch.int32, device="cuda")
    t4 = torch.tensor([0.5, 0.25, 1.0, float("nan")], dtype=torch.float32, device="cuda")
    acc4, r4 = ev.rank_metrics_counts(t4, big_a, big_e, ranks=True)
    ranks = [1.0 + (2 ** 24 + 1) + 0.5, 1.0 + (2 ** 31 - 1) + 0.5 * (2 ** 31 - 1), 1.0, 0.0]
    assert r4.cpu().tolist() == ranks and float(np.float32(ranks[0])) != ranks[0]
    s = 0.0
    for r in ranks[:3]:
        s += 1.0 / r
    assert acc4.cpu().tolist() == [s, 1.0, 1.0, 1.0, 3.0]
    with pytest.raises(ValueError):
        ev.rank_metrics_counts(t4.double(), big_a, big_e)
    with pytest.raises(ValueError):
        ev.rank_metrics_counts(t4, big_a[:3], big_e)


# ---- 4. TGN.rank_of on a stepped model ------------------------------------------------------------------------------------
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


MODEL = dict(D=20, F=7, T=20, k=5, al=[0.2, 0.1], be=[0.8, 0.5], N=80, E=250, bs=50, seed=61)


def _stream():
    from zebra_amd.tppr import get_neighbor_finder
    c = MODEL
    src, dst, neg, ts, eidx = I.make_stream("general", c["N"], c["E"], c["seed"])
    N = int(max(src.max(), dst.max())) + 1
    w = I.model_weights(c["D"], c["F"], c["T"], len(c["al"]), c["seed"])
    _, efeat = I.random_tables(N, c["E"] + 1, c["D"], c["F"], c["seed"])
    nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    return (src, dst, neg, ts, eidx), N, w, efeat, nf


def _build(N, w, efeat, strategy="streaming", nf=None):
    c = MODEL
    return build_tgn(N, c["E"] + 1, c["D"], c["F"], c["T"], c["k"], c["al"], c["be"], w, efeat, strategy=strategy, nf=nf).eval()


def _reference(tgn, sources, times, targets, table):
    """(rank float64 [Q], prob float32 [Q]) of column 0 of [target | table] (-1: absent): rank_candidates + rank_metrics"""
    from zebra_amd import evaluation as ev
    full = np.concatenate([np.asarray(targets, np.int32)[:, None], table], axis=1).astype(np.int32)
    p = tgn.rank_candidates(sources, times, full)
    _, rank = ev.rank_metrics(p, torch.from_numpy(full).cuda(), ranks=True)
    return rank.double().cpu().numpy(), p[:, 0].cpu().numpy()


def _same_rank(got, want, what):
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.float32
    assert np.array_equal(got[0].cpu().numpy(), want[0]), "ranks differ: %s\n%s\n%s" % (what, got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32)), "probabilities differ: %s" % (what,)


@pytest.mark.parametrize("strategy", ["streaming", "pruning"])
def test_rank_of_matches_rank_candidates(strategy):
    (src, dst, neg, ts, eidx), N, w, efeat, nf = _stream()
    tgn = _build(N, w, efeat, strategy, nf if strategy == "pruning" else None)
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    bs = MODEL["bs"]
    for b in range(3):
        tgn.step_device(*[x[b * bs:(b + 1) * bs] for x in t], check_status=True)
    s, Q = 150, 9
    sources, targets, t0, tq = src[s:s + Q], dst[s:s + Q].copy(), float(ts[s]), ts[s:s + Q]
    targets[2] = -1                                                        # a query without a target: rank 0
    times = np.full(Q, t0)
    indptr, nbr, ats = adjacency(src, dst, ts, N)

    def seen_at(tt):
        b, l = seen_ranges(indptr, ats, sources, tt)
        return [set(nbr[b[q]:b[q] + l[q]].tolist()) for q in range(Q)]

    tx = tq.copy()
    tx[::2] = ts[40]                                                       # exclusion times apart from the query time
    seen0, seenq, seenx = seen_at(times), seen_at(tq), seen_at(tx)
    assert seen0 != seenx and sum(len(x) for x in seen0) > 20 and sum(len(x) for x in seenx) > 10
    pool = np.arange(1, N, dtype=np.int32)

    def table_of(cands2d, seen=None, no_self=False):
        """cands2d [Q, C] with -1 at the target's columns, the excluded ids and (no_self) the source"""
        tb = np.array(cands2d, np.int32)
        for q in range(Q):
            gone = tb[q] == targets[q]
            if no_self:
                gone |= tb[q] == sources[q]
            if seen is not None:
                gone |= np.isin(tb[q], list(seen[q]))
            tb[q, gone] = -1
        return tb

    before = _model_state(tgn)
    pool2d = np.broadcast_to(pool, (Q, N - 1))
    exclude = "seen" if strategy == "pruning" else nf                      # (the streaming model holds no finder)
    # the default pool, at one query time
    want = _reference(tgn, sources, times, targets, table_of(pool2d, no_self=True))
    assert want[0][2] == 0 and (want[0][[0, 1, 3, 4]] >= 1).all() and want[0].max() > 3
    _same_rank(tgn.rank_of(sources, t0, targets), want, "default")
    _same_rank(tgn.rank_of(sources, times, targets, pool_chunk=48), want, "chunks of 48, times [Q]")
    _same_rank(tgn.rank_of(sources, t0, targets, exclude_self=False), _reference(tgn, sources, times, targets, table_of(pool2d)),
               "exclude_self=False")
    want_seen = _reference(tgn, sources, times, targets, table_of(pool2d, seen0, True))
    assert not np.array_equal(want_seen[0], want[0])
    _same_rank(tgn.rank_of(sources, t0, targets, exclude=exclude, pool_chunk=48), want_seen, "seen at t0")
    lists = [np.array(sorted(x, reverse=True) + [N + 50], np.int32) for x in seen0]
    lptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    _same_rank(tgn.rank_of(sources, t0, targets, exclude=(lptr, np.concatenate(lists))), want_seen, "(ptr, ids)")
    want_q = _reference(tgn, sources, times, targets, table_of(pool2d, seenx, True))
    assert not np.array_equal(want_q[0], want_seen[0])
    _same_rank(tgn.rank_of(sources, t0, targets, exclude=exclude, exclude_timestamps=tx, pool_chunk=32), want_q,
               "seen at times of their own")
    if strategy == "streaming":
        with pytest.raises(ValueError, match="neighbor_finder"):
            tgn.rank_of(sources, t0, targets, exclude="seen")
    # counts: identical whatever the chunk
    runs = [tgn.rank_of(sources, t0, targets, exclude=exclude, exclude_timestamps=tx, pool_chunk=c, counts=True) for c in (32, 48, 65536)]
    for r in runs:
        assert r[0].dtype == torch.int32 and r[1].dtype == torch.int32
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2])
    a, e = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert np.array_equal(np.where(targets >= 0, 1 + a + 0.5 * e, 0), want_q[0]) and a[2] == e[2] == 0
    # a 1-D list with duplicates of targets and -1 entries
    shared = np.array([5, 9, -1, 3, int(targets[0]), 41, 17, int(targets[0]), 60, 9, 1, int(targets[4]), -1, 53, 29, 33, 70, 12], np.int32)
    sh2d = np.broadcast_to(shared, (Q, len(shared)))
    _same_rank(tgn.rank_of(sources, t0, targets, candidates=shared, pool_chunk=4), _reference(tgn, sources, times, targets, table_of(sh2d)),
               "shared list")
    _same_rank(tgn.rank_of(sources, t0, targets, candidates=shared, pool_chunk=5, exclude=exclude),
               _reference(tgn, sources, times, targets, table_of(sh2d, seen0)), "shared list, seen")
    # [Q, C] candidates with per-query times
    rng = np.random.RandomState(3)
    cands = rng.randint(1, N, (Q, 40)).astype(np.int32)
    cands[rng.random_sample(cands.shape) < 0.2] = -1
    cands[0, 7] = targets[0]
    want_2d = _reference(tgn, sources, tq, targets, table_of(cands, seenq))
    _same_rank(tgn.rank_of(sources, tq, targets, candidates=cands, exclude=exclude), want_2d, "[Q, C]")
    a2, e2, p2 = tgn.rank_of(sources, tq, targets, candidates=cands, exclude=exclude, counts=True)
    assert np.array_equal(np.where(targets >= 0, 1 + a2.cpu().numpy() + 0.5 * e2.cpu().numpy(), 0), want_2d[0])
    # read-only
    after = _model_state(tgn)
    for kk in before:
        assert np.array_equal(before[kk], after[kk]), "rank_of changed %s" % kk
    # refusals: recommend's
    with pytest.raises(ValueError, match="time"):
        tgn.rank_of(sources, tq, targets)
    with pytest.raises(ValueError):
        tgn.rank_of(sources, t0, targets[:-1])
    tgn.test_mode = False
    with pytest.raises(RuntimeError):
        tgn.rank_of(sources, t0, targets)
    tgn.test_mode = True


# ---- 5. eval_edge_ranking_full --------------------------------------------------------------------------------------------
def test_full_edge_ranking_matches_a_restatement():
    from zebra_amd import evaluation as ev
    (src, dst, neg, ts, eidx), N, w, efeat, nf = _stream()
    E, bs = 150, MODEL["bs"]
    data = types.SimpleNamespace(sources=src[:E], destinations=dst[:E], timestamps=ts[:E], edge_idxs=eidx[:E], n_interactions=E)
    m_plain, m_filt = _build(N, w, efeat), _build(N, w, efeat)
    plain = ev.eval_edge_ranking_full(m_plain, data, 10, batch_size=bs, pool_chunk=48)
    filt = ev.eval_edge_ranking_full(m_filt, data, 10, batch_size=bs, filtered=True, finder=nf)
    with pytest.raises(ValueError, match="finder"):                        # (the streaming model holds no finder)
        ev.eval_edge_ranking_full(_build(N, w, efeat), data, 10, filtered=True)
    # the restatement: per batch everyone at t0, rank_candidates over [destination | every other id], rank_metrics, the eval step
    indptr, nbr, ats = adjacency(src, dst, ts, N)
    model = _build(N, w, efeat)
    model.update_memory_in_test(model.memory)
    model.test_mode = True
    acc = {True: torch.zeros(5, dtype=torch.float64, device="cuda"), False: torch.zeros(5, dtype=torch.float64, device="cuda")}
    pool = np.arange(1, N, dtype=np.int32)
    masked = 0
    for s in range(0, E, bs):
        e = s + bs
        begin, length = seen_ranges(indptr, ats, src[s:e], ts[s:e])
        for filtered in (False, True):
            table = np.broadcast_to(pool, (bs, N - 1)).copy()
            for q in range(bs):
                gone = (table[q] == dst[s + q]) | (table[q] == src[s + q])
                if filtered:
                    seen = np.isin(table[q], nbr[begin[q]:begin[q] + length[q]])
                    masked += int((seen & ~gone).sum())
                    gone |= seen
                table[q, gone] = -1
            full = np.concatenate([dst[s:e, None], table], axis=1).astype(np.int32)
            prob = model.rank_candidates(src[s:e], np.full(bs, ts[s]), full)
            ev.rank_metrics(prob, torch.from_numpy(full).cuda(), out=acc[filtered])
        model.compute_temporal_embeddings(src[s:e], dst[s:e], dst[s:e], ts[s:e], eidx[s:e], 10, False)
    assert masked > 0
    for res, a in ((plain, acc[False].cpu().numpy()), (filt, acc[True].cpu().numpy())):
        assert a[4] == E
        assert res == dict(mrr=float(a[0] / E), hits1=float(a[1] / E), hits3=float(a[2] / E), hits10=float(a[3] / E))
    print("full-pool unfiltered:", plain, "filtered:", filt, "candidates masked:", masked)
    assert filt != plain and filt["mrr"] >= plain["mrr"]
    # the state afterwards: the same batches stepped directly
    direct = _build(N, w, efeat)
    for s in range(0, E, bs):
        e = s + bs
        direct.compute_temporal_embeddings(src[s:e], dst[s:e], dst[s:e], ts[s:e], eidx[s:e], 10, False)
    want = _model_state(direct)
    for m in (m_plain, m_filt, model):
        got = _model_state(m)
        assert set(got) == set(want)
        for kk in want:
            assert np.array_equal(got[kk], want[kk]), "the state after the pass differs in %s" % kk
