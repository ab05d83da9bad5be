"""The negative sampler on the GPU, everything exact (integers): zt_neg_sample against the numpy restatement of its rule
(tests/helpers_negsample.py) on every case of the table -- each K at which the plan turns, the list lengths around the
workgroup's strides, the flags, pools that run dry, the caller's lists, clipped ranges --, every element written, the same bits
twice, split invariance; then zebra_amd.sampling.NegativeSampler against the same restatement, eval_edge_ranking with it
against a replay of the restatement's rows and against a numpy restatement of the ranks, and TGN.compute_rank_loss with a
device tensor against its numpy copy."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn
from helpers_filtered import add_rank_sums, adjacency, masked_idx, seen_ranges
from helpers_negsample import CASES, DISTINCT, EXCLUDE_SOURCE, FILTER, case_expected, case_inputs, sample_rows, world
from helpers_query import rank_of_positive

pytestmark = pytest.mark.gpu

SENTINEL = 0x7f7f7f7f


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _finder():
    """the world's adjacency as a NeighborFinder: the handle's neighbour array is helpers_filtered.adjacency's"""
    from zebra_amd.tppr import get_neighbor_finder
    w = world()
    nf = get_neighbor_finder(types.SimpleNamespace(sources=w.src, destinations=w.dst, edge_idxs=w.eidx, timestamps=w.ts))
    assert np.array_equal(nf._nbr, w.nbr) and np.array_equal(nf._indptr, w.indptr[:nf.num_nodes + 1]) and np.array_equal(nf._ts, w.ats)
    return nf


def _sample(a, lo=0, hi=None, row_base=None, with_count=True):
    """zt_neg_sample over rows lo .. hi of a case's inputs into buffers pre-filled with a sentinel: (neg, count) on the host"""
    from zebra_amd import _capi
    hi = a.rows if hi is None else hi
    Q = hi - lo
    d = _capi.NegDesc(seed=a.seed & (2 ** 64 - 1), row_base=a.row_base + lo if row_base is None else row_base, K=a.K,
                      K_hist=a.K_hist, rounds=a.rounds, hist_rounds=a.hist_rounds, flags=a.flags)
    neg = torch.full((Q, a.K), SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.full((Q, 2), SENTINEL, dtype=torch.int32, device="cuda")
    handle = ids = begin = length = None
    if a.ids is not None:
        begin, length = _cuda(a.begin[lo:hi], np.int64), _cuda(a.length[lo:hi], np.int64)
        if a.n_ids is None:
            ids = _cuda(a.ids, np.int32)
        else:
            handle = _finder()._h
    src, dst, pool = _cuda(a.src[lo:hi], np.int32), _cuda(a.dst[lo:hi], np.int32), _cuda(a.pool, np.int32)      # (kept alive by name)
    _capi.check(_capi.lib().zt_neg_sample(C.byref(d), _capi.ptr(src), _capi.ptr(dst),
                                          C.c_int64(Q), _capi.ptr(pool), C.c_int64(len(a.pool)), handle,
                                          _capi.ptr(ids), _capi.ptr(begin), _capi.ptr(length), _capi.ptr(neg),
                                          _capi.ptr(count) if with_count else None, _capi.stream_ptr()), "zt_neg_sample")
    torch.cuda.synchronize()
    return neg.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_restatement(name):
    a = case_inputs(name)
    want_neg, want_count, _ = case_expected(name)
    neg, count = _sample(a)
    assert not (neg == SENTINEL).any() and not (count == SENTINEL).any()          # every element is written
    bad = np.argwhere(neg != want_neg)
    assert bad.size == 0, "%s: %d slots differ, first (row, slot) %s: %d against %d" % (
        name, len(bad), bad[0], neg[tuple(bad[0])], want_neg[tuple(bad[0])])
    assert np.array_equal(count, want_count)
    again, count2 = _sample(a)                                                    # two runs give the same bits
    assert np.array_equal(again, neg) and np.array_equal(count2, count)
    alone, untouched = _sample(a, with_count=False)                               # count_dev may be NULL
    assert np.array_equal(alone, neg) and (untouched == SENTINEL).all()


@pytest.mark.parametrize("name", ["K65", "K257", "dry-pool40-K32-mixed", "own-lists-negative", "big-row-base"])
def test_split_invariance_through_the_abi(name):
    """Q = 10 at row_base = 100 equals rows 100 .. 103 followed by rows 104 .. 109; one row alone equals its row of the batch"""
    a = case_inputs(name)
    base = a.row_base + 100
    whole = _sample(a, 0, 10, row_base=base)
    head, tail = _sample(a, 0, 4, row_base=base), _sample(a, 4, 10, row_base=base + 4)
    assert np.array_equal(whole[0], np.concatenate([head[0], tail[0]])) and np.array_equal(whole[1], np.concatenate([head[1], tail[1]]))
    one = _sample(a, 7, 8, row_base=base + 7)
    assert np.array_equal(one[0], whole[0][7:8]) and np.array_equal(one[1], whole[1][7:8])
    lists = {} if a.ids is None else dict(ids=a.ids, begin=a.begin[:10], length=a.length[:10], n_ids=a.n_ids)
    want = sample_rows(a.seed, base, a.K, a.K_hist, a.rounds, a.hist_rounds, a.flags, a.src[:10], a.dst[:10], a.pool, **lists)
    assert np.array_equal(whole[0], want[0]) and np.array_equal(whole[1], want[1])
    assert not np.array_equal(whole[0], _sample(a, 0, 10, row_base=base + 1)[0])       # another base: other draws


# ---- zebra_amd.sampling.NegativeSampler -----------------------------------------------------------------------------------
def _want(a, sampler_kw, K, row_base=0):
    """the restatement's rows for a NegativeSampler(**sampler_kw) over a case's rows, lists from the numpy adjacency"""
    w = world()
    rounds = sampler_kw.get("rounds", 4)
    hist_rounds = (rounds + 1) // 2 if sampler_kw.get("fill", True) else rounds
    strategy = sampler_kw.get("strategy", "random")
    K_hist = {"random": 0, "historical": K, "mixed": int(sampler_kw.get("hist_ratio", 0.5) * K)}[strategy]
    flags = ((FILTER if sampler_kw.get("filtered", False) else 0) | (DISTINCT if sampler_kw.get("distinct", True) else 0)
             | (EXCLUDE_SOURCE if sampler_kw.get("exclude_source", True) else 0))
    begin, length = seen_ranges(w.indptr, w.ats, a.src, a.ts)
    return sample_rows(sampler_kw["seed"], row_base, K, K_hist, rounds, hist_rounds, flags, a.src, a.dst, w.pool, w.nbr, begin, length,
                       len(w.nbr))


@pytest.mark.parametrize("kw,K", [
    (dict(strategy="random"), 20), (dict(strategy="random", filtered=True, rounds=8), 65),
    (dict(strategy="historical"), 33), (dict(strategy="historical", fill=False, rounds=3), 33),
    (dict(strategy="mixed", filtered=True), 100), (dict(strategy="mixed", hist_ratio=0.3, distinct=False, exclude_source=False), 10),
], ids=["random", "random-filtered", "historical", "historical-nofill", "mixed-filtered", "mixed-ratio-plain"])
def test_sampler_object_equals_the_restatement(kw, K):
    from zebra_amd.sampling import NegativeSampler
    w, a = world(), case_inputs("K65")
    kw = dict(kw, seed=77)
    needs = kw["strategy"] != "random" or kw.get("filtered", False)
    smp = NegativeSampler(w.dst, finder=_finder() if needs else None, **kw)
    assert np.array_equal(smp.dst_list, w.pool) and smp.seed == 77
    smp.reset_random_state()
    neg, count = smp.sample_for(a.src, a.dst, a.ts, K, row_base=40)
    assert neg.is_cuda and count.is_cuda and neg.dtype == count.dtype == torch.int32
    assert neg.shape == (a.rows, K) and count.shape == (a.rows, 2)
    want = _want(a, kw, K, row_base=40)
    assert np.array_equal(neg.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
    again = smp.sample_for(_cuda(a.src), _cuda(a.dst), _cuda(a.ts), K, row_base=40)           # device tensors in; the same bits
    assert torch.equal(again[0], neg) and torch.equal(again[1], count)
    if needs:
        # the caller's own lists: the same ranges copied out give the same rows
        begin, length = seen_ranges(w.indptr, w.ats, a.src, a.ts)
        parts = [w.nbr[b:b + n] for b, n in zip(begin, length)]
        lptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        own = NegativeSampler(w.dst, **kw).sample_for(a.src, a.dst, a.ts, K, row_base=40, history=(lptr, np.concatenate(parts)))
        assert torch.equal(own[0], neg) and torch.equal(own[1], count)
        with pytest.raises(ValueError, match="finder"):
            NegativeSampler(w.dst, **kw).sample_for(a.src, a.dst, a.ts, K)
        with pytest.raises(ValueError, match="ptr"):
            smp.sample_for(a.src, a.dst, a.ts, K, history=(lptr[:-1], np.concatenate(parts)))
    empty = smp.sample_for(a.src[:0], a.dst[:0], a.ts[:0], K)
    assert empty[0].shape == (0, K) and empty[1].shape == (0, 2)
    for bad_k in (0, 4097):
        with pytest.raises(ValueError):
            smp.sample_for(a.src, a.dst, a.ts, bad_k)


# ---- through eval_edge_ranking and compute_rank_loss, on the 250-edge stream of test_filtered_gpu ----------------------------
N0, E, D, F, T, K_TPPR, AL, BE, SEED, BS, N_NEG, N_FULL = 80, 250, 20, 7, 20, 5, [0.2, 0.1], [0.8, 0.5], 61, 50, 20, 10


@functools.lru_cache(maxsize=None)
def _stream():
    from zebra_amd.tppr import get_neighbor_finder
    src, dst, neg, ts, eidx = I.make_stream("general", N0, E, SEED)
    N = int(max(src.max(), dst.max())) + 1
    data = types.SimpleNamespace(sources=src, destinations=dst, timestamps=ts, edge_idxs=eidx, n_interactions=E)
    return data, N, get_neighbor_finder(data), adjacency(src, dst, ts, N)


def _fresh_model():
    data, N, _, _ = _stream()
    w = I.model_weights(D, F, T, len(AL), SEED)
    _, efeat = I.random_tables(N, E + 1, D, F, SEED)
    return build_tgn(N, E + 1, D, F, T, K_TPPR, AL, BE, w, efeat)


def _stream_rows(kw, K):
    """the restatement's [E, K] rows of a NegativeSampler(**kw) over the whole stream, row s being edge s"""
    data, N, _, (indptr, nbr, ats) = _stream()
    rounds = kw.get("rounds", 4)
    K_hist = {"random": 0, "historical": K, "mixed": K // 2}[kw["strategy"]]
    flags = (FILTER if kw.get("filtered", False) else 0) | DISTINCT | EXCLUDE_SOURCE
    begin, length = seen_ranges(indptr, ats, data.sources, data.timestamps)
    return sample_rows(kw["seed"], 0, K, K_hist, rounds, (rounds + 1) // 2, flags, data.sources, data.destinations,
                       np.unique(data.destinations).astype(np.int32), nbr, begin, length, len(nbr))[0]


class _Replay:
    """RandEdgeSampler's interface handing out prepared rows: sample(B * K) returns the next B rows"""

    def __init__(self, rows):
        self.rows, self.seed, self.at = rows, 0, 0

    def reset_random_state(self):
        self.at = 0

    def sample(self, size):
        K = self.rows.shape[1]
        assert size % K == 0
        out = self.rows[self.at:self.at + size // K].reshape(-1)
        self.at += size // K
        assert out.size == size
        return None, out


@pytest.mark.parametrize("strategy", ["random", "mixed", "historical"])
def test_edge_ranking_with_the_sampler_equals_a_replay_of_its_rows(strategy):
    """the full-* settings (eight rounds, ten distinct negatives of the stream's 53 destinations: nothing is absent -- with twenty,
    rows run dry), eval unfiltered: the dict of the sampler's pass is exactly the dict of today's path fed the restatement's rows"""
    from zebra_amd import evaluation as ev
    from zebra_amd.sampling import NegativeSampler
    data, N, nf, _ = _stream()
    kw = dict(strategy=strategy, rounds=8, seed=5)
    rows = _stream_rows(kw, N_FULL)
    assert (rows >= 0).all()                                               # (the equality means something only if nothing is absent)
    got = ev.eval_edge_ranking(_fresh_model(), NegativeSampler(data.destinations, finder=nf, **kw), data, 10, batch_size=BS,
                               n_negatives=N_FULL)
    want = ev.eval_edge_ranking(_fresh_model(), _Replay(rows), data, 10, batch_size=BS, n_negatives=N_FULL)
    print(strategy, got)
    assert got == want and 0.0 < got["mrr"] <= 1.0
    # another batch size: the same negatives (rows are numbered by their position in the split), so the same ranks wherever
    # the batches' boundaries leave the state alone -- here only that the pass runs and counts every edge
    other = ev.eval_edge_ranking(_fresh_model(), NegativeSampler(data.destinations, finder=nf, **kw), data, 10, batch_size=125,
                                 n_negatives=N_FULL)
    assert 0.0 < other["mrr"] <= 1.0


def test_filtered_edge_ranking_with_mixed_negatives_matches_a_restatement():
    """strategy="mixed", one round (so slots stay empty), eval filtered: numpy ranks over [destination | row], -1 columns and
    the filtered ones not counted; the state advances by eval steps over the first column, the destination where that is -1"""
    from zebra_amd import evaluation as ev
    from zebra_amd.sampling import NegativeSampler
    data, N, nf, (indptr, nbr, ats) = _stream()
    src, dst, ts, eidx = data.sources, data.destinations, data.timestamps, data.edge_idxs
    kw = dict(strategy="mixed", rounds=1, filtered=False, seed=21)
    rows = _stream_rows(kw, N_NEG)
    assert (rows < 0).any() and (rows[:, 0] < 0).any() and (rows >= 0).any()
    got = ev.eval_edge_ranking(_fresh_model(), NegativeSampler(dst, finder=nf, **kw), data, 10, batch_size=BS, n_negatives=N_NEG,
                               filtered=True, finder=nf)
    model = _fresh_model().eval()
    model.update_memory_in_test(model.memory)
    model.test_mode = True
    acc, masked = np.zeros(5), 0
    for s in range(0, E, BS):
        e = s + BS
        cands = np.concatenate([dst[s:e, None], rows[s:e]], axis=1)
        prob = model.rank_candidates(src[s:e], ts[s:e], cands).cpu().numpy()
        begin, length = seen_ranges(indptr, ats, src[s:e], ts[s:e])
        gone = cands < 0
        for q in range(BS):
            seen = set(nbr[begin[q]:begin[q] + length[q]].tolist()) | {int(dst[s + q])}
            gone[q, 1:] |= np.array([int(v) in seen for v in cands[q, 1:]])
        gone[:, 0] = False
        masked += int(gone.sum() - (cands < 0).sum())
        acc = add_rank_sums(acc, rank_of_positive(prob, masked_idx(None, gone)))
        first = np.where(rows[s:e, 0] >= 0, rows[s:e, 0], dst[s:e])
        model.compute_temporal_embeddings(src[s:e], dst[s:e], first, ts[s:e], eidx[s:e], 10, False)
    assert masked > 0 and acc[4] == E                                      # historical negatives are partners: the filter bites
    assert got == dict(mrr=float(acc[0] / E), hits1=float(acc[1] / E), hits3=float(acc[2] / E), hits10=float(acc[3] / E))


def test_rank_loss_takes_the_samplers_tensor():
    """compute_rank_loss with sample_for's CUDA tensor (holes included): the loss and the logits of its numpy copy, bit for bit"""
    from test_rank_train_gpu import _batch, _model, _stream as train_stream
    from zebra_amd.sampling import NegativeSampler
    src, dst, ts, eidx = _batch()
    smp = NegativeSampler(train_stream()[1], seed=5, rounds=1)
    neg_d, _ = smp.sample_for(src, dst, ts, 7, row_base=3)
    neg_d[5] = -1                                                          # an edge without a negative, and a column with holes
    neg_d[::3, 2] = -1
    neg = neg_d.cpu().numpy()
    assert neg_d.is_cuda and (neg < 0).any() and (neg >= 0).any()
    a, b = _model(2), _model(2)
    loss_a, logits_a = a.compute_rank_loss(src, dst, neg_d, ts, eidx, 10)
    loss_b, logits_b = b.compute_rank_loss(src, dst, neg, ts, eidx, 10)
    assert torch.equal(loss_a.detach().view(torch.int32), loss_b.detach().view(torch.int32))
    assert torch.equal(logits_a.view(torch.int32), logits_b.view(torch.int32)) and logits_a.shape == (len(src), 8)
    loss_c, logits_c = _model(2).compute_rank_loss(src, dst, neg_d.cpu(), ts, eidx, 10)          # a host tensor as well
    assert torch.equal(loss_c.detach().view(torch.int32), loss_b.detach().view(torch.int32)) and torch.equal(logits_c, logits_b)
