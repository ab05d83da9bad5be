"""Shared by tests/test_query_cpu.py and tests/test_query_gpu.py (own code): the row emission of a read-only T-PPR query
restated in numpy, which rows of a batch a query can be held against, hand-made rank cases, a float64 MergeLayer."""
import numpy as np


def emit_rows(rows, t):
    """extract_streaming_tppr (utils/util.py:447-469) restated on ``export_rows``'s dense view (len [n], eidx / node / ts / w
    [n, k] in dictionary order) at the times ``t`` [n]: (nodes, eidx, dt, w) as int32, int32, float32, float32 [n, k].
    dt = f32(f64(t) - f64(f32(entry ts))); entries j >= len of a non-empty row read 0, 0, f32(t), 0; an empty row is zeros."""
    ln = np.asarray(rows["len"])
    k = rows["node"].shape[1]
    live = np.arange(k)[None, :] < ln[:, None]
    nodes = np.where(live, rows["node"], 0).astype(np.int32)
    eidx = np.where(live, rows["eidx"], 0).astype(np.int32)
    w = np.where(live, rows["w"].astype(np.float32), np.float32(0)).astype(np.float32)
    tsf = np.where(live, rows["ts"].astype(np.float32), np.float32(0)).astype(np.float32)
    dt = (np.asarray(t, np.float64)[:, None] - tsf.astype(np.float64)).astype(np.float32)
    dt[ln == 0] = 0
    return nodes, eidx, dt, w


def comparable(src, dst, neg):
    """bool [3B] over a batch's rows [src | dst | neg]: True where the row's node is not an endpoint of an EARLIER edge of
    the same batch -- an edge's three rows are extracted before its own update, so such a row of the stream is the row of
    the state before the batch, which is what a query ahead of the batch reads."""
    B = len(src)
    seen, ok = set(), np.zeros(3 * B, bool)
    for i in range(B):
        for r, x in enumerate((src[i], dst[i], neg[i])):
            ok[r * B + i] = int(x) not in seen
        seen.add(int(src[i]))
        seen.add(int(dst[i]))
    return ok


def rank_of_positive(prob, cand_idx=None):
    """The definition zt_rank_metrics implements, restated in numpy (pinned on rank_cases, the kernel held against it):
    column 0 of ``prob`` [Q, C] is the positive, rank = 1 + #{c >= 1 present : p_c > p_0} + 0.5 #{c >= 1 present : p_c == p_0}
    -- the mean of the optimistic and the pessimistic rank; ``cand_idx`` [Q, C] (or None: all present) marks absent entries
    with -1.  Returns float32 [Q], 0 for a query whose positive is absent (skipped, not counted)."""
    p = np.asarray(prob, np.float32)
    live = np.ones(p.shape, bool) if cand_idx is None else np.asarray(cand_idx) >= 0
    rest = live[:, 1:]
    gt = (rest & (p[:, 1:] > p[:, :1])).sum(axis=1)
    eq = (rest & (p[:, 1:] == p[:, :1])).sum(axis=1)
    rank = (1.0 + gt + 0.5 * eq).astype(np.float32)
    return np.where(live[:, 0], rank, np.float32(0))


def rank_sums(rank):
    """float64 [5] of ``rank_of_positive``'s ranks: sum of 1 / rank, Hits@1, Hits@3, Hits@10, queries counted."""
    r = np.asarray(rank, np.float64)
    r = r[r > 0]
    return np.array([np.sum(1.0 / r), np.sum(r <= 1), np.sum(r <= 3), np.sum(r <= 10), len(r)], np.float64)


# hand-made rank cases: (prob [Q][C], cand_idx [Q][C] or None, expected ranks -- 0: skipped)
def rank_cases():
    A = -1
    return [
        # no ties; a tie with the positive; every entry equal (rank = 1 + (C - 1) / 2); the positive last; the positive first
        (np.array([[0.5, 0.9, 0.1, 0.3], [0.5, 0.5, 0.1, 0.9], [0.25, 0.25, 0.25, 0.25], [0.1, 0.2, 0.3, 0.4],
                   [0.9, 0.2, 0.3, 0.4]], np.float32), None, [2.0, 2.5, 2.5, 4.0, 1.0]),
        # C = 1: the positive alone
        (np.array([[0.3], [0.0]], np.float32), None, [1.0, 1.0]),
        # absent entries do not count, whatever their probability; an absent positive skips the query; two exact ties
        (np.array([[0.5, 0.9, 0.7, 0.5], [0.5, 0.9, 0.9, 0.9], [0.2, 0.2, 0.2, 0.9], [0.6, 0.0, 0.0, 0.0]], np.float32),
         np.array([[0, A, 1, 2], [A, 0, 1, 2], [0, 1, A, A], [3, A, A, A]], np.int32), [2.5, 0.0, 1.5, 1.0]),
        # eleven above the positive: outside Hits@10; exactly ten with a tie: rank 10.5
        (np.concatenate([[[0.1]], np.full((1, 11), 0.2)], axis=1).astype(np.float32), None, [12.0]),
        (np.concatenate([[[0.2]], np.full((1, 9), 0.3), [[0.2]]], axis=1).astype(np.float32), None, [10.5]),
    ]


def merge_f64(emb_q, emb_c, idx, w):
    """float64 MergeLayer (utils/util.py:14-26) of emb_q[q] against emb_c[idx[q, c]] -> prob [Q, C]; absent (-1) reads 0"""
    W1, b1 = w["aff1_w"].astype(np.float64), w["aff1_b"].astype(np.float64)
    W2, b2 = w["aff2_w"].astype(np.float64), w["aff2_b"].astype(np.float64)
    H = emb_q.shape[1]
    pq = emb_q.astype(np.float64) @ W1[:, :H].T + b1
    pc = emb_c.astype(np.float64) @ W1[:, H:].T
    out = np.zeros(idx.shape, np.float64)
    for q in range(idx.shape[0]):
        live = idx[q] >= 0
        hid = np.maximum(pq[q][None, :] + pc[idx[q][live]], 0.0)
        out[q, live] = 1.0 / (1.0 + np.exp(-(hid @ W2[0] + b2[0])))
    return out
