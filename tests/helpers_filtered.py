"""Shared by tests/test_filtered_cpu.py and tests/test_filtered_gpu.py (own code): the adjacency, the "seen" lists, the absent
bits (include/zebra_amd.h, zt_affinity_topk_masked) and the sequential rank sums restated in numpy."""
import numpy as np


def adjacency(src, dst, ts, num_nodes):
    """(indptr int64 [N + 1], nbr int32 [2E], ts float64 [2E]) of an edge stream: both directions of every edge in stream
    order, then each node's entries stably sorted by time -- get_neighbor_finder's arrays."""
    per = [[] for _ in range(num_nodes)]
    for i in range(len(src)):
        per[int(src[i])].append((float(ts[i]), int(dst[i])))
        per[int(dst[i])].append((float(ts[i]), int(src[i])))
    indptr = np.zeros(num_nodes + 1, np.int64)
    nbr, tt = [], []
    for v in range(num_nodes):
        order = sorted(range(len(per[v])), key=lambda j: per[v][j][0])       # (sorted is stable)
        nbr += [per[v][j][1] for j in order]
        tt += [per[v][j][0] for j in order]
        indptr[v + 1] = len(nbr)
    return indptr, np.array(nbr, np.int32), np.array(tt, np.float64)


def seen_ranges(indptr, ats, nodes, times):
    """(begin, len) int64 [Q]: begin = indptr[v], len = the number of v's entries with a timestamp strictly below t, counted
    one by one; a node outside [0, N) gives (0, 0)."""
    n = len(indptr) - 1
    begin, length = np.zeros(len(nodes), np.int64), np.zeros(len(nodes), np.int64)
    for q, (v, t) in enumerate(zip(nodes, times)):
        if 0 <= v < n:
            begin[q] = indptr[v]
            length[q] = sum(1 for x in ats[indptr[v]:indptr[v + 1]] if x < t)
    return begin, length


def mark_bits(ids, begin, length, C, W, id_lo=0, cand=None):
    """uint32 [Q, W] absent bits: bit c & 31 of word c >> 5 of row q is set where column c of the pool holds an id of query q's
    list ids[begin[q] : begin[q] + length[q]].  The pool is ``cand`` ([C] or [Q, C]; -1: an absent entry, never matched) or the
    ids id_lo .. id_lo + C - 1.  Negative list ids and ids outside the pool are ignored; every other bit is 0."""
    Q = len(begin)
    out = np.zeros((Q, W), np.uint32)
    for q in range(Q):
        members = set(int(x) for x in ids[begin[q]:begin[q] + length[q]] if x >= 0)
        row = (np.arange(C) + id_lo) if cand is None else (cand if np.ndim(cand) == 1 else cand[q])
        for c in range(C):
            if int(row[c]) >= 0 and int(row[c]) in members:
                out[q, c >> 5] |= np.uint32(1 << (c & 31))
    return out


def bits_to_mask(absent, C):
    """bool [Q, C]: True where the column's absent bit is set"""
    a = np.asarray(absent).view(np.uint32)
    c = np.arange(C)
    return ((a[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


def mask_to_bits(mask, W=None):
    """uint32 [Q, W] absent bits of a bool [Q, C] mask (W: ceil(C / 32) by default; spare bits 0)"""
    Q, C = mask.shape
    W = (C + 31) // 32 if W is None else W
    out = np.zeros((Q, W), np.uint32)
    for q, c in zip(*np.nonzero(mask)):
        out[q, c >> 5] |= np.uint32(1 << (c & 31))
    return out


def masked_idx(cand_idx, mask):
    """cand_idx [Q, C] for select_topk with the masked columns turned into -1 (cand_idx None: every column present before)"""
    base = np.zeros(mask.shape, np.int32) if cand_idx is None else np.asarray(cand_idx, np.int32)
    return np.where(mask, np.int32(-1), base)


def add_rank_sums(acc, rank):
    """zt_rank_metrics' accumulation restated: float64 [5] ``acc`` plus, query by query in order, 1 / rank, Hits@1, Hits@3,
    Hits@10 and the count (rank 0: skipped) -- the same additions in the same order, so the bits agree."""
    acc = np.array(acc, np.float64)
    for r in np.asarray(rank, np.float32):
        if r == 0:
            continue
        acc[0] += 1.0 / float(r)
        acc[1] += 1.0 if r <= 1 else 0.0
        acc[2] += 1.0 if r <= 3 else 0.0
        acc[3] += 1.0 if r <= 10 else 0.0
        acc[4] += 1.0
    return acc
