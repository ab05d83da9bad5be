"""Shared by tests/test_topk_cpu.py and tests/test_topk_gpu.py (own code): the selection rule of zt_affinity_topk /
TGN.topk_scores restated in numpy."""
import numpy as np


def select_topk(prob, cand_idx, K, skip=None, idx_base=0):
    """(idx [Q, K] int32, prob [Q, K] float32) of ``prob`` [Q, C]: per row the K present entries with the largest
    probability, descending, equal probabilities in ascending column; slots beyond the present ones read -1 and 0.
    ``idx`` = ``idx_base`` + column.  Present: ``cand_idx`` [Q, C] (or None: all) is >= 0, the probability is not NaN, and
    ``idx_base`` + column differs from ``skip[q]`` (or None; -1: nothing left out)."""
    p = np.asarray(prob, np.float32)
    Q, C = p.shape
    live = ~np.isnan(p)
    if cand_idx is not None:
        live &= np.asarray(cand_idx) >= 0
    cols = np.arange(C, dtype=np.int64) + idx_base
    if skip is not None:
        live &= cols[None, :] != np.asarray(skip, np.int64)[:, None]
    out_i = np.full((Q, K), -1, np.int32)
    out_p = np.zeros((Q, K), np.float32)
    for q in range(Q):
        c = np.nonzero(live[q])[0]
        order = c[np.lexsort((c, -p[q, c].astype(np.float64)))][:K]      # by (-prob, column)
        out_i[q, :len(order)] = cols[order]
        out_p[q, :len(order)] = p[q, order]
    return out_i, out_p
