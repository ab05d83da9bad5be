"""The evaluation metrics from integer counts (numpy and `fractions` only): what tests/test_metrics_exact_gpu.py holds
zt_link_metrics and zt_rank_metrics to, and tests/test_metrics_exact_cpu.py the torch composition of zebra_amd.evaluation.

link_metrics_exact   AP, AUC and accuracy of P positive and N negative float32 scores, scikit-learn's definitions
                     (average_precision_score, roc_auc_score; the reference's accuracy, evaluation/evaluation.py:40-45):
                     the distinct thresholds are the distinct scores under IEEE equality (-0.0 and +0.0 are ONE level),
                     tp / fp at a threshold are integers, every term is a rational number rounded once.
rank_exact           one positive (column 0) against the present candidates of its row: integer counts above and equal, the
                     rank 1 + gt + eq / 2, and the five sums zt_rank_metrics accumulates.

Scores are NaN-free (scikit-learn raises on NaN; the kernels leave it undefined)."""
import math
from fractions import Fraction

import numpy as np


def _counts(pos, neg):
    """(tp, fp) int64 per distinct threshold, thresholds descending: how many positives / negatives score >= it"""
    levels = np.unique(np.concatenate([pos, neg]))[::-1]          # np.unique compares with !=: +-0 are one level
    sp, sn = np.sort(pos), np.sort(neg)
    tp = pos.size - np.searchsorted(sp, levels, side="left")
    fp = neg.size - np.searchsorted(sn, levels, side="left")
    return tp.astype(np.int64), fp.astype(np.int64)


def link_metrics_exact(pos, neg):
    """float64 [AP, AUC, accuracy]; accuracy is NaN when the classes differ in size (it pairs pos[i] with neg[i])."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1)
    neg = np.ascontiguousarray(neg, np.float32).reshape(-1)
    P, N = int(pos.size), int(neg.size)
    if P == 0 or N == 0:
        raise ValueError("link_metrics_exact needs at least one score of each class")
    if np.isnan(pos).any() or np.isnan(neg).any():
        raise ValueError("link_metrics_exact: NaN scores are outside the contract")
    tp, fp = _counts(pos, neg)
    tp_prev = np.concatenate([[0], tp[:-1]])
    fp_prev = np.concatenate([[0], fp[:-1]])
    # AUC: trapezoids (fp - fp_prev) / N x (tp + tp_prev) / (2 P), one exact integer over 2 P N
    area2 = sum(int(a) * int(b) for a, b in zip(fp - fp_prev, tp + tp_prev))
    auc = float(Fraction(area2, 2 * P * N))
    # AP: sum over thresholds of (R_n - R_{n-1}) P_n = (tp - tp_prev) / P x tp / (tp + fp); thresholds no positive takes add 0
    terms = [float(Fraction(int(d) * int(t), P * (int(t) + int(f))))
             for d, t, f in zip(tp - tp_prev, tp, fp) if d]
    ap = math.fsum(terms)
    acc = int(np.count_nonzero(pos >= neg)) / P if P == N else float("nan")
    return np.array([ap, auc, acc], np.float64)


def auc_pairwise(pos, neg):
    """AUC as P(pos > neg) + P(pos == neg) / 2 over all P x N pairs: an O(P N) count, for pinning link_metrics_exact"""
    pos = np.asarray(pos, np.float32).reshape(-1, 1)
    neg = np.asarray(neg, np.float32).reshape(1, -1)
    gt, eq = int(np.count_nonzero(pos > neg)), int(np.count_nonzero(pos == neg))
    return float(Fraction(2 * gt + eq, 2 * pos.size * neg.size))


def rank_exact(prob, cand_idx=None):
    """prob float32 [Q, C], column 0 the positive; cand_idx [Q, C] or None (all present), < 0: absent.  Returns dict(gt, eq
    int64 [Q]; rank float64 [Q], 0 where the positive is absent (the query is skipped); sums float64 [5]: sum of 1 / rank,
    Hits@1, Hits@3, Hits@10, queries counted; exact: the five as Fractions before rounding)."""
    prob = np.asarray(prob, np.float32)
    Q, C = prob.shape
    live = np.ones((Q, C), bool) if cand_idx is None else np.asarray(cand_idx) >= 0
    counted = live[:, 0].copy()
    others = live[:, 1:] & counted[:, None]
    p0 = prob[:, :1]
    gt = np.count_nonzero((prob[:, 1:] > p0) & others, axis=1).astype(np.int64)
    eq = np.count_nonzero((prob[:, 1:] == p0) & others, axis=1).astype(np.int64)
    rank = np.where(counted, 1.0 + gt + 0.5 * eq, 0.0)
    twice = 2 + 2 * gt + eq                                        # 2 x rank, an integer
    exact = [sum((Fraction(2, int(t)) for t, c in zip(twice, counted) if c), Fraction(0)),
             Fraction(int(np.count_nonzero(counted & (twice <= 2)))), Fraction(int(np.count_nonzero(counted & (twice <= 6)))),
             Fraction(int(np.count_nonzero(counted & (twice <= 20)))), Fraction(int(np.count_nonzero(counted)))]
    return dict(gt=gt, eq=eq, rank=rank, sums=np.array([float(x) for x in exact], np.float64), exact=exact)
