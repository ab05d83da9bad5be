"""Negative sampling on the device (include/zebra_amd.h, zt_neg_sample; csrc/neg_sample.hip): the negatives of the ranking
paths -- eval_edge_ranking, TGN.compute_rank_loss -- drawn per edge from the destination pool and from the source's own
history, with the exclusions applied while drawing.  There is no host path: every draw is the HIP kernel's."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import check, lib, ptr, stream_ptr

STRATEGIES = ("random", "historical", "mixed")


class NegativeSampler:
    """Up to ``n_negatives`` negatives per edge, reproducible: row ``row_base + q`` of a pass gets the same ids whatever batch
    it arrives in (a counter-based generator keyed by ``seed``; the rule is stated at zt_neg_sample in the header).
    The pool is ``np.unique(dst_list)``, as the reference's RandEdgeSampler draws its destinations.  ``strategy``:
    "random" -- every slot draws from the pool; "historical" -- every slot draws from the source's partners strictly before
    the edge's timestamp (Poursafaei et al. 2022); "mixed" -- the first ``int(hist_ratio * n_negatives)`` slots are
    historical, the others random.  ``fill`` (default) lets a historical slot that found nothing in the history within the first
    ``(rounds + 1) // 2`` rounds draw from the pool in the others; without it such a slot stays -1.
    An edge's own destination is never drawn; ``exclude_source`` leaves its source out as well, ``distinct`` allows no id twice
    in a row, ``filtered`` rejects pool draws that are partners of the source before the edge's time (history draws are
    partners by construction).  A slot that is still empty after ``rounds`` rounds reads -1: absent, which rank_candidates,
    zt_rank_metrics and compute_rank_loss understand.
    ``finder``: the NeighborFinder the histories come from (``seen_ranges_device``); only "random" without ``filtered`` does
    without one -- unless ``sample_for`` is given the caller's own lists."""

    def __init__(self, dst_list, seed, finder=None, strategy="random", hist_ratio=0.5, filtered=False, distinct=True,
                 exclude_source=True, rounds=4, fill=True, device=None):
        if strategy not in STRATEGIES:
            raise ValueError("NegativeSampler: strategy is one of %s" % (STRATEGIES,))
        if not 0.0 <= float(hist_ratio) <= 1.0:
            raise ValueError("NegativeSampler: hist_ratio is a fraction of the slots, 0 .. 1")
        if not 1 <= int(rounds) <= _capi.NEG_MAX_ROUNDS:
            raise ValueError("NegativeSampler: rounds is 1 .. %d" % _capi.NEG_MAX_ROUNDS)
        if seed is None:
            raise ValueError("NegativeSampler: a seed is required (the draws are a function of it)")
        self.seed = int(seed)
        self.dst_list = np.unique(np.asarray(dst_list)).astype(np.int32)
        if self.dst_list.size == 0:
            raise ValueError("NegativeSampler: the destination pool is empty")
        self.device = torch.device(device if device is not None else "cuda")
        self.pool = torch.from_numpy(self.dst_list).to(self.device)
        self.finder, self.strategy, self.hist_ratio = finder, strategy, float(hist_ratio)
        self.filtered, self.distinct, self.exclude_source = bool(filtered), bool(distinct), bool(exclude_source)
        self.rounds = int(rounds)
        self.hist_rounds = (self.rounds + 1) // 2 if fill else self.rounds
        self.flags = ((_capi.NEG_FILTER if self.filtered else 0) | (_capi.NEG_DISTINCT if self.distinct else 0)
                      | (_capi.NEG_EXCLUDE_SOURCE if self.exclude_source else 0))

    def reset_random_state(self):
        """Nothing to reset: a draw is a function of (seed, row, slot, round), not of what was drawn before."""

    def k_hist(self, n_negatives):
        """the historical slots among ``n_negatives``"""
        K = int(n_negatives)
        return {"random": 0, "historical": K, "mixed": int(self.hist_ratio * K)}[self.strategy]

    def _as_device(self, a, dtype):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device, dtype).reshape(-1).contiguous()

    def _lists(self, src_d, ts_d, history):
        """(handle, ids, begin, len) of the rows' lists, or four Nones where no slot and no filter reads one"""
        Q = src_d.numel()
        if history is None:
            if self.strategy == "random" and not self.filtered:
                return None, None, None, None
            if self.finder is None:
                raise ValueError("NegativeSampler: strategy=%r%s needs a finder (or sample_for(history=(ptr, ids)))"
                                 % (self.strategy, ", filtered=True" if self.filtered else ""))
            begin, length = self.finder.seen_ranges_device(src_d, ts_d)
            return self.finder._h, None, begin, length
        if not (isinstance(history, (tuple, list)) and len(history) == 2):
            raise ValueError("NegativeSampler: history is (ptr [B + 1], ids)")
        lp = self._as_device(history[0], torch.int64)
        ids = self._as_device(history[1], torch.int32)
        if lp.numel() != Q + 1:
            raise ValueError("NegativeSampler: history=(ptr, ids): ptr holds B + 1 offsets into ids")
        if Q > 0:                                                         # (the kernel trusts the caller's ranges: one host read)
            bad = (lp[1:] < lp[:-1]).any() | (lp[0] < 0) | (lp[-1] > ids.numel())
            if bool(bad):
                raise ValueError("NegativeSampler: history=(ptr, ids): ptr must ascend from >= 0 to <= len(ids)")
        if ids.numel() == 0:
            ids = torch.zeros(1, dtype=torch.int32, device=self.device)   # (an address to hand over; never read)
        return None, ids, lp[:-1].contiguous(), (lp[1:] - lp[:-1]).contiguous()

    @torch.no_grad()
    def sample_for(self, sources, destinations, timestamps, n_negatives, row_base=0, history=None):
        """(neg int32 CUDA [B, n_negatives], count int32 CUDA [B, 2]) for the edges (sources[b], destinations[b]) at
        timestamps[b]: -1 where a slot stayed empty; count[b] = (slots filled from the history, slots filled from the pool).
        Row b is row ``row_base + b`` of the pass: give every batch its position in the split and the pass draws the same
        negatives at any batch size.  ``history=None``: the lists are the source's partners strictly before the timestamp in
        the finder (never copied); ``history=(ptr [B + 1], ids)``: the caller's own per-row lists ids[ptr[b]:ptr[b + 1]], as
        TGN.absent_bits takes them -- an inductive set, say.  No host synchronisation beyond the finder's status read."""
        K = int(n_negatives)
        if not 1 <= K <= _capi.NEG_MAX_K:
            raise ValueError("NegativeSampler: n_negatives is 1 .. %d" % _capi.NEG_MAX_K)
        src_d = self._as_device(sources, torch.int32)
        dst_d = self._as_device(destinations, torch.int32)
        B = src_d.numel()
        if dst_d.numel() != B:
            raise ValueError("NegativeSampler: one destination per source")
        ts_d = self._as_device(timestamps, torch.float64)
        if ts_d.numel() != B:
            raise ValueError("NegativeSampler: one timestamp per source")
        handle, ids, begin, length = self._lists(src_d, ts_d, history)
        neg = torch.empty((B, K), dtype=torch.int32, device=self.device)
        count = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        if B == 0:
            return neg, count
        d = _capi.NegDesc(seed=self.seed & 0xFFFFFFFFFFFFFFFF, row_base=int(row_base), K=K, K_hist=self.k_hist(K),
                          rounds=self.rounds, hist_rounds=self.hist_rounds, flags=self.flags)
        check(lib().zt_neg_sample(C.byref(d), ptr(src_d), ptr(dst_d), C.c_int64(B), ptr(self.pool), C.c_int64(self.pool.numel()),
                                  handle, ptr(ids), ptr(begin), ptr(length), ptr(neg), ptr(count), stream_ptr()),
              "zt_neg_sample")
        return neg, count
