"""Shared by tests/test_negsample_cpu.py and tests/test_negsample_gpu.py (own code): the rule of zt_neg_sample
(include/zebra_amd.h) restated in numpy -- a direct loop over rows, rounds and slots --, Philox4x32-10, and the case table."""
import functools
import types

import numpy as np

from helpers_filtered import adjacency, seen_ranges

FILTER, DISTINCT, EXCLUDE_SOURCE = 1, 2, 4
ALL = FILTER | DISTINCT | EXCLUDE_SOURCE
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """The four output words of Philox4x32-10 (Salmon et al. 2011, Random123): ``ctr`` = four and ``key`` = two 32-bit words,
    each an int or an array (broadcast together); uint64 arrays holding 32-bit values come back."""
    c = [np.asarray(x, np.uint64) & M32 for x in ctr]
    k = [np.asarray(x, np.uint64) & M32 for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]      # (32 x 32 bits: no overflow in 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return c


def draw_words(seed, row, slots, r):
    """x of the rule for slots ``slots`` (array) of row ``row`` in round ``r``: python ints"""
    seed, row = int(seed) & (2 ** 64 - 1), int(row) & (2 ** 64 - 1)
    x = philox4x32_10((row & 0xFFFFFFFF, row >> 32, np.asarray(slots, np.uint64), r), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return [int(v) for v in np.broadcast_to(x, np.shape(slots))]


def clip_range(b, n, n_ids):
    """zt_exclude_mark's convention: a negative begin or len is an empty list; a range of the handle's array (n_ids: its
    length, None for the caller's own array) is clipped to it"""
    b, n = int(b), int(n)
    if b < 0 or n < 0:
        n = 0
    if n_ids is not None:
        n = 0 if b > n_ids else min(n, n_ids - b)
    return b, n


def sample_rows(seed, row_base, K, K_hist, rounds, hist_rounds, flags, src, dst, pool, ids=None, begin=None, length=None,
                n_ids=None, trace=False):
    """(neg int32 [Q, K], count int32 [Q, 2]) by the rule, and with ``trace`` also a dict: ``round`` [Q, K] the round that
    filled a slot (-1: none), ``kind`` [Q, K] 1 = from the list, 2 = from the pool, 0 = empty, and ``rejects`` -- per row a dict
    counting the rejections by rule (negative, destination, source, filter, earlier, same_round)."""
    Q, n_pool = len(src), len(pool)
    neg = np.full((Q, K), -1, np.int32)
    count = np.zeros((Q, 2), np.int32)
    rnd = np.full((Q, K), -1, np.int32)
    kind = np.zeros((Q, K), np.int32)
    rejects = []
    for q in range(Q):
        b, n = (0, 0) if ids is None or begin is None else clip_range(begin[q], length[q], n_ids)
        lst = [] if n == 0 else [int(v) for v in ids[b:b + n]]
        members = set(v for v in lst if v >= 0)
        rej = dict(negative=0, destination=0, source=0, filter=0, earlier=0, same_round=0)
        for r in range(rounds):
            empty = [j for j in range(K) if neg[q, j] < 0]
            if not empty:
                break
            earlier = set(int(v) for v in neg[q] if v >= 0)            # slots filled in earlier rounds
            passed = set()                                             # ids of this round's passing draws so far
            for j, x in zip(empty, draw_words(seed, row_base + q, empty, r)):
                from_list = j < K_hist and r < hist_rounds and n > 0
                v = lst[(x * n) >> 32] if from_list else int(pool[(x * n_pool) >> 32])
                if v < 0:
                    rej["negative"] += 1
                elif v == int(dst[q]):
                    rej["destination"] += 1
                elif flags & EXCLUDE_SOURCE and v == int(src[q]):
                    rej["source"] += 1
                elif flags & FILTER and not from_list and v in members:
                    rej["filter"] += 1
                elif flags & DISTINCT and v in earlier:
                    rej["earlier"] += 1
                elif flags & DISTINCT and v in passed:                 # passes, but a lower slot's draw passed with it first
                    rej["same_round"] += 1
                else:
                    passed.add(v)
                    neg[q, j], rnd[q, j], kind[q, j] = v, r, 1 if from_list else 2
        count[q] = [(kind[q] == 1).sum(), (kind[q] == 2).sum()]
        rejects.append(rej)
    if trace:
        return neg, count, dict(round=rnd, kind=kind, rejects=rejects)
    return neg, count


# ---- the world of the cases: hubs whose histories have the lengths the kernel's strides and tiles turn at ----------------------
LENS = (0, 1, 255, 256, 257, 1000)
HUBS = (1, 2, 3, 4, 5, 6)                   # hub i holds LENS[i] entries; node 1 none at all
N_NODES = 1200
OUTSIDE = 1150                              # a destination that is in no pool


@functools.lru_cache(maxsize=None)
def world():
    """An edge stream hub -> partner with duplicate partners (ids 100 ..), background edges that widen the pool (ids 700 ..),
    its adjacency (helpers_filtered.adjacency) and the time after everything"""
    rng = np.random.RandomState(7)
    src, dst = [], []
    for hub, n in zip(HUBS, LENS):
        src += [hub] * n
        dst += rng.randint(100, 100 + max(1, (6 * n) // 10), n).tolist()      # ~45 % of a long list are repeats
    nb = 400
    src += rng.randint(700, 1100, nb).tolist()
    dst += rng.randint(700, 1100, nb).tolist()
    order = rng.permutation(len(src))
    src, dst = np.array(src, np.int32)[order], np.array(dst, np.int32)[order]
    ts = np.arange(1, len(src) + 1, dtype=np.float64)
    indptr, nbr, ats = adjacency(src, dst, ts, N_NODES)
    return types.SimpleNamespace(src=src, dst=dst, ts=ts, eidx=np.arange(1, len(src) + 1, dtype=np.int64), indptr=indptr,
                                 nbr=nbr, ats=ats, t_end=float(len(src) + 10), pool=np.unique(dst).astype(np.int32))


def _rows(n_rows):
    """(sources, destinations, timestamps) of a case: every hub, the longest one also at half time, a pool member; destinations that are a
    partner of the source, one that is not, and one outside every pool"""
    w = world()
    deg = np.diff(w.indptr)
    bg = int(w.pool[np.argmax(deg[w.pool] * (w.pool >= 700))])          # a source that is in the pool itself, with a history
    srcs = np.array([1, 2, 3, 4, 5, 6, 6, bg, 3, 4, 5, 6, 6, bg, 2, 5][:n_rows], np.int32)
    ts = np.full(n_rows, w.t_end)
    if n_rows > 6:
        ts[6] = w.ats[w.indptr[6] + 500]                                # 500 entries (or a few less: none AT the time) before it
    dsts = np.zeros(n_rows, np.int32)
    for q, s in enumerate(srcs):
        lo, hi = w.indptr[s], w.indptr[s + 1]
        dsts[q] = w.nbr[lo + (q % (hi - lo))] if hi > lo and q % 2 == 0 else w.pool[(37 * q + 11) % len(w.pool)]
    dsts[min(3, n_rows - 1)] = OUTSIDE
    return srcs, dsts, ts


def _case(K, K_hist=None, rounds=4, hist_rounds=None, flags=ALL, pool="world", lists="handle", rows=16, seed=2024, row_base=0):
    return dict(K=K, K_hist=K // 2 if K_hist is None else K_hist, rounds=rounds,
                hist_rounds=(rounds + 1) // 2 if hist_rounds is None else hist_rounds, flags=flags, pool_kind=pool, lists_kind=lists,
                rows=rows, seed=seed, row_base=row_base)


# K at the one-wave form's end (128), at every sort width (a power of two) and beside it, at the workgroup sizes' seams
# (128 | 129: 64 -> 256 threads, 1024 | 1025: 256 -> 1024) and at the limit
K_SEAMS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096)
CASES = {"K%d" % K: _case(K, rows=16 if K <= 300 else 8, seed=100 + K, row_base=K) for K in K_SEAMS}
CASES.update({
    "khist-0": _case(100, K_hist=0), "khist-1": _case(100, K_hist=1), "khist-K": _case(100, K_hist=100),
    "hist-rounds-0": _case(100, hist_rounds=0), "hist-rounds-all": _case(100, hist_rounds=4),
    "rounds-1": _case(100, rounds=1), "rounds-8": _case(100, rounds=8),
    "rounds-8-nofill": _case(300, K_hist=300, rounds=8, hist_rounds=8),
    "flags-none": _case(100, flags=0), "flags-filter": _case(100, flags=FILTER), "flags-distinct": _case(100, flags=DISTINCT),
    "flags-source": _case(100, flags=EXCLUDE_SOURCE), "flags-none-K1000": _case(1000, flags=0, rows=8),
    "flags-filter-K1000": _case(1000, flags=FILTER, rows=8),
    "no-lists": _case(100, lists="none"),
    "dry-pool40-K32": _case(32, K_hist=0, pool="forty", seed=5),
    "dry-pool40-K32-mixed": _case(32, pool="forty", seed=6, rounds=8),
    "source-off-pool40": _case(32, K_hist=0, pool="forty", flags=FILTER | DISTINCT, seed=8),
    "source-on-pool40": _case(32, K_hist=0, pool="forty", seed=8),
    "covered-pool": _case(24, K_hist=0, pool="covered", flags=FILTER | DISTINCT),
    "covered-pool-undistinct": _case(24, K_hist=0, pool="covered", flags=FILTER),
    "own-lists-negative": _case(100, lists="own"), "own-lists-negative-K600": _case(600, lists="own", rows=8),
    "clipped": _case(64, lists="clipped", rows=8),
    "big-row-base": _case(65, row_base=(1 << 33) + 5, seed=(1 << 63) + 12345),
    # (the first five hubs: at most a fifth of the pool is filtered away, eight rounds leave nothing empty)
    "full-random": _case(20, K_hist=0, rounds=8, rows=5), "full-mixed": _case(20, rounds=8, rows=5),
    "full-historical": _case(20, K_hist=20, rounds=8, rows=5),
})

# what a case's id promises, shown from the trace by test_negsample_cpu.py
REACHES = {
    "rounds-8-nofill": "last_round_accept", "flags-distinct": "same_round", "K255": "earlier", "flags-filter": "filter",
    "dry-pool40-K32": "ends_empty", "khist-K": "hist_slot_from_pool",
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The arguments of zt_neg_sample for a case, on the host: namespace(desc fields, src, dst, ts, pool, ids, begin, length,
    n_ids, lists).  ids None: no lists at all; n_ids None: the caller's own array."""
    c = CASES[name]
    w = world()
    src, dst, ts = _rows(c["rows"])
    ids = begin = length = n_ids = None
    if c["lists_kind"] != "none":
        begin, length = seen_ranges(w.indptr, w.ats, src, ts)
        ids, n_ids = w.nbr, len(w.nbr)
    if c["lists_kind"] == "clipped":                       # ranges that leave the handle's array, and negative ones
        begin, length = begin.copy(), length.copy()
        begin[0], length[0] = n_ids - 3, 10
        begin[1], length[1] = n_ids, 5
        begin[2], length[2] = -4, 2
        begin[3], length[3] = 7, -1
        begin[4], length[4] = n_ids + 9, 3
    if c["lists_kind"] == "own":                           # the caller's (ptr, ids): each row's list copied out, negative ids mixed in
        parts = [w.nbr[b:b + n].copy() for b, n in zip(begin, length)]
        for i, p in enumerate(parts):
            p[i % 3::3] = np.array([-1, -7])[np.arange(len(p[i % 3::3])) % 2]
        ptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        ids, n_ids = np.concatenate(parts).astype(np.int32), None
        begin, length = ptr[:-1].copy(), np.diff(ptr)
    if c["pool_kind"] == "world":
        pool = w.pool
    elif c["pool_kind"] == "forty":                        # 40 ids, most of them partners of the hubs: rows collide and run dry
        base = np.unique(np.concatenate([w.nbr[w.indptr[6]:w.indptr[6] + 30], w.pool[-25:]]))
        pool = np.sort(np.concatenate([base[base != src[7]][:39], src[7:8]])).astype(np.int32)      # ... and row 7's source
        assert len(pool) == 40
    else:                                             # every pool id is a partner of hub 6 (and of nobody's list else)
        pool = np.unique(w.nbr[w.indptr[6] + 600:w.indptr[6] + 640]).astype(np.int32)
    return types.SimpleNamespace(src=src, dst=dst, ts=ts, pool=pool, ids=ids, begin=begin, length=length, n_ids=n_ids, **c)


@functools.lru_cache(maxsize=None)
def case_expected(name):
    """(neg, count, trace) of the restatement for a case -- computed once, shared, read-only"""
    a = case_inputs(name)
    neg, count, tr = sample_rows(a.seed, a.row_base, a.K, a.K_hist, a.rounds, a.hist_rounds, a.flags, a.src, a.dst, a.pool,
                                 a.ids, a.begin, a.length, a.n_ids, trace=True)
    for arr in (neg, count, tr["round"], tr["kind"]):
        arr.setflags(write=False)
    return neg, count, tr
