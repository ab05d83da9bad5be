"""Shared by tests/test_count_exact_cpu.py and tests/test_count_exact_gpu.py (own code): planted cases for zt_affinity_count on
the dialled scorer of tests/helpers_topk_planted.py, with the seam each one names, and the expectation computed on the host
from the planted levels alone.

A pair scores exactly its planted level (helpers_topk_planted.py), float32's sigmoid is strictly increasing over the levels
(test_float32_sigmoid_orders_every_level), so equal levels are exactly the equal bits and the counts follow from comparing
SCORES: a threshold is the score of a planted target row -- ("level", L): the query's dial at level L; its float32 bits come
from zt_affinity_rank on that row, the host cannot reproduce expf's -- or a constant that stands for a score: 0.5f for score 0,
1.0f for +U_ONE (every level's sigmoid is below it), +-0.0f for -U_ZERO on a falling dial (every level's sigmoid is above it),
NaN for nothing at all."""
import functools

import numpy as np

import helpers_topk_planted as P

MAX_SKIP = 4
STEP, WAVE_COLS = 128, 32
CONST_SCORE = {"half": 0.0, "one": P.U_ONE, "zero": -P.U_ZERO, "negzero": -P.U_ZERO, "nan": np.nan}
CONST_BITS = {"half": np.float32(0.5), "one": np.float32(1.0), "zero": np.float32(0.0), "negzero": np.float32(-0.0),
              "nan": np.float32(np.nan)}


def plan_of(Q, Nc, H=20, ws_rows=None):
    """count_plan restated for the recommended workspace (or one cut to ws_rows slab rows): (slab_rows, n_slabs, span_cols,
    n_spans); test_count_exact_cpu.py holds every case's ``reach`` against _capi.count_plan"""
    cap = max(32, min(1 << 18, (128 << 20) // (H * 4) // 32 * 32))
    slab = min(cap, (max(Nc, 32) + 31) // 32 * 32) if ws_rows is None else ws_rows
    n_slabs = max(1, (Nc + slab - 1) // slab)
    cols = min(slab, max(Nc, 1))
    q_tiles = (Q + 3) // 4
    max_spans = max(1, (2048 + q_tiles - 1) // max(1, q_tiles))
    n = min(max_spans, max(1, cols // (STEP * 4)))
    span_cols = ((cols + n - 1) // n + STEP - 1) // STEP * STEP
    return slab, n_slabs, span_cols, max(1, (cols + span_cols - 1) // span_cols)


class CountCase:
    """One planted input.  ``make()`` -> dict(u [D, C] float64 levels * LEVEL_U (or U_ONE / U_ZERO), falling, mask [D, C] or
    None, thr: one ("level", L) or ("const", name) per query, skip [Q, n] GLOBAL columns or None, nan_cols: candidate rows that
    are NaN).  Query q sits on dial q % D.  ``pieces``: [(begin, end), ...] the pool is given in, in that order, under
    accumulate with idx_base + begin; ``incoming``: the counts the outputs hold before the first call."""

    def __init__(self, id, Q, C, make, H=20, ws_rows=None, reach=None, B=64.0, pieces=None, idx_base=0, incoming=None,
                 nan_rows=(), coords=None):
        self.id, self.Q, self.C, self.make, self.H, self.ws_rows = id, Q, C, make, H, ws_rows
        self.reach, self.B, self.pieces, self.idx_base, self.incoming = dict(reach or {}), B, pieces, idx_base, incoming
        self.nan_rows, self.coords = tuple(nan_rows), coords

    def __repr__(self):
        return self.id

    def workspace_bytes(self, capi, Q=None, Nc=None):
        import ctypes as C_
        ws = capi.lib().zt_affinity_count_workspace_bytes
        Q = self.Q if Q is None else Q
        if self.ws_rows is None:
            return int(ws(C_.c_int64(Q), C_.c_int64(self.C if Nc is None else Nc), C_.c_int32(self.H)))
        return int(ws(C_.c_int64(Q), C_.c_int64(32), C_.c_int32(self.H))) + (self.ws_rows - 32) * self.H * 4

    def plan(self, capi):
        return capi.count_plan(self.Q, self.C, self.H, self.workspace_bytes(capi))

    @functools.lru_cache(maxsize=None)
    def data(self):
        """helpers_topk_planted.Case.data() of the pool (u, S, coord, dial_of, emb_q, emb_c, mask, bits) plus thr_spec,
        thr_score [Q] (the score a threshold stands for, NaN: none), emb_t [Q, H] (the planted target rows of the level
        thresholds), skip [Q, n] or None, nan_cols"""
        m = dict(self.make())
        base = P.Case(self.id, 1, True, self.Q, self.C, lambda: dict(u=m["u"], falling=m.get("falling", ()), mask=m.get("mask")),
                      H=self.H, B=self.B, nan_rows=self.nan_rows, coords=self.coords)
        d = dict(base.data())
        d["emb_c"] = d["emb_c"].copy()
        nan_cols = np.asarray(sorted(m.get("nan_cols", ())), np.int64)
        d["emb_c"][nan_cols] = np.nan
        sign = np.where(np.isin(d["coord"], P.FALLING), -1.0, 1.0)[d["dial_of"]]
        thr_score = np.full(self.Q, np.nan)
        emb_t = np.zeros((self.Q, self.H), np.float32)
        assert len(m["thr"]) == self.Q
        for q, (kind, v) in enumerate(m["thr"]):
            if kind == "level":
                thr_score[q] = sign[q] * P.lev(v) + 0.0
                emb_t[q, d["coord"][d["dial_of"][q]]] = P.lev(v)
            else:
                thr_score[q] = CONST_SCORE[v]
        skip = m.get("skip")
        if skip is not None:
            skip = np.asarray(skip, np.int32).reshape(self.Q, -1)
            assert skip.shape[1] <= MAX_SKIP
        d.update(thr_spec=m["thr"], thr_score=thr_score, emb_t=emb_t, skip=skip, nan_cols=nan_cols)
        return d


def present(case, d):
    """bool [Q, C] on the host: the candidate row is not NaN, the query's mask bit is clear, idx_base + column is none of the
    query's skipped columns"""
    live = np.ones((case.Q, case.C), bool)
    live[:, d["nan_cols"]] = False
    if d["mask"] is not None:
        live &= ~d["mask"][d["dial_of"]]
    if d["skip"] is not None:
        col = case.idx_base + np.arange(case.C)
        for j in range(d["skip"].shape[1]):
            live &= col[None, :] != d["skip"][:, j:j + 1]
    return live


def expected(case, d):
    """(above [Q], equal [Q]) int64 from the levels alone: scores compared with the score the threshold stands for (a NaN one
    counts nothing), plus the incoming counts.  Rows of ``nan_rows`` queries are not the host's to say (the relu drops the
    NaN: whatever rank_scores writes for them is the reference): they read -1."""
    live = present(case, d)
    S = d["S"][d["dial_of"]]
    t = d["thr_score"][:, None]
    with np.errstate(invalid="ignore"):
        above, equal = (live & (S > t)).sum(axis=1), (live & (S == t)).sum(axis=1)
    if case.incoming is not None:
        above, equal = above + case.incoming[0], equal + case.incoming[1]
    for q in case.nan_rows:
        above[q] = equal[q] = -1
    return above.astype(np.int64), equal.astype(np.int64)


def brute_force(case, d):
    """the same counts the slow way, in the PROBABILITY domain: float64 sigmoids, one pair at a time"""
    above, equal = np.zeros(case.Q, np.int64), np.zeros(case.Q, np.int64)
    sig = lambda s: 1.0 / (1.0 + np.exp(-s))
    nan_cols = set(d["nan_cols"].tolist())
    for q in range(case.Q):
        if q in case.nan_rows:
            above[q] = equal[q] = -1
            continue
        t = d["thr_score"][q]
        skipped = set() if d["skip"] is None else set(int(x) for x in d["skip"][q])
        for c in range(case.C):
            if c in nan_cols or (d["mask"] is not None and d["mask"][d["dial_of"][q], c]):
                continue
            if case.idx_base + c in skipped or np.isnan(t):
                continue
            p, pt = sig(d["S"][d["dial_of"][q], c]), sig(t)
            above[q] += p > pt
            equal[q] += p == pt
        if case.incoming is not None:
            above[q] += case.incoming[0][q]
            equal[q] += case.incoming[1][q]
    return above, equal


def pack_bits(mask):
    """uint32 [Q, ceil(C / 32)] absent bits of a bool [Q, C]"""
    Q, C_ = mask.shape
    W = (C_ + 31) // 32
    padded = np.zeros((Q, W * 32), bool)
    padded[:, :C_] = mask
    return (padded.reshape(Q, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.RandomState(np.array(seed, np.int64) % (2 ** 31))


CASES = []


def _add(*a, **kw):
    CASES.append(CountCase(*a, **kw))


def _few_levels(Q, C_, seed, levels=5, thr=None):
    """every query on its own dial (the second one falling), levels 1 .. ``levels``: many columns equal to the threshold, level 3"""
    def make():
        u = np.stack([P.lev(_rng(Q, C_, q, seed).randint(1, levels + 1, C_)) for q in range(Q)]) if C_ > 0 else np.zeros((Q, 0))
        return dict(u=u, falling=(1,) if Q > 1 else (), thr=thr or [("level", 3)] * Q)
    return make


# 1. the query tile of 4 and a ragged last tile x the step of 128 columns and a wave's 32
for _Q in (1, 4, 5, 9):
    for _C in (0, 1, 31, 32, 33, 127, 128, 129):
        _add("tiles-Q%d-C%d" % (_Q, _C), _Q, _C, _few_levels(_Q, _C, 1), reach=dict(q_tiles=(_Q + 3) // 4, n_spans=1, n_slabs=1))

# 2. two spans under the recommended workspace; slabs of 32 rows
_SPAN_C = 1500
_sl, _nsl, SPAN_COLS, _ns = plan_of(5, _SPAN_C)
assert _ns == 2 and SPAN_COLS == 768
_add("spans2-C1500", 5, _SPAN_C, _few_levels(5, _SPAN_C, 2), reach=dict(n_spans=2, span_cols=SPAN_COLS, n_slabs=1))
for _C in (33, 65, 100):
    _add("slab32-C%d" % _C, 5, _C, _few_levels(5, _C, 3), ws_rows=32, reach=dict(slab_rows=32, n_slabs=(_C + 31) // 32))

# 3. the RK_HC chunk seam: the dial of query 3 on the last coordinate
for _H in (20, 1024, 1028):
    _add("width-H%d" % _H, 5, 200, _few_levels(5, 200, 4), H=_H, coords={3: _H - 1} if _H > 20 else None, reach=dict(h_chunks=(_H + 1023) // 1024))

# 4. thresholds: everything equal; 1.0f; +-0.0f on falling dials; 0.5f; NaN; one of each kind in a tile
def _all_equal(Q, C_):
    def make():
        return dict(u=np.full((Q, C_), P.lev(7)), falling=(1,), thr=[("level", 7)] * Q)
    return make


def _ones(Q, C_):
    def make():
        u = np.stack([P.lev(_rng(Q, C_, q, 5).randint(1, P.MAX_LEVEL, C_)) for q in range(Q)])
        for q in range(Q):
            u[q, _rng(q, 6).choice(C_, 10 + q, replace=False)] = P.U_ONE
        return dict(u=u, thr=[("const", "one")] * Q)
    return make


def _zeros(Q, C_, name):
    def make():
        u = np.full((2, C_), P.U_ZERO)
        for dial in range(2):
            cols = _rng(C_, dial, 7).choice(C_, 20 + dial, replace=False)
            u[dial, cols] = P.lev(_rng(dial, 8).randint(0, P.MAX_LEVEL, len(cols)))
        return dict(u=u, falling=(0, 1), thr=[("const", name)] * Q)
    return make


_add("thr-all-equal", 5, 300, _all_equal(5, 300))
_add("thr-one", 5, 300, _ones(5, 300))
_add("thr-zero", 4, 300, _zeros(4, 300, "zero"), B=256.0)
_add("thr-negzero", 4, 300, _zeros(4, 300, "negzero"), B=256.0)
_add("thr-nan-and-half", 6, 300, _few_levels(6, 300, 9, thr=[("const", "nan"), ("level", 2), ("const", "half"), ("const", "nan"),
                                                             ("const", "one"), ("level", 5)]))

# 5. NaN candidate rows at the seams of a wave, a step, a span and the last column, and elsewhere; a NaN query row
def _with(base_make, **extra):
    def make():
        d = dict(base_make())
        d.update({k: (v() if callable(v) else v) for k, v in extra.items()})
        return d
    return make


_add("nan-cols-seams", 5, _SPAN_C, _with(_few_levels(5, _SPAN_C, 10), nan_cols=(0, 31, 32, 127, 128, 500, SPAN_COLS - 1, SPAN_COLS,
                                                                               _SPAN_C - 1)), reach=dict(n_spans=2))
_add("nan-cols-slab32", 5, 100, _with(_few_levels(5, 100, 11), nan_cols=(31, 32, 63, 64, 70, 99)), ws_rows=32, reach=dict(n_slabs=4))
_add("nan-query-row", 5, 300, _few_levels(5, 300, 12), nan_rows=(2,))

# 6. skips: none, 1, 2 and 4 per query, at the first and last column of a step, a span and a slab, -1 entries, and a column
# outside the call
def _skips(Q, n, cols, base=0):
    def make():
        if n == 0:
            return None
        s = np.full((Q, n), -1, np.int64)
        for q in range(Q):
            for j in range(n):
                s[q, j] = base + cols[(q * n + j) % len(cols)]
        if n > 1:
            s[Q - 1, n - 1] = -1
        return s
    return make


_SEAMS = (0, _SPAN_C - 1, _SPAN_C + 5, SPAN_COLS - 1, SPAN_COLS, 127, 128, 255, 256)
for _n in (0, 1, 2, 4):
    _add("skip%d-span-seams" % _n, 5, _SPAN_C, _with(_few_levels(5, _SPAN_C, 13), skip=_skips(5, _n, _SEAMS)), reach=dict(n_spans=2))
    _add("skip%d-slab32-seams" % _n, 5, 100, _with(_few_levels(5, 100, 14), skip=_skips(5, _n, (0, 99, 4000, 31, 32, 63, 64, 95, 96, 100))),
         ws_rows=32, reach=dict(n_slabs=4))

# 7. absent bits at columns 0, 31, 32, 63 and C - 1; a query with every column absent; bits beside skips
def _mask(Q, C_, cols, all_gone=None):
    def make():
        m = np.zeros((Q, C_), bool)
        m[:, [c for c in cols if c < C_]] = True
        m[np.arange(Q) % 2 == 1, 5 % max(C_, 1)] = True            # (rows differ: every query tests its own row of bits)
        if all_gone is not None:
            m[all_gone] = True
        return m
    return make


for _C in (64, 100, 129):
    _add("bits-C%d" % _C, 5, _C, _with(_few_levels(5, _C, 15), mask=_mask(5, _C, (0, 31, 32, 63, _C - 1), all_gone=3)))
_add("bits-spans2", 5, _SPAN_C, _with(_few_levels(5, _SPAN_C, 16), mask=_mask(5, _SPAN_C, (0, 31, 32, 63, SPAN_COLS - 1, SPAN_COLS,
                                                                                           _SPAN_C - 1), all_gone=1)), reach=dict(n_spans=2))
_add("bits-slab32-with-skips", 5, 100, _with(_few_levels(5, 100, 17), mask=_mask(5, 100, (0, 31, 32, 63, 99)),
                                             skip=_skips(5, 2, (1, 31, 33, 64, 98, 99))), ws_rows=32, reach=dict(n_slabs=4))

# 8. the pool in three pieces, in two orders, under accumulate with idx_base set, from non-zero incoming counts -- with bits,
# skips (global columns) and a NaN row, so that every local / global offset counts
_PIECES = [(0, 100), (100, 133), (133, 300)]
_INC = (np.array([3, 0, 7, 1, 1000000]), np.array([0, 5, 2, 9, 12]))
for _name, _order in (("forward", (0, 1, 2)), ("shuffled", (2, 0, 1))):
    _add("pieces-%s" % _name, 5, 300,
         _with(_few_levels(5, 300, 18), mask=_mask(5, 300, (0, 99, 100, 132, 133, 299)), nan_cols=(101, 200),
               skip=_skips(5, 2, (50, 99, 100, 133, 250, 299), base=7000)),
         pieces=[_PIECES[i] for i in _order], idx_base=7000, incoming=_INC)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
