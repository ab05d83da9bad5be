"""Shared by tests/test_topk_exact_cpu.py and tests/test_topk_exact_gpu.py (own code): a MergeLayer whose scores the test
dials, the table of planted cases with the seam each one names, the expectation computed on the host alone, and a host model
of the kernel's running list that records where every insert lands.

The scorer: fc1.weight = [I | I], fc1.bias = 0, fc2.weight = +1 on the rising coordinates and -1 on the falling ones
(FALLING), fc2.bias = 0.  A query's embedding is -B everywhere and 0 at its own coordinate, so relu leaves that coordinate
alone: pair (q, c) scores exactly s = +-emb_c[c, coord(q)], every other addend is an exact zero, and no summation order
matters.  A column of emb_c is a DIAL; queries on different dials have unrelated orders.  Planted values are
u = level * LEVEL_U with 0 <= level <= MAX_LEVEL (u <= 6: float32's sigmoid is strictly increasing over 16 384 equally spaced
values of [0, 6], and a level is 15 of those apart), or one of the special values U_ONE (sigmoid = 1.0f), U_ZERO on a falling
dial (sigmoid = +0.0f) and 0 (0.5f).  B exceeds every planted value of its case (64, or 256 where U_ZERO = 200 is planted)."""
import functools

import numpy as np

FALLING = (18, 19)                 # the coordinates with fc2.weight = -1 (every planted width is >= 20)
LEVEL_U = 15 * 6.0 / 16384         # u of level 1: level * 45 * 2^-13, exact in float32 for every level <= MAX_LEVEL
MAX_LEVEL = 16384 // 15            # 1092 >= 4 K + 2 = 1026
U_ONE, U_ZERO = 40.0, 200.0
STEP = {True: 128, False: 32}      # columns a workgroup takes per step: shared pool, indexed
IDX_BASE_ACC = 5000                # idx_base of the cases with an incoming list


def lev(x):
    """u of integer levels (float64, exact in float32)"""
    x = np.asarray(x, np.float64)
    assert (x >= 0).all() and (x <= MAX_LEVEL).all()
    return x * LEVEL_U


def scorer_weights(H):
    """(fc1.weight [H, 2H], fc1.bias [H], fc2.weight [1, H], fc2.bias [1]) of the dialled scorer, float32"""
    eye = np.eye(H, dtype=np.float32)
    w2 = np.ones((1, H), np.float32)
    w2[0, list(FALLING)] = -1.0
    return np.concatenate([eye, eye], axis=1), np.zeros(H, np.float32), w2, np.zeros(1, np.float32)


class Case:
    """One planted input.  ``make()`` -> dict(u [D, C] float64 (NaN: an absent index column), falling: the falling dials,
    mask [D, C] bool or None (absent bits), incoming: dict(idx [D, K], s [D, K]) or None).  Query q sits on dial
    ``q % D``.  ``reach``: the plan fields the id names.  ``ws_rows``: slab rows the workspace is cut down to (None: the
    recommended size).  ``pieces``: [(begin, end), ...] the pool is given in, in that order (accumulate)."""

    def __init__(self, id, K, shared, Q, C, make, H=20, ws_rows=None, reach=None, positions=False, B=64.0, pieces=None,
                 nan_rows=(), coords=None, identity=False):
        self.id, self.K, self.shared, self.Q, self.C, self.make, self.H = id, K, shared, Q, C, make, H
        self.ws_rows, self.reach, self.positions, self.B, self.pieces = ws_rows, dict(reach or {}), positions, B, pieces
        self.nan_rows, self.coords, self.identity = tuple(nan_rows), coords, identity
        self.Nc = C                    # shared: the pool; indexed: one row of emb_c per index column

    def __repr__(self):
        return self.id

    def workspace_bytes(self, capi, Q=None, Nc=None):
        import ctypes as C_
        Q = self.Q if Q is None else Q
        Nc = self.Nc if Nc is None else Nc
        ws = capi.lib().zt_affinity_topk_workspace_bytes
        if self.ws_rows is None:
            return int(ws(C_.c_int64(Q), C_.c_int64(Nc), C_.c_int32(self.H), C_.c_int32(self.K)))
        least = int(ws(C_.c_int64(Q), C_.c_int64(32), C_.c_int32(self.H), C_.c_int32(self.K)))
        return least + (self.ws_rows - 32) * self.H * 4

    def plan(self, capi):
        return capi.topk_plan(self.Q, self.Nc, self.C, self.H, self.K, not self.shared, self.workspace_bytes(capi))

    @functools.lru_cache(maxsize=None)
    def data(self):
        """dict: u, S [D, C] (signed scores, NaN absent), coord [D], emb_q [Q, H], emb_c [Nc, H], idx [Q, C] or None,
        mask [D, C] or None, bits [Q, W] uint32 or None, incoming, D"""
        d = dict(self.make())
        u = np.asarray(d["u"], np.float64)
        D, C_ = u.shape
        assert C_ == self.C and D <= self.Q and np.nanmax(u, initial=0.0) < self.B and not (u < 0).any()
        assert self.shared or self.C == self.Nc
        falling = set(d.get("falling", ()))
        rising_coords = [h for h in range(self.H) if h not in FALLING]
        fall_coords = list(FALLING)
        coord = np.zeros(D, np.int64)
        for dial in range(D):
            if self.coords and dial in self.coords:
                coord[dial] = self.coords[dial]
                assert (coord[dial] in FALLING) == (dial in falling)
            else:
                coord[dial] = fall_coords.pop(0) if dial in falling else rising_coords.pop(0)
        assert len(set(coord.tolist())) == D
        sign = np.where(np.isin(coord, FALLING), -1.0, 1.0)
        S = u * sign[:, None] + 0.0                                   # (-0.0 -> +0.0: one zero)
        dial_of = np.arange(self.Q) % D
        emb_q = np.full((self.Q, self.H), -self.B, np.float32)
        emb_q[np.arange(self.Q), coord[dial_of]] = 0.0
        for q in self.nan_rows:
            emb_q[q] = np.nan
        emb_c = np.zeros((self.Nc, self.H), np.float32)
        idx = None
        if self.shared:
            assert not np.isnan(u).any()
            emb_c[:, coord] = u.T
        else:
            rng = np.random.RandomState(len(self.id) + 7 * self.K + self.C)
            idx_d = np.empty((D, C_), np.int32)
            for dial in range(D):
                rows = np.arange(C_) if self.identity else rng.permutation(C_)     # a dial's own rows of emb_c
                live = ~np.isnan(u[dial])
                emb_c[rows[live], coord[dial]] = u[dial, live]
                idx_d[dial] = np.where(live, rows, -1)
            idx = idx_d[dial_of]
        fin = ~np.isnan(u)
        assert np.array_equal(u[fin].astype(np.float32).astype(np.float64), u[fin])      # the planted values are exact in float32
        mask = d.get("mask")
        bits = None
        if mask is not None:
            mask = np.asarray(mask, bool)
            W = (C_ + 31) // 32
            padded = np.zeros((D, W * 32), bool)
            padded[:, :C_] = mask
            words = (padded.reshape(D, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
            bits = words[dial_of]
        return dict(u=u, S=S, coord=coord, dial_of=dial_of, emb_q=emb_q, emb_c=emb_c, idx=idx, mask=mask, bits=bits,
                    incoming=d.get("incoming"), D=D)


def expected(S, K, mask=None, idx_base=0, incoming=None):
    """(idx [D, K] int64, s [D, K] float64) on the host alone: per dial the K present columns by lexsort(-score, column) --
    a score is +-level, so this is lexsort(-level, column) --, -1 / NaN behind.  Present: S is not NaN and the mask bit is
    clear.  ``incoming`` (idx [D, K], s [D, K]): entries with idx >= 0 and a score that is not NaN compete under their own
    indices."""
    D, C_ = S.shape
    out_i = np.full((D, K), -1, np.int64)
    out_s = np.full((D, K), np.nan)
    for dial in range(D):
        live = ~np.isnan(S[dial])
        if mask is not None:
            live &= ~mask[dial]
        cols = np.nonzero(live)[0]
        ids, sc = cols + idx_base, S[dial, cols]
        if incoming is not None:
            ok = (incoming["idx"][dial] >= 0) & ~np.isnan(incoming["s"][dial])
            ids = np.concatenate([ids, incoming["idx"][dial][ok]])
            sc = np.concatenate([sc, incoming["s"][dial][ok]])
            assert len(set(ids.tolist())) == len(ids)
        order = np.lexsort((ids, -sc))[:K]
        out_i[dial, :len(order)] = ids[order]
        out_s[dial, :len(order)] = sc[order]
    return out_i, out_s


# ---- the host model of the kernel's list ----------------------------------------------------------------------------------
class ModelList:
    """A descending list of K slots fed batches of keys (score, index) the way tk_offer is: one test of the whole batch
    against the K-th key, then the survivors one by one in batch order, each tested again.  ``log``: the position of every
    insert."""

    def __init__(self, K):
        self.K, self.keys, self.log = K, [], []            # keys ascending in (-score, index) = descending list order

    def offer(self, batch):
        import bisect
        kth = self.keys[self.K - 1] if len(self.keys) >= self.K else None
        for key in [k for k in batch if k is not None and (kth is None or k < kth)]:
            kth = self.keys[self.K - 1] if len(self.keys) >= self.K else None
            if kth is None or key < kth:
                pos = bisect.bisect_left(self.keys, key)
                self.keys.insert(pos, key)
                del self.keys[self.K:]
                self.log.append(pos)


def _chunks(keys, n=64):
    return [keys[i:i + n] for i in range(0, len(keys), n)]


def model_query(S_row, mask_row, K, shared, span_cols, n_spans, incoming=None, idx_base=0):
    """One query through the model of one slab: (result keys, dict stage -> list of insert positions; "wave<w>" is wave w's
    list in the pair kernel (shared form), "pairs" the indexed form's, "wave_merge" the merge of the four waves' lists and
    "merge" the merge kernel's)."""
    C_ = len(S_row)

    def key(c):
        if c >= C_ or np.isnan(S_row[c]) or (mask_row is not None and mask_row[c]):
            return None
        return (-float(S_row[c]), c + idx_base)

    stages = {}
    span_lists = []
    for span in range(n_spans):
        lo, hi = min(C_, span * span_cols), min(C_, (span + 1) * span_cols)
        if shared:
            waves = [ModelList(K) for _ in range(4)]
            for t0 in range(lo, hi, 128):
                for w in range(4):
                    waves[w].offer([key(c) if c < hi else None for c in range(t0 + 32 * w, t0 + 32 * w + 32)])
            for w in range(4):
                stages.setdefault("wave%d" % w, []).extend(waves[w].log)
            final = ModelList(K)
            final.keys = list(waves[0].keys)
            for v in range(1, 4):
                for ch in _chunks(waves[v].keys + [None] * (-len(waves[v].keys) % 64)):
                    final.offer(ch)
            stages.setdefault("wave_merge", []).extend(final.log)
            span_lists.append(final.keys)
        else:
            lst = ModelList(K)
            for t0 in range(lo, hi, 32):
                lst.offer([key(c) if c < hi else None for c in range(t0, t0 + 32)])
            stages.setdefault("pairs", []).extend(lst.log)
            span_lists.append(lst.keys)
    merged = ModelList(K)
    if incoming is not None:
        inc = [None if (i < 0 or np.isnan(s)) else (-float(s), int(i)) for i, s in zip(*incoming)]
        for ch in _chunks(inc):
            merged.offer(ch)
    flat = []
    for keys in span_lists:
        flat.extend(keys + [None] * (K - len(keys)))
    for ch in _chunks(flat):
        merged.offer(ch)
    stages["merge"] = merged.log
    return merged.keys, stages


# ---- patterns -----------------------------------------------------------------------------------------------------------
def ladder_levels(K, n=None):
    """columns 0 .. K-1 carry levels 4K, 4K-4, .., 4 and columns K .. 2K-1 levels 6, 10, .., 4K+2: key K + j lands at exactly
    position K-1-j.  ``n`` < 2K cuts the tail off."""
    lv = np.concatenate([4 * K - 4 * np.arange(K), 6 + 4 * np.arange(K)])
    return lv[:2 * K if n is None else n]


def _rng(*seed):
    return np.random.RandomState(np.array(seed, np.int64) % (2 ** 31))


CASES = []


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


# 1. every list position: the ladder
LADDER_K = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)


def ladder_shape(K, shared):
    """(C, columns of the ladder): shared -- the columns wave w sees, 32 of every 128, in a pool that is one span (below 2048
    columns, so waves 0..2 see 512); indexed -- 2K index columns, 511 at K = 256 (512 would be two spans)"""
    if shared:
        return min(128 * ((2 * K + 31) // 32), 2047), 2 * K
    return min(2 * K, 511), min(2 * K, 511)


def wave_columns(w, n):
    j = np.arange(n)
    return 128 * (j // 32) + 32 * w + j % 32


def _ladder_make(K, shared, Q=5):
    def make():
        C_, n = ladder_shape(K, shared)
        u = np.zeros((Q, C_))
        for q in range(Q):
            cols = wave_columns(q % 3, n) if shared else np.arange(n)
            u[q, cols] = lev(ladder_levels(K, n))
        return dict(u=u)
    return make


for _K in LADDER_K:
    for _sh in (True, False):
        _add("ladder-%s-K%d" % ("shared" if _sh else "indexed", _K), _K, _sh, 5, ladder_shape(_K, _sh)[0],
             _ladder_make(_K, _sh), positions=True, reach=dict(n_spans=1, n_slabs=1, form=1 if _K <= 64 else 2))

# 2. orders: one dial each for ascending, descending, all equal, two levels with K-1 / K / K+1 members of the upper one
ORDER_K = (1, 64, 65, 128, 129, 256)


def _orders_make(K, C_):
    def make():
        u = np.zeros((6, C_))
        u[0] = lev(1 + np.arange(C_))
        u[1] = lev(C_ - np.arange(C_))
        u[2] = lev(np.full(C_, 77))
        for j, m in enumerate((K - 1, K, K + 1)):
            lv = np.full(C_, 5)
            lv[C_ - min(m, C_):] = 9                     # the upper level arrives last
            u[3 + j] = lev(lv)
        return dict(u=u)
    return make


for _K in ORDER_K:
    for _C in (_K - 1, _K, _K + 1, 2 * _K + 1, 1000):
        for _sh in (True, False):
            _add("orders-%s-K%d-C%d" % ("shared" if _sh else "indexed", _K, _C), _K, _sh, 6, _C, _orders_make(_K, _C))

# 3. ties at the cut across a boundary b: K-2 columns above level L, level L at b-2 .. b+1, everything else below
TIE_K = (10, 65, 256)


def _tie_make(K, C_, b, Q=5, masked_cols=None):
    def make():
        u = np.zeros((Q, C_))
        mask = None if masked_cols is None else np.zeros((Q, C_), bool)
        for q in range(Q):
            rng = _rng(K, C_, b, q)
            lv = rng.randint(1, 400, C_)
            tie = [b - 2, b - 1, b, b + 1]
            rest = np.setdiff1d(np.arange(C_), tie)
            lv[rng.choice(rest, K - 2, replace=False)] = rng.randint(600, 1000, K - 2)
            lv[tie] = 500
            u[q] = lev(lv)
            if mask is not None:
                mask[q, [c for c in masked_cols if c < C_]] = True
        return dict(u=u, mask=mask)
    return make


def _plan_of(Q, Nc, C_, K, shared, H=20):
    """the spans of the recommended workspace, restated: test_topk_exact_cpu.py holds every case's ``reach`` against
    _capi.topk_plan"""
    q_tiles = (Q + 3) // 4
    max_spans = max(1, (2048 + q_tiles - 1) // q_tiles)
    step = STEP[shared]
    n = min(max_spans, max(1, C_ // (step * 8)))
    span_cols = ((C_ + n - 1) // n + step - 1) // step * step
    return span_cols, max(1, (C_ + span_cols - 1) // span_cols)


for _K in TIE_K:
    _C = max(2 * _K + 100, 300)
    for _sh in (True, False):
        _add("tie-block32-%s-K%d" % ("shared" if _sh else "indexed", _K), _K, _sh, 5, _C, _tie_make(_K, _C, 32))
    _add("tie-step128-shared-K%d" % _K, _K, True, 5, _C, _tie_make(_K, _C, 128))
    _sc, _ns = _plan_of(5, 2500, 2500, _K, True)
    _add("tie-span-shared-K%d" % _K, _K, True, 5, 2500, _tie_make(_K, 2500, _sc), reach=dict(n_spans=2, span_cols=_sc))
    _sc, _ns = _plan_of(5, 700, 700, _K, False)
    _add("tie-span-indexed-K%d" % _K, _K, False, 5, 700, _tie_make(_K, 700, _sc), reach=dict(n_spans=2, span_cols=_sc))
    for _rows in (32, 128):
        for _sh in (True, False):
            _add("tie-slab%d-%s-K%d" % (_rows, "shared" if _sh else "indexed", _K), _K, _sh, 5, _C,
                 _tie_make(_K, _C, 2 * _rows), ws_rows=_rows, identity=True,
                 reach=dict(slab_rows=_rows, n_slabs=(_C + _rows - 1) // _rows))
    _add("tie-piece-forward-K%d" % _K, _K, True, 5, _C, _tie_make(_K, _C, 100), pieces=[(0, 100), (100, _C)])
    _add("tie-piece-backward-K%d" % _K, _K, True, 5, _C, _tie_make(_K, _C, 100), pieces=[(100, _C), (0, 100)])

# 4. spans: the winners in the last span, and in the last (partial) step
def _span_make(K, C_, D, where, shared, Q):
    def make():
        span_cols, n_spans = _plan_of(Q, C_, C_, K, shared)
        u = np.zeros((D, C_))
        for dial in range(D):
            rng = _rng(K, C_, dial, len(where))
            lv = rng.randint(1, 500, C_)
            if where == "lastspan":
                lo = (n_spans - 1) * span_cols
            else:
                lo = (C_ - 1) // STEP[shared] * STEP[shared]          # the last step, partial where C is no multiple
            lv[lo:] = rng.randint(600, MAX_LEVEL, C_ - lo)
            u[dial] = lev(lv)
        return dict(u=u, falling=(D - 1,) if D > 1 else ())
    return make


SPANS = [  # (name, shared, Q, C, K, reach)
    ("indexed-Q1-C8192", False, 1, 8192, 256, dict(n_spans=32, span_cols=256)),
    ("indexed-C512", False, 5, 512, 65, dict(n_spans=2, span_cols=256)),
    ("indexed-C511", False, 5, 511, 65, dict(n_spans=1, span_cols=512)),
    ("shared-Nc2048", True, 5, 2048, 64, dict(n_spans=2, span_cols=1024)),
    ("shared-Nc2047", True, 5, 2047, 64, dict(n_spans=1, span_cols=2048)),
    ("shared-Nc4096", True, 5, 4096, 129, dict(n_spans=4, span_cols=1024)),
    ("shared-Nc2500-partial", True, 5, 2500, 100, dict(n_spans=2, span_cols=1280)),
    ("cap-indexed-Q4096-C1024", False, 4096, 1024, 10, dict(n_spans=2, span_cols=512, q_tiles=1024)),
    ("cap-shared-Q4096-Nc4096", True, 4096, 4096, 65, dict(n_spans=2, span_cols=2048, q_tiles=1024)),
]
for _name, _sh, _Q, _C, _K, _reach in SPANS:
    for _where in ("lastspan", "laststep"):
        _add("spans-%s-K%d-%s" % (_name, _K, _where), _K, _sh, _Q, _C, _span_make(_K, _C, min(_Q, 18), _where, _sh, _Q),
             reach=_reach)

# 5. query tiles: every query on its own dial and its own pattern
def _tiles_make(Q, C_, holes=False):
    def make():
        u = np.stack([lev(_rng(Q, C_, q).randint(0, MAX_LEVEL + 1, C_)) for q in range(Q)])
        if holes:                                           # absent index columns, a tenth of them
            u[_rng(Q, C_, 4).random_sample(u.shape) < 0.1] = np.nan
        return dict(u=u, falling=(1,) if Q > 1 else ())
    return make


for _Q in (1, 2, 3, 4, 5, 7, 8, 9):
    for _sh in (True, False):
        _add("tiles-%s-Q%d" % ("shared" if _sh else "indexed", _Q), 65, _sh, _Q, 300, _tiles_make(_Q, 300, not _sh),
             reach=dict(q_tiles=(_Q + 3) // 4))

# 6. extremes
def _ones_make(K, C_, Q=5):
    def make():
        u = np.zeros((Q, C_))
        for q in range(Q):
            rng = _rng(K, C_, q, 1)
            u[q] = lev(rng.randint(1, MAX_LEVEL, C_))
            u[q, rng.choice(C_, K + 5, replace=False)] = U_ONE
        return dict(u=u)
    return make


def _zeros_make(K, C_, n_above, Q=4):
    """every dial falling (two of them, the queries share them): n_above columns above +0.0f, the rest exactly +0.0f"""
    def make():
        u = np.full((2, C_), U_ZERO)
        for dial in range(2):
            rng = _rng(K, C_, dial, 2)
            cols = rng.choice(C_, min(n_above, C_), replace=False)
            u[dial, cols] = lev(rng.randint(0, MAX_LEVEL, len(cols)))
        return dict(u=u, falling=(0, 1))
    return make


for _sh in (True, False):
    _f = "shared" if _sh else "indexed"
    for _K in (10, 65):
        _add("extreme-ones-%s-K%d" % (_f, _K), _K, _sh, 5, 300, _ones_make(_K, 300))
    for _K in (10, 65, 256):
        _add("extreme-fewabovezero-%s-K%d" % (_f, _K), _K, _sh, 4, 300, _zeros_make(_K, 300, _K // 2), B=256.0)
        _add("extreme-allzero-%s-K%d" % (_f, _K), _K, _sh, 4, 300, _zeros_make(_K, 300, 0), B=256.0)
    _add("extreme-allzero-short-%s-K65" % _f, 65, _sh, 4, 40, _zeros_make(65, 40, 0), B=256.0)
    _add("extreme-nanquery-%s-K10" % _f, 10, _sh, 5, 300, _tiles_make(5, 300), nan_rows=(2,))
    _add("extreme-H1028-coord1027-%s-K65" % _f, 65, _sh, 5, 300, _tiles_make(5, 300), H=1028, coords={3: 1027})
    _add("extreme-H300-%s-K65" % _f, 65, _sh, 5, 300, _tiles_make(5, 300), H=300, coords={2: 299})

# 7. accumulate: an incoming list as include/zebra_amd.h specifies it -- index -1 an empty slot, indices outside
# [idx_base, idx_base + C) -- whose probabilities are bits of this pool's own (the score names them)
ACC_K = (64, 65, 129, 256)


def _acc_make(K, C_, kind, Q=5):
    def make():
        u = np.zeros((Q, C_))
        inc_i = np.full((Q, K), -1, np.int64)
        inc_s = np.full((Q, K), np.nan)
        for q in range(Q):
            rng = _rng(K, C_, q, 3)
            lv = rng.randint(1, 300, C_)                   # a few hundred levels over C columns: ties inside the pool too
            u[q] = lev(lv)
            if kind == "ones":
                u[q, rng.choice(C_, K // 2, replace=False)] = U_ONE
                inc_s[q] = U_ONE                           # a full list of 1.0f: half below the pool's indices, half above
                inc_i[q] = np.where(np.arange(K) % 2 == 0, np.arange(K), IDX_BASE_ACC + C_ + np.arange(K))
                continue
            # the pool's own best scores again (ties bit for bit), descending, under smaller or larger indices; every third
            # slot a hole, one entry with a NaN probability under an index that would otherwise win
            best = np.sort(u[q])[::-1][:K]
            slots = np.arange(K)
            inc_s[q] = best
            inc_i[q] = (slots if kind == "smaller" else IDX_BASE_ACC + C_ + slots)
            inc_i[q, slots % 3 == 1] = -1
            if K > 3:
                inc_s[q, 3] = np.nan
        return dict(u=u, incoming=dict(idx=inc_i, s=inc_s))
    return make


for _K in ACC_K:
    for _kind in ("smaller", "larger", "ones"):
        _add("accumulate-%s-shared-K%d" % (_kind, _K), _K, True, 5, 2 * _K + 40, _acc_make(_K, 2 * _K + 40, _kind))
    _add("accumulate-smaller-indexed-K%d" % _K, _K, False, 5, 2 * _K + 40, _acc_make(_K, 2 * _K + 40, "smaller"))

# 8. the masked form
MASK_K = (64, 65, 129, 256)


def _masked_winners(base_make, K):
    """the bits remove exactly the unmasked winners: the answer is ranks K .. 2K-1"""
    def make():
        d = dict(base_make())
        u = np.asarray(d["u"])
        win, _ = expected(u, K)                             # (rising dials only: the score is u)
        mask = np.zeros(u.shape, bool)
        for dial in range(u.shape[0]):
            mask[dial, win[dial][win[dial] >= 0]] = True
        d["mask"] = mask
        return d
    return make


for _K in MASK_K:
    for _sh in (True, False):
        _f = "shared" if _sh else "indexed"
        _C = ladder_shape(_K, _sh)[0]
        _add("masked-winners-ladder-%s-K%d" % (_f, _K), _K, _sh, 5, _C, _masked_winners(_ladder_make(_K, _sh), _K),
             reach=dict(n_spans=1))
        _C = max(2 * _K + 100, 300)
        _add("masked-bits31-32-last-tie-%s-K%d" % (_f, _K), _K, _sh, 5, _C, _tie_make(_K, _C, 32, masked_cols=(31, 32, _C - 1)))
        _add("masked-winners-tie-slab32-%s-K%d" % (_f, _K), _K, _sh, 5, _C, _masked_winners(_tie_make(_K, _C, 64), _K),
             ws_rows=32, identity=True, reach=dict(slab_rows=32, n_slabs=(_C + 31) // 32))

# 9. the last slot: the K-1 best in one list, the K-th best in another -- the only insert of the merge lands at position K-1
LASTSLOT_K = (2, 64, 65, 256)


def lastslot_wave_cols(K):
    """a pool that is one span in which wave 0 sees at least K - 1 + 32 columns"""
    return 128 * ((K + 30) // 32 + 1)


def _lastslot_make(K, C_, kind, shared, Q=5):
    def make():
        span_cols, n_spans = _plan_of(Q, C_, C_, K, shared)
        u = np.zeros((Q, C_))
        for q in range(Q):
            rng = _rng(K, C_, q, 5)
            lv = rng.randint(1, 400, C_)
            if kind == "wave":                             # wave 0's columns hold the K-1 best, wave 1 + q % 3 the K-th
                best = wave_columns(0, K - 1)
                mine = wave_columns(1 + q % 3, C_ // 4)
                last = mine[rng.randint(len(mine))]
            else:                                          # the first span holds the K-1 best, the last span the K-th
                best = rng.choice(span_cols, K - 1, replace=False)
                last = (n_spans - 1) * span_cols + rng.randint(C_ - (n_spans - 1) * span_cols)
            lv[best] = 600 + rng.permutation(K - 1)
            lv[last] = 500
            u[q] = lev(lv)
        return dict(u=u)
    return make


for _K in LASTSLOT_K:
    _C = lastslot_wave_cols(_K)
    _add("lastslot-wave-shared-K%d" % _K, _K, True, 5, _C, _lastslot_make(_K, _C, "wave", True), reach=dict(n_spans=1))
    _add("lastslot-span-shared-K%d" % _K, _K, True, 5, 2500, _lastslot_make(_K, 2500, "span", True), reach=dict(n_spans=2))
    _add("lastslot-span-indexed-K%d" % _K, _K, False, 5, 700, _lastslot_make(_K, 700, "span", False), reach=dict(n_spans=2))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
