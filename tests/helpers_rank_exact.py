"""The ranking step's scorer held to EXACT sums (tests/test_rank_train_exact_cpu.py, tests/test_rank_train_exact_gpu.py).

Exact inputs.  Embeddings in {-1, 0, 1}; each row of fc1.weight with min(8, H) entries of +-1 in its left half and as many in
its right half, zero elsewhere; fc1.bias in {-1, 0, 1}; fc2.weight in {-2, -1, 1, 2}; fc2.bias an integer; dl in
{-2, -1, 1, 2}.  Every product and every partial sum of the scorer and of its six gradients is then an integer far below 2^24
(the CPU file shows it for every case from the composition on absolute values), so float32 cannot round in ANY order of
association: the kernels' results must have the bits of the float64 composition rounded once, and a dropped, duplicated or
misattributed term moves a sum by a non-zero integer.  |z| <= 17 with many units at z = 0 exactly: the mask convention
(z > 0, the gradient is 0 at 0) is pinned by every case.

The index builder (planted_index) PLANTS the number of pairs that name each row of emb_c; the cases (CASES) each cross one seam
of csrc/rank_train.hip's tiling and say so in their id; seams() reads the tile constants from the sources, and the CPU file
holds every id to them.

The bound of the random-input family (error_bound).  With u = 2^-24 and A the composition evaluated on the absolute values
of every input (an upper bound of the sum of |terms| of each output element), an output whose every term passes through at
most L float32 roundings -- in any order of association, the kernels' or torch's -- is within L u A of the exact value (to
first order in u; L u < 1e-3 here), plus one float32 ulp of the reference for the reference's own rounding.  L, counted
from the kernels' headers:
  logit[q][c]    a term emb[k] W[h][k] w2[h]: its product and at most H - 1 additions in zt_gemm_f32 (H), + b1 and + P_c
                 (rk_query_bias, rk_pair_z: 2), the product with w2 (1), at most H additions on the way through the lane's
                 accumulator, rk_fold16 and the addition of b2 (H + 1; the kernel's own chain is H / 16 + 5)  -> 2H + 4
  dP[.][h]       a term dl w2[h]: its product (1) and one addition per pair of the sum, C for a query, n_r for row r of emb_c
  d_emb_q[q][k]  a term dP_q[q][h] W_a[h][k]: dP's roundings (C + 1), the product (1), at most H additions  -> H + C + 2
  d_emb_c[r][k]  likewise                                                                                     -> H + n_r + 2
(the ReLU mask is a comparison, not a rounding: margin_ok keeps every float64 z of a live pair 1e-5 max(1, max|z|) from 0,
so that float32 takes the float64 mask)."""
import functools
import os
import re

import numpy as np
import torch

from helpers_rank_train import NEG_INF, composed_scorer, merge_layer, scorer_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("logit", "d_emb_q", "d_emb_c", "d_fc1_w", "d_fc1_b", "d_fc2_w", "d_fc2_b")
U = 2.0 ** -24
# the margin condition asks that NO unit of a live pair lies within 1e-5 max(1, max|z|) of zero.  z of scorer_inputs is about
# N(0, 0.8^2) with max|z| near 4: a unit lies inside with probability 4e-5, so a draw of n units passes with exp(-4e-5 n) --
# one seed in fifty at 1e5 units, none at the 1.3e6 of (9, 33, 4352) or the 6e6 of the workload.  Cases above this count keep
# the exact comparison only.
MARGIN_MAX_UNITS = 65536
MARGIN_TRIES = 50


def seams():
    """The tile constants of csrc/rank_pair.hpp and csrc/rank_train.hip, read from the sources"""
    vals = {}
    for name in ("common.hpp", "rank_pair.hpp", "rank_train.hip"):
        text = open(os.path.join(ROOT, "zebra_amd", "csrc", name)).read()
        for decl in re.findall(r"constexpr int ([^;]+);", text):
            for item in decl.split(","):
                m = re.fullmatch(r"\s*(\w+)\s*=\s*([\w\s()*/+-]+)", item)
                if m and re.fullmatch(r"(WAVE|R[KT]_\w+|RANK_M\w+)", m.group(1)):
                    try:
                        vals[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, dict(vals)))
                    except NameError:
                        pass
    return vals


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def exact_inputs(Q, C_, H, Nc, seed):
    """(emb_q, emb_c, dl float32 tensors, [fc1.weight, fc1.bias, fc2.weight, fc2.bias] float32 numpy) of small integers"""
    rng = np.random.RandomState(seed)
    emb_q = rng.randint(-1, 2, (Q, H)).astype(np.float32)
    emb_c = rng.randint(-1, 2, (Nc, H)).astype(np.float32)
    w1 = np.zeros((H, 2 * H), np.float32)
    n = min(8, H)
    for half in (0, 1):                                                # n distinct columns per row: sorted draws, spread apart
        pos = np.sort(rng.randint(0, H - n + 1, (H, n)), axis=1) + np.arange(n)
        w1[np.arange(H)[:, None], half * H + pos] = rng.choice([-1.0, 1.0], (H, n))
    b1 = rng.randint(-1, 2, H).astype(np.float32)
    w2 = rng.choice([-2.0, -1.0, 1.0, 2.0], (1, H)).astype(np.float32)
    b2 = rng.randint(-3, 4, 1).astype(np.float32)
    dl = rng.choice([-2.0, -1.0, 1.0, 2.0], (Q, C_)).astype(np.float32)
    return torch.from_numpy(emb_q), torch.from_numpy(emb_c), torch.from_numpy(dl), [w1, b1, w2, b2]


def planted_index(Q, C_, n_r, seed, closed=None, pins=()):
    """cand_idx int32 [Q, C] in which row r of emb_c is named exactly n_r[r] times and every other cell is -1.  ``pins``:
    (row, pair ids) placed first; the rest of each row's names go to a seeded permutation of the cells that are left and
    not ``closed`` (bool [Q, C]: cells that stay -1)."""
    flat = np.full(Q * C_, -1, np.int32)
    free = np.ones(Q * C_, bool) if closed is None else ~np.asarray(closed, bool).reshape(-1)
    left = [int(n) for n in n_r]
    for r, ids in pins:
        for p in ids:
            assert free[p] and flat[p] == -1
            flat[p] = r
            left[r] -= 1
    assert min(left + [0]) >= 0
    cells = np.random.RandomState(seed).permutation(np.flatnonzero(free & (flat == -1)))
    rows = np.repeat(np.arange(len(left)), left)
    assert rows.size <= cells.size, "more names than cells"
    flat[cells[:rows.size]] = rows
    return torch.from_numpy(flat.reshape(Q, C_))


def spread(total, Nc, unnamed=()):
    """``total`` names over the Nc rows, as evenly as integers allow, none for the rows in ``unnamed``"""
    rows = [r for r in range(Nc) if r not in unnamed]
    n = [0] * Nc
    for i, r in enumerate(rows):
        n[r] = total // len(rows) + (1 if i < total % len(rows) else 0)
    return n


class Case:
    """One exact case: Q queries, C columns, width H, Nc rows of emb_c; ``n_r`` None: no index (C == Nc), else the planted
    pair counts; ``closed`` / ``pins`` as planted_index takes them; ``dl_nan``: NaN in dl at the absent pairs."""

    def __init__(self, id, Q, C_, H, Nc=None, n_r=None, closed=None, pins=(), dl_nan=False):
        self.id, self.Q, self.C, self.H = id, Q, C_, H
        self.Nc = C_ if Nc is None else Nc
        self.n_r, self.closed, self.pins, self.dl_nan = n_r, closed, pins, dl_nan
        assert n_r is not None or self.Nc == C_
        assert n_r is None or len(n_r) == self.Nc
        self.seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(id)) % 100000

    def __repr__(self):
        return self.id

    @property
    def indexed(self):
        return self.n_r is not None

    def index(self):
        if self.n_r is None:
            return None
        closed = None if self.closed is None else self.closed(self.Q, self.C)
        return planted_index(self.Q, self.C, self.n_r, self.seed, closed, self.pins)

    def pair_counts(self):
        """pairs that name each row of emb_c"""
        return [self.Q] * self.Nc if self.n_r is None else list(self.n_r)

    def live_units(self):
        return sum(self.pair_counts()) * self.H

    def exact(self):
        """(emb_q, emb_c, cand_idx, dl, weights)"""
        emb_q, emb_c, dl, wts = exact_inputs(self.Q, self.C, self.H, self.Nc, self.seed)
        return emb_q, emb_c, self.index(), dl, wts

    def random(self):
        """the same shape and index with scorer_inputs' draws at the case's margin seed"""
        return self.random_at(margin_seed(self))

    def random_at(self, seed):
        emb_q, emb_c, dl, wts = scorer_inputs(self.Q, self.C, self.H, Nc=self.Nc, seed=seed)
        return emb_q, emb_c, self.index(), dl, wts


def _queries(*qs):
    def closed(Q, C_):
        m = np.zeros((Q, C_), bool)
        m[list(qs)] = True
        return m
    return closed


def _column(c):
    def closed(Q, C_):
        m = np.zeros((Q, C_), bool)
        m[:, c] = True
        return m
    return closed


def _cases():
    s = seams()
    CU, CROWS, CCOLS, SLAB = s["RT_CU"], s["RT_CROWS"], s["RT_CCOLS"], s["RT_SLAB"]
    NC, TC, TQ, HC = s["RK_NC"], s["RK_TC"], s["RK_TQ"], s["RK_HC"]
    out = []
    # pairs per row of emb_c across RT_CU: ONE index with the whole ladder, 9 x 16 cells; row 9 is named by the first and by
    # the last pair id, row 8 twice by query 4
    ladder = [0, 1, CU - 1, CU, CU + 1, 2 * CU - 1, 2 * CU, 2 * CU + 1, 3 * CU, 3 * CU + 1]
    out.append(Case("cu-ladder", 9, 16, 20, Nc=10, n_r=ladder, pins=((9, (0, 9 * 16 - 1)), (8, (4 * 16 + 3, 4 * 16 + 11)))))
    for Q in (CU - 1, CU, CU + 1, 2 * CU, 2 * CU + 1):
        out.append(Case("cu-shared-Q%d" % Q, Q, 5, 20))
    # rows of emb_c across RT_CROWS
    for Nc in (1, CROWS - 1, CROWS, CROWS + 1, 2 * CROWS, 2 * CROWS + 1):
        out.append(Case("crows-indexed-Nc%d" % Nc, 5, 7, 20, Nc=Nc, n_r=spread(28, Nc)))
        out.append(Case("crows-shared-Nc%d" % Nc, 5, Nc, 20))
    out.append(Case("crows-indexed-Nc%d-lastunnamed" % (CROWS + 1), 5, 7, 20, Nc=CROWS + 1, n_r=spread(28, CROWS + 1, (CROWS,))))
    # H across the candidate pass's 256 columns, the query pass's 64 and the forward's chunk of 1024
    for i, H in enumerate((CCOLS - 4, CCOLS, CCOLS + 4, 2 * CCOLS - 4, 2 * CCOLS, 2 * CCOLS + 4)):
        out.append(Case("ccols-indexed-H%d" % H, 5, 9, H, Nc=6, n_r=spread(38, 6)) if i % 2 == 0 else
                   Case("ccols-shared-H%d" % H, 5, 6, H))
    for i, H in enumerate((SLAB - 4, SLAB, SLAB + 4, 2 * SLAB - 4, 2 * SLAB, 2 * SLAB + 4)):
        out.append(Case("slab-shared-H%d" % H, 5, 6, H) if i % 2 == 0 else
                   Case("slab-indexed-H%d" % H, 5, 9, H, Nc=6, n_r=spread(38, 6)))
    for i, H in enumerate((HC - 4, HC, HC + 4, 2 * HC, 2 * HC + 4)):
        out.append(Case("hc-indexed-H%d" % H, 3, 5, H, Nc=4, n_r=spread(12, 4)) if i % 2 == 0 else
                   Case("hc-shared-H%d" % H, 3, 4, H))
    W, N = s["RANK_MAX_H"], s["RANK_MIN_H"]
    out.append(Case("widest-indexed-H%d" % W, 9, 33, W, Nc=20, n_r=spread(220, 20)))
    out.append(Case("widest-shared-H%d-small" % W, 2, 5, W))
    for H in (N, 2 * N):
        out.append(Case("narrow-indexed-H%d" % H, 5, 9, H, Nc=6, n_r=spread(38, 6)))
        out.append(Case("narrow-shared-H%d" % H, 5, 6, H))
    # C across the lane group's RK_NC candidates and the wave's RK_TC
    for i, C_ in enumerate((1, NC - 1, NC, NC + 1, TC - 1, TC, TC + 1, 2 * TC - 1, 2 * TC, 2 * TC + 1, 3 * TC + 1)):
        Nc = max(2, C_ // 2 + 1)
        out.append(Case("nc-indexed-C%d" % C_, 5, C_, 20, Nc=Nc, n_r=spread((5 * C_ * 3 + 3) // 4, Nc)) if i % 2 == 0 else
                   Case("nc-shared-C%d" % C_, 5, C_, 20))
    # Q across RK_TQ; 3 RK_TQ + 1 = 13 queries: four partial rows of d_fc2_w
    for i, Q in enumerate((1, TQ - 1, TQ, TQ + 1, 2 * TQ, 2 * TQ + 1, 3 * TQ + 1)):
        out.append(Case("tq-shared-Q%d" % Q, Q, 9, 20) if i % 2 == 0 else
                   Case("tq-indexed-Q%d" % Q, Q, 9, 20, Nc=6, n_r=spread(Q * 7, 6)))
    out.append(Case("tq-indexed-Q%d-lastlive" % (2 * TQ), 2 * TQ, 9, 20, Nc=6, n_r=spread(5 * 7, 6),
                    closed=_queries(*range(TQ, 2 * TQ - 1))))
    # absent and empty
    out.append(Case("absent-all", 5, 9, 20, Nc=6, n_r=[0] * 6))
    out.append(Case("absent-query", 5, 9, 20, Nc=6, n_r=spread(30, 6), closed=_queries(2)))
    out.append(Case("absent-column", 5, 9, 20, Nc=6, n_r=spread(30, 6), closed=_column(3)))
    out.append(Case("dlnan-holes", 9, 33, 68, Nc=12, n_r=spread(208, 12), dl_nan=True))
    # the workload's shape
    out.append(Case("workload-indexed", 200, 101, 300, Nc=104, n_r=spread(14140, 104)))
    out.append(Case("workload-shared", 200, 101, 300))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
RANDOM_CASES = [c for c in CASES if 0 < c.live_units() <= MARGIN_MAX_UNITS]
# the three shapes of the direct C-ABI calls: an index, none, and Q C a multiple of nothing
ABI_CASES = [BY_ID["cu-ladder"], [c for c in CASES if c.id.startswith("ccols-shared-")][-1],
             Case("abi-indexed-odd", 5, 33, 68, Nc=7, n_r=[0, 31, 9, 17, 25, 8, 33])]


# ---- references ------------------------------------------------------------------------------------------------------------
def _compose(emb_q, emb_c, ix, dl, wts, dtype):
    if ix is not None:
        dl = torch.where(ix < 0, torch.zeros_like(dl), dl)             # (dl at an absent pair is ignored)
    m = merge_layer(wts[0].shape[0], wts, dtype, "cpu")
    return [t.detach() for t in composed_scorer(m, emb_q.to(dtype), emb_c.to(dtype), ix, dl.to(dtype))]


def compose64(emb_q, emb_c, ix, dl, wts):
    """the seven outputs (OUTPUTS) of the float64 composition on the CPU"""
    return _compose(emb_q, emb_c, ix, dl, wts, torch.float64)


def compose32(emb_q, emb_c, ix, dl, wts):
    """... of torch's float32 composition on the CPU"""
    return _compose(emb_q, emb_c, ix, dl, wts, torch.float32)


def compose_abs(emb_q, emb_c, ix, dl, wts):
    """... of the float64 composition on the ABSOLUTE values of every input: element i is an upper bound of the sum of
    |terms| of element i of the output (every z >= 0 there: no unit is masked, except where all of its terms are zero)"""
    return compose64(emb_q.abs(), emb_c.abs(), ix, dl.abs(), [np.abs(w) for w in wts])


def live_z(emb_q, emb_c, ix, wts):
    """float64 z [live pairs, H] of the hidden layer"""
    w1, b1 = torch.from_numpy(wts[0]).double(), torch.from_numpy(wts[1]).double()
    H = emb_q.shape[1]
    pq = emb_q.double() @ w1[:, :H].T + b1
    pc = emb_c.double() @ w1[:, H:].T
    if ix is None:
        return (pq.unsqueeze(1) + pc.unsqueeze(0)).reshape(-1, H)
    q, c = torch.nonzero(ix >= 0, as_tuple=True)
    return pq[q] + pc[ix[q, c].long()]


@functools.lru_cache(maxsize=None)
def exact_reference(cid):
    """(float64 composition rounded once to float32 [7 tensors], the composition on absolute values [7 float64 tensors])"""
    case = BY_ID.get(cid) or {c.id: c for c in ABI_CASES}[cid]
    args = case.exact()
    return [t.float() for t in compose64(*args)], compose_abs(*args)


def margin_ok(z):
    a = z.abs()
    return z.numel() == 0 or float(a.min()) > 1e-5 * max(1.0, float(a.max()))


@functools.lru_cache(maxsize=None)
def margin_seed(case):
    """the first seed from the case's base at which no float64 z of a live pair lies within 1e-5 max(1, max|z|) of zero"""
    for seed in range(MARGIN_TRIES):
        emb_q, emb_c, ix, _, wts = case.random_at(seed)
        if margin_ok(live_z(emb_q, emb_c, ix, wts)):
            return seed
    raise AssertionError("%s: no seed in %d meets the margin condition" % (case.id, MARGIN_TRIES))


@functools.lru_cache(maxsize=None)
def random_reference(cid):
    """(inputs, float64 composition, elementwise bounds of logit / d_emb_q / d_emb_c) of a case of RANDOM_CASES"""
    case = BY_ID[cid]
    args = case.random()
    ref = compose64(*args)
    return args, ref, error_bound(case, ref, compose_abs(*args))


def chain_lengths(case):
    """L of (logit, d_emb_q, d_emb_c per row of emb_c) -- the module's docstring derives them"""
    H = case.H
    rows = torch.tensor(case.pair_counts(), dtype=torch.float64).reshape(-1, 1)
    return 2 * H + 4, H + case.C + 2, H + rows + 2


def error_bound(case, ref, A):
    """L 2^-24 A[i] + one float32 ulp of the reference, for the logits (0 where a pair is absent: -inf is exact), d_emb_q and
    d_emb_c"""
    out = []
    for L, r, a in zip(chain_lengths(case), ref[:3], A[:3]):
        fin = torch.isfinite(r)
        r0, a0 = torch.where(fin, r, torch.zeros_like(r)), torch.where(fin, a, torch.zeros_like(a))
        ulp = torch.from_numpy(np.spacing(np.abs(r0.numpy()).astype(np.float32)).astype(np.float64))
        out.append(L * U * a0 + ulp)
    return out


def share_of_bound(got, ref, bound):
    """max over the elements of |got - ref| / bound; the -inf pattern of the logits must be the reference's"""
    g, r = got.detach().double().cpu(), ref.double()
    gone = r == NEG_INF
    assert torch.equal(g == NEG_INF, gone), "the absent pairs differ"
    err = torch.where(gone, torch.zeros_like(r), g - torch.where(gone, torch.zeros_like(r), r)).abs()
    assert bool(torch.isfinite(err).all())
    return float((err / bound).max()) if err.numel() else 0.0


def bits_equal(a, b):
    """float32 tensors with the same bits.  The sign of a ZERO is not held (x + 0 first): whether an empty or cancelling sum is
    +0 or -0 depends on whether its chain starts from +0 or from its first product, in torch as in the kernels."""
    a, b = a.detach().cpu().contiguous() + 0.0, b.detach().cpu().contiguous() + 0.0
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
