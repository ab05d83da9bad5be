"""The pair scorer's and the node decoder's TRAINING kernels held to EXACT sums (tests/test_train_exact_cpu.py,
tests/test_train_exact_gpu.py): csrc/scoring_train.hip and csrc/decoder.hip, the method and the vocabulary of
tests/helpers_rank_exact.py.  Own code.

Exact inputs.  Pair scorer: emb [3B][H] in {-1, 0, 1}; each row of fc1.weight with min(8, H) entries of +-1 in its left half
and as many in its right half, zero elsewhere; fc1.bias in {-1, 0, 1}; fc2.weight in {+-1, +-2} and fc2.bias a small integer,
both times ONE power of two 2^-e per case, the smallest e with max|s| <= 8 (e <= 10: the probabilities are not saturated and
a missing unit moves s by at least 2^-10).  For the backward prob is PLANTED in {1/4, 1/2, 3/4} and dprob in {+-16, +-32}
(the C-ABI takes prob_dev and hid_dev as inputs), so ds = dprob p (1 - p) is +-3, +-4, +-6 or +-8 exactly, in the kernel's
order of operations; hid is the exact relu(z) of the forward.  Decoder: x in {-1, 0, 1}; rows of fc_1.weight with min(8, H)
entries of +-1, rows of fc_2.weight with 8, every column in one row; biases in {-1, 0, 1}; fc_3.weight in {+-1, +-2}, an
integer fc_3.bias, dz in {+-1, +-2}; dropout at p = 0 and p = 0.5, whose scale 1 / (1 - p) is exactly 2, the masks from
zebra_amd.decoder.decoder_dropout_mask.  Every product and every partial sum is then an integer (times 2^-e) far below 2^24
-- the CPU file shows it for every case from the composition on absolute values, intermediates included --, so float32
cannot round in ANY order of association: the kernels must return the bits of the float64 composition rounded once, and a
dropped, duplicated or misattributed term moves a sum by a non-zero integer.

Cases (CASES): one seam of the kernels' tiling or of the backward's plan each, the seam in the id.  seams() reads the tile
constants from the sources; score_plan / dec_plan restate the plan entries (zt_affinity_train_plan, zt_node_decoder_plan)
from the kernels' comments; crossed() says from the shape and the restated plan alone whether a case crosses what it names.
Seam rows -- the last row of a K-part and the first of the next, pair rows B - 1, B and 2B - 1, the last row of a ragged
tile -- get a planted live unit and +-1 inputs, and the CPU file asserts that each feeds every gradient a non-zero term.

The float64 restatements (score_forward64, score_backward64, dec_backward64; the decoder's forward is
helpers_decoder.forward64) add d_fc1_w K-part by K-part as the plan cuts it, so that the defects the comparison is there
for can be applied to them (MUTATIONS).

The bound of the random-input family (inputs drawn as tests/test_scoring_train_gpu.py and tests/helpers_decoder.py draw
them, at a committed margin seed).  With u = 2^-24 and A the composition on the absolute values of every input, an output
whose every term passes through at most L float32 roundings, in any order of association, is within L u A of the exact
value (first order in u; L u < 1e-3 here), plus one float32 ulp of the reference for its own rounding.  The backward is
called on PLANTED float32 prob / hid (h1 / h2): the float64 forward rounded once.  Every output of the backward is then a
multilinear form of its inputs, and A is well defined.  L, counted from the kernels' headers, a rounding for every product
and for every addition of a chain, whichever way the chain is associated:
 pair scorer, forward
  hid[r][h]      a term emb[k] W[h][k]: the product (1), at most H additions in its accumulator (the kernel keeps W_a src and
                 W_b x apart and adds them; torch adds 2H terms in one chain: 2H), the bias (1)               -> 2H + 3
 pair scorer, backward
  ds[r]          dprob p (1), 1 - p (1), their product (1)                                                    -> 3
  dh[r][h]       ds w2 (1)                                                                                    -> 4
  d_emb[.][k]    dh_pos + dh_neg (1), the product with W (1), H additions over the hidden index               -> H + 6
  d_fc2_b        2B additions of ds                                                                           -> 2B + 3
  d_fc1_b[h]     2B additions of dh                                                                           -> 2B + 4
  d_fc2_w[h]     ds hid (1), 2B additions                                                                     -> 2B + 4
  d_fc1_w[h][c]  dh x (1), 2B additions over the pair rows, at most ST_MAX_SPLIT - 1 = 7 of the partials      -> 2B + 12
 decoder, forward
  h1[r][k]       H products and additions, the bias, the dropout scale                                        -> H + 3
  h2[r][c]       h1 W2 (1), 80 additions, the bias, the scale                                                 -> H + 86
  logit[r]       h2 w3 (1), 10 additions, the bias                                                            -> H + 98
 decoder, backward
  dh2[r][c]      dz w3 (1), the scale (1)                                                                     -> 2
  dh1[r][k]      dh2 W2 (1), 10 additions, the scale (1)                                                      -> 14
  d_x[r][j]      dh1 W1 (1), 80 additions                                                                     -> 95
  d_fc3_b, d_fc3_w, d_fc2_b, d_fc2_w, d_fc1_b   at most dh1's 14, a product, N additions                      -> N + 15
  d_fc1_w        dh1 x (1), N additions, at most DEC_MAX_SPLIT - 1 = 7 of the partials                        -> N + 22
(the ReLU mask is a comparison, not a rounding: the margin condition keeps every float64 pre-activation
1e-5 max(1, max|z|) from zero, so that float32 takes the float64 mask)."""
import functools
import os
import re

import numpy as np
import torch

import helpers_decoder as hd
from helpers_rank_exact import bits_equal  # noqa: F401  (the comparison of both test files)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
MARGIN_MAX_UNITS = 65536           # pre-activations of a case of the random family (helpers_rank_exact.py says why)
MARGIN_TRIES = 64
H1, H2 = hd.H1, hd.H2
SCORE_OUT = ("d_emb", "d_fc1_w", "d_fc1_b", "d_fc2_w", "d_fc2_b")
DEC_OUT = ("d_x",) + tuple("g_" + k for k in hd.KEYS)
OLD_ABS, OLD_REL = 1e-5, 1e-4      # the max-norm tolerances of the direct tests: d_emb / d_x, + OLD_REL max|ref| for a parameter


def seams():
    """{"score": ..., "dec": ...}: the integer constants of csrc/scoring_fwd.hpp + scoring_train.hip and of csrc/decoder.hip,
    read from the sources"""
    out = {}
    for key, names in (("score", ("scoring_fwd.hpp", "scoring_train.hip")), ("dec", ("decoder.hip",))):
        vals = {}
        for name in names:
            text = open(os.path.join(ROOT, "zebra_amd", "csrc", name)).read()
            for decl in re.findall(r"constexpr int ([^;]+);", text):
                for item in decl.split(","):
                    m = re.fullmatch(r"\s*(\w+)\s*=\s*([\w\s()*/+-]+)", item)
                    if m:
                        try:
                            vals[m.group(1)] = int(eval(m.group(2).replace("/", "//"), {"__builtins__": {}}, dict(vals)))
                        except (NameError, SyntaxError):
                            pass
        out[key] = vals
    return out


S = seams()
SC, DC = S["score"], S["dec"]
GK = SC["GK"]                      # rows of a K-step of k_score_bwd_dw and of k_dec_bwd_dw
FIN_ROWS_SCORE = SC["SCORE_WAVES"] * 8        # k_score_bwd_fin: sixteen waves stride over the rows, eight loads in flight
FIN_ROWS_DEC = DC["FIN_WAVES"] * 4            # k_dec_bwd_fin: four loads in flight
FIN_OUTS = H1 + H2 * H1 + H2 + H2 + 1


def cdiv(a, b):
    return -(-a // b)


# ---- the plans, restated from the kernels' comments ------------------------------------------------------------------------
def score_max_split(H):
    """the 64 x 64 tiles of [H][2H] alone leave the chip idle: up to 256 workgroups, at most ST_MAX_SPLIT parts"""
    return max(1, min(SC["ST_MAX_SPLIT"], 256 // (cdiv(H, 64) * cdiv(2 * H, 64))))


def dec_max_split(H):
    return max(1, min(DC["DEC_MAX_SPLIT"], 256 // cdiv(H, 64)))


def _split(K, max_split):
    """K rows in partial products of whole 64-row steps, at least two steps each; the split recomputed from the rounded part"""
    steps = cdiv(K, GK)
    want = max(1, steps // 2)
    split = min(want, max_split)
    kper = cdiv(steps, split) * GK
    return dict(steps=steps, want=want, asked=split, k_per=kper, split=cdiv(K, kper))


def score_plan(B, H):
    """what zt_affinity_train_plan reports, restated"""
    p = _split(2 * B, score_max_split(H))
    p.update(max_split=score_max_split(H), grid_dx=cdiv(B, 16), grid_dw_x=cdiv(2 * H, 64), grid_dw_y=cdiv(H, 64),
             grid_dw_z=p["split"], lds_dx=(48 * (cdiv(H, 16) * 16 + 4) + 32) * 4,
             grid_fin=cdiv(H, 64) + (cdiv(H * 2 * H // 4, SC["SCORE_THREADS"]) if p["split"] > 1 else 0))
    return p


def dec_plan(N, H):
    """the backward's share of zt_node_decoder_plan, restated"""
    p = _split(N, dec_max_split(H))
    p.update(max_split=dec_max_split(H))
    return p


def parts_of(K, plan):
    """[(first row, end row)] of the K-parts"""
    return [(z * plan["k_per"], min(K, (z + 1) * plan["k_per"])) for z in range(plan["split"])]


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """kind "score": n = B edges, K = 2B pair rows; kind "dec": n = K = N rows, p the dropout probability"""

    def __init__(self, id, kind, n, H, p=0.0):
        self.id, self.kind, self.n, self.H, self.p = id, kind, n, H, p
        self.seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(id)) % 100000

    def __repr__(self):
        return self.id

    @property
    def K(self):
        return 2 * self.n if self.kind == "score" else self.n

    def plan(self):
        return score_plan(self.n, self.H) if self.kind == "score" else dec_plan(self.n, self.H)

    def units(self):
        return 2 * self.n * self.H if self.kind == "score" else self.n * (H1 + H2)

    def drop_seed(self):
        return hd.drop_seed(self.p, self.n, self.H)

    def masks(self):
        return hd.masks_of(self.p, self.n, self.H)

    def seam_rows(self):
        """rows of the K dimension that lie on a seam"""
        K, rows = self.K, set()
        for beg, end in parts_of(K, self.plan()):
            rows.update((beg, end - 1))
        rows.add(K - 1)
        if self.kind == "score":
            rows.update((self.n - 1, self.n))
        return sorted(rows)


def _first_reaching(max_split_of, m, widths):
    return next(H for H in widths if max_split_of(H) == m)


def score_widths():
    return range(4, SC["SCORE_MAX_H"] + 1, 4)


def dec_widths():
    return range(DC["DEC_MIN_H"], DC["DEC_MAX_H"] + 1, 4)


def split_values(max_split_of, widths):
    return sorted(set(max_split_of(H) for H in widths), reverse=True)


def _cases():
    out = []
    sc = lambda id, B, H: out.append(Case("score-%s-B%d-H%d" % (id, B, H), "score", B, H))
    dc = lambda id, N, H, p=0.0: out.append(Case("dec-%s-N%d-H%d%s" % (id, N, H, "-p0.5" if p else ""), "dec", N, H, p))
    W = SC["SCORE_MAX_H"]
    # ---- scoring_train.hip ----
    for B in (1, 15, 16, 17, 33):
        sc("tile16", B, 20)
    sc("hmin", 17, 4)
    for H in (16, 20, 24, 28):
        sc("hmod16", 17, H)
    for H in (60, 64, 68):
        sc("colgroup", 17, H)
    for H in (320, 324):
        sc("dxitems", 17, H)
    for H in (256, 260, 512, 516, W):
        sc("ntile", 17, H)
    for m in split_values(score_max_split, score_widths()):
        H = _first_reaching(score_max_split, m, score_widths()) if m < SC["ST_MAX_SPLIT"] else 20
        if m == 1:                                         # (want is never below 1: here the cap is what holds the split down)
            sc("maxsplit1-capped", 97, H)
            continue
        B = GK // 2 * (2 * m - 1)                          # 2B = 2m - 1 steps: want = m - 1; one row more: want = m
        sc("maxsplit%d-below" % m, B, H)
        sc("maxsplit%d-reached" % m, B + 1, H)
    sc("steps3", 96, 20)
    sc("steps4", 97, 20)
    sc("lowered-raggedpart", 529, 20)                      # 17 steps asked in 8 parts: 6 of 192 rows, the last one of 98
    sc("rowB-stepedge", 64, 20)
    sc("rowB-partedge", 128, 20)
    sc("rowB-straddle", 100, 20)
    for H in (40, 300, W):
        sc("workload", 4096, H)
    for B in (63, 64, 65, 129):
        sc("finrows", B, 24)
    for B in (511, 512, 513):
        sc("finthreads", B, 24)
    # ---- decoder.hip ----
    for N in (1, 15, 16, 17, 63, 64, 65):
        dc("tile16", N, 20)
    dc("hmin", 17, 4)
    for H in (16, 24, 28, 36):
        dc("hmod16", 17, H)
    for H in (252, 256, 260, 512, 516):
        dc("kchunk", 17, H)
    dc("widest", 17, DC["DEC_MAX_H"])
    for m in split_values(dec_max_split, dec_widths()):
        H = _first_reaching(dec_max_split, m, dec_widths())
        H = 2048 if m == DC["DEC_MAX_SPLIT"] else H        # the LAST width of the largest value: the next one takes 7
        N = GK * (2 * m - 1)
        dc("maxsplit%d-below" % m, N, H)
        dc("maxsplit%d-reached" % m, N + 1, H)
    for s in range(1, DC["DEC_MAX_SPLIT"] + 1):
        dc("split%d-below" % s, 2 * GK * s - GK, 12)
        dc("split%d" % s, 2 * GK * s, 12)
    dc("lowered3", 545, 20)
    dc("lowered6", 1057, 20)
    dc("lastpart-step-and-row", 4097, 20)
    dc("largest", 4097, DC["DEC_MAX_H"])
    dc("finrows", 129, 20)
    for N, H in ((17, 20), (200, 300), (1025, 516)):
        dc("dropout", N, H, 0.5)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
SCORE_CASES = [c for c in CASES if c.kind == "score"]
DEC_CASES = [c for c in CASES if c.kind == "dec"]
RANDOM_CASES = [c for c in CASES if c.units() <= MARGIN_MAX_UNITS]
# the calls with outputs left out and with a workspace planned for a larger batch: one product, and partial products
OPTIONAL_CASES = [BY_ID["score-tile16-B17-H20"], BY_ID["score-rowB-straddle-B100-H20"], BY_ID["dec-tile16-N17-H20"],
                  BY_ID["dec-split2-N256-H12"], BY_ID["dec-dropout-N200-H300-p0.5"]]


def crossed(case):
    """Does the case cross the seam its id names?  From its shape and the RESTATED plan alone."""
    fam = case.id.split("-")[1]
    n, H, K, p = case.n, case.H, case.K, case.plan()
    parts = parts_of(K, p)
    score = case.kind == "score"
    max_of = score_max_split if score else dec_max_split
    if fam == "tile16":
        return n in ((1, 15, 16, 17, 33) if score else (1, 15, 16, 17, 63, 64, 65))
    if fam == "hmin":
        return H == 4
    if fam == "hmod16":
        return H > 4 and H < 64
    if fam == "colgroup":                                  # one column workgroup | two; a ragged last group
        return (H, cdiv(H, 64), H % 64 != 0) in ((60, 1, True), (64, 1, False), (68, 2, True))
    if fam == "dxitems":                                   # 3 ceil(H / 64) work items on sixteen waves
        return (H, 3 * cdiv(H, 64) > SC["SCORE_WAVES"]) in ((320, False), (324, True))
    if fam == "ntile":                                     # N-tiles w, w + 16, ...: a wave's second, third, fourth
        return (H, cdiv(cdiv(H, 16), SC["SCORE_WAVES"])) in ((256, 1), (260, 2), (512, 2), (516, 3), (768, 3)) and H <= SC["SCORE_MAX_H"]
    if fam == "kchunk":                                    # chunks of DEC_KC columns; ceil(H / 64) items of d_x on four waves
        return (H, cdiv(H, DC["DEC_KC"]), cdiv(H, 64) > 4) in ((252, 1, False), (256, 1, False), (260, 2, True), (512, 2, True), (516, 3, True))
    if fam == "widest":
        return H == DC["DEC_MAX_H"] and dec_max_split(H) == min(dec_max_split(h) for h in dec_widths())
    if fam.startswith("maxsplit"):
        m = int(fam[len("maxsplit"):])
        if max_of(H) != m:
            return False
        if case.id.split("-")[2] == "capped":
            return p["want"] > 1 and p["split"] == 1
        below = case.id.split("-")[2] == "below"
        return (p["want"] == m - 1 and p["steps"] == 2 * m - 1) if below else (p["want"] == m and p["split"] == m and K % GK == (2 if score else 1))
    if fam == "steps3":
        return p["steps"] == 3 and p["split"] == 1
    if fam == "steps4":
        return p["steps"] == 4 and p["split"] == 2
    if fam == "lowered":
        return p["steps"] == 17 and p["asked"] == 8 and p["split"] == 6 and (parts[-1][1] - parts[-1][0]) % GK != 0
    if fam == "lowered3":
        return p["asked"] == 4 and p["split"] == 3
    if fam == "lowered6":
        return p["asked"] == 8 and p["split"] == 6
    if fam == "rowB":
        kind = case.id.split("-")[2]
        if kind == "stepedge":
            return n % GK == 0 and p["split"] == 1 and p["steps"] == 2
        if kind == "partedge":
            return p["split"] == 2 and parts[0][1] == n
        return p["split"] == 2 and n % GK != 0 and parts[0][0] < n < parts[0][1]
    if fam == "workload":
        return n == 4096 and p["split"] == max_of(H) and H in (40, 300, SC["SCORE_MAX_H"])
    if fam == "finrows":
        return K in ((126, 128, 130, 258) if score else (129,)) and FIN_ROWS_SCORE == 128 and FIN_ROWS_DEC == 64
    if fam == "finthreads":
        return K in (1022, 1024, 1026) and SC["SCORE_THREADS"] == 1024
    if fam.startswith("split"):
        s = int(fam[len("split"):])
        below = case.id.split("-")[2] == "below"
        return (p["steps"] == 2 * s - 1 and p["want"] == max(1, s - 1)) if below else (p["split"] == s and p["k_per"] == 2 * GK)
    if fam == "lastpart":
        return p["split"] == 8 and parts[-1][1] - parts[-1][0] == GK + 1
    if fam == "largest":
        return (n, H) == (4097, DC["DEC_MAX_H"])
    if fam == "dropout":
        return case.p == 0.5 and (n, H) in ((17, 20), (200, 300), (1025, 516))
    return False


# ---- exact inputs ----------------------------------------------------------------------------------------------------------
def _sparse_rows(rng, rows, cols, n):
    """[rows][cols] with n entries of +-1 per row at distinct columns (sorted draws, spread apart)"""
    w = np.zeros((rows, cols), np.float32)
    pos = np.sort(rng.randint(0, cols - n + 1, (rows, n)), axis=1) + np.arange(n)
    w[np.arange(rows)[:, None], pos] = rng.choice([-1.0, 1.0], (rows, n))
    return w


def _cover_rows(rng, rows, cols):
    """[rows][cols] with cols / rows entries of +-1 per row, every column in exactly one row: no column is idle"""
    w = np.zeros((rows, cols), np.float32)
    w[np.repeat(np.arange(rows), cols // rows), rng.permutation(cols)] = rng.choice([-1.0, 1.0], cols)
    return w


def _plant_row(x, w_row):
    """x gets w_row's signs at w_row's non-zero columns: x . w_row = the number of its entries"""
    nz = w_row != 0
    x[nz] = w_row[nz]


SALTS = 32                         # draws tried until every seam row counts (the first one serves nearly every case)


@functools.lru_cache(maxsize=4)
def score_exact(cid):
    """dict(emb, wts [fc1.weight, fc1.bias, fc2.weight, fc2.bias], e, prob, dprob) float32 numpy; prob / dprob are the PLANTED
    inputs of the backward.  The first draw from the case's seed in which every seam row counts and no output is all zero."""
    case = BY_ID[cid]
    for salt in range(SALTS):
        d = _score_draw(case, salt)
        hid = f32(score_forward64(d["emb"], d["wts"])["hid"])
        out = score_backward64(d["emb"], d["wts"], d["prob"], hid, d["dprob"], case.plan())
        if not score_seam_rows_missing(case, d, hid) and all(np.any(o != 0) for o in out):     # (no output is all zero: d_fc2_b too)
            return d
    raise AssertionError("%s: no draw in which every seam row counts" % cid)


def score_seam_rows_missing(case, d, hid):
    """[(row, gradient)] of the seam rows whose own term is zero in every element of a gradient they feed"""
    B, H = case.n, case.H
    w1 = d["wts"][0].astype(np.float64)
    _, im = score_backward64(d["emb"], d["wts"], d["prob"], hid, d["dprob"], case.plan(), intermediates=True)
    nz = lambda a: bool(np.any(a != 0))
    bad = []
    for r in case.seam_rows():
        dh, x, ds = im["dh"][r], im["X"][r], im["ds"][r]
        ok = {"d_fc2_b": ds != 0, "d_fc1_b": nz(dh), "d_fc2_w": nz(ds * hid[r]), "d_fc1_w": nz(dh) and nz(x[:H]) and nz(x[H:]),
              "d_emb": nz(dh @ w1[:, :H]) and nz(dh @ w1[:, H:])}
        bad += [(r, k) for k, v in ok.items() if not v]
    return bad


def _score_draw(case, salt):
    B, H = case.n, case.H
    rng = np.random.RandomState(case.seed + 100003 * salt)
    emb = rng.randint(-1, 2, (3 * B, H)).astype(np.float32)
    n = min(8, H)
    w1 = np.concatenate([_sparse_rows(rng, H, H, n), _sparse_rows(rng, H, H, n)], axis=1)
    b1 = rng.randint(-1, 2, H).astype(np.float32)
    w2 = rng.choice([-2.0, -1.0, 1.0, 2.0], (1, H)).astype(np.float32)
    b2 = rng.randint(-3, 4, 1).astype(np.float32)
    prob = rng.choice([0.25, 0.5, 0.75], 2 * B).astype(np.float32)
    dprob = rng.choice([-32.0, -16.0, 16.0, 32.0], 2 * B).astype(np.float32)
    for r in case.seam_rows():                             # a live unit and +-1 inputs on every seam row
        e, h0 = r % B, (r % B) % H                         # (the two pair rows of an edge share its src row: one unit for both)
        _plant_row(emb[e], w1[h0, :H])
        _plant_row(emb[B + r], w1[h0, H:])                 # (pair row r reads row B + r of emb: dst, then neg)
    s_int = score_forward64(emb, [w1, b1, w2, b2])["s"]
    e = 0
    while float(np.abs(s_int).max()) * 2.0 ** -e > 8.0:
        e += 1
    scale = np.float32(2.0 ** -e)
    return dict(emb=emb, wts=[w1, b1, w2 * scale, b2 * scale], e=e, prob=prob, dprob=dprob)


@functools.lru_cache(maxsize=4)
def dec_exact(cid):
    """dict(P, x, dz) float32 numpy: the first draw from the case's seed in which every seam row counts and no output is all zero"""
    case = BY_ID[cid]
    m1, m2 = case.masks()
    for salt in range(SALTS):
        d = _dec_draw(case, salt)
        fwd = hd.forward64(d["P"], d["x"], m1, m2)
        out = dec_backward64(d["P"], d["x"], f32(fwd["h1"]), f32(fwd["h2"]), d["dz"], m1, m2, case.plan())
        if not dec_seam_rows_missing(case, d, f32(fwd["h1"]), f32(fwd["h2"])) and all(np.any(o != 0) for o in out):
            return d
    raise AssertionError("%s: no draw in which every seam row counts" % cid)


def dec_seam_rows_missing(case, d, h1, h2):
    m1, m2 = case.masks()
    P = d["P"]
    _, im = dec_backward64(P, d["x"], h1, h2, d["dz"], m1, m2, case.plan(), intermediates=True)
    nz = lambda a: bool(np.any(a != 0))
    bad = []
    for r in case.seam_rows():
        dh1, dh2 = im["dh1"][r], im["dh2"][r]
        ok = {"d_fc3_b": d["dz"][r] != 0, "d_fc3_w": nz(h2[r]), "d_fc2_b": nz(dh2), "d_fc2_w": nz(dh2) and nz(h1[r]), "d_fc1_b": nz(dh1),
              "d_fc1_w": nz(dh1) and nz(d["x"][r]), "d_x": nz(dh1 @ P["fc_1.weight"].astype(np.float64))}
        bad += [(r, k) for k, v in ok.items() if not v]
    return bad


def _dec_draw(case, salt):
    N, H = case.n, case.H
    rng = np.random.RandomState(case.seed + 100003 * salt)
    x = rng.randint(-1, 2, (N, H)).astype(np.float32)
    P = {"fc_1.weight": _sparse_rows(rng, H1, H, min(8, H)), "fc_1.bias": rng.randint(-1, 2, H1).astype(np.float32),
         "fc_2.weight": _cover_rows(rng, H2, H1), "fc_2.bias": rng.randint(-1, 2, H2).astype(np.float32),
         "fc_3.weight": rng.choice([-2.0, -1.0, 1.0, 2.0], (1, H2)).astype(np.float32),
         "fc_3.bias": rng.randint(-3, 4, 1).astype(np.float32)}
    dz = rng.choice([-2.0, -1.0, 1.0, 2.0], N).astype(np.float32)
    m1, _ = case.masks()
    for r in case.seam_rows():
        kept = np.arange(H1) if m1 is None else np.flatnonzero(m1[r] > 0)
        _plant_row(x[r], P["fc_1.weight"][kept[r % len(kept)]])
    return dict(P=P, x=x, dz=dz)


# ---- the float64 restatements ----------------------------------------------------------------------------------------------
def score_forward64(emb, wts, absolute=False):
    """dict(z, hid [2B][H], s [2B]) in float64; absolute: on the absolute values of every input"""
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    emb, (w1, b1, w2, b2) = f(emb), [f(w) for w in wts]
    B, H = emb.shape[0] // 3, emb.shape[1]
    u = emb[:B] @ w1[:, :H].T
    z = np.concatenate([u + emb[B:2 * B] @ w1[:, H:].T, u + emb[2 * B:] @ w1[:, H:].T]) + b1
    hid = np.maximum(z, 0.0)
    return dict(z=z, hid=hid, s=hid @ w2[0] + b2[0])


def _without_a_kstep(dh):
    """dh with the last k-step of four hidden units that carries anything set to zero"""
    k0 = int(np.flatnonzero(np.any(dh != 0, axis=0))[-1]) // 4 * 4
    out = dh.copy()
    out[:, k0:k0 + 4] = 0.0
    return out


def _parts_product(dh, X, parts, mut):
    """dh^T X added K-part by K-part, first to last"""
    total = None
    for i, (beg, end) in enumerate(parts):
        rows = np.arange(beg, end)
        if mut == "row_out" and i == len(parts) - 1:
            rows = rows[:-1]                               # the last row of the last K-part: the ragged end
        part = dh[rows].T @ X[rows]
        if mut == "part_twice" and i == len(parts) - 1:
            part = part + part
        total = part if total is None else total + part
    return total


def score_backward64(emb, wts, prob, hid, dprob, plan, mut=None, absolute=False, intermediates=False):
    """the five outputs (SCORE_OUT) in float64 from the backward's own inputs"""
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    emb, (w1, b1, w2, b2), prob, hid, dprob = f(emb), [f(w) for w in wts], np.asarray(prob, np.float64), f(hid), f(dprob)
    B, H = emb.shape[0] // 3, emb.shape[1]
    ds = dprob * prob * (1.0 - prob)
    live = hid >= 0 if mut == "mask_ge" else hid > 0
    dh = ds[:, None] * w2 * live
    src2 = np.concatenate([emb[:B], emb[:B]])
    x2 = np.concatenate([emb[2 * B:], emb[B:2 * B]]) if mut == "swap_dst_neg" else emb[B:]
    X = np.concatenate([src2, x2], axis=1)
    dhx = _without_a_kstep(dh) if mut == "kstep_out" else dh
    d_emb = np.concatenate([(dhx[:B] + dhx[B:]) @ w1[:, :H], dhx[:B] @ w1[:, H:], dhx[B:] @ w1[:, H:]])
    out = [d_emb, _parts_product(dh, X, parts_of(2 * B, plan), mut), dh.sum(0), (ds[:, None] * hid).sum(0), np.array([ds.sum()])]
    return (out, dict(ds=ds, dh=dh, X=X)) if intermediates else out


def dec_forward64(P, x, m1, m2, absolute=False):
    if absolute:
        P, x = {k: np.abs(v) for k, v in P.items()}, np.abs(x)
    return hd.forward64(P, x, m1, m2)


def dec_backward64(P, x, h1, h2, dz, m1, m2, plan, mut=None, absolute=False, intermediates=False):
    """the seven outputs (DEC_OUT) in float64 from the backward's own inputs: h1 / h2 after ReLU and dropout, the masks"""
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    W1, b1, W2, b2, W3, b3 = [f(P[k]) for k in hd.KEYS]
    x, h1, h2, dz = f(x), f(h1), f(h2), f(dz)
    N = x.shape[0]
    s1 = np.ones((N, H1)) if m1 is None else np.asarray(m1, np.float64)
    s2 = np.ones((N, H2)) if m2 is None else np.asarray(m2, np.float64)
    live1, live2 = (h1 >= 0, h2 >= 0) if mut == "mask_ge" else (h1 > 0, h2 > 0)
    dh2 = dz[:, None] * W3 * s2 * live2
    dh1 = (dh2 @ W2) * (1.0 if mut == "no_scale" else s1) * live1
    dhx = _without_a_kstep(dh1) if mut == "kstep_out" else dh1
    out = [dhx @ W1, _parts_product(dh1, x, parts_of(N, plan), mut), dh1.sum(0), dh2.T @ h1, dh2.sum(0),
           (dz[:, None] * h2).sum(0)[None, :], np.array([dz.sum()])]
    return (out, dict(dh1=dh1, dh2=dh2)) if intermediates else out


MUTATIONS = ("row_out", "part_twice", "swap_dst_neg", "mask_ge", "kstep_out", "no_scale")


def mutation_applies(mut, case):
    if mut == "swap_dst_neg":
        return case.kind == "score"
    if mut == "no_scale":
        return case.kind == "dec" and case.p > 0
    return True


# ---- references ------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


@functools.lru_cache(maxsize=4)
def exact_reference(cid):
    """dict of one exact case: its inputs, the planted inputs of the backward, "fwd" (the forward's float32 outputs), "out"
    (the backward's outputs: the float64 composition rounded once), "out64", and "worst" (the largest value, in units of the
    case's power of two, that the composition on absolute values reaches in any output or intermediate)"""
    case = BY_ID[cid]
    plan = case.plan()
    if case.kind == "score":
        d = dict(score_exact(cid))
        fwd = score_forward64(d["emb"], d["wts"])
        d["hid"], d["s64"] = f32(fwd["hid"]), fwd["s"]
        d["z64"] = fwd["z"]
        d["out64"] = score_backward64(d["emb"], d["wts"], d["prob"], d["hid"], d["dprob"], plan)
        fa = score_forward64(d["emb"], d["wts"], absolute=True)
        oa, ia = score_backward64(d["emb"], d["wts"], d["prob"], fa["hid"], d["dprob"], plan, absolute=True, intermediates=True)
        unit = 2.0 ** d["e"]
        # (d_fc2_w = sum ds hid and d_fc2_b = sum ds do not carry fc2.weight's power of two; z and hid neither)
        d["worst"] = max([float(fa["z"].max()), float(fa["s"].max()) * unit, float(ia["dh"].max()) * unit] +
                         [float(o.max()) * (1.0 if k in (3, 4) else unit) for k, o in enumerate(oa)])
    else:
        d = dict(dec_exact(cid))
        m1, m2 = case.masks()
        fwd = hd.forward64(d["P"], d["x"], m1, m2)
        d["m1"], d["m2"], d["fwd64"] = m1, m2, fwd
        d["h1"], d["h2"], d["logit"] = f32(fwd["h1"]), f32(fwd["h2"]), f32(fwd["z"])
        d["out64"] = dec_backward64(d["P"], d["x"], d["h1"], d["h2"], d["dz"], m1, m2, plan)
        fa = dec_forward64(d["P"], d["x"], m1, m2, absolute=True)
        oa, ia = dec_backward64(d["P"], d["x"], fa["h1"], fa["h2"], d["dz"], m1, m2, plan, absolute=True, intermediates=True)
        d["worst"] = max([float(fa[k].max()) for k in ("pre1", "h1", "pre2", "h2", "z")] + [float(ia["dh1"].max()), float(ia["dh2"].max())] +
                         [float(o.max()) for o in oa])
    d["out"] = [f32(o) for o in d["out64"]]
    return d


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ---- torch's float32 composition on the CPU --------------------------------------------------------------------------------
def score_forward32(emb, wts):
    emb, (w1, b1, w2, b2) = t32(emb), [t32(w) for w in wts]
    B = emb.shape[0] // 3
    z = torch.nn.functional.linear(torch.cat([torch.cat([emb[:B], emb[:B]]), emb[B:]], dim=1), w1, b1)
    hid = torch.relu(z)
    return hid.numpy(), torch.nn.functional.linear(hid, w2, b2)[:, 0].numpy()


def score_backward32(emb, wts, prob, hid, dprob):
    emb, (w1, b1, w2, b2), prob, hid, dprob = t32(emb), [t32(w) for w in wts], t32(prob), t32(hid), t32(dprob)
    B, H = emb.shape[0] // 3, emb.shape[1]
    ds = dprob * prob * (1.0 - prob)
    dh = ds[:, None] * w2 * (hid > 0)
    X = torch.cat([torch.cat([emb[:B], emb[:B]]), emb[B:]], dim=1)
    dX = dh @ w1
    d_emb = torch.cat([dX[:B, :H] + dX[B:, :H], dX[:B, H:], dX[B:, H:]])
    return [t.numpy() for t in (d_emb, dh.T @ X, dh.sum(0), (ds[:, None] * hid).sum(0), ds.sum().reshape(1))]


def dec_forward32(P, x, m1, m2):
    W1, b1, W2, b2, W3, b3 = [t32(P[k]) for k in hd.KEYS]
    h1 = torch.relu(torch.nn.functional.linear(t32(x), W1, b1))
    if m1 is not None:
        h1 = h1 * t32(m1)
    h2 = torch.relu(torch.nn.functional.linear(h1, W2, b2))
    if m2 is not None:
        h2 = h2 * t32(m2)
    return h1.numpy(), h2.numpy(), torch.nn.functional.linear(h2, W3, b3)[:, 0].numpy()


def dec_backward32(P, x, h1, h2, dz, m1, m2):
    W1, b1, W2, b2, W3, b3 = [t32(P[k]) for k in hd.KEYS]
    x, h1, h2, dz = t32(x), t32(h1), t32(h2), t32(dz)
    dh2 = dz[:, None] * W3 * (h2 > 0)
    if m2 is not None:
        dh2 = dh2 * t32(m2)
    dh1 = (dh2 @ W2) * (h1 > 0)
    if m1 is not None:
        dh1 = dh1 * t32(m1)
    return [t.numpy() for t in (dh1 @ W1, dh1.T @ x, dh1.sum(0), dh2.T @ h1, dh2.sum(0), (dz[:, None] * h2).sum(0)[None, :],
                                dz.sum().reshape(1))]


# ---- the random family -----------------------------------------------------------------------------------------------------
# tests/test_scoring_train_gpu.py's WIDTHS: hidden width H = D (n_tppr + 1) -> (D, n_tppr)
OLD_WIDTHS = {40: (20, 1), 60: (20, 2), 200: (100, 1), 300: (100, 2), 344: (172, 1), 516: (172, 2), 768: (256, 2), 400: (100, 3)}


def score_random_at(case, seed):
    """tests/test_scoring_train_gpu.py's _inputs(B, H) -- emb ~ 0.7 N(0, 1), dprob at the scale of BCE's mean, the weight
    generator of the scorer tests -- with the seed free: seed 0 is that test's own draw"""
    import inputs as I
    B, H = case.n, case.H
    g = torch.Generator().manual_seed(1000 * H + B + 7919 * seed)
    emb = (torch.randn((3 * B, H), generator=g) * 0.7).numpy()
    sign = torch.cat([-torch.ones(B), torch.ones(B)])
    dprob = (sign * (0.25 + 0.5 * torch.rand(2 * B, generator=g)) / B).numpy()
    D, M = OLD_WIDTHS.get(H, (H // 2, 1) if H >= 8 else (H, 0))
    assert D * (M + 1) == H
    w = I.model_weights(D, 1, 20, M, 7 + H + 7919 * seed)
    return emb, dprob, [w["aff1_w"], w["aff1_b"], w["aff2_w"], w["aff2_b"]]


def dec_random_at(case, seed):
    """helpers_decoder.draw_case at seed_base + seed"""
    return hd.draw_case(case.n, case.H, hd.seed_base(case.n, case.H, case.p) + seed)


def _margin(z):
    a = np.abs(z)
    return a.size == 0 or float(a.min()) > 1e-5 * max(1.0, float(a.max()))


def margin_ok(case, seed):
    if case.kind == "score":
        emb, _, wts = score_random_at(case, seed)
        return _margin(score_forward64(emb, wts)["z"])
    P, x, _ = dec_random_at(case, seed)
    m1, m2 = case.masks()
    return hd.margin_ok(hd.forward64(P, x, m1, m2))


def derive_margin_seed(case):
    """the first seed at which no float64 pre-activation lies within 1e-5 max(1, max|z|) of zero"""
    for seed in range(MARGIN_TRIES):
        if margin_ok(case, seed):
            return seed
    raise AssertionError("%s: no seed in %d meets the margin condition" % (case.id, MARGIN_TRIES))


# case id -> the seed derive_margin_seed returns where it is not 0: committed, re-derived by tests/test_train_exact_cpu.py
MARGIN_SEEDS = {"score-ntile-B17-H512": 2, "score-ntile-B17-H768": 2, "score-maxsplit8-reached-B481-H20": 4,
                "score-lowered-raggedpart-B529-H20": 1, "score-finthreads-B513-H24": 3, "dec-kchunk-N17-H260": 1,
                "dec-maxsplit6-below-N704-H2308": 3, "dec-maxsplit6-reached-N705-H2308": 4, "dec-maxsplit5-below-N576-H2692": 8,
                "dec-maxsplit5-reached-N577-H2692": 1, "dec-maxsplit4-below-N448-H3268": 9, "dec-maxsplit4-reached-N449-H3268": 3,
                "dec-split3-below-N320-H12": 2, "dec-split4-below-N448-H12": 4, "dec-split4-N512-H12": 4,
                "dec-split5-below-N576-H12": 15, "dec-split5-N640-H12": 2, "dec-split6-below-N704-H12": 2, "dec-lowered3-N545-H20": 7}


def margin_seed(case):
    return MARGIN_SEEDS.get(case.id, 0)


def chain_lengths(case):
    """(L of the forward's outputs, L of the backward's outputs) -- the module's docstring derives them"""
    n, H = case.n, case.H
    if case.kind == "score":
        return dict(hid=2 * H + 3), [H + 6, 2 * n + 12, 2 * n + 4, 2 * n + 4, 2 * n + 3]
    return dict(h1=H + 3, h2=H + 86, logit=H + 98), [95, n + 22] + [n + 15] * 5


def _bound(L, ref, A):
    return L * U * np.asarray(A, np.float64) + np.spacing(np.abs(f32(ref))).astype(np.float64)


@functools.lru_cache(maxsize=4)
def random_reference(cid):
    """dict of one case of the random family at its margin seed: the inputs, the planted float32 inputs of the backward,
    "fwd64" / "fwd_bound" (name -> float64 reference / elementwise bound of the forward's exact-chain outputs), "out64" /
    "bound" (the backward's), and for the scorer "s64" (the scores, whose probabilities test_scoring_f64_gpu.py's bound holds)"""
    case = BY_ID[cid]
    plan, seed = case.plan(), margin_seed(case)
    Lf, Lb = chain_lengths(case)
    if case.kind == "score":
        emb, dprob, wts = score_random_at(case, seed)
        fwd, fa = score_forward64(emb, wts), score_forward64(emb, wts, absolute=True)
        d = dict(emb=emb, dprob=dprob, wts=wts, s64=fwd["s"], z64=fwd["z"], prob=f32(hd.sigmoid64(fwd["s"])), hid=f32(fwd["hid"]))
        d["fwd64"] = dict(hid=fwd["hid"])
        d["fwd_bound"] = dict(hid=_bound(Lf["hid"], fwd["hid"], fa["hid"]))
        d["out64"] = score_backward64(emb, wts, d["prob"], d["hid"], dprob, plan)
        A = score_backward64(emb, wts, d["prob"], d["hid"], dprob, plan, absolute=True)
    else:
        P, x, dz = dec_random_at(case, seed)
        m1, m2 = case.masks()
        fwd, fa = hd.forward64(P, x, m1, m2), dec_forward64(P, x, m1, m2, absolute=True)
        d = dict(P=P, x=x, dz=dz, m1=m1, m2=m2, h1=f32(fwd["h1"]), h2=f32(fwd["h2"]))
        d["fwd64"] = dict(h1=fwd["h1"], h2=fwd["h2"], logit=fwd["z"])
        d["fwd_bound"] = {k: _bound(Lf[k], fwd[r], fa[r]) for k, r in (("h1", "h1"), ("h2", "h2"), ("logit", "z"))}
        d["out64"] = dec_backward64(P, x, d["h1"], d["h2"], dz, m1, m2, plan)
        A = dec_backward64(P, x, d["h1"], d["h2"], dz, m1, m2, plan, absolute=True)
    d["bound"] = [_bound(L, r, a) for L, r, a in zip(Lb, d["out64"], A)]
    return d


def share_of_bound(got, ref, bound):
    """max over the elements of |got - ref| / bound"""
    err = np.abs(np.asarray(got, np.float64).reshape(np.shape(ref)) - ref)
    assert np.isfinite(err).all()
    return float((err / bound).max()) if err.size else 0.0


def np_bits_equal(a, b):
    return bits_equal(t32(a), t32(np.asarray(b).reshape(np.shape(a))))
