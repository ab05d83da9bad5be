"""The link scorers (csrc/scoring.hip: k_affinity, k_affinity_tiled, k_affinity_gen, k_affinity_gen_tiled behind
zt::affinity_kernel_plan; csrc/rank.hip: k_rank_pairs) at every form and seam of their plans, against the plain float64
restatement oracle/score_f64.py (pinned to torch's float64 MergeLayer and to the C oracle in tests/test_scoring_f64_cpu.py,
which also shows that every seam named below is in a list, that the bound has room for float32 on these inputs and that it
rejects wrong results of the kinds it is there to catch).

Bound, per element, nothing fitted:  |p - p64| <= p64 (1 - p64) TOL_Z + 2^-23,  TOL_Z = 1e-5 max(1, max |z64|).
1e-5 max(1, max|ref|) is what the suite asserts for a linear layer's output (the aggregation's H, the memory cell's rows);
p (1 - p) is the sigmoid's derivative; 2^-23 covers the final expf, division and rounding to float32.  torch's float32
composition on the device, in the reference's concatenated form and in the kernels' split form, is held to HALF of it.

Pair scorer: every case goes through TGN.score_device with ZT_CHOICE_SCORE pinned and the plan asked first; it runs twice and
the bits are equal.  The first run reads the embeddings as the TAIL of a larger allocation (NaN in front); the second reads them
as the HEAD of one (NaN behind) and writes its probabilities in front of a sentinel.
  latency      k_affinity<13 | 19>: all eight H of the two padded widths 208 / 304; B over a ragged tile, whole tiles, the pick's
               511 | 512; B = 2560 | 2561 | 2577: 160 | 161 | 162 tiles on a grid capped at 160 -- a wave's second tile (its
               weights kept, a counter per tile), some waves with one tile, a ragged last tile
  tiled        k_affinity_tiled<13 | 19, 16 | 32>: the same eight H (the `c4 < h4` zeroing of a ragged last chunk), ET 16 | 32 at
               B = 8192 | 8193, ragged 32-edge tiles (8200, 8223)
  gen_latency  k_affinity_gen: rounds of AG_U = 8 k-chunks and of 8 partials: NT = 8 | 9 (H = 128 | 132), 16 | 17 (256 | 260),
               32 | 33 (512 | 516), 48 (764 | 768); H mod 16 in 0, 4, 8, 12; the grid cap at H = 132
  gen_tiled    score_fwd_body: k-chunks four a round plus a remainder loop (NT mod 4 = 1, 2, 3, 0: H = 4, 20, 36, 52), a wave's
               second and third N-tile (NT = 16 | 17, 32 | 33, 48), H mod 16 in 0, 4, 8, 12
The four forms against each other at H = 200, 300 and B = 511 | 512, 8192 | 8193; embeddings x 4, x 30, x 400 (saturation: p is
exactly 1 where z64 >= 18 and exactly 0 where z64 <= -104); NaN and +inf rows; the one-vs-many scorer at the seams of its
4 x 32 tile and its chunks of 1024 columns.

Measured on an MI355X (the table per form and H is in DESIGN.md, "The link scorers against float64"): over the 203 pair cases
the kernels use at most 0.077 of the bound (largest |p - p64| 4.2e-07, gen_tiled at H = 768), torch's float32 compositions at
most 0.116 (5.9e-07); latency and gen_latency give the same bits; any two forms differ by <= 2.4e-07; the one-vs-many scorer uses
at most 0.123 (H = 2048; torch 0.192); stress cases at most 0.50 of the plain bound, as torch.  Nothing wrong found.  Six
single-line defects put into the kernels on a scratch copy each fail between 2 and 74 of this file's 238 cases."""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

import inputs as I
from conftest import ROOT

pytestmark = pytest.mark.gpu

LATENCY, TILED, GEN_LATENCY, GEN_TILED = 1, 2, 3, 4
FORM_NAMES = {LATENCY: "latency", TILED: "tiled", GEN_LATENCY: "gen_latency", GEN_TILED: "gen_tiled"}
TOL_LINEAR = 1e-5                  # of a linear layer's output, times max(1, max|ref|): test_memory_f64_gpu.py, test_attention_f64_gpu.py
ULP_P = 2.0 ** -23                 # the final expf, division and rounding of a probability <= 1
OLD_TOL = 1e-4                     # what tests/test_scoring_gpu.py and test_scoring_wide_gpu.py assert on a probability
FORM_TOL = 1e-5                    # two float32 associations of the same sums (tests/test_scoring_wide_gpu.py: FORM_TOL)
SENTINEL = 777.0
SPEC_H = (196, 200, 204, 208, 292, 296, 300, 304)          # round_up16(H) in {208, 304}: the specialised kernels' widths
GEN_LATENCY_H = (4, 8, 12, 16, 20, 36, 128, 132, 256, 260, 512, 516, 764, 768)
GEN_TILED_H = (4, 20, 36, 52, 68, 256, 260, 344, 512, 516, 764, 768)
# hidden width H = D (n_tppr + 1) -> (D, n_tppr) of the weight generator where the suite has named one (test_scoring_wide_gpu.py,
# test_query_gpu.py); every other width: (H / 2, 1)
WIDTHS = {4: (2, 1), 20: (10, 1), 200: (100, 1), 300: (100, 2), 344: (172, 1), 512: (256, 1), 516: (172, 2), 768: (256, 2),
          4352: (256, 16)}

# (form, B, H)
CASES = ([(LATENCY, B, H) for H in SPEC_H for B in (1, 15, 16, 17, 33, 511, 512)] +
         [(LATENCY, B, H) for H in (204, 300) for B in (2560, 2561, 2577)] +
         [(TILED, B, H) for H in SPEC_H for B in (1, 17, 511, 512, 1000)] +
         [(TILED, B, H) for H in (204, 304) for B in (8192, 8193, 8200, 8223)] +
         [(GEN_LATENCY, B, H) for H in GEN_LATENCY_H for B in (1, 17, 200)] +
         [(GEN_LATENCY, B, 132) for B in (2560, 2561, 2577)] +
         [(GEN_TILED, B, H) for H in GEN_TILED_H for B in (1, 17, 512, 1000)])
CROSS = [(B, H) for H in (200, 300) for B in (511, 512, 8192, 8193)]
# (H, scale of the embeddings); B = 200, every form the width has
STRESS = [(H, s) for H in (20, 300, 516, 768) for s in (4.0, 30.0)] + [(20, 400.0), (300, 400.0)]
# (x 4: |z| to 11; x 30: to 84, a third of the pairs at exactly 1 and none at 0; x 400: |z| in the hundreds, both ends)
STRESS_B = 200
NONFINITE_H = (300, 516)
NONFINITE_B = 40                   # three tiles of 16 edges: the planted rows lie in the second, the third is ragged
# one-vs-many: (Q, C, H)
RANK_CASES = ([(Q, Cn, 300) for Q in (3, 4, 5) for Cn in (31, 32, 33)] +
              [(5, 33, H) for H in (1024, 1028, 2048, 2052, 4352)] + [(1, 1, 4352)])


def round_up16(x):
    return (x + 15) // 16 * 16


def forms_of(H):
    return (LATENCY, TILED, GEN_LATENCY, GEN_TILED) if round_up16(H) in (208, 304) else (GEN_LATENCY, GEN_TILED)


def expected_launch(form, B, H):
    """dict(form, gx, gy, ET) a case is ABOUT, restated from the kernels' comments (not read from the plan): the latency forms
    run min(tiles, 160) x NT waves, the tiled form 16 edges per workgroup up to 8192 edges and 32 beyond, the generic tiled
    form 16 edges per workgroup."""
    tiles, NT = (B + 15) // 16, round_up16(H) // 16
    if form in (LATENCY, GEN_LATENCY):
        return dict(form=form, gx=min(tiles, 160), gy=NT, ET=0)
    if form == TILED:
        ET = 16 if B <= 8192 else 32
        return dict(form=form, gx=(B + ET - 1) // ET, gy=1, ET=ET)
    return dict(form=form, gx=tiles, gy=1, ET=0)


def ident(case):
    form, B, H = case
    e = expected_launch(form, B, H)
    return "%s-H%d-B%d-grid%dx%d" % (FORM_NAMES[form], H, B, e["gx"], e["gy"]) + ("-ET%d" % e["ET"] if e["ET"] else "")


def plan(B, H, choice):
    """dict(form, KC, ET, gx, gy, threads, lds) of zt::affinity_kernel_plan (host code only: no GPU needed)"""
    from zebra_amd import _capi
    out = (C.c_int64 * 7)()
    assert _capi.hooks_lib().zt_test_affinity_plan(C.c_int64(B), C.c_int32(H), C.c_int32(choice), out) == _capi.ZT_OK
    return dict(zip(("form", "KC", "ET", "gx", "gy", "threads", "lds"), [int(v) for v in out]))


def oracle64():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import score_f64
    return score_f64


@functools.lru_cache(maxsize=None)
def weights(H):
    """(fc1_w [H][2H], fc1_b [H], fc2_w [1][H], fc2_b [1]) float32 of the weight generator, seed 7 + H as in the other
    scorer tests.  Three entries keep their drawn sign and get a fixed size, because the draw leaves them too small to be
    missed at some widths (|b1 w2| = 1.9e-5 at H = 344, 2.8e-5 at 304): fc1's bias of the LAST real unit (half the generator's
    range, 0.5 / sqrt(2H)), that unit's fc2 weight (one standard deviation, sqrt(2 / (H + 1))) and fc2's bias
    (0.5 / sqrt(H)).  A kernel that dropped one of them on a padded or last column then moves a logit by >= 0.5 / (H + 1)."""
    D, M = WIDTHS.get(H, (H // 2, 1))
    assert D * (M + 1) == H
    w = I.model_weights(D, 1, 20, M, 7 + H)
    out = (w["aff1_w"], w["aff1_b"], w["aff2_w"], w["aff2_b"])
    sized = lambda v, size: np.float32(size if v >= 0 else -size)
    out[1][H - 1] = sized(out[1][H - 1], 0.5 / np.sqrt(2.0 * H))
    out[2][0, H - 1] = sized(out[2][0, H - 1], np.sqrt(2.0 / (H + 1)))
    out[3][0] = sized(out[3][0], 0.5 / np.sqrt(H))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=6)
def embeddings(B, H, scale=1.0):
    """float32 [3B][H], this file's own draw: randn x 0.7 (x scale), the same for every form at a shape"""
    rng = np.random.RandomState(520000 + 1009 * H + B)
    e = (rng.standard_normal((3 * B, H)) * 0.7).astype(np.float32) * np.float32(scale)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=6)
def reference(B, H, scale=1.0):
    """(z64 [2B], p64 [2B]) of oracle/score_f64.py, computed once per shape"""
    z, p = oracle64().merge_layer_f64(embeddings(B, H, scale), *weights(H))
    z.setflags(write=False)
    p.setflags(write=False)
    return z, p


def bound(z64, p64):
    """per element; entries whose z64 is not finite get the floor alone"""
    zf = np.abs(z64[np.isfinite(z64)])
    tol_z = TOL_LINEAR * max(1.0, float(zf.max()) if zf.size else 0.0)
    return np.where(np.isfinite(z64), p64 * (1.0 - p64) * tol_z, 0.0) + ULP_P


def used(p, z64, p64, floor=0.0):
    """(max |p - p64|, largest share of the bound any element uses); floor: a scalar the bound is raised to (stress cases)"""
    err = np.abs(np.asarray(p, np.float64) - p64)
    return float(err.max()), float((err / np.maximum(bound(z64, p64), floor)).max())


def torch_compositions(emb, w):
    """torch's composition of the scorer on emb's device in emb's dtype -> (p of the reference's concatenated form, p of the
    split form W_a src + W_b dst + b1 the kernels compute), each [2B]"""
    W1, b1, W2, b2 = w
    B, H = emb.shape[0] // 3, emb.shape[1]
    with torch.no_grad():
        x = torch.cat([torch.cat([emb[:B], emb[:B]]), emb[B:]], dim=1)
        cat = (torch.relu(x @ W1.t() + b1) @ W2.t() + b2).squeeze(1)
        ps = emb[:B] @ W1[:, :H].t()
        pd = emb[B:] @ W1[:, H:].t()
        split = (torch.relu(torch.cat([ps, ps]) + pd + b1) @ W2.t() + b2).squeeze(1)
        return cat.sigmoid(), split.sigmoid()


def _t(a):
    return torch.from_numpy(np.array(a))


def _merge_layer(H, device):
    from zebra_amd.modules import MergeLayer
    m = MergeLayer(H, H, H, 1)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), weights(H)):
            p.copy_(_t(w))
    return m.to(device)


@functools.lru_cache(maxsize=4)
def scorer(H):
    """TGN.score_device / rank_scores on a MergeLayer of width H alone (some widths have no (D, M) a TGN takes)"""
    from zebra_amd.tgn import TGN
    holder = types.SimpleNamespace(affinity_score=_merge_layer(H, "cuda"), device=torch.device("cuda"))
    for name in ("_affinity_state", "score_device", "rank_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    return holder


def device_weights(sc):
    a = sc.affinity_score
    return a.fc1.weight, a.fc1.bias, a.fc2.weight, a.fc2.bias


class pinned:
    def __init__(self, choice):
        self.choice = choice

    def __enter__(self):
        from zebra_amd import _capi
        _capi.set_kernel_choice(_capi.CHOICE_SCORE, self.choice)

    def __exit__(self, *exc):
        from zebra_amd import _capi
        _capi.set_kernel_choice(_capi.CHOICE_SCORE, 0)


def as_tail(e):
    """e [3B][H] on the device as the LAST bytes of a larger tensor, NaN in front.  The front pad keeps the tensor's size off
    the allocator's 512-byte granule (128 floats past one), so what follows the block is the allocation's own slack."""
    n = e.size
    pad = 64 + (32 - (64 + n)) % 128
    big = torch.full((pad + n,), float("nan"), dtype=torch.float32, device="cuda")
    big[pad:] = _t(e).reshape(-1)
    return big[pad:].view(e.shape)


def as_head(e):
    """e as the FIRST bytes of a larger tensor, 64 NaN behind it"""
    n = e.size
    big = torch.full((n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    big[:n] = _t(e).reshape(-1)
    return big[:n].view(e.shape)


def score_twice(sc, e, form):
    """[2B] float32 numpy of score_device on `e` as a tail block; then zt_affinity itself on `e` as a head block into a
    probability array with SENTINEL behind it: the same bits, the sentinel untouched."""
    from zebra_amd import _capi
    B, H = e.shape[0] // 3, e.shape[1]
    with pinned(form):
        got = sc.score_device(as_tail(e))
        st, w, ready = sc._affinity_state(B)
        assert ready                                                  # (score_device has packed the weights)
        prob = torch.full((2 * B + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        _capi.check(_capi.lib().zt_affinity(_capi.ptr(as_head(e)), C.c_int64(B), C.c_int32(H), C.byref(w), _capi.ptr(prob),
                                            _capi.ptr(st["ws"]), C.c_int64(st["max_B"]), C.c_int32(1), _capi.stream_ptr()),
                    "zt_affinity")
        torch.cuda.synchronize()
    assert got.shape == (2 * B,) and got.dtype == torch.float32
    assert bool((prob[2 * B:] == SENTINEL).all()), "a write behind the 2B probabilities"
    assert torch.equal(got.view(torch.int32), prob[:2 * B].view(torch.int32)), "two runs, two results"     # (bits: NaN included)
    return got.cpu().numpy()


def assert_plan(form, B, H):
    got, want = plan(B, H, form), expected_launch(form, B, H)
    assert {k: got[k] for k in want} == want, "the plan does not run what this case is about"


# ------------------------------------------------------------------------------------------------------- the pair scorer --
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_pair_scorer_against_float64(case):
    form, B, H = case
    assert_plan(form, B, H)
    e = embeddings(B, H)
    z64, p64 = reference(B, H)
    sc = scorer(H)
    got = score_twice(sc, e, form)
    t_cat, t_split = torch_compositions(_t(e).cuda(), device_weights(sc))
    (e_hip, u_hip), (e_cat, u_cat), (e_split, u_split) = (used(x, z64, p64) for x in (got, t_cat.cpu().numpy(), t_split.cpu().numpy()))
    print("score %s max|z64| %.2f: HIP %.2e (%.3f of the bound), torch cat %.2e (%.3f), torch split %.2e (%.3f)"
          % (ident(case), np.abs(z64).max(), e_hip, u_hip, e_cat, u_cat, e_split, u_split))
    assert np.isfinite(got).all()
    assert u_cat <= 0.5 and u_split <= 0.5                             # the reference method has room
    assert u_hip <= 1.0


@pytest.mark.parametrize("B,H", CROSS, ids=["H%d-B%d" % (H, B) for B, H in CROSS])
def test_four_forms_agree_at_the_picks_seams(B, H):
    """B = 511 | 512 and 8192 | 8193: the library's pick changes form (and ET) there, so each side is otherwise run by one
    form only.  Pinned, all four run on both sides: each within the bound, any two within FORM_TOL."""
    e = embeddings(B, H)
    z64, p64 = reference(B, H)
    sc = scorer(H)
    got = {}
    for form in forms_of(H):
        assert_plan(form, B, H)
        got[form] = score_twice(sc, e, form)
        err, share = used(got[form], z64, p64)
        print("score forms H=%d B=%d %s: %.2e (%.3f of the bound)" % (H, B, FORM_NAMES[form], err, share))
        assert share <= 1.0, FORM_NAMES[form]
    for a in got:
        for b in got:
            if a < b:
                d = float(np.abs(got[a] - got[b]).max())
                print("score forms H=%d B=%d %s vs %s: %.2e" % (H, B, FORM_NAMES[a], FORM_NAMES[b], d))
                assert d <= FORM_TOL, (FORM_NAMES[a], FORM_NAMES[b])


@pytest.mark.parametrize("H,scale", STRESS, ids=["H%d-x%g" % c for c in STRESS])
def test_pair_scorer_saturates_as_float32_must(H, scale):
    """Embeddings x 4, x 30 and x 400: |z| in the tens and hundreds.  Finite and in [0, 1]; exactly 1 where z64 >= 18 (expf(-18) is
    below half an ulp of 1) and exactly 0 where z64 <= -104 (expf(104) overflows; 1 / inf); elsewhere four times torch's own
    float32 error on the case, the plain bound as floor -- the rule of the memory and attention stress cases."""
    B = STRESS_B
    e = embeddings(B, H, scale)
    z64, p64 = reference(B, H, scale)
    sc = scorer(H)
    t_cat, t_split = (t.cpu().numpy() for t in torch_compositions(_t(e).cuda(), device_weights(sc)))
    e_cat, u_cat = used(t_cat, z64, p64)
    e_split, u_split = used(t_split, z64, p64)
    one, zero = z64 >= 18.0, z64 <= -104.0
    print("score stress H=%d x%g: max|z64| %.1f, %d of %d at p = 1, %d at p = 0; torch cat %.2e (%.3f of the plain bound), split "
          "%.2e (%.3f)" % (H, scale, np.abs(z64).max(), one.sum(), 2 * B, zero.sum(), e_cat, u_cat, e_split, u_split))
    for form in forms_of(H):
        assert_plan(form, B, H)
        got = score_twice(sc, e, form)
        err, plain = used(got, z64, p64)
        _, share = used(got, z64, p64, floor=4.0 * e_cat)
        print("score stress H=%d x%g %s: HIP %.2e (%.3f of the plain bound, %.3f of the stress bound)"
              % (H, scale, FORM_NAMES[form], err, plain, share))
        assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0, FORM_NAMES[form]
        assert np.all(got[one] == 1.0) and np.all(got[zero] == 0.0), FORM_NAMES[form]
        assert share <= 1.0, FORM_NAMES[form]


def nonfinite_case(H):
    """(clean [3B][H], planted copy, {(block, edge): value}): one NaN and one +inf in one src, one dst and one neg row, six
    different edges of the second 16-edge tile.  NaN sits in a row's FIRST column, +inf in its LAST: the float4 a kernel would
    fetch for the row before it, were the ragged last k-chunk read unmasked, and the last chunk a k-round clamps to."""
    B = NONFINITE_B
    clean = embeddings(B, H)
    e = np.array(clean)
    plants = {(0, 17): np.nan, (1, 19): np.nan, (2, 22): np.nan, (0, 24): np.inf, (1, 27): np.inf, (2, 31): np.inf}
    for (blk, edge), v in plants.items():
        e[blk * B + edge, 0 if np.isnan(v) else H - 1] = v
    e.setflags(write=False)
    return clean, e, plants


def nonfinite_rule(H, plants, p_clean):
    """What the kernels give on the planted edges, as float64 [2B] with NaN where they give NaN.  The ReLU is written
    `h > 0 ? h : 0`, which sends NaN to 0.  A NaN in a row makes every hidden unit of its pairs NaN, hence 0: the pair scores
    sigmoid(b2).  +inf in column c makes unit u +inf where fc1's weight on c is positive (relu keeps it), -inf where negative
    (relu: 0) and NaN where it is a padded zero (relu: 0); the units times fc2's weights then hold +inf and -inf, whose sum is
    NaN -- unless all the kept ones have one sign, which gives 1 or 0."""
    W1, b1, W2, b2 = [np.asarray(a, np.float64) for a in weights(H)]
    B = NONFINITE_B
    want = np.array(p_clean, np.float64)
    sig_b2 = 1.0 / (1.0 + np.exp(-b2[0]))
    for (blk, edge), v in plants.items():
        pairs = [edge, B + edge] if blk == 0 else [edge if blk == 1 else B + edge]
        if np.isnan(v):
            val = sig_b2
        else:
            col = (H - 1) + (0 if blk == 0 else H)
            signs = np.sign(W2[0][W1[:, col] > 0])
            val = np.nan if (signs > 0).any() and (signs < 0).any() else (1.0 if (signs > 0).any() else 0.0)
        for i in pairs:
            want[i] = val
    return want


@pytest.mark.parametrize("H", NONFINITE_H)
def test_nonfinite_rows_stay_in_their_pairs(H):
    """Every other edge's two probabilities are those of the run without the planted values, bit for bit; the planted edges
    give the same value in every form of the width, and it is the one nonfinite_rule states (where torch gives NaN
    for a NaN row, zt_affinity gives sigmoid(b2))."""
    B = NONFINITE_B
    clean, e, plants = nonfinite_case(H)
    sc = scorer(H)
    hit = np.zeros(2 * B, bool)
    for (blk, edge) in plants:
        for i in ([edge, B + edge] if blk == 0 else [edge if blk == 1 else B + edge]):
            hit[i] = True
    first = None
    for form in forms_of(H):
        assert_plan(form, B, H)
        base = score_twice(sc, clean, form)
        got = score_twice(sc, e, form)
        assert np.array_equal(got[~hit], base[~hit]), FORM_NAMES[form]
        want = nonfinite_rule(H, plants, base)
        print("score nonfinite H=%d %s: planted edges give %s" % (H, FORM_NAMES[form], got[hit]))
        assert np.array_equal(np.isnan(got[hit]), np.isnan(want[hit])), FORM_NAMES[form]
        ok = hit & ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max() <= ULP_P, FORM_NAMES[form]
        if first is None:
            first = got
        assert np.array_equal(got[hit], first[hit], equal_nan=True), FORM_NAMES[form]


# ------------------------------------------------------------------------------------------------- the one-vs-many scorer --
@functools.lru_cache(maxsize=2)
def rank_inputs(Q, Cn, H, shared):
    """(emb_q [Q][H], emb_c [Nc][H], cand_idx [Q][C] or None, z64, p64).  With cand_idx: Nc != C, repeats inside a row, -1
    entries (the last slot of the first row among them), a row all present."""
    rng = np.random.RandomState(770000 + 10007 * Q + 101 * Cn + H + (1 if shared else 0))
    Nc = Cn if shared else max(1, Cn // 2 + 3)
    emb_q = (rng.standard_normal((Q, H)) * 0.7).astype(np.float32)
    emb_c = (rng.standard_normal((Nc, H)) * 0.7).astype(np.float32)
    idx = None
    if not shared:
        idx = rng.randint(0, Nc, (Q, Cn)).astype(np.int32)
        idx[rng.random_sample((Q, Cn)) < 0.2] = -1
        idx[0, Cn - 1] = -1
        idx[Q - 1] = np.arange(Cn) % Nc
    z, p = oracle64().rank_f64(emb_q, emb_c, idx, weights(H))
    return emb_q, emb_c, idx, z, p


@pytest.mark.parametrize("Q,Cn,H", RANK_CASES, ids=["Q%d-C%d-H%d" % c for c in RANK_CASES])
def test_rank_scorer_against_float64(Q, Cn, H):
    """k_rank_pairs tiles 4 queries x 32 candidate slots and takes H in chunks of 1024: Q = 3 | 4 | 5, C = 31 | 32 | 33, H =
    1024 exactly, 1028, 2048 | 2052, and 4352, the widest.  Shared candidates, then per-query indices."""
    sc = scorer(H)
    for shared in (True, False):
        emb_q, emb_c, idx, z64, p64 = rank_inputs(Q, Cn, H, shared)
        eq, ec = as_tail(emb_q), as_head(emb_c)
        ix = None if shared else _t(idx).cuda()
        got = sc.rank_scores(eq, ec, ix)
        again = sc.rank_scores(eq, ec, ix)
        torch.cuda.synchronize()
        assert got.shape == (Q, Cn) and got.dtype == torch.float32 and torch.equal(got, again)
        g = got.cpu().numpy()
        live = np.ones((Q, Cn), bool) if shared else idx >= 0
        assert np.all(g[~live] == 0.0) and np.all(p64[~live] == 0.0)
        with torch.no_grad():
            a = sc.affinity_score
            rows = ec.unsqueeze(0).expand(Q, -1, -1) if shared else ec[ix.long().clamp(min=0)]
            x = torch.cat([eq.unsqueeze(1).expand(-1, Cn, -1), rows], dim=2)
            t = a.fc2(torch.relu(a.fc1(x))).squeeze(2).sigmoid().cpu().numpy()
        e_hip, u_hip = used(g[live], z64[live], p64[live])
        e_t, u_t = used(t[live], z64[live], p64[live])
        print("rank Q=%d C=%d H=%d %s max|z64| %.2f: HIP %.2e (%.3f of the bound), torch %.2e (%.3f)"
              % (Q, Cn, H, "shared" if shared else "indexed", np.abs(z64[live]).max(), e_hip, u_hip, e_t, u_t))
        assert u_t <= 0.5
        assert u_hip <= 1.0
