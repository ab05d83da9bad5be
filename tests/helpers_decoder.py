"""Shared by tests/test_decoder_cpu.py and tests/test_decoder_gpu.py: the plain float64 restatement of the node-classification
decoder (the reference's MLP, utils/util.py:28-42, forward and backward with explicit dropout masks), the inputs of the GPU
cases, their bounds and the committed seeds.  Own code; the fixture tests/golden/g14_node_decoder.npz pins the restatement to
the reference."""
import functools

import numpy as np

H1, H2 = 80, 10
KEYS = ("fc_1.weight", "fc_1.bias", "fc_2.weight", "fc_2.bias", "fc_3.weight", "fc_3.bias")
TOL_LINEAR = 1e-5                  # of a linear layer's output, times max(1, max|ref|): test_scoring_f64_gpu.py
ULP_P = 2.0 ** -23                 # the final expf, division and rounding of a probability <= 1
TOL_DX = 1e-5                      # test_scoring_train_gpu.py: d_emb within 1e-5 * scale
TOL_G_ABS, TOL_G_REL = 1e-5, 1e-4  # ... a parameter gradient within 1e-5 + 1e-4 max|ref|
K_CHUNK = 256                      # csrc/decoder.hip DEC_KC: the widths below lie on each side of 256, 512, 768
ARR_ONE, ARR_FIVE = 1, 5
ROWS = {ARR_ONE: 64, ARR_FIVE: 16}  # rows per workgroup of the two arrangements
BIG_N = 16385                      # a grid of more than a thousand workgroups, a ragged last one
SPLIT_SEAM = 192                   # d_fc1_w: one product up to three 64-row steps, two partial products from 193 rows

FWD_N = (1, 15, 16, 17, 63, 64, 65, 200, 1000)
FWD_H = (4, 8, 12, 16, 20, 36, 52, 68, 200, 300, 344, 516, 768, 772, 4352)
# (arrangement pin, N, H): a sparse cross -- every N at H = 300, every H at N = 17, then the seams together
FWD_CASES = sorted(set([(a, N, 300) for a in (ARR_ONE, ARR_FIVE) for N in FWD_N] +
                       [(a, 17, H) for a in (ARR_ONE, ARR_FIVE) for H in FWD_H] +
                       [(a, N, H) for a in (ARR_ONE, ARR_FIVE) for N, H in ((65, 516), (200, 772), (64, 768), (1000, 20), (33, 4352))] +
                       [(a, BIG_N, 20) for a in (0, ARR_ONE)] + [(0, 200, 300), (0, 200, 516)]))
BWD_N = (1, 16, 17, 65, 200, 273, SPLIT_SEAM, SPLIT_SEAM + 1)
BWD_H = (4, 20, 300, 516)
BWD_CASES = [(N, H) for H in BWD_H for N in BWD_N] + [(17, 4352)]
# (p, N, H): the dropout seed is drop_seed(p, N, H)
DROP_CASES = [(p, N, H) for p in (0.3, 0.999) for N in (17, 200) for H in (20, 300)]


def drop_seed(p, N, H):
    return (0x5DEECE66D << 20) + int(1000 * p) * 1000003 + 131 * N + H


def fwd_id(case):
    a, N, H = case
    return "%s-N%d-H%d" % ({0: "plan", ARR_ONE: "one", ARR_FIVE: "five"}[a], N, H)


def expected_launch(arr, N, H):
    """What a forward case is ABOUT, restated from decoder.hip's comments (not read from the plan)."""
    if arr == 0:
        arr = ARR_FIVE                                           # the plan's pick at every N
    rows = ROWS[arr]
    return dict(arrangement=arr, waves=4 if arr == ARR_ONE else 5, rows=rows, k_chunk=K_CHUNK, grid=(N + rows - 1) // rows,
                chunks=(H + K_CHUNK - 1) // K_CHUNK)


def expected_split(N, H):
    steps = (N + 63) // 64
    max_split = max(1, min(8, 256 // ((H + 63) // 64)))
    split = min(max(1, steps // 2), max_split)
    kper = (steps + split - 1) // split * 64
    return (N + kper - 1) // kper, kper


# ---- the float64 restatement -------------------------------------------------------------------------------------------
def forward64(P, x, m1=None, m2=None):
    """dict(pre1, h1, pre2, h2, z) of z = fc3(m2 relu(fc2(m1 relu(fc1(x))))) in float64; m1 [N, 80] / m2 [N, 10] are the
    dropout masks (scale where kept, 0 where dropped; None: no dropout)."""
    W1, b1, W2, b2, W3, b3 = [np.asarray(P[k], np.float64) for k in KEYS]
    x = np.asarray(x, np.float64)
    pre1 = x @ W1.T + b1
    h1 = np.maximum(pre1, 0.0)
    if m1 is not None:
        h1 = h1 * np.asarray(m1, np.float64)
    pre2 = h1 @ W2.T + b2
    h2 = np.maximum(pre2, 0.0)
    if m2 is not None:
        h2 = h2 * np.asarray(m2, np.float64)
    z = (h2 @ W3.T + b3)[:, 0]
    return dict(pre1=pre1, h1=h1, pre2=pre2, h2=h2, z=z)


def backward64(P, x, f, dz, m1=None, m2=None):
    """The gradients of sum(dz * z): dict(d_x, g_<key> for the six parameters) in float64."""
    W1, b1, W2, b2, W3, b3 = [np.asarray(P[k], np.float64) for k in KEYS]
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    g = {"g_fc_3.weight": (dz[:, None] * f["h2"]).sum(0)[None, :], "g_fc_3.bias": np.array([dz.sum()])}
    dh2 = dz[:, None] * W3                                       # [N, 10]
    if m2 is not None:
        dh2 = dh2 * np.asarray(m2, np.float64)
    dh2 = dh2 * (f["pre2"] > 0)
    g["g_fc_2.weight"], g["g_fc_2.bias"] = dh2.T @ f["h1"], dh2.sum(0)
    dh1 = dh2 @ W2
    if m1 is not None:
        dh1 = dh1 * np.asarray(m1, np.float64)
    dh1 = dh1 * (f["pre1"] > 0)
    g["g_fc_1.weight"], g["g_fc_1.bias"] = dh1.T @ x, dh1.sum(0)
    g["d_x"] = dh1 @ W1
    return g


def sigmoid64(z):
    z = np.asarray(z, np.float64)
    return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def bce64(prob, labels):
    """(loss, dprob) of torch.nn.BCELoss() (mean) in float64, torch's clamps included."""
    x, y = np.asarray(prob, np.float64), np.asarray(labels, np.float64)
    with np.errstate(divide="ignore"):
        l1, l0 = np.maximum(np.log(x), -100.0), np.maximum(np.log(1.0 - x), -100.0)
    n = x.size
    return float(-(y * l1 + (1.0 - y) * l0).sum() / n), (x - y) / np.maximum((1.0 - x) * x, 1e-12) / n


# ---- inputs ------------------------------------------------------------------------------------------------------------
def draw_params(H, seed):
    """The six parameters (float32) as torch initialises a Linear layer -- uniform within 1 / sqrt(fan_in) -- from a numpy
    seed.  As in test_scoring_f64_gpu.py::weights, entries a kernel could drop on a last or padded column keep their drawn
    sign and get a fixed size, half the generator's range: the bias and the outgoing weights of unit 79 of layer 1, the bias
    and the outgoing weight of unit 9 of layer 2, and fc_3's bias."""
    rng = np.random.RandomState(seed)
    u = lambda fan_in, *shape: rng.uniform(-1.0, 1.0, shape).astype(np.float64) / np.sqrt(fan_in)
    P = {"fc_1.weight": u(H, H1, H), "fc_1.bias": u(H, H1), "fc_2.weight": u(H1, H2, H1), "fc_2.bias": u(H1, H2),
         "fc_3.weight": u(H2, 1, H2), "fc_3.bias": u(H2, 1)}
    fix = lambda v, size: np.where(v >= 0, size, -size)
    P["fc_1.bias"][H1 - 1] = fix(P["fc_1.bias"][H1 - 1], 0.5 / np.sqrt(H))
    P["fc_2.weight"][:, H1 - 1] = fix(P["fc_2.weight"][:, H1 - 1], 0.5 / np.sqrt(H1))
    P["fc_2.bias"][H2 - 1] = fix(P["fc_2.bias"][H2 - 1], 0.5 / np.sqrt(H1))
    P["fc_3.weight"][0, H2 - 1] = fix(P["fc_3.weight"][0, H2 - 1], 0.5 / np.sqrt(H2))
    P["fc_3.bias"][0] = fix(P["fc_3.bias"][0], 0.5 / np.sqrt(H2))
    return {k: v.astype(np.float32) for k, v in P.items()}


def draw_case(N, H, seed):
    """(P, x [N, H], dz [N]) float32 from one seed: x ~ 0.5 N(0, 1), dz ~ N(0, 1) / N"""
    P = draw_params(H, seed)
    rng = np.random.RandomState(seed + 77777)
    x = (0.5 * rng.randn(N, H)).astype(np.float32)
    dz = (rng.randn(N) / N).astype(np.float32)
    return P, x, dz


def margin_ok(f):
    """No float64 pre-activation of layer 1 or layer 2 within 1e-5 max(1, max|pre|) of zero: float32 may legitimately flip
    the ReLU of such a unit, which costs a whole gradient term."""
    for k in ("pre1", "pre2"):
        a = np.abs(f[k])
        if a.min() <= TOL_LINEAR * max(1.0, a.max()):
            return False
    return True


def seed_base(N, H, p=0.0):
    return 100000 + 1000 * N + H + int(1000 * p) * 7


def masks_of(p, N, H):
    if p == 0.0:
        return None, None
    from zebra_amd.decoder import decoder_dropout_mask
    return decoder_dropout_mask(drop_seed(p, N, H), p, N)


def first_good_seed(N, H, p=0.0, tries=64):
    """The first seed from the case's base whose draw satisfies margin_ok (under the case's dropout masks)"""
    m1, m2 = masks_of(p, N, H)
    base = seed_base(N, H, p)
    for s in range(base, base + tries):
        P, x, _ = draw_case(N, H, s)
        if margin_ok(forward64(P, x, m1, m2)):
            return s
    raise AssertionError("no seed within %d tries for N=%d H=%d p=%g" % (tries, N, H, p))


# (N, H, p) -> the seed first_good_seed returns: committed, re-derived by tests/test_decoder_cpu.py
# (as offsets from seed_base: 0 where the first draw already satisfies the condition)
SEED_OFFSETS = {(200, 4, 0.0): 1, (192, 4, 0.0): 1, (273, 20, 0.0): 5, (193, 20, 0.0): 1, (200, 300, 0.0): 3, (273, 300, 0.0): 1,
                (193, 300, 0.0): 3, (200, 20, 0.999): 1}
SEEDS = {(N, H, 0.0): seed_base(N, H) + SEED_OFFSETS.get((N, H, 0.0), 0) for N, H in BWD_CASES}
SEEDS.update({(N, H, p): seed_base(N, H, p) + SEED_OFFSETS.get((N, H, p), 0) for p, N, H in DROP_CASES})


@functools.lru_cache(maxsize=None)
def bwd_case(N, H, p=0.0):
    """(P, x, dz, m1, m2, forward64, backward64) of a backward or dropout case, at its committed seed"""
    P, x, dz = draw_case(N, H, SEEDS[(N, H, p)])
    m1, m2 = masks_of(p, N, H)
    f = forward64(P, x, m1, m2)
    return P, x, dz, m1, m2, f, backward64(P, x, f, dz, m1, m2)


@functools.lru_cache(maxsize=None)
def fwd_case(N, H):
    """(P, x, forward64) of a forward case: seed 7 + H for the parameters' draw, as the scorer tests"""
    P, x, _ = draw_case(N, H, 7 + H)
    return P, x, forward64(P, x)


def logit_bound(z64):
    return TOL_LINEAR * max(1.0, float(np.abs(z64).max()))


def prob_bound(z64):
    p = sigmoid64(z64)
    return p * (1.0 - p) * logit_bound(z64) + ULP_P


def grad_ok(got, want):
    """|got - want| <= 1e-5 + 1e-4 max|want| for a parameter gradient; returns (ok, worst / bound)"""
    want = np.asarray(want, np.float64)
    bound = TOL_G_ABS + TOL_G_REL * float(np.abs(want).max())
    err = float(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want).max())
    return err <= bound, err / bound


def dx_ok(got, want):
    """|got - want| <= 1e-5 * scale, scale = max(1, max|want|) (test_scoring_train_gpu.py's d_emb tolerance)"""
    want = np.asarray(want, np.float64)
    bound = TOL_DX * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    return err <= bound, err / bound
