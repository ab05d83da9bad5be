"""k_temporal_attention (csrc/attention.hip) at every tiling zt::attention_plan makes, against the plain float64 restatement
oracle/attention_np.py (pinned to torch's float64 layer at these very shapes in tests/test_attention_cpu.py).

Shapes: the accepted rows of the plan table in test_attention_cpu.py -- the 16-row cap on queries per workgroup (k <= 5), a tile
with padded key rows inside it (k = 6: 78 of 80), one query row over 3 and over 5 M-tiles (k = 41, 80), heads 1, 2, 3 and 4,
F = 0, an output width that decides ldq (out = 70), and the widest tiles that fit (D = 172 at k = 16, D = T = 224 at k = 10).
Rows: N = 2 rq + 1 with rq read from the plan -- two full tiles and a ragged one; rq = 1 has no ragged tile and three rows
cannot hold the five kinds of row below, so those cases run N = 5.  Each shape family also runs N = 1.

Inputs: this file's own seeded generator (make_case), not inputs.attention_inputs: edge features are non-zero at every F, the
query's time columns are cosines (not all ones, which would hide a query time column that multiplied nothing), neighbour
times lie in [-1, 1].  The mask of every case holds (SPECIAL, checked without a GPU): a row without any neighbour as the last
row of a tile, its slot-0 key scaled by 1e3; one as the first row of a tile (rq >= 3); one at row N - 1 (the first row of the
ragged tile); a row with only slot 0 masked; a row with exactly one neighbour, in the last slot; a row with no slot masked.
At k = 1 a row has its neighbour or has none.  For rows without a neighbour attn_w is exactly 0 and out is the merger applied to
[0 | src] (in float64), the row with the 1e3 key included.

Tolerances against float64, none fitted to the kernel:
  out     1e-5 max(1, max|ref|)   what test_memory_f64_gpu.py asserts for a float32 cell fed by sums of up to ~1 000 terms
  attn_w  1e-6 absolute           five times the worst error of torch's float32 layer on the CPU over these shapes
torch's own float32 layer on the device, on the same inputs, is held to HALF of each.  Stress cases (node and edge features
x 4 or x 8: scores in the tens, a softmax close to one-hot): four times the error torch's float32 layer on the device makes on
the same case, the plain tolerance as floor; every output finite.

Every HIP forward is counted at lib().zt_temporal_attention: one call per forward, none for forward_torch, none for a
refused shape.

Measured on an MI355X (max |error| against float64; the table per case is in DESIGN.md, "The attention layer against
float64"): out -- kernel <= 2.1e-06, torch <= 2.0e-06, tolerance >= 1.5e-05; attn_w -- kernel <= 2.2e-07 (at (172, 172, 172), where
torch makes 3.2e-08), torch <= 1.3e-07, tolerance 1e-06.  Stress cases -- out: kernel 9.6e-06 ... 2.8e-05, torch 9.8e-06 ... 2.1e-05,
the kernel at most 2.6 times torch; attn_w: kernel <= 1.6e-06, torch <= 1.1e-06, at most 1.7 times.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

OUT_TOL, AW_TOL = 1e-5, 1e-6
# (D, F, T, heads, out_dim, k); the merger's hidden width is D (TemporalAttentionLayer builds it so)
CASES = [
    (20, 4, 12, 4, 20, 1), (20, 4, 12, 4, 20, 3), (20, 4, 12, 4, 20, 5), (20, 4, 12, 4, 20, 6),
    (20, 4, 12, 2, 20, 16), (20, 4, 12, 2, 20, 17), (20, 4, 12, 2, 20, 40), (20, 4, 12, 2, 20, 41), (20, 4, 12, 2, 20, 80),
    (20, 7, 13, 3, 70, 5), (20, 0, 12, 1, 20, 5),
    (100, 172, 100, 2, 100, 20), (100, 172, 100, 2, 100, 48),
    (128, 16, 128, 2, 128, 20), (172, 172, 172, 2, 172, 16), (224, 1, 224, 2, 224, 10),
]
# the first case of each shape family: run once more with one row
FAMILIES = [(20, 4, 12, 4, 20, 5), (20, 7, 13, 3, 70, 5), (20, 0, 12, 1, 20, 5), (100, 172, 100, 2, 100, 20),
            (128, 16, 128, 2, 128, 20), (172, 172, 172, 2, 172, 16), (224, 1, 224, 2, 224, 10)]
# (case, scale of the node and edge features)
STRESS = [((100, 172, 100, 2, 100, 20), 4.0), ((100, 1, 100, 2, 100, 40), 4.0), ((20, 4, 12, 4, 20, 5), 8.0)]
# refused by the plan; the last two cannot be built as a torch layer (E % heads != 0) and are put to the library alone
REFUSED = [
    (20, 4, 12, 2, 20, 81), (100, 172, 100, 2, 100, 49), (100, 1, 100, 2, 100, 80), (172, 172, 172, 2, 172, 17),
    (228, 1, 228, 2, 228, 10), (240, 1, 240, 2, 240, 10), (256, 1, 256, 2, 256, 10), (256, 172, 256, 2, 256, 1),
    (20, 4, 12, 5, 20, 5), (20, 4, 12, 3, 20, 5),
]
SENTINEL = 777.0


def ident(c):
    return "-".join(str(v) for v in c)


def _oracle():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import attention_np
    return attention_np


def plan(D, F, T, heads, out_dim, k):
    """dict(supported, rq, mt, lds) of zt::attention_plan (host code only: no GPU needed)"""
    from zebra_amd import _capi
    o = (C.c_int64 * 4)()
    rc = _capi.hooks_lib().zt_test_attention_plan(C.c_int32(D), C.c_int32(F), C.c_int32(T), C.c_int32(heads), C.c_int32(D),
                                                  C.c_int32(out_dim), C.c_int32(k), o)
    assert rc == _capi.ZT_OK
    return dict(zip(("supported", "rq", "mt", "lds"), [int(v) for v in o]))


def rows_of(rq):
    return 2 * rq + 1 if rq > 1 else 5


def make_weights(D, F, T, out_dim, seed):
    """Parameters of TemporalAttentionLayer(D, D, F, T, output_dimension=out_dim) in torch layout (inputs.attention_weights
    with an output width of its own)."""
    rng = np.random.RandomState(seed)
    E, K = D + T, D + T + F
    mat = lambda o, i: (rng.standard_normal((o, i)) * np.sqrt(2.0 / (o + i))).astype(np.float32)
    vec = lambda n: rng.uniform(-0.1, 0.1, n).astype(np.float32)
    return dict(q_w=mat(E, E), k_w=mat(E, K), v_w=mat(E, K), in_b=vec(3 * E), out_w=mat(E, E), out_b=vec(E),
                m1_w=mat(D, E + D), m1_b=vec(D), m2_w=mat(out_dim, D), m2_b=vec(out_dim))


def special_rows(rq, N, k):
    """kind -> row.  `none_*`: rows without any neighbour, by where they sit in their tile."""
    none = {"none_last_of_tile_key_1e3": rq - 1, "none_at_end": N - 1}
    if rq >= 3:
        none["none_first_of_tile"] = rq
    free = [r for r in range(N) if r not in none.values()]
    if k == 1:
        return dict(none, all_neighbours=free[0])
    return dict(none, only_slot0_masked=free[0], one_neighbour_last_slot=free[1], all_neighbours=free[2])


@functools.lru_cache(maxsize=None)
def make_case(D, F, T, heads, out_dim, k, scale=1.0):
    """The one seeded generator of this file and of test_attention_cpu.py (numpy arrays; nobody writes to them)."""
    rq = plan(D, F, T, heads, out_dim, k)["rq"]
    N = rows_of(rq)
    seed = 11000 + 131 * D + 17 * F + 5 * T + 1009 * heads + 3 * out_dim + k
    rng = np.random.RandomState(seed)
    src = rng.standard_normal((N, D)).astype(np.float32)
    src_t = np.cos(rng.standard_normal((N, 1, T)) * 5).astype(np.float32)
    nbr = rng.standard_normal((N, k, D)).astype(np.float32)
    nbr_t = np.cos(rng.standard_normal((N, k, T)) * 5).astype(np.float32)
    edge = rng.standard_normal((N, k, F)).astype(np.float32)
    mask = rng.random_sample((N, k)) < 0.4
    sp = special_rows(rq, N, k)
    for kind, r in sp.items():
        mask[r] = kind.startswith("none")
    if k > 1:
        mask[sp["only_slot0_masked"], 0] = True
        mask[sp["one_neighbour_last_slot"], :k - 1] = True
    if scale != 1.0:
        src, nbr, edge = src * np.float32(scale), nbr * np.float32(scale), edge * np.float32(scale)
    r = sp["none_last_of_tile_key_1e3"]
    nbr[r, 0] *= 1e3
    edge[r, 0] *= 1e3
    nbr_t[r, 0] *= 1e3
    x = (src, src_t, nbr, nbr_t, edge, mask)
    for a in x:
        a.setflags(write=False)
    return dict(x=x, w=make_weights(D, F, T, out_dim, seed + 1), N=N, rq=rq, special=sp, heads=heads,
                dims=(D, F, T, heads, out_dim, k))


@functools.lru_cache(maxsize=None)
def reference(D, F, T, heads, out_dim, k, scale=1.0):
    """(out, attn_w) in float64, computed once per case"""
    c = make_case(D, F, T, heads, out_dim, k, scale)
    out, aw = _oracle().temporal_attention(*c["x"], c["w"], heads, f64=True)
    assert out.dtype == np.float64 and aw.dtype == np.float64
    out.setflags(write=False)
    aw.setflags(write=False)
    return out, aw


def merger_of_zero(c):
    """merger([0 | src]) in float64: what a row without any neighbour must give"""
    w, src = c["w"], c["x"][0].astype(np.float64)
    E = w["q_w"].shape[0]
    h = np.maximum(src @ w["m1_w"].astype(np.float64)[:, E:].T + w["m1_b"].astype(np.float64), 0)
    return h @ w["m2_w"].astype(np.float64).T + w["m2_b"].astype(np.float64)


def build_layer(D, F, T, heads, out_dim, w, dtype=torch.float32):
    from zebra_amd.modules import TemporalAttentionLayer
    layer = TemporalAttentionLayer(D, D, F, T, output_dimension=out_dim, n_head=heads, dropout=0.1).eval()
    mha = layer.multi_head_target
    t = lambda kk: torch.from_numpy(w[kk])
    with torch.no_grad():
        if F == 0:          # kdim == embed_dim: torch keeps one packed weight
            mha.in_proj_weight.copy_(torch.cat([t("q_w"), t("k_w"), t("v_w")]))
        else:
            for p, kk in ((mha.q_proj_weight, "q_w"), (mha.k_proj_weight, "k_w"), (mha.v_proj_weight, "v_w")):
                p.copy_(t(kk))
        for p, kk in ((mha.in_proj_bias, "in_b"), (mha.out_proj.weight, "out_w"), (mha.out_proj.bias, "out_b"),
                      (layer.merger.fc1.weight, "m1_w"), (layer.merger.fc1.bias, "m1_b"),
                      (layer.merger.fc2.weight, "m2_w"), (layer.merger.fc2.bias, "m2_b")):
            p.copy_(t(kk))
    return layer.to(dtype)


def torch_forward(layer, x, device="cpu", dtype=torch.float32):
    """forward_torch on `device`; numpy float64 arrays back"""
    ten = [torch.from_numpy(np.array(a)).to(device) for a in x]
    ten = [a if a.dtype == torch.bool else a.to(dtype) for a in ten]
    with torch.no_grad():
        out, aw = layer.to(device).forward_torch(*ten)
    return out.double().cpu().numpy(), aw.double().cpu().numpy()


def hip_forward(layer, x, rows=slice(None)):
    ten = [torch.from_numpy(np.array(a[rows])).cuda() for a in x]
    with torch.no_grad():
        out, aw = layer(*ten)
    torch.cuda.synchronize()
    return out.cpu().numpy(), aw.cpu().numpy()


def err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


@pytest.fixture
def attention_calls(monkeypatch):
    """[n]: calls of lib().zt_temporal_attention from here on"""
    from zebra_amd import _capi
    lib = _capi.lib()
    calls, fwd = [0], lib.zt_temporal_attention

    def counted(*args):
        calls[0] += 1
        return fwd(*args)

    monkeypatch.setattr(lib, "zt_temporal_attention", counted)
    return calls


def _check_rows_without_neighbour(c, out, aw, tol_out):
    want = merger_of_zero(c)
    for kind, r in c["special"].items():
        if kind.startswith("none"):
            assert np.all(aw[r] == 0.0), kind
            assert err(out[r], want[r]) <= tol_out, kind


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_attention_against_float64(case, attention_calls):
    c = make_case(*case)
    ref_out, ref_aw = reference(*case)
    tol_out = OUT_TOL * max(1.0, np.abs(ref_out).max())
    layer = build_layer(*case[:5], c["w"]).cuda()
    out, aw = hip_forward(layer, c["x"])
    assert attention_calls[0] == 1                                  # the HIP kernel is what ran ...
    t_out, t_aw = torch_forward(layer, c["x"], "cuda")
    assert attention_calls[0] == 1                                  # ... and forward_torch is not it
    e = (err(out, ref_out), err(aw, ref_aw), err(t_out, ref_out), err(t_aw, ref_aw))
    print("attention %s N=%d rq=%d: out kernel %.2e torch %.2e (max|ref| %.2f), attn_w kernel %.2e torch %.2e"
          % (ident(case), c["N"], c["rq"], e[0], e[2], np.abs(ref_out).max(), e[1], e[3]))
    assert out.shape == ref_out.shape and aw.shape == ref_aw.shape and out.dtype == aw.dtype == np.float32
    assert np.isfinite(out).all() and np.isfinite(aw).all()
    assert e[2] <= 0.5 * tol_out and e[3] <= 0.5 * AW_TOL           # the reference method has room
    assert e[0] <= tol_out
    assert e[1] <= AW_TOL
    _check_rows_without_neighbour(c, out, aw, tol_out)
    out2, aw2 = hip_forward(layer, c["x"])                          # the same bits twice
    assert attention_calls[0] == 2
    assert np.array_equal(out, out2) and np.array_equal(aw, aw2)


@pytest.mark.parametrize("case", FAMILIES, ids=ident)
def test_attention_one_row(case, attention_calls):
    """N = 1: the case's row with every neighbour, alone (one workgroup, one row of its tile)."""
    c = make_case(*case)
    ref_out, ref_aw = reference(*case)
    r = c["special"]["all_neighbours"]
    out, aw = hip_forward(build_layer(*case[:5], c["w"]).cuda(), c["x"], slice(r, r + 1))
    assert attention_calls[0] == 1
    assert out.shape == (1, case[4]) and aw.shape == (1, case[5])
    assert err(out, ref_out[r:r + 1]) <= OUT_TOL * max(1.0, np.abs(ref_out[r]).max())
    assert err(aw, ref_aw[r:r + 1]) <= AW_TOL


@pytest.mark.parametrize("case,scale", STRESS, ids=[ident(c) + "-x%g" % s for c, s in STRESS])
def test_attention_stress(case, scale, attention_calls):
    c = make_case(*case, scale)
    ref_out, ref_aw = reference(*case, scale)
    layer = build_layer(*case[:5], c["w"]).cuda()
    out, aw = hip_forward(layer, c["x"])
    t_out, t_aw = torch_forward(layer, c["x"], "cuda")
    assert attention_calls[0] == 1
    e = (err(out, ref_out), err(aw, ref_aw), err(t_out, ref_out), err(t_aw, ref_aw))
    print("attention stress %s x%g: out kernel %.2e torch %.2e (max|ref| %.2f), attn_w kernel %.2e torch %.2e; max attn_w %.4f"
          % (ident(case), scale, e[0], e[2], np.abs(ref_out).max(), e[1], e[3], ref_aw.max()))
    assert np.isfinite(out).all() and np.isfinite(aw).all()
    tol_out = max(4.0 * e[2], OUT_TOL * max(1.0, np.abs(ref_out).max()))
    assert e[0] <= tol_out
    assert e[1] <= max(4.0 * e[3], AW_TOL)
    _check_rows_without_neighbour(c, out, aw, tol_out)


def test_workspace_grows_and_is_reused(attention_calls):
    """One layer at k = 5, k = 40, k = 5 again: each result is a fresh layer's, bit for bit.  (The workspace holds the padded
    weights only, so its size does not depend on k today: allocated at the first call, reused by the other two.)"""
    base = (20, 4, 12, 2, 20)
    w = make_case(*base, 5)["w"]
    layer = build_layer(*base, w).cuda()
    sizes = []
    for k in (5, 40, 5):
        x = make_case(*base, k)["x"]
        got = hip_forward(layer, x)
        sizes.append(layer._ws.numel())
        want = hip_forward(build_layer(*base, w).cuda(), x)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
        ref_out, ref_aw = _oracle().temporal_attention(*x, w, 2, f64=True)
        assert err(got[0], ref_out) <= OUT_TOL * max(1.0, np.abs(ref_out).max()) and err(got[1], ref_aw) <= AW_TOL, k
    assert attention_calls[0] == 6
    assert sizes[0] <= sizes[1] == sizes[2]


def test_weight_changed_in_place_is_followed(attention_calls):
    case = (20, 7, 13, 3, 70, 5)
    c = make_case(*case)
    layer = build_layer(*case[:5], c["w"]).cuda()
    first = hip_forward(layer, c["x"])
    w2 = dict(c["w"])
    for kk in ("k_w", "v_w", "m2_w", "in_b"):
        w2[kk] = (c["w"][kk] * np.float32(1.5)).astype(np.float32)
    with torch.no_grad():
        layer.multi_head_target.k_proj_weight.mul_(1.5)
        layer.multi_head_target.v_proj_weight.mul_(1.5)
        layer.multi_head_target.in_proj_bias.mul_(1.5)
        layer.merger.fc2.weight.mul_(1.5)
    second = hip_forward(layer, c["x"])
    assert attention_calls[0] == 2
    ref_out, ref_aw = _oracle().temporal_attention(*c["x"], w2, case[3], f64=True)
    assert err(second[0], ref_out) <= OUT_TOL * max(1.0, np.abs(ref_out).max())
    assert err(second[1], ref_aw) <= AW_TOL
    assert err(first[0], ref_out) > 100 * OUT_TOL and err(first[1], ref_aw) > 100 * AW_TOL      # the change is a visible one


@pytest.mark.parametrize("case", REFUSED, ids=ident)
def test_refused_shapes_launch_nothing(case, attention_calls):
    """A refusal by host code, before any launch: ZT_ERR_UNSUPPORTED from the library with the outputs untouched, the
    module's ValueError with no call of the library's forward at all."""
    from zebra_amd import _capi
    D, F, T, heads, out_dim, k = case
    assert plan(*case)["supported"] == 0
    lib, N, E = _capi.lib(), 3, D + T
    assert lib.zt_attention_workspace_bytes(*[C.c_int32(v) for v in (D, F, T, heads, D, out_dim, k)]) == -1
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    ten = [z(N, D), z(N, T), z(N, k, D), z(N, k, max(F, 1)), z(N, k, T), torch.zeros((N, k), dtype=torch.uint8, device="cuda")]
    wt = [z(E, E), z(E, D + F + T), z(E, D + F + T), z(3 * E), z(E, E), z(E), z(D, E + D), z(D), z(out_dim, D), z(out_dim)]
    out = torch.full((N, out_dim), SENTINEL, dtype=torch.float32, device="cuda")
    aw = torch.full((N, k), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")       # never written: the refusal comes first
    weights = _capi.AttnWeights(*[_capi.ptr(t) for t in wt])
    torch.cuda.synchronize()
    rc = lib.zt_temporal_attention(*[_capi.ptr(t) for t in ten], C.c_int64(N), C.c_int32(k), C.c_int32(D), C.c_int32(F),
                                   C.c_int32(T), C.c_int32(heads), C.c_int32(D), C.c_int32(out_dim), C.byref(weights),
                                   _capi.ptr(out), _capi.ptr(aw), _capi.ptr(ws), _capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _capi.ZT_ERR_UNSUPPORTED
    assert b"unsupported shape" in lib.zt_last_error()
    assert bool((out == SENTINEL).all()) and bool((aw == SENTINEL).all()) and bool((ws == 0x5A).all())
    assert attention_calls[0] == 1
    if (D + T) % heads == 0:
        from zebra_amd.modules import TemporalAttentionLayer
        layer = TemporalAttentionLayer(D, D, F, T, output_dimension=out_dim, n_head=heads).eval().cuda()
        with pytest.raises(ValueError, match="unsupported shape"), torch.no_grad():
            layer(ten[0], ten[1].reshape(N, 1, T), ten[2], ten[4], ten[3][:, :, :F], ten[5].bool())
        assert attention_calls[0] == 1                              # the module asked zt_attention_workspace_bytes and stopped
        assert layer._ws is None
