"""The attention layer's training kernels (csrc/attention_train.hip) on the device: zt_attention_train_forward and
zt_attention_train_backward put to the library directly, and through TemporalAttentionLayer.fused_training.

Shapes: the small end of tests/test_attention_f64_gpu.py's table, where every tiling seam sits -- the 16-row cap on queries per
workgroup (k = 1, 5), padded key rows inside a tile (k = 6), one query row over several M-tiles (k = 17: rq = 4; k = 41, 80:
rq = 1 over 3 and 5 tiles), heads 4, 2, 3 and 1, F = 0 (one packed in_proj_weight), an output width that decides ldq
(out = 70) -- and one realistic tile (D = T = 100, F = 172, k = 20).  Rows and inputs are that file's (make_case: N = 2 rq + 1,
or 5 where rq = 1, with its special rows); d_out is seeded normal.

Reference: helpers_attention_train.forward in float64 on the CPU with the keep-mask modules.dropout_mask gives for the seed
(pinned to torch's float64 layer in test_attention_train_cpu.py).  Bound per tensor, out and each of the 15 gradients:
max(1e-5 max(1, max|ref|), 4 e32), e32 the error the same helper makes in float32 on the device on the same case and mask --
the rule test_attention_f64_gpu.py applies to its stress cases, with its OUT_TOL as the floor.  attn_w: that file's AW_TOL.
Measured errors: DESIGN.md, "The attention layer's training step"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers_attention_train as H
import test_attention_f64_gpu as G

pytestmark = pytest.mark.gpu

CASES = [(20, 4, 12, 4, 20, 1), (20, 4, 12, 4, 20, 5), (20, 4, 12, 4, 20, 6),
         (20, 4, 12, 2, 20, 17), (20, 4, 12, 2, 20, 41), (20, 4, 12, 2, 20, 80),
         (20, 7, 13, 3, 70, 5), (20, 0, 12, 1, 20, 5), (100, 172, 100, 2, 100, 20)]
REFUSED = (100, 172, 100, 2, 100, 49)
DROPS = (0.0, 0.3)
SEED = 0x1234_5678_9ABC
SENTINEL = 777.0
# zt_attn_grads' members in order, by the helper's names
GRAD_ORDER = ("src", "src_t", "nbr", "edge", "nbr_t") + H.W_KEYS
CASE_DROPS = [(c, p) for c in CASES for p in DROPS]
IDS = ["%s-p%g" % (G.ident(c), p) for c, p in CASE_DROPS]


def _capi():
    from zebra_amd import _capi
    return _capi


@functools.lru_cache(maxsize=None)
def d_out_of(case):
    c = G.make_case(*case)
    a = np.random.RandomState(77 + case[5]).standard_normal((c["N"], case[4])).astype(np.float32)
    a.setflags(write=False)
    return a


def keep_of(case, p):
    c = G.make_case(*case)
    return None if p == 0 else H.keep_mask(SEED, p, c["N"], case[3], case[5])


@functools.lru_cache(maxsize=None)
def reference(case, p):
    """float64 on the CPU, once per (case, p): name -> array"""
    ref = H.run(G.make_case(*case), d_out_of(case), keep_of(case, p), torch.float64)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def helper_f32_error(case, p):
    """e32 per tensor: the helper in float32 on the device against the float64 reference"""
    got = H.run(G.make_case(*case), d_out_of(case), keep_of(case, p), torch.float32, "cuda")
    ref = reference(case, p)
    return {kk: H.err(got[kk], ref[kk]) for kk in ref}


def bound(case, p, kk):
    ref = reference(case, p)[kk]
    return max(G.OUT_TOL * max(1.0, float(np.abs(ref).max(initial=0.0))), 4.0 * helper_f32_error(case, p)[kk])


def grad_shapes(case, N):
    D, F, T, heads, out_dim, k = case
    E, Ek = D + T, D + F + T
    return dict(src=(N, D), src_t=(N, T), nbr=(N, k, D), edge=(N, k, F), nbr_t=(N, k, T), q_w=(E, E), k_w=(E, Ek), v_w=(E, Ek),
                in_b=(3 * E,), out_w=(E, E), out_b=(E,), m1_w=(D, E + D), m1_b=(D,), m2_w=(out_dim, D), m2_b=(out_dim,))


class Device:
    """A case on the device, in the C entry points' argument order"""

    def __init__(self, case):
        capi = _capi()
        self.case, self.c = case, G.make_case(*case)
        D, F, T, heads, out_dim, k = case
        src, src_t, nbr, nbr_t, edge, mask = self.c["x"]
        N = self.N = self.c["N"]
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.ten = [dev(src), dev(src_t.reshape(N, T)), dev(nbr), dev(edge), dev(nbr_t), dev(mask.astype(np.uint8))]
        self.wts = [dev(self.c["w"][kk]) for kk in H.W_KEYS]
        self.weights = capi.AttnWeights(*[capi.ptr(t) for t in self.wts])
        self.plan = capi.attention_train_plan(D, F, T, heads, D, out_dim, k)
        assert self.plan["supported"] == 1 and self.plan["rq"] == self.c["rq"]
        self.dims = [C.c_int64(N), C.c_int32(k)] + [C.c_int32(v) for v in (D, F, T, heads, D, out_dim)]

    def head(self, p):
        capi = _capi()
        return [capi.ptr(t) for t in self.ten] + self.dims + [C.byref(self.weights), C.c_float(p), C.c_uint64(SEED if p else 0)]

    def forward(self, p):
        capi = _capi()
        N, k, out_dim = self.N, self.case[5], self.case[4]
        out = torch.full((N, out_dim), SENTINEL, dtype=torch.float32, device="cuda")
        aw = torch.full((N, k), SENTINEL, dtype=torch.float32, device="cuda")
        saved = torch.empty(N * self.plan["saved_row"] // 4, dtype=torch.float32, device="cuda")
        ws = torch.empty(self.plan["ws_fixed"], dtype=torch.uint8, device="cuda")
        capi.check(capi.lib().zt_attention_train_forward(*self.head(p), capi.ptr(out), capi.ptr(aw), capi.ptr(saved), capi.ptr(ws),
                                                         capi.stream_ptr()), "zt_attention_train_forward")
        torch.cuda.synchronize()
        return out, aw, saved

    def backward(self, p, saved, names=GRAD_ORDER, buffers=None):
        """name -> float32 tensor for the gradients asked for (NULL for the rest); buffers: name -> tensor to write into"""
        capi = _capi()
        shapes = grad_shapes(self.case, self.N)
        got = {}
        for kk in names:
            got[kk] = buffers[kk] if buffers else torch.full(shapes[kk], SENTINEL, dtype=torch.float32, device="cuda")
        gs = capi.AttnGrads(*[capi.ptr(got.get(kk)) for kk in GRAD_ORDER])
        ws = torch.empty(self.plan["ws_fixed"] + self.N * self.plan["ws_row"], dtype=torch.uint8, device="cuda")
        d_out = torch.from_numpy(np.array(d_out_of(self.case))).cuda()
        capi.check(capi.lib().zt_attention_train_backward(*self.head(p), capi.ptr(saved), capi.ptr(d_out), C.byref(gs), capi.ptr(ws),
                                                          capi.stream_ptr()), "zt_attention_train_backward")
        torch.cuda.synchronize()
        return got


@functools.lru_cache(maxsize=None)
def hip_result(case, p):
    """out, attn_w and the 15 gradients of the kernels, once per (case, p): name -> float32 numpy array (helper's shapes)"""
    dv = Device(case)
    out, aw, saved = dv.forward(p)
    grads = dv.backward(p, saved)
    res = {"out": out, "attn_w": aw}
    res.update(grads)
    res = {kk: v.cpu().numpy() for kk, v in res.items()}
    res["src_t"] = res["src_t"].reshape(dv.N, 1, case[2])
    return res


@pytest.mark.parametrize("case", CASES, ids=G.ident)
def test_forward_without_dropout_is_the_eval_kernel_bit_for_bit(case):
    c = G.make_case(*case)
    layer = G.build_layer(*case[:5], c["w"]).cuda()
    e_out, e_aw = G.hip_forward(layer, c["x"])
    got = hip_result(case, 0.0)
    assert got["out"].dtype == got["attn_w"].dtype == np.float32
    assert np.array_equal(got["out"], e_out) and np.array_equal(got["attn_w"], e_aw)


@pytest.mark.parametrize("case,p", CASE_DROPS, ids=IDS)
def test_gradients_against_float64(case, p):
    ref, got, e32 = reference(case, p), hip_result(case, p), helper_f32_error(case, p)
    lines, bad = [], []
    for kk in ("out",) + H.GRAD_KEYS:
        e, b = H.err(got[kk], ref[kk]), bound(case, p, kk)
        lines.append("%s %.2e (helper f32 %.2e, max|ref| %.3g, bound %.2e)" % (kk, e, e32[kk], np.abs(ref[kk]).max(initial=0), b))
        assert got[kk].shape == ref[kk].shape, kk
        if not e <= b:
            bad.append(kk)
    e_aw = H.err(got["attn_w"], ref["attn_w"])
    print("attention train %s p=%g N=%d: %s; attn_w %.2e (helper f32 %.2e)"
          % (G.ident(case), p, ref["out"].shape[0], "; ".join(lines), e_aw, e32["attn_w"]))
    assert not bad, bad
    assert e_aw <= max(G.AW_TOL, 4.0 * e32["attn_w"])
    if p:
        assert H.err(reference(case, 0.0)["out"], ref["out"]) > 100 * G.OUT_TOL        # the mask is a visible one


@pytest.mark.parametrize("case,p", CASE_DROPS, ids=IDS)
def test_exact_zeros_and_finite(case, p):
    c, got = G.make_case(*case), hip_result(case, p)
    mask = c["x"][5]
    for kk, v in got.items():
        assert np.isfinite(v).all(), kk
        assert not (v == SENTINEL).any() or v.size == 0, kk                           # every element was written
    for kk in ("nbr", "edge", "nbr_t"):
        inv = mask.all(axis=1)
        m = mask.copy()
        m[inv, 0] = False
        assert np.all(got[kk][m] == 0.0), kk                                           # masked slots
    none = [r for kind, r in c["special"].items() if kind.startswith("none")]
    assert c["special"]["none_last_of_tile_key_1e3"] in none and len(none) >= 2
    for kk in ("nbr", "edge", "nbr_t", "src_t"):
        assert np.all(got[kk][none] == 0.0), kk                                        # rows without a neighbour, slot 0 included
    assert np.all(got["attn_w"][none] == 0.0)
    assert all(np.abs(got["src"][r]).max() > 0 for r in none)                          # ... which still send gradient through src
    assert np.abs(got["nbr"][c["special"]["all_neighbours"]]).max() > 0


@pytest.mark.parametrize("case,p", CASE_DROPS, ids=IDS)
def test_two_backward_calls_give_the_same_bits(case, p):
    dv = Device(case)
    out, aw, saved = dv.forward(p)
    first = hip_result(case, p)
    again = dv.backward(p, saved)
    assert np.array_equal(out.cpu().numpy(), first["out"]) and np.array_equal(aw.cpu().numpy(), first["attn_w"])
    for kk in GRAD_ORDER:
        assert np.array_equal(again[kk].cpu().numpy().reshape(first[kk].shape), first[kk]), kk


@pytest.mark.parametrize("case", [(20, 4, 12, 4, 20, 6), (20, 0, 12, 1, 20, 5), (100, 172, 100, 2, 100, 20)], ids=G.ident)
def test_null_gradients_are_not_computed(case):
    """Only d_src and d_m2_w asked for: both are the full call's bit for bit, and nothing else is written -- the two lie inside one
    sentinel-filled arena with guard bands, and sentinel-filled buffers of the other thirteen shapes, handed to nobody, stay."""
    p = 0.3
    dv, full = Device(case), hip_result(case, p)
    _, _, saved = dv.forward(p)
    shapes = grad_shapes(case, dv.N)
    n_src, n_w2, guard = int(np.prod(shapes["src"])), int(np.prod(shapes["m2_w"])), 4096
    arena = torch.full((3 * guard + n_src + n_w2,), SENTINEL, dtype=torch.float32, device="cuda")
    bufs = {"src": arena[guard:guard + n_src].view(shapes["src"]),
            "m2_w": arena[2 * guard + n_src:2 * guard + n_src + n_w2].view(shapes["m2_w"])}
    others = {kk: torch.full(shapes[kk], SENTINEL, dtype=torch.float32, device="cuda") for kk in GRAD_ORDER if kk not in bufs}
    got = dv.backward(p, saved, names=("src", "m2_w"), buffers=bufs)
    assert set(got) == {"src", "m2_w"}
    assert np.array_equal(got["src"].cpu().numpy(), full["src"]) and np.array_equal(got["m2_w"].cpu().numpy(), full["m2_w"])
    a = arena.cpu().numpy()
    for lo, hi in ((0, guard), (guard + n_src, 2 * guard + n_src), (2 * guard + n_src + n_w2, a.size)):
        assert np.all(a[lo:hi] == SENTINEL), (lo, hi)
    assert all(bool((t == SENTINEL).all()) for t in others.values())
    # nothing asked for: nothing launched, nothing written
    assert dv.backward(p, saved, names=()) == {}


@pytest.fixture
def library_calls(monkeypatch):
    """name -> [n]: calls of the three attention entry points from here on"""
    lib = _capi().lib()
    calls = {}
    for name in ("zt_attention_train_forward", "zt_attention_train_backward", "zt_temporal_attention"):
        def counted(*args, _f=getattr(lib, name), _n=name):
            calls[_n][0] += 1
            return _f(*args)
        calls[name] = [0]
        monkeypatch.setattr(lib, name, counted)
    return calls


def _module_run(layer, c):
    x = [torch.from_numpy(np.array(a)).cuda() for a in c["x"]]
    x = [a if a.dtype == torch.bool else a.requires_grad_(True) for a in x]
    out, aw = layer(*x)
    return x, out, aw


@pytest.mark.parametrize("case", [(20, 4, 12, 4, 20, 5), (20, 0, 12, 1, 20, 5)], ids=G.ident)
def test_module_trains_on_the_device(case, library_calls):
    p = 0.3
    c = G.make_case(*case)
    layer = G.build_layer(*case[:5], c["w"]).cuda().train()
    layer.multi_head_target.dropout = p
    layer.fused_training, layer.drop_seed_override = True, SEED
    x, out, aw = _module_run(layer, c)
    assert out.requires_grad and not aw.requires_grad and layer._last_drop_seed == SEED
    (out * torch.from_numpy(np.array(d_out_of(case))).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert [library_calls[n][0] for n in ("zt_attention_train_forward", "zt_attention_train_backward", "zt_temporal_attention")] == [1, 1, 0]
    mha = layer.multi_head_target
    qkv = mha.in_proj_weight.grad.chunk(3) if mha._qkv_same_embed_dim else [t.grad for t in (mha.q_proj_weight, mha.k_proj_weight,
                                                                                              mha.v_proj_weight)]
    got = {"out": out, "q_w": qkv[0], "k_w": qkv[1], "v_w": qkv[2], "in_b": mha.in_proj_bias.grad, "out_w": mha.out_proj.weight.grad,
           "out_b": mha.out_proj.bias.grad, "m1_w": layer.merger.fc1.weight.grad, "m1_b": layer.merger.fc1.bias.grad,
           "m2_w": layer.merger.fc2.weight.grad, "m2_b": layer.merger.fc2.bias.grad}
    got.update({kk: t.grad if t.grad is not None else torch.zeros_like(t) for kk, t in zip(H.X_KEYS, x)})
    ref, direct = reference(case, p), hip_result(case, p)
    for kk in ("out",) + H.GRAD_KEYS:
        v = got[kk].detach().cpu().numpy()
        assert v.shape == ref[kk].shape, kk
        assert H.err(v, ref[kk]) <= bound(case, p, kk), kk
        assert np.array_equal(v, direct[kk]), kk                                      # the same kernels, the same bits
    assert np.array_equal(aw.cpu().numpy(), direct["attn_w"])
    # a drawn seed: kept, and another one the next time
    layer.drop_seed_override = None
    _module_run(layer, c)
    s1 = layer._last_drop_seed
    _module_run(layer, c)
    assert 0 <= s1 < 2 ** 62 and layer._last_drop_seed != s1
    # eval and no-grad forwards are the eval kernel's, as before
    with torch.no_grad():
        layer(*[a.detach() for a in x])
    assert library_calls["zt_temporal_attention"][0] == 1 and library_calls["zt_attention_train_forward"][0] == 3


def test_module_refused_shape_and_switch_off_stay_on_torch(library_calls):
    from zebra_amd.modules import TemporalAttentionLayer
    D, F, T, heads, out_dim, k = REFUSED
    rng = np.random.RandomState(3)
    N = 3
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda().requires_grad_(True)
    x = [f(N, D), f(N, 1, T), f(N, k, D), f(N, k, T), f(N, k, F), torch.from_numpy(rng.random_sample((N, k)) < 0.4).cuda()]
    layer = TemporalAttentionLayer(D, D, F, T, output_dimension=out_dim, n_head=heads).cuda().train()
    layer.fused_training = True
    out, _ = layer(*x)
    out.sum().backward()
    assert out.shape == (N, out_dim) and x[2].grad is not None and layer.merger.fc2.weight.grad is not None
    assert all(v[0] == 0 for v in library_calls.values())
    case = (20, 4, 12, 4, 20, 5)                                                       # a shape the kernels take, the switch off
    c = G.make_case(*case)
    layer = G.build_layer(*case[:5], c["w"]).cuda().train()
    assert layer.fused_training is False
    x, out, _ = _module_run(layer, c)
    out.sum().backward()
    assert x[0].grad is not None and all(v[0] == 0 for v in library_calls.values())


def test_keep_fraction_and_dropped_slots():
    from zebra_amd.modules import dropout_mask
    p, N, heads, k = 0.3, 600, 2, 20                                                   # a layer-sized index range
    m = dropout_mask(SEED, p, (1, N, heads), k)
    n = m.size
    assert n == N * heads * k and set(np.unique(m)) == {np.float32(0), np.float32(1.0 / (1.0 - float(np.float32(p))))}
    assert abs((m != 0).mean() - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n)
    seen = 0
    for case in CASES:
        keep, got = keep_of(case, p), hip_result(case, p)
        dropped = (keep == 0).all(axis=1)                                              # [N, k]: every head of the slot dropped
        seen += int(dropped.sum())
        assert np.all(got["attn_w"][dropped] == 0.0), case
        live = reference(case, p)["attn_w"] > 1e-5
        assert np.all(got["attn_w"][live] > 0.0) and not (live & dropped).any(), case  # a kept head of a real neighbour shows
    assert seen > 50
