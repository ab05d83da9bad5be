"""The attention layer's training pair without a GPU (csrc/attention_train.hip): the tests' own restatement
(helpers_attention_train.forward) against torch's float64 layer, out, attn_w and all 15 gradients; what attn_w means under
dropout; zt::attention_train_plan through zt_attention_train_plan -- shapes, tile, LDS, workspace and saved sizes --; the
argument checks of the C entry points, which come before any device call; and the module's switch.

The sizes the plan must give (include/zebra_amd.h), with Ep, Ekp, E2p, Hp, Op = E, Ek, E + D, hidden, out rounded up to 16 and
every matrix on a 256-byte boundary:
  fixed     = the forward's six padded weights (test_attention_cpu.py) + Hp Op + E2p Hp + Ep Ep floats (merger.fc2, merger.fc1
              and out_proj transposed)
  per row   = 4 (hidden + 2 E + 2 k E) bytes: d_hid, d_y, d_q / sqrt(hd), d_K, d_V
  saved/row = 4 (k heads + 2 E + hidden) bytes: p, o, y, relu(fc1)
The backward runs in the forward's LDS carve-up, so the tile table is the forward's (test_attention_cpu.PLAN_TABLE's numbers,
restated here) and the plan refuses exactly what zt::attention_plan refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_attention_train as H
import test_attention_f64_gpu as G

LDS_BOUND = 158 * 1024
REFUSED = None
S4, S2, W = (20, 4, 12, 4, 20, 20), (20, 4, 12, 2, 20, 20), (100, 172, 100, 2, 100, 100)
# (D, F, T, heads, hidden, out, k) -> (rq, mt, LDS bytes of the forward = of the backward) or REFUSED
TRAIN_PLAN_TABLE = [
    (S4 + (1,), (16, 1, 16704)), (S4 + (5,), (16, 5, 38208)), (S4 + (6,), (13, 5, 38208)),
    (S2 + (17,), (4, 5, 38208)), (S2 + (41,), (1, 3, 26432)), (S2 + (80,), (1, 5, 38208)), (S2 + (81,), REFUSED),
    ((20, 7, 13, 3, 20, 70, 5), (16, 5, 45376)), ((20, 0, 12, 1, 20, 20, 5), (16, 5, 33088)),
    (W + (20,), (2, 3, 155456)), (W + (48,), (1, 3, 155456)), (W + (49,), REFUSED),
    ((100, 1, 100, 2, 100, 100, 40), (1, 3, 121664)), ((100, 1, 100, 2, 100, 100, 80), REFUSED),
    ((128, 16, 128, 2, 128, 128, 20), (2, 3, 153408)), ((172, 172, 172, 2, 172, 172, 16), (1, 1, 136512)),
    ((172, 172, 172, 2, 172, 172, 17), REFUSED), ((224, 1, 224, 2, 224, 224, 10), (1, 1, 160064)),
    ((228, 1, 228, 2, 228, 228, 10), REFUSED), ((20, 4, 12, 5, 20, 20, 5), REFUSED), ((20, 4, 12, 3, 20, 20, 5), REFUSED),
    ((20, 4, 12, 0, 20, 20, 5), REFUSED), ((20, 4, 12, 2, 20, 20, 0), REFUSED), ((0, 4, 12, 2, 20, 20, 5), REFUSED),
    ((20, -1, 12, 2, 20, 20, 5), REFUSED), ((20, 4, 0, 2, 20, 20, 5), REFUSED), ((20, 4, 12, 2, 0, 20, 5), REFUSED),
    ((20, 4, 12, 2, 20, 0, 5), REFUSED),
]
FAMILIES = G.FAMILIES[:4]            # one case of each shape family the GPU file trains: heads 4, 3, 1 (F = 0), the realistic tile


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def i32(*v):
    return [C.c_int32(x) for x in v]


def sizes(capi, N, *shape):
    lib = capi.lib()
    return (int(lib.zt_attention_train_workspace_bytes(C.c_int64(N), *i32(*shape))),
            int(lib.zt_attention_train_saved_bytes(C.c_int64(N), *i32(*shape))))


def eval_plan(capi, *shape):
    o = (C.c_int64 * 4)()
    assert capi.hooks_lib().zt_test_attention_plan(*i32(*shape), o) == capi.ZT_OK
    return [int(v) for v in o]


@pytest.mark.parametrize("case", FAMILIES, ids=G.ident)
def test_helper_is_torch_float64(case):
    """Without dropout the helper IS forward_torch of a float64 layer: out, attn_w and the gradients of sum(out * d_out) with
    respect to the five inputs and the ten parameters, within 1e-12 max(1, max|ref|) each."""
    c = G.make_case(*case)
    d_out = np.random.RandomState(5).standard_normal((c["N"], case[4]))
    got = H.run(c, d_out, None, torch.float64)
    layer = G.build_layer(*case[:5], c["w"], torch.float64)                    # eval mode: its dropout is the identity
    x, _ = H.tensors(c, torch.float64)
    out, aw = layer.forward_torch(*x)
    (out * torch.from_numpy(d_out)).sum().backward()
    mha, E = layer.multi_head_target, case[0] + case[2]
    qkv = mha.in_proj_weight.grad.chunk(3) if mha._qkv_same_embed_dim else [p.grad for p in (mha.q_proj_weight, mha.k_proj_weight,
                                                                                              mha.v_proj_weight)]
    want = {"out": out, "attn_w": aw, "q_w": qkv[0], "k_w": qkv[1], "v_w": qkv[2], "in_b": mha.in_proj_bias.grad,
            "out_w": mha.out_proj.weight.grad, "out_b": mha.out_proj.bias.grad, "m1_w": layer.merger.fc1.weight.grad,
            "m1_b": layer.merger.fc1.bias.grad, "m2_w": layer.merger.fc2.weight.grad, "m2_b": layer.merger.fc2.bias.grad}
    want.update({kk: t.grad if t.grad is not None else torch.zeros_like(t) for kk, t in zip(H.X_KEYS, x)})
    assert set(want) == set(H.GRAD_KEYS) | {"out", "attn_w"} and len(H.GRAD_KEYS) == 15
    for kk, ref in want.items():
        ref = ref.detach().numpy()
        assert got[kk].shape == ref.shape, kk
        assert H.err(got[kk], ref) <= 1e-12 * max(1.0, np.abs(ref).max(initial=0)), kk
    assert np.abs(want["k_w"].numpy()).max() > 1e-3 and np.abs(got["src_t"]).max() > 1e-3       # gradients that say something


def test_attn_w_is_the_head_mean_of_the_dropped_weights():
    case = (20, 4, 12, 4, 20, 5)
    c = G.make_case(*case)
    N, heads, k = c["N"], case[3], case[5]
    keep = H.keep_mask(1234, 0.3, N, heads, k)
    assert keep.shape == (N, heads, k) and set(np.unique(keep)) == {np.float32(0), np.float32(1.0 / (1.0 - float(np.float32(0.3))))}
    x, w = H.tensors(c, torch.float64, requires_grad=False)
    _, aw0 = H.forward(x, w, heads)
    _, aw = H.forward(x, w, heads, torch.from_numpy(keep).double())
    # the undropped per-head weights, from the composition's own pieces
    src, src_t, nbr, nbr_t, edge, mask = x
    E = case[0] + case[2]
    q = (torch.cat([src, src_t.reshape(N, -1)], 1) @ w["q_w"].T + w["in_b"][:E]) / np.sqrt(E // heads)
    K = torch.cat([nbr, edge, nbr_t], 2) @ w["k_w"].T + w["in_b"][E:2 * E]
    inv = mask.all(1)
    m = mask.clone()
    m[inv, 0] = False
    s = torch.einsum("nhc,nkhc->nhk", q.reshape(N, heads, -1), K.reshape(N, k, heads, -1)).masked_fill(m[:, None], float("-inf"))
    p = torch.softmax(s, -1).numpy()
    want = (p * keep.astype(np.float64)).mean(axis=1)
    want[inv.numpy()] = 0
    assert H.err(aw.numpy(), want) <= 1e-15
    assert H.err(aw0.numpy(), p.mean(axis=1) * ~inv.numpy()[:, None]) <= 1e-15
    none = [r for kind, r in c["special"].items() if kind.startswith("none")]
    assert len(none) >= 2 and np.all(aw.numpy()[none] == 0.0) and np.all(aw0.numpy()[none] == 0.0)
    dropped = (keep == 0).all(axis=1)                                         # every head of a slot dropped
    assert dropped.any() and np.all(aw.numpy()[dropped] == 0.0)
    assert np.abs(aw.numpy() - aw0.numpy()).max() > 1e-2                      # the mask is visible in attn_w


@pytest.mark.parametrize("shape,want", TRAIN_PLAN_TABLE, ids=[G.ident(s) for s, _ in TRAIN_PLAN_TABLE])
def test_train_plan_table(capi, shape, want):
    D, F, T, heads, hidden, out, k = shape
    out8 = (C.c_int64 * 8)()
    assert capi.lib().zt_attention_train_plan(*i32(*shape), out8) == capi.ZT_OK
    got = [int(v) for v in out8]
    if want is REFUSED:
        assert got == [0] * 8
        assert sizes(capi, 3, *shape) == (-1, -1)
        return
    assert got[0] == 1 and tuple(got[1:5]) == (want[0], want[1], want[2], want[2])
    assert got[3] <= LDS_BOUND and got[4] <= LDS_BOUND
    assert eval_plan(capi, *shape) == [1, want[0], want[1], want[2]]          # the eval kernel's tile
    r16 = lambda v: (v + 15) // 16 * 16
    E, Ek = D + T, D + F + T
    Ep, Ekp, E2p, Hp, Op = r16(E), r16(Ek), r16(E + D), r16(hidden), r16(out)
    al = lambda a, b: (4 * a * b + 255) // 256 * 256
    fixed = sum(al(a, b) for a, b in ((Ep, Ep), (Ep, Ekp), (Ep, Ekp), (Ep, Ep), (Hp, E2p), (Op, Hp), (Hp, Op), (E2p, Hp), (Ep, Ep)))
    ws_row, saved_row = 4 * (hidden + 2 * E + 2 * k * E), 4 * (k * heads + 2 * E + hidden)
    assert got[5:] == [ws_row, fixed, saved_row]
    assert capi.attention_train_plan(*shape) == dict(zip(capi.ATTN_TRAIN_PLAN_FIELDS, got))
    for N in (0, 1, 7, 600):
        assert sizes(capi, N, *shape) == (fixed + N * ws_row, N * saved_row)
    assert sizes(capi, -1, *shape) == (-1, -1)
    assert fixed > int(capi.lib().zt_attention_workspace_bytes(*i32(*shape))) > 0


@pytest.mark.parametrize("base", [S2[:3], W[:3], (128, 16, 128), (224, 1, 224)], ids=G.ident)
def test_train_plan_accepts_nothing_the_eval_plan_refuses(capi, base):
    D, F, T = base
    taken = 0
    for heads in (1, 2, 3, 4, 5):
        for k in range(1, 83):
            shape = (D, F, T, heads, D, D, k)
            p = capi.attention_train_plan(*shape)
            ev = eval_plan(capi, *shape)
            assert p["supported"] <= ev[0], shape
            assert (sizes(capi, 4, *shape)[0] >= 0) == (p["supported"] == 1), shape
            if p["supported"]:
                taken += 1
                assert (p["rq"], p["mt"]) == tuple(ev[1:3]) and p["lds_fwd"] == ev[3], shape
                assert p["lds_fwd"] <= LDS_BOUND and p["lds_bwd"] <= LDS_BOUND, shape
    assert taken > 0


def _call_args(capi, N, k, D, F, T, heads, hidden, out, drop_p=0.0, null=()):
    """arguments of zt_attention_train_forward / _backward over pointers that are never dereferenced"""
    p = C.c_void_p(1 << 20)
    ten = [None if i in null else p for i in range(6)]
    wt = capi.AttnWeights(*([p] * 10))
    head = ten + [C.c_int64(N), C.c_int32(k)] + i32(D, F, T, heads, hidden, out) + [C.byref(wt), C.c_float(drop_p), C.c_uint64(7)]
    return p, wt, head


def test_entry_points_refuse_bad_arguments_without_a_device(capi):
    lib = capi.lib()
    ok = (3, 5, 20, 4, 12, 2, 20, 20)
    gr = capi.AttnGrads(*([C.c_void_p(1 << 20)] * 15))

    def both(args, **kw):
        p, wt, head = _call_args(capi, *args, **kw)
        return (lib.zt_attention_train_forward(*head, p, p, p, p, None),
                lib.zt_attention_train_backward(*head, p, p, C.byref(gr), p, None))

    assert both((0,) + ok[1:]) == (capi.ZT_OK, capi.ZT_OK)                                    # N = 0: nothing to launch
    assert both((0, 49, 100, 172, 100, 2, 100, 100)) == (capi.ZT_OK, capi.ZT_OK)
    assert both((-1,) + ok[1:]) == (capi.ZT_ERR_ARG,) * 2
    for bad_p in (-0.1, 1.0, 1.5, float("nan")):
        assert both(ok, drop_p=bad_p) == (capi.ZT_ERR_ARG,) * 2, bad_p
    for i in range(6):
        assert both(ok, null=(i,)) == (capi.ZT_ERR_ARG,) * 2, i
        assert b"NULL buffer" in lib.zt_last_error()
    for bad in ((3, 0) + ok[2:], (3, 5, 0) + ok[3:], (3, 5, 20, -1) + ok[4:], (3, 5, 20, 4, 0) + ok[5:]):
        assert both(bad) == (capi.ZT_ERR_ARG,) * 2, bad
    p, wt, head = _call_args(capi, *ok)
    for slot in range(4):                                                                    # out, attn_w, saved, workspace
        a = [p] * 4
        a[slot] = None
        assert lib.zt_attention_train_forward(*head, *a, None) == capi.ZT_ERR_ARG, slot
    for slot in range(4):                                                                    # saved, d_out, grads, workspace
        a = [p, p, C.byref(gr), p]
        a[slot] = None
        assert lib.zt_attention_train_backward(*head, *a, None) == capi.ZT_ERR_ARG, slot
    head_now = list(head)
    head_now[14] = None                                                                      # the weights
    assert lib.zt_attention_train_forward(*head_now, p, p, p, p, None) == capi.ZT_ERR_ARG
    for shape in [s for s, want in TRAIN_PLAN_TABLE if want is REFUSED and min(s[0], s[2], s[6]) > 0 and s[1] >= 0]:
        D, F, T, heads, hidden, out, k = shape
        assert both((3, k, D, F, T, heads, hidden, out)) == (capi.ZT_ERR_UNSUPPORTED,) * 2, shape
        assert b"unsupported shape" in lib.zt_last_error()


def test_edge_pointer_may_be_null_only_without_edge_features(capi):
    """F = 0: the edge array has no element and may be NULL; the call then gets as far as a refused shape's
    ZT_ERR_UNSUPPORTED (k = 81), the last host-side check."""
    lib = capi.lib()
    p, wt, head = _call_args(capi, 3, 81, 20, 0, 12, 2, 20, 20, null=(3,))
    assert lib.zt_attention_train_forward(*head, p, p, p, p, None) == capi.ZT_ERR_UNSUPPORTED
    p, wt, head = _call_args(capi, 3, 81, 20, 4, 12, 2, 20, 20, null=(3,))
    assert lib.zt_attention_train_forward(*head, p, p, p, p, None) == capi.ZT_ERR_ARG


def test_module_plan_answers_torch_off_the_device_path(capi):
    from zebra_amd.modules import attention_train_plan
    ok = (100, 172, 100, 2, 100, 100, 20)
    assert attention_train_plan("cuda", torch.float32, *ok) == "hip"
    assert attention_train_plan("cuda", torch.float32, *ok, fused=True) == "hip"
    assert attention_train_plan("cpu", torch.float32, *ok) == "torch"
    assert attention_train_plan("cuda", torch.float64, *ok) == "torch"
    assert attention_train_plan("cuda", torch.float32, *ok, fused=False) == "torch"
    assert attention_train_plan("cuda", torch.float32, 100, 172, 100, 2, 100, 100, 49) == "torch"
    assert attention_train_plan("cuda", torch.float32, 20, 4, 12, 5, 20, 20, 5) == "torch"


def test_fused_training_defaults_to_false():
    from zebra_amd.modules import TemporalAttentionLayer
    layer = TemporalAttentionLayer(20, 20, 4, 12, output_dimension=20, n_head=2)
    assert layer.fused_training is False and TemporalAttentionLayer.fused_training is False
    assert layer.drop_seed_override is None
    # on the CPU the switch changes nothing: a training forward under grad is forward_torch's
    c = G.make_case(20, 4, 12, 2, 20, 5)
    layer = G.build_layer(20, 4, 12, 2, 20, c["w"]).train()
    layer.multi_head_target.dropout = 0.0
    x, _ = H.tensors(c, torch.float32)
    want = layer.forward_torch(*x)
    layer.fused_training = True
    got = layer(*x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].requires_grad


def test_row_tile_kernels_use_no_scratch(capi, tmp_path):
    """The eval forward, the training forward and the backward tile kernel keep lds_linear's accumulators (up to five MFMA tiles)
    in registers: a private segment of 0 bytes and no vector register spilled, read from the built objects' code-object
    metadata as test_capi_cpu.py does for k_fc1_agg* (no GPU needed)."""
    import re
    import test_capi_cpu as K
    seen = {}
    for name in ("attention", "attention_train"):
        notes = K._code_object_notes(capi, tmp_path, name)
        for kern, seg, spill in re.findall(r"\.name:\s+(\S+)\s.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)",
                                           notes, re.S):
            seen[kern] = (int(seg), int(spill))
    for stem in ("20k_temporal_attention", "21k_attention_train_fwd", "15k_attention_bwd"):
        hit = [v for kern, v in seen.items() if stem in kern]
        assert hit == [(0, 0)], (stem, seen)
