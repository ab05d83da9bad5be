"""The training link scorer without a GPU (csrc/scoring_train.hip, TGN.score_train): the three entry points are declared and
listed, their argument and bound checks come before any device call, link_score_plan's decisions, and score_train on CPU
tensors is MergeLayer's composition bit for bit."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zt_affinity_train_workspace_bytes", "zt_affinity_train_forward", "zt_affinity_train_backward")


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def test_training_scorer_symbols_are_declared_listed_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    declared = set(re.findall(r"\b(zt_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.lib()
    for s in NEW:
        assert s in declared, s
        assert s in capi.SYMBOLS, s
        assert hasattr(lib, s), s


def test_workspace_query_names_the_supported_widths(capi):
    ws = capi.lib().zt_affinity_train_workspace_bytes
    for H in (0, -4, 2, 50, 302, 772, 1024):
        assert ws(C.c_int64(200), C.c_int32(H)) == -1, H
    assert ws(C.c_int64(-1), C.c_int32(300)) == -1
    for H in (4, 40, 60, 200, 300, 344, 516, 768):
        need = ws(C.c_int64(200), C.c_int32(H))
        assert need >= 2 * 200 * H * 4 + 2 * 200 * 4, H                       # at least d(hidden) [2B][H] and d(score) [2B]
    assert ws(C.c_int64(0), C.c_int32(300)) > 0
    assert ws(C.c_int64(4096), C.c_int32(300)) > ws(C.c_int64(200), C.c_int32(300))


def test_argument_and_bound_checks_need_no_device(capi):
    """NULL / negative arguments: ZT_ERR_ARG; a width outside H % 4 == 0, 4 <= H <= 768: ZT_ERR_UNSUPPORTED with a text that
    names the bound; B = 0: ZT_OK, nothing touched.  All before the first HIP call (this process has no GPU to call)."""
    lib = capi.lib()
    p = C.c_void_p(1 << 20)                        # never dereferenced: every call below returns from its checks
    wt = capi.AffinityWeights(p, p, p, p)
    fwd = lambda emb, B, H, w, prob, hid: lib.zt_affinity_train_forward(emb, C.c_int64(B), C.c_int32(H), w, prob, hid, None)
    bwd = lambda emb, B, H, w, ws, max_b, dprob=p: lib.zt_affinity_train_backward(
        emb, C.c_int64(B), C.c_int32(H), w, p, p, dprob, p, p, p, p, p, ws, C.c_int64(max_b), None)
    assert fwd(None, 16, 300, C.byref(wt), p, p) == capi.ZT_ERR_ARG
    assert fwd(p, 16, 300, None, p, p) == capi.ZT_ERR_ARG
    assert fwd(p, 16, 300, C.byref(wt), None, p) == capi.ZT_ERR_ARG
    assert fwd(p, 16, 300, C.byref(wt), p, None) == capi.ZT_ERR_ARG
    assert fwd(p, -1, 300, C.byref(wt), p, p) == capi.ZT_ERR_ARG
    assert fwd(p, 16, -300, C.byref(wt), p, p) == capi.ZT_ERR_ARG
    assert fwd(C.c_void_p((1 << 20) + 4), 16, 300, C.byref(wt), p, p) == capi.ZT_ERR_ARG       # rows are read as 16-byte vectors
    half = capi.AffinityWeights(p, None, p, p)
    assert fwd(p, 16, 300, C.byref(half), p, p) == capi.ZT_ERR_ARG
    for H in (50, 772, 0, 1024):
        assert fwd(p, 16, H, C.byref(wt), p, p) == capi.ZT_ERR_UNSUPPORTED, H
        msg = lib.zt_last_error()
        assert (b"H=%d" % H) in msg and b"768" in msg and b"% 4" in msg, msg
        assert bwd(p, 16, H, C.byref(wt), p, 16) == capi.ZT_ERR_UNSUPPORTED, H
    assert fwd(None, 0, 300, C.byref(wt), None, None) == capi.ZT_OK
    assert bwd(None, 16, 300, C.byref(wt), p, 16) == capi.ZT_ERR_ARG
    assert bwd(p, 16, 300, None, p, 16) == capi.ZT_ERR_ARG
    assert bwd(p, 16, 300, C.byref(wt), None, 16) == capi.ZT_ERR_ARG
    assert bwd(p, 16, 300, C.byref(wt), p, 16, dprob=None) == capi.ZT_ERR_ARG
    assert bwd(p, 16, 300, C.byref(wt), p, 8) == capi.ZT_ERR_ARG                                # workspace sized for fewer edges
    assert bwd(p, -2, 300, C.byref(wt), p, 16) == capi.ZT_ERR_ARG
    assert bwd(None, 0, 300, C.byref(wt), None, 0) == capi.ZT_OK
    with pytest.raises(ValueError):
        capi.check(fwd(p, 16, 50, C.byref(wt), p, p), "zt_affinity_train_forward")


def test_link_score_plan_table():
    from zebra_amd.tgn import link_score_plan
    f32, f64, f16 = torch.float32, torch.float64, torch.float16
    table = [
        (("cuda", f32, 300, True), "hip"), (("cuda", f32, 200, True), "hip"), (("cuda", f32, 40, True), "hip"),
        (("cuda", f32, 4, True), "hip"), (("cuda", f32, 344, True), "hip"), (("cuda", f32, 516, True), "hip"),
        (("cuda", f32, 768, True), "hip"),
        (("cuda", f32, 300, False), "torch"), (("cuda", f32, 768, False), "torch"),
        (("cpu", f32, 300, True), "torch"), (("cpu", f32, 300, False), "torch"),
        (("cuda", f64, 300, True), "torch"), (("cuda", f16, 300, True), "torch"),
        (("cuda", f32, 50, True), "torch"), (("cuda", f32, 302, True), "torch"), (("cuda", f32, 772, True), "torch"),
        (("cuda", f32, 1024, True), "torch"), (("cuda", f32, 0, True), "torch"), (("cuda", f32, 2, True), "torch"),
    ]
    for args, want in table:
        assert link_score_plan(*args) == want, args


def test_plan_and_library_agree_on_the_widths(capi):
    from zebra_amd.tgn import link_score_plan
    ws = capi.lib().zt_affinity_train_workspace_bytes
    for H in range(0, 800):
        assert (link_score_plan("cuda", torch.float32, H, True) == "hip") == (ws(C.c_int64(16), C.c_int32(H)) > 0), H


def test_score_train_on_cpu_is_merge_layers_composition():
    """TGN.score_train on CPU tensors (link_score_plan: torch) against the reference's expression (model/tgn_model.py:185-188)
    written out here: the probabilities and every gradient, bit for bit, with fused_scoring on and off."""
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN
    B, H = 9, 24
    torch.manual_seed(3)
    layer = MergeLayer(H, H, H, 1)
    emb0 = torch.randn(3 * B, H)
    w = torch.rand(2 * B, 1)

    def run(score):
        layer.zero_grad()
        emb = emb0.clone().requires_grad_(True)
        pos, neg = score(emb)
        assert pos.shape == (B, 1) and neg.shape == (B, 1)
        (torch.cat([pos, neg]) * w).sum().backward()
        return [pos.detach().clone(), neg.detach().clone(), emb.grad.clone()] + [p.grad.clone() for p in layer.parameters()]

    def reference(emb):
        s, d, n = emb[:B], emb[B:2 * B], emb[2 * B:]
        score = layer(torch.cat([s, s], dim=0), torch.cat([d, n])).squeeze(dim=0)
        return score[:B].sigmoid(), score[B:].sigmoid()

    want = run(reference)
    for fused in (True, False):
        holder = types.SimpleNamespace(affinity_score=layer, fused_scoring=fused)
        holder._score_pairs = types.MethodType(TGN._score_pairs, holder)
        got = run(types.MethodType(TGN.score_train, holder))
        for a, b in zip(got, want):
            assert torch.equal(a, b)
