"""The eval link scorer at every hidden width the training scorer takes (csrc/scoring.hip: k_affinity_gen, k_affinity_gen_tiled
behind zt::affinity_kernel_plan): the probabilities against torch's MergeLayer in float64 and against the oracle's scorer, the
generic forms against the specialised ones and against each other (ZT_CHOICE_SCORE), weight changes, the scorer as the tail of
the native step at D = 172, and the widths that stay refused.

Largest |error| against the float64 MergeLayer per shape, measured on an MI355X (printed by the accuracy test): DESIGN.md
section 5, "Scoring and metrics"."""
import functools
import types

import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn

pytestmark = pytest.mark.gpu
TOL = 1e-4            # the project's tolerance for a probability (tests/test_scoring_gpu.py)
FORM_TOL = 1e-5       # two float32 associations of the same sums (the float32 composition lies within 2.9e-7 of float64 here)
LATENCY, TILED, GEN_LATENCY, GEN_TILED = 1, 2, 3, 4
# hidden width H = D (n_tppr + 1) -> (D, n_tppr)
WIDTHS = {4: (2, 1), 20: (10, 1), 200: (100, 1), 300: (100, 2), 344: (172, 1), 512: (256, 1), 516: (172, 2), 768: (256, 2)}


@functools.lru_cache(maxsize=None)
def _weights(H):
    D, M = WIDTHS[H]
    w = I.model_weights(D, 1, 20, M, 7 + H)
    return w["aff1_w"], w["aff1_b"], w["aff2_w"], w["aff2_b"]


def _merge_layer(H, dtype, device):
    from zebra_amd.modules import MergeLayer
    m = MergeLayer(H, H, H, 1).to(dtype)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), _weights(H)):
            p.copy_(torch.from_numpy(w).to(dtype))
    return m.to(device)


def _scorer(H):
    """TGN.score_device on a MergeLayer of width H alone (no model around it: some of the widths have no (D, M) a TGN takes)"""
    from zebra_amd.tgn import TGN
    holder = types.SimpleNamespace(affinity_score=_merge_layer(H, torch.float32, "cuda"), device=torch.device("cuda"))
    holder._affinity_state = types.MethodType(TGN._affinity_state, holder)
    holder.score_device = types.MethodType(TGN.score_device, holder)
    return holder


def _emb(B, H):
    g = torch.Generator().manual_seed(B + WIDTHS[H][1])                # as tests/test_scoring_gpu.py seeds them
    return torch.randn((3 * B, H), generator=g) * 0.7


@functools.lru_cache(maxsize=None)
def _reference(B, H):
    """float64 MergeLayer on the CPU, computed once per shape: [2B] probabilities"""
    emb = _emb(B, H).double()
    with torch.no_grad():
        return _merge_layer(H, torch.float64, "cpu")(torch.cat([emb[:B], emb[:B]]), emb[B:]).squeeze(1).sigmoid()


def _pinned(choice):
    from zebra_amd import _capi

    class _Pin:
        def __enter__(self):
            _capi.set_kernel_choice(_capi.CHOICE_SCORE, choice)

        def __exit__(self, *exc):
            _capi.set_kernel_choice(_capi.CHOICE_SCORE, 0)
    return _Pin()


# H = 4: one partial k-chunk, one N-tile; 20: ragged second chunk and tile; 344 / 516: H % 16 = 8 / 4; 512: whole tiles;
# 768: the LDS limit, three N-tiles per wave.  (form, B, H); form 0: the library's pick
ACCURACY = ([(GEN_LATENCY, B, H) for H in (4, 20, 344, 512, 516) for B in (1, 17, 200)] +
            [(GEN_TILED, B, H) for H in (4, 20, 344, 512, 516) for B in (17, 512, 1000)] +
            [(0, 8200, 516)] +
            [(form, B, 768) for form in (GEN_LATENCY, GEN_TILED) for B in (17, 520)])


@pytest.mark.parametrize("form,B,H", ACCURACY)
def test_generic_scorer_matches_float64_and_oracle(oracle, form, B, H):
    """Probabilities within 1e-4 of a float64 MergeLayer and of the oracle's scorer, and two launches give the same bits (no
    float atomics: the N-tiles' partial scores are added first to last whichever wave arrives last)."""
    from zebra_amd import _capi
    import ctypes as C
    out = (C.c_int64 * 7)()
    _capi.hooks_lib().zt_test_affinity_plan(C.c_int64(B), C.c_int32(H), C.c_int32(form), out)
    assert out[0] == (form or GEN_TILED), "the plan does not run the form this case is about"
    sc = _scorer(H)
    emb = _emb(B, H).cuda()
    with _pinned(form):
        got = sc.score_device(emb)
        again = sc.score_device(emb)
        torch.cuda.synchronize()
    assert got.shape == (2 * B,) and torch.equal(got, again)
    err = float((got.double().cpu() - _reference(B, H)).abs().max())
    print("form %d B=%d H=%d: max |prob - float64| = %.3g" % (out[0], B, H, err))
    assert err <= TOL
    e = emb.cpu().numpy()
    w = _weights(H)
    want = oracle.affinity(np.concatenate([e[:B], e[:B]]), e[B:], dict(fc1_w=w[0], fc1_b=w[1], fc2_w=w[2], fc2_b=w[3]))
    assert np.abs(got.cpu().numpy() - want).max() <= TOL


@pytest.mark.parametrize("H", [200, 300])
@pytest.mark.parametrize("B", [17, 200, 1000])
def test_generic_forms_match_the_specialised_kernels(B, H):
    """H = 200 / 300: each generic form, pinned, against the library's specialised pick on the same inputs -- float32
    re-association only."""
    sc = _scorer(H)
    emb = _emb(B, H).cuda()
    spec = sc.score_device(emb)
    for form in (GEN_LATENCY, GEN_TILED):
        with _pinned(form):
            got = sc.score_device(emb)
            torch.cuda.synchronize()
        d = float((got - spec).abs().max())
        print("B=%d H=%d generic form %d vs specialised: %.3g" % (B, H, form, d))
        assert d <= FORM_TOL, form
    assert float((spec.double().cpu() - _reference(B, H)).abs().max()) <= TOL


@pytest.mark.parametrize("B", [17, 200, 1000])
def test_generic_latency_matches_generic_tiled(B):
    H = 516
    sc = _scorer(H)
    emb = _emb(B, H).cuda()
    got = {}
    for form in (GEN_LATENCY, GEN_TILED):
        with _pinned(form):
            got[form] = sc.score_device(emb)
            torch.cuda.synchronize()
    d = float((got[GEN_LATENCY] - got[GEN_TILED]).abs().max())
    print("B=%d H=%d generic latency vs generic tiled: %.3g" % (B, H, d))
    assert d <= FORM_TOL


def test_wide_affinity_follows_weight_changes():
    """The packed copy of the scorer's weights is remade when a weight changes in place (tests/test_scoring_gpu.py:
    test_affinity_follows_weight_changes, at H = 516)."""
    H, B = 516, 64
    sc = _scorer(H)
    emb = torch.randn((3 * B, H), generator=torch.Generator().manual_seed(1)).cuda()
    a = sc.score_device(emb)
    with torch.no_grad():
        sc.affinity_score.fc1.weight.mul_(0.5)
        sc.affinity_score.fc2.bias.add_(0.25)
        ref = sc.affinity_score(torch.cat([emb[:B], emb[:B]]), emb[B:]).squeeze(1).sigmoid()
    b = sc.score_device(emb)
    assert float((b - ref).abs().max()) <= TOL and float((a - b).abs().max()) > 1e-3


@pytest.mark.parametrize("bs,nb", [(200, 6), (600, 3)])
def test_pipeline_scores_at_d172(bs, nb):
    """D = 172 with two T-PPR models (H = 516): with TGN.enable_scoring the native step writes the batch's probabilities behind
    its aggregation; they equal score_device on the embeddings the step returned bit for bit (bs = 200: the generic latency
    form, bs = 600: the generic tiled one), lie within 1e-4 of torch's composition and follow a weight change."""
    D = F = 172
    N, T, k, al, be, seed = 2000, 100, 20, [0.1, 0.1], [0.5, 0.95], 516
    E = bs * nb
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()
    tgn.enable_pipeline(tppr_cus=0, max_batch=max(256, bs), group=2)
    try:
        tgn.enable_scoring()
        t = [torch.from_numpy(x).to(tgn.device) for x in (src, dst, neg, ts, eidx)]
        batches = [tuple(x[b * bs:(b + 1) * bs] for x in t) for b in range(nb)]
        with torch.cuda.stream(tgn.main_stream):
            for q, cur in enumerate(batches):
                if q == 2:
                    with torch.no_grad():
                        tgn.affinity_score.fc1.bias.add_(0.1)
                emb = tgn.step_device(*cur, ahead=batches[q + 1: q + 4])
                got = tgn.last_prob().clone()
                want = tgn.score_device(emb)
                assert torch.equal(got, want), "batch %d" % q
                with torch.no_grad():
                    ref = tgn.affinity_score(torch.cat([emb[:bs], emb[:bs]]), emb[bs:]).squeeze(1).sigmoid()
                assert float((want - ref).abs().max()) <= TOL, "batch %d" % q
        torch.cuda.synchronize()
    finally:
        tgn.enable_pipeline(False)


def test_refused_widths_keep_torch_and_the_error():
    """D = 102 with one model (H = 204: round_up16(H) = 208, the specialised kernels over a ragged last chunk) scores on the device; a MergeLayer of width 770 (770 % 4 != 0) sends
    score_device to torch's composition and makes enable_scoring raise."""
    import ctypes as C
    from zebra_amd import _capi
    from zebra_amd.modules import MergeLayer
    D, T = 102, 100
    w = I.model_weights(D, 1, T, 1, 5)
    _, efeat = I.random_tables(50, 60, D, 1, 5)
    tgn = build_tgn(50, 60, D, 1, T, 20, [0.1], [0.9], w, efeat).eval()
    B = 33
    emb = (torch.randn((3 * B, 204), generator=torch.Generator().manual_seed(B)) * 0.7).cuda()
    # (asked of the library, not of TGN._affinity_state: that call marks the weights as packed for the call that follows it)
    assert _capi.lib().zt_affinity_workspace_bytes(C.c_int64(B), C.c_int32(204)) > 0
    got = tgn.score_device(emb)
    with torch.no_grad():
        ref = tgn.affinity_score(torch.cat([emb[:B], emb[:B]]), emb[B:]).squeeze(1).sigmoid()
    assert float((got - ref).abs().max()) <= TOL
    tgn.enable_pipeline(tppr_cus=0, max_batch=64)
    try:
        torch.manual_seed(0)
        tgn.affinity_score = MergeLayer(770, 770, 770, 1).cuda()
        assert _capi.lib().zt_affinity_workspace_bytes(C.c_int64(B), C.c_int32(770)) == -1
        emb = (torch.randn((3 * B, 770), generator=torch.Generator().manual_seed(B)) * 0.7).cuda()
        with torch.no_grad():
            ref = tgn.affinity_score(torch.cat([emb[:B], emb[:B]]), emb[B:]).squeeze(1).sigmoid()
        assert torch.equal(tgn.score_device(emb), ref)
        with pytest.raises(ValueError):
            tgn.enable_scoring()
    finally:
        tgn.enable_pipeline(False)
