"""The link scorer of a training step on the device (csrc/scoring_train.hip: zt_affinity_train_forward / _backward through
modules._HipLinkScore and TGN.score_train): the op against a float64 MergeLayer under autograd -- with torch's own float32
composition held to HALF the tolerances on the same inputs, so that the reference method has room of its own --, bit-equal
repeats, skipped outputs, the training loops of the reference's gradient fixtures (g8, g11, g12) with a proof that the HIP
scorer ran, fused against composed on whole steps, the data-parallel step, and the fallbacks."""
import ctypes as C

import numpy as np
import pytest
import torch

import inputs as I
from conftest import golden
from helpers import build_tgn, load_weights, make_args

pytestmark = pytest.mark.gpu

# hidden width H = D (n_tppr + 1) -> (D, n_tppr)
WIDTHS = {40: (20, 1), 60: (20, 2), 200: (100, 1), 300: (100, 2), 344: (172, 1), 516: (172, 2), 768: (256, 2),
          400: (100, 3)}                                   # (three models: run from tests/test_many_models_gpu.py)
# every H with a ragged B and with B = 4096; the other batch sizes of the issue's list spread over the widths
SHAPES = [(1, 40), (17, 40), (4096, 40), (15, 60), (17, 60), (4096, 60), (16, 200), (17, 200), (4096, 200),
          (17, 300), (200, 300), (600, 300), (4096, 300), (17, 344), (600, 344), (4096, 344),
          (15, 516), (200, 516), (4096, 516), (17, 768), (600, 768), (4096, 768)]
PARAMS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def _scorer_weights(H, seed):
    D, M = WIDTHS[H]
    w = I.model_weights(D, 1, 20, M, seed)
    return [w["aff1_w"], w["aff1_b"], w["aff2_w"], w["aff2_b"]]


def _inputs(B, H):
    g = torch.Generator().manual_seed(1000 * H + B)
    emb = torch.randn((3 * B, H), generator=g) * 0.7                   # as tests/test_scoring_gpu.py draws them
    # d(loss)/d(prob) at the scale BCE's mean gives: -1 / (B p) and 1 / (B (1 - p)) are O(1 / B).  The constant is 1/4 .. 3/4:
    # about one hidden pre-activation in 6e6 lies within float32 rounding of zero, where float32 (these kernels and torch's
    # composition alike) and the float64 reference take different sides of the ReLU; that one element moves a row of
    # d fc1.weight by ds w2 x = (c / B) p (1 - p) w2 x -- with c in 1 .. 3 at B = 4096, H = 344: 6.7e-6, identical for both
    # float32 methods and above HALF the absolute tolerance torch's composition is held to -- so the inputs are scaled until
    # such an element costs a fraction of that half (1.7e-6 there), not the tolerance widened
    sign = torch.cat([-torch.ones(B), torch.ones(B)])
    dprob = sign * (0.25 + 0.5 * torch.rand(2 * B, generator=g)) / B
    return emb, dprob, _scorer_weights(H, 7 + H)


def _merge_layer(H, wts, dtype, device):
    from zebra_amd.modules import MergeLayer
    m = MergeLayer(H, H, H, 1).to(dtype)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), wts):
            p.copy_(torch.from_numpy(w).to(dtype))
    return m.to(device)


def _composed(m, emb, dprob):
    """torch's composition (model/tgn_model.py:185-188) under autograd: prob [2B], d_emb, the four parameter gradients"""
    B = emb.shape[0] // 3
    emb = emb.clone().requires_grad_(True)
    prob = m(torch.cat([emb[:B], emb[:B]], dim=0), emb[B:]).squeeze(1).sigmoid()
    prob.backward(dprob)
    return [prob.detach(), emb.grad] + [p.grad for p in (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)]


def _hip(emb, dprob, wts, emb_grad=True, param_grad=True):
    from zebra_amd.modules import _HipLinkScore
    e = emb.cuda().requires_grad_(emb_grad)
    ps = [torch.from_numpy(w).cuda().requires_grad_(param_grad) for w in wts]
    prob = _HipLinkScore.apply(e, *ps)
    prob.backward(dprob.cuda())
    return [prob.detach(), e.grad] + [p.grad for p in ps]


def _errors(got, ref):
    """(max |error| of prob, of d_emb, [(max |error|, max |ref|) of the four parameter gradients])"""
    d = [float((g.detach().double().cpu().reshape(-1) - r.reshape(-1)).abs().max()) for g, r in zip(got, ref)]
    return d[0], d[1], [(d[2 + q], float(ref[2 + q].abs().max())) for q in range(4)]


@pytest.mark.parametrize("B,H", SHAPES)
def test_hip_link_score_against_float64(B, H):
    """_HipLinkScore forward and backward against a float64 MergeLayer under autograd on the CPU: prob and d_emb within 1e-5,
    the four parameter gradients within 1e-5 + 1e-4 max|ref| (the project's training tolerances); torch's float32
    composition on the GPU, same inputs, within HALF of each."""
    emb, dprob, wts = _inputs(B, H)
    ref = _composed(_merge_layer(H, wts, torch.float64, "cpu"), emb.double(), dprob.double())
    hip = _errors(_hip(emb, dprob, wts), ref)
    tor = _errors(_composed(_merge_layer(H, wts, torch.float32, "cuda"), emb.cuda(), dprob.cuda()), ref)
    print("B=%d H=%d hip: prob %.3g d_emb %.3g params %s | torch: prob %.3g d_emb %.3g params %s"
          % (B, H, hip[0], hip[1], ["%.3g" % e for e, _ in hip[2]], tor[0], tor[1], ["%.3g" % e for e, _ in tor[2]]))
    for name, (p_err, x_err, par), scale in (("torch", tor, 0.5), ("hip", hip, 1.0)):
        assert p_err <= scale * 1e-5, "%s prob: %g" % (name, p_err)
        assert x_err <= scale * 1e-5, "%s d_emb: %g" % (name, x_err)
        for pn, (err, mx) in zip(PARAMS, par):
            assert err <= scale * (1e-5 + 1e-4 * mx), "%s %s: %g (max |ref| %g)" % (name, pn, err, mx)


@pytest.mark.parametrize("B,H", [(17, 300), (4096, 300), (17, 516), (4096, 768)])
def test_hip_link_score_is_bit_equal_across_runs(B, H):
    """Two forward + backward runs on the same inputs: identical probabilities and identical gradients (every sum of the
    kernels has a fixed order)."""
    emb, dprob, wts = _inputs(B, H)
    a, b = _hip(emb, dprob, wts), _hip(emb, dprob, wts)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("B,H", [(17, 60), (600, 300)])
def test_hip_link_score_skips_outputs_that_are_not_needed(B, H):
    """emb.requires_grad = False: only the parameter gradients come back, the same bits as with it; frozen parameters:
    only d_emb, the same bits."""
    emb, dprob, wts = _inputs(B, H)
    full = _hip(emb, dprob, wts)
    par = _hip(emb, dprob, wts, emb_grad=False)
    assert par[1] is None
    for q in range(2, 6):
        assert torch.equal(par[q], full[q]), PARAMS[q - 2]
    inp = _hip(emb, dprob, wts, param_grad=False)
    assert all(g is None for g in inp[2:])
    assert torch.equal(inp[0], full[0]) and torch.equal(inp[1], full[1])


# ---------------------------------------------------------------------------------------------------------
# through the model
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def scorer_calls(monkeypatch):
    """[n]: calls of lib().zt_affinity_train_forward from here on"""
    from zebra_amd import _capi
    lib = _capi.lib()
    calls, fwd = [0], lib.zt_affinity_train_forward

    def counted(*args):
        calls[0] += 1
        return fwd(*args)

    monkeypatch.setattr(lib, "zt_affinity_train_forward", counted)
    return calls


def _train_steps(tgn, stream, bs, nb):
    """[(loss, {parameter: gradient})] of nb training steps in the reference's style (train.py:205-215)"""
    src, dst, neg, ts, eidx = stream
    crit = torch.nn.BCELoss()
    dev = torch.device("cuda")
    out = []
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        tgn.zero_grad()
        pos, negp = tgn.compute_edge_probabilities(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
        assert pos.shape == (bs, 1) and negp.shape == (bs, 1)
        loss = crit(pos.squeeze(), torch.ones(bs, device=dev)) + crit(negp.squeeze(), torch.zeros(bs, device=dev))
        loss.backward()
        out.append((float(loss.item()), {pn: p.grad.detach().cpu().numpy().copy() for pn, p in tgn.named_parameters()
                                         if p.grad is not None}))
        tgn.memory.detach_memory()
    return out


def _build_rnn_tgn(N, E1, D, F, T, k, al, be, w, rw, efeat):
    from zebra_amd.tgn import TGN
    tgn = TGN(neighbor_finder=None, node_features=None, edge_features=efeat, device="cuda", n_layers=2, n_heads=2,
              dropout=0.0, use_memory=True, node_dimension=D, time_dimension=T, memory_dimension=D,
              embedding_module_type="diffusion", message_function="identity", aggregator_type="last",
              memory_updater_type="rnn", n_neighbors=10, args=make_args(N, E1, k, al, be))
    w = dict(w)
    w.update(rw)
    return load_weights(tgn.to("cuda"), w)


@pytest.mark.parametrize("fixture", ["g8_train_grads", "g11_rnn_train_grads"])
def test_fused_scorer_training_step_matches_reference(fixture, scorer_calls):
    """The training loops of test_training_step_gradients_match_reference (GRU) and
    test_rnn_training_step_gradients_match_reference (RNN) with the HIP scorer (H = 40): the reference's loss within 1e-5 and
    every parameter gradient within 1e-5 + 1e-4 max|ref|; the HIP forward ran once per batch."""
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES["d20_f7"]
    g = golden(fixture)
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    if fixture.startswith("g11"):
        tgn = _build_rnn_tgn(N, E + 1, D, F, T, k, al, be, w, {kk: g["rnn_" + kk] for kk in ("w_ih", "w_hh", "b_ih", "b_hh")}, efeat)
    else:
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    assert tgn.fused_scoring is True
    tgn.train(True)
    seen = scorer = 0
    for b, (loss, grads) in enumerate(_train_steps(tgn, stream, bs, nb)):
        assert abs(loss - float(g["b%d_loss" % b])) <= 1e-5, "loss of batch %d" % b
        for pn in [kk[len("b%d_grad_" % b):] for kk in g.files if kk.startswith("b%d_grad_" % b)]:
            assert pn in grads, pn
            want = g["b%d_grad_%s" % (b, pn)]
            err = np.abs(grads[pn] - want).max()
            assert err <= 1e-5 + 1e-4 * np.abs(want).max(), "%s in batch %d: %g" % (pn, b, err)
            seen += 1
            scorer += pn.startswith("affinity_score.")
    assert scorer_calls[0] == nb
    assert seen >= 12 * nb and scorer == 4 * nb


def test_fused_scorer_training_step_matches_reference_d172(scorer_calls):
    """The loop of test_wide_d_training_step_matches_reference (D = F = 172, H = 516) with the HIP scorer against
    g12_train_grads_d172: values at the fixture's sampled indices, row and column sums, max |g|, that test's tolerances."""
    N, E, D, F, T, k, al, be, seed, bs, nb = (120, 400, 172, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 34, 20, 4)
    g = golden("g12_train_grads_d172")
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    tgn.train(True)
    seen = scorer = 0
    for b, (loss, grads) in enumerate(_train_steps(tgn, stream, bs, nb)):
        assert abs(loss - float(g["b%d_loss" % b])) <= 1e-5, "loss of batch %d" % b
        for pn in [kk[len("b%d_at_" % b):] for kk in g.files if kk.startswith("b%d_at_" % b)]:
            assert pn in grads, pn
            got, mx = grads[pn], float(g["b%d_max_%s" % (b, pn)])
            tol = 1e-5 + 1e-4 * mx
            err = np.abs(got.ravel()[g["idx_" + pn]] - g["b%d_at_%s" % (b, pn)]).max()
            assert err <= tol, "%s in batch %d: %g" % (pn, b, err)
            assert abs(np.abs(got).max() - mx) <= tol, pn
            if got.ndim == 2:
                for axis, key in ((1, "rows"), (0, "cols")):
                    d = np.abs(got.sum(axis=axis, dtype=np.float64) - g["b%d_%s_%s" % (b, key, pn)]).max()
                    assert d <= tol * got.shape[axis], "%s %s in batch %d: %g" % (pn, key, b, d)
            seen += 1
            scorer += pn.startswith("affinity_score.")
    assert scorer_calls[0] == nb
    assert seen >= 12 * nb and scorer == 4 * nb


def _d100_case():
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES["d100_f172"]
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    return (N, E + 1, D, F, T, k, al, be, w, efeat), stream, bs, nb


def _assert_steps_close(got, want):
    for b, ((la, ga), (lb, gb)) in enumerate(zip(got, want)):
        assert abs(la - lb) <= 1e-5, "loss of step %d" % b
        assert sorted(ga) == sorted(gb)
        for pn in ga:
            err = np.abs(ga[pn] - gb[pn]).max()
            assert err <= 1e-5 + 1e-4 * np.abs(gb[pn]).max(), "%s in step %d: %g" % (pn, b, err)


def test_fused_scoring_equals_torch_composition(scorer_calls):
    """fused_scoring True against False on the same steps of d100_f172 (H = 300): losses within 1e-5, every gradient -- the
    embedding module's and the memory updater's included, they receive d_emb -- within 1e-5 + 1e-4 max; with False the HIP
    scorer is never called."""
    args, stream, bs, nb = _d100_case()
    res, calls = {}, {}
    for fused in (True, False):
        tgn = build_tgn(*args)
        tgn.fused_scoring = fused
        tgn.train(True)
        before = scorer_calls[0]
        res[fused] = _train_steps(tgn, stream, bs, nb)
        calls[fused] = scorer_calls[0] - before
    assert calls == {True: nb, False: 0}
    _assert_steps_close(res[True], res[False])
    names = set(res[True][-1][1])
    assert any(pn.startswith("embedding_module.") for pn in names) and any(pn.startswith("memory_updater.") for pn in names)


def test_sharded_train_step_uses_the_fused_scorer(scorer_calls):
    """ShardedTGN(tgn, 0, 1).train_step scores through TGN.score_train: the loss and the gradients of the plain step."""
    from zebra_amd.distributed import ShardedTGN
    args, stream, bs, nb = _d100_case()
    plain = build_tgn(*args)
    plain.train(True)
    want = _train_steps(plain, stream, bs, nb)
    assert scorer_calls[0] == nb
    tgn = build_tgn(*args)
    tgn.train(True)
    runner = ShardedTGN(tgn, 0, 1)
    src, dst, neg, ts, eidx = stream
    got = []
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        tgn.zero_grad()
        loss = runner.train_step(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, torch.nn.BCELoss())
        got.append((float(loss.item()), {pn: p.grad.detach().cpu().numpy().copy() for pn, p in tgn.named_parameters()
                                         if p.grad is not None}))
        tgn.memory.detach_memory()
    assert scorer_calls[0] == 2 * nb
    _assert_steps_close(got, want)


def test_unsupported_width_falls_back_to_torch(scorer_calls):
    """H = 50 (D = 25, one T-PPR model) is no multiple of 4: the step runs on torch's composition without error; the
    workspace query says so for 50, 772 and 0."""
    from zebra_amd import _capi
    from zebra_amd.tgn import link_score_plan
    lib = _capi.lib()
    for H in (50, 772, 0):
        assert lib.zt_affinity_train_workspace_bytes(C.c_int64(64), C.c_int32(H)) == -1, H
    assert lib.zt_affinity_train_workspace_bytes(C.c_int64(64), C.c_int32(768)) > 0
    N, E, D, F, T, k, al, be, seed, bs, nb = 60, 300, 25, 7, 20, 5, [0.2], [0.8], 33, 16, 2
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    tgn.train(True)
    assert link_score_plan("cuda", torch.float32, 50, tgn.fused_scoring) == "torch"
    steps = _train_steps(tgn, stream, bs, nb)
    assert scorer_calls[0] == 0
    assert all(np.isfinite(loss) for loss, _ in steps)
    assert all("affinity_score.fc1.weight" in grads for _, grads in steps)
