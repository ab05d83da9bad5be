"""Node classification without a GPU: the float64 restatement of the decoder (tests/helpers_decoder.py) against the reference's
fixture g14_node_decoder; zebra_amd.decoder.MLP on CPU tensors (torch's composition) against the same fixture; the host-side
plans (decoder_plan, label_bce_plan, zt_node_decoder_plan at every seam tests/test_decoder_gpu.py names); the refusals that
come before any device call; the numpy dropout mask; node_auc against exact counts; and the margin condition at every
committed seed of the GPU file's backward and dropout cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import helpers_decoder as hd

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import metrics_exact  # noqa: E402

DIMS = (40, 300)


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def g():
    return golden("g14_node_decoder")


def fixture_params(g, dim):
    return {k: g["d%d_%s" % (dim, k)] for k in hd.KEYS}


# ---- the restatement and the torch path against the reference --------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_restatement_equals_the_reference(g, dim):
    pre = "d%d_" % dim
    P, x, y = fixture_params(g, dim), g[pre + "x"], g[pre + "labels"]
    f = hd.forward64(P, x)
    assert np.abs(f["z"] - g[pre + "logits"]).max() <= 1e-12
    loss, dprob = hd.bce64(hd.sigmoid64(f["z"]), y)
    assert abs(loss - float(g[pre + "loss"])) <= 1e-12
    p = hd.sigmoid64(f["z"])
    grads = hd.backward64(P, x, f, dprob * p * (1.0 - p))
    # ... and with explicit masks of ones: the same
    ones = hd.backward64(P, x, hd.forward64(P, x, np.ones((len(x), 80)), np.ones((len(x), 10))), dprob * p * (1.0 - p),
                         np.ones((len(x), 80)), np.ones((len(x), 10)))
    for k in hd.KEYS:
        want = g[pre + "g_" + k]
        assert np.abs(grads["g_" + k].reshape(want.shape) - want).max() <= 1e-12, k
        assert np.array_equal(grads["g_" + k], ones["g_" + k])
    assert np.abs(grads["d_x"] - g[pre + "d_x"]).max() <= 1e-12


def test_restatement_masks_scale_and_zero():
    P, x, dz = hd.draw_case(9, 20, 5)
    rng = np.random.RandomState(3)
    m1, m2 = (rng.rand(9, 80) < 0.7) / 0.7, (rng.rand(9, 10) < 0.7) / 0.7
    f = hd.forward64(P, x, m1, m2)
    assert np.all(f["h1"][m1 == 0] == 0) and np.all(f["h2"][m2 == 0] == 0)
    gr = hd.backward64(P, x, f, dz, m1, m2)
    # a finite difference on one weight of each layer (float64: 1e-6 steps resolve 1e-8)
    for key, idx in (("fc_1.weight", (3, 5)), ("fc_2.weight", (2, 7)), ("fc_3.weight", (0, 4))):
        Pp = {k: np.asarray(v, np.float64).copy() for k, v in P.items()}
        Pm = {k: v.copy() for k, v in Pp.items()}
        Pp[key][idx] += 1e-6
        Pm[key][idx] -= 1e-6
        fd = ((hd.forward64(Pp, x, m1, m2)["z"] - hd.forward64(Pm, x, m1, m2)["z"]) * dz).sum() / 2e-6
        assert abs(fd - gr["g_" + key][idx]) <= 1e-7 * max(1.0, abs(fd)), key


@pytest.mark.parametrize("dim", DIMS)
def test_mlp_on_cpu_takes_the_torch_path_and_matches_the_fixture(g, dim):
    from zebra_amd.decoder import MLP
    from zebra_amd.losses import label_bce_loss, label_bce_plan
    pre = "d%d_" % dim
    m = MLP(dim, drop=0.0)
    assert list(m.state_dict().keys()) == [str(k) for k in g[pre + "keys"]]
    for (k, v), shp in zip(m.state_dict().items(), g[pre + "shapes"]):
        assert list(v.shape) == [int(s) for s in shp[:v.dim()]], k
    m.load_state_dict({k: torch.from_numpy(g[pre + k].astype(np.float32)) for k in hd.KEYS})
    x = torch.from_numpy(g[pre + "x"].astype(np.float32)).requires_grad_(True)
    y = torch.from_numpy(g[pre + "labels"].astype(np.float32))
    assert m._plan(x) == "torch" and label_bce_plan(x[:, 0], y) == "torch"
    m.eval()
    with torch.no_grad():
        z = m(x)
        assert torch.equal(m.predict(x), z.sigmoid())
    assert z.shape == (len(y),)
    assert np.abs(z.numpy() - g[pre + "logits"]).max() <= 1e-5
    m.train()
    loss = label_bce_loss(m(x).sigmoid(), y)
    loss.backward()
    assert abs(float(loss.detach()) - float(g[pre + "loss"])) <= 1e-5
    for k, p in m.named_parameters():
        want = g[pre + "g_" + k]
        assert np.abs(p.grad.numpy() - want).max() <= 1e-5 + 1e-4 * np.abs(want).max(), k
    want = g[pre + "d_x"]
    assert np.abs(x.grad.numpy() - want).max() <= 1e-5 + 1e-4 * np.abs(want).max()


def test_state_dict_is_the_reference_s(g):
    from zebra_amd.decoder import MLP
    assert tuple(MLP(40).state_dict().keys()) == hd.KEYS
    m = MLP(300)
    assert m.dropout.p == 0.3 and m.fc_1.in_features == 300 and m.fc_1.out_features == 80 and m.fc_2.out_features == 10
    import zebra_amd
    assert zebra_amd.MLP is MLP
    from zebra_amd.losses import label_bce_loss
    assert zebra_amd.label_bce_loss is label_bce_loss


# ---- the plans ------------------------------------------------------------------------------------------------------------
def test_python_plans_pick_as_documented():
    from zebra_amd.decoder import decoder_plan
    from zebra_amd.losses import label_bce_plan
    for H in hd.FWD_H + (40, 4348):
        assert decoder_plan("cuda", torch.float32, H) == "hip"
        assert decoder_plan("cuda", torch.float32, H, fused=False) == "torch"
        assert decoder_plan("cpu", torch.float32, H) == "torch"
        assert decoder_plan("cuda", torch.float64, H) == "torch"
        assert decoder_plan("cuda", torch.float16, H) == "torch"
    for H in (0, 2, 6, 301, 4356, 8192):
        assert decoder_plan("cuda", torch.float32, H) == "torch"
    # training batches beyond TRAIN_MAX_ROWS go to torch (measured slower there); eval keeps the kernels at every N
    from zebra_amd.decoder import TRAIN_MAX_ROWS
    assert TRAIN_MAX_ROWS == 16384
    assert decoder_plan("cuda", torch.float32, 300, rows=TRAIN_MAX_ROWS, training=True) == "hip"
    assert decoder_plan("cuda", torch.float32, 300, rows=TRAIN_MAX_ROWS + 1, training=True) == "torch"
    assert decoder_plan("cuda", torch.float32, 300, rows=1 << 20, training=False) == "hip"
    a, b = torch.rand(5), torch.rand(5)
    assert label_bce_plan(a, b) == "torch" and label_bce_plan(a.double(), b.double()) == "torch"


def plan(capi, N, H, training=False):
    return capi.decoder_plan(N, H, training)


def test_plan_reaches_the_seam_every_forward_case_names(capi):
    hooks = capi.hooks_lib()
    try:
        for case in hd.FWD_CASES:
            arr, N, H = case
            assert hooks.zt_test_decoder_arrangement(C.c_int32(arr)) == capi.ZT_OK
            want = hd.expected_launch(arr, N, H)
            for training in (False, True):
                got = plan(capi, N, H, training)
                for k in ("arrangement", "waves", "rows", "k_chunk", "grid"):
                    assert got[k] == want[k], (hd.fwd_id(case), k, got)
                assert got["lds_bytes"] == want["rows"] * (hd.K_CHUNK + 4) * 4 <= 160 * 1024
        assert hooks.zt_test_decoder_arrangement(C.c_int32(3)) == capi.ZT_ERR_ARG
    finally:
        hooks.zt_test_decoder_arrangement(C.c_int32(0))
    # what the lists are there for: both arrangements, a ragged and a whole last workgroup of each, one workgroup and several,
    # one K-chunk and several with a width on each side of every chunk seam up to 768, every H mod 16, the plan's own switch
    cases = set(hd.FWD_CASES)
    for arr in (hd.ARR_ONE, hd.ARR_FIVE):
        r = hd.ROWS[arr]
        assert {(arr, r, 300), (arr, r + 1, 300), (arr, 1, 300), (arr, 1000, 300)} <= cases
        for seam in (256, 512, 768):
            hs = [H for a, _, H in cases if a == arr]
            assert any(seam - hd.K_CHUNK < H <= seam for H in hs) and any(seam < H <= seam + hd.K_CHUNK for H in hs), seam
        assert {H % 16 for a, _, H in cases if a == arr} == {0, 4, 8, 12}
        assert (arr, 17, 4352) in cases and (arr, 17, 4) in cases
    for N in (1, 200, 4096, hd.BIG_N, 1 << 20):                  # unpinned: five waves per tile at every N
        assert plan(capi, N, 20)["arrangement"] == hd.ARR_FIVE and plan(capi, N, 4352, True)["arrangement"] == hd.ARR_FIVE
    assert set(hd.FWD_N) <= {N for _, N, _ in cases} and set(hd.FWD_H) <= {H for _, _, H in cases}


def test_plan_reaches_the_split_every_backward_case_names(capi):
    for N, H in hd.BWD_CASES + [(N, H) for _, N, H in hd.DROP_CASES]:
        got = plan(capi, N, H, True)
        split, kper = hd.expected_split(N, H)
        assert (got["split"], got["k_per"]) == (split, kper), (N, H, got)
        assert split * kper >= N > (split - 1) * kper and kper % 64 == 0
    for H in hd.BWD_H:
        assert plan(capi, hd.SPLIT_SEAM, H, True)["split"] == 1 and plan(capi, hd.SPLIT_SEAM + 1, H, True)["split"] == 2
    assert {plan(capi, N, 300, True)["split"] for N in hd.BWD_N} == {1, 2}
    assert plan(capi, 17, 4352, True)["split"] == 1
    assert set(hd.BWD_CASES) >= {(N, H) for N in (1, 16, 17, 65, 200, 273) for H in (4, 20, 300, 516)}


# ---- refusals before any device call ---------------------------------------------------------------------------------------
def test_refusals_need_no_device(capi):
    lib = capi.lib()
    w = capi.DecoderWeights()
    for f in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"):
        setattr(w, f, 4096)                                      # (never dereferenced: every call below is refused first)
    X, OUT = C.c_void_p(4096), C.c_void_p(8192)
    out = (C.c_int64 * 8)()
    for H in (0, 6, 4356):
        assert lib.zt_node_decoder_plan(C.c_int64(10), C.c_int32(H), C.c_int32(0), out) == capi.ZT_ERR_UNSUPPORTED
        assert lib.zt_node_decoder(X, C.c_int64(10), C.c_int32(H), C.byref(w), OUT, None, None) == capi.ZT_ERR_UNSUPPORTED
        assert lib.zt_node_decoder_train_forward(X, C.c_int64(10), C.c_int32(H), C.byref(w), C.c_float(0.0), C.c_uint64(0), OUT, OUT,
                                                 OUT, None) == capi.ZT_ERR_UNSUPPORTED
        assert lib.zt_node_decoder_train_backward(X, C.c_int64(10), C.c_int32(H), C.byref(w), X, X, X, C.c_float(0.0), C.c_uint64(0),
                                                  None, None, None, None, None, None, None, OUT, C.c_int64(10),
                                                  None) == capi.ZT_ERR_UNSUPPORTED
        assert lib.zt_node_decoder_train_workspace_bytes(C.c_int64(10), C.c_int32(H)) == -1
        assert b"unsupported" in lib.zt_last_error()
    assert lib.zt_node_decoder_train_workspace_bytes(C.c_int64(-1), C.c_int32(300)) == -1
    assert lib.zt_node_decoder_train_workspace_bytes(C.c_int64(200), C.c_int32(300)) >= 200 * 90 * 4 + 8 * 80 * 300 * 4
    # NULL pointers, N < 0, a misaligned x, p outside [0, 1)
    assert lib.zt_node_decoder_plan(C.c_int64(10), C.c_int32(300), C.c_int32(0), None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder_plan(C.c_int64(-1), C.c_int32(300), C.c_int32(0), out) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder(None, C.c_int64(10), C.c_int32(300), C.byref(w), OUT, None, None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder(X, C.c_int64(-1), C.c_int32(300), C.byref(w), OUT, None, None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder(X, C.c_int64(10), C.c_int32(300), None, OUT, None, None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder(C.c_void_p(4100), C.c_int64(10), C.c_int32(300), C.byref(w), OUT, None, None) == capi.ZT_ERR_ARG
    w2 = capi.DecoderWeights()
    C.memmove(C.byref(w2), C.byref(w), C.sizeof(w))
    w2.fc3_b = None
    assert lib.zt_node_decoder(X, C.c_int64(10), C.c_int32(300), C.byref(w2), OUT, None, None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder_train_forward(X, C.c_int64(10), C.c_int32(300), C.byref(w), C.c_float(0.0), C.c_uint64(0), OUT, None,
                                             OUT, None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder_train_forward(X, C.c_int64(10), C.c_int32(300), C.byref(w), C.c_float(1.0), C.c_uint64(0), OUT, OUT,
                                             OUT, None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder_train_backward(X, C.c_int64(10), C.c_int32(300), C.byref(w), X, X, None, C.c_float(0.0), C.c_uint64(0),
                                              None, None, None, None, None, None, None, OUT, C.c_int64(10), None) == capi.ZT_ERR_ARG
    assert lib.zt_node_decoder_train_backward(X, C.c_int64(10), C.c_int32(300), C.byref(w), X, X, X, C.c_float(0.0), C.c_uint64(0),
                                              None, None, None, None, None, None, None, OUT, C.c_int64(9), None) == capi.ZT_ERR_ARG
    # N = 0: ZT_OK, nothing touched (the pointers above are not memory)
    assert lib.zt_node_decoder(X, C.c_int64(0), C.c_int32(300), C.byref(w), OUT, OUT, None) == capi.ZT_OK
    assert lib.zt_node_decoder_train_forward(X, C.c_int64(0), C.c_int32(300), C.byref(w), C.c_float(0.3), C.c_uint64(1), OUT, OUT, OUT,
                                             None) == capi.ZT_OK
    assert lib.zt_node_decoder_train_backward(X, C.c_int64(0), C.c_int32(300), C.byref(w), X, X, X, C.c_float(0.3), C.c_uint64(1),
                                              None, OUT, OUT, OUT, OUT, OUT, OUT, OUT, C.c_int64(0), None) == capi.ZT_OK
    # the label loss
    for N in (0, -1):
        assert lib.zt_label_bce_forward(X, X, C.c_int64(N), OUT, OUT, None) == capi.ZT_ERR_ARG
        assert lib.zt_label_bce_backward(X, X, C.c_int64(N), OUT, None) == capi.ZT_ERR_ARG
    assert lib.zt_label_bce_forward(X, None, C.c_int64(4), OUT, OUT, None) == capi.ZT_ERR_ARG
    assert lib.zt_label_bce_backward(X, X, C.c_int64(4), None, None) == capi.ZT_ERR_ARG


def test_header_constants(capi):
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    assert "#define ZT_DECODER_H1 80" in hdr and "#define ZT_DECODER_H2 10" in hdr
    assert (capi.DECODER_H1, capi.DECODER_H2) == (hd.H1, hd.H2)
    assert len(capi.DECODER_PLAN_FIELDS) == 8 and "#define ZT_DECODER_PLAN_FIELDS 8" in hdr


# ---- the dropout mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.3, 0.999, 0.1])
def test_dropout_mask_statistics(p):
    from zebra_amd.decoder import decoder_dropout_mask
    from zebra_amd.modules import dropout_mask
    N = 4000
    m1, m2 = decoder_dropout_mask(12345678901234, p, N)
    assert m1.shape == (N, 80) and m2.shape == (N, 10) and m1.dtype == m2.dtype == np.float32
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for m in (m1, m2):
        assert set(np.unique(m)) <= {np.float32(0), scale}
        keep, n = float((m > 0).mean()), m.size
        assert abs(keep - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n), (keep, p)
    o1, o2 = decoder_dropout_mask(12345678901235, p, N)
    assert (o1 != m1).any() and (o2 != m2).any()
    # the two layers are independent: layer 2's mask is not a slice of layer 1's, and they agree as often as chance has it
    a, b = m1[:, :10] > 0, m2 > 0
    q = 1 - p
    agree, want = float((a == b).mean()), q * q + p * p
    assert abs(agree - want) <= 4 * np.sqrt(want * (1 - want) / a.size)
    # the same arithmetic as the aggregation's mask, at the decoder's element indices
    flat = dropout_mask(12345678901234, p, (1, 1, 1), N * 90).reshape(-1)
    assert np.array_equal(flat[:N * 80].reshape(N, 80), m1) and np.array_equal(flat[N * 80:].reshape(N, 10), m2)
    z1, z2 = decoder_dropout_mask(5, 0.0, 7)
    assert np.all(z1 == 1) and np.all(z2 == 1)


# ---- node_auc -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,levels", [(0, 0), (1, 5), (2, 2), (3, 40)])
def test_node_auc_against_exact_counts(seed, levels):
    from zebra_amd.evaluation import node_auc
    rng = np.random.RandomState(seed)
    n = 300
    prob = rng.rand(n).astype(np.float32)
    if levels:
        prob = (np.floor(prob * levels) / levels).astype(np.float32)     # heavy ties
    labels = (rng.rand(n) < 0.2).astype(np.float64)
    got = float(node_auc(torch.from_numpy(prob), torch.from_numpy(labels)))
    want = metrics_exact.auc_pairwise(prob[labels == 1], prob[labels == 0])
    assert abs(got - float(want)) <= 1e-12
    try:
        from sklearn.metrics import roc_auc_score
    except ImportError:
        roc_auc_score = None
    if roc_auc_score is not None:
        assert abs(got - roc_auc_score(labels, prob)) <= 1e-12
    assert abs(float(node_auc(prob, labels)) - got) == 0                 # numpy in: the same


def test_node_auc_refuses_a_single_class():
    from zebra_amd.evaluation import node_auc
    p = torch.rand(10)
    for lab in (torch.zeros(10), torch.ones(10)):
        with pytest.raises(ValueError, match="one class"):
            node_auc(p, lab)
    with pytest.raises(ValueError):
        node_auc(p, torch.ones(9))
    assert float(node_auc(torch.tensor([0.5, 0.5]), torch.tensor([1.0, 0.0]))) == 0.5
    assert float(node_auc(torch.tensor([0.9, 0.1]), torch.tensor([1.0, 0.0]))) == 1.0


# ---- the committed seeds ---------------------------------------------------------------------------------------------------
def test_every_committed_seed_is_the_first_that_meets_the_margin_condition():
    keys = [(N, H, 0.0) for N, H in hd.BWD_CASES] + [(N, H, p) for p, N, H in hd.DROP_CASES]
    assert sorted(keys) == sorted(hd.SEEDS)
    for N, H, p in keys:
        assert hd.SEEDS[(N, H, p)] == hd.first_good_seed(N, H, p), (N, H, p)
        f = hd.bwd_case(N, H, p)[5]
        assert hd.margin_ok(f)
    # the condition is not vacuous: a draw with a unit planted on zero fails it
    P, x, _ = hd.draw_case(17, 20, hd.SEEDS[(17, 20, 0.0)])
    P = dict(P)
    P["fc_1.bias"] = P["fc_1.bias"].copy()
    P["fc_1.bias"][3] -= np.float32(hd.forward64(P, x)["pre1"][5, 3])
    assert not hd.margin_ok(hd.forward64(P, x))
