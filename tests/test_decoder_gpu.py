"""Node classification on the GPU (csrc/decoder.hip, the label loss of csrc/train_tail.hip, zebra_amd/decoder.py,
evaluation.eval_node_classification, TGN.classify_nodes) against the float64 restatement of tests/helpers_decoder.py, which
tests/test_decoder_cpu.py pins to the reference's fixture; that file also shows that every case below reaches the seam of
zt_node_decoder_plan it names and that every backward seed meets the margin condition.

Bounds, taken from the suite and not fitted:
  logits          |z - z64| <= 1e-5 max(1, max|z64|)
  probabilities   |p - p64| <= p64 (1 - p64) 1e-5 max(1, max|z64|) + 2^-23
  d_x             within 1e-5 max(1, max|ref|);  the six parameter gradients within 1e-5 + 1e-4 max|ref|
torch's float32 composition on the device is held to HALF of the forward bounds.
Every kernel case runs twice with equal bits; x is once the tail and once the head of a larger NaN-filled allocation; the
outputs sit in front of a sentinel; the six parameters are views into one flat buffer with NaN between and around them.

Figures measured on an MI355X: DESIGN.md section 5, "Node classification"."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import inputs as I
from conftest import golden
import helpers_decoder as hd
from helpers import build_tgn

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
H1, H2 = hd.H1, hd.H2


@pytest.fixture(scope="module")
def capi():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd import _capi
    return _capi


def dev():
    return torch.device("cuda")


def flat_params(P):
    """The six parameters as views into ONE flat buffer with NaN between and around them; only fc_1.weight is 16-byte
    aligned (four NaN in front; the gaps behind are 3, 1, 1, 2, 1 floats: the others lie at odd offsets)."""
    gaps = (4, 3, 1, 1, 2, 1)
    total = sum(gaps) + sum(P[k].size for k in hd.KEYS) + 5
    buf = torch.full((total,), float("nan"), dtype=torch.float32, device=dev())
    views, o = [], 0
    for k, gap in zip(hd.KEYS, gaps):
        o += gap
        n = P[k].size
        buf[o:o + n] = torch.from_numpy(np.ascontiguousarray(P[k]).reshape(-1)).to(dev())
        views.append(buf[o:o + n].view(P[k].shape))
        o += n
    assert views[0].data_ptr() % 16 == 0
    return buf, views


def weights_struct(capi, views):
    w = capi.DecoderWeights()
    w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b, w.fc3_w, w.fc3_b = (v.data_ptr() for v in views)
    return w


def place_x(x, head):
    """x [N][H] inside a larger NaN-filled allocation: its head (NaN behind) or its tail (64 NaN in front)"""
    n = x.size
    buf = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=dev())
    o = 0 if head else 64
    buf[o:o + n] = torch.from_numpy(x.reshape(-1)).to(dev())
    v = buf[o:o + n].view(x.shape)
    assert v.data_ptr() % 16 == 0
    return buf, v


def out_buf(*shape):
    """an output in front of a sentinel: (whole buffer, the view the kernel writes)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=dev())
    return buf, buf[:n].view(shape)


def sentinel_ok(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_eval(capi, x, w, want_logit=True, want_prob=True):
    N, H = x.shape
    lb, logit = out_buf(N)
    pb, prob = out_buf(N)
    capi.check(capi.lib().zt_node_decoder(ptr(x), C.c_int64(N), C.c_int32(H), C.byref(w), ptr(logit) if want_logit else None,
                                          ptr(prob) if want_prob else None, capi.stream_ptr()), "zt_node_decoder")
    torch.cuda.synchronize()
    assert sentinel_ok(lb, N) and sentinel_ok(pb, N)
    return logit.cpu().numpy(), prob.cpu().numpy()


def run_train_fwd(capi, x, w, p=0.0, seed=0):
    N, H = x.shape
    lb, logit = out_buf(N)
    b1, h1 = out_buf(N, H1)
    b2, h2 = out_buf(N, H2)
    capi.check(capi.lib().zt_node_decoder_train_forward(ptr(x), C.c_int64(N), C.c_int32(H), C.byref(w), C.c_float(p),
                                                        C.c_uint64(seed), ptr(logit), ptr(h1), ptr(h2), capi.stream_ptr()),
               "zt_node_decoder_train_forward")
    torch.cuda.synchronize()
    assert sentinel_ok(lb, N) and sentinel_ok(b1, N * H1) and sentinel_ok(b2, N * H2)
    return logit, h1, h2


def run_bwd(capi, x, w, h1, h2, dz, p=0.0, seed=0, want_dx=True):
    """dict(d_x, g_<key>) as numpy; every output in front of a sentinel"""
    N, H = x.shape
    shapes = [(N, H), (H1, H), (H1,), (H2, H1), (H2,), (1, H2), (1,)]
    bufs = [out_buf(*s) for s in shapes]
    if not want_dx:
        bufs[0] = (None, None)
    need = int(capi.lib().zt_node_decoder_train_workspace_bytes(C.c_int64(N), C.c_int32(H)))
    assert need > 0
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev())
    capi.check(capi.lib().zt_node_decoder_train_backward(ptr(x), C.c_int64(N), C.c_int32(H), C.byref(w), ptr(h1), ptr(h2), ptr(dz),
                                                         C.c_float(p), C.c_uint64(seed), *[ptr(v) for _, v in bufs], ptr(ws),
                                                         C.c_int64(N), capi.stream_ptr()), "zt_node_decoder_train_backward")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the workspace was overrun"
    out = {}
    for name, (b, v), s in zip(("d_x",) + tuple("g_" + k for k in hd.KEYS), bufs, shapes):
        if v is None:
            continue
        assert sentinel_ok(b, int(np.prod(s))), name
        out[name] = v.cpu().numpy()
    return out


def torch_forward(views, x):
    w1, b1, w2, b2, w3, b3 = views
    h = torch.relu(torch.nn.functional.linear(x, w1, b1))
    h = torch.relu(torch.nn.functional.linear(h, w2, b2))
    return torch.nn.functional.linear(h, w3, b3).squeeze(1)


@pytest.fixture
def pin(capi):
    hooks = capi.hooks_lib()

    def set_pin(v):
        assert hooks.zt_test_decoder_arrangement(C.c_int32(v)) == capi.ZT_OK
    yield set_pin
    hooks.zt_test_decoder_arrangement(C.c_int32(0))


# ---- forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hd.FWD_CASES, ids=hd.fwd_id)
def test_forward_against_float64(capi, pin, case):
    arr, N, H = case
    pin(arr)
    assert capi.decoder_plan(N, H)["arrangement"] == hd.expected_launch(arr, N, H)["arrangement"]
    P, x, f = hd.fwd_case(N, H)
    z64 = f["z"]
    _, views = flat_params(P)
    w = weights_struct(capi, views)
    _, x_tail = place_x(x, head=False)
    _, x_head = place_x(x, head=True)
    z1, p1 = run_eval(capi, x_tail, w)
    z2, p2 = run_eval(capi, x_head, w)
    assert np.array_equal(z1.view(np.uint32), z2.view(np.uint32)) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    zl, _ = run_eval(capi, x_head, w, want_prob=False)          # either output may be NULL
    _, pl = run_eval(capi, x_head, w, want_logit=False)
    assert np.array_equal(zl, z1) and np.array_equal(pl, p1)
    logit, h1, h2 = run_train_fwd(capi, x_tail, w)              # the training entry at p = 0: the same bits
    assert np.array_equal(logit.cpu().numpy().view(np.uint32), z1.view(np.uint32))
    for got, name in ((h1, "h1"), (h2, "h2")):
        want = f[name]
        assert np.abs(got.cpu().numpy() - want).max() <= hd.TOL_LINEAR * max(1.0, np.abs(want).max()), name
    zb, pb = hd.logit_bound(z64), hd.prob_bound(z64)
    p64 = hd.sigmoid64(z64)
    ez, ep = np.abs(z1 - z64).max(), (np.abs(p1 - p64) / pb).max()
    zt = torch_forward(views, x_head)
    tz, tp = np.abs(zt.cpu().numpy() - z64).max(), (np.abs(zt.sigmoid().cpu().numpy() - p64) / pb).max()
    print("%s: logits %.3g of %.3g (torch %.3g), probabilities %.3f of the bound (torch %.3f)" % (hd.fwd_id(case), ez, zb, tz, ep, tp))
    assert np.isfinite(z1).all() and np.isfinite(p1).all()
    assert tz <= 0.5 * zb and tp <= 0.5, "torch's float32 composition must fit half the bound"
    assert ez <= zb and ep <= 1.0


def test_arrangements_give_the_same_bits(capi, pin):
    P, x, _ = hd.fwd_case(200, 516)
    _, views = flat_params(P)
    w = weights_struct(capi, views)
    _, xd = place_x(x, head=True)
    res = []
    for arr in (hd.ARR_ONE, hd.ARR_FIVE):
        pin(arr)
        res.append(run_eval(capi, xd, w))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- backward --------------------------------------------------------------------------------------------------------------
def check_backward(capi, N, H, p):
    P, x, dz, m1, m2, f, g = hd.bwd_case(N, H, p)
    seed = hd.drop_seed(p, N, H) if p else 0
    _, views = flat_params(P)
    w = weights_struct(capi, views)
    _, xd = place_x(x, head=True)
    dzd = torch.from_numpy(dz).to(dev())
    logit, h1, h2 = run_train_fwd(capi, xd, w, p, seed)
    logit_b, h1_b, h2_b = run_train_fwd(capi, xd, w, p, seed)
    assert torch.equal(logit, logit_b) and torch.equal(h1, h1_b) and torch.equal(h2, h2_b)
    z = logit.cpu().numpy()
    assert np.abs(z - f["z"]).max() <= hd.logit_bound(f["z"])
    if p:
        assert bool((h1.cpu().numpy()[m1 == 0] == 0).all()) and bool((h2.cpu().numpy()[m2 == 0] == 0).all())
        for got, name in ((h1, "h1"), (h2, "h2")):
            assert np.abs(got.cpu().numpy() - f[name]).max() <= hd.TOL_LINEAR * max(1.0, np.abs(f[name]).max()), name
    a = run_bwd(capi, xd, w, h1, h2, dzd, p, seed, want_dx=True)
    b = run_bwd(capi, xd, w, h1, h2, dzd, p, seed, want_dx=True)
    c = run_bwd(capi, xd, w, h1, h2, dzd, p, seed, want_dx=False)
    assert "d_x" not in c
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "two runs differ in %s" % k
        if k != "d_x":
            assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), "%s depends on d_x being asked for" % k
    ok, frac = hd.dx_ok(a["d_x"], g["d_x"])
    worst = {"d_x": frac}
    assert ok, "d_x: %.3g of the bound" % frac
    for k in hd.KEYS:
        ok, frac = hd.grad_ok(a["g_" + k], g["g_" + k])
        worst[k] = frac
        assert ok, "%s: %.3g of the bound" % (k, frac)
    print("N=%d H=%d p=%g: share of the bound used: %s" % (N, H, p, ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("N,H", hd.BWD_CASES, ids=["N%d-H%d-split%d" % (N, H, hd.expected_split(N, H)[0]) for N, H in hd.BWD_CASES])
def test_backward_against_float64(capi, N, H):
    assert capi.decoder_plan(N, H, True)["split"] == hd.expected_split(N, H)[0]
    check_backward(capi, N, H, 0.0)


@pytest.mark.parametrize("p,N,H", hd.DROP_CASES, ids=["p%g-N%d-H%d" % c for c in hd.DROP_CASES])
def test_dropout_against_float64_with_the_numpy_masks(capi, p, N, H):
    check_backward(capi, N, H, p)


# ---- the label loss --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 4097])
@pytest.mark.parametrize("kind", ["zeros", "ones", "mixed"])
def test_label_bce_against_float64(capi, N, kind):
    from zebra_amd.losses import label_bce_loss, label_bce_plan
    rng = np.random.RandomState(N + len(kind))
    prob = rng.rand(N).astype(np.float32)
    prob[0] = 0.0                                                # the clamps: log at -100, the quotient at 1e-12
    if N > 1:
        prob[-1] = 1.0
    if N > 255:
        prob[7], prob[8] = 1.0, 0.0
    y = {"zeros": np.zeros(N), "ones": np.ones(N), "mixed": (rng.rand(N) < 0.5).astype(np.float64)}[kind].astype(np.float32)
    want_loss, want_d = hd.bce64(prob, y)
    pd = torch.from_numpy(prob).to(dev()).requires_grad_(True)
    yd = torch.from_numpy(y).to(dev())
    assert label_bce_plan(pd, yd) == "hip"
    loss = label_bce_loss(pd, yd)
    loss.backward()
    again = label_bce_loss(pd.detach(), yd)
    assert torch.equal(loss.detach(), again)
    assert abs(float(loss.detach()) - want_loss) <= 1e-6 * abs(want_loss)
    got = pd.grad.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - want_d) <= 1e-6 * np.abs(want_d))
    # a scaled incoming gradient is applied on the device
    pd.grad = None
    (3.0 * label_bce_loss(pd, yd)).backward()
    assert np.all(np.abs(pd.grad.cpu().numpy().astype(np.float64) - 3.0 * want_d) <= 2e-6 * np.abs(3.0 * want_d))
    # torch's own loss on the device agrees (float32: 1e-5)
    t = torch.nn.BCELoss()(pd.detach(), yd)
    assert abs(float(t) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))


# ---- the fixture through the module ----------------------------------------------------------------------------------------
@pytest.fixture
def decoder_calls(monkeypatch, capi):
    """[n]: calls of lib().zt_node_decoder_train_forward from here on"""
    lib = capi.lib()
    calls, fwd = [0], lib.zt_node_decoder_train_forward

    def counted(*args):
        calls[0] += 1
        return fwd(*args)

    monkeypatch.setattr(lib, "zt_node_decoder_train_forward", counted)
    return calls


@pytest.mark.parametrize("dim", [40, 300])
def test_mlp_on_the_gpu_matches_the_reference_fixture(capi, decoder_calls, dim):
    from zebra_amd.decoder import MLP
    from zebra_amd.losses import label_bce_loss
    g = golden("g14_node_decoder")
    pre = "d%d_" % dim
    m = MLP(dim, drop=0.0)
    m.load_state_dict({k: torch.from_numpy(g[pre + k].astype(np.float32)) for k in hd.KEYS})
    m = m.to(dev())
    x = torch.from_numpy(g[pre + "x"].astype(np.float32)).to(dev()).requires_grad_(True)
    y = torch.from_numpy(g[pre + "labels"].astype(np.float32)).to(dev())
    assert m._plan(x) == "hip"
    m.eval()
    with torch.no_grad():
        z = m(x)
        assert torch.equal(m.predict(x), torch.from_numpy(run_eval(capi, x.detach(), weights_struct(capi, list(m._params())))[1]).to(dev()))
    assert decoder_calls[0] == 0
    assert z.shape == (len(y),) and np.abs(z.cpu().numpy() - g[pre + "logits"]).max() <= 1e-5
    m.train()
    loss = label_bce_loss(m(x).sigmoid(), y)
    loss.backward()
    assert decoder_calls[0] == 1
    assert abs(float(loss.detach()) - float(g[pre + "loss"])) <= 1e-5
    for k, p in m.named_parameters():
        want = g[pre + "g_" + k]
        assert np.abs(p.grad.cpu().numpy() - want).max() <= 1e-5 + 1e-4 * np.abs(want).max(), k
    want = g[pre + "d_x"]
    assert np.abs(x.grad.cpu().numpy() - want).max() <= 1e-5 + 1e-4 * np.abs(want).max()
    # fused_decoder = False: torch's composition, the same results at the same tolerances, no kernel call
    m.fused_decoder = False
    assert m._plan(x) == "torch"
    m.zero_grad()
    loss_t = label_bce_loss(m(x).sigmoid(), y)
    assert decoder_calls[0] == 1 and abs(float(loss_t.detach()) - float(g[pre + "loss"])) <= 1e-5


def test_module_dropout_draws_a_seed_per_forward(capi):
    from zebra_amd.decoder import MLP, decoder_dropout_mask
    m = MLP(20, drop=0.3).to(dev()).train()
    x = torch.randn(50, 20, device=dev())
    torch.manual_seed(5)
    a = m(x)
    s1 = m._last_drop_seed
    b = m(x)
    s2 = m._last_drop_seed
    assert s1 != s2 and not torch.equal(a, b)
    torch.manual_seed(5)
    a2 = m(x)
    assert m._last_drop_seed == s1 and torch.equal(a.detach(), a2.detach())
    P = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    m1, m2 = decoder_dropout_mask(s1, 0.3, 50)
    z64 = hd.forward64(P, x.cpu().numpy(), m1, m2)["z"]
    assert np.abs(a.detach().cpu().numpy() - z64).max() <= hd.logit_bound(z64)
    m.eval()
    assert torch.equal(m(x), m(x))


# ---- the protocol ----------------------------------------------------------------------------------------------------------
def _model_state(tgn):
    m = tgn.memory
    st = {kk: getattr(m, kk).cpu().numpy().copy() for kk in ("memory", "last_update", "messages", "timestamps", "_flag_buf")}
    em = tgn.embedding_module
    for mi in range(em.n_tppr):
        for kk, v in em.tppr_finder.export_state(mi).items():
            st["tppr%d_%s" % (mi, kk)] = v
    return st


def _protocol():
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES["d20_f7"]
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    labels = (np.random.RandomState(seed).rand(E) < 0.3).astype(np.float64)
    assert 0 < labels.sum() < E
    data = types.SimpleNamespace(sources=src, destinations=dst, timestamps=ts, edge_idxs=eidx, labels=labels, n_interactions=E)
    make = lambda: build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    return data, make, D * (len(al) + 1), bs


def _decoder(dim, seed=11, drop=0.0):
    from zebra_amd.decoder import MLP
    torch.manual_seed(seed)
    return MLP(dim, drop=drop).to(dev())


def test_eval_node_classification_is_the_batch_loop(capi):
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import metrics_exact
    from zebra_amd.evaluation import eval_node_classification
    data, make, dim, bs = _protocol()
    dec = _decoder(dim)
    a, b = make(), make()
    got = eval_node_classification(a, dec, data, bs, 10)
    assert isinstance(got, float) and not dec.training and not a.training
    b.eval()
    probs = []
    E = len(data.sources)
    for s in range(0, E, bs):
        e = min(E, s + bs)
        with torch.no_grad():
            emb, _, _ = b.compute_temporal_embeddings(data.sources[s:e], data.destinations[s:e], data.destinations[s:e],
                                                      data.timestamps[s:e], data.edge_idxs[s:e], 10, train=False)
            probs.append(dec.predict(emb).cpu().numpy())
    prob = np.concatenate(probs)
    want = float(metrics_exact.auc_pairwise(prob[data.labels == 1], prob[data.labels == 0]))
    assert abs(got - want) <= 1e-12
    sa, sb = _model_state(a), _model_state(b)
    for kk in sa:
        assert np.array_equal(sa[kk], sb[kk]), kk
    one = types.SimpleNamespace(**vars(data))
    one.labels = np.zeros(E)
    with pytest.raises(ValueError, match="one class"):
        eval_node_classification(make(), dec, one, bs, 10)


def test_classify_nodes_is_read_only(capi):
    data, make, dim, bs = _protocol()
    dec = _decoder(dim).eval()
    tgn = make().eval()
    with pytest.raises(RuntimeError):                            # a fresh model is not in test mode
        tgn.classify_nodes(dec, data.sources[:3], data.timestamps[:3])
    for s in range(0, 3 * bs, bs):
        with torch.no_grad():
            tgn.compute_temporal_embeddings(data.sources[s:s + bs], data.destinations[s:s + bs], data.destinations[s:s + bs],
                                            data.timestamps[s:s + bs], data.edge_idxs[s:s + bs], 10, train=False)
    s, e = 3 * bs, 4 * bs
    nodes, ts = np.concatenate([data.sources[s:e], data.destinations[s:e]]), np.concatenate([data.timestamps[s:e]] * 2)
    before = _model_state(tgn)
    counter = tgn.batch_counter
    got = tgn.classify_nodes(dec, nodes, ts)
    after = _model_state(tgn)
    for kk in before:
        assert np.array_equal(before[kk], after[kk]), "classify_nodes changed %s" % kk
    assert tgn.batch_counter == counter
    want = dec.predict(tgn.embed_nodes(nodes, ts))
    assert got.shape == (2 * bs,) and torch.equal(got, want)
    assert bool(((got > 0) & (got < 1)).all())
    tgn.test_mode = False
    with pytest.raises(RuntimeError):
        tgn.classify_nodes(dec, nodes, ts)


def test_train_epoch_fused_against_the_torch_composition(capi, decoder_calls):
    """Three epochs (consecutive thirds of the stream, the model's state carried on) of the fused path with zebra_amd.Adam
    against fused_decoder = False with torch.optim.Adam, from the same state and parameters, drop = 0."""
    import zebra_amd
    from zebra_amd.decoder import train_epoch
    data, make, dim, bs = _protocol()
    E = len(data.sources)
    third = E // 3
    parts = [types.SimpleNamespace(**{k: getattr(data, k)[i * third:(i + 1) * third]
                                      for k in ("sources", "destinations", "timestamps", "edge_idxs", "labels")}) for i in range(3)]
    nb = sum((third + bs - 1) // bs for _ in parts)
    res = {}
    for fused in (True, False):
        tgn, dec = make(), _decoder(dim, seed=3)
        dec.fused_decoder = fused
        opt = (zebra_amd.Adam if fused else torch.optim.Adam)(dec.parameters(), lr=1e-3)
        before = decoder_calls[0]
        losses = [train_epoch(tgn, dec, opt, part, bs, 10) for part in parts]
        assert decoder_calls[0] - before == (nb if fused else 0)
        assert dec.training and not tgn.training
        res[fused] = (losses, {k: v.detach().cpu().numpy() for k, v in dec.state_dict().items()})
    for a, b in zip(*[res[f][0] for f in (True, False)]):
        assert np.isfinite(a) and abs(a - b) <= 1e-5, (a, b)
    for k in hd.KEYS:
        a, b = res[True][1][k], res[False][1][k]
        assert np.abs(a - b).max() <= 1e-5 + 1e-4 * np.abs(b).max(), k
    start = _decoder(dim, seed=3).state_dict()
    assert any(np.abs(res[True][1][k] - start[k].cpu().numpy()).max() > 2e-3 for k in hd.KEYS), "the epochs trained nothing"
