"""The pair scorer's and the node decoder's training kernels (csrc/scoring_train.hip, csrc/decoder.hip) held to exact results
on the device, through the C-ABI (tests/helpers_train_exact.py; tests/test_train_exact_cpu.py proves the cases' premises):
  A  small-integer inputs at every seam of the tiling and of the backward's plan: the hidden rows, the decoder's logits and
     every gradient have the bits of the float64 composition rounded once -- no tolerance --, twice per call; the plan entry is
     asked first and is the restatement's; the scorer's probabilities are within tests/test_scoring_f64_gpu.py's bound;
  B  outputs left out (every one alone, d_fc1_w alone, all parameter gradients) and a workspace planned for a larger batch:
     what is written keeps the bits of the full call;
  C  random inputs at the same seams, held elementwise to L 2^-24 A + ulp (the helper derives L).
Every input is the tail of a NaN-filled allocation, the parameters lie in one flat NaN-filled buffer, every output sits in
front of a sentinel, and the workspace, of exactly the asked size and filled with 0xA5, is followed by a guard.
Figures measured on an MI355X: DESIGN.md, "The pair scorer's and the decoder's training kernels, held to exact sums"."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import helpers_decoder as hd
import helpers_train_exact as X

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
NAN = float("nan")
H1, H2 = X.H1, X.H2


@pytest.fixture(scope="module")
def capi():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd import _capi
    return _capi


@pytest.fixture(scope="module", autouse=True)
def total_time():
    t = time.time()
    yield
    print("\ntests/test_train_exact_gpu.py: %.1f s in all" % (time.time() - t))


@pytest.fixture
def pin(capi):
    hooks = capi.hooks_lib()

    def set_pin(v):
        assert hooks.zt_test_decoder_arrangement(C.c_int32(v)) == capi.ZT_OK
    yield set_pin
    hooks.zt_test_decoder_arrangement(C.c_int32(0))


def place(a):
    """a float32 numpy array as the 16-byte-aligned TAIL of a NaN-filled allocation: (allocation, view)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    n = t.numel()
    buf = torch.full((64 + n,), NAN, dtype=torch.float32, device="cuda")
    buf[64:] = t.reshape(-1).cuda()
    v = buf[64:].view(t.shape)
    assert v.data_ptr() % 16 == 0
    return v


class Out:
    """an output of ``shape`` in front of a sentinel"""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        self.view = self.buf[:self.n].view(shape)

    def intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())

    def numpy(self):
        return self.view.cpu().numpy()


def flat_params(arrays, gaps):
    """the parameters as views into ONE flat NaN-filled buffer, ``gaps`` NaN in front of each"""
    buf = torch.full((sum(gaps) + sum(a.size for a in arrays) + 7,), NAN, dtype=torch.float32, device="cuda")
    views, o = [], 0
    for a, gap in zip(arrays, gaps):
        o += gap
        buf[o:o + a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).cuda()
        views.append(buf[o:o + a.size].view(a.shape))
        o += a.size
    return buf, views


def workspace(need):
    return torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")


def bits(a):
    return (np.ascontiguousarray(a, dtype=np.float32) + np.float32(0)).view(np.uint32)       # (the sign of a zero is not held)


def assert_bits(got, want, what):
    if not X.np_bits_equal(got, want):
        g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        bad = np.flatnonzero(bits(g) != bits(w))
        raise AssertionError("%s differs from the exact sums at %d of %d elements, first at flat index %d: %r, exact %r"
                             % (what, bad.size, g.size, int(bad[0]), float(g[bad[0]]), float(w[bad[0]])))


# ---- the pair scorer through the C-ABI -------------------------------------------------------------------------------------
class Score:
    def __init__(self, capi, case, emb, wts):
        self.capi, self.lib, self.B, self.H = capi, capi.lib(), case.n, case.H
        self.emb = place(emb)
        self.pbuf, self.params = flat_params(wts, (4, 4, 4, 1))          # fc1.weight, fc1.bias, fc2.weight aligned; fc2.bias at an odd offset
        assert all(v.data_ptr() % 16 == 0 for v in self.params[:3]) and (self.params[3].data_ptr() // 4) % 2 == 1
        self.wt = capi.AffinityWeights(*[capi.ptr(v) for v in self.params])

    def forward(self):
        B, H, ptr = self.B, self.H, self.capi.ptr
        prob, hid = Out((2 * B,)), Out((2 * B, H))
        self.capi.check(self.lib.zt_affinity_train_forward(ptr(self.emb), C.c_int64(B), C.c_int32(H), C.byref(self.wt), ptr(prob.view),
                                                           ptr(hid.view), self.capi.stream_ptr()), "zt_affinity_train_forward")
        torch.cuda.synchronize()
        assert prob.intact() and hid.intact(), "the forward wrote outside an output"
        return prob.numpy(), hid.numpy()

    def backward(self, prob, hid, dprob, want=(True,) * 5, ws_max_B=None):
        """[the five outputs (X.SCORE_OUT) or None] of one call on the given prob / hid / dprob"""
        B, H, ptr = self.B, self.H, self.capi.ptr
        ws_max_B = B if ws_max_B is None else ws_max_B
        shapes = [(3 * B, H), (H, 2 * H), (H,), (1, H), (1,)]
        outs = [Out(s) if w else None for s, w in zip(shapes, want)]
        need = int(self.lib.zt_affinity_train_workspace_bytes(C.c_int64(ws_max_B), C.c_int32(H)))
        assert need > 0
        ws = workspace(need)
        p, h, dp = place(prob), place(hid), place(dprob)
        self.capi.check(self.lib.zt_affinity_train_backward(
            ptr(self.emb), C.c_int64(B), C.c_int32(H), C.byref(self.wt), ptr(p), ptr(h), ptr(dp),
            *[None if o is None else ptr(o.view) for o in outs], ptr(ws), C.c_int64(ws_max_B), self.capi.stream_ptr()),
            "zt_affinity_train_backward")
        torch.cuda.synchronize()
        for name, o in zip(X.SCORE_OUT, outs):
            assert o is None or o.intact(), "the backward wrote outside %s" % name
        assert bool((ws[need:] == 0xA5).all()), "the workspace was overrun"
        return [None if o is None else o.numpy() for o in outs]


def prob_share(prob, s64):
    """the largest share of tests/test_scoring_f64_gpu.py's bound any probability uses"""
    return float((np.abs(prob.astype(np.float64) - hd.sigmoid64(s64)) / hd.prob_bound(s64)).max())


# ---- the decoder through the C-ABI -----------------------------------------------------------------------------------------
class Dec:
    def __init__(self, capi, case, P, x):
        self.capi, self.lib, self.case, self.N, self.H = capi, capi.lib(), case, case.n, case.H
        self.x = place(x)
        self.pbuf, self.params = flat_params([P[k] for k in hd.KEYS], (4, 3, 1, 1, 2, 1))     # only fc_1.weight is aligned
        assert self.params[0].data_ptr() % 16 == 0
        self.wt = capi.DecoderWeights()
        self.wt.fc1_w, self.wt.fc1_b, self.wt.fc2_w, self.wt.fc2_b, self.wt.fc3_w, self.wt.fc3_b = (v.data_ptr() for v in self.params)
        self.p = case.p
        self.seed = case.drop_seed() if case.p else 0

    def eval(self):
        N, H, ptr = self.N, self.H, self.capi.ptr
        logit = Out((N,))
        self.capi.check(self.lib.zt_node_decoder(ptr(self.x), C.c_int64(N), C.c_int32(H), C.byref(self.wt), ptr(logit.view), None,
                                                 self.capi.stream_ptr()), "zt_node_decoder")
        torch.cuda.synchronize()
        assert logit.intact()
        return logit.numpy()

    def forward(self):
        N, H, ptr = self.N, self.H, self.capi.ptr
        logit, h1, h2 = Out((N,)), Out((N, H1)), Out((N, H2))
        self.capi.check(self.lib.zt_node_decoder_train_forward(ptr(self.x), C.c_int64(N), C.c_int32(H), C.byref(self.wt), C.c_float(self.p),
                                                               C.c_uint64(self.seed), ptr(logit.view), ptr(h1.view), ptr(h2.view),
                                                               self.capi.stream_ptr()), "zt_node_decoder_train_forward")
        torch.cuda.synchronize()
        assert logit.intact() and h1.intact() and h2.intact(), "the forward wrote outside an output"
        return logit.numpy(), h1.numpy(), h2.numpy()

    def backward(self, h1, h2, dz, want=(True,) * 7, ws_max_N=None):
        """[the seven outputs (X.DEC_OUT) or None] of one call on the given h1 / h2 / dz"""
        N, H, ptr = self.N, self.H, self.capi.ptr
        ws_max_N = N if ws_max_N is None else ws_max_N
        shapes = [(N, H), (H1, H), (H1,), (H2, H1), (H2,), (1, H2), (1,)]
        outs = [Out(s) if w else None for s, w in zip(shapes, want)]
        need = int(self.lib.zt_node_decoder_train_workspace_bytes(C.c_int64(ws_max_N), C.c_int32(H)))
        assert need > 0
        ws = workspace(need)
        a, b, d = place(h1), place(h2), place(dz)
        self.capi.check(self.lib.zt_node_decoder_train_backward(
            ptr(self.x), C.c_int64(N), C.c_int32(H), C.byref(self.wt), ptr(a), ptr(b), ptr(d), C.c_float(self.p), C.c_uint64(self.seed),
            *[None if o is None else ptr(o.view) for o in outs], ptr(ws), C.c_int64(ws_max_N), self.capi.stream_ptr()),
            "zt_node_decoder_train_backward")
        torch.cuda.synchronize()
        for name, o in zip(X.DEC_OUT, outs):
            assert o is None or o.intact(), "the backward wrote outside %s" % name
        assert bool((ws[need:] == 0xA5).all()), "the workspace was overrun"
        return [None if o is None else o.numpy() for o in outs]


def ask_plan(capi, case):
    """the plan entry, asked first: it must be the restatement's"""
    got = capi.score_train_plan(case.n, case.H) if case.kind == "score" else capi.decoder_plan(case.n, case.H, True)
    want = case.plan()
    assert all(got[k] == want[k] for k in got if k in want), (case.id, got, want)
    assert X.crossed(case)
    return got


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.SCORE_CASES, ids=repr)
def test_scorer_exact_sums(capi, case):
    ask_plan(capi, case)
    d = X.exact_reference(case.id)
    k = Score(capi, case, d["emb"], d["wts"])
    for run in (1, 2):
        prob, hid = k.forward()
        assert_bits(hid, d["hid"], "%s run %d: hid" % (case.id, run))
        share = prob_share(prob, d["s64"])
        assert share <= 1.0, "%s: a probability uses %.3g of its bound" % (case.id, share)
        if run == 1:
            first = prob
        assert np.array_equal(bits(prob), bits(first)), "two runs give different probabilities"
        got = k.backward(d["prob"], d["hid"], d["dprob"])
        for name, g, w in zip(X.SCORE_OUT, got, d["out"]):
            assert_bits(g, w, "%s run %d: %s" % (case.id, run, name))


@pytest.mark.parametrize("case", X.DEC_CASES, ids=repr)
def test_decoder_exact_sums(capi, pin, case):
    ask_plan(capi, case)
    d = X.exact_reference(case.id)
    k = Dec(capi, case, d["P"], d["x"])
    eval_logit = d["logit"] if not case.p else X.f32(hd.forward64(d["P"], d["x"])["z"])       # (eval: no dropout)
    for arr in (hd.ARR_ONE, hd.ARR_FIVE):
        pin(arr)
        assert capi.decoder_plan(case.n, case.H)["arrangement"] == arr
        assert_bits(k.eval(), eval_logit, "%s arrangement %d: eval logit" % (case.id, arr))
        for run in (1, 2):
            logit, h1, h2 = k.forward()
            for name, g, w in (("logit", logit, d["logit"]), ("h1", h1, d["h1"]), ("h2", h2, d["h2"])):
                assert_bits(g, w, "%s arrangement %d run %d: %s" % (case.id, arr, run, name))
    pin(0)
    for run in (1, 2):
        got = k.backward(d["h1"], d["h2"], d["dz"])
        for name, g, w in zip(X.DEC_OUT, got, d["out"]):
            assert_bits(g, w, "%s run %d: %s" % (case.id, run, name))


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _left_out(n):
    """the calls with outputs left out: each alone, the input gradient with the weight gradient, all parameter gradients"""
    alone = [tuple(j != i for j in range(n)) for i in range(n)]
    return alone + [tuple(j > 1 for j in range(n)), (True,) + (False,) * (n - 1)]


@pytest.mark.parametrize("case", X.OPTIONAL_CASES, ids=repr)
def test_outputs_left_out_and_a_larger_workspace(capi, case):
    """an output that is NULL is skipped and what is written keeps the bits of the full call -- without d_fc1_w no product is
    launched and the split is 1 --; a workspace planned for a larger batch moves the offsets, not the bits"""
    d = X.exact_reference(case.id)
    if case.kind == "score":
        k = Score(capi, case, d["emb"], d["wts"])
        run = lambda **kw: k.backward(d["prob"], d["hid"], d["dprob"], **kw)
        names, larger = X.SCORE_OUT, dict(ws_max_B=3 * case.n + 5)
    else:
        k = Dec(capi, case, d["P"], d["x"])
        run = lambda **kw: k.backward(d["h1"], d["h2"], d["dz"], **kw)
        names, larger = X.DEC_OUT, dict(ws_max_N=3 * case.n + 5)
    n = len(names)
    for want in _left_out(n):
        got = run(want=want)
        assert [g is not None for g in got] == list(want)
        for name, g, w in zip(names, got, d["out"]):
            if g is not None:
                assert_bits(g, w, "%s with %s asked for: %s" % (case.id, [nm for nm, a in zip(names, want) if a], name))
    for name, g, w in zip(names, run(**larger), d["out"]):
        assert_bits(g, w, "%s in a larger workspace: %s" % (case.id, name))


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.RANDOM_CASES, ids=repr)
def test_random_inputs_within_the_derived_bound(capi, case):
    """every element of the forward's kept rows and of every gradient within L 2^-24 A + one float32 ulp of the float64
    reference, at the case's margin seed; the backward runs on the PLANTED float32 rows of the float64 forward"""
    d = X.random_reference(case.id)
    if case.kind == "score":
        k = Score(capi, case, d["emb"], d["wts"])
        prob, hid = k.forward()
        shares = dict(prob=prob_share(prob, d["s64"]), hid=X.share_of_bound(hid, d["fwd64"]["hid"], d["fwd_bound"]["hid"]))
        assert np.array_equal(hid > 0, d["hid"] > 0), "the kernel's ReLU mask is not the float64 one"
        got, names = k.backward(d["prob"], d["hid"], d["dprob"]), X.SCORE_OUT
    else:
        k = Dec(capi, case, d["P"], d["x"])
        fwd = dict(zip(("logit", "h1", "h2"), k.forward()))
        shares = {name: X.share_of_bound(fwd[name], d["fwd64"][name], d["fwd_bound"][name]) for name in ("h1", "h2", "logit")}
        assert np.array_equal(fwd["h1"] > 0, d["h1"] > 0) and np.array_equal(fwd["h2"] > 0, d["h2"] > 0)
        got, names = k.backward(d["h1"], d["h2"], d["dz"]), X.DEC_OUT
    shares.update({name: X.share_of_bound(g, r, b) for name, g, r, b in zip(names, got, d["out64"], d["bound"])})
    print("%s seed %d: share of the bound used: %s" % (case.id, X.margin_seed(case), ", ".join("%s %.3f" % kv for kv in shares.items())))
    assert max(shares.values()) <= 1.0, shares
