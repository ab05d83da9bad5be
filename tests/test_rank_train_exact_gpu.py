"""The ranking step's scorer (csrc/rank_train.hip) and its listwise loss (k_rank_loss_fwd, csrc/train_tail.hip) held to exact
results on the device (tests/helpers_rank_exact.py; tests/test_rank_train_exact_cpu.py proves the cases' premises):
  A  small-integer inputs at every seam of the tiling: the logits and all six gradients have the bits of the float64
     composition rounded once -- no tolerance --, twice per call;
  B  the C-ABI called directly on such inputs: inputs inside NaN-filled allocations (head and tail), the parameters in one
     flat NaN-filled buffer, every output in front of a sentinel, a workspace of exactly the asked size filled with 0xA5 and
     guarded, every gradient output NULL in turn, and the backward's status word for a transpose corrupted IN BOUNDS;
  C  random inputs at the same seams, held elementwise to L 2^-24 A + ulp (the helper derives L);
  D  the loss at logits 0 / -inf, where its counts decide every bit of dl.
Figures measured on an MI355X: DESIGN.md, "The scorer of a ranking step, held to exact sums"."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import helpers_rank_exact as X
from helpers_rank_train import NEG_INF

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
NAN = float("nan")
GRADS = X.OUTPUTS[1:]


@pytest.fixture(scope="module", autouse=True)
def total_time():
    t = time.time()
    yield
    print("\ntests/test_rank_train_exact_gpu.py: %.1f s in all" % (time.time() - t))


def _hip(emb_q, emb_c, ix, dl, wts):
    """the seven outputs through modules._HipRankScore"""
    from zebra_amd.modules import _HipRankScore
    eq, ec = emb_q.cuda().requires_grad_(True), emb_c.cuda().requires_grad_(True)
    ps = [torch.from_numpy(w).cuda().requires_grad_(True) for w in wts]
    lg = _HipRankScore.apply(eq, ec, None if ix is None else ix.cuda(), *ps)
    lg.backward(dl.cuda())
    return [lg.detach(), eq.grad, ec.grad] + [p.grad for p in ps]


def _assert_bits(got, ref, what):
    for name, g, r in zip(X.OUTPUTS, got, ref):
        if g is None:
            continue
        if not X.bits_equal(g, r):
            g, r = g.detach().cpu().reshape(-1), r.reshape(-1)
            bad = torch.nonzero(~((g == r) | (torch.isnan(g) & torch.isnan(r)))).reshape(-1)
            raise AssertionError("%s: %s differs from the exact sums at %d of %d elements, first at flat index %d: %g, exact %g"
                                 % (what, name, bad.numel(), g.numel(), int(bad[0]), float(g[bad[0]]), float(r[bad[0]])))


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_exact_sums(case):
    """every output has the bits of the float64 composition rounded once; a second call has them too"""
    emb_q, emb_c, ix, dl, wts = case.exact()
    ref, _ = X.exact_reference(case.id)
    for run in (1, 2):
        _assert_bits(_hip(emb_q, emb_c, ix, dl, wts), ref, "%s run %d" % (case.id, run))
    if case.id == "absent-all":
        got = _hip(emb_q, emb_c, ix, dl, wts)
        assert bool((got[0] == NEG_INF).all()) and all(float(g.abs().max()) == 0.0 for g in got[1:])
    if case.dl_nan:
        assert bool((ix < 0).any())
        poisoned = torch.where(ix < 0, torch.full_like(dl, NAN), dl)
        zeroed = torch.where(ix < 0, torch.zeros_like(dl), dl)
        a, b = _hip(emb_q, emb_c, ix, poisoned, wts), _hip(emb_q, emb_c, ix, zeroed, wts)
        _assert_bits(a, ref, case.id + " NaN in dl at the absent pairs")
        _assert_bits(b, ref, case.id + " 0 in dl at the absent pairs")


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _place(t, head, fill=NAN):
    """a CPU tensor as a 16-byte-aligned view inside a larger allocation filled with ``fill``: its head or its tail"""
    n = t.numel()
    o = 0 if head else 64
    buf = torch.full((n + 64,), fill, dtype=t.dtype, device="cuda")
    buf[o:o + n] = t.reshape(-1).cuda()
    v = buf[o:o + n].view(t.shape)
    assert v.data_ptr() % 16 == 0
    return buf, v


class _Out:
    """an output of ``shape`` in front of a sentinel (and, as the tail, behind 64 NaN)"""

    def __init__(self, shape, head=True):
        self.n, self.o = int(np.prod(shape)), 0 if head else 64
        self.buf = torch.full((self.o + self.n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        self.buf[:self.o] = NAN
        self.view = self.buf[self.o:self.o + self.n].view(shape)
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.buf[self.o + self.n:] == SENTINEL).all()) and bool(torch.isnan(self.buf[:self.o]).all())


def _flat_params(wts):
    """the four parameters as views into ONE flat NaN-filled buffer: fc1.weight, fc1.bias and fc2.weight 16-byte aligned with
    four NaN between them, fc2.bias one float further, at an odd offset"""
    H = wts[1].size
    gaps = (4, 4, 4, 1)
    buf = torch.full((sum(gaps) + sum(w.size for w in wts) + 7,), NAN, dtype=torch.float32, device="cuda")
    views, o = [], 0
    for w, gap in zip(wts, gaps):
        o += gap
        buf[o:o + w.size] = torch.from_numpy(np.ascontiguousarray(w).reshape(-1)).cuda()
        views.append(buf[o:o + w.size].view(w.shape))
        o += w.size
    assert all(v.data_ptr() % 16 == 0 for v in views[:3]) and (views[3].data_ptr() // 4) % 2 == 1 and H % 4 == 0
    return buf, views


class _Abi:
    """one case's inputs on the device and the two entry points called on them"""

    def __init__(self, case, head):
        from zebra_amd import _capi
        self.capi, self.lib, self.case, self.head = _capi, _capi.lib(), case, head
        emb_q, emb_c, ix, dl, wts = case.exact()
        self.keep = [_place(emb_q, head), _place(emb_c, head), _place(dl, head)]
        self.emb_q, self.emb_c, self.dl = (v for _, v in self.keep)
        self.ix = None if ix is None else ix.cuda()
        self.pbuf, self.params = _flat_params(wts)
        self.wt = _capi.AffinityWeights(*[_capi.ptr(v) for v in self.params])
        Q, C_, H, Nc = case.Q, case.C, case.H, case.Nc
        self.dims = (C.c_int64(Q), C.c_int64(Nc), C.c_int64(C_), C.c_int32(H))
        self.need = int(self.lib.zt_affinity_rank_train_workspace_bytes(*self.dims))
        assert self.need > 0
        self.shapes = [(Q, H), (Nc, H), (H, 2 * H), (H,), (1, H), (1,)]
        if ix is not None:
            from zebra_amd.modules import rank_transpose
            self.row_ptr, self.pairs = rank_transpose(ix, Nc)                 # (on the CPU: corrupt() edits it there)
        else:
            self.row_ptr = self.pairs = None

    def workspace(self):
        return torch.full((self.need + 64,), 0xA5, dtype=torch.uint8, device="cuda")

    def forward(self):
        case, ptr = self.case, self.capi.ptr
        self.logit, self.pq, self.pc = _Out((case.Q, case.C)), _Out((case.Q, case.H), self.head), _Out((case.Nc, case.H), self.head)
        ws = self.workspace()
        self.capi.check(self.lib.zt_affinity_rank_train_forward(
            ptr(self.emb_q), C.c_int64(case.Q), ptr(self.emb_c), C.c_int64(case.Nc), ptr(self.ix), C.c_int64(case.C), C.c_int32(case.H),
            C.byref(self.wt), ptr(self.logit.view), ptr(self.pq.view), ptr(self.pc.view), ptr(ws), self.capi.stream_ptr()),
            "zt_affinity_rank_train_forward")
        torch.cuda.synchronize()
        assert self.logit.intact() and self.pq.intact() and self.pc.intact(), "the forward wrote outside an output"
        assert bool((ws[self.need:] == 0xA5).all()) and int(ws[:4].view(torch.int32).item()) == 0
        return self.logit.view

    def backward(self, want=(True,) * 6, transpose=None):
        """([six gradients or None], status word) of one call; every output asked for sits in front of a sentinel"""
        case, ptr = self.case, self.capi.ptr
        outs = [_Out(s) if w else None for s, w in zip(self.shapes, want)]
        ws = self.workspace()
        row_ptr, pairs = transpose or (self.row_ptr, self.pairs)
        n_pairs = 0 if pairs is None else int(pairs.numel())
        rp = None if row_ptr is None else row_ptr.cuda()
        pr = pairs.cuda() if n_pairs else None
        self.capi.check(self.lib.zt_affinity_rank_train_backward(
            ptr(self.emb_q), C.c_int64(case.Q), ptr(self.emb_c), C.c_int64(case.Nc), ptr(self.ix), C.c_int64(case.C), C.c_int32(case.H),
            C.byref(self.wt), ptr(self.pq.view), ptr(self.pc.view), ptr(self.dl), ptr(rp), ptr(pr), C.c_int64(n_pairs),
            *[None if o is None else ptr(o.view) for o in outs], ptr(ws), self.capi.stream_ptr()), "zt_affinity_rank_train_backward")
        torch.cuda.synchronize()
        for name, o in zip(GRADS, outs):
            assert o is None or o.intact(), "the backward wrote outside %s" % name
        assert bool((ws[self.need:] == 0xA5).all()), "the workspace was overrun"
        assert self.pq.intact() and self.pc.intact()
        return [None if o is None else o.view for o in outs], int(ws[:4].view(torch.int32).item())


@pytest.mark.parametrize("case", X.ABI_CASES, ids=repr)
def test_c_abi_with_nothing_to_hide_behind(case):
    ref, _ = X.exact_reference(case.id)
    runs = {}
    for head in (True, False):
        abi = _Abi(case, head)
        logit = abi.forward()
        grads, status = abi.backward()
        assert status == 0
        runs[head] = [logit] + grads
        _assert_bits(runs[head], ref, "%s %s" % (case.id, "head" if head else "tail"))
    for name, a, b in zip(X.OUTPUTS, runs[True], runs[False]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "head and tail differ in %s" % name
    full = runs[False]
    for i, name in enumerate(GRADS):                                   # `abi` is the tail placement
        only, status = abi.backward(want=tuple(j == i for j in range(6)))
        assert status == 0 and [g is not None for g in only] == [j == i for j in range(6)]
        assert torch.equal(only[i].view(torch.int32), full[1 + i].view(torch.int32)), "%s alone" % name
        rest, status = abi.backward(want=tuple(j != i for j in range(6)))
        assert status == 0 and rest[i] is None
        for j, g in enumerate(rest):
            assert g is None or torch.equal(g.view(torch.int32), full[1 + j].view(torch.int32)), "%s without %s" % (GRADS[j], name)


def _corrupt(abi, kind):
    """(row_ptr, pairs, rows the corruption touches): the correct transpose with one defect, every id inside [0, Q C) and
    row_ptr unchanged -- nothing can be read out of bounds"""
    case = abi.case
    row_ptr, pairs = abi.row_ptr.clone(), abi.pairs.clone()
    flat = abi.ix.cpu().reshape(-1)
    rows = [r for r in range(case.Nc) if int(row_ptr[r + 1] - row_ptr[r]) >= 2]
    r1, r2 = rows[0], rows[-1]
    assert r1 != r2
    i, j = int(row_ptr[r1]) + 1, int(row_ptr[r2])
    if kind == "swapped":
        pairs[i], pairs[j] = pairs[j].clone(), pairs[i].clone()
        touched = [r1, r2]
    elif kind == "absent":
        gone = torch.nonzero(flat == -1).reshape(-1)
        pairs[i] = int(gone[len(gone) // 2])
        touched = [r1]
    else:                                                              # "twice": legal by the kernel's check, the caller's error
        pairs[i] = pairs[i - 1]
        touched = [r1]
    assert int(pairs.min()) >= 0 and int(pairs.max()) < case.Q * case.C and torch.equal(row_ptr, abi.row_ptr)
    return row_ptr, pairs, touched


@pytest.mark.parametrize("case", [c for c in X.ABI_CASES if c.indexed], ids=repr)
def test_backward_status_word(case):
    """a pair listed under the wrong row, or an absent pair listed at all: ZT_ERR_RANGE in the status word, the pair left out,
    and d_emb_c of every row the corruption does not touch keeps the bits of the correct call.  A pair listed twice under its
    own row passes the kernel's check (the header calls it the caller's error): the call returns and writes inside its
    outputs, no more is asked."""
    abi = _Abi(case, True)
    abi.forward()
    good, status = abi.backward()
    assert status == 0
    for kind in ("swapped", "absent"):
        row_ptr, pairs, touched = _corrupt(abi, kind)
        got, status = abi.backward(transpose=(row_ptr, pairs))
        assert status == abi.capi.ZT_ERR_RANGE, kind
        keep = [r for r in range(case.Nc) if r not in touched]
        assert torch.equal(got[1][keep].view(torch.int32), good[1][keep].view(torch.int32)), kind
        assert any(not torch.equal(got[1][r], good[1][r]) for r in touched), kind      # (the pair IS left out)
        again, status = abi.backward(want=(False, True, False, False, False, False), transpose=(row_ptr, pairs))
        assert status == abi.capi.ZT_ERR_RANGE and torch.equal(again[1].view(torch.int32), got[1].view(torch.int32))
    row_ptr, pairs, _ = _corrupt(abi, "twice")
    abi.backward(transpose=(row_ptr, pairs))


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.RANDOM_CASES, ids=repr)
def test_random_inputs_within_the_derived_bound(case):
    """logits, d_emb_q and d_emb_c elementwise within L 2^-24 A + one float32 ulp of the float64 reference, at the case's
    margin seed; the parameter gradients within 1e-5 + 1e-4 max|ref| (the exact cases are what hold them)"""
    args, ref, bound = X.random_reference(case.id)
    got = _hip(*args)
    shares = [X.share_of_bound(g, r, b) for g, r, b in zip(got[:3], ref[:3], bound)]
    print("%s seed %d: share of the bound used: logit %.3f d_emb_q %.3f d_emb_c %.3f" % ((case.id, X.margin_seed(case)) + tuple(shares)))
    assert max(shares) <= 1.0, shares
    for name, g, r in zip(X.OUTPUTS[3:], got[3:], ref[3:]):
        err, mx = float((g.double().cpu() - r).abs().max()), float(r.abs().max())
        assert err <= 1e-5 + 1e-4 * mx, "%s: %g (max |ref| %g)" % (name, err, mx)


# ---- D ---------------------------------------------------------------------------------------------------------------------
def _loss_case(Q, C_, with_target):
    """(logits [Q, C] of 0 and -inf, target or None): 30 % of the pairs absent, every target present but that of one query in
    the last wave's share (query 15, or the last one where Q < 16), and query 1 with its target as its only present column"""
    g = torch.Generator().manual_seed(1000 * Q + C_ + (7 if with_target else 0))
    t = torch.randint(0, C_, (Q,), generator=g) if with_target else torch.zeros(Q, dtype=torch.long)
    present = torch.rand((Q, C_), generator=g) >= 0.3
    present[torch.arange(Q), t] = True
    skip = 15 if Q > 15 else Q - 1
    present[skip, t[skip]] = False
    present[1] = False
    present[1, t[1]] = True
    lg = torch.where(present, torch.zeros((Q, C_)), torch.full((Q, C_), NEG_INF))
    return lg, (t.to(torch.int32) if with_target else None), t, present, skip


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


@pytest.mark.parametrize("mode", ["softmax", "bce"])
@pytest.mark.parametrize("with_target", [False, True], ids=["column0", "target"])
@pytest.mark.parametrize("C_", [63, 64, 65, 129])
@pytest.mark.parametrize("Q", [15, 16, 17, 33])
def test_loss_counts_decide_every_bit(Q, C_, with_target, mode):
    """Every present logit 0: sigma = 1/2 and softmax = 1 / n_q, so dl is a quotient of the kernel's COUNTS -- n_live, n_neg and
    the present columns n_q of a query -- formed in float64 and rounded once, as the host forms it here: the bits must agree.
    The bce loss is float32(2 ln 2) in every bit; the softmax loss, a mean of logarithms added in the kernel's own order, is
    held to one float32 ulp for that reason."""
    from zebra_amd.losses import listwise_loss, rank_loss_plan
    lg, target, t, present, skip = _loss_case(Q, C_, with_target)
    x = lg.cuda().requires_grad_(True)
    td = None if target is None else target.cuda()
    assert rank_loss_plan(x, td) == "hip"
    loss = listwise_loss(x, td, mode)
    loss.backward()
    live = present[torch.arange(Q), t].numpy()
    P = present.numpy()
    n_live = int(live.sum())
    assert n_live == Q - 1 and not live[skip]
    onehot = np.zeros((Q, C_), bool)
    onehot[np.arange(Q), t.numpy()] = True
    n_q = P.sum(1)
    assert n_q[1] == 1
    want = np.zeros((Q, C_), np.float64)
    if mode == "bce":
        neg = P & ~onehot & live[:, None]
        n_neg = int(neg.sum())
        want[neg] = 0.5 / n_neg
        want[onehot & live[:, None]] = -0.5 / n_live
        want_loss = 2 * math.log(2.0)
    else:
        rows = live[:, None] & P
        want = np.where(rows, (1.0 / np.maximum(n_q, 1)[:, None] - onehot) / n_live, 0.0)
        want_loss = float(np.log(n_q[live].astype(np.float64)).mean())
    got = x.grad.cpu().numpy()
    assert np.array_equal((got + np.float32(0)).view(np.uint32), (_f32(want) + np.float32(0)).view(np.uint32)), \
        "dl differs at %d pairs" % int((got != _f32(want)).sum())
    assert float(np.abs(got[skip]).max()) == 0.0 and float(np.abs(got[~P]).max()) == 0.0
    got_loss = np.float32(loss.detach().cpu().numpy())
    if mode == "bce":
        assert got_loss == _f32(want_loss), (float(got_loss), want_loss)
    else:
        assert abs(float(got_loss) - float(_f32(want_loss))) <= float(np.spacing(_f32(want_loss))), (float(got_loss), want_loss)


def test_bce_loss_without_a_negative_is_ln_2():
    """every query's only present column is its target: n_neg = 0, the loss is float32(ln 2) and dl = -1 / (2 n_live)"""
    from zebra_amd.losses import listwise_loss
    Q, C_ = 17, 65
    lg = torch.full((Q, C_), NEG_INF)
    lg[:, 0] = 0.0
    x = lg.cuda().requires_grad_(True)
    loss = listwise_loss(x, None, "bce")
    loss.backward()
    assert np.float32(loss.detach().cpu().numpy()) == _f32(math.log(2.0))
    want = np.zeros((Q, C_))
    want[:, 0] = -0.5 / Q
    assert np.array_equal(x.grad.cpu().numpy(), _f32(want))
