"""The tail of a training step on the device (csrc/train_tail.hip): the pair loss (zt_link_bce_forward / _backward through
losses._HipLinkBCE, losses.link_bce_loss and TGN.compute_edge_loss) and the one-launch Adam step (zt_adam_step through
zebra_amd.Adam), each against torch's float64 composition on the CPU.

No tolerance here is taken from the code under test.  For every compared value the bound is
    2 x (the error of torch's own float32 result on the CPU against the float64 result) + one float32 ulp of the float64 value
on the same inputs: the operations are the same, only contraction and the order of a sum may differ (factor two), and the
kernel's result has to be written down as a float32 (the ulp, elementwise).  For the loss and its gradient torch's error is
taken element by element.  For Adam it is the largest error in the tensor compared: where an update cancels (m + 0.1 (g - m)
near zero, a parameter about as large as its step) every float32 implementation is off by a rounding of the LARGER operand,
which one lands nearer is chance, and an element-by-element bound refuses a result for being unlucky where torch was lucky
-- a numpy float32 restatement of the formulas misses it at about one element in 2000, fused or not, closer to float64 than
torch or not.  Measured on the CPU for the shapes below, that restatement stays within 0.55 of the per-tensor bound."""
import copy
import functools

import numpy as np
import pytest
import torch

import inputs as I
from conftest import golden
from helpers import build_tgn

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bound(t32, t64):
    """the module docstring's bound, elementwise (float64 arrays)"""
    t32, t64 = np.asarray(t32, np.float64), np.asarray(t64, np.float64)
    return 2.0 * np.abs(t32 - t64) + np.spacing(np.abs(t64).astype(np.float32)).astype(np.float64)


def _bound_tensor(t32, t64):
    """... with torch-float32's LARGEST error in the tensor (the module docstring: Adam)"""
    t32, t64 = np.asarray(t32, np.float64), np.asarray(t64, np.float64)
    worst = np.abs(t32 - t64).max() if t64.size else 0.0
    return 2.0 * worst + np.spacing(np.abs(t64).astype(np.float32)).astype(np.float64)


def _assert_within(got, t32, t64, what, bound=_bound):
    got, t64 = np.asarray(got, np.float64), np.asarray(t64, np.float64)
    err, tol = np.abs(got - t64), bound(t32, t64)
    worst = int(np.argmax(err / tol))
    print("%s: max err %.3e (torch-float32's: %.3e), largest err / bound %.3f" %
          (what, err.max(), np.abs(np.asarray(t32, np.float64) - t64).max(), (err / tol).max()))
    assert np.all(err <= tol), "%s: error %g against a bound of %g at element %d" % (what, err.ravel()[worst], tol.ravel()[worst], worst)


# ---------------------------------------------------------------------------------------------------------
# the pair loss
# ---------------------------------------------------------------------------------------------------------
LOSS_B = [1, 2, 63, 64, 65, 200, 257, 4097]
PLANTED = [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24]         # the -100 clamp of the logarithm, the 1e-12 floor of the gradient's divisor


def _torch_loss(prob, B):
    """BCELoss(pos, 1) + BCELoss(neg, 0) and its gradient, in prob's precision on the CPU"""
    prob = prob.clone().requires_grad_(True)
    crit = torch.nn.BCELoss()
    loss = crit(prob[:B], torch.ones(B, dtype=prob.dtype)) + crit(prob[B:], torch.zeros(B, dtype=prob.dtype))
    loss.backward()
    return loss.detach().numpy(), prob.grad.numpy()


@functools.lru_cache(maxsize=None)
def _loss_case(B):
    """prob [2B] float32 and (loss, gradient) of torch's float32 and float64 compositions on it; computed once, shared"""
    g = torch.Generator().manual_seed(4000 + B)
    prob = torch.rand(2 * B, generator=g)
    if B >= 3:
        for side in (0, 1):
            at = torch.randperm(B, generator=g)[:len(PLANTED)] + side * B
            prob[at] = torch.tensor(PLANTED, dtype=torch.float32)
    return prob, _torch_loss(prob, B), _torch_loss(prob.double(), B)


def _hip_loss(prob, scale=None):
    from zebra_amd.losses import _HipLinkBCE
    p = prob.to(DEV).requires_grad_(True)
    loss = _HipLinkBCE.apply(p)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("B", LOSS_B)
def test_link_bce_matches_float64(B):
    prob, (l32, g32), (l64, g64) = _loss_case(B)
    if B >= 3:
        assert all((prob[s * B:(s + 1) * B] == np.float32(v)).sum() >= 1 for s in (0, 1) for v in PLANTED)
    loss, grad = _hip_loss(prob)
    assert loss.shape == () and loss.dtype == torch.float32 and grad.shape == (2 * B,)
    _assert_within(loss.cpu().numpy(), l32, l64, "loss, B=%d" % B)
    _assert_within(grad.cpu().numpy(), g32, g64, "d_prob, B=%d" % B)


@pytest.mark.parametrize("B", LOSS_B)
def test_link_bce_twice_gives_the_same_bits_and_scales_its_gradient(B):
    prob = _loss_case(B)[0]
    l1, g1 = _hip_loss(prob)
    l2, g2 = _hip_loss(prob)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    # (0.37 loss).backward(): the backward kernel multiplies by the incoming gradient, one rounding per element
    l3, g3 = _hip_loss(prob, 0.37)
    assert torch.equal(l3, l1)
    assert torch.equal(g3, torch.tensor(0.37, dtype=torch.float32, device=DEV) * g1)


@pytest.mark.parametrize("B", [1, 65, 200])
def test_link_bce_loss_takes_columns_and_is_the_op(B):
    import zebra_amd
    prob = _loss_case(B)[0]
    want_l, want_g = _hip_loss(prob)
    for shape in ((B, 1), (B,)):
        pos = prob[:B].reshape(shape).to(DEV).requires_grad_(True)
        neg = prob[B:].reshape(shape).to(DEV).requires_grad_(True)
        loss = zebra_amd.link_bce_loss(pos, neg)
        loss.backward()
        assert torch.equal(loss, want_l)
        assert pos.grad.shape == shape and torch.equal(torch.cat([pos.grad.reshape(-1), neg.grad.reshape(-1)]), want_g)


# ---------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------
SENTINEL = -7777.25
LR = 1e-3


def _carve(shapes, odd_at, seed):
    """Parameters as views into ONE float32 buffer filled with a sentinel: each starts on a 16-byte boundary behind a gap of
    at least four floats -- the one at index odd_at one float further --, so a write outside a tensor lands in a gap.
    Returns (buffer, [parameter], boolean mask of the gaps, [initial values on the CPU])."""
    g = torch.Generator().manual_seed(seed)
    offs, o = [], 4
    for i, s in enumerate(shapes):
        o = (o + 3) // 4 * 4 + (1 if i == odd_at else 0)
        offs.append(o)
        o += int(np.prod(s)) + 4
    buf = torch.full((o + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    gap = torch.ones(o + 4, dtype=torch.bool)
    params, init = [], []
    for s, off in zip(shapes, offs):
        n = int(np.prod(s))
        v = torch.randn(n, generator=g) * 3.0
        buf[off:off + n] = v.to(DEV)
        gap[off:off + n] = False
        p = buf[off:off + n].view(s).requires_grad_(True)
        assert p.is_contiguous() and p.data_ptr() % 16 == (4 if offs.index(off) == odd_at else 0)
        params.append(p)
        init.append(v.view(s).clone())
    return buf, params, gap.to(DEV), init


def _grads(shapes, step, seed, none_at=None):
    """gradients of magnitudes 1e-6 .. 1 with exact zeros; None for the parameter none_at"""
    g = torch.Generator().manual_seed(seed + 17 * step)
    out = []
    for i, s in enumerate(shapes):
        gr = torch.randn(s, generator=g) * 10.0 ** (-6.0 * torch.rand(s, generator=g))
        gr[torch.rand(s, generator=g) < 0.1] = 0.0
        out.append(None if i == none_at else gr)
    return out


def _set_grads(params, grads, dtype=None, device=None):
    for p, gr in zip(params, grads):
        p.grad = None if gr is None else gr.to(device=device or p.device, dtype=dtype or p.dtype).clone()


def _cpu_refs(init):
    """torch.optim.Adam on float64 and (foreach=False) float32 copies on the CPU"""
    out = []
    for dt in (torch.float32, torch.float64):
        ps = [torch.nn.Parameter(v.to(dt).clone()) for v in init]
        out.append((ps, torch.optim.Adam(ps, lr=LR, foreach=False)))
    return out


def _check_against_refs(tag, params, opt, refs):
    (p32, o32), (p64, o64) = refs
    for i, (p, a, b) in enumerate(zip(params, p32, p64)):
        _assert_within(p.detach().cpu().numpy(), a.detach().numpy(), b.detach().numpy(), "%s param %d" % (tag, i), _bound_tensor)
        if p in opt.state and len(opt.state[p]):
            assert float(opt.state[p]["step"]) == float(o64.state[b]["step"]), (tag, i)
            assert opt.state[p]["step"].device.type == "cpu" and opt.state[p]["step"].dtype == torch.float32
            for k in ("exp_avg", "exp_avg_sq"):
                _assert_within(opt.state[p][k].cpu().numpy(), o32.state[a][k].numpy(), o64.state[b][k].numpy(), "%s %s %d" % (tag, k, i),
                               _bound_tensor)
        else:
            assert b not in o64.state or not len(o64.state[b])


def _adam_shapes():
    from zebra_amd import _capi
    ch = _capi.ADAM_CHUNK
    # index 4 (1023 elements) sits one float off a 16-byte boundary
    return [(1,), (3,), (4,), (5,), (1023,), (1025,), (ch - 1,), (ch,), (ch + 1,), (2 * ch + 3,), (100, 372)], 4


def test_adam_three_steps_match_float64(adam_calls):
    import zebra_amd
    from zebra_amd import _capi
    shapes, odd = _adam_shapes()
    buf, params, gap, init = _carve(shapes, odd, 11)
    opt = zebra_amd.Adam(params, lr=LR)
    refs = _cpu_refs(init)
    skipped = 5                                              # has no gradient in the second step
    for step in range(3):
        grads = _grads(shapes, step, 23, skipped if step == 1 else None)
        before = params[skipped].detach().clone()
        versions = [p._version for p in params]
        _set_grads(params, grads)
        for ps, o in refs:
            _set_grads(ps, grads)
            o.step()
        opt.step()
        assert torch.all(buf[gap] == SENTINEL), "a write outside a tensor in step %d" % step
        # an in-place update as far as autograd is concerned (the model keys its packed weights on a parameter's _version)
        # (the views of one buffer share its counter: only "every stepped parameter moved on" can be said here)
        assert all(p._version > v for p, v, gr in zip(params, versions, grads) if gr is not None)
        if step == 1:
            assert torch.equal(params[skipped].detach(), before) and float(opt.state[params[skipped]]["step"]) == 1.0
        _check_against_refs("step %d" % step, params, opt, refs)
    assert float(opt.state[params[skipped]]["step"]) == 2.0 and float(opt.state[params[0]]["step"]) == 3.0
    assert adam_calls[0] == 3 and len(_capi.adam_plan([int(np.prod(s)) for s in shapes])) == 1


def test_adam_one_tensor_more_than_a_launch_holds(adam_calls):
    import zebra_amd
    from zebra_amd import _capi
    n = _capi.ADAM_MAX_TENSORS + 1
    shapes = [(1 + (7 * i) % 70,) for i in range(n)]
    assert len(_capi.adam_plan([s[0] for s in shapes])) == 2
    buf, params, gap, init = _carve(shapes, 3, 12)
    opt = zebra_amd.Adam(params, lr=LR)
    refs = _cpu_refs(init)
    for step in range(2):
        grads = _grads(shapes, step, 29)
        _set_grads(params, grads)
        for ps, o in refs:
            _set_grads(ps, grads)
            o.step()
        opt.step()
        assert torch.all(buf[gap] == SENTINEL), "a write outside a tensor in step %d" % step
        _check_against_refs("step %d" % step, params, opt, refs)
    assert adam_calls[0] == 2                                # one call per step, two launches inside it


@pytest.mark.parametrize("first", ["zebra", "torch"])
def test_adam_state_dict_interchange(first):
    """three steps with one optimizer, its state_dict into the other over clones of the parameters, one more step with each
    on the same gradients: the two agree within the bound of the fourth step"""
    import zebra_amd
    shapes = [(5,), (1023,), (100, 372), (4097,)]
    kinds = {"zebra": zebra_amd.Adam, "torch": torch.optim.Adam}
    other = "torch" if first == "zebra" else "zebra"
    g = torch.Generator().manual_seed(31)
    init = [torch.randn(s, generator=g) * 3.0 for s in shapes]
    pa = [torch.nn.Parameter(v.clone().to(DEV)) for v in init]
    oa = kinds[first](pa, lr=LR)
    refs = _cpu_refs(init)
    for step in range(4):
        grads = _grads(shapes, step, 37)
        if step == 3:
            pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
            ob = kinds[other](pb, lr=LR)
            ob.load_state_dict(copy.deepcopy(oa.state_dict()))
            _set_grads(pb, grads)
            ob.step()
        _set_grads(pa, grads)
        oa.step()
        for ps, o in refs:
            _set_grads(ps, grads)
            o.step()
    (p32, o32), (p64, o64) = refs
    for i, (x, y) in enumerate(zip(pa, pb)):
        sx, sy = oa.state[x], ob.state[y]
        assert float(sx["step"]) == float(sy["step"]) == 4.0
        assert sy["step"].device.type == "cpu" and sy["step"].dtype == torch.float32
        for what, a, b, r32, r64 in [("param", x.detach(), y.detach(), p32[i].detach(), p64[i].detach())] + \
                [(k, sx[k], sy[k], o32.state[p32[i]][k], o64.state[p64[i]][k]) for k in ("exp_avg", "exp_avg_sq")]:
            tol = _bound_tensor(r32.numpy(), r64.numpy())
            err = np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64))
            print("%s -> %s, %s %d: max difference %.3e, smallest bound %.3e" % (first, other, what, i, err.max(), tol.min()))
            assert np.all(err <= tol), (what, i, float(err.max()))


# ---------------------------------------------------------------------------------------------------------
# through the model
# ---------------------------------------------------------------------------------------------------------
def _counted(monkeypatch, name):
    from zebra_amd import _capi
    lib = _capi.lib()
    calls, fn = [0], getattr(lib, name)

    def counted(*args):
        calls[0] += 1
        return fn(*args)

    monkeypatch.setattr(lib, name, counted)
    return calls


@pytest.fixture
def adam_calls(monkeypatch):
    """[n]: calls of lib().zt_adam_step from here on"""
    return _counted(monkeypatch, "zt_adam_step")


@pytest.fixture
def bce_calls(monkeypatch):
    """[n]: calls of lib().zt_link_bce_forward from here on"""
    return _counted(monkeypatch, "zt_link_bce_forward")


def test_training_step_with_the_hip_tail_matches_reference(bce_calls, adam_calls):
    """The loop of test_fused_scorer_training_step_matches_reference (g8_train_grads, d20_f7) with TGN.compute_edge_loss in
    place of the two BCELoss lines: the reference's loss within 1e-5, every parameter gradient within 1e-5 + 1e-4 max|ref|;
    then ONE optimizer step on those very gradients by zebra_amd.Adam against torch.optim.Adam on float64 (and float32) clones
    on the CPU, within the Adam bound.  The fixture's losses and gradients are those of the INITIAL weights in every batch, so
    the parameters are put back after each compared step (in the model and in the clones); the optimizers keep their
    moments and step counts, which therefore grow over the batches as in training.  One step on identical gradients is what
    is compared, not two trajectories: an element whose gradient is rounding noise around zero can take +lr in one run and
    -lr in another, which says nothing about the kernel."""
    import zebra_amd
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES["d20_f7"]
    g = golden("g8_train_grads")
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    tgn.train(True)
    names = [pn for pn, _ in tgn.named_parameters()]
    params = [p for _, p in tgn.named_parameters()]
    init = [p.detach().cpu().clone() for p in params]
    opt = zebra_amd.Adam(params, lr=LR)
    refs = _cpu_refs(init)
    seen = 0
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        opt.zero_grad()
        loss, pos, negp = tgn.compute_edge_loss(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10)
        assert loss.shape == () and pos.shape == (bs, 1) and negp.shape == (bs, 1)
        assert not pos.requires_grad and not negp.requires_grad
        loss.backward()
        assert abs(float(loss.item()) - float(g["b%d_loss" % b])) <= 1e-5, "loss of batch %d" % b
        grads = {pn: p.grad for pn, p in zip(names, params) if p.grad is not None}
        for pn in [kk[len("b%d_grad_" % b):] for kk in g.files if kk.startswith("b%d_grad_" % b)]:
            assert pn in grads, pn
            want = g["b%d_grad_%s" % (b, pn)]
            err = np.abs(grads[pn].cpu().numpy() - want).max()
            assert err <= 1e-5 + 1e-4 * np.abs(want).max(), "%s in batch %d: %g" % (pn, b, err)
            seen += 1
        host = [None if p.grad is None else p.grad.detach().cpu() for p in params]
        for ps, o in refs:
            _set_grads(ps, host)
            o.step()
        opt.step()
        assert bce_calls[0] == b + 1 and adam_calls[0] == b + 1
        _check_against_refs("batch %d" % b, params, opt, refs)
        idle = [i for i, gr in enumerate(host) if gr is None]
        assert idle, "the model has modules a step never calls"
        for i in idle:                                       # no gradient: the bits stay, no state appears
            assert torch.equal(params[i].detach().cpu(), init[i]) and params[i] not in opt.state, names[i]
        with torch.no_grad():
            for p, v in zip(params, init):
                p.copy_(v)
            for ps, _ in refs:
                for p, v in zip(ps, init):
                    p.copy_(v)
        tgn.memory.detach_memory()
    assert seen >= 12 * nb
    assert float(opt.state[params[names.index("affinity_score.fc1.weight")]]["step"]) == float(nb)


def test_next_step_sees_the_weights_the_hip_tail_wrote():
    """Four training steps of d20_f7 WITHOUT putting the parameters back, once with torch's loss and torch.optim.Adam and once
    with compute_edge_loss and zebra_amd.Adam (lr 1e-4, train.py:29): the losses agree within 1e-5 in every step -- the model
    keeps packed copies of its weights keyed on the parameters' _version, so a kernel that updates them behind autograd's back
    would train on with the initial weights -- and from the second step on they are NOT the fixture's, whose weights never
    move."""
    import zebra_amd
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES["d20_f7"]
    g = golden("g8_train_grads")
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    crit = torch.nn.BCELoss()
    losses = {}
    for tail in ("torch", "hip"):
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
        tgn.train(True)
        opt = (zebra_amd.Adam if tail == "hip" else torch.optim.Adam)(tgn.parameters(), lr=1e-4)
        losses[tail] = []
        for b in range(nb):
            s, e = b * bs, (b + 1) * bs
            opt.zero_grad()
            if tail == "hip":
                loss, _, _ = tgn.compute_edge_loss(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10)
            else:
                pos, negp = tgn.compute_edge_probabilities(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
                loss = crit(pos.squeeze(), torch.ones(bs, device=DEV)) + crit(negp.squeeze(), torch.zeros(bs, device=DEV))
            loss.backward()
            opt.step()
            tgn.memory.detach_memory()
            losses[tail].append(float(loss.item()))
    print("losses:", losses, "fixture:", [float(g["b%d_loss" % b]) for b in range(nb)])
    for b in range(nb):
        assert abs(losses["hip"][b] - losses["torch"][b]) <= 1e-5, "loss of step %d" % b
    assert abs(losses["hip"][0] - float(g["b0_loss"])) <= 1e-5
    assert max(abs(losses["torch"][b] - float(g["b%d_loss" % b])) for b in range(1, nb)) > 1e-4, "the steps moved nothing"
