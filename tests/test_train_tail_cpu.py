"""The training step's tail without a GPU (csrc/train_tail.hip, zebra_amd/optim.py, zebra_amd/losses.py): the entry points
refuse bad arguments on the host, zt_adam_plan against a numpy restatement, adam_plan's answers, and zebra_amd.Adam on CPU
parameters -- torch's own code path there -- bit for bit against torch.optim.Adam, state_dict interchange included."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def _entry(capi, param=1, grad=1, m=1, v=1, numel=4):
    """a table entry whose pointers are never followed (every case here is refused, or empty, before any device call)"""
    buf = np.zeros(8, np.float32)
    a = buf.ctypes.data
    e = capi.AdamTensor(a if param else None, a if grad else None, a if m else None, a if v else None, numel, 1e-3, 1.0)
    e._keep = buf
    return e


def test_link_bce_refuses_bad_arguments_on_the_host(capi):
    lib = capi.lib()
    x = np.full(8, 0.5, np.float32)
    p = capi.ptr(x)
    for B in (0, -1):
        assert lib.zt_link_bce_forward(p, C.c_int64(B), p, p, None) == capi.ZT_ERR_ARG
        assert lib.zt_link_bce_backward(p, p, C.c_int64(B), p, None) == capi.ZT_ERR_ARG
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        assert lib.zt_link_bce_forward(args[0], C.c_int64(4), args[1], args[2], None) == capi.ZT_ERR_ARG, hole
        assert lib.zt_link_bce_backward(args[0], args[1], C.c_int64(4), args[2], None) == capi.ZT_ERR_ARG, hole
    assert b"zt_link_bce_backward" in lib.zt_last_error()


def test_adam_step_refuses_bad_arguments_on_the_host(capi):
    lib = capi.lib()
    f = C.c_float
    one = (capi.AdamTensor * 1)(_entry(capi))
    assert lib.zt_adam_step(one, C.c_int32(-1), f(0.9), f(0.999), f(1e-8), None) == capi.ZT_ERR_ARG
    assert lib.zt_adam_step(None, C.c_int32(1), f(0.9), f(0.999), f(1e-8), None) == capi.ZT_ERR_ARG
    for hole in ("param", "grad", "m", "v"):
        bad = (capi.AdamTensor * 2)(_entry(capi), _entry(capi, **{hole: 0}))
        assert lib.zt_adam_step(bad, C.c_int32(2), f(0.9), f(0.999), f(1e-8), None) == capi.ZT_ERR_ARG, hole
        assert b"tensor 1" in lib.zt_last_error()
    for numel in (-1, 2 ** 31, 2 ** 40):
        bad = (capi.AdamTensor * 1)(_entry(capi, numel=numel))
        assert lib.zt_adam_step(bad, C.c_int32(1), f(0.9), f(0.999), f(1e-8), None) == capi.ZT_ERR_ARG, numel


def test_adam_step_of_nothing_is_ok(capi):
    lib = capi.lib()
    f = C.c_float
    assert lib.zt_adam_step(None, C.c_int32(0), f(0.9), f(0.999), f(1e-8), None) == capi.ZT_OK
    one = (capi.AdamTensor * 1)(_entry(capi))
    assert lib.zt_adam_step(one, C.c_int32(0), f(0.9), f(0.999), f(1e-8), None) == capi.ZT_OK


def _plan_np(numel, chunk, limit):
    """zt_adam_plan restated: the non-empty tensors in order, `limit` to a launch, ceil(numel / chunk) workgroups each"""
    blocks = -(-np.asarray([x for x in numel if x > 0], np.int64) // chunk)
    return [int(blocks[i:i + limit].sum()) for i in range(0, len(blocks), limit)]


def test_adam_plan_matches_its_restatement(capi):
    ch, lim = capi.ADAM_CHUNK, capi.ADAM_MAX_TENSORS
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    assert "#define ZT_ADAM_CHUNK %d " % ch in hdr and "#define ZT_ADAM_MAX_TENSORS %d " % lim in hdr
    assert lim >= 32
    cases = [[], [0], [0, 0, 0], [1], [ch - 1], [ch], [ch + 1], [2 * ch + 3], [ch - 1, ch, ch + 1, 2 * ch + 3],
             [ch + 1, 0, 1, 0, 2 * ch + 3], [1] * lim, [1] * (lim + 1), [1] * (2 * lim + 1), [0] * lim + [1],
             [1] * lim + [0] * 5, [ch + 1] * (lim - 1) + [0, 3 * ch, 7], [2 ** 31 - 1, 5],
             [100 * 372, 100, 100 * 372, 100, 300 * 472, 300, 300 * 100, 300]]
    for numel in cases:
        want = _plan_np(numel, ch, lim)
        assert capi.adam_plan(numel) == want, numel
    assert capi.adam_plan([1] * lim) == [lim] and capi.adam_plan([1] * (lim + 1)) == [lim, 1]
    assert capi.adam_plan([1] * (2 * lim + 1)) == [lim, lim, 1]
    assert capi.adam_plan([ch - 1, ch, ch + 1, 2 * ch + 3]) == [1 + 1 + 2 + 3]
    assert capi.adam_plan([0, 0]) == []
    lib = capi.lib()
    out = (C.c_int64 * 4)()
    sizes = (C.c_int64 * 2)(4, -1)
    assert lib.zt_adam_plan(sizes, C.c_int32(2), out) == capi.ZT_ERR_ARG
    sizes = (C.c_int64 * 2)(4, 2 ** 31)
    assert lib.zt_adam_plan(sizes, C.c_int32(2), out) == capi.ZT_ERR_ARG
    assert lib.zt_adam_plan(sizes, C.c_int32(-1), out) == capi.ZT_ERR_ARG
    assert lib.zt_adam_plan(sizes, C.c_int32(1), None) == capi.ZT_ERR_ARG
    assert lib.zt_adam_plan(None, C.c_int32(1), out) == capi.ZT_ERR_ARG


def _group(**kw):
    import zebra_amd
    p = torch.nn.Parameter(torch.zeros(3))
    return zebra_amd.Adam([p], **kw).param_groups[0]


def _with_grad(t, grad=None):
    p = torch.nn.Parameter(t)
    p.grad = torch.ones_like(t) if grad is None else grad
    return p


def test_adam_plan_answers_torch_for_what_the_kernel_does_not_take():
    from zebra_amd.optim import adam_plan
    plain = _group(lr=1e-4)
    cpu = _with_grad(torch.zeros(4, 3))
    assert adam_plan(plain, [cpu]) == "torch"                                        # a CPU parameter
    assert adam_plan(plain, [_with_grad(torch.zeros(4, dtype=torch.float64))]) == "torch"
    # the remaining answers must come from the group / the gradient alone: a parameter that looks like a CUDA one to the plan
    class Fake:
        is_cuda, dtype, device, shape = True, torch.float32, torch.device("cuda", 0), (4, 3)

        def __init__(self, grad_contiguous=True):
            self.grad = None if grad_contiguous is None else Fake(None)
            self._c = True
            if self.grad is not None:
                self.grad.layout = torch.strided
                self.grad._c = grad_contiguous

        def is_contiguous(self):
            return self._c

    assert adam_plan(plain, [Fake()]) == "hip"                                       # (the plan itself is host code)
    assert adam_plan(plain, [Fake(), Fake()]) == "hip"
    assert adam_plan(plain, [Fake(grad_contiguous=False)]) == "torch"               # a non-contiguous gradient
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        assert adam_plan(_group(lr=1e-4, **kw), [Fake()]) == "torch", kw
    assert adam_plan(_group(lr=torch.tensor(1e-4)), [Fake()]) == "torch"
    assert adam_plan(_group(lr=1e-4, betas=(torch.tensor(0.9), torch.tensor(0.999)), capturable=False), [Fake()]) == "torch"
    # ... and a real non-contiguous gradient on a real (CPU) parameter is refused for either reason
    nc = _with_grad(torch.zeros(4, 3), torch.ones(3, 4).t())
    assert not nc.grad.is_contiguous() and adam_plan(plain, [nc]) == "torch"


def _models(seed=3):
    torch.manual_seed(seed)
    shapes = [(5, 7), (7,), (1,), (3, 4, 2), (9,)]
    a = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    return a, b


def _grads(ps, step, skip=None):
    g = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(ps):
        gr = torch.randn(p.shape, generator=g) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))
        p.grad = None if i == skip else gr


def _same_state(oa, ob, pa, pb):
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
        sa, sb = oa.state[x], ob.state[y]
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and sa[k].device == sb[k].device and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("kw", [dict(lr=1e-3), dict(lr=1e-2, weight_decay=0.1, amsgrad=True), dict(lr=1e-3, foreach=False)])
def test_adam_on_cpu_parameters_is_torch_adam_bit_for_bit(kw):
    import zebra_amd
    pa, pb = _models()
    oa, ob = zebra_amd.Adam(pa, **kw), torch.optim.Adam(pb, **kw)
    assert isinstance(oa, torch.optim.Adam)
    for step in range(3):
        skip = 4 if step == 1 else None                  # a parameter without a gradient: skipped, its step does not advance
        _grads(pa, step, skip)
        _grads(pb, step, skip)
        oa.step()
        ob.step()
        _same_state(oa, ob, pa, pb)
    assert float(oa.state[pa[4]]["step"]) == 2.0 and float(oa.state[pa[0]]["step"]) == 3.0
    assert oa.step(lambda: torch.tensor(1.5)) == torch.tensor(1.5)                    # the closure's loss comes back


def test_state_dict_goes_to_torch_adam_and_back():
    import zebra_amd
    pa, pb = _models(5)
    oa, ob = zebra_amd.Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    for step in range(2):
        _grads(pa, step)
        oa.step()
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))   # ours -> torch's (state_dict() hands out the live tensors)
    with torch.no_grad():
        for x, y in zip(pa, pb):
            y.copy_(x)
    _same_state(oa, ob, pa, pb)
    _grads(pa, 7)
    _grads(pb, 7)
    oa.step()
    ob.step()
    _same_state(oa, ob, pa, pb)
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    oc = zebra_amd.Adam(pc, lr=1e-3)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))   # torch's -> ours
    _grads(pb, 8)
    _grads(pc, 8)
    ob.step()
    oc.step()
    _same_state(ob, oc, pb, pc)
    sd = oc.state_dict()
    assert sorted(sd) == sorted(ob.state_dict()) and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert sd["state"][0]["step"].device.type == "cpu" and sd["state"][0]["step"].dtype == torch.float32


def test_link_bce_loss_on_cpu_is_torch_bce():
    import zebra_amd
    g = torch.Generator().manual_seed(2)
    pos, neg = torch.rand((9, 1), generator=g), torch.rand((9, 1), generator=g)
    crit = torch.nn.BCELoss()
    want = crit(pos.squeeze(), torch.ones(9)) + crit(neg.squeeze(), torch.zeros(9))
    assert torch.equal(zebra_amd.link_bce_loss(pos, neg), want)
    assert torch.equal(zebra_amd.link_bce_loss(pos.squeeze(1), neg.squeeze(1)), want)
    d = pos.double().requires_grad_(True)
    zebra_amd.link_bce_loss(d, neg.double()).backward()
    assert d.grad.shape == (9, 1) and torch.allclose(d.grad, -1.0 / (9 * pos.double()))
