"""torch.optim.Adam with the whole step of a parameter group in ONE HIP launch (csrc/train_tail.hip: zt_adam_step).

``Adam`` keeps torch's constructor and torch's state -- ``state[p] = {step: CPU float32 scalar, exp_avg, exp_avg_sq}``, the
layout of torch's non-capturable path -- so ``state_dict()`` / ``load_state_dict()`` go to and from ``torch.optim.Adam``
in both directions and a checkpoint written by either loads into the other.  ``adam_plan`` is the one place that decides,
per group and step, between the kernel and torch's own implementation (train.py:150,215: Adam(lr) with the defaults, which
is the kernel's case).
"""
import ctypes as C

import torch
from torch.optim.adam import adam as _torch_adam
from torch.optim.optimizer import _use_grad_for_differentiable

from . import _capi
from ._capi import check, lib, stream_ptr


def adam_plan(group, params_with_grad, state=None):
    """Which implementation steps a parameter group (pure host code, in the style of tgn.link_score_plan): "hip" -- one
    zt_adam_step on the current stream -- when the group is plain Adam (no weight decay, amsgrad, maximize, capturable,
    differentiable or fused; float ``lr`` and ``betas``) and every parameter with a gradient is a contiguous float32 CUDA
    tensor, all on one device, with a dense contiguous float32 gradient there; else "torch": torch.optim.adam.adam on the same
    state.  With ``state`` (the optimizer's) the moments must be as torch creates them too: contiguous float32 beside their
    parameter, ``step`` on the host (a state loaded from a capturable or fused optimizer keeps it on the device)."""
    if group.get("weight_decay", 0) != 0 or group.get("amsgrad") or group.get("maximize") or group.get("capturable") or \
            group.get("differentiable") or group.get("fused"):
        return "torch"
    if not isinstance(group["lr"], float) or not all(isinstance(b, float) for b in group["betas"]):
        return "torch"
    if not isinstance(group.get("eps", 0.0), float):
        return "torch"
    dev = None
    for p in params_with_grad:
        g = p.grad
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            return "torch"
        if g is None or g.layout != torch.strided or g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() \
                or g.shape != p.shape:
            return "torch"
        if dev is None:
            dev = p.device
        elif p.device != dev:
            return "torch"
        if state is not None:
            st = state[p]
            if st["step"].is_cuda:
                return "torch"
            for m in (st["exp_avg"], st["exp_avg_sq"]):
                if m.dtype != torch.float32 or m.device != p.device or not m.is_contiguous() or m.shape != p.shape:
                    return "torch"
    return "hip"


class Adam(torch.optim.Adam):
    """Drop-in for ``torch.optim.Adam`` (same constructor, same state, same ``state_dict``).  A group ``adam_plan`` answers
    "hip" for is stepped by one zt_adam_step -- every parameter of the group in one launch, no host synchronisation --, any
    other group by torch's implementation on the same state.  Parameters without a gradient are skipped and their ``step``
    does not advance, as in torch."""

    @_use_grad_for_differentiable
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, steps = [], [], [], [], [], []
            has_complex = self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, steps)
            if not params:
                continue
            beta1, beta2 = group["betas"]
            if adam_plan(group, params, self.state) == "hip":
                self._step_hip(params, grads, exp_avgs, exp_avg_sqs, steps, group["lr"], beta1, beta2, group["eps"])
                continue
            _torch_adam(params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, steps, amsgrad=group["amsgrad"],
                        has_complex=has_complex, beta1=beta1, beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"],
                        eps=group["eps"], maximize=group["maximize"], foreach=group["foreach"], capturable=group["capturable"],
                        differentiable=group["differentiable"], fused=group["fused"], grad_scale=getattr(self, "grad_scale", None),
                        found_inf=getattr(self, "found_inf", None), decoupled_weight_decay=group["decoupled_weight_decay"])
        return loss

    @staticmethod
    def _step_hip(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps):
        table = (_capi.AdamTensor * len(params))()
        n = 0
        touched = []
        for p, g, m, v, step_t in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
            step_t += 1
            if p.numel() == 0:
                continue
            t = step_t.item()
            e = table[n]
            n += 1
            touched += [p, m, v]
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            e.numel = p.numel()
            # (torch/optim/adam.py, _single_tensor_adam: the two factors in the host's float64)
            e.step_size = lr / (1 - beta1 ** t)
            e.bias2_sqrt = (1 - beta2 ** t) ** 0.5
        with torch.cuda.device(params[0].device):
            check(lib().zt_adam_step(table, C.c_int32(n), C.c_float(beta1), C.c_float(beta2), C.c_float(eps), stream_ptr()),
                  "zt_adam_step")
        # the kernel wrote through raw pointers: tell autograd, as an in-place torch op would -- a parameter's _version is
        # what the model's packed copies of its weights are keyed on (modules.py, tgn.py), and what a graph that saved the
        # parameter checks on backward
        torch.autograd.graph.increment_version(touched)
