"""The loss of a training step (train.py:212-213) as one HIP kernel with its gradient (csrc/train_tail.hip:
zt_link_bce_forward / zt_link_bce_backward), and the label loss of node classification beside it (zt_label_bce_forward /
zt_label_bce_backward)."""
import ctypes as C

import torch
import torch.nn.functional as F

from ._capi import check, lib, ptr, stream_ptr


class _HipLinkBCE(torch.autograd.Function):
    """loss [] = BCELoss(prob[:B], 1) + BCELoss(prob[B:], 0) for the [2B] float32 CUDA vector the link scorer returns -- B
    positive pairs, then B negative ones.  The forward is one launch that also writes d(loss)/d(prob); the backward is one
    launch that scales it by the incoming gradient, read on the device.  No double backward."""

    @staticmethod
    def forward(ctx, prob):
        prob = prob.contiguous()
        B = prob.numel() // 2
        if prob.dim() != 1 or B < 1 or prob.numel() != 2 * B:
            raise ValueError("_HipLinkBCE: prob [2B] with B >= 1 expected")
        loss = torch.empty((), dtype=torch.float32, device=prob.device)
        dprob = torch.empty_like(prob)
        check(lib().zt_link_bce_forward(ptr(prob), C.c_int64(B), ptr(loss), ptr(dprob), stream_ptr()), "zt_link_bce_forward")
        ctx.save_for_backward(dprob)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        dprob, = ctx.saved_tensors
        out = torch.empty_like(dprob)
        grad_loss = grad_loss.to(torch.float32).contiguous()
        check(lib().zt_link_bce_backward(ptr(dprob), ptr(grad_loss), C.c_int64(dprob.numel() // 2), ptr(out), stream_ptr()),
              "zt_link_bce_backward")
        return out


def link_bce_plan(pos, neg):
    """Which loss link_bce_loss runs (pure host code): "hip" for float32 CUDA probabilities of one non-empty batch on one
    device, else "torch"."""
    if not (pos.is_cuda and neg.is_cuda and pos.device == neg.device and pos.dtype == neg.dtype == torch.float32):
        return "torch"
    return "hip" if pos.numel() == neg.numel() >= 1 else "torch"


def link_bce_loss(pos, neg):
    """criterion(pos.squeeze(), ones) + criterion(neg.squeeze(), zeros) with criterion = torch.nn.BCELoss() (train.py:163,
    212-213) for the [B] or [B, 1] probabilities of B positive and B negative pairs: _HipLinkBCE for float32 CUDA inputs,
    F.binary_cross_entropy with ones and zeros otherwise."""
    pos, neg = pos.reshape(-1), neg.reshape(-1)
    if link_bce_plan(pos, neg) == "hip":
        with torch.cuda.device(pos.device):
            return _HipLinkBCE.apply(torch.cat([pos, neg]))
    return F.binary_cross_entropy(pos, torch.ones_like(pos)) + F.binary_cross_entropy(neg, torch.zeros_like(neg))


class _HipLabelBCE(torch.autograd.Function):
    """loss [] = BCELoss()(prob, labels) (mean) for float32 CUDA vectors [N]: one launch forward that also writes
    d(loss)/d(prob), one launch backward.  The labels get no gradient.  No double backward."""

    @staticmethod
    def forward(ctx, prob, labels):
        prob, labels = prob.contiguous(), labels.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=prob.device)
        dprob = torch.empty_like(prob)
        check(lib().zt_label_bce_forward(ptr(prob), ptr(labels), C.c_int64(prob.numel()), ptr(loss), ptr(dprob), stream_ptr()),
              "zt_label_bce_forward")
        ctx.save_for_backward(dprob)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        dprob, = ctx.saved_tensors
        out = torch.empty_like(dprob)
        grad_loss = grad_loss.to(torch.float32).contiguous()
        check(lib().zt_label_bce_backward(ptr(dprob), ptr(grad_loss), C.c_int64(dprob.numel()), ptr(out), stream_ptr()),
              "zt_label_bce_backward")
        return out, None


def label_bce_plan(prob, labels):
    """Which loss label_bce_loss runs (pure host code): "hip" for float32 CUDA probabilities and labels of one non-empty
    batch on one device, the labels without a gradient; else "torch"."""
    if not (prob.is_cuda and labels.is_cuda and prob.device == labels.device and prob.dtype == labels.dtype == torch.float32):
        return "torch"
    if labels.requires_grad:
        return "torch"
    return "hip" if prob.numel() == labels.numel() >= 1 else "torch"


def label_bce_loss(prob, labels):
    """torch.nn.BCELoss()(prob, labels) for the [N] or [N, 1] probabilities of N rows and a float label per row (the
    decoder's loss in node classification): _HipLabelBCE for float32 CUDA inputs, F.binary_cross_entropy otherwise."""
    prob, labels = prob.reshape(-1), labels.reshape(-1)
    if label_bce_plan(prob, labels) == "hip":
        with torch.cuda.device(prob.device):
            return _HipLabelBCE.apply(prob, labels)
    return F.binary_cross_entropy(prob, labels.to(prob.dtype))
