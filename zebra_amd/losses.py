"""The loss of a training step (train.py:212-213) as one HIP kernel with its gradient (csrc/train_tail.hip:
zt_link_bce_forward / zt_link_bce_backward), and the label loss of node classification beside it (zt_label_bce_forward /
zt_label_bce_backward); the listwise loss of a ranking step (zt_rank_loss_forward / zt_rank_loss_backward)."""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _capi
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


RANK_LOSS_MODES = {"softmax": _capi.RANK_LOSS_SOFTMAX, "bce": _capi.RANK_LOSS_BCE}


class _HipRankLoss(torch.autograd.Function):
    """loss [] of logits [Q, C] (float32 CUDA, -inf: absent pair) against the positive's column ``target`` int32 [Q] (None:
    column 0), ``mode`` "softmax" or "bce" (listwise_loss): one launch forward that also writes d(loss)/d(logit), one launch
    backward that scales it by the incoming gradient, read on the device (csrc/train_tail.hip: zt_rank_loss_forward /
    zt_rank_loss_backward).  No double backward."""

    @staticmethod
    def forward(ctx, logits, target, mode):
        logits = logits.contiguous()
        Q, C_ = logits.shape
        tgt = None if target is None else target.to(logits.device, torch.int32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        dl = torch.empty_like(logits)
        check(lib().zt_rank_loss_forward(ptr(logits), ptr(tgt), C.c_int64(Q), C.c_int64(C_), C.c_int32(RANK_LOSS_MODES[mode]),
                                         ptr(loss), ptr(dl), stream_ptr()), "zt_rank_loss_forward")
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        dl, = ctx.saved_tensors
        out = torch.empty_like(dl)
        grad_loss = grad_loss.to(torch.float32).contiguous()
        check(lib().zt_rank_loss_backward(ptr(dl), ptr(grad_loss), C.c_int64(dl.numel()), ptr(out), stream_ptr()),
              "zt_rank_loss_backward")
        return out, None, None


def rank_loss_plan(logits, target=None):
    """Which loss listwise_loss runs (pure host code): "hip" for a non-empty float32 CUDA matrix [Q, C] (and a target without
    a gradient on the same device, if one is given), else "torch"."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.numel() >= 1):
        return "torch"
    if target is not None and (target.device != logits.device or target.is_floating_point() or target.numel() != logits.shape[0]):
        return "torch"
    return "hip"


def listwise_loss(logits, target=None, mode="softmax"):
    """The loss of a ranking step over logits [Q, C], -inf where a pair is absent (TGN.score_many_train); ``target`` [Q]
    (integer; None: column 0) is the positive's column.  A query whose target is absent is skipped; with none left the loss
    is 0 and so is its gradient.
      "softmax": mean over live queries of logsumexp over the present columns - the target's logit (cross-entropy);
      "bce":     mean over live queries of -max(log sigmoid(target logit), -100) plus the mean over the present non-target
                 pairs of live queries of -max(log(1 - sigmoid(logit)), -100): link_bce_loss when C = 2.
    _HipRankLoss for float32 CUDA logits (rank_loss_plan), torch's composition otherwise."""
    if mode not in RANK_LOSS_MODES:
        raise ValueError("listwise_loss: mode must be 'softmax' or 'bce'")
    if logits.dim() != 2:
        raise ValueError("listwise_loss: logits [Q, C] expected")
    if rank_loss_plan(logits, target) == "hip":
        with torch.cuda.device(logits.device):
            return _HipRankLoss.apply(logits, target, mode)
    Q, C_ = logits.shape
    zero = torch.where(torch.isfinite(logits), logits, torch.zeros_like(logits)).sum() * 0     # (0 with an all-zero gradient)
    if Q == 0 or C_ == 0:
        return zero
    t = torch.zeros(Q, dtype=torch.long, device=logits.device) if target is None else target.to(logits.device).long()
    ok = (t >= 0) & (t < C_)
    tl = logits.gather(1, t.clamp(0, C_ - 1).unsqueeze(1)).squeeze(1)
    live = ok & (tl != float("-inf"))
    if not bool(live.any()):
        return zero
    lg, t, tl = logits[live], t[live], tl[live]
    if mode == "softmax":
        return (torch.logsumexp(lg, dim=1) - tl).mean()
    other = lg != float("-inf")
    other[torch.arange(lg.shape[0], device=lg.device), t] = False
    loss = (-F.logsigmoid(tl).clamp(min=-100)).mean()
    if bool(other.any()):
        loss = loss + (-F.logsigmoid(-lg[other]).clamp(min=-100)).mean()
    return loss
