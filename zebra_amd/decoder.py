"""Dynamic node classification: the reference's decoder head (MLP, utils/util.py:28-42) on the HIP kernels of
csrc/decoder.hip, and the epoch that trains it on a frozen TGN's source embeddings.

``MLP`` keeps the reference's parameter names and initialisation, so its state dict goes to and from the reference's.
float32 CUDA inputs of a width the kernels take run ONE launch in eval (zt_node_decoder) and one forward plus at most three
backward launches in training (``_HipNodeDecoder``); ``decoder_plan`` is the one place that decides between that and
torch's composition.  The training dropout is a hash of (seed, element): ``decoder_dropout_mask`` restates it in numpy.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from ._capi import check, lib, ptr, stream_ptr

H1, H2 = _capi.DECODER_H1, _capi.DECODER_H2


# Training batches of more rows than this take torch's composition: measured on an MI355X (tools/decoder_time.py, forward +
# loss + backward, H = 300, microseconds per step, fused / torch): 338.7 / 408.4 at 16384 rows, 1246.9 / 779.7 at 65536 -- the
# backward's small sums and its split of d_fc1_w are laid out for batches, not for whole splits.
TRAIN_MAX_ROWS = 16384


def decoder_plan(device_type, dtype, dim, fused=True, rows=None, training=False):
    """Which decoder runs (pure host code, in the manner of tgn.link_score_plan): "hip" when ``fused`` is on, the input is
    float32 on the GPU and its width is one the kernels take (dim % 4 == 0, 4 <= dim <= 4352: zt_node_decoder); else "torch",
    the composition of three Linear layers.  ``rows`` with ``training``: a training forward over more than TRAIN_MAX_ROWS
    rows is "torch" too -- the one range where the fused form measured slower ("Node classification");
    at the timed batch shapes (200 to 4096 rows) it is 2.1 to 3.9 times faster, in eval at every size measured."""
    if not fused or device_type != "cuda" or dtype != torch.float32:
        return "torch"
    if training and rows is not None and rows > TRAIN_MAX_ROWS:
        return "torch"
    return "hip" if (dim % 4 == 0 and _capi.DECODER_MIN_H <= dim <= _capi.DECODER_MAX_H) else "torch"


def _drop_hash(idx, seed, p):
    """csrc/common.hpp drop_scale for uint64 element indices: float32 1 / (1 - p) where kept, else 0 (modules.dropout_mask's
    arithmetic)."""
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        h = ((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) * np.uint32(0x9E3779B1)) ^ lo
        h = h ^ ((idx >> np.uint64(32)).astype(np.uint32) * np.uint32(0x85EBCA77) + hi)
        h ^= h >> np.uint32(16); h *= np.uint32(0x85EBCA6B); h ^= h >> np.uint32(13); h *= np.uint32(0xC2B2AE35); h ^= h >> np.uint32(16)
    pf = float(np.float32(p))
    if not pf > 0:
        return np.ones(idx.shape, np.float32)
    t = pf * 4294967296.0
    thr = np.uint32(4294967295 if t >= 4294967295.0 else int(t))
    return (h >= thr).astype(np.float32) * (np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def decoder_dropout_mask(seed, p, N):
    """The masks the training kernels derive from (seed, element): (m1 [N, 80], m2 [N, 10]) float32 of 1 / (1 - p) and 0 --
    layer 1's element index is row * 80 + col, layer 2's N * 80 + row * 10 + col.  For tests (the kernels never materialise
    them)."""
    i1 = np.arange(N * H1, dtype=np.uint64)
    i2 = np.uint64(N * H1) + np.arange(N * H2, dtype=np.uint64)
    return _drop_hash(i1, seed, p).reshape(N, H1), _drop_hash(i2, seed, p).reshape(N, H2)


def _weights(params):
    w = _capi.DecoderWeights()
    w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b, w.fc3_w, w.fc3_b = (t.data_ptr() for t in params)
    return w


class _HipNodeDecoder(torch.autograd.Function):
    """logits [N] of x [N, H] (float32, CUDA) through zt_node_decoder_train_forward / _backward: one launch forward, at most
    three backward, dropout ``p`` from ``seed`` regenerated in the backward.  No double backward."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, p, seed):
        x = x.contiguous()
        params = [t.detach().contiguous() for t in (w1, b1, w2, b2, w3, b3)]
        N, H = x.shape
        logit = torch.empty(N, dtype=torch.float32, device=x.device)
        h1 = torch.empty((N, H1), dtype=torch.float32, device=x.device)
        h2 = torch.empty((N, H2), dtype=torch.float32, device=x.device)
        w = _weights(params)
        check(lib().zt_node_decoder_train_forward(ptr(x), C.c_int64(N), C.c_int32(H), C.byref(w), C.c_float(p), C.c_uint64(seed),
                                                  ptr(logit), ptr(h1), ptr(h2), stream_ptr()), "zt_node_decoder_train_forward")
        ctx.save_for_backward(x, h1, h2, *params)
        ctx.misc = (p, seed)
        return logit

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dlogit):
        x, h1, h2, *params = ctx.saved_tensors
        p, seed = ctx.misc
        N, H = x.shape
        need = ctx.needs_input_grad
        dev = x.device
        outs = [torch.empty_like(x) if need[0] else None]
        outs += [torch.empty_like(t) if need[1 + i] else None for i, t in enumerate(params)]
        if N == 0:
            return tuple(None if o is None else o.zero_() for o in outs) + (None, None)
        ws = torch.empty(int(lib().zt_node_decoder_train_workspace_bytes(C.c_int64(N), C.c_int32(H))), dtype=torch.uint8, device=dev)
        w = _weights(params)
        check(lib().zt_node_decoder_train_backward(ptr(x), C.c_int64(N), C.c_int32(H), C.byref(w), ptr(h1), ptr(h2),
                                                   ptr(dlogit.to(torch.float32).contiguous()), C.c_float(p), C.c_uint64(seed),
                                                   *[ptr(o) for o in outs], ptr(ws), C.c_int64(N), stream_ptr()),
              "zt_node_decoder_train_backward")
        return tuple(outs) + (None, None)


class MLP(torch.nn.Module):
    """utils/util.py:28-42: fc_1 dim -> 80, fc_2 80 -> 10, fc_3 10 -> 1, ReLU, dropout after each hidden layer.  ``forward``
    returns logits [N]; ``predict`` probabilities.  ``fused_decoder = False`` keeps torch's composition everywhere."""

    def __init__(self, dim, drop=0.3):
        super().__init__()
        self.fc_1 = torch.nn.Linear(dim, H1)
        self.fc_2 = torch.nn.Linear(H1, H2)
        self.fc_3 = torch.nn.Linear(H2, 1)
        self.act = torch.nn.ReLU()
        self.dropout = torch.nn.Dropout(p=drop, inplace=False)
        self.fused_decoder = True
        self._last_drop_seed = 0

    def _params(self):
        return (self.fc_1.weight, self.fc_1.bias, self.fc_2.weight, self.fc_2.bias, self.fc_3.weight, self.fc_3.bias)

    def _plan(self, x, training=False):
        if x.dim() != 2 or x.shape[1] != self.fc_1.in_features or any(t.device != x.device or t.dtype != x.dtype
                                                                      for t in self._params()):
            return "torch"
        return decoder_plan(x.device.type, x.dtype, x.shape[1], self.fused_decoder, rows=x.shape[0], training=training)

    def _torch_forward(self, x):
        x = self.dropout(self.act(self.fc_1(x)))
        x = self.dropout(self.act(self.fc_2(x)))
        return self.fc_3(x).squeeze(dim=1)

    def _eval_launch(self, x, want_prob):
        x = x.detach().contiguous()
        N, H = x.shape
        out = torch.empty(N, dtype=torch.float32, device=x.device)
        w = _weights([t.detach().contiguous() for t in self._params()])
        with torch.cuda.device(x.device):
            check(lib().zt_node_decoder(ptr(x), C.c_int64(N), C.c_int32(H), C.byref(w), None if want_prob else ptr(out),
                                        ptr(out) if want_prob else None, stream_ptr()), "zt_node_decoder")
        return out

    def forward(self, x):
        if self._plan(x) != "hip":
            return self._torch_forward(x)
        p = float(self.dropout.p) if self.training else 0.0
        grad = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in self._params()))
        if not grad and p == 0.0:
            return self._eval_launch(x, False)
        # (nn.Dropout(1.0): everything dropped; not the kernels' case)
        if p >= 1.0 or self._plan(x, training=True) != "hip":
            return self._torch_forward(x)
        # a seed per forward from torch's generator, as the aggregation's dropout draws it (modules.py)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
        self._last_drop_seed = seed
        with torch.cuda.device(x.device):
            return _HipNodeDecoder.apply(x, *self._params(), p, seed)

    @torch.no_grad()
    def predict(self, x):
        """sigmoid(forward(x)) [N] without a graph: one launch in eval mode on the fused path."""
        if self._plan(x) == "hip" and not (self.training and self.dropout.p > 0):
            return self._eval_launch(x, True)
        return self.forward(x).sigmoid()


def train_epoch(tgn, decoder, optimizer, data, batch_size, n_neighbors):
    """One epoch of the decoder's training on a FROZEN model: the TGN is stepped in eval mode over ``data`` (Data with a
    ``labels`` column), the decoder sees the source embeddings of every batch, the loss is BCELoss of the sigmoid against the
    labels.  ``optimizer``: zebra_amd.Adam or torch.optim.Adam over the decoder's parameters.  Returns the mean loss of the
    batches, read from the device once."""
    from .losses import label_bce_loss
    tgn.eval()
    decoder.train()
    n = len(data.sources)
    nb = math.ceil(n / batch_size)
    total = None
    for b in range(nb):
        s, e = b * batch_size, min(n, (b + 1) * batch_size)
        optimizer.zero_grad()
        with torch.no_grad():
            src_emb, _, _ = tgn.compute_temporal_embeddings(data.sources[s:e], data.destinations[s:e], data.destinations[s:e],
                                                            data.timestamps[s:e], data.edge_idxs[s:e], n_neighbors, train=False)
        labels = torch.from_numpy(np.ascontiguousarray(data.labels[s:e], np.float32)).to(src_emb.device, non_blocking=True)
        loss = label_bce_loss(decoder(src_emb).sigmoid(), labels)
        loss.backward()
        optimizer.step()
        total = loss.detach().clone() if total is None else total + loss.detach()
    return float(total.item()) / nb if nb else float("nan")
