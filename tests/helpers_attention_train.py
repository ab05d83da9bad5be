"""TemporalAttentionLayer as a plain composition of tensor operations with an explicit keep-mask on the softmax weights -- what
nn.MultiheadAttention computes (q scaled by 1 / sqrt(head_dim), key-padding mask, softmax, dropout ON the weights, the weighted
sum, out_proj) followed by the layer's zeroing of rows without a neighbour and its MergeLayer -- for the tests of the training
kernels (csrc/attention_train.hip): nn.MultiheadAttention draws its mask itself and cannot be given ours.  dtype-generic, runs
under torch autograd on any device.  attn_w is the head mean of the weights after dropout, as torch returns them.

Cases, inputs and weights are tests/test_attention_f64_gpu.py's (make_case, make_weights), imported by the test files."""
import math

import numpy as np
import torch

X_KEYS = ("src", "src_t", "nbr", "nbr_t", "edge")           # the order of make_case's x and of the layer's forward
W_KEYS = ("q_w", "k_w", "v_w", "in_b", "out_w", "out_b", "m1_w", "m1_b", "m2_w", "m2_b")
GRAD_KEYS = X_KEYS + W_KEYS                                 # the 15 gradients


def err(a, b):
    """max |a - b| in float64; 0 for arrays without an element (the edge gradient at F = 0)"""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0.0))


def keep_mask(seed, p, N, heads, k):
    """float32 [N, heads, k] of 1 / (1 - p) and 0: the kernels' mask (element (n * heads + h) * k + j of the hash)"""
    from zebra_amd.modules import dropout_mask
    return dropout_mask(seed, p, (1, N, heads), k)[0]


def forward(x, w, heads, keep=None):
    """x = (src [N, D], src_t [N, 1, T] or [N, T], nbr [N, k, D], nbr_t [N, k, T], edge [N, k, F], mask bool [N, k]) and
    w = {name: tensor} in torch layout; keep [N, heads, k] or None -> (out [N, out_dim], attn_w [N, k])"""
    src, src_t, nbr, nbr_t, edge, mask = x
    N, k, D = nbr.shape
    xq = torch.cat([src, src_t.reshape(N, -1)], dim=1)
    a = torch.cat([nbr, edge, nbr_t], dim=2)
    E = xq.shape[1]
    hd = E // heads
    b = w["in_b"]
    q = (xq @ w["q_w"].T + b[:E]) / math.sqrt(hd)
    K = a @ w["k_w"].T + b[E:2 * E]
    V = a @ w["v_w"].T + b[2 * E:]
    inv = mask.all(dim=1)
    m = mask.clone()
    m[inv, 0] = False
    s = torch.einsum("nhc,nkhc->nhk", q.reshape(N, heads, hd), K.reshape(N, k, heads, hd))
    s = s.masked_fill(m[:, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    pt = p if keep is None else p * keep
    o = torch.einsum("nhk,nkhc->nhc", pt, V.reshape(N, k, heads, hd)).reshape(N, E)
    y = (o @ w["out_w"].T + w["out_b"]).masked_fill(inv[:, None], 0)
    hid = torch.relu(torch.cat([y, src], dim=1) @ w["m1_w"].T + w["m1_b"])
    out = hid @ w["m2_w"].T + w["m2_b"]
    return out, pt.mean(dim=1).masked_fill(inv[:, None], 0)


def tensors(c, dtype, device="cpu", requires_grad=True):
    """(x, w) of a make_case dict as fresh leaf tensors"""
    def leaf(a):
        t = torch.from_numpy(np.array(a)).to(device)
        if t.dtype == torch.bool:
            return t
        return t.to(dtype).requires_grad_(requires_grad)
    return [leaf(a) for a in c["x"]], {kk: leaf(c["w"][kk]) for kk in W_KEYS}


def run(c, d_out, keep, dtype, device="cpu"):
    """out, attn_w and the 15 gradients of sum(out * d_out), as float64 numpy arrays by name"""
    x, w = tensors(c, dtype, device)
    kt = None if keep is None else torch.from_numpy(np.array(keep)).to(device).to(dtype)
    out, aw = forward(x, w, c["heads"], kt)
    (out * torch.from_numpy(np.array(d_out)).to(device).to(dtype)).sum().backward()
    res = {"out": out, "attn_w": aw}
    res.update({kk: t.grad if t.grad is not None else torch.zeros_like(t) for kk, t in zip(X_KEYS, x)})     # (F = 0: no edge column)
    res.update({kk: w[kk].grad for kk in W_KEYS})
    return {kk: v.detach().double().cpu().numpy() for kk, v in res.items()}
