"""Forward + backward of TemporalAttentionLayer in training mode: the HIP kernels (csrc/attention_train.hip,
fused_training=True) against the same layer on nn.MultiheadAttention under autograd (fused_training=False), in ONE process on
one GPU.  Per shape DxFxTxkxN (heads = 2, hidden = out = D, dropout 0.1, 40 % of the slots padding) the two alternate round by
round after a warm-up; a round is `--iters` times (forward, backward from a fixed d_out to the five inputs and all parameters)
between two device synchronisations.  Prints one JSON line per shape: the median and minimum microseconds per forward +
backward of both over `--rounds` rounds, and each mode's peak device memory above what is allocated before its first
iteration (inputs, parameters and d_out), measured over one iteration of its own with torch's allocator statistics.

    python tools/attention_train_time.py [--shapes 100x172x100x20x600,100x1x100x40x3000,20x4x12x5x600] [--rounds 30]
                                         [--iters 10] [--warmup 3] [--out profiles/attention_train_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from zebra_amd.modules import TemporalAttentionLayer, attention_train_plan  # noqa: E402


def make_case(D, F, T, k, N, heads=2, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * D + 3 * F + k + N)
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = TemporalAttentionLayer(D, D, F, T, output_dimension=D, n_head=heads, dropout=0.1).to(dev).train()
    r = lambda *s: torch.randn(s, generator=g).to(dev).requires_grad_(True)
    mask = (torch.rand((N, k), generator=g) < 0.4).to(dev)
    x = [r(N, D), r(N, 1, T), r(N, k, D), r(N, k, T), r(N, k, F), mask]
    d_out = (torch.randn((N, D), generator=g) / N).to(dev)
    assert attention_train_plan("cuda", torch.float32, D, F, T, heads, D, D, k) == "hip", "no HIP training path for this shape"
    return layer, x, d_out


def run(layer, x, d_out, fused, iters):
    layer.fused_training = fused
    for _ in range(iters):
        for t in x[:5]:
            t.grad = None
        for p in layer.parameters():
            p.grad = None
        out, _ = layer(*x)
        out.backward(d_out)


def peak_above_inputs(layer, x, d_out, fused):
    run(layer, x, d_out, fused, 1)                       # gradients exist afterwards, as in the timed rounds
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run(layer, x, d_out, fused, 1)
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x172x100x20x600,100x1x100x40x3000,20x4x12x5x600")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    modes = {"fused": True, "torch": False}
    for shape in a.shapes.split(","):
        D, F, T, k, N = [int(v) for v in shape.lower().split("x")]
        layer, x, d_out = make_case(D, F, T, k, N)
        us = {m: [] for m in modes}
        names = list(modes)
        for r in range(a.warmup + a.rounds):
            for m in (names if r % 2 == 0 else names[::-1]):          # the order alternates too
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(layer, x, d_out, modes[m], a.iters)
                torch.cuda.synchronize()
                if r >= a.warmup:
                    us[m].append(1e6 * (time.perf_counter() - t0) / a.iters)
        out = dict(D=D, F=F, T=T, k=k, N=N, heads=2, rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(0))
        for m in names:
            out[m + "_us_median"] = round(float(np.median(us[m])), 1)
            out[m + "_us_min"] = round(float(np.min(us[m])), 1)
            out[m + "_peak_bytes_above_inputs"] = peak_above_inputs(layer, x, d_out, modes[m])
        out["fused_over_torch"] = round(out["fused_us_median"] / out["torch_us_median"], 3)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
