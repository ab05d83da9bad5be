"""Forward + backward of a ranking step's scorer and loss against the clock (csrc/rank_train.hip, csrc/train_tail.hip), in ONE
process on one GPU: TGN.score_many_train + losses.listwise_loss (softmax) + backward to the embeddings and the scorer's four
parameters, for (B, K, H) = (200, 100, 300), (200, 100, 516), (600, 100, 300), (200, 1000, 200) -- B sources, each against its
destination and K negatives of its own: Q = B, C = 1 + K, emb_c of B + B K rows, every row named once, as
TGN.compute_rank_loss lays them out.

  hip     rank_score_plan "hip": _HipRankScore (two projections, the pair kernel; the backward from the saved projections)
  torch   fused_scoring = False on the same device: MergeLayer over the [Q, C, 2H] concatenation under autograd, a chunk of
          queries at a time -- what a user without the kernels composes.  The yardstick.

The two alternate round by round after a warm-up; a round is `--iters` steps between two events on the stream.  Each mode's
peak memory is torch.cuda.max_memory_allocated over one step above what is allocated before it -- inputs and parameters only:
the gradients of the step before are released first, so the step's own outgoing gradients are part of its peak.
Prints one JSON line per shape (and appends it to --out, if given): the median microseconds per step of both over `--rounds`
rounds with the spread (min, max), the peaks, and the largest difference of the two modes' logits and gradients.

    python tools/rank_train_time.py [--rounds 10] [--iters 50] [--warmup 2] [--out profiles/r12/rank_train_time.jsonl]
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from zebra_amd.losses import listwise_loss  # noqa: E402
from zebra_amd.modules import MergeLayer  # noqa: E402
from zebra_amd.tgn import TGN, rank_score_plan  # noqa: E402

SHAPES = [(200, 100, 300), (200, 100, 516), (600, 100, 300), (200, 1000, 200)]


def timed(fns, rounds, iters, warmup):
    """{name: [us per call, one per round]} for the callables of `fns`, alternating in order round by round"""
    us = {m: [] for m in fns}
    names = list(fns)
    for r in range(warmup + rounds):
        for m in (names if r % 2 == 0 else names[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fns[m]()
            t1.record()
            t1.synchronize()
            if r >= warmup:
                us[m].append(1e3 * t0.elapsed_time(t1) / iters)
    return us


def summary(us):
    return {m: dict(median_us=round(float(np.median(v)), 2), min_us=round(float(np.min(v)), 2), max_us=round(float(np.max(v)), 2))
            for m, v in us.items()}


def case(B, K, H, seed=0):
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = MergeLayer(H, H, H, 1).to(dev)
    g = torch.Generator().manual_seed(seed + B + K)
    emb_q = (torch.randn((B, H), generator=g) * 0.7).to(dev).requires_grad_(True)
    emb_c = (torch.randn((B + B * K, H), generator=g) * 0.7).to(dev).requires_grad_(True)
    idx = torch.cat([torch.arange(B).unsqueeze(1), B + torch.arange(B * K).reshape(B, K)], dim=1).to(torch.int32).to(dev)
    holders = {m: types.SimpleNamespace(affinity_score=layer, device=dev, fused_scoring=(m == "hip")) for m in ("hip", "torch")}
    assert rank_score_plan("cuda", torch.float32, H, True) == "hip"

    def step(mode):
        layer.zero_grad(set_to_none=True)
        emb_q.grad = emb_c.grad = None
        logits = TGN.score_many_train(holders[mode], emb_q, emb_c, idx)
        listwise_loss(logits, None, "softmax").backward()
        return logits.detach()

    def outputs(mode):
        lg = step(mode)
        return [lg, emb_q.grad.clone(), emb_c.grad.clone()] + [p.grad.clone() for p in layer.parameters()]

    def peak(mode):
        step(mode)
        # the warm-up step's gradients go before the baseline is read: the measured step would free them first, and its peak
        # above a baseline that still held them would come out too low by their size
        layer.zero_grad(set_to_none=True)
        emb_q.grad = emb_c.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(mode)
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    diff = max(float((a - b).abs().max()) for a, b in zip(outputs("hip"), outputs("torch")))
    peaks = {m: peak(m) for m in ("hip", "torch")}
    return {m: (lambda m=m: step(m)) for m in ("hip", "torch")}, diff, peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for B, K, H in SHAPES:
        fns, diff, peaks = case(B, K, H)
        res = dict(tool="rank_train_time", device=torch.cuda.get_device_name(0), rounds=a.rounds, iters=a.iters, warmup=a.warmup,
                   B=B, K=K, H=H, max_abs_diff_hip_torch=diff, peak_bytes=peaks, **summary(timed(fns, a.rounds, a.iters, a.warmup)))
        res["hip_over_torch"] = round(res["hip"]["median_us"] / res["torch"]["median_us"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        del fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
