"""Forward + backward of a training step's link scorer: the HIP kernels (csrc/scoring_train.hip through TGN.score_train,
fused_scoring=True) against torch's composition of MergeLayer under autograd (fused_scoring=False), in ONE process on one
GPU.  Per shape BxH -- defaults: C2's training shape 200x300, C5's batch 4096x300, D = 172 with two T-PPR models 200x516 --
the two alternate round by round after a warm-up; a round is `--iters` times (scores from the [3B, H] embeddings, backward
from d(pos), d(neg) to the embeddings and the four parameters) between two device synchronisations.  Prints one JSON line
per shape with the median microseconds per forward + backward of both, over `--rounds` (>= 20) rounds.

GPU time and launch count come from a run of its own under the profiler, one mode at a time:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/score_train_time.py --only fused --shapes 200x300 --rounds 1 --iters 100 --warmup 0
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/score_train_time.py --only torch ...

(kernel calls / iters = launches per forward + backward; sum of the kernels' time / iters = GPU time.)

    python tools/score_train_time.py [--shapes 200x300,4096x300,200x516] [--rounds 30] [--iters 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from zebra_amd.modules import MergeLayer  # noqa: E402
from zebra_amd.tgn import TGN, link_score_plan  # noqa: E402


def make_case(B, H, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * H + B)
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = MergeLayer(H, H, H, 1).to(dev)
    emb = (torch.randn((3 * B, H), generator=g) * 0.7).to(dev).requires_grad_(True)
    dpos = (-(1.0 + torch.rand((B, 1), generator=g)) / B).to(dev)
    dneg = ((1.0 + torch.rand((B, 1), generator=g)) / B).to(dev)
    scorers = {}
    for mode in ("fused", "torch"):
        holder = types.SimpleNamespace(affinity_score=layer, fused_scoring=mode == "fused")
        holder._score_pairs = types.MethodType(TGN._score_pairs, holder)
        scorers[mode] = types.MethodType(TGN.score_train, holder)
    assert link_score_plan("cuda", torch.float32, H, True) == "hip", "no HIP scorer for H=%d" % H
    return layer, emb, (dpos, dneg), scorers


def run(layer, emb, dout, score, iters):
    for _ in range(iters):
        emb.grad = None
        for p in layer.parameters():
            p.grad = None
        pos, neg = score(emb)
        torch.autograd.backward([pos, neg], list(dout))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200x300,4096x300,200x516")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", choices=["", "fused", "torch"], help="one mode alone (a profiler run)")
    a = ap.parse_args()
    modes = [a.only] if a.only else ["fused", "torch"]
    for shape in a.shapes.split(","):
        B, H = [int(x) for x in shape.lower().split("x")]
        layer, emb, dout, scorers = make_case(B, H)
        us = {m: [] for m in modes}
        for r in range(a.warmup + a.rounds):
            for m in (modes if r % 2 == 0 else modes[::-1]):          # the order alternates too
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(layer, emb, dout, scorers[m], a.iters)
                torch.cuda.synchronize()
                if r >= a.warmup:
                    us[m].append(1e6 * (time.perf_counter() - t0) / a.iters)
        out = dict(B=B, H=H, rounds=a.rounds, iters=a.iters, total_iters={m: (a.warmup + a.rounds) * a.iters for m in modes})
        for m in modes:
            out[m + "_us_median"] = round(float(np.median(us[m])), 2)
            out[m + "_us_min"] = round(float(np.min(us[m])), 2)
        if len(modes) == 2:
            out["fused_over_torch"] = round(out["fused_us_median"] / out["torch_us_median"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
