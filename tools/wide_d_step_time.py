"""Eval and training step time at memory / embedding widths D = 100, 172, 256 on C2's stream shape (bs = 200, F = 172,
T = 100, k = 20, two T-PPR models; a synthetic bipartite stream).  Prints one JSON line: per D, the median and minimum ms of
  eval_ms  : compute_temporal_embeddings(train=False) (T-PPR, aggregation, output layers, messages, GRU update)
  train_ms : compute_temporal_embeddings(train=True) + backward of a fixed linear loss (fused training)

    python tools/wide_d_step_time.py [--D 100,172,256] [--bs 200] [--k 20] [--F 172] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import inputs as I  # noqa: E402
from helpers import build_tgn  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(steps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median": round(float(np.median(ts)), 3), "min": round(float(np.min(ts)), 3)}


def step_time(D, train, a):
    T, N, bs = 100, a.N, a.bs
    E = (a.steps + a.warmup) * bs
    src, dst, neg, ts, eidx = I.make_stream("bipartite", N, E, 13)
    w = I.model_weights(D, a.F, T, 2, 13)
    _, efeat = I.random_tables(N, E + 1, D, a.F, 13)
    tgn = build_tgn(N, E + 1, D, a.F, T, a.k, [0.1, 0.1], [0.5, 0.95], w, efeat)
    tgn.train(train)
    G = torch.randn((3 * bs, 3 * D), generator=torch.Generator().manual_seed(5)).cuda()
    pos = [0]

    def step():
        s = pos[0]
        e = s + bs
        pos[0] = e
        if train:
            tgn.zero_grad()
            se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
            (torch.cat([se, de, ne]) * G).sum().backward()
            tgn.memory.detach_memory()
        else:
            with torch.no_grad():
                tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, False)

    return timed(step, a.steps, a.warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", default="100,172,256")
    ap.add_argument("--bs", type=int, default=200)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--F", type=int, default=172)
    ap.add_argument("--N", type=int, default=9227)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"bs": a.bs, "k": a.k, "F": a.F, "T": 100, "M": 2}
    for D in [int(x) for x in a.D.split(",")]:
        out["D%d" % D] = {"eval_ms": step_time(D, False, a), "train_ms": step_time(D, True, a)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
