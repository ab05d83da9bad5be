"""Training step at a wide k: the fused neighbour aggregation (row split beyond k = 80, csrc/aggregate_split.hip) against
the torch composition (fused_training = False).  C2's training shape by default: bs = 200, D = T = 100, F = 172, two
T-PPR models.  Prints one JSON line:
  agg_ms   : the neighbour half alone on [M, 3 bs, k] rows (forward + backward of _NeighbourAggregate, or the composition)
  step_ms  : compute_temporal_embeddings(train=True) + backward of a fixed linear loss over the whole model (this includes
             the streaming T-PPR update, the same in both, ~150 us per edge at k = 100 on the wide path)

    python tools/wide_k_train_time.py [--k 100] [--F 172] [--bs 200] [--steps 10] [--warmup 3]
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
from zebra_amd.modules import _NeighbourAggregate  # noqa: E402


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
    return float(np.median(ts)), float(np.min(ts))


def agg_times(tgn, k, n, steps, warmup):
    em, dev = tgn.embedding_module, tgn.device
    D, T, M = em.embedding_dimension, em.n_time_features, em.n_tppr
    N, E1 = tgn.memory.memory.shape[0], em.edge_features.shape[0]
    g = torch.Generator().manual_seed(3)
    mem = torch.randn((N, D), generator=g).to(dev)
    U = n // 2
    ids = torch.randperm(N, generator=g)[:U].to(dev)
    overlay = torch.randn((U, D), generator=g).to(dev).requires_grad_(True)
    row_map = torch.full((N,), -1, dtype=torch.int32, device=dev)
    row_map[ids] = torch.arange(U, dtype=torch.int32, device=dev)
    on = torch.randint(0, N, (M, n, k), generator=g, dtype=torch.int32).to(dev)
    oe = torch.randint(0, E1, (M, n, k), generator=g, dtype=torch.int32).to(dev)
    od = (torch.rand((M, n, k), generator=g) * 1e5).to(dev)
    ow = torch.rand((M, n, k), generator=g).to(dev)
    G = torch.randn((M, n, D), generator=g).to(dev)
    fc1_w = em.fc1.weight.detach().clone().requires_grad_(True)
    fc1_b = em.fc1.bias.detach().clone().requires_grad_(True)

    def fused():
        H, _ = _NeighbourAggregate.apply(overlay, fc1_w, fc1_b, em, mem, row_map, ids.to(torch.int32), on, oe, od, ow, 0.0, 0)
        (H * G).sum().backward()
        row_map[ids] = torch.arange(U, dtype=torch.int32, device=dev)

    def composed():
        rows = torch.where((row_map[on.long()] >= 0).unsqueeze(-1), overlay[row_map[on.long()].long().clamp(min=0)], mem[on.long()])
        x = torch.cat([rows, em.edge_features[oe.long()], em.time_encoder(od.reshape(M * n, k)).reshape(M, n, k, T)], dim=-1)
        h = torch.relu(torch.nn.functional.linear(x, fc1_w, fc1_b))
        ws = ow.sum(dim=2, keepdim=True)
        H = (h * torch.where(ws == 0, torch.zeros_like(ow), ow / ws).unsqueeze(-1)).sum(dim=2)
        (H * G).sum().backward()

    return {"fused": timed(fused, steps, warmup), "composed": timed(composed, steps, warmup)}


def step_times(cfg, fused, steps, warmup):
    D = T = 100
    N, E, F, k, bs = cfg["N"], cfg["E"], cfg["F"], cfg["k"], cfg["bs"]
    src, dst, neg, ts, eidx = I.make_stream("bipartite", N, E, 11)
    w = I.model_weights(D, F, T, 2, 11)
    _, efeat = I.random_tables(N, E + 1, D, F, 11)
    tgn = build_tgn(N, E + 1, D, F, T, k, [0.1, 0.1], [0.5, 0.95], w, efeat)
    tgn.embedding_module.fused_training = fused
    tgn.train(True)
    G = torch.randn((3 * bs, 3 * D), generator=torch.Generator().manual_seed(5)).cuda()
    pos = [0]

    def step():
        s = pos[0]
        e = s + bs
        pos[0] = e
        tgn.zero_grad()
        se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
        (torch.cat([se, de, ne]) * G).sum().backward()
        tgn.memory.detach_memory()

    return timed(step, steps, warmup), tgn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--F", type=int, default=172)
    ap.add_argument("--bs", type=int, default=200)
    ap.add_argument("--N", type=int, default=9227)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    cfg = dict(N=a.N, E=(a.steps + a.warmup) * a.bs, F=a.F, k=a.k, bs=a.bs)
    out = {"k": a.k, "F": a.F, "bs": a.bs, "D": 100, "T": 100, "M": 2}
    for fused in (True, False):
        (med, mn), tgn = step_times(cfg, fused, a.steps, a.warmup)
        out["step_ms_%s" % ("fused" if fused else "composed")] = {"median": round(med, 3), "min": round(mn, 3)}
    ag = agg_times(tgn, a.k, 3 * a.bs, a.steps, a.warmup)
    out["agg_ms"] = {kk: {"median": round(v[0], 3), "min": round(v[1], 3)} for kk, v in ag.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
