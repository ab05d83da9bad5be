"""The read-only T-PPR query and the one-vs-many scorer (csrc/tppr_query.hip, csrc/rank.hip) against the clock, in ONE process
on one GPU:

  zt_tppr_query     N = 12 288 rows, k = 20, two models, on a state a power-law stream of 40 000 edges over 10 000 nodes filled;
  zt_affinity_rank  (Q, C, H) = (200, 100, 300), (200, 1000, 300), (4096, 100, 300), with shared candidates (cand_idx NULL) and
                    with per-query indices into a pool of 4 C candidate rows -- its two GEMMs included;
  torch             the same shapes as a user of the library without the kernel would write them: the two projections, then
                    relu(P_q[:, None, :] + P_c[idx]) @ w2 + b2 and the sigmoid -- the broadcast form, which materialises
                    [Q, C, H].  This is the yardstick.

The modes alternate round by round after a warm-up; a round is `--iters` calls between two events on the stream.  Prints ONE
JSON line: the median microseconds per call of every mode over `--rounds` rounds, with the spread (min, max).

    python tools/rank_time.py [--rounds 20] [--iters 20] [--warmup 3]
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

from zebra_amd import synth  # noqa: E402
from zebra_amd.modules import MergeLayer  # noqa: E402
from zebra_amd.tgn import TGN  # noqa: E402
from zebra_amd.tppr import tppr_finder  # noqa: E402

SHAPES = [(200, 100, 300), (200, 1000, 300), (4096, 100, 300)]


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


def query_case():
    dev = torch.device("cuda")
    n_nodes, n_edges, k = 10000, 40000, 20
    src, dst, ts, eidx = synth.power_law_stream(n_nodes, n_edges, seed=5)
    f = tppr_finder(n_nodes + 1, k, 2, [0.1, 0.1], [0.5, 0.95])
    for s in range(0, n_edges, 4096):
        e = min(n_edges, s + 4096)
        nodes = np.concatenate([src[s:e], dst[s:e]])
        n, t, ei, _ = f._upload(nodes, ts[s:e], eidx[s:e], 2)
        f.stream_device(n, t, ei, 2, False, -1, check_status=False)
    f.check_status()
    rng = np.random.RandomState(6)
    q = torch.from_numpy(np.concatenate([src[-8192:], dst[-4096:]]).astype(np.int32)).to(dev)
    tq = torch.from_numpy(np.full(12288, ts[-1] + 1.0) + rng.random_sample(12288)).to(dev)
    return {"tppr_query": lambda: f.query_device(q, tq, check_status=False)}


def rank_case(Q, C_, H, seed=0):
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = MergeLayer(H, H, H, 1).to(dev)
    g = torch.Generator().manual_seed(seed + Q + C_)
    emb_q = (torch.randn((Q, H), generator=g) * 0.7).to(dev)
    pool = (torch.randn((4 * C_, H), generator=g) * 0.7).to(dev)
    idx = torch.randint(0, 4 * C_, (Q, C_), generator=g).to(torch.int32).to(dev)
    idx_l = idx.long()
    shared = pool[:C_].contiguous()
    holder = types.SimpleNamespace(affinity_score=layer, device=dev)
    hip = types.MethodType(TGN.rank_scores, holder)
    Wa, Wb = layer.fc1.weight[:, :H], layer.fc1.weight[:, H:]
    w2, b1, b2 = layer.fc2.weight[0], layer.fc1.bias, layer.fc2.bias

    @torch.no_grad()
    def composed(emb_c, ix):
        pq, pc = emb_q @ Wa.t() + b1, emb_c @ Wb.t()
        pc = pc.unsqueeze(0) if ix is None else pc[ix]
        return (torch.relu(pq.unsqueeze(1) + pc) @ w2 + b2).sigmoid()

    fns = {"hip_shared": lambda: hip(emb_q, shared, None, check_status=False),
           "torch_shared": lambda: composed(shared, None),
           "hip_indexed": lambda: hip(emb_q, pool, idx, check_status=False),
           "torch_indexed": lambda: composed(pool, idx_l)}
    diff = max(float((fns["hip_shared"]() - fns["torch_shared"]()).abs().max()),
               float((fns["hip_indexed"]() - fns["torch_indexed"]()).abs().max()))
    return fns, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = dict(tool="rank_time", rounds=a.rounds, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    out["tppr_query"] = dict(N=12288, k=20, M=2, **summary(timed(query_case(), a.rounds, a.iters, a.warmup))["tppr_query"])
    out["shapes"] = []
    for Q, C_, H in SHAPES:
        fns, diff = rank_case(Q, C_, H)
        res = dict(Q=Q, C=C_, H=H, max_abs_diff_to_torch=diff, **summary(timed(fns, a.rounds, a.iters, a.warmup)))
        for mode in ("shared", "indexed"):
            res["hip_over_torch_" + mode] = round(res["hip_" + mode]["median_us"] / res["torch_" + mode]["median_us"], 3)
        out["shapes"].append(res)
        del fns
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
