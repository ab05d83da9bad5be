"""Time of the pruning query for walks beyond its LDS form (csrc/tppr_prune.hip: k_pruned_topk_ws) at C4's shape: one
batch of 1 000 edges = 3 000 queries, k = 40, C4's two (alpha, beta) models, on a prefix of C4's stream (bench.py's
generator and seeds).  Shapes: 10 x 2 (the LDS form, for scale), 40 x 2, 20 x 3 and 10 x 4.  The parent of the commit that
added the workspace form refuses all but the first, so the baseline is the CPU oracle (zo_pruned_topk, one thread) on
the same queries; the tool also holds the kernel's outputs to the oracle's, bit for bit, at the sizes it times.

For each shape: one JSON line with the plan (form, slabs, slab bytes), the median and the spread of `--repeat` timed calls
(host clock around zt_pruned_topk_multi + a device synchronise, after `--warmup` calls), and the oracle's seconds.

    python tools/prune_wide_time.py [--edges 300000] [--repeat 7] [--warmup 2] [--shapes 10x2,40x2,20x3,10x4]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from zebra_amd import synth  # noqa: E402
from zebra_amd.tppr import get_neighbor_finder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=300000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="10x2,40x2,20x3,10x4")
    ap.add_argument("--max-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prune_wide_time: needs the GPU (a time taken elsewhere says nothing)")
    import pyoracle
    wl = synth.WORKLOADS["c4"]
    bs, k, al, be = wl["bs"], wl["k"], wl["alpha"], wl["beta"]
    src, dst, ts, eidx = synth.power_law_stream(wl["n_nodes"], a.edges, bipartite=wl["bipartite"], seed=2020, perm_seed=7)
    neg = synth.negatives(dst, a.edges, seed=2021)
    nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    csr = pyoracle.CsrOracle(src, dst, eidx, ts, nf.num_nodes)
    q = np.concatenate([src[-bs:], dst[-bs:], neg[-bs:]]).astype(np.int32)
    qt = np.concatenate([ts[-bs:]] * 3)
    dev = torch.device("cuda")
    q_d, qt_d = torch.from_numpy(q).to(dev), torch.from_numpy(qt).to(dev)
    M, n = len(al), len(q)
    for shape in a.shapes.split(","):
        width, depth = (int(x) for x in shape.split("x"))
        plan = nf.reserve_pruning(width, depth, M, k, a.max_bytes)
        outs = [torch.zeros((M, n, k), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32, torch.float32)]
        times = []
        for it in range(a.warmup + a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nf.pruned_topk_multi_device(q_d, qt_d, width, depth, al, be, k, *outs, check_status=False)
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        refs = [[np.zeros((n, k), dt) for dt in (np.int32, np.int32, np.float32, np.float32)] for _ in range(M)]
        for m in range(M):                                          # (the oracle walks once per model)
            csr.get_pruned_topk(q, qt, width, depth, al[m], be[m], k, *refs[m])
        t_oracle = time.perf_counter() - t0
        same = all(np.array_equal(o[m].cpu().numpy(), r) for m in range(M) for o, r in zip(outs, refs[m]))
        print(json.dumps(dict(shape=shape, states=plan["states"], form=plan["form"], slabs=plan["slabs"],
                              slab_bytes=plan["slab_bytes"], queries=n, k=k, models=M,
                              gpu_ms_median=round(1e3 * float(np.median(times)), 3),
                              gpu_ms_min=round(1e3 * min(times), 3), gpu_ms_max=round(1e3 * max(times), 3),
                              oracle_s=round(t_oracle, 3), equal_to_oracle=bool(same))), flush=True)


if __name__ == "__main__":
    main()
