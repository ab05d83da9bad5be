"""Step time with the RNN memory updater against the GRU (RNNMemoryUpdater, zt_rnn_update).  For each cell, in alternating
rounds on one GPU:
  c2, c5    : ms per eval step of the bench's C2 / C5 workloads through the native batch loop (zt_pipeline_run), from a
              state the first `--prefill` batches have filled
  c2_train  : ms per training step of bench.py's c2_train leg (bench.run_train_workload, host baseline off)
The model is bench.py's, with its memory updater swapped for an RNNMemoryUpdater of the same widths where the cell is
rnn.  Prints one JSON line per (round, cell, shape) and a summary line with the medians.  The memory kernel's own time
comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/rnn_step_time.py --shapes c2 ...`
(k_gru<0> / k_out_gru* against their <1, ...> instantiations).

    python tools/rnn_step_time.py [--shapes c2,c5,c2_train] [--cells gru,rnn] [--rounds 2] [--steps 50] [--warmup 5]
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

import bench  # noqa: E402
from zebra_amd import synth  # noqa: E402
from zebra_amd.modules import RNNMemoryUpdater  # noqa: E402

_build_model = bench.build_model


def build_model(cell):
    def build(wl, device, n_edge_rows):
        tgn = _build_model(wl, device, n_edge_rows)
        if cell == "rnn":
            g = tgn.memory_updater
            torch.manual_seed(1)
            tgn.memory_updater = RNNMemoryUpdater(g.message_dimension, g.memory_updater.hidden_size, device).to(device)
        return tgn
    return build


def eval_ms(name, cell, steps, warmup, prefill):
    wl = dict(synth.WORKLOADS[name])
    bs, F = wl["bs"], wl["F"]
    n = prefill + warmup + steps
    src, dst, neg, ts, eidx = bench.make_stream(wl, n * bs)
    dev = torch.device("cuda")
    tgn = build_model(cell)(wl, dev, (wl["n_edges"] if F == 1 else n * bs) + 1)
    tppr_cus, group = synth.pipeline_settings(wl, steps)
    tgn.enable_pipeline(tppr_cus=tppr_cus, group=group)
    d = [torch.from_numpy(x).to(dev) for x in (src, dst, neg, ts, eidx)]
    bt = [tuple(x[b * bs:(b + 1) * bs] for x in d) for b in range(n)]
    look = synth.pipeline_look(group)
    with torch.cuda.stream(tgn.main_stream):
        tgn.run_device(tgn.prepare_run(bt[:prefill + warmup]), look=look)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tgn.run_device(tgn.prepare_run(bt[prefill + warmup:]), look=look)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    tgn.embedding_module.tppr_finder.check_status()
    tgn.enable_pipeline(False)
    del tgn, d, bt
    torch.cuda.empty_cache()
    return 1e3 * dt / steps


def train_ms(cell, steps, warmup):
    bench.build_model = build_model(cell)
    try:
        r = bench.run_train_workload(types.SimpleNamespace(perm_seed=-1, cpu_edges=0), "c2_train", steps, warmup,
                                     torch.device("cuda"))
    finally:
        bench.build_model = _build_model
    torch.cuda.empty_cache()
    return r["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c5,c2_train")
    ap.add_argument("--cells", default="gru,rnn")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prefill", type=int, default=20)
    a = ap.parse_args()
    res = {}
    for r in range(a.rounds):
        for cell in a.cells.split(","):
            for shape in a.shapes.split(","):
                ms = train_ms(cell, a.steps, a.warmup) if shape == "c2_train" else eval_ms(shape, cell, a.steps, a.warmup, a.prefill)
                res.setdefault((cell, shape), []).append(ms)
                print(json.dumps(dict(round=r, cell=cell, shape=shape, ms_per_step=round(ms, 4))), flush=True)
    print(json.dumps({"median_ms_per_step": {"%s/%s" % k: round(float(np.median(v)), 4) for k, v in res.items()}}))


if __name__ == "__main__":
    main()
