"""The training step of bench.py's c2_train leg with its tail on torch and on the HIP kernels of csrc/train_tail.hip:

  --tail torch : crit(pos.squeeze(), ones) + crit(neg.squeeze(), zeros) with torch.nn.BCELoss and torch.optim.Adam -- the
                 step bench.run_train_workload times, line for line
  --tail hip   : TGN.compute_edge_loss (the scorer's [2B] vector straight into _HipLinkBCE) and zebra_amd.Adam (one
                 zt_adam_step per step)

on the same model, stream and warm state (bench.build_model / bench.make_stream, the first 10 % of C2's stream as eval steps
through the native loop), each leg in a PROCESS OF ITS OWN: without --tail this script starts `--repeats` processes per
leg, alternating torch, hip, torch, hip, ..., and prints one JSON line per process and a summary with the median ms per step
of each leg and the spread between its processes.  Inside a process the timed steps come in `--rounds` windows of `--steps`
steps, each between two device synchronisations.

Launches per step are counted on the host by wrapping every zt_* entry point that takes a stream (calls, not kernels: an
entry point may launch several kernels); torch's own launches are not visible from here -- for those, and for GPU time:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/train_tail_time.py --tail hip --rounds 1 --steps 50

    python tools/train_tail_time.py [--repeats 3] [--rounds 5] [--steps 40] [--warmup 10]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def count_zt_calls(lib, names):
    """[n]: calls of the library's entry points from here on (the ctypes handle's attributes are wrapped)"""
    calls = [0]

    def wrap(fn):
        def counted(*args):
            calls[0] += 1
            return fn(*args)
        return counted

    for nm in names:
        if nm.endswith(("_bytes", "_plan", "_offset")) or nm in ("zt_last_error", "zt_version"):
            continue
        setattr(lib, nm, wrap(getattr(lib, nm)))
    return calls


def run_leg(a):
    import numpy as np
    import torch

    import bench
    import zebra_amd
    from zebra_amd import _capi, synth

    device = torch.device("cuda")
    wl = dict(synth.WORKLOADS["c2"])
    bs, F = wl["bs"], wl["F"]
    prefill = (wl["n_edges"] // 10) // bs
    n_timed = a.rounds * a.steps
    n_total = prefill + a.warmup + n_timed
    src, dst, neg, ts, eidx = bench.make_stream(wl, n_total * bs)
    tgn = bench.build_model(wl, device, (wl["n_edges"] if F == 1 else n_total * bs) + 1)
    d = [torch.from_numpy(x[:prefill * bs]).to(device) for x in (src, dst, neg, ts, eidx)]
    tppr_cus, group = synth.pipeline_settings(wl, prefill)
    tgn.enable_pipeline(tppr_cus=tppr_cus, group=group)
    bt = [tuple(x[b * bs:(b + 1) * bs] for x in d) for b in range(prefill)]
    with torch.cuda.stream(tgn.main_stream):
        tgn.run_device(tgn.prepare_run(bt), look=synth.pipeline_look(group))
    torch.cuda.synchronize()
    tgn.embedding_module.tppr_finder.check_status()
    tgn.enable_pipeline(False)
    del d, bt
    tgn.train()
    hip = a.tail == "hip"
    opt = (zebra_amd.Adam if hip else torch.optim.Adam)(tgn.parameters(), lr=1e-4)      # train.py:29,150
    crit = torch.nn.BCELoss()
    ones, zeros = torch.ones(bs, device=device), torch.zeros(bs, device=device)

    def step(b):
        s_, e_ = b * bs, (b + 1) * bs
        opt.zero_grad()
        if hip:
            loss, _, _ = tgn.compute_edge_loss(src[s_:e_], dst[s_:e_], neg[s_:e_], ts[s_:e_], eidx[s_:e_], 10)
        else:
            pos, negp = tgn.compute_edge_probabilities(src[s_:e_], dst[s_:e_], neg[s_:e_], ts[s_:e_], eidx[s_:e_], 10, True)
            loss = crit(pos.squeeze(), ones) + crit(negp.squeeze(), zeros)
        loss.backward()
        opt.step()
        tgn.memory.detach_memory()
        return loss

    b = prefill
    for _ in range(a.warmup):
        step(b)
        b += 1
    calls = count_zt_calls(_capi.lib(), _capi.SYMBOLS)
    ms, losses = [], []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            losses.append(step(b))
            b += 1
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / a.steps)
    tgn.embedding_module.tppr_finder.check_status()
    out = dict(tail=a.tail, steps=a.steps, rounds=a.rounds, warmup=a.warmup, ms_per_step_rounds=[round(x, 4) for x in ms],
               ms_per_step_median=round(float(np.median(ms)), 4), ms_per_step_min=round(float(np.min(ms)), 4),
               zt_calls_per_step=round(calls[0] / n_timed, 2), loss_first=round(float(losses[0].item()), 6),
               loss_last=round(float(losses[-1].item()), 6))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tail", default="", choices=["", "torch", "hip"], help="one leg in this process (default: both, in child processes)")
    ap.add_argument("--repeats", type=int, default=3, help="processes per leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds a child process may take")
    a = ap.parse_args()
    if a.tail:
        run_leg(a)
        return
    import numpy as np
    res = {"torch": [], "hip": []}
    for r in range(a.repeats):
        for tail in (("torch", "hip") if r % 2 == 0 else ("hip", "torch")):
            cmd = [sys.executable, os.path.abspath(__file__), "--tail", tail, "--rounds", str(a.rounds), "--steps", str(a.steps),
                   "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            res[tail].append(json.loads(line))
    summ = {}
    for tail, rs in res.items():
        med = [x["ms_per_step_median"] for x in rs]
        summ[tail] = dict(ms_per_step_median=round(float(np.median(med)), 4), processes=[round(x, 4) for x in med],
                          spread_ms=round(float(max(med) - min(med)), 4),
                          rounds_min=round(min(min(x["ms_per_step_rounds"]) for x in rs), 4),
                          rounds_max=round(max(max(x["ms_per_step_rounds"]) for x in rs), 4),
                          zt_calls_per_step=rs[0]["zt_calls_per_step"])
    summ["hip_over_torch"] = round(summ["hip"]["ms_per_step_median"] / summ["torch"]["ms_per_step_median"], 4)
    print(json.dumps({"summary": summ}), flush=True)


if __name__ == "__main__":
    main()
