"""What the metrics tail of the native step costs and what a native validation pass saves (zt_pipeline_set_metrics,
TGN.enable_metrics, evaluation.eval_edge_prediction(native=True)), in ONE process on one GPU.  Three measurements:

  tail    per workload (defaults: bench.py's C2, bs = 200, and C5, bs = 4096): ms per step of TGN.run_device with the scorer
          only and with the scorer and the metrics tail, over consecutive segments of `--steps` batches of one stream on one
          model, after `--prefill` batches; the two modes alternate segment by segment, the order alternates round by round.
          The yardstick of the tail is the scoring-only run of the same build.
  pass    per workload: eval_edge_prediction over the same `--eval-batches` batches with native=False (a Python iteration,
          a staging copy, a host synchronisation and a metrics launch per batch) and with native=True (one staging copy, one
          native call, one read), each on a fresh model brought to the same state by the same prefill; seconds per pass and
          the three means of both (they must agree).
  kernel  the metrics kernel alone at B = 200, 4096, 8192 (the single sort of 64-bit words) and 16384 (the two-run form):
          microseconds per call, median over `--rounds` rounds of `--iters` calls between two events.

If `tail` lengthens a step by more than the kernel's stand-alone time at that batch size, the kernel is not running beside the
next step as intended: look at the kernel trace (rocprofv3 --kernel-trace -- python tools/metrics_run_time.py --only tail).
Prints one JSON line per measurement and a summary line ("Scoring and metrics").

    python tools/metrics_run_time.py [--workloads c2,c5] [--only tail,pass,kernel] [--rounds 3] [--steps 100] [--prefill 20]
                                     [--eval-batches 100] [--iters 20]
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
from zebra_amd import _capi, synth  # noqa: E402
from zebra_amd import evaluation as ev  # noqa: E402

KERNEL_BATCHES = (200, 4096, 8192, 16384)
FORMS = {_capi.METRICS_FORM_SINGLE: "single", _capi.METRICS_FORM_SPLIT: "split"}


class Sampler:
    """RandEdgeSampler's interface (utils/util.py:54-84): uniform over the observed destinations"""

    def __init__(self, dsts, seed):
        self.seed, self.dst_list = seed, np.unique(dsts)
        self.random_state = np.random.RandomState(seed)

    def reset_random_state(self):
        self.random_state = np.random.RandomState(self.seed)

    def sample(self, size):
        i = self.random_state.randint(0, len(self.dst_list), size)
        return self.dst_list[i], self.dst_list[self.random_state.randint(0, len(self.dst_list), size)]


def make_model(name, n_batches):
    """bench.py's model and stream of workload `name` with the pipeline of synth.pipeline_settings and the scorer on"""
    wl = dict(synth.WORKLOADS[name])
    bs, F = wl["bs"], wl["F"]
    stream = bench.make_stream(wl, n_batches * bs)
    dev = torch.device("cuda")
    tgn = bench.build_model(wl, dev, (wl["n_edges"] if F == 1 else n_batches * bs) + 1)
    tppr_cus, group = synth.pipeline_settings(wl, n_batches)
    tgn.enable_pipeline(tppr_cus=tppr_cus, group=group)
    tgn.enable_scoring()
    return wl, tgn, stream, synth.pipeline_look(group)


def drop(tgn):
    tgn.enable_pipeline(False)
    del tgn
    torch.cuda.empty_cache()


def tail_ms(name, rounds, steps, prefill):
    n = prefill + 2 * rounds * steps
    wl, tgn, stream, look = make_model(name, n)
    bs = wl["bs"]
    d = [torch.from_numpy(x).to(tgn.device) for x in stream]
    bt = [tuple(x[b * bs:(b + 1) * bs] for x in d) for b in range(n)]
    ms = {"scoring": [], "metrics": []}
    with torch.cuda.stream(tgn.main_stream):
        tgn.run_device(tgn.prepare_run(bt[:prefill]), look=look)
        torch.cuda.synchronize()
        at = prefill
        for r in range(rounds):
            for mode in (("scoring", "metrics") if r % 2 == 0 else ("metrics", "scoring")):
                tgn.enable_metrics(mode == "metrics")
                prepared = tgn.prepare_run(bt[at:at + steps])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tgn.run_device(prepared, look=look)
                torch.cuda.synchronize()
                ms[mode].append(1e3 * (time.perf_counter() - t0) / steps)
                at += steps
                if mode == "metrics":
                    assert tgn.metrics()[1] == steps
    tgn.check_status()
    drop(tgn)
    return {k: round(float(np.median(v)), 4) for k, v in ms.items()}


def pass_s(name, prefill, eval_batches):
    out = {}
    for native in (False, True):
        n = prefill + eval_batches
        wl, tgn, stream, look = make_model(name, n)
        bs = wl["bs"]
        src, dst, neg, ts, eidx = stream
        d = [torch.from_numpy(x[:prefill * bs]).to(tgn.device) for x in stream]
        bt = [tuple(x[b * bs:(b + 1) * bs] for x in d) for b in range(prefill)]
        with torch.cuda.stream(tgn.main_stream):
            tgn.run_device(tgn.prepare_run(bt), look=look)
        torch.cuda.synchronize()
        s0 = prefill * bs
        data = types.SimpleNamespace(sources=src[s0:], destinations=dst[s0:], timestamps=ts[s0:], edge_idxs=eidx[s0:],
                                     n_interactions=eval_batches * bs)
        t0 = time.perf_counter()
        got = ev.eval_edge_prediction(tgn, Sampler(dst, 7), data, wl.get("width", 10), bs, native=native)
        torch.cuda.synchronize()
        out["native" if native else "stepwise"] = dict(seconds=round(time.perf_counter() - t0, 4), means=got)
        drop(tgn)
    out["max_abs_diff_of_means"] = float(np.abs(np.asarray(out["native"]["means"]) - np.asarray(out["stepwise"]["means"])).max())
    out["stepwise_over_native"] = round(out["stepwise"]["seconds"] / out["native"]["seconds"], 3)
    return out


def kernel_us(B, rounds, iters):
    rng = np.random.RandomState(B)
    p = torch.from_numpy(np.clip(rng.normal(0.65, 0.2, B), 0, 1).astype(np.float32)).cuda()
    n = torch.from_numpy(np.clip(rng.normal(0.4, 0.2, B), 0, 1).astype(np.float32)).cuda()
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    us = []
    for r in range(rounds + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            ev.link_metrics(p, n, out=acc)
        t1.record()
        t1.synchronize()
        if r > 0:                                  # (round 0 warms up)
            us.append(1e3 * t0.elapsed_time(t1) / iters)
    return dict(B=B, form=FORMS[_capi.link_metrics_plan(B)["form"]], us=round(float(np.median(us)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c5")
    ap.add_argument("--only", default="tail,pass,kernel")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--prefill", type=int, default=20)
    ap.add_argument("--eval-batches", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    only = a.only.split(",")
    summary = dict(tool="metrics_run_time", device=torch.cuda.get_device_name(0), rounds=a.rounds, steps=a.steps)
    if "kernel" in only:
        summary["kernel"] = [kernel_us(B, a.rounds, a.iters) for B in KERNEL_BATCHES]
        print(json.dumps(dict(kernel=summary["kernel"])), flush=True)
    for name in [w for w in a.workloads.split(",") if w]:
        if "tail" in only:
            r = tail_ms(name, a.rounds, a.steps, a.prefill)
            r["tail_us_per_step"] = round(1e3 * (r["metrics"] - r["scoring"]), 2)
            summary.setdefault("tail_ms_per_step", {})[name] = r
            print(json.dumps(dict(workload=name, tail_ms_per_step=r)), flush=True)
        if "pass" in only:
            r = pass_s(name, a.prefill, a.eval_batches)
            summary.setdefault("pass", {})[name] = r
            print(json.dumps(dict(workload=name, **{"pass": r})), flush=True)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
