"""The eval link scorer (csrc/scoring.hip through TGN.score_device) form by form against torch's composition of MergeLayer, in
ONE process on one GPU.  For every hidden width H and batch size B of the lists -- defaults: H in 200, 300 (D = 100), 344, 516
(D = 172), 768 (D = 256) and B in 200, 512, 1000, 4096 -- each form zt::affinity_kernel_plan allows at that shape is pinned
through ZT_CHOICE_SCORE (1 latency, 2 tiled: the kernels specialised for H = 200 / 300; 3 generic latency, 4 generic tiled)
and timed beside torch's composition (a concatenation, two GEMMs, ReLU, sigmoid).  The modes alternate round by round after
a warm-up; a round is `--iters` calls between two events on the stream.  Prints ONE JSON line: per shape the median
microseconds per call of every mode over `--rounds` rounds, the library's own pick and the fastest HIP form.

This is where the switches of affinity_kernel_plan come from ("Scoring and metrics").

    python tools/score_eval_time.py [--widths 200,300,344,516,768] [--batches 200,512,1000,4096] [--rounds 20] [--iters 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from zebra_amd import _capi  # noqa: E402
from zebra_amd.modules import MergeLayer  # noqa: E402
from zebra_amd.tgn import TGN  # noqa: E402

FORMS = {1: "latency", 2: "tiled", 3: "generic_latency", 4: "generic_tiled"}


def plan_form(B, H, choice):
    out = (C.c_int64 * 7)()
    _capi.check(_capi.hooks_lib().zt_test_affinity_plan(C.c_int64(B), C.c_int32(H), C.c_int32(choice), out), "zt_test_affinity_plan")
    return int(out[0])


def make_case(B, H, seed=0):
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = MergeLayer(H, H, H, 1).to(dev)
    g = torch.Generator().manual_seed(seed + 1000 * H + B)
    emb = (torch.randn((3 * B, H), generator=g) * 0.7).to(dev)
    holder = types.SimpleNamespace(affinity_score=layer, device=dev)
    holder._affinity_state = types.MethodType(TGN._affinity_state, holder)
    hip = types.MethodType(TGN.score_device, holder)

    @torch.no_grad()
    def composed(e):
        return layer(torch.cat([e[:B], e[:B]]), e[B:]).squeeze(1).sigmoid()

    return emb, hip, composed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="200,300,344,516,768")
    ap.add_argument("--batches", default="200,512,1000,4096")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    shapes = []
    for H in [int(x) for x in a.widths.split(",")]:
        for B in [int(x) for x in a.batches.split(",")]:
            emb, hip, composed = make_case(B, H)
            forms = [f for f in FORMS if plan_form(B, H, f) == f]
            modes = [FORMS[f] for f in forms] + ["torch"]
            us = {m: [] for m in modes}
            ref = composed(emb)
            worst = 0.0
            try:
                for r in range(a.warmup + a.rounds):
                    order = list(zip(forms + [0], modes))
                    for f, m in (order if r % 2 == 0 else order[::-1]):          # the order alternates too
                        if m != "torch":
                            _capi.set_kernel_choice(_capi.CHOICE_SCORE, f)
                        fn = composed if m == "torch" else hip
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        for _ in range(a.iters):
                            out = fn(emb)
                        t1.record()
                        t1.synchronize()
                        if r == 0:
                            worst = max(worst, float((out - ref).abs().max()))
                        if r >= a.warmup:
                            us[m].append(1e3 * t0.elapsed_time(t1) / a.iters)
            finally:
                _capi.set_kernel_choice(_capi.CHOICE_SCORE, 0)
            res = dict(B=B, H=H, pick=FORMS[plan_form(B, H, 0)], max_abs_diff_to_torch=worst)
            for m in modes:
                res[m + "_us"] = round(float(np.median(us[m])), 2)
            res["fastest_hip"] = min((m for m in modes if m != "torch"), key=lambda m: res[m + "_us"])
            res["pick_over_torch"] = round(res[res["pick"] + "_us"] / res["torch_us"], 3)
            shapes.append(res)
    print(json.dumps(dict(tool="score_eval_time", rounds=a.rounds, iters=a.iters, warmup=a.warmup,
                          device=torch.cuda.get_device_name(0), shapes=shapes)), flush=True)


if __name__ == "__main__":
    main()
