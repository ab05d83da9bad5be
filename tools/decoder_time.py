"""The node-classification decoder (zebra_amd/decoder.py MLP): the HIP kernels of csrc/decoder.hip, in both arrangements of a
16-row tile (one wave per tile / five waves per tile, pinned through the test hook zt_test_decoder_arrangement), against
torch's composition (fused_decoder=False), in ONE process on one GPU.  Per shape NxH -- defaults: C2's batch 200x300, 600x300,
C5's batch 4096x300, D = 172 with two T-PPR models 200x516 -- two measurements:

  eval    decoder.predict(x): probabilities from the embeddings
  train   label_bce_loss(decoder(x).sigmoid(), labels).backward(): forward, loss and backward to the six parameters (the
          embeddings need no gradient: the TGN is frozen), dropout 0.3

The modes alternate round by round after a warm-up; a round is `--iters` calls between two device synchronisations.  Prints
one JSON line per shape: per measurement and mode the median and the minimum microseconds per call over `--rounds` rounds, and
the mode's spread against ITSELF -- |median of its even rounds - median of its odd rounds| / median -- which is what a
difference between two modes has to exceed to mean anything.

GPU time and launch count come from a run of its own under the profiler, one mode and one measurement at a time:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/decoder_time.py --only five --what train --shapes 200x300 --rounds 1 --iters 100 --warmup 0

(kernel calls / iters = launches per call; sum of the kernels' time / iters = GPU time.)

    python tools/decoder_time.py [--shapes 200x300,600x300,4096x300,200x516] [--rounds 30] [--iters 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from zebra_amd import _capi  # noqa: E402
from zebra_amd.decoder import MLP, decoder_plan  # noqa: E402
from zebra_amd.losses import label_bce_loss  # noqa: E402

MODES = ("one", "five", "torch")
PIN = {"one": _capi.DECODER_ARR_ONE, "five": _capi.DECODER_ARR_FIVE, "torch": 0}


def make_case(N, H, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * H + N)
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    dec = MLP(H, drop=0.3).to(dev)
    x = (torch.randn((N, H), generator=g) * 0.5).to(dev)
    labels = (torch.rand(N, generator=g) < 0.3).float().to(dev)
    assert decoder_plan("cuda", torch.float32, H) == "hip", "no HIP decoder for H=%d" % H
    return dec, x, labels


def set_mode(dec, mode):
    dec.fused_decoder = mode != "torch"
    _capi.check(_capi.hooks_lib().zt_test_decoder_arrangement(C.c_int32(PIN[mode])), "zt_test_decoder_arrangement")


def run(dec, x, labels, what, iters):
    if what == "eval":
        dec.eval()
        for _ in range(iters):
            dec.predict(x)
        return
    dec.train()
    for _ in range(iters):
        for p in dec.parameters():
            p.grad = None
        label_bce_loss(dec(x).sigmoid(), labels).backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200x300,600x300,4096x300,200x516")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", choices=("",) + MODES, help="one mode alone (a profiler run)")
    ap.add_argument("--what", default="", choices=["", "eval", "train"], help="one measurement alone")
    a = ap.parse_args()
    modes = [a.only] if a.only else list(MODES)
    whats = [a.what] if a.what else ["eval", "train"]
    try:
        for shape in a.shapes.split(","):
            N, H = [int(v) for v in shape.lower().split("x")]
            dec, x, labels = make_case(N, H)
            out = dict(N=N, H=H, rounds=a.rounds, iters=a.iters)
            for what in whats:
                us = {m: [] for m in modes}
                for r in range(a.warmup + a.rounds):
                    for m in (modes if r % 2 == 0 else modes[::-1]):      # the order alternates too
                        set_mode(dec, m)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        run(dec, x, labels, what, a.iters)
                        torch.cuda.synchronize()
                        if r >= a.warmup:
                            us[m].append(1e6 * (time.perf_counter() - t0) / a.iters)
                for m in modes:
                    v = np.asarray(us[m])
                    med = float(np.median(v))
                    out["%s_%s_us_median" % (what, m)] = round(med, 2)
                    out["%s_%s_us_min" % (what, m)] = round(float(v.min()), 2)
                    if len(v) >= 2:
                        out["%s_%s_spread" % (what, m)] = round(abs(float(np.median(v[0::2])) - float(np.median(v[1::2]))) / med, 4)
            print(json.dumps(out), flush=True)
    finally:
        _capi.hooks_lib().zt_test_decoder_arrangement(C.c_int32(0))


if __name__ == "__main__":
    main()
