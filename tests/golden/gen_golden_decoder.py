#!/usr/bin/env python3
"""Generate the node-classification decoder fixture tests/golden/g14_node_decoder.npz from the reference itself.

The reference's decoder is MLP (utils/util.py:28-42): fc_1 dim -> 80, fc_2 80 -> 10, fc_3 10 -> 1, ReLU, dropout.  Like
gen_golden.py this runs only where the reference is present: it imports the reference's Python source unmodified (through
gen_golden's setup) and runs its MLP in float64 on seeded inputs.  Only the resulting data is committed.

    python tests/golden/gen_golden_decoder.py [--check]

Per case (dim = 40 and dim = 300, N = 37), keys prefixed "d<dim>_":
  keys, shapes        the reference MLP's state-dict keys and the shape of each
  fc_1.weight, ...    the parameters (float64: torch's default initialisation drawn in float32 from the case's seed)
  x, labels           the inputs [N][dim] (0.5 N(0, 1)) and a 0 / 1 label per row
  logits              eval mode
  loss, g_<key>, d_x  with drop = 0.0 in train mode: BCELoss(sigmoid(logits), labels), its gradient for each of the six
                      parameters and for x

--check regenerates in memory and compares with the committed file.
"""
import argparse
import os
import sys

import numpy as np
import torch

import gen_golden as G          # (sets up the import of the reference)

MLP = G.U.MLP
HERE = G.HERE
N = 37
DIMS = (40, 300)
NAME = "g14_node_decoder"


def gen_case(dim, out):
    torch.manual_seed(1400 + dim)
    rng = np.random.RandomState(1400 + dim)
    pre = "d%d_" % dim
    ref = MLP(dim, drop=0.3)
    sd = ref.state_dict()
    out[pre + "keys"] = np.array(list(sd.keys()))
    out[pre + "shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], np.int64)
    ref = ref.double()
    for k, v in ref.state_dict().items():
        out[pre + k] = v.numpy().copy()
    x = 0.5 * rng.randn(N, dim)
    labels = (rng.rand(N) < 0.4).astype(np.float64)
    assert 0 < labels.sum() < N
    out[pre + "x"], out[pre + "labels"] = x, labels
    ref.eval()
    with torch.no_grad():
        out[pre + "logits"] = ref(torch.from_numpy(x)).numpy().copy()
    tr = MLP(dim, drop=0.0).double()
    tr.load_state_dict(ref.state_dict())
    tr.train()
    xt = torch.from_numpy(x).requires_grad_(True)
    loss = torch.nn.BCELoss()(tr(xt).sigmoid(), torch.from_numpy(labels))
    loss.backward()
    out[pre + "loss"] = np.float64(loss.item())
    for k, p in tr.named_parameters():
        out[pre + "g_" + k] = p.grad.numpy().copy()
    out[pre + "d_x"] = xt.grad.numpy().copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    arrays = {}
    for dim in DIMS:
        gen_case(dim, arrays)
    path = os.path.join(HERE, NAME + ".npz")
    bad = 0
    if a.check:
        old = np.load(path)
        if sorted(old.files) != sorted(arrays):
            print("MISMATCH", NAME, "keys")
            bad += 1
        for kk, v in arrays.items():
            if kk not in old.files or not np.array_equal(old[kk], np.asarray(v)):
                print("MISMATCH", NAME, kk)
                bad += 1
    else:
        np.savez_compressed(path, **arrays)
        print("%-32s %7.1f KB" % (NAME, os.path.getsize(path) / 1024))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
