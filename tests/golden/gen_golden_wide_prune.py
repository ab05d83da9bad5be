#!/usr/bin/env python3
"""Generate the wide pruning-walk fixtures tests/golden/g13_prune_*.npz from the reference itself.

The reference bounds neither --n_degree (the walk's width) nor --n_layer (its depth), train.py:25,28: its
NeighborFinder.get_pruned_topk (utils/util.py:185-276) walks width + width^2 + ... + width^depth states per query.  The
two cases below are the smallest walks beyond the LDS form of the pruning query (more than 1 280 states), so they take the
workspace form.  Like gen_golden.py this runs only where the reference is present: it imports the reference's Python
source unmodified under oracle/numba_standin (through gen_golden's setup).  Only the resulting data is committed.

    python tests/golden/gen_golden_wide_prune.py [--check]

  g13_prune_w36d2_k20.npz, g13_prune_w11d3_k20.npz    the layout of g3_prune_*: q_nodes, q_ts, the four outputs
                                                      (nodes, eidx, dt, w), probe and the probed adjacencies

The cases have a table of their own: tests/test_tppr_gpu.py::test_pruning_golden iterates inputs.PRUNE_CASES on a finder
that holds no workspace.  --check regenerates in memory and compares with the committed files.
"""
import argparse
import os
import sys
import types

import numpy as np

import gen_golden as G          # (sets up the import of the reference under oracle/numba_standin)

I = G.I
U = G.U
HERE = G.HERE
# name -> (kind, n_nodes, n_edges, seed, n_queries, width, depth, k, alpha, beta); beta = 0.5 makes exact ties at the cut
WIDE_PRUNE_CASES = {
    "w36d2_k20": ("hub", 400, 24000, 305, 24, 36, 2, 20, 0.1, 0.5),
    "w11d3_k20": ("hub", 400, 24000, 305, 24, 11, 3, 20, 0.1, 0.5),
}
OUT = {}


def queries(src, dst, neg, ts, nq):
    """src, dst and neg of the last nq / 3 edges, at those edges' times"""
    n = nq // 3
    return (np.concatenate([src[-n:], dst[-n:], neg[-n:]]).astype(np.int32),
            np.concatenate([ts[-n:]] * 3).astype(np.float64))


def gen(name):
    kind, N, E, seed, nq, width, depth, k, alpha, beta = WIDE_PRUNE_CASES[name]
    src, dst, neg, ts, eidx = I.make_stream(kind, N, E, seed)
    nf = U.get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    qn, qt = queries(src, dst, neg, ts, nq)
    qn = np.minimum(qn, len(nf.node_to_neighbors) - 1).astype(np.int32)   # beyond the adjacency: IndexError in the reference
    on = np.zeros((nq, k), np.int32)
    oe = np.zeros((nq, k), np.int32)
    od = np.zeros((nq, k), np.float32)
    ow = np.zeros((nq, k), np.float32)
    nf.get_pruned_topk(qn, qt, width, depth, alpha, beta, k, on, oe, od, ow)
    probe = np.unique(qn)[:4]
    adj = {}
    for v in probe:
        adj["adj%d_nbr" % v] = nf.node_to_neighbors[v]
        adj["adj%d_eid" % v] = nf.node_to_edge_idxs[v]
        adj["adj%d_ts" % v] = nf.node_to_edge_timestamps[v]
    OUT["g13_prune_" + name] = dict(q_nodes=qn, q_ts=qt, nodes=on, eidx=oe, dt=od, w=ow, probe=probe, **adj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    for name in WIDE_PRUNE_CASES:
        gen(name)
    bad = 0
    for name, arrays in OUT.items():
        path = os.path.join(HERE, name + ".npz")
        if a.check:
            old = np.load(path)
            if sorted(old.files) != sorted(arrays):
                print("MISMATCH", name, "keys")
                bad += 1
            for kk, v in arrays.items():
                if kk not in old.files or not np.array_equal(old[kk], np.asarray(v)):
                    print("MISMATCH", name, kk)
                    bad += 1
        else:
            np.savez_compressed(path, **arrays)
            print("%-32s %7.1f KB" % (name, os.path.getsize(path) / 1024))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
