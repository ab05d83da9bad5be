"""Runs the workspace form of the pruning query (k_pruned_topk_ws, csrc/tppr_prune.hip) as host code against the CPU oracle
(tools/exp/prune_ws_emu.cpp has the how and the limits).  Needs g++ with C++20; no GPU.

    python tools/exp/prune_ws_emu.py [--queries 4]

Cases: the shapes of tests/test_prune_wide_gpu.py on its hub stream, with one to three models, k = 20 / 100 / 255, one to five
slabs (slab reuse; slabs start out filled with garbage), rows left untouched or zero-filled, and an id out of range.
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402

import inputs as I  # noqa: E402
import pyoracle  # noqa: E402

DT = (np.int32, np.int32, np.float32, np.float32)


def kernel_body():
    """the device code the kernel needs beyond csrc/prune_walk.hpp, cut out of the sources"""
    src = open(os.path.join(ROOT, "zebra_amd", "csrc", "tppr_prune.hip")).read()
    ns = open(os.path.join(ROOT, "zebra_amd", "csrc", "numba_sort.hpp")).read()
    cut = lambda s, a, b: s[s.index(a):s.index(b)]
    return (cut(ns, "__device__ __forceinline__ bool lt_f", "// LDS scratch of the wave-parallel sort") +
            cut(src, "struct WsLds {", "}  // namespace\n\nstatic int csr_upload"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4, help="edges whose src, dst and neg are queried, per case")
    a = ap.parse_args()
    pyoracle.lib()
    src, dst, neg, ts, eidx = I.make_stream("hub", 400, 24000, 305)
    N, E = int(max(src.max(), dst.max())) + 1, len(src)
    csr = pyoracle.CsrOracle(src, dst, eidx, ts, N)
    # the adjacency as zt_csr_build lays it out: both directions per edge in stream order, stably sorted by time per node
    node2 = np.empty(2 * E, np.int64); node2[0::2] = src; node2[1::2] = dst
    oth2 = np.empty(2 * E, np.int32); oth2[0::2] = dst; oth2[1::2] = src
    e2, t2 = np.repeat(eidx, 2).astype(np.int32), np.repeat(ts, 2)
    order = np.lexsort((np.arange(2 * E), t2, node2))
    indptr = np.zeros(N + 1, np.int64); np.add.at(indptr, node2 + 1, 1)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "kernel_body.inc"), "w").write(kernel_body())
        subprocess.run(["g++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", d,
                        "-I", os.path.join(ROOT, "zebra_amd", "csrc"),
                        os.path.join(ROOT, "tools", "exp", "prune_ws_emu.cpp"), "-o", os.path.join(d, "emu")], check=True)
        w = lambda name, arr: arr.tofile(os.path.join(d, name + ".bin"))
        w("indptr", np.cumsum(indptr).astype(np.int64)); w("nbr", oth2[order]); w("eid", e2[order]); w("ts", t2[order])
        n = a.queries
        bad = 0
        # (width, depth, k, models, zero_empty, slabs, early queries too, an id out of range)
        for width, depth, k, models, ze, slabs, early, oob in (
                (36, 2, 20, [(0.1, 0.5)], 0, 2, True, False), (36, 2, 20, [(0.1, 0.95)], 0, 3, True, False),
                (11, 3, 20, [(0.1, 0.5), (0.1, 0.95)], 0, 1, True, True), (11, 3, 20, [(0.1, 0.5), (0.1, 0.95)], 1, 2, True, True),
                (20, 3, 20, [(0.1, 0.5)], 0, 2, True, False), (20, 3, 100, [(0.1, 0.95), (0.2, 0.7), (0.0, 0.5)], 1, 2, True, False),
                (20, 3, 255, [(0.1, 0.5)], 0, 2, False, False), (6, 5, 20, [(0.1, 0.5), (0.3, 0.9)], 0, 1, False, False),
                (3000, 1, 255, [(0.1, 0.5), (0.1, 0.95)], 0, 2, True, False), (3000, 1, 20, [(0.1, 0.95)], 1, 5, True, False),
                (1281, 1, 20, [(0.1, 0.5)], 0, 2, False, False)):
            q = np.concatenate([src[-n:], dst[-n:], neg[-n:]]).astype(np.int32)
            qt = np.concatenate([ts[-n:]] * 3)
            if early:
                q = np.concatenate([q, src[[0, 4, 49]], [0]]).astype(np.int32)
                qt = np.concatenate([qt, ts[[0, 4, 49]], [ts[0]]])
            fill = 0 if ze else 7
            exp = [[], [], [], []]
            for al, be in models:
                o = [np.full((len(q), k), fill, dt) for dt in DT]
                csr.get_pruned_topk(q, qt, width, depth, al, be, k, *o)
                for x, y in zip(exp, o):
                    x.append(np.insert(y, 2, fill, axis=0) if oob else y)     # the bad row: untouched / zeros
            if oob:
                q, qt = np.insert(q, 2, N + 5).astype(np.int32), np.insert(qt, 2, qt[0])
            w("q", q); w("qt", qt); w("ab", np.array(models, np.float64).ravel())
            for nm, x in zip("nedw", exp):
                w("exp_" + nm, np.stack(x))
            r = subprocess.run([os.path.join(d, "emu"), str(width), str(depth), str(k), str(len(models)), str(ze), "7",
                                str(slabs)], cwd=d, capture_output=True, text=True)
            print(r.stdout.strip(), r.stderr.strip()[:200], flush=True)
            want_status = "status -2" if oob else "status 0"
            bad += r.returncode != 0 or want_status not in r.stdout
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
