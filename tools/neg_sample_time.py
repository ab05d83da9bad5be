"""Negative sampling (csrc/neg_sample.hip) against the clock, in ONE process on one GPU:

  device  zebra_amd.sampling.NegativeSampler.sample_for -- zt_csr_seen_ranges and zt_neg_sample -- on inputs that are on the
          device already, "mixed" strategy, distinct, without the source, filtered;
  numpy   a host sampler that applies the same exclusions with python sets: per row, uniform draws from the pool (and, for the
          historical half, from the row's history) until the row is full or four passes are over.  Not the same draws: a
          yardstick for what the exclusions cost on the host, where today's callers would have to apply them.

at (B, K) = (200, 100), (200, 1000), and (200, 100) with a hub source whose history holds 10^6 entries (every row's source is
the hub: what the list scan of a filtered round costs).  The modes alternate round by round after a warm-up; a round is
`--iters` calls between two events on the stream.  Appends ONE JSON line to `--out`: the median microseconds per call of both
modes over `--rounds` rounds with the spread (min, max) and their ratio.  No threshold: the line reports, it does not judge.

    python tools/neg_sample_time.py [--rounds 10] [--iters 3] [--warmup 2] [--out profiles/r13/neg_sample_time.jsonl]
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

from zebra_amd.sampling import NegativeSampler  # noqa: E402
from zebra_amd.tppr import get_neighbor_finder  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_time import summary, timed  # noqa: E402

SHAPES = [dict(name="B200_K100", B=200, K=100, hub=0), dict(name="B200_K1000", B=200, K=1000, hub=0),
          dict(name="B200_K100_hub1e6", B=200, K=100, hub=10 ** 6)]
N_NODES, N_EDGES = 20000, 200000


def numpy_sampler(pool, indptr, nbr, ats, rng):
    """sample(sources, destinations, timestamps, K) -> int32 [B, K] on the host: the exclusions with python sets"""
    def sample(src, dst, ts, K):
        out = np.full((len(src), K), -1, np.int32)
        sets = {}                                             # one set per distinct history of the call (a hub's is built once)
        for b in range(len(src)):
            lo, hi = indptr[src[b]], indptr[src[b] + 1]
            hist = nbr[lo:lo + np.searchsorted(ats[lo:hi], ts[b])]
            seen = sets.get((int(src[b]), len(hist)))
            if seen is None:
                seen = sets[(int(src[b]), len(hist))] = set(hist.tolist())
            taken = {int(dst[b]), int(src[b])}
            row, want_hist = [], K // 2
            for _ in range(4):
                if len(row) >= K:
                    break
                n_h = max(0, want_hist - len(row)) if len(hist) else 0
                draws = np.concatenate([hist[rng.randint(0, len(hist), n_h)] if n_h else np.zeros(0, np.int32),
                                        pool[rng.randint(0, len(pool), K - len(row) - n_h)]])
                for i, v in enumerate(draws.tolist()):
                    if v in taken or (i >= n_h and v in seen):
                        continue
                    taken.add(v)
                    row.append(v)
            out[b, :len(row)] = row[:K]
        return out
    return sample


def case(shape, seed=0):
    dev = torch.device("cuda")
    rng = np.random.RandomState(seed)
    B, K, hub = shape["B"], shape["K"], shape["hub"]
    src = rng.randint(1, N_NODES, N_EDGES).astype(np.int32)
    dst = rng.randint(1, N_NODES, N_EDGES).astype(np.int32)
    if hub:                                                   # node 1 gets `hub` more edges, to partners all over the pool
        src = np.concatenate([src, np.ones(hub, np.int32)])
        dst = np.concatenate([dst, rng.randint(2, N_NODES, hub).astype(np.int32)])
    E = len(src)
    order = rng.permutation(E)
    data = types.SimpleNamespace(sources=src[order], destinations=dst[order], edge_idxs=np.arange(1, E + 1),
                                 timestamps=np.sort(rng.random_sample(E)))
    nf = get_neighbor_finder(data)
    q_src = np.ones(B, np.int32) if hub else data.sources[-B:]
    q_dst, q_ts = data.destinations[-B:], np.full(B, 2.0)     # (after everything: whole histories)
    smp = NegativeSampler(data.destinations, seed=seed + 1, finder=nf, strategy="mixed", filtered=True)
    src_d, dst_d, ts_d = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (q_src, q_dst, q_ts))
    host = numpy_sampler(smp.dst_list, nf._indptr, nf._nbr, nf._ts, np.random.RandomState(seed + 2))
    fns = {"device": lambda: smp.sample_for(src_d, dst_d, ts_d, K), "numpy": lambda: host(q_src, q_dst, q_ts, K)}
    neg, count = fns["device"]()
    begin, length = nf.seen_ranges_device(src_d, ts_d)
    facts = dict(list_entries_mean=float(length.float().mean()), filled=float((neg >= 0).float().mean()),
                 from_list=float(count[:, 0].float().mean()), numpy_filled=float((fns["numpy"]() >= 0).mean()))
    return fns, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "neg_sample_time.jsonl"))
    a = ap.parse_args()
    out = dict(tool="neg_sample_time", rounds=a.rounds, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               shapes=[])
    for shape in SHAPES:
        fns, facts = case(shape)
        res = dict(shape, **facts, **summary(timed(fns, a.rounds, a.iters, a.warmup)))
        res["device_over_numpy"] = round(res["device"]["median_us"] / res["numpy"]["median_us"], 4)
        out["shapes"].append(res)
        del fns
        torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
