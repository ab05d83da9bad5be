"""The full-pool count (csrc/rank_count.hip) against the clock, in ONE process on one GPU:

  count       TGN.count_scores (zt_affinity_count: its GEMMs and the pair kernel, slab by slab) on random embeddings at
              (Q, N, H) = (200, 9 228, 200), (200, 100 000, 300), (200, 1 000 000, 300), thresholds = the probabilities of
              one column per query;
  topk1       TGN.topk_scores at k = 1 -- the same pair sums, plus a running list per wave and the merge;
  topk10      ... at k = 10;
  rank_count  what the library offered before: TGN.rank_scores into prob [Q, N], then evaluation.rank_metrics on [Q, N] -- only
              where prob [Q, N] fits (N <= 100 000 here).

The modes alternate round by round after a warm-up; a round is `--iters` calls between two events on the stream.  Then ONE
pass of evaluation.eval_edge_ranking_full (the whole pool of 9 227 ids per edge) over a synthetic Wikipedia-shaped stream
(workload c1 of zebra_amd.synth: 9 227 nodes, 172 edge features, batches of 200) beside evaluation.eval_edge_ranking with 100
sampled negatives over the same batches, wall-clock milliseconds each.  Prints ONE JSON line and appends it to
profiles/r14/rank_of_time.jsonl.

    python tools/rank_of_time.py [--rounds 10] [--iters 3] [--warmup 2] [--eval-batches 20] [--out FILE]
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

from zebra_amd.modules import MergeLayer  # noqa: E402
from zebra_amd.tgn import TGN  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_time import summary, timed  # noqa: E402

SHAPES = [(200, 9228, 200), (200, 100000, 300), (200, 1000000, 300)]
PROB_FITS = 100000                      # prob [200, N] float32 beyond this is what the count exists to avoid


def count_case(Q, N, H, seed=0):
    from zebra_amd import evaluation as ev
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = MergeLayer(H, H, H, 1).to(dev)
    g = torch.Generator().manual_seed(seed + Q + N)
    emb_q = (torch.randn((Q, H), generator=g) * 0.7).to(dev)
    emb_c = (torch.randn((N, H), generator=g) * 0.7).to(dev)
    holder = types.SimpleNamespace(affinity_score=layer, device=dev)
    for name in ("rank_scores", "topk_scores", "count_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    # thresholds: query q's probability at column q, the column itself skipped (a target is not counted against itself)
    ix = torch.arange(Q, dtype=torch.int32, device=dev).unsqueeze(1)
    thr = holder.rank_scores(emb_q, emb_c[:Q].contiguous(), ix, check_status=False)[:, 0].contiguous()
    skip = torch.arange(Q, dtype=torch.int32, device=dev)
    fns = {"count": lambda: holder.count_scores(emb_q, emb_c, thr, skip=skip),
           "topk1": lambda: holder.topk_scores(emb_q, emb_c, 1, check_status=False),
           "topk10": lambda: holder.topk_scores(emb_q, emb_c, 10, check_status=False)}
    checks = {}
    above, equal = fns["count"]()
    # the count of candidates above the best one is zero, and the best one's own count is what topk1 says
    top = fns["topk1"]()
    best = holder.count_scores(emb_q, emb_c, top[1][:, 0].contiguous())
    checks["nothing_above_the_top1"] = bool((best[0] == 0).all() and (best[1] >= 1).all())
    if N <= PROB_FITS:
        def yardstick():
            prob = holder.rank_scores(emb_q, emb_c, None, check_status=False)
            # column 0 of rank_metrics is the positive: the target's column swapped to the front
            front = torch.cat([prob.gather(1, skip.long().unsqueeze(1)), prob], dim=1)
            cix = torch.zeros(front.shape, dtype=torch.int32, device=dev)
            cix.scatter_(1, (skip.long() + 1).unsqueeze(1), -1)
            return ev.rank_metrics(front, cix, ranks=True)
        fns["rank_count"] = yardstick
        rank = 1.0 + above.double() + 0.5 * equal.double()
        checks["ranks_equal_rank_metrics"] = bool(torch.equal(rank, yardstick()[1].double()))
    return fns, checks


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


def eval_case(n_batches, warm_batches=20):
    """wall-clock ms of one eval_edge_ranking_full pass and of one eval_edge_ranking(n_negatives=100) pass over the same
    `n_batches` batches of workload c1, each on a fresh model warmed over the `warm_batches` batches before them"""
    import bench
    from zebra_amd import evaluation as ev
    from zebra_amd import synth
    wl = dict(synth.WORKLOADS["c1"])
    bs = wl["bs"]
    n = (warm_batches + n_batches) * bs
    src, dst, neg, ts, eidx = bench.make_stream(wl, n)
    w = warm_batches * bs
    data = types.SimpleNamespace(sources=src[w:], destinations=dst[w:], timestamps=ts[w:], edge_idxs=eidx[w:], n_interactions=n - w)
    out = dict(workload="c1", pool=wl["n_nodes"], batch=bs, batches=n_batches)
    for name in ("full", "sampled100"):
        tgn = bench.build_model(wl, torch.device("cuda"), n + 1)
        for s in range(0, w, bs):
            tgn.compute_temporal_embeddings(src[s:s + bs], dst[s:s + bs], neg[s:s + bs], ts[s:s + bs], eidx[s:s + bs], wl["k"], False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "full":
            res = ev.eval_edge_ranking_full(tgn, data, wl["k"], batch_size=bs)
        else:
            res = ev.eval_edge_ranking(tgn, Sampler(dst, 7), data, wl["k"], batch_size=bs, n_negatives=100)
        torch.cuda.synchronize()
        out[name] = dict(ms=round(1e3 * (time.perf_counter() - t0), 1), **{k: round(v, 5) for k, v in res.items()})
        del tgn
        torch.cuda.empty_cache()
    out["full_over_sampled100"] = round(out["full"]["ms"] / out["sampled100"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eval-batches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "rank_of_time.jsonl"))
    a = ap.parse_args()
    out = dict(tool="rank_of_time", rounds=a.rounds, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), shapes=[])
    for Q, N, H in SHAPES:
        fns, checks = count_case(Q, N, H)
        res = dict(Q=Q, N=N, H=H, **checks, **summary(timed(fns, a.rounds, a.iters, a.warmup)))
        res["count_over_topk1"] = round(res["count"]["median_us"] / res["topk1"]["median_us"], 3)
        res["count_over_topk10"] = round(res["count"]["median_us"] / res["topk10"]["median_us"], 3)
        if "rank_count" in res:
            res["count_over_rank_count"] = round(res["count"]["median_us"] / res["rank_count"]["median_us"], 3)
        del fns
        torch.cuda.empty_cache()
        out["shapes"].append(res)
    if a.eval_batches > 0:
        out["eval"] = eval_case(a.eval_batches)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
