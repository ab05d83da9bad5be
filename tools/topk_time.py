"""Top-K link scoring over a large shared pool (csrc/rank_topk.hip) against the clock, in ONE process on one GPU:

  topk       TGN.topk_scores (zt_affinity_topk: its GEMMs, the pair kernel and the merge, slab by slab) at
             (Q, C, H, K) = (200, 100 000, 300, 10), (200, 1 000 000, 300, 10), (4096, 10 000, 300, 50), cand_idx NULL;
  rank_topk  what the library offered before: TGN.rank_scores (zt_affinity_rank) into prob [Q, C], then torch.topk.  This is
             the yardstick.

The modes alternate round by round after a warm-up; a round is `--iters` calls between two events on the stream.  Prints ONE
JSON line: the median microseconds per call of both modes over `--rounds` rounds, with the spread (min, max), their ratio, and
whether the new median lies below the yardstick's minimum.

    python tools/topk_time.py [--rounds 10] [--iters 3] [--warmup 2] [--exclude-seen]

--exclude-seen adds, per shape, what TGN.recommend does behind its embeddings, over a random graph on the pool's C ids (5 C
edges, half of them at one of the Q sources: ~ 5 C / 2 Q entries per source, about half of them before the query time):
  chunks     the pool in chunks of 65 536 rows through topk_scores with accumulate: recommend(exclude=None);
  filtered   zt_csr_seen_ranges once, then per chunk zt_exclude_mark and zt_affinity_topk_masked: recommend(exclude="seen");
  mark       the seen ranges and the mark kernels of `filtered` alone -- `mark_share` is its median over `filtered`'s.
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from zebra_amd.modules import MergeLayer  # noqa: E402
from zebra_amd.tgn import TGN  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_time import summary, timed  # noqa: E402

SHAPES = [(200, 100000, 300, 10), (200, 1000000, 300, 10), (4096, 10000, 300, 50)]


def topk_case(Q, C_, H, K, seed=0):
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = MergeLayer(H, H, H, 1).to(dev)
    g = torch.Generator().manual_seed(seed + Q + C_)
    emb_q = (torch.randn((Q, H), generator=g) * 0.7).to(dev)
    emb_c = (torch.randn((C_, H), generator=g) * 0.7).to(dev)
    holder = types.SimpleNamespace(affinity_score=layer, device=dev)
    for name in ("rank_scores", "topk_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))

    def yardstick():
        return torch.topk(holder.rank_scores(emb_q, emb_c, None, check_status=False), K, dim=1)

    fns = {"topk": lambda: holder.topk_scores(emb_q, emb_c, K, check_status=False), "rank_topk": yardstick}
    # the same probabilities (torch.topk's order among equal ones is its own)
    same = bool(torch.equal(fns["topk"]()[1], fns["rank_topk"]().values))
    return fns, same


POOL_CHUNK = 65536


def seen_case(Q, C_, H, K, seed=0):
    """the three --exclude-seen modes on topk_case's embeddings; node id v is column v of the pool, the sources are ids 0 .. Q - 1"""
    import numpy as np
    from zebra_amd.tppr import get_neighbor_finder
    dev = torch.device("cuda")
    torch.manual_seed(seed)
    layer = MergeLayer(H, H, H, 1).to(dev)
    g = torch.Generator().manual_seed(seed + Q + C_)
    emb_q = (torch.randn((Q, H), generator=g) * 0.7).to(dev)
    emb_c = (torch.randn((C_, H), generator=g) * 0.7).to(dev)
    rng = np.random.RandomState(seed)
    E = 5 * C_
    src = np.where(rng.random_sample(E) < 0.5, rng.randint(0, Q, E), rng.randint(0, C_, E)).astype(np.int32)
    data = types.SimpleNamespace(sources=src, destinations=rng.randint(0, C_, E).astype(np.int32), edge_idxs=np.arange(1, E + 1),
                                 timestamps=np.sort(rng.random_sample(E)))
    data.sources[0] = C_ - 1                                                 # (the finder covers every id of the pool)
    nf = get_neighbor_finder(data)
    holder = types.SimpleNamespace(affinity_score=layer, device=dev, neighbor_finder=nf)
    for name in ("rank_scores", "topk_scores", "_as_device", "_exclude_lists", "_mark_absent"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    src_d = torch.arange(Q, dtype=torch.int32, device=dev)
    ts_d = torch.full((Q,), 0.5, dtype=torch.float64, device=dev)
    chunks = [(s, min(C_, s + POOL_CHUNK)) for s in range(0, C_, POOL_CHUNK)]
    rows = [emb_c[s:e].contiguous() for s, e in chunks]

    def run(filtered, score):
        lists = holder._exclude_lists(src_d, ts_d, "seen") if filtered else None
        out = (torch.full((Q, K), -1, dtype=torch.int32, device=dev), torch.zeros((Q, K), dtype=torch.float32, device=dev))
        for (s, e), ec in zip(chunks, rows):
            absent = holder._mark_absent(lists, Q, id_lo=s, n_cols=e - s) if filtered else None
            if score:
                holder.topk_scores(emb_q, ec, K, idx_base=s, out=out, check_status=False, absent=absent)
        return out

    fns = {"chunks": lambda: run(False, True), "filtered": lambda: run(True, True), "mark": lambda: run(True, False)}
    whole = holder.topk_scores(emb_q, emb_c, K, check_status=False)
    same = bool(torch.equal(fns["chunks"]()[0], whole[0]) and torch.equal(fns["chunks"]()[1], whole[1]))
    begin, length = holder._exclude_lists(src_d, ts_d, "seen")[2:]
    got = fns["filtered"]()[0]
    clean = all(int(v) not in set(nf._nbr[int(begin[q]):int(begin[q]) + int(length[q])].tolist()) for q in (0, Q - 1)
                for v in got[q].tolist())
    return fns, dict(chunks_equal_one_call=same, filtered_returns_no_seen_partner=clean, seen_entries_mean=float(length.float().mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exclude-seen", action="store_true")
    a = ap.parse_args()
    out = dict(tool="topk_time", rounds=a.rounds, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), shapes=[])
    for Q, C_, H, K in SHAPES:
        fns, same = topk_case(Q, C_, H, K)
        res = dict(Q=Q, C=C_, H=H, K=K, same_probabilities=same, **summary(timed(fns, a.rounds, a.iters, a.warmup)))
        res["topk_over_rank_topk"] = round(res["topk"]["median_us"] / res["rank_topk"]["median_us"], 3)
        res["below_yardstick_min"] = res["topk"]["median_us"] < res["rank_topk"]["min_us"]
        del fns
        torch.cuda.empty_cache()
        if a.exclude_seen:
            fns, checks = seen_case(Q, C_, H, K)
            res["exclude_seen"] = dict(pool_chunk=POOL_CHUNK, **checks, **summary(timed(fns, a.rounds, a.iters, a.warmup)))
            res["exclude_seen"]["mark_share"] = round(res["exclude_seen"]["mark"]["median_us"] / res["exclude_seen"]["filtered"]["median_us"], 3)
            del fns
            torch.cuda.empty_cache()
        out["shapes"].append(res)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
