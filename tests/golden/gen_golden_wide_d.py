#!/usr/bin/env python3
"""Generate the wide-memory fixtures tests/golden/g12_*.npz from the reference itself.

The reference puts no bound on --node_dim / --memory_dim (train.py:53-55); 172 is the edge-feature width of Wikipedia and
Reddit and a memory size many TGN configurations use.  Like gen_golden.py this runs only where the reference is present:
it imports the reference's Python source unmodified under oracle/numba_standin (through gen_golden's setup) and runs
gen_golden's protocols on the case table below.  Only the resulting data is committed.

    python tests/golden/gen_golden_wide_d.py [--check]

  g12_embed_d172_f172.npz    the G5 protocol of gen_golden.gen_embed (eval and train mode, four dependent batches): per
                             batch the probabilities, the embeddings of the last batch, and after it memory, last_update,
                             timestamps, flags and the message rows of the last batch's nodes
                             (msg_ids, msg_rows -- the whole [N][2D+F+T] table would not fit a fixture)
  g12_train_grads_d172.npz   the reference's loss of one training step per batch (as g8_train_grads) and every parameter
                             gradient as a fingerprint: the values at 1024 fixed flat indices (idx_<param>), the row and
                             column sums and max |g| (the full gradients of the 172-wide GRU would not fit a fixture)

--check regenerates in memory and compares with the committed files.
"""
import argparse
import os
import sys

import numpy as np
import torch

import gen_golden as G          # (sets up the import of the reference under oracle/numba_standin)

I = G.I
HERE = G.HERE
# name -> (n_nodes, n_edges, D, F, T, k, alpha, beta, seed, bs, n_batches): the G4/G5 shape with D = F = 172
WIDE_CASES = {
    "d172_f172": (120, 400, 172, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 34, 20, 4),
}
N_SAMPLE = 1024
OUT = {}


def case(name):
    N, E, D, F, T, k, al, be, seed, bs, nb = WIDE_CASES[name]
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    return (N, E, D, F, T, k, al, be, seed, bs, nb), stream, w, efeat


def gen_embed(name):
    torch.set_num_threads(1)
    (N, E, D, F, T, k, al, be, seed, bs, nb), (src, dst, neg, ts, eidx), w, efeat = case(name)
    out = {}
    for mode, train in (("eval", False), ("train", True)):
        tgn = G.build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
        tgn.train(train)
        for b in range(nb):
            s, e_ = b * bs, (b + 1) * bs
            ctx = torch.enable_grad() if train else torch.no_grad()
            with ctx:
                se, de, ne = tgn.compute_temporal_embeddings(src[s:e_], dst[s:e_], neg[s:e_], ts[s:e_], eidx[s:e_], 10, train)
                score = tgn.affinity_score(torch.cat([se, se], dim=0), torch.cat([de, ne])).squeeze(dim=0)
                prob = score.sigmoid()
            out["%s_b%d_prob" % (mode, b)] = prob.detach().numpy().copy().ravel()
            if train:
                tgn.memory.detach_memory()
            if b == nb - 1:
                pre = "%s_b%d_" % (mode, b)
                out[pre + "emb"] = torch.cat([se, de, ne]).detach().numpy().copy()
                st = G.mem_state(tgn, pre)
                msgs = st.pop(pre + "messages")
                ids = np.unique(np.concatenate([src[s:e_], dst[s:e_]])).astype(np.int32)
                st[pre + "msg_ids"] = ids
                st[pre + "msg_rows"] = msgs[ids].astype(np.float32)
                out.update(st)
    OUT["g12_embed_" + name] = out


def fingerprint(g, idx):
    g = np.asarray(g, np.float32)
    f = {"at": g.ravel()[idx].copy(), "max": np.float32(np.abs(g).max())}
    if g.ndim == 2:
        f["rows"] = g.sum(axis=1, dtype=np.float64).astype(np.float32)
        f["cols"] = g.sum(axis=0, dtype=np.float64).astype(np.float32)
    return f


def gen_train_grads(name):
    torch.set_num_threads(1)
    (N, E, D, F, T, k, al, be, seed, bs, nb), (src, dst, neg, ts, eidx), w, efeat = case(name)
    tgn = G.build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    tgn.train(True)
    crit = torch.nn.BCELoss()
    out = {}
    rng = np.random.RandomState(seed + 1200)
    for b in range(nb):
        s, e_ = b * bs, (b + 1) * bs
        tgn.zero_grad()
        pos, negp = tgn.compute_edge_probabilities(src[s:e_], dst[s:e_], neg[s:e_], ts[s:e_], eidx[s:e_], 10, True)
        loss = crit(pos.squeeze(), torch.ones(bs)) + crit(negp.squeeze(), torch.zeros(bs))
        loss.backward()
        out["b%d_loss" % b] = np.float64(loss.item())
        for pn, p in tgn.named_parameters():
            if p.requires_grad and p.grad is not None:
                if "idx_" + pn not in out:
                    n = p.grad.numel()
                    out["idx_" + pn] = np.sort(rng.choice(n, min(n, N_SAMPLE), replace=False)).astype(np.int32)
                for kk, v in fingerprint(p.grad.detach().numpy(), out["idx_" + pn]).items():
                    out["b%d_%s_%s" % (b, kk, pn)] = v
        tgn.memory.detach_memory()
    assert any(kk.startswith("b%d_at_memory_updater.memory_updater." % (nb - 1)) for kk in out)
    OUT["g12_train_grads_" + name.split("_")[0]] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    for name in WIDE_CASES:
        gen_embed(name)
        gen_train_grads(name)
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
