#!/usr/bin/env python3
"""Generate the RNN memory-updater fixtures tests/golden/g11_rnn_*.npz from the reference itself.

The reference's `--memory_updater rnn` (train.py:39) runs RNNMemoryUpdater, i.e. nn.RNNCell in update_memory,
update_memory_in_test and get_updated_memory (modules/memory_updater.py:100-103).  Like gen_golden.py this runs
only where the reference is present: it imports the reference's Python source unmodified under
oracle/numba_standin (through gen_golden's setup) and builds the reference TGN with memory_updater_type="rnn".
Only the resulting data is committed.

    python tests/golden/gen_golden_rnn.py [--check]

  g11_rnn_embed_<case>.npz   the G5 protocol of gen_golden.gen_embed (eval and train mode): per batch the
                             embeddings and probabilities, after the last batch memory, last_update, messages,
                             timestamps and flags, and in eval mode the memory after the batch before it;
                             the RNN weights used (rnn_w_ih [D][msg], rnn_w_hh [D][D], rnn_b_ih, rnn_b_hh [D])
  g11_rnn_train_grads.npz    the reference's loss and every parameter gradient of one training step per batch
                             (as g8_train_grads), RNN weights included
  g11_rnn_state_dict.npz     the reference RNNMemoryUpdater's state_dict keys and shapes

--check regenerates in memory and compares with the committed files.
"""
import argparse
import os
import sys

import numpy as np
import torch

import gen_golden as G          # (sets up the import of the reference under oracle/numba_standin)

I = G.I
TGN = G.TGN
HERE = G.HERE
EMBED = ("d20_f7", "d100_f172")
OUT = {}


def rnn_weights(D, msg, seed):
    """nn.RNNCell parameters in torch layout, drawn as torch initialises them (uniform, +-1/sqrt(D))."""
    rng = np.random.RandomState(seed + 1100)
    s = 1.0 / np.sqrt(D)
    u = lambda *shape: rng.uniform(-s, s, shape).astype(np.float32)
    return dict(rnn_w_ih=u(D, msg), rnn_w_hh=u(D, D), rnn_b_ih=u(D), rnn_b_hh=u(D))


def build_tgn(N, E1, D, F, T, k, al, be, w, rw, efeat):
    """gen_golden.build_tgn with memory_updater_type="rnn" and the RNN's weights."""
    import types
    args = types.SimpleNamespace(alpha_list=list(al), beta_list=list(be), topk=k, tppr_strategy="streaming",
                                 n_degree=10, n_layer=2, n_nodes=N, n_edges=E1)
    tgn = TGN(neighbor_finder=None, node_features=None, edge_features=efeat.astype(np.float64), device="cpu",
              n_layers=2, n_heads=2, dropout=0.0, use_memory=True, node_dimension=D, time_dimension=T,
              memory_dimension=D, embedding_module_type="diffusion", message_function="identity",
              aggregator_type="last", memory_updater_type="rnn", n_neighbors=10, args=args)
    assert isinstance(tgn.memory_updater.memory_updater, torch.nn.RNNCell)
    em = tgn.embedding_module
    with torch.no_grad():
        for mod, pre in ((em.fc1, "fc1"), (em.fc2, "fc2"), (em.fc1_source, "fc1s"), (em.fc2_source, "fc2s")):
            mod.weight.copy_(torch.from_numpy(w[pre + "_w"]))
            mod.bias.copy_(torch.from_numpy(w[pre + "_b"]))
        g = tgn.memory_updater.memory_updater
        g.weight_ih.copy_(torch.from_numpy(rw["rnn_w_ih"]))
        g.weight_hh.copy_(torch.from_numpy(rw["rnn_w_hh"]))
        g.bias_ih.copy_(torch.from_numpy(rw["rnn_b_ih"]))
        g.bias_hh.copy_(torch.from_numpy(rw["rnn_b_hh"]))
        tgn.affinity_score.fc1.weight.copy_(torch.from_numpy(w["aff1_w"]))
        tgn.affinity_score.fc1.bias.copy_(torch.from_numpy(w["aff1_b"]))
        tgn.affinity_score.fc2.weight.copy_(torch.from_numpy(w["aff2_w"]))
        tgn.affinity_score.fc2.bias.copy_(torch.from_numpy(w["aff2_b"]))
    em.drop.p = 0.0
    tgn.reset_timer()
    return tgn


def case(name):
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES[name]
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    rw = rnn_weights(D, 2 * D + F + T, seed)
    return (N, E, D, F, T, k, al, be, seed, bs, nb), stream, w, rw, efeat


def gen_embed():
    torch.set_num_threads(1)
    for name in EMBED:
        (N, E, D, F, T, k, al, be, seed, bs, nb), (src, dst, neg, ts, eidx), w, rw, efeat = case(name)
        out = dict(rw)
        for mode, train in (("eval", False), ("train", True)):
            tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat)
            tgn.train(train)
            for b in range(nb):
                s, e_ = b * bs, (b + 1) * bs
                ctx = torch.enable_grad() if train else torch.no_grad()
                with ctx:
                    se, de, ne = tgn.compute_temporal_embeddings(src[s:e_], dst[s:e_], neg[s:e_], ts[s:e_],
                                                                 eidx[s:e_], 10, train)
                    score = tgn.affinity_score(torch.cat([se, se], dim=0), torch.cat([de, ne])).squeeze(dim=0)
                    prob = score.sigmoid()
                out["%s_b%d_emb" % (mode, b)] = torch.cat([se, de, ne]).detach().numpy().copy()
                out["%s_b%d_prob" % (mode, b)] = prob.detach().numpy().copy().ravel()
                if train:
                    tgn.memory.detach_memory()
                if not train and b == nb - 2:
                    out["eval_b%d_memory" % b] = tgn.memory.memory.detach().numpy().copy()
                if b == nb - 1:
                    out.update(G.mem_state(tgn, "%s_b%d_" % (mode, b)))
        OUT["g11_rnn_embed_" + name] = out


def gen_train_grads():
    torch.set_num_threads(1)
    (N, E, D, F, T, k, al, be, seed, bs, nb), (src, dst, neg, ts, eidx), w, rw, efeat = case("d20_f7")
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat)
    tgn.train(True)
    crit = torch.nn.BCELoss()
    out = dict(rw)
    for b in range(nb):
        s, e_ = b * bs, (b + 1) * bs
        tgn.zero_grad()
        pos, negp = tgn.compute_edge_probabilities(src[s:e_], dst[s:e_], neg[s:e_], ts[s:e_], eidx[s:e_], 10, True)
        loss = crit(pos.squeeze(), torch.ones(bs)) + crit(negp.squeeze(), torch.zeros(bs))
        loss.backward()
        out["b%d_loss" % b] = np.float64(loss.item())
        for pn, p in tgn.named_parameters():
            if p.requires_grad and p.grad is not None:
                out["b%d_grad_%s" % (b, pn)] = p.grad.detach().numpy().copy()
        tgn.memory.detach_memory()
    assert any("_grad_memory_updater.memory_updater." in kk for kk in out)      # (batch 0 has no pending message)
    OUT["g11_rnn_train_grads"] = out


def gen_state_dict():
    (N, E, D, F, T, k, al, be, seed, bs, nb), _, w, rw, efeat = case("d20_f7")
    sd = build_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat).memory_updater.state_dict()
    keys = list(sd)
    out = dict(keys=np.array(keys), message_dimension=np.int64(2 * D + F + T), memory_dimension=np.int64(D))
    for kk in keys:
        out["shape_" + kk] = np.array(sd[kk].shape, np.int64)
    OUT["g11_rnn_state_dict"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    gen_state_dict()
    gen_embed()
    gen_train_grads()
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
