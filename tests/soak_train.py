"""Randomised soak of the training path: the fused HIP forward + backward (aggregation over the overlay, GRU rows, fc2,
source transform: aggregate_bwd.hip, train_ops.hip) against the plain torch composition of the same step -- which fixture
g8_train_grads pins to the reference's gradients -- on random shapes.  Test infrastructure, run on a GPU box:
    python tests/soak_train.py [seconds] [first seed]
The cotangent of the embeddings is a fixed random matrix (a linear loss: nothing downstream amplifies rounding); embeddings
to 1e-5, every parameter gradient to 1e-4 of its scale in all but 1 % of the elements and to 2e-3 in norm (a ReLU whose
pre-activation is within rounding of zero may flip).  One or two models; three or four now and then from seed 100000 on
(soak_tppr.many_models)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def one(seed, torch):
    import inputs as I
    from helpers import build_tgn
    from soak_tppr import many_models
    rng = np.random.RandomState(seed)
    D, T = [(100, 100), (100, 100), (32, 16), (64, 100)][rng.randint(4)]
    F = int(rng.choice([1, 4, 16, 172]))
    k = int(rng.choice([5, 10, 20, 40]))
    M = int(rng.choice([1, 2]))
    N = int(rng.choice([60, 900, 5000]))
    bs = int(rng.choice([20, 200, 600]))
    nb = int(rng.randint(2, 5))
    kind = ["bipartite", "general", "hub"][rng.randint(3)]
    al = [float(rng.choice([0.1, 0.2])) for _ in range(M)]
    be = [float(rng.choice([0.5, 0.8, 0.95])) for _ in range(M)]
    many = many_models(seed, [0.1, 0.2], [0.5, 0.8, 0.95])       # (seeds from soak_tppr.MANY_MODELS_SEED on: three or four models)
    if many is not None:
        M, al, be = many
    E = bs * nb
    tag = "seed %d: N=%d bs=%d nb=%d k=%d D=%d T=%d F=%d M=%d %s" % (seed, N, bs, nb, k, D, T, F, M, kind)
    if os.environ.get("ZT_SOAK_VERBOSE"):
        print(tag, flush=True)
    src, dst, neg, ts, eidx = I.make_stream(kind, N, E, seed)
    w = I.model_weights(D, F, T, M, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    dev = torch.device("cuda")
    G = [torch.from_numpy(np.random.RandomState(seed * 7 + b).standard_normal((3 * bs, (M + 1) * D)).astype(np.float32)).to(dev)
         for b in range(nb)]
    res = {}
    for fused in (True, False):
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
        tgn.embedding_module.fused_training = fused
        tgn.train(True)
        out = []
        for b in range(nb):
            s, e = b * bs, (b + 1) * bs
            tgn.zero_grad()
            se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
            emb = torch.cat([se, de, ne])
            (emb * G[b]).sum().backward()
            out.append((emb.detach().cpu().numpy(), {pn: p.grad.detach().cpu().numpy().copy()
                                                    for pn, p in tgn.named_parameters() if p.grad is not None}))
        res[fused] = out
    for b in range(nb):
        ea, ga = res[True][b]
        eb, gb = res[False][b]
        if not np.abs(ea - eb).max() <= 1e-5:
            return "%s: embeddings of batch %d differ by %g" % (tag, b, np.abs(ea - eb).max())
        if set(ga) != set(gb):
            return "%s: different sets of parameters have gradients in batch %d" % (tag, b)
        # A ReLU of the hidden layer whose pre-activation is within rounding of zero may come out on the other side (the two
        # paths round the fc1 product differently).  Then ONE hidden unit's row of fc1's gradient changes by one term, and
        # everything upstream of it (the overlay rows, hence the GRU's gradients) by a small dense amount.  Up to five such
        # units per batch and layer are left out of the comparison of that layer; the GRU's gradients are then held to the norm only.
        flipped, off = False, {}
        for layer in ("embedding_module.fc1", "embedding_module.fc1_source"):            # the two layers in front of a ReLU
            fw, fb = layer + ".weight", layer + ".bias"
            if fw not in ga:
                continue
            u = (np.abs(ga[fw] - gb[fw]) > 1e-4 * max(1.0, np.abs(gb[fw]).max())).any(axis=1)
            u |= np.abs(ga[fb] - gb[fb]) > 1e-4 * max(1.0, np.abs(gb[fb]).max())
            if u.sum() > 5:
                return "%s: the gradient of %s differs in %d hidden units in batch %d" % (tag, layer, int(u.sum()), b)
            off[fw] = off[fb] = u
            flipped = flipped or bool(u.any())
        for pn in ga:
            x, y = ga[pn], gb[pn]
            if pn in off:
                x, y = x[~off[pn]], y[~off[pn]]
            d, scale = np.abs(x - y), max(1.0, np.abs(y).max())
            if flipped and pn.startswith("memory_updater"):
                continue        # (a flipped unit whose input row occurs hundreds of times in the batch -- a hub's memory row, a
                                #  node of a tiny graph -- flips hundreds of terms at once: what reaches the GRU's gradients
                                #  through the overlay rows has no useful bound; the batches without a flip, the vast majority,
                                #  check them to 1e-4)
            if (d > 1e-4 * scale).mean() > 0.01:
                return "%s: %s in batch %d: %.3g of the elements differ" % (tag, pn, b, (d > 1e-4 * scale).mean())
            if np.linalg.norm(x - y) > 2e-3 * max(1.0, np.linalg.norm(y)):
                return "%s: %s in batch %d differs in norm" % (tag, pn, b)
    return None


def main():
    import torch
    assert torch.cuda.is_available()
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
    t0, n = time.time(), 0
    while time.time() - t0 < budget:
        err = one(seed, torch)
        if err:
            print("FAIL", err)
            sys.exit(1)
        n += 1
        seed += 1
        if n % 5 == 0:
            print("%d configurations within tolerance (%.0f s)" % (n, time.time() - t0), flush=True)
    print("soak ok: %d configurations, seeds up to %d" % (n, seed - 1))


if __name__ == "__main__":
    main()
