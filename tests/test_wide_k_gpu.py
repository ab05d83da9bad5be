"""Neighbour aggregation over query rows wider than one LDS tile (csrc/aggregate_split.hip, the chunked tiles of
k_fc1_agg_bwd): the fused training path for 80 < k <= 255 against the torch composition of the same step, and eval
with 172-wide edge features past k = 136 against the CPU oracle."""
import types

import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _grads_agree(a, b, what):
    # float32 sums in another order, and now and then a ReLU whose pre-activation is within rounding of zero: all but a
    # sliver of the elements to 1e-4 of the scale, the whole to 2e-3 in norm (test_fused_training_backward_full_dims)
    d, scale = np.abs(a - b), max(1.0, np.abs(b).max())
    assert (d > 1e-4 * scale).mean() <= 0.01, "%s: %.3g of the elements differ" % (what, (d > 1e-4 * scale).mean())
    assert np.linalg.norm(a - b) <= 2e-3 * max(1.0, np.linalg.norm(b)), what


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("F", [1, 172])
@pytest.mark.parametrize("k", [81, 100, 128, 255])
def test_row_split_aggregate_forward_backward(k, F, p):
    """_NeighbourAggregate (zt_agg_train_forward / zt_agg_train_backward) beyond one 80-row tile against the torch
    composition with the kernels' own dropout mask: overlay rows that repeat within and across query rows, query rows
    whose weights are all zero (S = 0), and H the same bits from run to run."""
    from zebra_amd.modules import _NeighbourAggregate, dropout_mask
    D = T = 100
    N, E1, n, M = 600, 2000, 37, 2
    g = torch.Generator().manual_seed(1000 + k + F)
    w = I.model_weights(D, F, T, M, 56)
    _, efeat = I.random_tables(N, E1, D, F, 56)
    tgn = build_tgn(N, E1, D, F, T, k, [0.1, 0.1], [0.5, 0.95], w, efeat)
    em = tgn.embedding_module
    dev = tgn.device
    mem = torch.randn((N, D), generator=g).to(dev)
    U = 30
    ids = torch.randperm(N, generator=g)[:U].to(dev)
    overlay = torch.randn((U, D), generator=g).to(dev).requires_grad_(True)
    row_map = torch.full((N,), -1, dtype=torch.int32, device=dev)
    row_map[ids] = torch.arange(U, dtype=torch.int32, device=dev)
    on = torch.randint(0, N, (M, n, k), generator=g, dtype=torch.int32)
    on[:, :, ::3] = ids.cpu()[torch.randint(0, U, (M, n, (k + 2) // 3), generator=g)].to(torch.int32)   # repeated overlay rows
    on = on.to(dev)
    oe = torch.randint(0, E1, (M, n, k), generator=g, dtype=torch.int32).to(dev)
    od = (torch.rand((M, n, k), generator=g) * 1e5).to(dev)
    ow = torch.rand((M, n, k), generator=g)
    ow[:, ::6] = 0.0                                                           # S = 0 rows
    ow = ow.to(dev)
    G = torch.randn((M, n, D), generator=g).to(dev)
    fc1_w = em.fc1.weight.detach().clone().requires_grad_(True)
    fc1_b = em.fc1.bias.detach().clone().requires_grad_(True)
    seed = 0x0BADC0DE12345678 if p > 0 else 0

    def fused():
        for t in (overlay, fc1_w, fc1_b):
            t.grad = None
        H, S = _NeighbourAggregate.apply(overlay, fc1_w, fc1_b, em, mem, row_map, ids.to(torch.int32), on, oe, od, ow, p, seed)
        (H * G).sum().backward()
        row_map[ids] = torch.arange(U, dtype=torch.int32, device=dev)       # (the backward resets the shared map)
        return H.detach().cpu().numpy(), S.cpu().numpy(), [t.grad.detach().cpu().numpy().copy() for t in (overlay, fc1_w, fc1_b)]

    def composed(mask):
        for t in (overlay, fc1_w, fc1_b):
            t.grad = None
        rows = torch.where((row_map[on.long()] >= 0).unsqueeze(-1), overlay[row_map[on.long()].long().clamp(min=0)], mem[on.long()])
        x = torch.cat([rows, em.edge_features[oe.long()], em.time_encoder(od.reshape(M * n, k)).reshape(M, n, k, T)], dim=-1)
        h = torch.relu(torch.nn.functional.linear(x, fc1_w, fc1_b)) * mask
        ws = ow.sum(dim=2, keepdim=True)
        wn = torch.where(ws == 0, torch.zeros_like(ow), ow / ws)
        H = (h * wn.unsqueeze(-1)).sum(dim=2)
        (H * G).sum().backward()
        return H.detach().cpu().numpy(), (ws.squeeze(-1) != 0).float().cpu().numpy(), \
            [t.grad.detach().cpu().numpy().copy() for t in (overlay, fc1_w, fc1_b)]

    mask = torch.from_numpy(dropout_mask(seed, p, (M, n, k), D)).to(dev) if p > 0 else torch.ones((M, n, k, D), device=dev)
    Hf, Sf, gf = fused()
    Hc, Sc, gc = composed(mask)
    assert np.array_equal(Sf, Sc) and (Sc == 0).any() and (Sc == 1).any()
    assert np.abs(Hf[Sc == 0]).max() == 0.0
    assert np.abs(Hf - Hc).max() <= 1e-5 * max(1.0, np.abs(Hc).max())
    for a, b, name in zip(gf, gc, ("d_overlay", "dW1", "db1")):
        _grads_agree(a, b, "%s (k=%d F=%d p=%g)" % (name, k, F, p))
    assert np.abs(gf[0]).max() > 0
    H2, _, _ = fused()
    assert np.array_equal(Hf, H2), "the forward is not deterministic"
    st = int(em._status.item()) if em._status is not None else 0
    assert st == 0


def _model_grads(F, k, strategy, nb=3, bs=40):
    D = T = 100
    N, E, al, be, seed = 400, 600, [0.1, 0.1], [0.5, 0.95], 300 + k + F
    src, dst, neg, ts, eidx = I.make_stream("general" if strategy == "pruning" else "bipartite", N, E, seed)
    w = I.model_weights(D, F, T, 2, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    dev = torch.device("cuda")
    G = [torch.from_numpy(np.random.RandomState(800 + b).standard_normal((3 * bs, 3 * D)).astype(np.float32)).to(dev)
         for b in range(nb)]
    nf = None
    if strategy == "pruning":
        from zebra_amd.tppr import get_neighbor_finder
        nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    res = {}
    for fused in (True, False):
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat, strategy=strategy, nf=nf)
        tgn.embedding_module.fused_training = fused
        tgn.train(True)
        out = []
        first = E - nb * bs                                    # late in the stream: full-width T-PPR rows
        if strategy == "streaming":
            with torch.no_grad():                              # (the history the rows are built from, as in an epoch)
                tgn.embedding_module.tppr_finder.compute_val_tppr(src[:first], dst[:first], ts[:first], eidx[:first])
                tgn.embedding_module.tppr_finder.restore_val_tppr()
        for b in range(nb):
            s, e = first + b * bs, first + (b + 1) * bs
            tgn.zero_grad()
            se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
            emb = torch.cat([se, de, ne])
            (emb * G[b]).sum().backward()
            out.append((emb.detach().cpu().numpy(), {pn: p.grad.detach().cpu().numpy().copy()
                                                    for pn, p in tgn.named_parameters() if p.grad is not None}))
            tgn.memory.detach_memory()
        res[fused] = out
    return res


@pytest.mark.parametrize("F,k,strategy", [(1, 100, "streaming"), (172, 128, "streaming"), (1, 100, "pruning")])
def test_fused_training_beyond_one_tile(F, k, strategy):
    """compute_temporal_embeddings(train=True) over dependent batches, fused_training True against False (the torch
    composition), a fixed cotangent: embeddings and the gradients of every embedding / GRU parameter."""
    res = _model_grads(F, k, strategy)
    for b in range(len(res[True])):
        ea, ga = res[True][b]
        eb, gb = res[False][b]
        assert np.abs(ea - eb).max() <= 1e-5, "embeddings of batch %d" % b
        assert set(ga) == set(gb) and len(ga) >= 8
        for pn in ga:
            _grads_agree(ga[pn], gb[pn], "%s in batch %d" % (pn, b))
    assert any(np.abs(res[True][b][1]["embedding_module.fc1.weight"]).max() > 0 for b in range(len(res[True])))


@pytest.mark.parametrize("k", [160, 255])
def test_eval_wide_edge_features_past_one_tile(oracle, k):
    """F = 172 (Wikipedia / Reddit) with k past what a tile holds: embeddings over dependent batches within 1e-4 of the
    CPU oracle, the T-PPR state bit-exact (the protocol of test_protocol_vs_oracle)."""
    D = T = 100
    F, al, be, seed = 172, [0.1, 0.1], [0.5, 0.95], 400 + k
    N, E, bs, warm, nb = 120, 1500, 60, 1200, 4
    M = len(al)
    src, dst, neg, ts, eidx = I.make_stream("bipartite", N, E, seed)
    w = I.model_weights(D, F, T, M, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tw = I.time_encode_weights(T)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()
    f = oracle.TpprOracle(N, k, M, al, be)
    mem = oracle.MemoryOracle(N, D, 2 * D + F + T)
    gru = {kk: w[kk] for kk in ("w_ih", "w_hh", "b_ih", "b_hh")}
    s, widest = 0, 0
    while s < warm + nb * bs:
        e = s + bs
        nodes = np.concatenate([src[s:e], dst[s:e], neg[s:e]])
        with torch.no_grad():
            se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, False)
        on, oe, od, ow = f.streaming_topk(nodes, ts[s:e], eidx[s:e])
        widest = max(widest, int((np.stack(ow) != 0).sum(axis=-1).max()))
        if s >= warm:
            emb = oracle.embed(mem.memory, efeat, tw, nodes, np.stack(on), np.stack(oe), np.stack(od), np.stack(ow), w,
                               n_threads=8)
            got = torch.cat([se, de, ne]).cpu().numpy()
            assert np.abs(got - emb).max() <= TOL, "embeddings differ at edge %d" % s
        mem.store_messages(efeat, tw, src[s:e], dst[s:e], ts[s:e], eidx[s:e])
        mem.gru_update(gru, np.unique(np.concatenate([src[s:e], dst[s:e]])), n_threads=8)
        s = e
    assert widest > 136, "no query row wider than one tile (%d)" % widest
    for m in range(M):
        a, b = tgn.embedding_module.tppr_finder.export_state(m), f.export(m)
        for kk in a:
            assert np.array_equal(a[kk], b[kk])
    assert np.abs(tgn.memory.memory.cpu().numpy() - mem.memory).max() <= TOL
