"""Memory / embedding widths 128 < D <= 256 (D % 4 == 0) on the device: the NTW_WIDE instantiations of k_fc1_agg,
k_fc1_agg_split, k_embed_out and k_project_rows, k_gru's two hidden N-tiles per wave and k_fc1_agg_bwd's wide form.
zt_embed on ragged row counts with and without the projected table, eval over dependent batches against the CPU oracle,
the GRU / RNN update against torch's cells, the native pipeline against the sequential path, the eval / train protocol
and the training step against the reference's fixtures (g12_*, tests/golden/gen_golden_wide_d.py), and the fused
training step against the torch composition."""
import types

import numpy as np
import pytest
import torch

import inputs as I
from conftest import golden
from helpers import build_tgn

# the g12_* case (tests/golden/gen_golden_wide_d.py: WIDE_CASES)
G12 = (120, 400, 172, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 34, 20, 4)

pytestmark = pytest.mark.gpu
TOL = 1e-4                  # the project's embedding gate


@pytest.mark.parametrize("D", [172, 256])
@pytest.mark.parametrize("F", [1, 172])
@pytest.mark.parametrize("k", [20, 100])
def test_wide_d_eval_against_oracle(oracle, D, F, k):
    """compute_temporal_embeddings(train=False) over dependent batches: embeddings within 1e-4 of the CPU oracle, the
    memory table within 1e-4 after every batch's GRU update, the T-PPR state bit-exact."""
    T = 100
    al, be, seed = [0.1, 0.1], [0.5, 0.95], 500 + D + F + k
    N, E, bs, warm, nb = 120, 560, 40, 400, 4
    M = len(al)
    src, dst, neg, ts, eidx = I.make_stream("bipartite", N, E, seed)
    w = I.model_weights(D, F, T, M, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tw = I.time_encode_weights(T)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()
    f = oracle.TpprOracle(N, k, M, al, be)
    mem = oracle.MemoryOracle(N, D, 2 * D + F + T)
    gru = {kk: w[kk] for kk in ("w_ih", "w_hh", "b_ih", "b_hh")}
    s, checked = 0, 0
    while s < warm + nb * bs:
        e = s + bs
        nodes = np.concatenate([src[s:e], dst[s:e], neg[s:e]])
        with torch.no_grad():
            se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, False)
        on, oe, od, ow = f.streaming_topk(nodes, ts[s:e], eidx[s:e])
        if s >= warm:
            emb = oracle.embed(mem.memory, efeat, tw, nodes, np.stack(on), np.stack(oe), np.stack(od), np.stack(ow), w,
                               n_threads=8)
            got = torch.cat([se, de, ne]).cpu().numpy()
            assert got.shape == (3 * bs, D * (M + 1))
            assert np.abs(got - emb).max() <= TOL, "embeddings differ at edge %d" % s
            checked += 1
        mem.store_messages(efeat, tw, src[s:e], dst[s:e], ts[s:e], eidx[s:e])
        mem.gru_update(gru, np.unique(np.concatenate([src[s:e], dst[s:e]])), n_threads=8)
        s = e
    assert checked == nb
    for m in range(M):
        a, b = tgn.embedding_module.tppr_finder.export_state(m), f.export(m)
        for kk in a:
            assert np.array_equal(a[kk], b[kk])
    assert np.abs(tgn.memory.memory.cpu().numpy() - mem.memory).max() <= TOL
    assert np.abs(mem.memory).max() > 0


def _cell_weights(cell, D, msg, seed):
    rng = np.random.RandomState(seed)
    s = 1.0 / np.sqrt(D)
    g = 3 if cell == "gru" else 1
    u = lambda *shape: rng.uniform(-s, s, shape).astype(np.float32)
    return dict(w_ih=u(g * D, msg), w_hh=u(g * D, D), b_ih=u(g * D), b_hh=u(g * D))


@pytest.mark.parametrize("cell", ["gru", "rnn"])
@pytest.mark.parametrize("D", [172, 256])
@pytest.mark.parametrize("n", [1, 37, 400, 8192])
def test_wide_d_memory_update(cell, D, n):
    """zt_gru_update / zt_rnn_update (k_gru, two hidden N-tiles per wave) against torch's GRUCell / RNNCell on the same
    flagged rows: memory, last_update, flags cleared, rows that are not flagged untouched, and the projected table kept
    up to date from the rows the update reports."""
    from zebra_amd.tgn import TGN
    from helpers import load_weights, make_args
    F = T = 100
    N, E1 = 9000, 100
    msg_dim = 2 * D + F + T
    w = I.model_weights(D, F, T, 2, 41)
    cw = _cell_weights(cell, D, msg_dim, 41 + D)
    w.update(cw)
    _, efeat = I.random_tables(N, E1, D, F, 41)
    tgn = TGN(neighbor_finder=None, node_features=None, edge_features=efeat, device="cuda", n_layers=2, n_heads=2,
              dropout=0.0, use_memory=True, node_dimension=D, time_dimension=T, memory_dimension=D,
              embedding_module_type="diffusion", message_function="identity", aggregator_type="last",
              memory_updater_type=cell, n_neighbors=10, args=make_args(N, E1, 20, [0.1, 0.1], [0.5, 0.95]))
    tgn = load_weights(tgn.to("cuda"), w).eval()
    em, m = tgn.embedding_module, tgn.memory
    g = torch.Generator().manual_seed(D + n)
    msg = torch.randn((N, msg_dim), generator=g)
    mem0 = torch.randn((N, D), generator=g) * 0.3
    ts = torch.rand(N, generator=g) * 1e6
    ids = (torch.randperm(N - 1, generator=g)[:n] + 1).to(torch.int32)
    m.messages.copy_(msg.cuda()); m.memory.copy_(mem0.cuda()); m.timestamps.copy_(ts.cuda())
    m.last_update.zero_()
    ids_d = ids.cuda()
    m._flag_buf[ids_d.long()] = 1
    table = em._projection(m)
    tgn.memory_updater.update_device(m, ids_d, ids_d.numel())
    torch.cuda.synchronize()
    got, lu_got, flags = m.memory.cpu().numpy(), m.last_update.cpu().numpy(), m._flag_buf.cpu().numpy()[:N]
    if table is not None:
        upd = em._projection(m).clone()
        em.invalidate_projection()
        full = em._projection(m).clone()
        torch.cuda.synchronize()
        assert torch.equal(upd, full)
    ref = torch.nn.GRUCell(msg_dim, D) if cell == "gru" else torch.nn.RNNCell(msg_dim, D)
    with torch.no_grad():
        for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            getattr(ref, name).copy_(torch.from_numpy(cw[key]))
        want = mem0.clone()
        want[ids.long()] = ref(msg[ids.long()], mem0[ids.long()])
    assert np.abs(got - want.numpy()).max() <= 1e-5
    lu = np.zeros(N, np.float32)
    lu[ids.numpy()] = ts.numpy()[ids.numpy()]
    assert np.array_equal(lu_got, lu)
    assert not flags.any()
    rest = np.ones(N, bool)
    rest[ids.numpy()] = False
    assert np.array_equal(got[rest], mem0.numpy()[rest])


def _grads_agree(a, b, what):
    # (test_wide_k_gpu.py: float32 sums in another order, now and then a ReLU within rounding of zero)
    d, scale = np.abs(a - b), max(1.0, np.abs(b).max())
    assert (d > 1e-4 * scale).mean() <= 0.01, "%s: %.3g of the elements differ" % (what, (d > 1e-4 * scale).mean())
    assert np.linalg.norm(a - b) <= 2e-3 * max(1.0, np.linalg.norm(b)), what


@pytest.mark.parametrize("F,k", [(172, 20), (1, 100)])
def test_wide_d_fused_training(F, k, monkeypatch):
    """compute_temporal_embeddings(train=True) at D = 172 over dependent batches, fused_training True (the wide
    k_fc1_agg / k_fc1_agg_split forward, k_fc1_agg_bwd<4>) against False (the torch composition): embeddings and the
    gradients of every parameter, for a fixed cotangent."""
    D, T = 172, 100
    N, E, al, be, seed, nb, bs = 300, 500, [0.1, 0.1], [0.5, 0.95], 700 + F + k, 3, 40
    src, dst, neg, ts, eidx = I.make_stream("bipartite", N, E, seed)
    w = I.model_weights(D, F, T, 2, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    dev = torch.device("cuda")
    G = [torch.from_numpy(np.random.RandomState(900 + b).standard_normal((3 * bs, 3 * D)).astype(np.float32)).to(dev)
         for b in range(nb)]
    from zebra_amd import modules
    calls = [0]
    apply = modules._NeighbourAggregate.apply

    def counted(*args):
        calls[0] += 1
        return apply(*args)

    monkeypatch.setattr(modules._NeighbourAggregate, "apply", counted)
    res, fused_calls = {}, {}
    for fused in (True, False):
        calls[0] = 0
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
        tgn.embedding_module.fused_training = fused
        assert tgn.embedding_module.fused_training_supported(3 * bs)
        tgn.train(True)
        out = []
        first = E - nb * bs
        with torch.no_grad():
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
        fused_calls[fused] = calls[0]
    assert fused_calls == {True: nb, False: 0}, fused_calls         # the fused kernels ran, once per batch
    for b in range(nb):
        ea, ga = res[True][b]
        eb, gb = res[False][b]
        assert np.abs(ea - eb).max() <= 1e-5, "embeddings of batch %d" % b
        assert set(ga) == set(gb) and len(ga) >= 8
        for pn in ga:
            _grads_agree(ga[pn], gb[pn], "%s in batch %d" % (pn, b))
    assert any(np.abs(res[True][b][1]["embedding_module.fc1.weight"]).max() > 0 for b in range(nb))


@pytest.mark.parametrize("D,F,k", [(172, 172, 20), (172, 1, 100), (256, 172, 20), (256, 1, 100)])
@pytest.mark.parametrize("N", [1, 37, 1001])
@pytest.mark.parametrize("table", [False, True])
def test_wide_d_embed_against_oracle(D, F, k, N, table, oracle):
    """zt_embed itself (embed_device) on random neighbour lists: ragged row counts (a one-row output tile, 37, 1001), with
    and without the projected table, against oracle.embed; rows whose weights are all zero included."""
    T, M = 100, 2
    nn, E1 = 3000, 4000
    seed = D + F + k + N
    w = I.model_weights(D, F, T, M, seed)
    _, efeat = I.random_tables(nn, E1, D, F, seed)
    tw = I.time_encode_weights(T)
    tgn = build_tgn(nn, E1, D, F, T, k, [0.1, 0.1], [0.5, 0.95], w, efeat).eval()
    em, mem = tgn.embedding_module, tgn.memory
    em.use_projection = table
    rng = np.random.RandomState(seed)
    memory = (rng.standard_normal((nn, D)) * 0.5).astype(np.float32)
    mem.memory.copy_(torch.from_numpy(memory).cuda())
    nodes = rng.randint(0, nn, N).astype(np.int32)
    on = rng.randint(0, nn, (M, N, k)).astype(np.int32)
    oe = rng.randint(0, E1, (M, N, k)).astype(np.int32)
    od = (rng.rand(M, N, k) * 1e5).astype(np.float32)
    ow = rng.rand(M, N, k).astype(np.float32)
    ow[:, ::5] = 0.0
    dev = torch.device("cuda")
    args = [torch.from_numpy(x).to(dev) for x in (nodes, on, oe, od, ow)]
    with torch.no_grad():
        got = em.embed_device(mem.memory, *args, memory_obj=mem).cpu().numpy()
    assert (em._proj is not None) == table
    want = oracle.embed(memory, efeat, tw, nodes, on, oe, od, ow, w, n_threads=8)
    assert got.shape == (N, D * (M + 1))
    assert np.abs(got - want).max() <= TOL


def _steps(tgn, t, bs, nbt, pipe, group=1):
    embs = []
    main = getattr(tgn, "main_stream", None) or torch.cuda.current_stream()
    with torch.cuda.stream(main):
        batches = [tuple(x[b * bs:(b + 1) * bs] for x in t) for b in range(nbt)]
        for b, cur in enumerate(batches):
            if pipe:
                embs.append(tgn.step_device(*cur, ahead=batches[b + 1:b + 1 + 3 * group]).clone())
            else:
                embs.append(tgn.step_device(*cur).clone())
    torch.cuda.synchronize()
    m = tgn.memory
    return torch.stack(embs), m.memory.clone(), m.last_update.clone(), m.messages.clone()


@pytest.mark.parametrize("strategy,group", [("streaming", 1), ("streaming", 4), ("pruning", 1), ("pruning", 4)])
def test_wide_d_pipeline_matches_sequential(strategy, group):
    """The native pipeline at D = 172 (the wide output layers held back and launched in front of k_gru<CELL, 2>, which
    keeps the projected table up to date in the same kernel) against the sequential step_device path, bit for bit over
    8 batches: embeddings, memory, last_update, messages; then zt_pipeline_run (run_device) over the same batches."""
    from zebra_amd.tppr import get_neighbor_finder
    N, D, F, T, k, al, be, seed, bs = 2000, 172, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 95, 200
    nbt = 8
    E = nbt * bs
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts)) \
        if strategy == "pruning" else None
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    outs = {}
    for mode in ("seq", "pipe", "run"):
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat, strategy=strategy, nf=nf).eval()
        if mode == "seq":
            outs[mode] = _steps(tgn, t, bs, nbt, False)
            continue
        tgn.enable_pipeline(tppr_cus=0, max_batch=bs, group=group)
        try:
            if mode == "pipe":
                outs[mode] = _steps(tgn, t, bs, nbt, True, group)
            else:
                batches = [tuple(x[b * bs:(b + 1) * bs] for x in t) for b in range(nbt)]
                out = torch.empty((nbt, 3 * bs, D * 3), dtype=torch.float32, device=t[0].device)
                with torch.cuda.stream(tgn.main_stream):
                    tgn.run_device(tgn.prepare_run(batches), out=out)
                torch.cuda.synchronize()
                m = tgn.memory
                outs[mode] = (out, m.memory.clone(), m.last_update.clone(), m.messages.clone())
        finally:
            tgn.enable_pipeline(False)
    for mode in ("pipe", "run"):
        for q in range(4):
            assert torch.equal(outs["seq"][q], outs[mode][q]), (mode, q)
    assert outs["seq"][0].abs().max() > 0 and outs["seq"][1].abs().max() > 0


def test_wide_d_pipeline_vs_protocol_oracle(oracle):
    """The native pipeline at D = 172 over 12 batches against pyoracle.ProtocolOracle (the CPU restatement of the
    reference's eval protocol): embeddings and memory within 1e-4, last_update exact."""
    N, D, F, T, k, al, be, seed, bs = 1500, 172, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 96, 200
    nbt = 12
    E = nbt * bs
    src, dst, neg, ts, eidx = I.make_stream("bipartite", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    po = oracle.ProtocolOracle(N, D, F, T, k, al, be, w, efeat, I.time_encode_weights(T), n_threads=8)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()
    tgn.enable_pipeline(tppr_cus=0, max_batch=bs)
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    batches = [tuple(x[b * bs:(b + 1) * bs] for x in t) for b in range(nbt)]
    try:
        for b, cur in enumerate(batches):
            with torch.cuda.stream(tgn.main_stream):
                emb = tgn.step_device(*cur, ahead=batches[b + 1:b + 4]).clone()
            torch.cuda.synchronize()
            s, e = b * bs, (b + 1) * bs
            want, _ = po.batch(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], False)
            assert np.abs(emb.cpu().numpy() - want).max() <= TOL, "embeddings of batch %d" % b
        m = tgn.memory
        assert np.abs(m.memory.cpu().numpy() - po.mem.memory).max() <= TOL
        assert np.array_equal(m.last_update.cpu().numpy(), po.mem.last_update)
        assert np.abs(po.mem.memory).max() > 0
    finally:
        tgn.enable_pipeline(False)


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_wide_d_protocol_golden(mode):
    """Four dependent batches of TGN.compute_temporal_embeddings at D = F = 172 against the reference's (g12_embed_d172_f172):
    probabilities of every batch, the last batch's embeddings, and after it memory, last_update, timestamps, flags and the
    message rows of the last batch's nodes."""
    N, E, D, F, T, k, al, be, seed, bs, nb = G12
    g = golden("g12_embed_d172_f172")
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    train = mode == "train"
    tgn.train(train)
    if train:
        assert tgn.embedding_module.fused_training_supported(3 * bs)
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        ctx = torch.enable_grad() if train else torch.no_grad()
        with ctx:
            se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, train)
            score = tgn.affinity_score(torch.cat([se, se], dim=0), torch.cat([de, ne])).squeeze(dim=0)
        prob = score.sigmoid().detach().cpu().numpy().ravel()
        assert np.abs(prob - g["%s_b%d_prob" % (mode, b)]).max() <= TOL, "batch %d" % b
        if b == nb - 1:
            emb = torch.cat([se, de, ne]).detach().cpu().numpy()
            assert np.abs(emb - g["%s_b%d_emb" % (mode, b)]).max() <= TOL
        if train:
            tgn.memory.detach_memory()
    m = tgn.memory
    pre = "%s_b%d_" % (mode, nb - 1)
    assert np.abs(m.memory.detach().cpu().numpy() - g[pre + "memory"]).max() <= TOL
    assert np.array_equal(m.last_update.cpu().numpy(), g[pre + "last_update"])
    assert np.array_equal(m.timestamps.cpu().numpy(), g[pre + "timestamps"])
    assert np.array_equal(m.nodes.astype(np.uint8), g[pre + "flags"])
    ids = g[pre + "msg_ids"]
    assert len(ids) > 0
    assert np.abs(m.messages.cpu().numpy()[ids] - g[pre + "msg_rows"]).max() <= TOL


def test_wide_d_training_step_matches_reference(monkeypatch):
    """A training step in the reference's style (train.py:205-215) at D = F = 172 with the fused kernels: the loss and
    every parameter gradient against the reference's (g12_train_grads_d172: values at fixed indices, row and column sums,
    max |g|)."""
    from zebra_amd import modules
    N, E, D, F, T, k, al, be, seed, bs, nb = G12
    g = golden("g12_train_grads_d172")
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    calls = [0]
    apply = modules._NeighbourAggregate.apply

    def counted(*args):
        calls[0] += 1
        return apply(*args)

    monkeypatch.setattr(modules._NeighbourAggregate, "apply", counted)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    tgn.train(True)
    crit = torch.nn.BCELoss()
    dev = torch.device("cuda")
    seen = cell = 0
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        tgn.zero_grad()
        pos, negp = tgn.compute_edge_probabilities(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
        loss = crit(pos.squeeze(), torch.ones(bs, device=dev)) + crit(negp.squeeze(), torch.zeros(bs, device=dev))
        loss.backward()
        assert abs(float(loss.item()) - float(g["b%d_loss" % b])) <= 1e-5, "loss of batch %d" % b
        grads = {pn: p.grad.detach().cpu().numpy() for pn, p in tgn.named_parameters() if p.grad is not None}
        for pn in [kk[len("b%d_at_" % b):] for kk in g.files if kk.startswith("b%d_at_" % b)]:
            assert pn in grads, pn
            got, mx = grads[pn], float(g["b%d_max_%s" % (b, pn)])
            tol = 1e-5 + 1e-4 * mx
            err = np.abs(got.ravel()[g["idx_" + pn]] - g["b%d_at_%s" % (b, pn)]).max()
            assert err <= tol, "%s in batch %d: %g" % (pn, b, err)
            assert abs(np.abs(got).max() - mx) <= tol, pn
            if got.ndim == 2:             # every element, through the sums (float32 sums of up to 616 terms in another order)
                for axis, key in ((1, "rows"), (0, "cols")):
                    d = np.abs(got.sum(axis=axis, dtype=np.float64) - g["b%d_%s_%s" % (b, key, pn)]).max()
                    assert d <= tol * got.shape[axis], "%s %s in batch %d: %g" % (pn, key, b, d)
            seen += 1
            cell += pn.startswith("memory_updater.memory_updater.")
        tgn.memory.detach_memory()
    assert calls[0] == nb                 # the fused kernels ran, once per batch
    assert seen >= 12 * nb and cell >= 4 * (nb - 1)
