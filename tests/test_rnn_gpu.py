"""The RNN memory updater on the device (RNNMemoryUpdater; the reference's `--memory_updater rnn`,
modules/memory_updater.py:100-103): zt_rnn_update's kernel forms against torch.nn.RNNCell and each other, the fused output
layers + update launch against the separate kernels, the reference fixtures g11_rnn_*, the training kernels
(zt_rnn_train_forward / _backward), the native pipeline (zt_pipeline_set_cell) against the sequential path and the CPU
oracle, and a pipeline switched between the cells."""
import numpy as np
import pytest
import torch

import inputs as I
from conftest import golden
from helpers import load_weights, make_args

pytestmark = pytest.mark.gpu

TOL = 1e-4                  # the g45_embed_* tests' tolerance


def rnn_weights(D, msg, seed):
    rng = np.random.RandomState(seed)
    s = 1.0 / np.sqrt(D)
    u = lambda *shape: rng.uniform(-s, s, shape).astype(np.float32)
    return dict(w_ih=u(D, msg), w_hh=u(D, D), b_ih=u(D), b_hh=u(D))


def build_rnn_tgn(N, E1, D, F, T, k, al, be, w, rw, efeat, strategy="streaming", nf=None):
    """helpers.build_tgn with memory_updater_type="rnn"; rw: the RNNCell's weights (w_ih [D][msg], ...)."""
    from zebra_amd.tgn import TGN
    tgn = TGN(neighbor_finder=nf, node_features=None, edge_features=efeat, device="cuda", n_layers=2, n_heads=2,
              dropout=0.0, use_memory=True, node_dimension=D, time_dimension=T, memory_dimension=D,
              embedding_module_type="diffusion", message_function="identity", aggregator_type="last",
              memory_updater_type="rnn", n_neighbors=10, args=make_args(N, E1, k, al, be, strategy))
    w = dict(w)
    w.update(rw)
    return load_weights(tgn.to("cuda"), w)


def rnn_cell(rw, dtype=torch.float32):
    D, msg = rw["w_ih"].shape
    cell = torch.nn.RNNCell(msg, D).to(dtype)
    with torch.no_grad():
        for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            getattr(cell, name).copy_(torch.from_numpy(rw[key]).to(dtype))
    return cell


# ---------------------------------------------------------------------------------------------------------
# 1. the kernel forms of zt_rnn_update
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,n", [(172, 400), (172, 37), (1, 512), (1, 2000), (4, 1), (1, 8192), (172, 1203)])
def test_rnn_kernels_agree(F, n):
    """k_gru<CELL_RNN> (tile) and k_gru_split<CELL_RNN> (split), pinned one after the other, and the library's pick,
    against torch's RNNCell on the same flagged rows: memory, last_update, flags cleared, untouched rows, and the
    projected table kept up to date from the rows the update reports."""
    from zebra_amd import _capi
    D = T = 100
    N, E1 = 12000, 100
    msg_dim = 2 * D + F + T
    w = I.model_weights(D, F, T, 2, 31)
    rw = rnn_weights(D, msg_dim, 31 + F)
    _, efeat = I.random_tables(N, E1, D, F, 31)
    g = torch.Generator().manual_seed(F + n)
    msg = torch.randn((N, msg_dim), generator=g)
    mem0 = torch.randn((N, D), generator=g) * 0.3
    ts = torch.rand(N, generator=g) * 1e6
    ids = (torch.randperm(N - 1, generator=g)[:n] + 1).to(torch.int32)
    outs = {}
    tgn = build_rnn_tgn(N, E1, D, F, T, 20, [0.1, 0.1], [0.5, 0.95], w, rw, efeat).eval()
    em, m = tgn.embedding_module, tgn.memory
    try:
        for mode, choice in (("tile", _capi.GRU_TILE), ("split", _capi.GRU_SPLIT), ("auto", 0)):
            _capi.set_kernel_choice(_capi.CHOICE_GRU, choice)
            m.messages.copy_(msg.cuda()); m.memory.copy_(mem0.cuda()); m.timestamps.copy_(ts.cuda())
            m.last_update.zero_()
            ids_d = ids.cuda()
            m._flag_buf[ids_d.long()] = 1
            table = em._projection(m)                       # the projected table follows the update
            tgn.memory_updater.update_device(m, ids_d, ids_d.numel())
            torch.cuda.synchronize()
            o = outs[mode] = dict(mem=m.memory.cpu().numpy(), lu=m.last_update.cpu().numpy(),
                                  flags=m._flag_buf.cpu().numpy()[:N])
            if table is not None:                           # the rows the update reported, against a rebuild of every row
                o["table"] = em._projection(m).clone()
                em.invalidate_projection()
                o["full"] = em._projection(m).clone()
                torch.cuda.synchronize()
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_GRU, 0)
    with torch.no_grad():
        want = mem0.clone()
        want[ids.long()] = rnn_cell(rw)(msg[ids.long()], mem0[ids.long()])
    for mode, o in outs.items():
        assert np.abs(o["mem"] - want.numpy()).max() <= 1e-5, mode
        lu = np.zeros(N, np.float32); lu[ids.numpy()] = ts.numpy()[ids.numpy()]
        assert np.array_equal(o["lu"], lu), mode
        assert not o["flags"].any(), mode
        rest = np.ones(N, bool); rest[ids.numpy()] = False
        assert np.array_equal(o["mem"][rest], mem0.numpy()[rest]), mode
        if "table" in o:
            assert torch.equal(o["table"], o["full"]), mode
    # (the two forms sum the pre-activation in different orders; unlike the GRU's, the RNN's output is that sum through tanh
    #  alone, with no gate to scale the difference down: measured up to 2.7e-6 where the GRU's stays within 2e-6)
    assert np.abs(outs["split"]["mem"] - outs["tile"]["mem"]).max() <= 4e-6


# ---------------------------------------------------------------------------------------------------------
# 2. the output layers beside the update in one launch
# ---------------------------------------------------------------------------------------------------------
def _steps(tgn, t, bs, nbt, pipe, ahead=False):
    embs = []
    main = getattr(tgn, "main_stream", None) or torch.cuda.current_stream()
    with torch.cuda.stream(main):
        batches = [tuple(x[b * bs:(b + 1) * bs] for x in t) for b in range(nbt)]
        for b, cur in enumerate(batches):
            if pipe and ahead:
                embs.append(tgn.step_device(*cur, ahead=batches[b + 1:]).clone())
            else:
                nxt = batches[b + 1] if (pipe and b + 1 < nbt) else None
                embs.append(tgn.step_device(*cur, prefetch=nxt).clone())
    torch.cuda.synchronize()
    m = tgn.memory
    return (torch.stack(embs).cpu().numpy(), m.memory.cpu().numpy(), m.last_update.cpu().numpy(), m.messages.cpu().numpy())


@pytest.mark.parametrize("F,bs", [(1, 400), (172, 400), (1, 150), (172, 150)])
def test_fused_output_and_rnn_launch_matches_separate_kernels(F, bs):
    """k_out_gru<CELL_RNN> (bs = 400: tiled output kernel, 16-row tiles) and k_out_gru2<CELL_RNN> (bs = 150: the
    latency-organised forms) of a pipelined step against the sequential path, which launches the output layers and the
    RNN update one after the other: every batch's embeddings, memory, last_update -- bit for bit."""
    N, D, T, k, al, be, seed = 3000, 100, 100, 20, [0.1, 0.1], [0.5, 0.95], 91
    nbt = 5
    E = nbt * bs
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    rw = rnn_weights(D, 2 * D + F + T, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    outs = {}
    for mode in ("seq", "pipe"):
        tgn = build_rnn_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat).eval()
        if mode == "pipe":
            tgn.enable_pipeline(tppr_cus=0, max_batch=bs)
        outs[mode] = _steps(tgn, t, bs, nbt, mode == "pipe")
        tgn.enable_pipeline(False)
    for q in range(3):
        assert np.array_equal(outs["seq"][q], outs["pipe"][q]), q
    assert np.abs(outs["seq"][0]).max() > 0


# ---------------------------------------------------------------------------------------------------------
# 3. the reference's fixtures
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", ["d20_f7", "d100_f172"])
def test_rnn_protocol_golden(name, mode):
    """Consecutive batches of TGN.compute_temporal_embeddings with the RNN updater against the reference's
    (g11_rnn_embed_*, generated from the reference with memory_updater_type="rnn")."""
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES[name]
    g = golden("g11_rnn_embed_" + name)
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    rw = {kk: g["rnn_" + kk] for kk in ("w_ih", "w_hh", "b_ih", "b_hh")}
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_rnn_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat)
    train = mode == "train"
    tgn.train(train)
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        ctx = torch.enable_grad() if train else torch.no_grad()
        with ctx:
            se, de, ne = tgn.compute_temporal_embeddings(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, train)
            score = tgn.affinity_score(torch.cat([se, se], dim=0), torch.cat([de, ne])).squeeze(dim=0)
        emb = torch.cat([se, de, ne]).detach().cpu().numpy()
        assert np.abs(emb - g["%s_b%d_emb" % (mode, b)]).max() <= TOL, "batch %d" % b
        prob = score.sigmoid().detach().cpu().numpy().ravel()
        assert np.abs(prob - g["%s_b%d_prob" % (mode, b)]).max() <= TOL, "batch %d" % b
        if train:
            tgn.memory.detach_memory()
    m = tgn.memory
    pre = "%s_b%d_" % (mode, nb - 1)
    assert np.abs(m.memory.detach().cpu().numpy() - g[pre + "memory"]).max() <= TOL
    assert np.array_equal(m.last_update.cpu().numpy(), g[pre + "last_update"])
    assert np.abs(m.messages.cpu().numpy() - g[pre + "messages"]).max() <= TOL
    assert np.array_equal(m.timestamps.cpu().numpy(), g[pre + "timestamps"])
    assert np.array_equal(m.nodes.astype(np.uint8), g[pre + "flags"])


# ---------------------------------------------------------------------------------------------------------
# 4. training
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,D,msg", [(1, 20, 67), (37, 100, 472), (600, 100, 301)])
def test_hip_rnn_rows_forward_and_backward(U, D, msg):
    """_HipRnnRows (zt_rnn_train_forward / _backward) against a float64 RNNCell under autograd."""
    from zebra_amd.modules import _HipRnnRows
    g = torch.Generator().manual_seed(U + D)
    N = 2 * U + 5
    messages = torch.randn((N, msg), generator=g).cuda()
    memory = (torch.randn((N, D), generator=g) * 0.5).cuda()
    ids = (torch.randperm(N, generator=g)[:U]).to(torch.int32).cuda()
    rw = rnn_weights(D, msg, U)
    params = [torch.from_numpy(rw[kk]).cuda().requires_grad_(True) for kk in ("w_ih", "w_hh", "b_ih", "b_hh")]
    h = _HipRnnRows.apply(*params, messages, memory, ids)
    dh = torch.randn((U, D), generator=g).cuda()
    h.backward(dh)
    cell = rnn_cell(rw, torch.float64)
    x, hx = messages[ids.long()].double().cpu(), memory[ids.long()].double().cpu()
    want = cell(x, hx)
    want.backward(dh.double().cpu())
    assert np.abs(h.detach().cpu().numpy() - want.detach().numpy()).max() <= 1e-5
    for p, q in zip(params, (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)):
        ref = q.grad.numpy()
        assert np.abs(p.grad.cpu().numpy() - ref).max() <= 1e-5 + 1e-5 * np.abs(ref).max()


def _train_step(tgn, stream, bs, nb, grads=None):
    src, dst, neg, ts, eidx = stream
    crit = torch.nn.BCELoss()
    dev = torch.device("cuda")
    out = []
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        tgn.zero_grad()
        pos, negp = tgn.compute_edge_probabilities(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
        loss = crit(pos.squeeze(), torch.ones(bs, device=dev)) + crit(negp.squeeze(), torch.zeros(bs, device=dev))
        loss.backward()
        out.append((float(loss.item()), {pn: p.grad.detach().cpu().numpy().copy() for pn, p in tgn.named_parameters()
                                         if p.grad is not None}))
        tgn.memory.detach_memory()
    return out


def test_rnn_training_step_gradients_match_reference():
    """A training step in the reference's style (train.py:205-215) with the RNN updater: loss and every parameter
    gradient, the RNNCell's included, against the reference's (g11_rnn_train_grads)."""
    name = "d20_f7"
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES[name]
    g = golden("g11_rnn_train_grads")
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    rw = {kk: g["rnn_" + kk] for kk in ("w_ih", "w_hh", "b_ih", "b_hh")}
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_rnn_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat)
    tgn.train(True)
    seen = cell = 0
    for b, (loss, grads) in enumerate(_train_step(tgn, stream, bs, nb)):
        assert abs(loss - float(g["b%d_loss" % b])) <= 1e-5, "loss of batch %d" % b
        for pn in [kk[len("b%d_grad_" % b):] for kk in g.files if kk.startswith("b%d_grad_" % b)]:
            assert pn in grads, pn
            want = g["b%d_grad_%s" % (b, pn)]
            err = np.abs(grads[pn] - want).max()
            assert err <= 1e-5 + 1e-4 * np.abs(want).max(), "%s in batch %d: %g" % (pn, b, err)
            seen += 1
            cell += pn.startswith("memory_updater.memory_updater.")
    assert seen >= 12 * nb and cell >= 4 * (nb - 1)


def test_rnn_fused_training_equals_torch_composition():
    """fused_training=True (the HIP kernels, _HipRnnRows) against False (torch ops on the RNNCell module) on the same
    steps: losses and gradients within rounding."""
    name = "d100_f172"
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES[name]
    stream = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    rw = rnn_weights(D, 2 * D + F + T, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    res = {}
    for fused in (True, False):
        tgn = build_rnn_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat)
        tgn.embedding_module.fused_training = fused
        tgn.train(True)
        res[fused] = _train_step(tgn, stream, bs, nb)
    for (la, ga), (lb, gb) in zip(res[True], res[False]):
        assert abs(la - lb) <= 1e-5
        assert sorted(ga) == sorted(gb)
        for pn in ga:
            assert np.abs(ga[pn] - gb[pn]).max() <= 1e-5 + 1e-4 * np.abs(gb[pn]).max(), pn
    assert any(pn.startswith("memory_updater.") for pn in res[True][-1][1])


# ---------------------------------------------------------------------------------------------------------
# 5. the native pipeline
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_rnn_pipeline_matches_sequential(group):
    """enable_pipeline with an RNN updater (zt_pipeline_set_cell) against the sequential step_device path, bit for bit
    over 8 batches: embeddings, memory, last_update, messages."""
    N, D, F, T, k, al, be, seed, bs = 2000, 100, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 93, 200
    nbt = 8
    E = nbt * bs
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    rw = rnn_weights(D, 2 * D + F + T, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    outs = {}
    for mode in ("seq", "pipe"):
        tgn = build_rnn_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat).eval()
        if mode == "pipe":
            tgn.enable_pipeline(tppr_cus=0, max_batch=bs, group=group)
        outs[mode] = _steps(tgn, t, bs, nbt, mode == "pipe", ahead=True)
        tgn.enable_pipeline(False)
    for q in range(4):
        assert np.array_equal(outs["seq"][q], outs["pipe"][q]), q


def test_rnn_pipeline_vs_oracle_c2_shape(oracle):
    """The native pipeline with the RNN updater over 24 batches at C2's shape (D = T = 100, F = 172, k = 20, two T-PPR
    models, bs = 200) against the CPU oracle's protocol with its memory update replaced by a NumPy RNNCell."""
    N, D, F, T, k, al, be, seed, bs = 1500, 100, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 94, 200
    nbt = 24
    E = nbt * bs
    src, dst, neg, ts, eidx = I.make_stream("bipartite", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    rw = rnn_weights(D, 2 * D + F + T, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    ow = dict(w)
    ow.update(rw)
    po = oracle.ProtocolOracle(N, D, F, T, k, al, be, ow, efeat, I.time_encode_weights(T), n_threads=8)

    def rnn_update(gru, ids=None, n_threads=1):                 # SequenceMemoryUpdater + nn.RNNCell, float32
        m = po.mem
        v = np.arange(m.n_nodes) if ids is None else np.unique(np.asarray(ids))
        v = v[m.flags[v] != 0]
        if len(v):
            x = m.messages[v] @ rw["w_ih"].T + rw["b_ih"]
            h = m.memory[v] @ rw["w_hh"].T + rw["b_hh"]
            m.memory[v] = np.tanh(x + h).astype(np.float32)
            m.last_update[v] = m.timestamps[v]
        if ids is None:
            m.flags[:] = 0
        else:
            m.flags[np.asarray(ids)] = 0
        return len(v)

    tgn = build_rnn_tgn(N, E + 1, D, F, T, k, al, be, w, rw, efeat).eval()
    tgn.enable_pipeline(tppr_cus=0, max_batch=bs)
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    batches = [tuple(x[b * bs:(b + 1) * bs] for x in t) for b in range(nbt)]
    worst = 0.0
    po.mem.gru_update = rnn_update
    try:
        for b, cur in enumerate(batches):
            with torch.cuda.stream(tgn.main_stream):
                emb = tgn.step_device(*cur, ahead=batches[b + 1:b + 4]).clone()
            torch.cuda.synchronize()
            s, e = b * bs, (b + 1) * bs
            want, _ = po.batch(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], False)
            worst = max(worst, float(np.abs(emb.cpu().numpy() - want).max()))
            assert worst <= TOL, "embeddings of batch %d" % b
        m = tgn.memory
        assert np.abs(m.memory.cpu().numpy() - po.mem.memory).max() <= TOL
        assert np.array_equal(m.last_update.cpu().numpy(), po.mem.last_update)
        assert np.abs(po.mem.memory).max() > 0
    finally:
        tgn.enable_pipeline(False)


# ---------------------------------------------------------------------------------------------------------
# 6. switching the cell of a live pipeline
# ---------------------------------------------------------------------------------------------------------
def test_pipeline_switched_gru_rnn_gru_equals_one_never_switched():
    """One pipeline runs GRU steps, then (the memory updater swapped for an RNNMemoryUpdater that shares the GRU's
    workspace) RNN steps, then GRU steps again.  The RNN steps repack the shared workspace with the RNN's one gate;
    after the switch back the pipeline must repack the GRU and give the bits of a pipeline that never switched,
    started from the same tables."""
    from zebra_amd.modules import RNNMemoryUpdater
    N, D, F, T, k, al, be, seed, bs = 2000, 100, 172, 100, 20, [0.1, 0.1], [0.5, 0.95], 95, 200
    n1, n2, n3 = 3, 3, 4
    nbt = n1 + n2 + n3
    E = nbt * bs
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    rw = rnn_weights(D, 2 * D + F + T, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    from helpers import build_tgn
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    batches = [tuple(x[b * bs:(b + 1) * bs] for x in t) for b in range(nbt)]
    a = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()       # switches
    b = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()       # never switches
    for x in (a, b):
        x.enable_pipeline(tppr_cus=0, max_batch=bs)
    gru = a.memory_updater
    rnn = RNNMemoryUpdater(gru.message_dimension, D, "cuda").cuda()
    with torch.no_grad():
        for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            getattr(rnn.memory_updater, name).copy_(torch.from_numpy(rw[key]))
    rnn._ws = gru._workspace(2 * bs, D)                                  # the same workspace: the RNN's packing overwrites the GRU's

    def run(x, lo, hi):
        out = []
        with torch.cuda.stream(x.main_stream):
            for q in range(lo, hi):
                out.append(x.step_device(*batches[q], ahead=batches[q + 1:min(hi, q + 4)]).clone())
        torch.cuda.synchronize()
        return out

    try:
        run(a, 0, n1)
        run(b, 0, n1)
        a.memory_updater = rnn
        rnn_embs = run(a, n1, n1 + n2)
        run(b, n1, n1 + n2)                                             # (b's T-PPR state follows the same edges)
        a.memory_updater = gru
        # b starts from a's tables; in place, so b's pipeline keeps its pointers (the version bump repacks its weights too)
        with torch.no_grad():
            for name in ("memory", "last_update", "messages", "timestamps", "_flag_buf"):
                getattr(b.memory, name).copy_(getattr(a.memory, name))
        ea, eb = run(a, n1 + n2, nbt), run(b, n1 + n2, nbt)
        for p, q in zip(ea, eb):
            assert torch.equal(p, q)
        for name in ("memory", "last_update", "messages"):
            assert torch.equal(getattr(a.memory, name), getattr(b.memory, name)), name
        assert torch.cat(rnn_embs).abs().max() > 0
    finally:
        a.enable_pipeline(False)
        b.enable_pipeline(False)
