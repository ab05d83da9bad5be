"""Three and more T-PPR models.  The reference takes any number of (alpha, beta) pairs (--alpha_list / --beta_list are
nargs='+'; its timing table runs 1 ... 4), the library up to 16, and M is no passive loop bound in the kernels: it enters
k_stream's work decomposition (idx / n_models, idx % n_models, blockIdx.x / n_models for the chain workgroups), the
hub-chain budget 2 grid / (3 M), the tile counts of the aggregation (tiles * M), the grids of the output layers, the gate
targets of the pipeline (B * M), row strides [M][N][k] and the scorer's width H = D (M + 1).  Everything else in the suite
runs M = 1 or 2; this file runs the same checks at M = 3, 4 and 16 -- the same references (oracle/pyoracle.py bit for bit,
oracle/aggregate_f64.py, the reference's own fixtures) at the same tolerances, through the helpers of the files that run
them at M = 2.  No number asserted here is new.
"""
import ctypes as C

import numpy as np
import pytest

import inputs as I
from conftest import golden

pytestmark = pytest.mark.gpu

# exact scaling at 0.5 and 0.25 (ties decide the top k), one alpha of 0
AL4, BE4 = [0.1, 0.1, 0.2, 0.0], [0.5, 0.95, 0.25, 0.8]
AL3, BE3 = AL4[:3], BE4[:3]
AL16, BE16 = (AL4 * 4)[:16], [0.5, 0.95, 0.25, 0.8, 0.9, 0.5, 0.7, 0.6, 0.25, 0.85, 0.5, 0.99, 0.3, 0.75, 0.5, 0.4]


@pytest.fixture(scope="module")
def zt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd import tppr
    return tppr


# ---------------------------------------------------------------------------------------------------------
# streaming T-PPR against the oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [
    dict(N=300, E=3000, bs=200, k=20, al=AL3, be=BE3, kind="general", seed=401),
    dict(N=50, E=600, bs=64, k=5, al=AL16, be=BE16, kind="general", seed=402),
    dict(N=300, E=1200, bs=200, k=64, al=AL3, be=BE3, kind="general", seed=403),       # k_stream_wide: one wavefront per model
], ids=["general-M3", "general-M16", "wide-k64-M3"])
def test_streaming_vs_oracle(zt, oracle, cfg):
    """The general queue with an odd model count, with the most models a handle takes, and the wide path: every batch's four
    arrays and every model's final state (test_tppr_gpu._streaming_vs_oracle)."""
    import test_tppr_gpu as TP
    TP._streaming_vs_oracle(zt, oracle, cfg)


def _plan_chains(f, B):
    """n_chains of the plan made last (test hook zt_test_tppr_plan_dump)."""
    from zebra_amd import _capi
    wo = np.zeros(3 * B, np.int32); pf = np.zeros_like(wo); hv = np.zeros_like(wo); own = np.zeros(B, np.int32)
    cn = np.zeros(16, np.int32); cl = np.zeros(16, np.int32); ce = np.zeros((16, 2048), np.int32); nc = np.zeros(1, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.hooks_lib().zt_test_tppr_plan_dump(f._live.h, P(wo), P(pf), P(hv), P(own), P(cn), P(cl), P(ce), P(nc)))
    return int(nc[0]), cl[:int(nc[0])].tolist()


@pytest.mark.parametrize("M,cus", [(3, 0), (4, 0), (4, 32)], ids=["M3", "M4", "M4-32cus"])
def test_hub_chains_vs_oracle(zt, oracle, M, cus):
    """Hub chains (k_stream's chain workgroups: blockIdx.x / n_models picks the chain, % n_models the model) under three and
    four models: the `hub` stream in 4096-edge launches, each launch planned ahead (plan_device), the plan read back --
    at least one launch must have picked a chain, or this case does not test what it is listed for -- and run with its token.
    cus = 32: on a stream masked to 32 compute units, as the pipeline's tppr_cus = 32 gives the T-PPR query; the first launch
    there tells the handle its stream's size, so the later plans budget 2 grid / (3 M) = 5 chains against a 32-workgroup
    grid."""
    import torch
    from zebra_amd._capi import lib, check
    import test_tppr_gpu as TP
    N, E, bs, k, seed = 400, 12288, 4096, 20, 410 + M
    al, be = AL4[:M], BE4[:M]
    src, dst, neg, ts, eidx = I.make_stream("hub", N, E, seed)
    f = zt.tppr_finder(N, k, M, al, be)
    o = oracle.TpprOracle(N, k, M, al, be)
    hs, run = C.c_void_p(), torch.cuda.current_stream()
    if cus:
        check(lib().zt_stream_create_masked(C.byref(hs), C.c_int32(0), C.c_int32(cus)))
        run = torch.cuda.ExternalStream(hs.value)
    chains = []
    try:
        for b, s in enumerate(range(0, E, bs)):
            e = s + bs
            n_d, t_d, e_d = TP._dev_batch(torch, src, dst, neg, ts, eidx, s, e)
            torch.cuda.synchronize()
            with torch.cuda.stream(run):
                tok = 0
                if not (cus and b == 0):                     # (a masked stream's first launch plans inline: it is what sizes the later plans)
                    tok = f.plan_device(n_d, e_d, 3, -1)
                    assert tok != 0
                    chains.append(_plan_chains(f, bs))
                got = f.stream_device(n_d, t_d, e_d, 3, True, -1, plan_token=tok)
            run.synchronize()
            want = o.streaming_topk(np.concatenate([src[s:e], dst[s:e], neg[s:e]]), ts[s:e], eidx[s:e])
            for x, y, nm in zip(got, want, ("nodes", "eidx", "dt", "w")):
                assert np.array_equal(x.cpu().numpy(), np.stack(y)), "%s differs in launch %d" % (nm, b)
        print("hub chains M=%d cus=%d: chains per planned launch %s, lengths %s" % (M, cus, [c[0] for c in chains], [c[1] for c in chains]))
        assert max(c[0] for c in chains) >= 1, "no launch planned a hub chain"
        if cus:
            assert max(c[0] for c in chains) <= (2 * cus) // (3 * M)
        for m in range(M):
            TP._cmp_state(f.export_state(m), o.export(m), "model %d" % m)
    finally:
        torch.cuda.synchronize()
        if cus:
            check(lib().zt_stream_destroy(hs))


@pytest.mark.parametrize("k", [20, 5])
def test_chain_head_and_lean_section(zt, oracle, k):
    """tests/test_chain_head_gpu.py's star streams under three models: chain lengths on both sides of the threshold (23: no
    chain; 24), of the scale table's first block (64, 65) and a long one, each on a fresh handle and on the state it left; then
    two hubs joined by edges that both chains hold, the first with self-loops (hops the lean section keeps), in launches whose
    prepass runs as eleven kernels."""
    import test_chain_head_gpu as CH
    for L in (23, 24, 64, 65, 200):
        spec = dict(B=L + CH.FUSED_FILL, hubs=[(0, L)])
        CH.run_case(zt, oracle, k, 6000 + L, [spec, spec], al=AL3, be=BE3)
    spec = dict(B=CH.BIG_B, hubs=[(0, 100), (1, 70)], joins=25, hub_negs=5, loops=(0, 50, 99))
    CH.run_case(zt, oracle, k, 6500, [spec, spec], al=AL3, be=BE3)


def test_other_entry_points_on_three_models(zt, oracle):
    """The finder's other entry points on one M = 3 handle, as test_streaming_wide_k_vs_oracle runs them: no_fake, the single
    model form for every m (grid and strides of one model inside a three-model state), the update-only fill, backup / restore,
    state_dict into a fresh finder, and a rejected call."""
    import test_tppr_gpu as TP
    N, E, k, seed, M = 300, 3000, 20, 420, 3
    al, be = AL3, BE3
    src, dst, neg, ts, eidx = I.make_stream("hub", N, E, seed)
    f = zt.tppr_finder(N, k, M, al, be)
    o = oracle.TpprOracle(N, k, M, al, be)
    n1 = 400
    f.compute_val_tppr(src[:n1], dst[:n1], ts[:n1], eidx[:n1], chunk=150)
    o.update_only(src[:n1], dst[:n1], ts[:n1], eidx[:n1])
    for m in range(M):
        TP._cmp_state(f.export_state(m), o.export(m), "model %d after the fill" % m)
    sl = slice(n1, 2 * n1)
    two = np.concatenate([src[sl], dst[sl]])
    a, b = f.streaming_topk_no_fake(two, ts[sl], eidx[sl]), o.streaming_topk_no_fake(two, ts[sl], eidx[sl])
    for x, y in zip(a, b):
        assert np.array_equal(np.stack(x), np.stack(y))
    bk = f.backup_tppr()
    sl = slice(2 * n1, 3 * n1)
    three = np.concatenate([src[sl], dst[sl], neg[sl]])
    want = []
    for m in range(M):
        a = f.single_streaming_topk(three, ts[sl], eidx[sl], m)
        want.append(o.single_streaming_topk(three, ts[sl], eidx[sl], m))
        for x, y in zip(a, want[m]):
            assert np.array_equal(x, y), "single model %d" % m
    for m in range(M):
        TP._cmp_state(f.export_state(m), o.export(m), "model %d" % m)
    f2 = zt.tppr_finder(N, k, M, al, be)
    f2.load_state_dict(f.state_dict(np.arange(N)))
    for m in range(M):
        TP._cmp_state(f2.export_state(m), o.export(m), "model %d after import" % m)
    f.restore_tppr(bk)
    for m in range(M):
        a = f.single_streaming_topk(three, ts[sl], eidx[sl], m)
        for x, y in zip(a, want[m]):
            assert np.array_equal(x, y), "single model %d after restore" % m
    with pytest.raises(IndexError):                                # a rejected launch: state untouched, reported
        f.streaming_topk(np.array([1, 2, N + 3], np.int32), np.array([1.0]), np.array([1], np.int64))
    sl = slice(3 * n1, 4 * n1)
    three = np.concatenate([src[sl], dst[sl], neg[sl]])
    a, b = f.streaming_topk(three, ts[sl], eidx[sl]), o.streaming_topk(three, ts[sl], eidx[sl])
    for x, y in zip(a, b):
        assert np.array_equal(np.stack(x), np.stack(y))
    for m in range(M):
        TP._cmp_state(f.export_state(m), o.export(m), "model %d at the end" % m)


def test_more_than_sixteen_models_are_refused(zt):
    """A handle takes 16 models (test_streaming_vs_oracle runs one); the seventeenth is an error, not a wrong row."""
    with pytest.raises(ValueError):
        zt.tppr_finder(50, 5, 17, [0.1] * 17, [0.5] * 17)


# ---------------------------------------------------------------------------------------------------------
# aggregation, output layers and fused training against float64 (tests/test_aggregate_f64_gpu.py's checks)
# ---------------------------------------------------------------------------------------------------------
# (form, D, F, T, k, projected table given): six of the eight aggregation forms at one shape each -- the two big-tile forms
# are left to the M = 2 cases -- and tiled_table's wide-D instantiation
EVAL_M3 = [("reg", 100, 1, 100, 20, True), ("wide", 100, 172, 100, 20, True), ("d100", 100, 172, 100, 10, True),
           ("tiled_table", 20, 7, 20, 5, True), ("tiled_full", 20, 7, 12, 5, False), ("split", 100, 1, 100, 255, False),
           ("tiled_table", 172, 172, 172, 20, True)]
# (M, D, F, T, k, p): every one with the overlay; test_aggregate_f64_cpu.py holds each to the undecided-unit caps
TRAIN_MANY = [(3, 100, 1, 100, 20, 0.0), (3, 100, 1, 100, 20, 0.1), (3, 100, 172, 100, 81, 0.0), (3, 100, 172, 100, 81, 0.1),
              (3, 20, 7, 12, 5, 0.0), (3, 20, 7, 12, 5, 0.1), (4, 100, 1, 100, 20, 0.1)]


@pytest.mark.parametrize("form,D,F,T,k,table", EVAL_M3,
                         ids=["%s-%d-%d-%d-%d-%s" % (c[0], c[1], c[2], c[3], c[4], "tab" if c[5] else "notab") for c in EVAL_M3])
def test_embed_against_float64_three_models(form, D, F, T, k, table):
    """embed_device against embed_f64 with M = 3 at N = 1 and 37 (tiles * M units, an odd count), the plan hook naming the form."""
    import test_aggregate_f64_gpu as G
    G._check_eval(form, D, F, T, k, table, Ns=(1, 37), M=3)


@pytest.mark.parametrize("form,D,F,T,k,table", [("reg", 100, 1, 100, 20, True), ("tiled_full", 128, 16, 128, 20, False)],
                         ids=["Dp112", "Dp128"])
def test_output_layers_against_float64_four_models(form, D, F, T, k, table):
    """The three output-layer forms pinned in turn with M = 4 at N = 257 (test_output_layers_against_float64): the persistent
    form's source / neighbour workgroup split (M + 2) and the latency form's grid both depend on M."""
    import test_aggregate_f64_gpu as G
    import test_launch_plan_cpu as LP
    from zebra_amd import _capi
    want = {_capi.OUT_TILED: "tiled", _capi.OUT_LATENCY: "latency", _capi.OUT_PERSIST: "persist" if D == 100 else "tiled"}
    try:
        for choice in (_capi.OUT_TILED, _capi.OUT_LATENCY, _capi.OUT_PERSIST):
            _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, choice)
            assert G._check_eval(form, D, F, T, k, table, out_choice=choice, Ns=(257,), M=4) == LP.OUT[want[choice]]
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, 0)


def test_embed_against_float64_sixteen_models():
    """The most models the library takes, on the generic tile (K1 = 39: nothing is a multiple of 16), N = 37."""
    import test_aggregate_f64_gpu as G
    G._check_eval("tiled_full", 20, 7, 12, 5, False, Ns=(37,), M=16)


@pytest.mark.parametrize("M,D,F,T,k,p", TRAIN_MANY, ids=["M%d-%d-%d-%d-%d-p%g" % c for c in TRAIN_MANY])
def test_train_aggregate_against_float64_many_models(M, D, F, T, k, p):
    """_NeighbourAggregate forward + backward with three and four models (agg_bwd: total = n_tiles * M; the dropout hash's
    index runs over [M][n][k]): test_train_aggregate_against_float64's check, unchanged."""
    import test_aggregate_f64_gpu as G
    G._check_train(D, F, T, k, p, M=M)


# ---------------------------------------------------------------------------------------------------------
# the reference's own loss and gradients with four models
# ---------------------------------------------------------------------------------------------------------
def test_training_step_gradients_match_reference_four_models():
    """test_training_step_gradients_match_reference on d20_f7_m4 (fixture g8_train_grads_m4, generated from the reference):
    loss within 1e-5, every parameter gradient within 1e-5 + 1e-4 max|ref|; the scorer is 100 wide (H = D (M + 1))."""
    import torch
    from helpers import build_tgn
    name = "d20_f7_m4"
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES[name]
    g = golden(I.TRAIN_GRAD_CASES[name])
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    tgn.train(True)
    crit = torch.nn.BCELoss()
    dev = torch.device("cuda")
    seen = 0
    for b in range(nb):
        s, e = b * bs, (b + 1) * bs
        tgn.zero_grad()
        pos, negp = tgn.compute_edge_probabilities(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
        loss = crit(pos.squeeze(), torch.ones(bs, device=dev)) + crit(negp.squeeze(), torch.zeros(bs, device=dev))
        loss.backward()
        assert abs(float(loss.item()) - float(g["b%d_loss" % b])) <= 1e-5, "loss of batch %d" % b
        for pn, p in tgn.named_parameters():
            key = "b%d_grad_%s" % (b, pn)
            if key in g.files:
                assert p.grad is not None, pn
                want = g[key]
                err = np.abs(p.grad.detach().cpu().numpy() - want).max()
                assert err <= 1e-5 + 1e-4 * np.abs(want).max(), "%s in batch %d: %g" % (pn, b, err)
                seen += 1
        tgn.memory.detach_memory()
    assert seen >= 12 * nb


# ---------------------------------------------------------------------------------------------------------
# the step, the pipeline and the scorer
# ---------------------------------------------------------------------------------------------------------
TOL = 1e-4                          # the project's tolerance for embeddings, memory and messages (tests/test_embed_gpu.py)
AL5, BE5 = AL4 + [0.3], BE4 + [0.7]
# name -> (alpha, beta, D, F, T, k, N, bs, whole batches, edges of a ragged last one, strategy, first edge)
STEP_CASES = {
    "stream_m3": (AL3, BE3, 100, 4, 100, 20, 2000, 150, 8, 50, "streaming", 0),
    # M * 3 * B * k * 4 = 1260 bytes of rows per batch: no multiple of 128, the case ADVICE.md describes for the member gate
    "gate_m3": (AL3, BE3, 20, 7, 20, 5, 60, 7, 11, 3, "streaming", 0),
    # the pruning strategy: a walk of width 10 and depth 2 over the static graph; it serves at most four models per launch
    "prune_m3": (AL3, BE3, 100, 1, 100, 20, 300, 100, 4, 0, "pruning", 1200),
    "prune_m5": (AL5, BE5, 100, 1, 100, 20, 300, 100, 4, 0, "pruning", 1200),
}
_SEQ = {}


def _step_world(name):
    import types
    al, be, D, F, T, k, N, bs, nb, tail, strategy, first = STEP_CASES[name]
    E = first + nb * bs + tail
    seed = 430 + sorted(STEP_CASES).index(name)
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    cuts = list(range(first, E, bs)) + [E]
    nf = None
    if strategy == "pruning":
        from zebra_amd.tppr import get_neighbor_finder
        nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    return dict(stream=(src, dst, neg, ts, eidx), w=w, efeat=efeat, nf=nf, E=E, spans=list(zip(cuts[:-1], cuts[1:])))


def _step_model(name, world):
    import torch
    from helpers import build_tgn
    al, be, D, F, T, k, N, bs, nb, tail, strategy, first = STEP_CASES[name]
    tgn = build_tgn(N, world["E"] + 1, D, F, T, k, al, be, world["w"], world["efeat"], strategy=strategy, nf=world["nf"]).eval()
    t = [torch.from_numpy(x).to(tgn.device) for x in world["stream"]]
    return tgn, [tuple(x[a:b] for x in t) for a, b in world["spans"]]


def _step_result(tgn, embs, strategy, M):
    import torch
    torch.cuda.synchronize()
    tgn.check_status()
    f = tgn.embedding_module.tppr_finder if strategy == "streaming" else None
    m = tgn.memory
    return dict(embs=[e.cpu().numpy() for e in embs], memory=m.memory.cpu().numpy(), last_update=m.last_update.cpu().numpy(),
                messages=m.messages.cpu().numpy(), flags=m.nodes.astype(np.uint8).copy(),
                states=[f.export_state(q) for q in range(M)] if f is not None else [])


def _sequential(oracle, name):
    """The case stepped batch by batch without the pipeline, held to ProtocolOracle: every batch's embeddings, the memory and
    the messages within 1e-4; last_update, the flags and every model's T-PPR state exactly.  Computed once per case."""
    if name in _SEQ:
        return _SEQ[name]
    al, be, D, F, T, k, N, bs, nb, tail, strategy, first = STEP_CASES[name]
    world = _step_world(name)
    src, dst, neg, ts, eidx = world["stream"]
    ref_nf = oracle.CsrOracle(src, dst, eidx, ts, N) if strategy == "pruning" else None
    p = oracle.ProtocolOracle(N, D, F, T, k, al, be, world["w"], world["efeat"], I.time_encode_weights(T), strategy, ref_nf, 10, 2,
                              n_threads=8)
    tgn, batches = _step_model(name, world)
    embs = [tgn.step_device(*cur, check_status=True).clone() for cur in batches]
    res = _step_result(tgn, embs, strategy, len(al))
    for q, (a, b) in enumerate(world["spans"]):
        want, _ = p.batch(src[a:b], dst[a:b], neg[a:b], ts[a:b], eidx[a:b], False)
        assert res["embs"][q].shape == want.shape == (3 * (b - a), D * (len(al) + 1))
        assert np.abs(res["embs"][q] - want).max() <= TOL, "%s: embeddings of batch %d" % (name, q)
    assert np.abs(res["memory"] - p.mem.memory).max() <= TOL
    assert np.abs(res["messages"] - p.mem.messages).max() <= TOL
    assert np.array_equal(res["last_update"], p.mem.last_update)
    assert np.array_equal(res["flags"], p.mem.flags)
    for m, st in enumerate(res["states"]):
        want = p.tppr.export(m)
        for kk in st:
            assert np.array_equal(st[kk], want[kk]), "%s: T-PPR state %s of model %d" % (name, kk, m)
    _SEQ[name] = (world, res)
    return _SEQ[name]


def _pipelined_equals_sequential(oracle, name, group, cus, release, look):
    import torch
    from zebra_amd import _capi
    al, be, D, F, T, k, N, bs, nb, tail, strategy, first = STEP_CASES[name]
    world, seq = _sequential(oracle, name)
    _capi.set_kernel_choice(_capi.CHOICE_GROUP_RELEASE, release)
    tgn, batches = _step_model(name, world)
    try:
        tgn.enable_pipeline(tppr_cus=cus, max_batch=max(64, bs), group=group)
        embs = []
        with torch.cuda.stream(tgn.main_stream):
            for q, cur in enumerate(batches):
                embs.append(tgn.step_device(*cur, ahead=batches[q + 1: q + 1 + look]).clone())
        got = _step_result(tgn, embs, strategy, len(al))
    finally:
        torch.cuda.synchronize()
        tgn.enable_pipeline(False)
        _capi.set_kernel_choice(_capi.CHOICE_GROUP_RELEASE, 0)
    for q in range(len(batches)):
        assert np.array_equal(got["embs"][q], seq["embs"][q]), "%s: batch %d" % (name, q)
    for kk in ("memory", "last_update", "messages", "flags"):
        assert np.array_equal(got[kk], seq[kk]), kk
    assert len(got["states"]) == len(seq["states"])
    for m, (a, b) in enumerate(zip(got["states"], seq["states"])):
        for kk in a:
            assert np.array_equal(a[kk], b[kk]), "%s: T-PPR state %s of model %d" % (name, kk, m)


def _release_launch():
    from zebra_amd import _capi
    return _capi.RELEASE_LAUNCH


@pytest.mark.parametrize("group,cus,by_launch", [(1, 0, False), (4, 0, False), (1, 32, False), (4, 32, False), (4, 0, True),
                                                 (4, 32, True)])
def test_pipelined_step_three_models(oracle, group, cus, by_launch):
    """D = T = 100, F = 4, k = 20, three models, eight batches of 150 edges and a ragged ninth: the sequential step against
    ProtocolOracle, then the native pipeline against the sequential step bit for bit -- T-PPR launches over one and over four
    batches (gate targets B * M), the T-PPR stream on the whole chip and masked to 32 compute units, the group's members
    released one by one and by the launch's event."""
    _pipelined_equals_sequential(oracle, "stream_m3", group, cus, _release_launch() if by_launch else 0, 3 * group - 1)


def test_member_gate_rows_not_a_multiple_of_128_bytes(oracle):
    """M = 3, k = 5, bs = 7, D = 20 in groups of four: a batch's block of rows is 1260 bytes per array."""
    assert (3 * 3 * 7 * 5 * 4) % 128 != 0
    _pipelined_equals_sequential(oracle, "gate_m3", 4, 0, 0, 11)


@pytest.mark.parametrize("name", ["prune_m3", "prune_m5"])
def test_pruning_through_the_pipeline(oracle, name):
    """The pruning strategy with three models (one walk) and five (two launches: four models, then one) against the oracle's
    protocol, and pipelined against sequential."""
    _pipelined_equals_sequential(oracle, name, 1, 0, 0, 2)


@pytest.mark.parametrize("bs", [400, 150], ids=["k_out_gru", "k_out_gru2"])
def test_fused_output_and_gru_launch_four_models(bs):
    """test_fused_output_and_gru_launch_matches_separate_kernels with four models: the grid of k_out_gru counts out_tiles (M + 1)
    workgroups in front of the GRU's, k_out_gru2 per_path M neighbour-path units."""
    import test_embed_gpu as TE
    TE.test_fused_output_and_gru_launch_matches_separate_kernels(1, bs, 100, al=AL4, be=BE4)


@pytest.mark.parametrize("M", [3, 4])
def test_scoring_and_metrics_through_the_pipeline(M):
    """enable_scoring with H = 400 and 500, the widths between and beyond the two specialised scorers: the plan names a generic
    form; every step's probabilities are score_device's on the embeddings it returned bit for bit and lie within 1e-4 of a
    float64 MergeLayer; per-batch (AP, AUC, accuracy) of the native batch loop equal those of the stepped batches."""
    import torch
    from helpers import build_tgn
    from zebra_amd import _capi, evaluation as ev
    from zebra_amd.modules import MergeLayer
    D = T = 100
    N, F, k, bs, nb, seed = 2000, 1, 20, 150, 5, 440 + M
    al, be = AL4[:M], BE4[:M]
    H = D * (M + 1)
    out = (C.c_int64 * 7)()
    _capi.check(_capi.hooks_lib().zt_test_affinity_plan(C.c_int64(bs), C.c_int32(H), C.c_int32(0), out))
    assert out[0] in (3, 4), "H = %d is scored by form %d, not by a generic one" % (H, out[0])     # GEN_LATENCY, GEN_TILED
    E = nb * bs - 30                                                                                # (a ragged last batch)
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, M, seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    ref64 = MergeLayer(H, H, H, 1).double()
    with torch.no_grad():
        for p, name in zip((ref64.fc1.weight, ref64.fc1.bias, ref64.fc2.weight, ref64.fc2.bias), ("aff1_w", "aff1_b", "aff2_w", "aff2_b")):
            p.copy_(torch.from_numpy(w[name]).double())
    res = {}
    for mode in ("step", "run"):
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()
        tgn.enable_pipeline(tppr_cus=0, max_batch=256, group=2)
        try:
            tgn.enable_scoring()
            t = [torch.from_numpy(x).to(tgn.device) for x in (src, dst, neg, ts, eidx)]
            batches = [tuple(x[s:s + bs] for x in t) for s in range(0, E, bs)]
            with torch.cuda.stream(tgn.main_stream):
                if mode == "run":
                    tgn.enable_metrics(per_batch=nb)
                    tgn.run_device(tgn.prepare_run(batches))
                    _, n, rows = tgn.metrics()
                    assert n == nb
                    res[mode] = rows.clone()
                else:
                    rows = []
                    for q, cur in enumerate(batches):
                        emb = tgn.step_device(*cur, ahead=batches[q + 1: q + 6])
                        B = cur[0].numel()
                        prob = tgn.last_prob().clone()
                        assert prob.shape == (2 * B,) and torch.equal(prob, tgn.score_device(emb)), "batch %d" % q
                        e64 = emb.double().cpu()
                        with torch.no_grad():
                            want = ref64(torch.cat([e64[:B], e64[:B]]), e64[B:]).squeeze(1).sigmoid()
                        err = float((prob.double().cpu() - want).abs().max())
                        print("scoring M=%d H=%d batch %d: max |prob - float64| = %.3g" % (M, H, q, err))
                        assert err <= TOL, "batch %d" % q
                        rows.append(ev.link_metrics(prob[:B], prob[B:]).clone())
                    res[mode] = torch.stack(rows)
            torch.cuda.synchronize()
            tgn.check_status()
        finally:
            tgn.enable_pipeline(False)
    assert torch.equal(res["run"].cpu(), res["step"].cpu())


def test_training_scorer_at_three_models_width():
    """_HipLinkScore forward and backward at H = 400 against a float64 MergeLayer (test_hip_link_score_against_float64)."""
    import test_scoring_train_gpu as ST
    ST.test_hip_link_score_against_float64(200, 400)


def test_sharded_step_three_models():
    """Two ranks sharing the GPU, the native pipeline with T-PPR launches over two batches, three models: every rank's rows,
    the memory tables and the T-PPR state equal the single run's (test_sharded_equals_single)."""
    import test_distributed_gpu as DG
    DG.test_sharded_equals_single(2, "streaming_pipe_m3")


# ---------------------------------------------------------------------------------------------------------
# soaks: the seeds that draw three and four models
# ---------------------------------------------------------------------------------------------------------
def _soak_seeds(n):
    import soak_tppr
    seeds = range(soak_tppr.MANY_MODELS_SEED, soak_tppr.MANY_MODELS_SEED + n)
    drawn = {soak_tppr.many_models(s, [0.1], [0.5])[0] for s in seeds if soak_tppr.many_models(s, [0.1], [0.5])}
    assert drawn == {3, 4}
    return seeds


def test_randomised_soak_many_models(zt, oracle):
    """A slice of tests/soak_tppr.py over the seeds that draw three or four models now and then."""
    import soak_tppr
    for seed in _soak_seeds(16):
        err = soak_tppr.one(seed, zt, oracle)
        assert err is None, err


def test_randomised_pipeline_soak_many_models(oracle):
    """The same of tests/soak_pipeline.py."""
    import torch
    import soak_pipeline
    for seed in _soak_seeds(12):
        err = soak_pipeline.one(seed, torch, oracle)
        assert err is None, err


def test_randomised_training_soak_many_models():
    """The same of tests/soak_train.py."""
    import torch
    import soak_train
    for seed in _soak_seeds(16):
        err = soak_train.one(seed, torch)
        assert err is None, err
