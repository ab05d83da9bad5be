"""Read-only queries and ranking on the GPU: zt_tppr_query against the reference's stream fixtures and against the stream's
own emission, TGN.embed_nodes against the eval step, zt_affinity_rank against a float64 MergeLayer and against the pair scorer,
zt_rank_metrics against numpy, TGN.rank_candidates / evaluation.eval_edge_ranking against a restatement.

Largest |prob - float64 MergeLayer| per shape, measured on an MI355X (printed by test_rank_scorer_matches_float64): DESIGN.md,
"Read-only queries and ranking"."""
import functools
import types

import numpy as np
import pytest
import torch

import inputs as I
from conftest import golden
from helpers import build_tgn
from helpers_query import comparable, merge_f64, rank_cases, rank_of_positive, rank_sums

pytestmark = pytest.mark.gpu
TOL = 1e-4            # the project's tolerance for a probability (tests/test_scoring_wide_gpu.py)
FORM_TOL = 1e-5       # two float32 associations of the same sums (that file's FORM_TOL)
RK_HC = 1024          # csrc/rank.hip: columns of H per LDS chunk; 1028 is the smallest width above it


@pytest.fixture(scope="module")
def zt():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd import tppr
    return tppr


def _batches(E, bs):
    return [(s, min(E, s + bs)) for s in range(0, E, bs)]


def _stack(lists):
    return [np.stack(x) for x in lists]


# ---- 4. query rows against the reference's fixtures ---------------------------------------------------------------------
@pytest.mark.parametrize("name,floor,exact", [("tiny_general", 0.75, False), ("bs1_single", 1.0, True), ("gen_m3", 0.75, False)])
def test_query_rows_match_the_reference_fixtures(zt, name, floor, exact):
    kind, N, E, seed, bs, k, al, be, _ = I.STREAM_CASES[name]
    g = golden("g1_stream_" + name)
    src, dst, neg, ts, eidx = I.make_stream(kind, N, E, seed)
    f = zt.tppr_finder(N, k, len(al), al, be)
    seen = cmp = 0
    for b, (s, e) in enumerate(_batches(E, bs)):
        nodes = np.concatenate([src[s:e], dst[s:e], neg[s:e]])
        t3 = np.concatenate([ts[s:e]] * 3)
        ok = comparable(src[s:e], dst[s:e], neg[s:e])
        got = _stack(f.query_topk(nodes, t3))
        for a, key in zip(got, ("nodes", "eidx", "dt", "w")):
            want = g["b%d_%s" % (b, key)]
            assert a.dtype == want.dtype and a.shape == want.shape
            assert np.array_equal(a[:, ok].view(np.uint32), want[:, ok].view(np.uint32)), (name, b, key)
        seen += len(ok)
        cmp += int(ok.sum())
        # the query has not disturbed the stream
        on, oe, od, ow = f.streaming_topk(nodes, t3, eidx[s:e])
        arrs = []
        for m in range(len(al)):
            arrs += [on[m], oe[m], od[m], ow[m]]
        assert I.digest(arrs) == str(g["digests"][b]), "batch %d differs from the reference" % b
    share = cmp / seen
    print("%s: %d of %d rows compared (%.3f)" % (name, cmp, seen, share))
    assert share == 1.0 if exact else share >= floor


# ---- 5. query rows against the stream's own emission --------------------------------------------------------------------
def _query_then_stream(zt, N, k, al, be, streams, bs):
    src, dst, neg, ts, eidx = streams
    f, twin = zt.tppr_finder(N, k, len(al), al, be), zt.tppr_finder(N, k, len(al), al, be)
    seen = cmp = 0
    for s, e in _batches(len(src), bs):
        nodes = np.concatenate([src[s:e], dst[s:e], neg[s:e]])
        t3 = np.concatenate([ts[s:e]] * 3)
        ok = comparable(src[s:e], dst[s:e], neg[s:e])
        got = _stack(f.query_topk(nodes, t3))
        want = _stack(f.streaming_topk(nodes, t3, eidx[s:e]))
        twin.streaming_topk(nodes, t3, eidx[s:e])
        for a, b_, key in zip(got, want, ("nodes", "eidx", "dt", "w")):
            assert np.array_equal(a[:, ok].view(np.uint32), b_[:, ok].view(np.uint32)), (s, key)
        seen += len(ok)
        cmp += int(ok.sum())
    for m in range(len(al)):
        a, b_ = f.export_state(m), twin.export_state(m)
        for kk in a:
            assert np.array_equal(a[kk], b_[kk]), "the queries changed state %s of model %d" % (kk, m)
    return f, cmp / seen


@pytest.mark.parametrize("name,floor", [("gen_k40", 0.35), ("hub_m4", 0.5)])
def test_query_rows_match_the_streams_emission(zt, name, floor):
    kind, N, E, seed, bs, k, al, be, _ = I.STREAM_CASES[name]
    _, share = _query_then_stream(zt, N, k, al, be, I.make_stream(kind, N, E, seed), bs)
    print("%s: share of rows compared %.3f" % (name, share))
    assert share >= floor


@pytest.mark.parametrize("k", [5, 64, 100])
def test_query_wide_k_and_edge_cases(zt, k):
    """k = 64, 100: the strided form beyond a wavefront (k = 5: the same cases on the wave-per-row form).  Then one model
    alone, N = 1, N = 0, node 0 (never an endpoint: an empty row), a node the stream never touched, and an id == num_nodes."""
    N, al, be = 62, [0.1, 0.2], [0.5, 0.9]                       # ids 1 .. 59 carry edges; 0, 60, 61 never do
    streams = I.make_stream("general", 60, 300, 300 + k)
    f, share = _query_then_stream(zt, N, k, al, be, streams, 25)
    assert share > 0.2
    dev = torch.device("cuda")
    t_end = float(streams[3][-1]) + 5.0
    nodes = torch.tensor([3, 0, 61, 7, 1], dtype=torch.int32, device=dev)
    tsq = torch.full((5,), t_end, dtype=torch.float64, device=dev)
    both = [x.cpu().numpy() for x in f.query_device(nodes, tsq)]
    assert both[0].shape == (2, 5, k)
    one = [x.cpu().numpy() for x in f.query_device(nodes, tsq, model=1)]
    for a, b_ in zip(both, one):
        assert b_.shape == (1, 5, k) and np.array_equal(a[1].view(np.uint32), b_[0].view(np.uint32))
    for a in both:                                               # node 0 and the untouched node: empty dictionaries
        assert not a[:, 1].any() and not a[:, 2].any()
    st = f.export_rows(0, [3])
    n3 = int(st["len"][0])
    assert n3 > 0 and np.array_equal(both[0][0, 0, :n3], st["node"][0, :n3].astype(np.int32))
    assert np.all(both[2][0, 0, n3:] == np.float32(t_end)) and not both[3][0, 0, n3:].any()   # beyond len: 0, 0, f32(t), 0
    single = [x.cpu().numpy() for x in f.query_device(nodes[:1], tsq[:1])]
    for a, b_ in zip(both, single):
        assert np.array_equal(a[:, :1].view(np.uint32), b_.view(np.uint32))
    empty = f.query_device(nodes[:0], tsq[:0])
    assert all(x.shape == (2, 0, k) for x in empty)
    # an id == num_nodes: an all-zero row, IndexError with check_status, the other rows right
    bad = torch.tensor([3, N, 7], dtype=torch.int32, device=dev)
    rows = [x.cpu().numpy() for x in f.query_device(bad, tsq[:3], check_status=False)]
    for a, b_ in zip(rows, both):
        assert not a[:, 1].any()
        assert np.array_equal(a[:, 0].view(np.uint32), b_[:, 0].view(np.uint32))
        assert np.array_equal(a[:, 2].view(np.uint32), b_[:, 3].view(np.uint32))
    with pytest.raises(IndexError):
        f.query_device(bad, tsq[:3], check_status=True)
    f.query_device(nodes, tsq, check_status=True)                # the status word was cleared
    f.check_status()                                             # ... and the handle's latch was never involved


# ---- 6. embed_nodes ------------------------------------------------------------------------------------------------------
def _model_state(tgn):
    m = tgn.memory
    st = {kk: getattr(m, kk).cpu().numpy().copy() for kk in ("memory", "last_update", "messages", "timestamps", "_flag_buf")}
    em = tgn.embedding_module
    if em.tppr_strategy == "streaming":
        for mi in range(em.n_tppr):
            for kk, v in em.tppr_finder.export_state(mi).items():
                st["tppr%d_%s" % (mi, kk)] = v
    st["batch_counter"] = np.int64(tgn.batch_counter)
    return st


@pytest.mark.parametrize("D,F,T,k,al,be", [(20, 7, 20, 5, [0.2, 0.1], [0.8, 0.5]), (172, 172, 100, 20, [0.1], [0.95])],
                         ids=["d20", "d172"])
@pytest.mark.parametrize("strategy", ["streaming", "pruning"])
def test_embed_nodes_is_the_eval_forward_without_the_update(D, F, T, k, al, be, strategy):
    from zebra_amd.tppr import get_neighbor_finder
    N, E, bs, seed = 80, 250, 50, 61
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    nf = None
    if strategy == "pruning":
        nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat, strategy=strategy, nf=nf).eval()
    dev = torch.device("cuda")
    t = [torch.from_numpy(x).to(dev) for x in (src, dst, neg, ts, eidx)]
    with pytest.raises(RuntimeError):                            # a fresh model is not in test mode
        tgn.embed_nodes(src[:3], ts[:3])
    for b in range(3):
        tgn.step_device(*[x[b * bs:(b + 1) * bs] for x in t], check_status=True)
    s, e = 3 * bs, 4 * bs
    nodes = np.concatenate([src[s:e], dst[s:e], neg[s:e]])
    before = _model_state(tgn)
    got = tgn.embed_nodes(nodes, np.concatenate([ts[s:e]] * 3))
    again = tgn.embed_nodes(torch.from_numpy(nodes).to(dev), torch.cat([t[3][s:e]] * 3))       # tensors in: the same
    after = _model_state(tgn)
    for kk in before:
        assert np.array_equal(before[kk], after[kk]), "embed_nodes changed %s" % kk
    assert got.shape == (3 * bs, D * (len(al) + 1)) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got, again)
    want = tgn.step_device(*[x[s:e] for x in t], check_status=True)
    ok = comparable(src[s:e], dst[s:e], neg[s:e]) if strategy == "streaming" else np.ones(3 * bs, bool)
    assert ok.sum() >= bs
    assert np.array_equal(got.cpu().numpy()[ok].view(np.uint32), want.cpu().numpy()[ok].view(np.uint32))
    # train state and an enabled pipeline are refused
    tgn.test_mode = False
    with pytest.raises(RuntimeError):
        tgn.embed_nodes(nodes, np.concatenate([ts[s:e]] * 3))
    tgn.test_mode = True
    tgn.enable_pipeline(max_batch=64)
    try:
        with pytest.raises(RuntimeError, match="pipeline"):
            tgn.embed_nodes(nodes, np.concatenate([ts[s:e]] * 3))
    finally:
        tgn.enable_pipeline(False)


# ---- 7. zt_affinity_rank against float64 ----------------------------------------------------------------------------------
# hidden width H = D (n_tppr + 1) -> (D, n_tppr) of the weight generator
WIDTHS = {4: (2, 1), 20: (10, 1), 300: (100, 2), 516: (172, 2), 772: (193, 3), RK_HC + 4: (257, 3)}


@functools.lru_cache(maxsize=None)
def _weights(H):
    D, M = WIDTHS[H]
    return I.model_weights(D, 1, 20, M, 7 + H)


def _ranker(H):
    """TGN.rank_scores / score_device on a MergeLayer of width H alone (some widths have no (D, M) a TGN takes)"""
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN
    m = MergeLayer(H, H, H, 1)
    w = _weights(H)
    with torch.no_grad():
        for p, key in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), ("aff1_w", "aff1_b", "aff2_w", "aff2_b")):
            p.copy_(torch.from_numpy(w[key]))
    holder = types.SimpleNamespace(affinity_score=m.to("cuda"), device=torch.device("cuda"))
    for name in ("rank_scores", "_affinity_state", "score_device"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    return holder


@functools.lru_cache(maxsize=None)
def _rank_inputs(Q, C, H, shared):
    """(emb_q, emb_c, cand_idx, float64 reference), computed once per shape.  With cand_idx: repeats, -1, a first row all
    present, and Nc != C."""
    rng = np.random.RandomState(1000 * Q + 10 * C + H + (1 if shared else 0))
    Nc = C if shared else max(2, C // 2 + 3)
    emb_q = (rng.standard_normal((Q, H)) * 0.7).astype(np.float32)
    emb_c = (rng.standard_normal((Nc, H)) * 0.7).astype(np.float32)
    if shared:
        idx = np.tile(np.arange(C, dtype=np.int32), (Q, 1))
    else:
        idx = rng.randint(0, Nc, (Q, C)).astype(np.int32)
        idx[rng.random_sample((Q, C)) < 0.15] = -1
        idx[0] = rng.randint(0, Nc, C)
        if Q > 1:
            idx[-1, -1] = -1
    return emb_q, emb_c, idx, merge_f64(emb_q, emb_c, idx, _weights(H))


RANK_SHAPES = ([(Q, C, H) for H in sorted(WIDTHS) for Q in (1, 17, 200) for C in (1, 2, 63, 65)] + [(17, 1000, 300)])


@pytest.mark.parametrize("Q,C,H", RANK_SHAPES)
def test_rank_scorer_matches_float64(Q, C, H):
    """Shared candidates (cand_idx NULL) and per-query indices with repeats and -1: within 1e-4 of the float64 MergeLayer,
    absent entries read 0, two calls give the same bits."""
    rk = _ranker(H)
    worst = {}
    for shared in (True, False):
        emb_q, emb_c, idx, ref = _rank_inputs(Q, C, H, shared)
        eq, ec = torch.from_numpy(emb_q).cuda(), torch.from_numpy(emb_c).cuda()
        ix = None if shared else torch.from_numpy(idx).cuda()
        got = rk.rank_scores(eq, ec, ix)
        again = rk.rank_scores(eq, ec, ix)
        torch.cuda.synchronize()
        assert got.shape == (Q, C) and got.dtype == torch.float32 and torch.equal(got, again)
        g = got.cpu().numpy()
        assert not g[idx < 0].any()
        worst[shared] = float(np.abs(g.astype(np.float64) - ref).max())
    print("Q=%d C=%d H=%d: max |prob - float64| = %.3g shared, %.3g indexed" % (Q, C, H, worst[True], worst[False]))
    assert max(worst.values()) <= TOL


def test_rank_scorer_reports_an_index_out_of_range():
    rk = _ranker(20)
    emb_q, emb_c, idx, ref = _rank_inputs(17, 63, 20, False)
    bad = idx.copy()
    bad[3, 5] = emb_c.shape[0]
    eq, ec = torch.from_numpy(emb_q).cuda(), torch.from_numpy(emb_c).cuda()
    got = rk.rank_scores(eq, ec, torch.from_numpy(bad).cuda(), check_status=False).cpu().numpy()
    assert got[3, 5] == 0
    keep = np.ones(bad.shape, bool)
    keep[3, 5] = False
    assert np.abs(got.astype(np.float64) - ref)[keep].max() <= TOL
    with pytest.raises(IndexError):
        rk.rank_scores(eq, ec, torch.from_numpy(bad).cuda())
    rk.rank_scores(eq, ec, torch.from_numpy(idx).cuda())         # the next call starts from a clean status word


@pytest.mark.parametrize("H", [300, 516])
def test_rank_scorer_matches_the_pair_scorer(H):
    """C = 2 with cand_idx = [dst, neg]: the probabilities TGN.score_device gives for the same [src | dst | neg] block"""
    B = 200
    rk = _ranker(H)
    g = torch.Generator().manual_seed(B + H)
    emb = (torch.randn((3 * B, H), generator=g) * 0.7).cuda()
    pair = rk.score_device(emb)
    ix = torch.stack([torch.arange(B), torch.arange(B) + B], dim=1).to(torch.int32).cuda()
    got = rk.rank_scores(emb[:B], emb[B:], ix)
    err = float((got.t().reshape(-1) - pair).abs().max())
    print("H=%d: max |rank scorer - pair scorer| = %.3g" % (H, err))
    assert err <= FORM_TOL


def test_rank_scores_falls_back_to_torch_off_the_bound():
    """CPU tensors and a width the kernel does not take go through torch's composition: the same function"""
    rk = _ranker(20)
    emb_q, emb_c, idx, ref = _rank_inputs(17, 63, 20, False)
    rk_cpu = types.SimpleNamespace(affinity_score=rk.affinity_score.cpu(), device=torch.device("cpu"))
    from zebra_amd.tgn import TGN
    got = TGN.rank_scores(rk_cpu, torch.from_numpy(emb_q), torch.from_numpy(emb_c), torch.from_numpy(idx))
    assert np.abs(got.numpy().astype(np.float64) - ref).max() <= TOL and not got.numpy()[idx < 0].any()


# ---- 8. zt_rank_metrics -------------------------------------------------------------------------------------------------
def test_rank_metrics_on_hand_made_and_tied_arrays():
    from zebra_amd import evaluation as ev
    dev = torch.device("cuda")
    for prob, idx, want in rank_cases():
        acc, rk = ev.rank_metrics(torch.from_numpy(prob).to(dev), None if idx is None else torch.from_numpy(idx).to(dev),
                                  ranks=True)
        assert rk.cpu().numpy().tolist() == want
        assert np.abs(acc.cpu().numpy() - rank_sums(np.array(want))).max() <= 1e-12
    # many ties: probabilities rounded to 3 decimals.  Then 1100 queries -- more than one chunk of the kernel's rank buffer --
    # of two distinct candidates: every 1 / rank is 1 or 0.5, so the sums are exact in any order and 1e-12 holds there too
    rng = np.random.RandomState(5)
    for Q, C, decimals in ((200, 101, 3), (1100, 2, None)):
        prob = rng.random_sample((Q, C))
        prob = (np.round(prob, decimals) if decimals else prob).astype(np.float32)
        assert decimals or not (prob[:, 0] == prob[:, 1]).any()
        idx = rng.randint(0, 50, (Q, C)).astype(np.int32)
        idx[rng.random_sample((Q, C)) < 0.1] = -1
        for ix in (None, idx):
            want = rank_of_positive(prob, ix)
            acc = torch.zeros(5, dtype=torch.float64, device=dev)
            p_d, i_d = torch.from_numpy(prob).to(dev), None if ix is None else torch.from_numpy(ix).to(dev)
            _, rk = ev.rank_metrics(p_d, i_d, out=acc, ranks=True)
            assert np.array_equal(rk.cpu().numpy(), want)
            sums = rank_sums(want)
            assert np.abs(acc.cpu().numpy() - sums).max() <= 1e-12
            ev.rank_metrics(p_d, i_d, out=acc)                   # a second call adds to the accumulator
            assert np.abs(acc.cpu().numpy() - 2 * sums).max() <= 1e-12
            assert ix is None or sums[4] < Q                     # some positives are absent: those queries are not counted


# ---- 9. rank_candidates and eval_edge_ranking ---------------------------------------------------------------------------
class _Sampler:
    def __init__(self, dst_list, seed):
        self.dst_list, self.seed = np.unique(dst_list), seed
        self.random_state = np.random.RandomState(seed)

    def reset_random_state(self):
        self.random_state = np.random.RandomState(self.seed)

    def sample(self, size):
        i = self.random_state.randint(0, len(self.dst_list), size)
        return self.dst_list[i], self.dst_list[self.random_state.randint(0, len(self.dst_list), size)]


def test_eval_edge_ranking_matches_a_restatement():
    from zebra_amd import evaluation as ev
    N, E, D, F, T, k, al, be, seed, bs, n_neg = 60, 300, 20, 7, 20, 5, [0.2, 0.1], [0.8, 0.5], 71, 50, 20
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    data = types.SimpleNamespace(sources=src, destinations=dst, timestamps=ts, edge_idxs=eidx, n_interactions=E)
    state_model = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat)
    got = ev.eval_edge_ranking(state_model, _Sampler(dst, 9), data, 10, batch_size=bs, n_negatives=n_neg)
    # the restatement: embed_nodes, a float64 MergeLayer (the tolerance of a probability), the numpy rank on the kernel's own
    # probabilities (near-ties cannot flip); the state advances by plain eval steps over the first-column negatives
    model = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat).eval()
    smp = _Sampler(dst, 9)
    smp.reset_random_state()
    model.update_memory_in_test(model.memory)
    model.test_mode = True
    sums = np.zeros(5)
    for s in range(0, E, bs):
        e = s + bs
        negs = smp.sample(bs * n_neg)[1].reshape(bs, n_neg)
        cands = np.concatenate([dst[s:e, None], negs], axis=1)
        prob = model.rank_candidates(src[s:e], ts[s:e], cands)
        assert prob.shape == (bs, 1 + n_neg) and prob.is_cuda
        emb_q = model.embed_nodes(src[s:e], ts[s:e]).cpu().numpy()
        emb_c = model.embed_nodes(cands.reshape(-1), np.repeat(ts[s:e], 1 + n_neg)).cpu().numpy()
        ref = merge_f64(emb_q, emb_c, np.arange(bs * (1 + n_neg)).reshape(bs, 1 + n_neg), w)
        assert np.abs(prob.cpu().numpy().astype(np.float64) - ref).max() <= TOL
        # a [C] list shared by all queries, with an absent entry
        shared = np.concatenate([cands[0, :5], [-1]])
        ps = model.rank_candidates(src[s:s + 4], np.full(4, ts[s]), shared).cpu().numpy()
        assert ps.shape == (4, 6) and not ps[:, 5].any() and np.abs(ps[0, :5] - prob[0, :5].cpu().numpy()).max() <= FORM_TOL
        sums += rank_sums(rank_of_positive(prob.cpu().numpy()))
        model.compute_temporal_embeddings(src[s:e], dst[s:e], negs[:, 0], ts[s:e], eidx[s:e], 10, False)
    assert sums[4] == E
    want = dict(mrr=sums[0] / E, hits1=sums[1] / E, hits3=sums[2] / E, hits10=sums[3] / E)
    print("ranking pass:", got)
    for kk in want:
        assert abs(got[kk] - want[kk]) <= 1e-12, kk
    assert 0.0 < got["mrr"] <= 1.0 and got["hits1"] <= got["hits3"] <= got["hits10"] <= 1.0
    a, b_ = _model_state(state_model), _model_state(model)
    for kk in a:
        assert np.array_equal(a[kk], b_[kk]), "state %s after the ranking pass differs from plain eval stepping" % kk
