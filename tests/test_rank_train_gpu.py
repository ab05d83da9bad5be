"""The ranking training step on the device: the one-vs-many scorer (csrc/rank_train.hip through modules._HipRankScore and
TGN.score_many_train) against a float64 MergeLayer under autograd at every seam of its tiling and every index pattern -- with
torch's own float32 composition held to HALF the tolerances on the same inputs --, its bits against TGN.rank_scores, across runs
and with outputs skipped, the listwise losses (csrc/train_tail.hip through losses.listwise_loss) against their float64
restatements, the status word, the memory a step takes per pair, and TGN.compute_rank_loss as a whole step against
compute_edge_loss (loss, gradients and the state it leaves) and against the torch composition."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn
from helpers_rank_train import (NEG_INF, check_transpose, composed_scorer, merge_layer, rank_loss_f64, scorer_inputs,
                                scorer_weights)

pytestmark = pytest.mark.gpu

PARAMS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
# (Q, C, H): Q across RK_TQ = 4 (1, 4, 5, 9; 9 gives three workgroup partials of d fc2.weight), C across RK_TC = 32 (1, 2, 31, 32,
# 33, 101), H across the 64-column step and the RK_HC = 1024 chunk (4, 60, 64, 68, 300, 516, 1024, 1028, 4352) -- every value
# once -- and the workload's own shape
SHAPES = [(5, 1, 4), (4, 2, 60), (5, 31, 64), (9, 32, 68), (1, 33, 300), (4, 101, 516), (5, 33, 1024), (9, 2, 1028), (3, 9, 4352),
          (200, 101, 300)]


def _index(kind, Q, C_, seed=11):
    """(cand_idx int32 [Q, C] or None, Nc) of one index pattern"""
    g = torch.Generator().manual_seed(seed + 31 * Q + C_)
    if kind == "none":                                   # the shared pool: C == Nc
        return None, C_
    if kind == "once":                                   # each row named once
        return torch.randperm(Q * C_, generator=g).to(torch.int32).reshape(Q, C_), Q * C_
    if kind == "shared":                                 # deduplicated candidates: rows shared by several queries
        Nc = max(2, C_ // 2 + 3)
        return torch.randint(0, Nc, (Q, C_), generator=g, dtype=torch.int32), Nc
    if kind == "unreferenced":                           # row 5 of emb_c is named by nobody
        Nc = C_ + 7
        ix = torch.randint(0, Nc, (Q, C_), generator=g, dtype=torch.int32)
        ix[ix == 5] = 6
        return ix, Nc
    if kind == "holes":                                  # scattered -1s
        Nc = C_ + 3
        ix = torch.randint(0, Nc, (Q, C_), generator=g, dtype=torch.int32)
        ix[torch.rand((Q, C_), generator=g) < 0.3] = -1
        return ix, Nc
    if kind == "empty_query":                            # a query whose columns are all absent
        Nc = C_ + 3
        ix = torch.randint(0, Nc, (Q, C_), generator=g, dtype=torch.int32)
        ix[Q // 2] = -1
        return ix, Nc
    raise ValueError(kind)


def _hip(emb_q, emb_c, ix, dl, wts, emb_grad=True, param_grad=True):
    from zebra_amd.modules import _HipRankScore
    eq, ec = emb_q.cuda().requires_grad_(emb_grad), emb_c.cuda().requires_grad_(emb_grad)
    ps = [torch.from_numpy(w).cuda().requires_grad_(param_grad) for w in wts]
    lg = _HipRankScore.apply(eq, ec, None if ix is None else ix.cuda(), *ps)
    lg.backward(dl.cuda())
    return [lg.detach(), eq.grad, ec.grad] + [p.grad for p in ps]


def _errors(got, ref):
    """(logits: the same -inf pattern and max |error| of the finite ones, max |error| of d_emb_q and d_emb_c,
    [(max |error|, max |ref|) of the four parameter gradients])"""
    gone = ref[0] == NEG_INF
    assert torch.equal(got[0].cpu() == NEG_INF, gone.cpu())
    d = [float((g.detach().double().cpu().reshape(-1) - r.detach().double().cpu().reshape(-1)).abs().max()) if r.numel() else 0.0
         for g, r in zip([torch.where(gone.to(got[0].device), torch.zeros_like(got[0]), got[0])] + list(got[1:]),
                         [torch.where(gone, torch.zeros_like(ref[0]), ref[0])] + list(ref[1:]))]
    return d[0], max(d[1], d[2]), [(d[3 + q], float(ref[3 + q].abs().max())) for q in range(4)]


def _against_float64(Q, C_, H, kind):
    ix, Nc = _index(kind, Q, C_)
    emb_q, emb_c, dl, wts = scorer_inputs(Q, C_, H, Nc=Nc)
    ref = composed_scorer(merge_layer(H, wts, torch.float64, "cpu"), emb_q.double(), emb_c.double(), ix, dl.double())
    got = _hip(emb_q, emb_c, ix, dl, wts)
    hip = _errors(got, ref)
    tor = _errors(composed_scorer(merge_layer(H, wts, torch.float32, "cuda"), emb_q.cuda(), emb_c.cuda(),
                                  None if ix is None else ix.cuda(), dl.cuda()), ref)
    print("Q=%d C=%d H=%d %s hip: logit %.3g d_emb %.3g params %s | torch: logit %.3g d_emb %.3g params %s"
          % (Q, C_, H, kind, hip[0], hip[1], ["%.3g" % e for e, _ in hip[2]], tor[0], tor[1], ["%.3g" % e for e, _ in tor[2]]))
    for name, (l_err, x_err, par), scale in (("torch", tor, 0.5), ("hip", hip, 1.0)):
        assert l_err <= scale * 1e-5, "%s logits: %g" % (name, l_err)
        assert x_err <= scale * 1e-5, "%s d_emb: %g" % (name, x_err)
        for pn, (err, mx) in zip(PARAMS, par):
            assert err <= scale * (1e-5 + 1e-4 * mx), "%s %s: %g (max |ref| %g)" % (name, pn, err, mx)
    return got, ix, Nc


@pytest.mark.parametrize("i,shape", list(enumerate(SHAPES)))
def test_hip_rank_score_against_float64(i, shape):
    """_HipRankScore forward and backward against a float64 MergeLayer under autograd on the CPU: logits and the embedding
    gradients within 1e-5, the four parameter gradients within 1e-5 + 1e-4 max|ref| (the project's training tolerances,
    tests/test_scoring_train_gpu.py); torch's float32 composition on the GPU, same inputs, within HALF of each.  The shapes
    alternate between the shared pool (no index) and an index with -1s."""
    _against_float64(*shape, "none" if i % 2 == 0 else "holes")


@pytest.mark.parametrize("kind", ["none", "once", "shared", "unreferenced", "holes", "empty_query"])
def test_hip_rank_score_index_patterns(kind):
    """(9, 33, 300) under every index pattern, same tolerances; the gradient row of an emb_c row nobody names is exactly zero,
    and so is the gradient of a query without a present column."""
    got, ix, Nc = _against_float64(9, 33, 300, kind)
    if kind == "unreferenced":
        assert not bool((ix == 5).any())
        assert float(got[2][5].abs().max()) == 0.0
    if kind == "empty_query":
        assert float(got[1][9 // 2].abs().max()) == 0.0
    if ix is not None:
        from zebra_amd.modules import rank_transpose
        check_transpose(ix, Nc, *rank_transpose(ix.cuda(), Nc))


def _bare_model(H, wts):
    """what TGN.rank_scores / score_many_train read of a model: the scorer's parameters and the device"""
    return types.SimpleNamespace(affinity_score=merge_layer(H, wts, torch.float32, "cuda"), device=torch.device("cuda"),
                                 fused_scoring=True)


@pytest.mark.parametrize("shape", [(9, 33, 300), (5, 33, 1024), (200, 101, 300)])
@pytest.mark.parametrize("kind", ["none", "holes"])
def test_sigmoid_of_the_logits_has_rank_scores_bits(shape, kind):
    """1 / (1 + exp(-logit)) in float32 -- rk_prob's expression -- equals TGN.rank_scores (zt_affinity_rank) on the same inputs
    bit for bit: the two kernels share rank_pair.hpp's pair sum.  An absent pair: -inf there, probability 0 here."""
    from zebra_amd.tgn import TGN
    Q, C_, H = shape
    ix, Nc = _index(kind, Q, C_)
    emb_q, emb_c, _, wts = scorer_inputs(Q, C_, H, Nc=Nc)
    model = _bare_model(H, wts)
    ixd = None if ix is None else ix.cuda()
    with torch.no_grad():
        lg = TGN.score_many_train(model, emb_q.cuda(), emb_c.cuda(), ixd)
    prob = TGN.rank_scores(model, emb_q.cuda(), emb_c.cuda(), ixd)
    assert torch.equal(1.0 / (1.0 + torch.exp(-lg)), prob)
    if ix is not None:
        assert torch.equal(lg == NEG_INF, ixd < 0)


@pytest.mark.parametrize("shape,kind", [((9, 33, 300), "shared"), ((5, 33, 1024), "none"), ((200, 101, 300), "holes")])
def test_hip_rank_score_is_bit_equal_across_runs(shape, kind):
    ix, Nc = _index(kind, *shape[:2])
    emb_q, emb_c, dl, wts = scorer_inputs(*shape, Nc=Nc)
    a, b = _hip(emb_q, emb_c, ix, dl, wts), _hip(emb_q, emb_c, ix, dl, wts)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape,kind", [((9, 33, 300), "shared"), ((4, 101, 516), "none")])
def test_hip_rank_score_skips_outputs_that_are_not_needed(shape, kind):
    """embeddings without a gradient: only the parameter gradients come back, the same bits as with it; frozen parameters:
    only the embedding gradients, the same bits."""
    ix, Nc = _index(kind, *shape[:2])
    emb_q, emb_c, dl, wts = scorer_inputs(*shape, Nc=Nc)
    full = _hip(emb_q, emb_c, ix, dl, wts)
    par = _hip(emb_q, emb_c, ix, dl, wts, emb_grad=False)
    assert par[1] is None and par[2] is None
    for q in range(3, 7):
        assert torch.equal(par[q], full[q]), PARAMS[q - 3]
    inp = _hip(emb_q, emb_c, ix, dl, wts, param_grad=False)
    assert all(g is None for g in inp[3:])
    for q in range(3):
        assert torch.equal(inp[q], full[q])


def test_index_out_of_range_raises_and_leaves_the_other_pairs():
    """An index >= Nc and an index < -1 (out of range by VALUE only: the kernel treats such a pair as absent and reads
    nothing for it) raise IndexError through _HipRankScore; through the C-ABI the status word says ZT_ERR_RANGE and every
    other pair's logit has the bits of the call where that pair is -1."""
    from zebra_amd import _capi
    from zebra_amd.modules import _HipRankScore
    Q, C_, H = 9, 33, 300
    ix, Nc = _index("holes", Q, C_)
    emb_q, emb_c, _, wts = scorer_inputs(Q, C_, H, Nc=Nc)
    ps = [torch.from_numpy(w).cuda() for w in wts]
    eq, ec = emb_q.cuda(), emb_c.cuda()
    lib = _capi.lib()
    for bad_value in (Nc, -2):
        bad = ix.clone()
        bad[3, 7] = bad_value
        with pytest.raises(IndexError):
            _HipRankScore.apply(eq, ec, bad.cuda(), *ps)
        masked = ix.clone()
        masked[3, 7] = -1
        want = _HipRankScore.apply(eq, ec, masked.cuda(), *ps)
        lg = torch.empty((Q, C_), device="cuda")
        pq, pc = torch.empty((Q, H), device="cuda"), torch.empty((Nc, H), device="cuda")
        ws = torch.empty(int(lib.zt_affinity_rank_train_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int64(C_), C.c_int32(H))),
                         dtype=torch.uint8, device="cuda")
        wt = _capi.AffinityWeights(*[_capi.ptr(t) for t in ps])
        badd = bad.cuda()
        _capi.check(lib.zt_affinity_rank_train_forward(_capi.ptr(eq), C.c_int64(Q), _capi.ptr(ec), C.c_int64(Nc), _capi.ptr(badd),
                                                       C.c_int64(C_), C.c_int32(H), C.byref(wt), _capi.ptr(lg), _capi.ptr(pq),
                                                       _capi.ptr(pc), _capi.ptr(ws), _capi.stream_ptr()))
        assert int(ws[:4].view(torch.int32).item()) == _capi.ZT_ERR_RANGE
        assert torch.equal(lg, want)
        assert float(lg[3, 7]) == NEG_INF


# ---------------------------------------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------------------------------------
def _logits(Q, C_, seed, absent=0.0, skip=None, all_skipped=False, with_target=False):
    g = torch.Generator().manual_seed(seed + 7 * Q + C_)
    lg = torch.randn((Q, C_), generator=g) * 3
    t = torch.randint(0, C_, (Q,), generator=g) if with_target else torch.zeros(Q, dtype=torch.long)
    if absent:
        keep = lg[torch.arange(Q), t].clone()
        lg[torch.rand((Q, C_), generator=g) < absent] = NEG_INF
        lg[torch.arange(Q), t] = keep
    if skip is not None:
        lg[skip, t[skip]] = NEG_INF
    if all_skipped:
        lg[torch.arange(Q), t] = NEG_INF
    return lg, (t.to(torch.int32) if with_target else None)


LOSS_CASES = [dict(Q=1, C_=1), dict(Q=1, C_=2), dict(Q=3, C_=1), dict(Q=17, C_=2), dict(Q=7, C_=65, absent=0.3),
              dict(Q=9, C_=33, absent=0.2, skip=4), dict(Q=9, C_=33, absent=0.2, skip=4, with_target=True),
              dict(Q=5, C_=64, with_target=True), dict(Q=6, C_=5, all_skipped=True), dict(Q=200, C_=1001, absent=0.1, skip=17)]


@pytest.mark.parametrize("mode", ["softmax", "bce"])
@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
def test_listwise_loss_against_float64(case, mode):
    """listwise_loss on the GPU (zt_rank_loss_forward / _backward) against the float64 restatement: the loss within 1e-6
    relative, d loss / d logit within 1e-7 + 1e-5 |ref| -- the kernels compute in float64 and round once, the bound is float32
    rounding of the result with room.  The incoming gradient (here 0.5) is applied on the device."""
    from zebra_amd.losses import listwise_loss, rank_loss_plan
    lg, target = _logits(seed=5, **case)
    x = lg.cuda().requires_grad_(True)
    td = None if target is None else target.cuda()
    assert rank_loss_plan(x, td) == "hip"
    loss = listwise_loss(x, td, mode)
    (0.5 * loss).backward()
    loss = loss.detach()
    want, dl = rank_loss_f64(lg, target, mode)
    err = abs(float(loss) - float(want))
    g_err = (x.grad.double().cpu() - 0.5 * dl).abs()
    print("%s %s loss %.9g ref %.9g err %.3g; dl max err %.3g" % (case, mode, float(loss), float(want), err, float(g_err.max())))
    assert err <= 1e-6 * abs(float(want))
    assert bool((g_err <= 1e-7 + 1e-5 * (0.5 * dl).abs()).all())
    if case.get("all_skipped"):
        assert float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0
    if case.get("skip") is not None:
        assert float(x.grad[case["skip"]].abs().max()) == 0.0


def test_listwise_loss_is_bit_equal_across_runs_and_clamps_at_100():
    from zebra_amd.losses import listwise_loss
    lg, _ = _logits(Q=200, C_=101, seed=9, absent=0.1)
    for mode in ("softmax", "bce"):
        outs = []
        for _ in range(2):
            x = lg.cuda().requires_grad_(True)
            loss = listwise_loss(x, None, mode)
            loss.backward()
            outs.append((loss.detach(), x.grad))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    far = torch.tensor([[-250.0, 300.0]], device="cuda")            # log sigma(-250) and log(1 - sigma(300)): both cut at -100
    assert float(listwise_loss(far, None, "bce")) == 200.0


def test_bce_mode_with_two_columns_is_the_link_loss():
    """mode "bce" with C = 2 against losses.link_bce_loss of the same probabilities.  The kernels do NOT share their
    arithmetic: zt_link_bce_forward takes the logarithm of a float32 probability, zt_rank_loss_forward forms log sigmoid from
    the logit in float64 -- so the two agree within 1e-6 (logits within +-4 here: 1 - p keeps its digits), not in bits."""
    from zebra_amd.losses import link_bce_loss, listwise_loss
    g = torch.Generator().manual_seed(3)
    lg = (torch.randn((200, 2), generator=g) * 1.5).clamp(-4, 4).cuda()
    prob = torch.sigmoid(lg)
    a = float(listwise_loss(lg, None, "bce"))
    b = float(link_bce_loss(prob[:, 0], prob[:, 1]))
    print("listwise bce %.9g link bce %.9g" % (a, b))
    assert abs(a - b) <= 1e-6


def test_memory_per_pair():
    """Forward + backward of score_many_train + listwise_loss at H = 512, Q = 64, a fixed emb_c of 64 rows and an index with
    repeats: going from C = 64 to C = 1024 the peak of torch.cuda.max_memory_allocated grows by at most 256 bytes per added
    pair -- logits, dl, index, transpose and sort temporaries are a few dozen bytes a pair; a materialised hidden layer alone
    would be 2048."""
    from zebra_amd.losses import listwise_loss
    from zebra_amd.tgn import TGN
    Q, Nc, H = 64, 64, 512
    wts = scorer_weights(H, 3)
    model = _bare_model(H, wts)
    g = torch.Generator().manual_seed(1)
    emb_q, emb_c = (torch.randn((Q, H), generator=g) * 0.7).cuda(), (torch.randn((Nc, H), generator=g) * 0.7).cuda()
    growth = {}
    for C_ in (64, 1024, 64, 1024):                                  # (the first round warms the allocator and the kernels)
        ix = torch.randint(0, Nc, (Q, C_), generator=g, dtype=torch.int32).cuda()
        eq, ec = emb_q.clone().requires_grad_(True), emb_c.clone().requires_grad_(True)
        model.affinity_score.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = listwise_loss(TGN.score_many_train(model, eq, ec, ix), None, "softmax")
        loss.backward()
        torch.cuda.synchronize()
        growth[C_] = torch.cuda.max_memory_allocated() - base
        del loss, eq, ec, ix
    per_pair = (growth[1024] - growth[64]) / float(Q * (1024 - 64))
    print("peak growth: C=64 %d bytes, C=1024 %d bytes: %.1f bytes per added pair" % (growth[64], growth[1024], per_pair))
    assert per_pair <= 256


# ---------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------
N_NODES, N_EDGES, D, F, T, K_TPPR, SEED, B, WARM = 60, 300, 20, 7, 20, 5, 33, 17, 3
MODELS = {1: ([0.2], [0.8]), 2: ([0.2, 0.1], [0.8, 0.5])}


def _stream():
    return I.make_stream("general", N_NODES, N_EDGES, SEED)


def _model(n_models, fused=True):
    """a model after WARM training batches of B edges (compute_edge_loss): the state the step under test starts from"""
    al, be = MODELS[n_models]
    w = I.model_weights(D, F, T, len(al), SEED)
    _, efeat = I.random_tables(N_NODES, N_EDGES + 1, D, F, SEED)
    tgn = build_tgn(N_NODES, N_EDGES + 1, D, F, T, K_TPPR, al, be, w, efeat)
    tgn.fused_scoring = fused
    tgn.train(True)
    src, dst, neg, ts, eidx = _stream()
    for b in range(WARM):
        s, e = b * B, (b + 1) * B
        tgn.compute_edge_loss(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10)
        tgn.memory.detach_memory()
    tgn.zero_grad()
    return tgn


def _batch():
    src, dst, _, ts, eidx = _stream()
    s, e = WARM * B, (WARM + 1) * B
    return src[s:e], dst[s:e], ts[s:e], eidx[s:e]


def _negatives(K, outside=True, holes=False, seed=2):
    """[B, K] negatives: nodes that are no endpoint of the batch (``outside``) or any node; ``holes``: some -1s"""
    src, dst, _, _ = _batch()
    rng = np.random.RandomState(seed + K)
    pool = np.setdiff1d(np.arange(1, N_NODES), np.concatenate([src, dst])) if outside else np.arange(1, N_NODES)
    assert pool.size >= 4
    neg = rng.choice(pool, (B, K)).astype(np.int32)
    if holes:
        neg[rng.random_sample((B, K)) < 0.25] = -1
        neg[5] = -1                                                   # an edge without a negative
    return neg


def _grads(tgn):
    return {pn: p.grad.detach().cpu().numpy().copy() for pn, p in tgn.named_parameters() if p.grad is not None}


def _state(tgn):
    m = tgn.memory
    torch.cuda.synchronize()
    st = dict(memory=m.memory.detach().cpu().numpy(), last_update=m.last_update.cpu().numpy(), messages=m.messages.detach().cpu().numpy(),
              msg_ts=m.timestamps.cpu().numpy(), flags=m.flags.cpu().numpy())
    finder = tgn.embedding_module.tppr_finder
    for mi in range(finder.n_tppr):
        for key, val in finder.export_state(mi).items():
            st["tppr%d_%s" % (mi, key)] = val
    return st


def _assert_close(ga, gb, la, lb):
    assert abs(la - lb) <= 1e-5, "loss %g against %g" % (la, lb)
    assert sorted(ga) == sorted(gb)
    for pn in ga:
        err = np.abs(ga[pn] - gb[pn]).max()
        assert err <= 1e-5 + 1e-4 * np.abs(gb[pn]).max(), "%s: %g" % (pn, err)


@pytest.fixture
def rank_calls(monkeypatch):
    """[n]: calls of lib().zt_affinity_rank_train_forward from here on"""
    from zebra_amd import _capi
    lib = _capi.lib()
    calls, fwd = [0], lib.zt_affinity_rank_train_forward

    def counted(*args):
        calls[0] += 1
        return fwd(*args)

    monkeypatch.setattr(lib, "zt_affinity_rank_train_forward", counted)
    return calls


@pytest.mark.parametrize("n_models", [1, 2])
def test_one_outside_negative_in_bce_mode_is_compute_edge_loss(n_models, rank_calls):
    """K = 1, mode "bce", the negative of every edge a node that is no endpoint of the batch: such a node's T-PPR row does not
    change inside the batch, so the row read before the batch is the row the stream would emit -- the loss and every
    parameter gradient agree with compute_edge_loss on the same batch from the same state within the training tolerances.
    And the state afterwards -- memory, last update, message store and flags, every T-PPR dictionary -- is bit-equal: the
    two-role stream updates what the three-role stream updates; negatives never write state."""
    src, dst, ts, eidx = _batch()
    neg = _negatives(1)
    a, b = _model(n_models), _model(n_models)
    loss_a, logits = a.compute_rank_loss(src, dst, neg, ts, eidx, 10, mode="bce")
    loss_a.backward()
    assert rank_calls[0] == 1 and logits.shape == (B, 2) and not logits.requires_grad
    loss_b, pos, negp = b.compute_edge_loss(src, dst, neg[:, 0], ts, eidx, 10)
    loss_b.backward()
    assert float((torch.sigmoid(logits[:, 0]) - pos[:, 0]).abs().max()) <= 1e-5
    assert float((torch.sigmoid(logits[:, 1]) - negp[:, 0]).abs().max()) <= 1e-5
    ga, gb = _grads(a), _grads(b)
    _assert_close(ga, gb, float(loss_a.detach()), float(loss_b.detach()))
    assert any(pn.startswith("embedding_module.") for pn in ga) and any(pn.startswith("memory_updater.") for pn in ga)
    sa, sb = _state(a), _state(b)
    assert sorted(sa) == sorted(sb)
    for key in sa:
        assert np.array_equal(sa[key], sb[key], equal_nan=True), key
    assert a.batch_counter == b.batch_counter and a.n_update_memory == b.n_update_memory


@pytest.mark.parametrize("K", [7, 33])
def test_state_after_the_step_does_not_depend_on_the_negatives(K):
    """K = 7 and 33 negatives drawn from ALL nodes, endpoints of the batch among them: the state after compute_rank_loss is bit-equal to the state
    after compute_edge_loss on the same batch with negatives[:, 0]."""
    src, dst, ts, eidx = _batch()
    neg = _negatives(K, outside=False)
    a, b = _model(2), _model(2)
    loss, logits = a.compute_rank_loss(src, dst, neg, ts, eidx, 10)
    assert logits.shape == (B, 1 + K) and bool(torch.isfinite(loss))
    b.compute_edge_loss(src, dst, neg[:, 0], ts, eidx, 10)
    sa, sb = _state(a), _state(b)
    for key in sa:
        assert np.array_equal(sa[key], sb[key], equal_nan=True), key


@pytest.mark.parametrize("mode", ["softmax", "bce"])
def test_hip_plan_against_torch_composition_on_the_same_step(mode, rank_calls):
    """fused_scoring True against False, K = 7 with some -1 negatives and an edge without any: the loss and every parameter
    gradient (scorer, embedding layers, GRU) within the training tolerances; with False the HIP scorer is never called."""
    src, dst, ts, eidx = _batch()
    neg = _negatives(7, outside=False, holes=True)
    res = {}
    for fused in (True, False):
        tgn = _model(2, fused)
        before = rank_calls[0]
        loss, logits = tgn.compute_rank_loss(src, dst, neg, ts, eidx, 10, mode=mode)
        loss.backward()
        assert rank_calls[0] - before == (1 if fused else 0)
        res[fused] = (float(loss.detach()), _grads(tgn), logits)
    assert torch.equal(res[True][2] == NEG_INF, res[False][2] == NEG_INF)
    assert torch.equal((res[True][2] == NEG_INF)[:, 1:].cpu(), torch.from_numpy(neg < 0))
    _assert_close(res[True][1], res[False][1], res[True][0], res[False][0])
    names = set(res[True][1])
    assert any(pn.startswith("affinity_score.") for pn in names) and any(pn.startswith("embedding_module.") for pn in names)
    assert any(pn.startswith("memory_updater.") for pn in names)


def test_negative_that_is_an_earlier_endpoint_reads_its_pre_batch_row(monkeypatch):
    """Every edge's negative is the SOURCE of the batch's first edge: an endpoint earlier in the batch.  The step runs, and the
    T-PPR rows it embeds for the negatives are those embedding_module.query_device returns on the state before the batch."""
    src, dst, ts, eidx = _batch()
    neg = np.full((B, 3), int(src[0]), np.int32)
    neg[:, 1] = int(dst[1])
    twin = _model(2)
    want = twin.embedding_module.query_device(torch.from_numpy(neg.reshape(-1)).cuda(),
                                              torch.from_numpy(np.repeat(ts, 3)).cuda())
    tgn = _model(2)
    em = tgn.embedding_module
    seen = {}
    inner = em._train_forward

    def spy(memory, nodes_d, on, oe, od, ow, memory_updater, index=None):
        seen["rows"] = [t.clone() for t in (on, oe, od, ow)]
        seen["nodes"] = nodes_d.clone()
        return inner(memory, nodes_d, on, oe, od, ow, memory_updater, index)

    monkeypatch.setattr(em, "_train_forward", spy)
    loss, logits = tgn.compute_rank_loss(src, dst, neg, ts, eidx, 10)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(logits).all())
    assert seen["nodes"].numel() == 2 * B + 3 * B
    assert torch.equal(seen["nodes"][2 * B:].cpu(), torch.from_numpy(neg.reshape(-1)))
    for got, ref in zip(seen["rows"], want):
        assert torch.equal(got[:, 2 * B:], ref)


def test_compute_rank_loss_refusals():
    src, dst, ts, eidx = _batch()
    tgn = _model(1)
    for bad in (np.zeros((B, 0), np.int32), np.ones(B, np.int32)):
        with pytest.raises(ValueError):
            tgn.compute_rank_loss(src, dst, bad, ts, eidx, 10)
    with pytest.raises(ValueError):
        tgn.compute_rank_loss(src, dst, _negatives(2), ts, eidx, 10, edge_sel=np.arange(4))
    tgn.enable_pipeline(True)
    try:
        with pytest.raises(RuntimeError):
            tgn.compute_rank_loss(src, dst, _negatives(2), ts, eidx, 10)
    finally:
        tgn.enable_pipeline(False)
