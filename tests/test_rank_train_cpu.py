"""The ranking training step without a GPU: the float64 restatements of the two listwise losses against torch's own losses,
the plans, the transpose of an index matrix, what the C-ABI refuses before any device call, and the CPU fallbacks of
TGN.score_many_train, listwise_loss and TGN.compute_rank_loss's argument checks."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers_rank_train import (NEG_INF, check_transpose, composed_logits, merge_layer, rank_loss_f64, scorer_inputs,
                                scorer_weights)


def _loss_case(Q=9, C_=7, seed=3, with_target=False):
    """logits [Q, C] with absent columns, one query whose target is absent (skipped), (target or None)"""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn((Q, C_), generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, C_, (Q,), generator=g) if with_target else torch.zeros(Q, dtype=torch.long)
    lg[torch.rand((Q, C_), generator=g) < 0.25] = NEG_INF
    lg[torch.arange(Q), t] = torch.randn(Q, generator=g, dtype=torch.float64)      # targets present ...
    lg[Q // 2, t[Q // 2]] = NEG_INF                                                 # ... but one: that query is skipped
    return lg, (t if with_target else None), t


@pytest.mark.parametrize("with_target", [False, True])
def test_softmax_restatement_is_cross_entropy_over_present_columns(with_target):
    lg, target, t = _loss_case(with_target=with_target)
    loss, dl = rank_loss_f64(lg, target, "softmax")
    live = [q for q in range(lg.shape[0]) if lg[q, t[q]] != NEG_INF]
    assert len(live) == lg.shape[0] - 1
    want, grad = 0.0, torch.zeros_like(lg)
    for q in live:
        cols = torch.nonzero(lg[q] != NEG_INF).squeeze(1)
        x = lg[q, cols].clone().requires_grad_(True)
        ce = F.cross_entropy(x.unsqueeze(0), torch.tensor([int((cols == t[q]).nonzero())]))
        ce.backward()
        want += float(ce.detach()) / len(live)
        grad[q, cols] = x.grad / len(live)
    assert abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want))
    assert float((dl - grad).abs().max()) <= 1e-12


@pytest.mark.parametrize("with_target", [False, True])
def test_bce_restatement_is_bceloss_on_ones_and_zeros(with_target):
    lg, target, t = _loss_case(with_target=with_target)
    loss, dl = rank_loss_f64(lg, target, "bce")
    Q = lg.shape[0]
    live = torch.tensor([bool(lg[q, t[q]] != NEG_INF) for q in range(Q)])
    onehot = torch.zeros_like(lg, dtype=torch.bool)
    onehot[torch.arange(Q), t] = True
    x = torch.where(lg != NEG_INF, lg, torch.zeros_like(lg)).requires_grad_(True)
    pos = x[onehot & live.unsqueeze(1)].sigmoid()
    neg = x[(lg != NEG_INF) & ~onehot & live.unsqueeze(1)].sigmoid()
    crit = torch.nn.BCELoss()
    want = crit(pos, torch.ones_like(pos)) + crit(neg, torch.zeros_like(neg))
    want.backward()
    want = want.detach()
    assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, float(want))
    assert float((dl - torch.where(lg != NEG_INF, x.grad, torch.zeros_like(lg))).abs().max()) <= 1e-12
    assert float(dl[Q // 2].abs().max()) == 0.0                     # the skipped query


def test_restatements_with_every_query_skipped_are_zero():
    lg = torch.randn((4, 5), dtype=torch.float64)
    lg[:, 0] = NEG_INF
    for mode in ("softmax", "bce"):
        loss, dl = rank_loss_f64(lg, None, mode)
        assert float(loss) == 0.0 and float(dl.abs().max()) == 0.0


def test_listwise_loss_torch_composition_matches_the_restatements():
    """listwise_loss on CPU float64 tensors (the torch plan) against rank_loss_f64, loss and gradient, both modes, with a
    target, absent columns, a skipped query and all queries skipped; an unknown mode is refused."""
    from zebra_amd.losses import listwise_loss, rank_loss_plan
    for with_target in (False, True):
        lg, target, _ = _loss_case(with_target=with_target)
        assert rank_loss_plan(lg, target) == "torch"
        for mode in ("softmax", "bce"):
            x = lg.clone().requires_grad_(True)
            loss = listwise_loss(x, target, mode)
            loss.backward()
            want, dl = rank_loss_f64(lg, target, mode)
            assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, float(want)), mode
            assert float((torch.nan_to_num(x.grad) - dl).abs().max()) <= 1e-12, mode
    gone = torch.full((3, 4), NEG_INF, dtype=torch.float64).requires_grad_(True)
    z = listwise_loss(gone, None, "softmax")
    z.backward()
    assert float(z) == 0.0 and float(gone.grad.abs().max()) == 0.0
    with pytest.raises(ValueError):
        listwise_loss(lg, None, "hinge")


def test_plans():
    from zebra_amd.losses import rank_loss_plan
    from zebra_amd.tgn import rank_score_plan
    assert rank_score_plan("cpu", torch.float32, 300) == "torch"
    assert rank_score_plan("cuda", torch.float64, 300) == "torch"
    assert rank_score_plan("cuda", torch.float32, 302) == "torch"
    assert rank_score_plan("cuda", torch.float32, 4356) == "torch"
    assert rank_score_plan("cuda", torch.float32, 0) == "torch"
    assert rank_score_plan("cuda", torch.float32, 300, fused_scoring=False) == "torch"
    for H in (4, 300, 1028, 4352):
        assert rank_score_plan("cuda", torch.float32, H) == "hip"
    assert rank_loss_plan(torch.zeros((3, 4))) == "torch"
    assert rank_loss_plan(torch.zeros((3, 4), dtype=torch.float64)) == "torch"
    meta = torch.empty((3, 4), device="meta")                          # (only .is_cuda and the dtype are looked at)
    assert rank_loss_plan(meta) == "torch"


def test_rank_transpose():
    """an index matrix with repeats, -1s and an unreferenced row (2)"""
    from zebra_amd.modules import rank_transpose
    ix = torch.tensor([[0, 3, 3, -1], [4, -1, 0, 1], [-1, -1, -1, -1], [1, 1, 4, 0]], dtype=torch.int32)
    row_ptr, pairs = rank_transpose(ix, 5)
    check_transpose(ix, 5, row_ptr, pairs)
    assert row_ptr.dtype == torch.int64 and pairs.dtype == torch.int32
    assert row_ptr.tolist() == [0, 3, 6, 6, 8, 10]
    assert pairs.tolist() == [0, 6, 15, 7, 12, 13, 1, 2, 4, 14]
    g = torch.Generator().manual_seed(5)
    big = torch.randint(-1, 40, (33, 57), generator=g, dtype=torch.int32)
    big[big == 17] = -1                                               # row 17: unreferenced
    check_transpose(big, 40, *rank_transpose(big, 40))
    row_ptr, pairs = rank_transpose(torch.full((2, 3), -1, dtype=torch.int32), 4)
    assert row_ptr.tolist() == [0] * 5 and pairs.numel() == 0


def test_c_abi_refuses_before_any_device_call():
    from zebra_amd import _capi
    lib = _capi.lib()
    buf = np.zeros(64, np.float32)
    p = _capi.ptr(buf)                                                # (never dereferenced: every call below is refused first)
    w = _capi.AffinityWeights(p, p, p, p)
    i64, i32 = C.c_int64, C.c_int32

    def fwd(eq, Q, ec, Nc, ix, C_, H):
        return lib.zt_affinity_rank_train_forward(eq, i64(Q), ec, i64(Nc), ix, i64(C_), i32(H), C.byref(w), p, p, p, p, None)

    def bwd(eq, Q, ec, Nc, ix, C_, H):
        return lib.zt_affinity_rank_train_backward(eq, i64(Q), ec, i64(Nc), ix, i64(C_), i32(H), C.byref(w), p, p, p, p, p, i64(0),
                                                   p, p, p, p, p, p, p, None)

    for call in (fwd, bwd):
        assert call(p, 4, p, 8, p, 3, 6) == _capi.ZT_ERR_UNSUPPORTED
        assert call(p, 4, p, 8, p, 3, 4356) == _capi.ZT_ERR_UNSUPPORTED
        assert b"4352" in lib.zt_last_error()
        assert call(None, 4, p, 8, p, 3, 300) == _capi.ZT_ERR_ARG
        assert call(p, 4, None, 8, p, 3, 300) == _capi.ZT_ERR_ARG
        assert call(p, 4, p, 8, None, 3, 300) == _capi.ZT_ERR_ARG       # no index: C must be Nc
        assert call(p, -1, p, 8, p, 3, 300) == _capi.ZT_ERR_ARG
        assert call(p, 4, p, -8, p, 3, 300) == _capi.ZT_ERR_ARG
        assert call(p, 4, p, 8, p, -3, 300) == _capi.ZT_ERR_ARG
        assert call(p, 0, p, 8, p, 3, 300) == _capi.ZT_OK               # nothing to do, nothing touched
        assert call(p, 4, p, 8, p, 0, 300) == _capi.ZT_OK
    wsb = lib.zt_affinity_rank_train_workspace_bytes
    assert wsb(i64(4), i64(8), i64(3), i32(6)) == -1
    assert wsb(i64(4), i64(8), i64(3), i32(4356)) == -1
    assert wsb(i64(-4), i64(8), i64(3), i32(300)) == -1
    assert wsb(i64(4), i64(8), i64(3), i32(300)) >= 256 + (4 + 8) * 300 * 4
    loss = lib.zt_rank_loss_forward
    assert loss(p, None, i64(4), i64(3), i32(2), p, p, None) == _capi.ZT_ERR_ARG
    assert b"mode" in lib.zt_last_error()
    assert loss(p, None, i64(4), i64(3), i32(-1), p, p, None) == _capi.ZT_ERR_ARG
    assert loss(None, None, i64(4), i64(3), i32(0), p, p, None) == _capi.ZT_ERR_ARG
    assert loss(p, None, i64(0), i64(3), i32(0), p, p, None) == _capi.ZT_ERR_ARG
    assert lib.zt_rank_loss_backward(p, p, i64(0), p, None) == _capi.ZT_ERR_ARG
    assert lib.zt_rank_loss_backward(p, None, i64(5), p, None) == _capi.ZT_ERR_ARG


def test_compute_rank_loss_refuses_what_it_does_not_cover():
    """edge_sel (data-parallel shares), negatives that are not [B, K >= 1] and an enabled pipeline or exchange are refused
    before anything is touched: the checks need no model state (a bare namespace stands in for the model)."""
    from zebra_amd.tgn import TGN
    src = dst = np.arange(4)
    ts, eidx = np.arange(4.0), np.arange(4)
    neg = np.zeros((4, 3), np.int64)
    bare = types.SimpleNamespace(_pipe=None, _xchg=None)
    with pytest.raises(ValueError, match="edge_sel"):
        TGN.compute_rank_loss(bare, src, dst, neg, ts, eidx, 10, edge_sel=[0, 1])
    for bad in (np.zeros(4, np.int64), np.zeros((4, 0), np.int64), np.zeros((3, 2), np.int64)):
        with pytest.raises(ValueError, match="K >= 1"):
            TGN.compute_rank_loss(bare, src, dst, bad, ts, eidx, 10)
    with pytest.raises(RuntimeError, match="pipeline"):
        TGN.compute_rank_loss(types.SimpleNamespace(_pipe=object(), _xchg=None), src, dst, neg, ts, eidx, 10)
    with pytest.raises(RuntimeError, match="pipeline"):
        TGN.compute_rank_loss(types.SimpleNamespace(_pipe=None, _xchg=object()), src, dst, neg, ts, eidx, 10)


@pytest.mark.parametrize("indexed", [False, True])
def test_score_many_train_on_cpu_matches_float64(indexed):
    """TGN.score_many_train on CPU float32 tensors (the torch plan) against the float64 restatement: finite logits within
    1e-6 relative, -inf exactly where the index is -1, and gradients flow to embeddings and parameters."""
    from zebra_amd.tgn import TGN
    Q, C_, H, Nc = 5, 7, 12, 9
    emb_q, emb_c, _, wts = scorer_inputs(Q, C_, H, Nc=Nc)
    ix = None
    if indexed:
        ix = torch.randint(-1, Nc, (Q, C_), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
        ix[1] = -1
    else:
        emb_c = emb_c[:C_]
    model = types.SimpleNamespace(affinity_score=merge_layer(H, wts, torch.float32, "cpu"), fused_scoring=True)
    eq, ec = emb_q.clone().requires_grad_(True), emb_c.clone().requires_grad_(True)
    got = TGN.score_many_train(model, eq, ec, ix)
    want = composed_logits(merge_layer(H, wts, torch.float64, "cpu"), emb_q.double(), emb_c.double(), ix)
    assert got.shape == want.shape == (Q, C_)
    gone = want == NEG_INF
    assert torch.equal(got == NEG_INF, gone)
    err = (got.double()[~gone] - want[~gone]).abs()
    assert float(err.max()) <= 1e-6 * float(want[~gone].abs().max())     # relative to the logits' scale
    torch.where(gone, torch.zeros_like(got), got).sum().backward()
    assert eq.grad is not None and ec.grad is not None and model.affinity_score.fc1.weight.grad is not None
    if indexed:
        assert float(eq.grad[1].abs().max()) == 0.0                  # every column of query 1 is absent
        with pytest.raises(IndexError):
            TGN.score_many_train(model, emb_q, emb_c, torch.full((Q, C_), Nc, dtype=torch.int32))
