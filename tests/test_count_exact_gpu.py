"""The fused count (csrc/rank_count.hip through TGN.count_scores) on the planted cases of tests/helpers_count_planted.py, all
exact: the counts above and equal to a threshold are the host's, computed from the planted levels alone; thresholds are
zt_affinity_rank's bits of a planted target row, or constants.  Every call runs twice -- fresh, and into a view of a larger
buffer whose sentinel rows must survive.  The refusals of the header's contract leave sentinel outputs alone.  No tolerance.
tests/test_count_exact_cpu.py shows that each case reaches the seam its id names."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import helpers_count_planted as K
import helpers_topk_planted as P

pytestmark = pytest.mark.gpu
SENT = -77


@functools.lru_cache(maxsize=None)
def _ranker(H):
    """TGN.rank_scores / count_scores on the dialled MergeLayer of width H alone"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN
    m = MergeLayer(H, H, H, 1)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), P.scorer_weights(H)):
            p.copy_(torch.from_numpy(w))
    holder = types.SimpleNamespace(affinity_score=m.to("cuda"), device=torch.device("cuda"))
    for name in ("rank_scores", "count_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    return holder


def _thresholds(rk, case, d, eq):
    """float32 [Q] on the device: zt_affinity_rank on the planted target rows, the constants' own bits"""
    et = torch.from_numpy(d["emb_t"]).cuda()
    ix = torch.arange(case.Q, dtype=torch.int32, device="cuda").unsqueeze(1)
    thr = rk.rank_scores(eq, et, ix)[:, 0].cpu().numpy().copy()
    for q, (kind, v) in enumerate(d["thr_spec"]):
        if kind == "const":
            thr[q] = K.CONST_BITS[v]
    return thr


def _run(rk, case, d, eq, ec, thr, ws, pieces, incoming, skip):
    """one count into a view [2 : 2 + Q] of sentinel buffers; (above, equal) on the host"""
    Q = case.Q
    big_a = torch.full((Q + 4,), SENT, dtype=torch.int32, device="cuda")
    big_e = torch.full((Q + 4,), SENT, dtype=torch.int32, device="cuda")
    va, ve = big_a[2:2 + Q], big_e[2:2 + Q]
    va.copy_(torch.from_numpy(incoming[0].astype(np.int32)))
    ve.copy_(torch.from_numpy(incoming[1].astype(np.int32)))
    for b, e in pieces:
        absent = None if d["mask"] is None else torch.from_numpy(K.pack_bits(d["mask"][d["dial_of"]][:, b:e]).view(np.int32)).cuda()
        out = rk.count_scores(eq, ec[b:e].contiguous(), thr, skip=skip, idx_base=case.idx_base + b, out=(va, ve), absent=absent,
                              workspace_bytes=ws)
        assert out[0] is va and out[1] is ve
    ha, he = big_a.cpu().numpy(), big_e.cpu().numpy()
    for r in (0, 1, Q + 2, Q + 3):
        assert ha[r] == SENT and he[r] == SENT, "sentinel row %d changed, %s" % (r, case.id)
    return ha[2:2 + Q].copy(), he[2:2 + Q].copy()


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_count_planted(case):
    from zebra_amd import _capi
    d, Q, C_ = case.data(), case.Q, case.C
    rk = _ranker(case.H)
    eq, ec = torch.from_numpy(d["emb_q"]).cuda(), torch.from_numpy(d["emb_c"]).cuda()
    thr_h = _thresholds(rk, case, d, eq)
    thr = torch.from_numpy(thr_h).cuda()
    skip = None if d["skip"] is None else torch.from_numpy(d["skip"]).cuda()
    want_a, want_e = K.expected(case, d)
    if case.nan_rows:                          # a NaN query row: the counts over whatever rank_scores writes for it
        prob = rk.rank_scores(eq, ec).cpu().numpy()
        live = K.present(case, d)
        for q in case.nan_rows:
            want_a[q] = (live[q] & (prob[q] > thr_h[q])).sum()
            want_e[q] = (live[q] & (prob[q] == thr_h[q])).sum()
    ws = case.workspace_bytes(_capi)
    pieces = case.pieces or [(0, C_)]
    zeros = (np.zeros(Q, np.int64), np.zeros(Q, np.int64))
    incoming = case.incoming or zeros
    got = _run(rk, case, d, eq, ec, thr, ws, pieces, incoming, skip)
    again = _run(rk, case, d, eq, ec, thr, ws, pieces, incoming, skip)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), "two calls differ, %s" % case.id
    print(case.id, "above", got[0].tolist(), "equal", got[1].tolist())
    assert np.array_equal(got[0], want_a), "%s: above %s, the host expects %s" % (case.id, got[0].tolist(), want_a.tolist())
    assert np.array_equal(got[1], want_e), "%s: equal %s, the host expects %s" % (case.id, got[1].tolist(), want_e.tolist())
    if case.pieces is None and case.incoming is None:
        # a fresh call (no out): the same numbers; and the recommended workspace where the case cuts it down
        fresh = rk.count_scores(eq, ec, thr, skip=skip, idx_base=case.idx_base,
                                absent=None if d["bits"] is None else torch.from_numpy(d["bits"].view(np.int32)).cuda())
        assert fresh[0].dtype == torch.int32 and fresh[0].shape == (Q,)
        assert np.array_equal(fresh[0].cpu().numpy(), want_a) and np.array_equal(fresh[1].cpu().numpy(), want_e), case.id


# ---- refusals: every ZT_ERR_ARG / ZT_ERR_UNSUPPORTED of the header's contract, before any device call ----------------------
def test_refusals_leave_the_outputs_alone():
    from zebra_amd import _capi
    lib = _capi.lib()
    rk = _ranker(20)
    Q, Nc, H = 5, 40, 20
    a = rk.affinity_score
    w = _capi.AffinityWeights()
    w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b = a.fc1.weight.data_ptr(), a.fc1.bias.data_ptr(), a.fc2.weight.data_ptr(), a.fc2.bias.data_ptr()
    eq = torch.zeros((Q, H), device="cuda")
    ec = torch.zeros((Nc, H), device="cuda")
    thr = torch.full((Q,), 0.25, device="cuda")
    skip = torch.full((Q, 4), -1, dtype=torch.int32, device="cuda")
    bits = torch.zeros((Q, 2), dtype=torch.int32, device="cuda")
    above = torch.full((Q,), SENT, dtype=torch.int32, device="cuda")
    equal = torch.full((Q,), SENT, dtype=torch.int32, device="cuda")
    least = int(lib.zt_affinity_count_workspace_bytes(C.c_int64(Q), C.c_int64(32), C.c_int32(H)))
    need = int(lib.zt_affinity_count_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H)))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = _capi.ptr
    good = dict(eq=p(eq), Q=Q, ec=p(ec), Nc=Nc, H=H, w=C.byref(w), thr=p(thr), skip=p(skip), n_skip=4, idx_base=0, acc=0,
                above=p(above), equal=p(equal), ws=p(ws), ws_bytes=need, absent=p(bits), words=2)

    def call(**kw):
        g = dict(good, **kw)
        return lib.zt_affinity_count(g["eq"], C.c_int64(g["Q"]), g["ec"], C.c_int64(g["Nc"]), C.c_int32(g["H"]), g["w"], g["thr"],
                                     g["skip"], C.c_int32(g["n_skip"]), C.c_int64(g["idx_base"]), C.c_int32(g["acc"]), g["above"],
                                     g["equal"], g["ws"], C.c_int64(g["ws_bytes"]), g["absent"], C.c_int64(g["words"]),
                                     _capi.stream_ptr())

    ARG, UNS = _capi.ZT_ERR_ARG, _capi.ZT_ERR_UNSUPPORTED
    refused = [
        (dict(eq=None), ARG), (dict(ec=None), ARG), (dict(w=None), ARG), (dict(thr=None), ARG), (dict(ws=None), ARG),
        (dict(Q=-1), ARG), (dict(Nc=-1), ARG), (dict(idx_base=-1), ARG),
        (dict(n_skip=-1), ARG), (dict(n_skip=5), ARG), (dict(skip=None, n_skip=1), ARG),
        (dict(words=1), ARG),                                              # ceil(40 / 32) = 2 words needed
        (dict(idx_base=0x7fffffff - Nc + 1), ARG),
        (dict(ws_bytes=least - 1), ARG),
        (dict(H=0), UNS), (dict(H=22), UNS), (dict(H=4356), UNS),
    ]
    for kw, code in refused:
        assert call(**kw) == code, kw
        assert _capi.lib().zt_last_error().decode() != ""
    assert call(above=None) == ARG and call(equal=None) == ARG
    torch.cuda.synchronize()
    assert (above.cpu().numpy() == SENT).all() and (equal.cpu().numpy() == SENT).all()
    # what is NOT refused: Q = 0 touches nothing; Nc = 0 leaves the outputs alone under accumulate and writes zeros without;
    # the smallest workspace, idx_base at the int32 limit, n_skip = 0 without a table, no bits
    assert call(Q=0) == _capi.ZT_OK
    assert call(Nc=0, acc=1, words=0) == _capi.ZT_OK
    torch.cuda.synchronize()
    assert (above.cpu().numpy() == SENT).all() and (equal.cpu().numpy() == SENT).all()
    assert call(Nc=0, words=0) == _capi.ZT_OK
    assert (above.cpu().numpy() == 0).all() and (equal.cpu().numpy() == 0).all()
    assert call(ws_bytes=least, idx_base=0x7fffffff - Nc, skip=None, n_skip=0, absent=None, words=0) == _capi.ZT_OK
    # zero embeddings on the dialled scorer: every pair scores 0, p = 0.5 > 0.25
    assert (above.cpu().numpy() == Nc).all() and (equal.cpu().numpy() == 0).all()
    with pytest.raises(ValueError):
        rk.count_scores(eq, ec, thr, skip=torch.zeros((Q, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        rk.count_scores(eq, ec, thr, absent=bits[:, :1])
    with pytest.raises(ValueError):
        rk.count_scores(eq, ec, thr[:-1])
    with pytest.raises(ValueError):
        rk.count_scores(eq, ec, thr, idx_base=0x7fffffff)
