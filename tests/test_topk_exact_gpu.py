"""The fused top-K (csrc/rank_topk.hip through TGN.topk_scores) on the planted cases of tests/helpers_topk_planted.py, all exact:
(a) the returned indices are the host's lexsort(-level, column)[:K]; (b) the returned probabilities are rank_scores' bits at
those columns; (c) rank_scores' own output has the planted structure -- distinct levels strictly ordered, equal levels equal
bits.  Every call runs twice, once into a view of a larger buffer whose sentinel rows must survive.  No tolerance, no skip.
tests/test_topk_exact_cpu.py shows that each case reaches the seam its id names."""
import functools
import types

import numpy as np
import pytest
import torch

import helpers_topk_planted as P
from helpers_topk import select_topk

pytestmark = pytest.mark.gpu
SENT_I, SENT_P = -77, 0.3125           # the sentinel rows around an output view
JUNK_P = 0.75                          # what an empty slot's probability holds on the way in: never read


@functools.lru_cache(maxsize=None)
def _ranker(H):
    """TGN.rank_scores / topk_scores on the dialled MergeLayer of width H alone"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN
    m = MergeLayer(H, H, H, 1)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), P.scorer_weights(H)):
            p.copy_(torch.from_numpy(w))
    holder = types.SimpleNamespace(affinity_score=m.to("cuda"), device=torch.device("cuda"))
    for name in ("rank_scores", "topk_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    return holder


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _structure(prob_row, S_row, what):
    """(c): over the present columns, sorted by planted score: a larger score has strictly larger bits, an equal one equal bits
    (probabilities are >= +0: the bits order as unsigned)"""
    live = ~np.isnan(S_row)
    s, b = S_row[live], _bits(prob_row)[live].astype(np.int64)
    order = np.argsort(s, kind="stable")
    s, b = s[order], b[order]
    up = s[1:] > s[:-1]
    assert (b[1:][up] > b[:-1][up]).all(), "rank_scores: distinct levels without strictly ordered bits, %s" % (what,)
    assert (b[1:][~up] == b[:-1][~up]).all(), "rank_scores: equal levels with different bits, %s" % (what,)
    assert (_bits(prob_row)[~live] == 0).all(), "rank_scores: an absent column is not +0.0f, %s" % (what,)


def _bits_of_score(prob_row, S_row, s):
    """rank_scores' bits for planted score s: those of a pool column that carries it"""
    cols = np.nonzero(S_row == s)[0]
    assert len(cols) > 0
    return prob_row[cols[0]]


def _call(rk, case, eq, ec, ix, absent, ws, idx_base=0, incoming=None):
    """one selection, twice: plainly (no incoming list: fresh outputs), and into a view of a larger buffer between sentinel rows
    -- with the incoming list, or with an all-empty one.  Both must agree to the bit; (idx, prob) on the host."""
    Q, K = case.Q, case.K
    kw = dict(cand_idx=ix, absent=absent, workspace_bytes=ws, idx_base=idx_base)

    def into_view():
        big_i = torch.full((Q + 4, K), SENT_I, dtype=torch.int32, device="cuda")
        big_p = torch.full((Q + 4, K), SENT_P, dtype=torch.float32, device="cuda")
        vi, vp = big_i[2:2 + Q], big_p[2:2 + Q]
        if incoming is None:
            vi.fill_(-1)
            vp.fill_(JUNK_P)
        else:
            vi.copy_(torch.from_numpy(incoming[0]))
            vp.copy_(torch.from_numpy(incoming[1]))
        out = rk.topk_scores(eq, ec, K, out=(vi, vp), **kw)
        assert out[0] is vi and out[1] is vp
        hi, hp = big_i.cpu().numpy(), big_p.cpu().numpy()
        for r in (0, 1, Q + 2, Q + 3):
            assert (hi[r] == SENT_I).all() and (hp[r] == np.float32(SENT_P)).all(), "sentinel row %d changed, %s" % (r, case.id)
        return hi[2:2 + Q].copy(), hp[2:2 + Q].copy()

    def plainly():
        got = rk.topk_scores(eq, ec, K, **kw)
        return got[0].cpu().numpy(), got[1].cpu().numpy()

    if incoming is not None:
        runs = [into_view(), into_view()]
    elif case.C == 0:                           # (C = 0 under accumulate leaves the output alone: nothing to compare)
        runs = [plainly(), plainly()]
    else:
        runs = [plainly(), into_view()]
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(_bits(r[1]), _bits(runs[0][1])), "two calls differ, %s" % case.id
    return runs[0]


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_topk_planted(case):
    from zebra_amd import _capi
    d, Q, K, C_ = case.data(), case.Q, case.K, case.C
    rk = _ranker(case.H)
    eq, ec = torch.from_numpy(d["emb_q"]).cuda(), torch.from_numpy(d["emb_c"]).cuda()
    ix = None if d["idx"] is None else torch.from_numpy(d["idx"]).cuda()
    absent = None if d["bits"] is None else torch.from_numpy(d["bits"].view(np.int32)).cuda()
    dial_of, D, S = d["dial_of"], d["D"], d["S"]
    prob = rk.rank_scores(eq, ec, ix).cpu().numpy()
    assert prob.shape == (Q, C_)
    # (c) the planted structure, once per dial; queries that share a dial share their rows bit for bit
    first = {}
    for q in range(Q):
        if q in case.nan_rows:
            continue
        if dial_of[q] not in first:
            first[dial_of[q]] = q
            _structure(prob[q], S[dial_of[q]], (case.id, q))
    if Q > D and not case.nan_rows:
        assert np.array_equal(_bits(prob), _bits(prob[:D])[dial_of]), "queries of one dial differ, %s" % case.id
    if "ones" in case.id:
        assert ((prob == np.float32(1.0)).sum(axis=1) >= K // 2).all()
    if "zero" in case.id:
        assert ((_bits(prob) == 0).sum(axis=1) >= C_ - K // 2).all()

    base = P.IDX_BASE_ACC if d["incoming"] is not None else 0
    want_i, want_s = P.expected(S, K, d["mask"], base, d["incoming"])                  # (a): the host alone
    want_p = np.zeros((D, K), np.float32)                                               # (b): rank_scores' bits there
    for dial, q in first.items():
        for j in range(K):
            if want_i[dial, j] >= 0:
                c = want_i[dial, j] - base
                want_p[dial, j] = prob[q, c] if 0 <= c < C_ else _bits_of_score(prob[q], S[dial], want_s[dial, j])
    want_i, want_p = want_i[dial_of].astype(np.int32), want_p[dial_of]
    for q in case.nan_rows:                     # a NaN query row: the selection over whatever rank_scores writes for it
        wi, wp = select_topk(prob[q:q + 1], None if d["idx"] is None else d["idx"][q:q + 1], K)
        want_i[q], want_p[q] = wi[0], wp[0]

    ws = case.workspace_bytes(_capi)
    incoming = None
    if d["incoming"] is not None:
        inc_i = d["incoming"]["idx"][dial_of].astype(np.int32)
        inc_p = np.full((Q, K), JUNK_P, np.float32)
        for q in range(Q):
            for j in range(K):
                s = d["incoming"]["s"][dial_of[q], j]
                if inc_i[q, j] >= 0:
                    inc_p[q, j] = np.nan if np.isnan(s) else _bits_of_score(prob[first[dial_of[q]]], S[dial_of[q]], s)
        incoming = (inc_i, inc_p)
    if case.pieces is None:
        got = _call(rk, case, eq, ec, ix, absent, ws, base, incoming)
    else:                                       # the pool in pieces, each with its own workspace size, accumulated
        assert ix is None and absent is None
        out = None
        for s, e in case.pieces:
            out = rk.topk_scores(eq, ec[s:e].contiguous(), K, idx_base=s, out=out)
        again = None
        for s, e in case.pieces:
            again = rk.topk_scores(eq, ec[s:e].contiguous(), K, idx_base=s, out=again)
        assert torch.equal(out[0], again[0]) and torch.equal(out[1].view(torch.int32), again[1].view(torch.int32))
        got = (out[0].cpu().numpy(), out[1].cpu().numpy())
    assert got[0].dtype == np.int32 and got[0].shape == (Q, K) and got[1].shape == (Q, K)
    bad = np.nonzero((got[0] != want_i).any(axis=1))[0]
    assert len(bad) == 0, "%s: indices differ from the host expectation in queries %s; query %d got %s, want %s" % (
        case.id, bad[:8].tolist(), bad[0], got[0][bad[0]].tolist(), want_i[bad[0]].tolist())
    assert np.array_equal(_bits(got[1]), _bits(want_p)), "%s: probabilities are not rank_scores' bits" % case.id
    if C_ < K and d["incoming"] is None:
        assert (got[0][:, C_:] == -1).all() and (_bits(got[1][:, C_:]) == 0).all()      # the tail reads -1 and +0.0f
