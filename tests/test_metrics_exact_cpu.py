"""What tests/test_metrics_exact_gpu.py relies on, checked without a GPU and without scikit-learn: oracle/metrics_exact.py on
hand-made cases whose rational values are written out here, against an O(B^2) pair count and (where it imports) scikit-learn;
the torch composition of zebra_amd.evaluation on CPU tensors within 1e-12 of it at every input the GPU file uses and at the
sizes only the composition takes; through zt_link_metrics_plan, that every GPU case reaches the form, padded length and chunk
length its id names and that the B list straddles every seam; and, from the multiplicities alone, that every constructed case
has the run it is named for where it is named for."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT
import test_metrics_exact_gpu as G

try:
    import sklearn.metrics as sk
except ImportError:                               # an optional cross-check, never a reason to skip
    sk = None

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import metrics_exact as X  # noqa: E402

ATOL = 1e-12
f32 = lambda *v: np.array(v, np.float32)


def composition(pos, neg, accuracy=True):
    from zebra_amd import evaluation as ev
    p, n = torch.from_numpy(np.array(pos)), torch.from_numpy(np.array(neg))
    return np.array([float(ev.average_precision(p, n)), float(ev.roc_auc(p, n)),
                     float(ev.accuracy(p, n)) if accuracy else float("nan")])


def sklearn_metrics(pos, neg):
    y = np.concatenate([np.ones(len(pos)), np.zeros(len(neg))])
    sc = np.concatenate([pos, neg]).astype(np.float64)
    return np.array([sk.average_precision_score(y, sc), sk.roc_auc_score(y, sc)])


# ---------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------
HAND = {
    "all_equal": (f32(0.5, 0.5, 0.5), f32(0.5, 0.5, 0.5), (Fraction(1, 2), Fraction(1, 2), Fraction(1))),
    "separated": (f32(0.9, 0.7, 0.8), f32(0.1, 0.3, 0.2), (Fraction(1), Fraction(1), Fraction(1))),
    # positives all 0, negatives all 1: thresholds 1 (tp 0, fp 3) and 0 (tp 3, fp 3): AP = 1 x 3 / 6
    "inverted": (f32(0, 0, 0), f32(1, 1, 1), (Fraction(1, 2), Fraction(0), Fraction(0))),
    # thresholds 0.5 (tp 1, fp 0), 0.25 (1, 1), +-0 (2, 2): AP = 1/2 x 1 + 1/2 x 2/4; AUC = (1/2 x 2/2 + 1/2 x 3/2) / 2
    "signed_zero": (f32(0.0, 0.5), f32(-0.0, 0.25), (Fraction(3, 4), Fraction(5, 8), Fraction(1))),
    "one_pair_above": (f32(0.7), f32(0.2), (Fraction(1), Fraction(1), Fraction(1))),
    "one_pair_equal": (f32(0.3), f32(0.3), (Fraction(1, 2), Fraction(1, 2), Fraction(1))),
    "one_pair_below": (f32(0.2), f32(0.7), (Fraction(1, 2), Fraction(0), Fraction(0))),
    # thresholds 0.8 (1, 0), 0.6 (2, 1), 0.4 (2, 2), 0.2 (3, 3): AP = 1/3 + 1/3 x 2/3 + 1/3 x 3/6; pairs won 5 + 2 halves of 9
    "mixed": (f32(0.8, 0.6, 0.2), f32(0.6, 0.4, 0.2), (Fraction(13, 18), Fraction(2, 3), Fraction(1))),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_on_hand_made_cases(name):
    pos, neg, exact = HAND[name]
    got = X.link_metrics_exact(pos, neg)
    assert got[1] == float(exact[1]) and got[2] == float(exact[2])         # one Fraction, rounded once
    assert abs(got[0] - float(exact[0])) <= 2.0 ** -52, (got, exact)       # fsum of terms rounded once each
    if name in ("all_equal", "inverted", "signed_zero"):                   # (dyadic terms: exact)
        assert got[0] == float(exact[0])
    assert np.allclose(composition(pos, neg), got, rtol=0, atol=ATOL)
    if sk is not None and len(pos) > 0:
        assert np.allclose(sklearn_metrics(pos, neg), got[:2], rtol=0, atol=ATOL)


def test_reference_takes_classes_of_different_sizes_and_refuses_nan():
    # thresholds 0.9 (1, 0), 0.5 (2, 1), 0.1 (2, 3): AP = 1/2 + 1/2 x 2/3; AUC = (1/3 x 3/2 + 2/3 x 4/2) / 2
    got = X.link_metrics_exact(f32(0.9, 0.5), f32(0.5, 0.1, 0.1))
    assert abs(got[0] - float(Fraction(5, 6))) <= 2.0 ** -52 and got[1] == float(Fraction(11, 12)) and np.isnan(got[2])
    with pytest.raises(ValueError):
        X.link_metrics_exact(f32(0.5, np.nan), f32(0.1, 0.2))


@pytest.mark.parametrize("B,decimals", [(1, 1), (2, 1), (37, 0), (150, 1), (300, 1), (300, 2), (300, None), (299, 3)])
def test_reference_auc_is_the_pair_count(B, decimals):
    pos, neg = G.draw(B, False, seed=100 + B)
    if decimals is not None:
        pos, neg = np.round(pos, decimals), np.round(neg, decimals)
    assert X.link_metrics_exact(pos, neg)[1] == X.auc_pairwise(pos, neg)
    neg2 = np.concatenate([neg, neg[: B // 3]])                           # P != N
    assert X.link_metrics_exact(pos, neg2)[1] == X.auc_pairwise(pos, neg2)


def test_rank_reference_on_hand_made_rows():
    prob = f32(0.5, 0.7, 0.5, 0.2, 0.5, 0.9,        # gt 2, eq 2 -> rank 4
               0.0, 0.0, 0.0, 0.0, 0.3, 0.0,        # gt 1, eq 4 -> rank 4;    with the mask: gt 0, eq 1 -> 1.5
               0.9, 0.1, 0.1, 0.1, 0.1, 0.1,        # rank 1
               0.4, 0.9, 0.9, 0.9, 0.9, 0.9).reshape(4, 6)      # rank 6;     with the mask: skipped
    r = X.rank_exact(prob)
    assert list(r["gt"]) == [2, 1, 0, 5] and list(r["eq"]) == [2, 4, 0, 0] and list(r["rank"]) == [4.0, 4.0, 1.0, 6.0]
    assert r["exact"] == [Fraction(1, 4) + Fraction(1, 4) + 1 + Fraction(1, 6), 1, 1, 4, 4]
    ix = np.array([[1] * 6, [1, -1, 1, -1, -1, -1], [1] * 6, [-1, 1, 1, 1, 1, 1]])
    r = X.rank_exact(prob, ix)
    assert list(r["rank"]) == [4.0, 1.5, 1.0, 0.0]
    assert r["exact"] == [Fraction(1, 4) + Fraction(2, 3) + 1, 1, 2, 3, 3]
    assert list(r["sums"]) == [float(v) for v in r["exact"]]


# ---------------------------------------------------------------------------------------------------------
# the GPU file's cases
# ---------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_form_its_id_names():
    from zebra_amd import _capi
    ids = G.link_case_ids()
    assert len(ids) == len(set(ids))
    for case in ids:
        pos, neg = G.link_inputs(case)
        p = _capi.link_metrics_plan(pos.size)
        tag = ("single-B%d-n%d-per%d" % (pos.size, p["n2"], p["n2"] // p["threads"]) if p["form"] == _capi.METRICS_FORM_SINGLE
               else "split-B%d-n%d" % (pos.size, p["n2"]))
        assert p["form"] in (_capi.METRICS_FORM_SINGLE, _capi.METRICS_FORM_SPLIT) and "-%s" % tag in case, (case, p)
        assert p["threads"] == G.MT_THREADS
    pers = {p: _capi.link_metrics_plan(B)["n2"] // G.MT_THREADS for p, B in G.SINGLE_LAYOUT_B.items()}
    assert pers == {1: 1, 2: 2, 4: 4, 8: 8, 16: 16}
    assert 2 * G.SINGLE_LAYOUT_B[1] < _capi.link_metrics_plan(G.SINGLE_LAYOUT_B[1])["n2"]          # padding behind the last run
    assert any(2 * B == _capi.link_metrics_plan(B)["n2"] for B in G.SINGLE_LAYOUT_B.values())     # and none


def test_the_batch_sizes_straddle_every_seam():
    from zebra_amd import _capi
    sizes = set(G.SINGLE_B + G.SPLIT_B)
    plans = {B: _capi.link_metrics_plan(B) for B in sizes | {16385}}
    for lo in (512, 1024, 2048, 4096):
        assert {lo, lo + 1} <= sizes and 2 * plans[lo]["n2"] == plans[lo + 1]["n2"], lo
    assert {8192, 8193} <= sizes
    assert plans[8192]["form"] == _capi.METRICS_FORM_SINGLE and plans[8193]["form"] == _capi.METRICS_FORM_SPLIT
    assert 16384 in sizes and plans[16384]["form"] == _capi.METRICS_FORM_SPLIT
    assert plans[16385]["form"] == _capi.METRICS_FORM_REFUSED                    # (the composition takes it: below)
    assert {plans[B]["n2"] // G.MT_THREADS for B in G.SINGLE_B} == {1, 2, 4, 8, 16}
    assert {plans[B]["n2"] for B in G.SPLIT_B} == {32768}


@pytest.mark.parametrize("per", sorted(G.SINGLE_LAYOUT_B))
def test_the_layout_has_the_runs_it_names(per):
    B = G.SINGLE_LAYOUT_B[per]
    mult, names = G.layout(per, B)
    runs = G.runs(mult)
    n = 2 * B
    assert sum(m[0] for m in mult) == sum(m[1] for m in mult) == B
    chunk = lambda i: i // per
    start = {k: runs[v][0] for k, v in names.items()}
    end = {k: runs[v][0] + runs[v][1] - 1 for k, v in names.items()}              # the run's last element
    mixed = lambda k: runs[names[k]][2] > 0 and runs[names[k]][3] > 0
    # the first run spans several chunks
    assert start["first"] == 0 and chunk(end["first"]) >= 2 and mixed("first")
    # a run that ends in another chunk than it starts in, at a chunk's last element, covering >= 3 whole chunks ...
    assert (end["mid"] + 1) % per == 0 and chunk(end["mid"]) - chunk(start["mid"]) >= 4 and mixed("mid")
    if per > 1:
        # ... starts mid-chunk, and the owner walk [chunk start, run start) begins at a POSITIVE (the previous run's positives lie
        # last: the label is the low bit of the sorted word)
        assert start["mid"] % per != 0
        first_start, first_len, first_pos, _ = runs[names["first"]]
        owner_first = chunk(start["mid"]) * per
        assert start["mid"] == first_start + first_len and owner_first >= first_start + first_len - first_pos
    else:
        assert all(s % per == 0 for s, _, _, _ in runs)                          # per = 1: every owner walk is empty
    # one element at a chunk's first element, directly after the long run
    assert start["single"] % per == 0 and runs[names["single"]][1] == 1 and start["single"] == end["mid"] + 1
    # a run that starts exactly at a chunk's first element and ends in a later chunk
    assert start["aligned"] % per == 0 and chunk(end["aligned"]) > chunk(start["aligned"]) and mixed("aligned")
    # the last run ends at n - 1 and began in an earlier chunk
    assert end["last"] == n - 1 and chunk(start["last"]) < chunk(end["last"]) and mixed("last")
    # and the generated scores have exactly these multiplicities
    pos, neg = G.link_inputs("layout-%s" % G.plan_tag(B))
    lv = np.unique(np.concatenate([pos, neg]))[::-1]
    assert [(int(np.sum(pos == v)), int(np.sum(neg == v))) for v in lv] == mult


@pytest.mark.parametrize("B", sorted(set(G.SINGLE_LAYOUT_B.values())))
def test_the_whole_cases_are_what_they_are_named(B):
    for name, mult in G.whole_cases(B).items():
        pos, neg = G.link_inputs("whole-%s-%s" % (G.plan_tag(B), name))
        assert sum(m[0] for m in mult) == sum(m[1] for m in mult) == B == pos.size
        both = np.concatenate([pos, neg])
        if name == "all_equal":
            assert np.unique(both).size == 1
        elif name == "all_distinct":
            assert np.unique(both).size == 2 * B
        else:
            assert all((a == 0) != (b == 0) for a, b in mult) and np.intersect1d(pos, neg).size == 0
            assert all((mult[i][0] == 0) != (mult[i + 1][0] == 0) for i in range(len(mult) - 1))
            assert max(max(m) for m in mult) > 1


@pytest.mark.parametrize("B", [8193, 16384])
def test_the_split_cases_are_what_they_are_named(B):
    for name, mult in G.split_cases(B).items():
        pos, neg = G.link_inputs("levels-%s-%s" % (G.plan_tag(B), name))
        assert sum(m[0] for m in mult) == sum(m[1] for m in mult) == B == pos.size
        sp, sn = np.sort(pos)[::-1], np.sort(neg)[::-1]                   # the kernel's two runs, descending
        if name == "pos_above_and_below":
            assert sp[0] > sn[0] and sp[-1] < sn[-1]                      # run_upper(negatives) = 0 and = B
        elif name == "absent_levels":
            assert np.intersect1d(pos, neg).size == 0
        elif name == "shared_ends":
            assert sp[0] == sn[0] and sp[B - 1] == sn[B - 1] and sp[0] == sp[1] and sn[B - 1] == sn[B - 2]
        else:
            assert np.unique(np.concatenate([pos, neg])).size == 1


def test_the_special_cases_hold_what_they_are_named_for():
    pos, neg = G.link_inputs("special-%s-pool8200" % G.plan_tag(8200))
    assert list(pos[:2]) == [0.0, 0.5] and list(neg[:2]) == [0.0, 0.25] and np.signbit(neg[0]) and not np.signbit(pos[0])
    for name, B in (("pool64", 64), ("pool1300", 1300), ("pool8200", 8200)):
        pos, neg = G.link_inputs("special-%s-%s" % (G.plan_tag(B), name))
        for x in (pos, neg):
            assert np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x)) and np.any(x == 1.0)
            assert np.any((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)) and np.any(x < 0) and np.any(x > 1)
    # +-0 is one level: the reference gives the same values with every zero made +0
    for case in [c for c in G.link_case_ids() if c.startswith("special-")]:
        pos, neg = G.link_inputs(case)
        assert np.array_equal(X.link_metrics_exact(pos, neg), X.link_metrics_exact(pos + np.float32(0), neg + np.float32(0)))


@pytest.mark.parametrize("case", G.link_case_ids())
def test_the_composition_matches_exact_counts(case):
    pos, neg = G.link_inputs(case)
    want = G.link_reference(case)
    got = composition(pos, neg)
    assert np.all(np.abs(got - want) <= ATOL), (got, want)
    if sk is not None:
        assert np.all(np.abs(sklearn_metrics(pos, neg) - want[:2]) <= ATOL)


@pytest.mark.parametrize("P,N,decimals", [(16385, 16385, None), (16385, 16385, 2), (300, 211, 1), (1, 5, None), (2049, 4097, 3)])
def test_the_composition_at_the_sizes_only_it_takes(P, N, decimals):
    pos, neg = G.draw(max(P, N), False, seed=P + N)
    pos, neg = pos[:P], neg[:N]
    if decimals is not None:
        pos, neg = np.round(pos, decimals), np.round(neg, decimals)
    want = X.link_metrics_exact(pos, neg)
    got = composition(pos, neg, accuracy=P == N)
    assert np.all(np.abs(got[:2] - want[:2]) <= ATOL), (got, want)
    assert P != N or got[2] == want[2]
    if sk is not None:
        assert np.all(np.abs(sklearn_metrics(pos, neg) - want[:2]) <= ATOL)


def test_the_rank_inputs_hold_the_planted_rows():
    assert any(G.rank_planted(Q, Cn) for Q in G.RANK_Q for Cn in G.RANK_C)
    assert {1, 65, 66, 129} <= set(G.RANK_C) and {16, 17, 1024, 1025} <= set(G.RANK_Q)
    for Q in G.RANK_Q:
        for Cn in G.RANK_C:
            for rounded in (True, False):
                prob, ix = G.rank_inputs(Q, Cn, rounded)
                assert np.all(prob[ix < 0] == G.ABSENT) and prob[ix >= 0].max() <= 1.0
                if not G.rank_planted(Q, Cn):
                    continue
                assert prob[0, 0] == 0.0 and ix[0, 0] >= 0 and np.any(ix[0, 1:] < 0)
                assert ix[1, 0] < 0 and ix[2, 0] >= 0 and np.all(ix[2, 1:] < 0) and np.all(prob[3] == 0.5) and np.all(ix[3] >= 0)
                if Cn > 2:
                    assert np.any((prob[0, 1:] == 0.0) & (ix[0, 1:] >= 0))        # a present tie at exactly 0.0
                if rounded and Q >= 1024 and Cn >= 64:
                    assert np.count_nonzero(G.oracle().rank_exact(prob, ix)["eq"]) > Q // 4   # many ties with column 0
