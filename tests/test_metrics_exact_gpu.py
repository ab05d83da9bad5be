"""The metrics kernels -- zt_link_metrics (csrc/scoring.hip: k_link_metrics up to 8192 pairs, k_link_metrics_split to 16384,
behind zt::link_metrics_plan) and zt_rank_metrics (csrc/rank.hip: k_rank_metrics) -- against the exact counts of
oracle/metrics_exact.py (pinned in tests/test_metrics_exact_cpu.py, which also shows without a GPU that every case below
reaches the form, padded length and chunk length its id names, that the B list straddles every seam of the plan and that every
constructed case has the run it is named for where it is named for).

Bounds, nothing fitted: |AP, AUC - exact| <= 1e-12 (what the suite asserts of this kernel everywhere; one miscounted element at
the largest B moves AUC by 1 / (2 B^2) = 1.9e-9); accuracy, a ratio of an integer count: the reference's bits; ranks: equal;
the rank sums: Q 2^-53 max(1, exact sum), the bound of a first-to-last float64 addition of Q correctly rounded quotients; the
Hits counts and the query count: equal.

Every case reads its scores out of one larger device buffer with NaN in front, between and behind (a read outside changes the
counts), once 16-byte aligned and once one float off; writes out[3] / acc[5] / rank[Q] in front of sentinel words; runs twice
(equal bits); and once more onto non-zero starting values.

The single form (thread t owns elements [t per, (t + 1) per) of the sorted n2 = 1024 per words; a run of equal scores that
ends in a chunk other than the one it starts in takes its `tps before the run` from the owner walk):
  random       B over every n2 seam, clipped normals unrounded / to one decimal / to three decimals
  constructed  per = 1, 2, 4, 8, 16: runs placed by their multiplicities (layout()), see SINGLE_LAYOUT_B and whole_cases()
  special      +-0, 0 and 1 on both sides, denormals, scores outside [0, 1]
The split form: B = 8193 .. 16384 the same three draws; constructed levels (split_cases()); the special pool.
Rank metrics: Q over the 16 waves and the chunks of 1024 queries, C over the ballots of 64 lanes; planted rows (rank_inputs()).

Measured on an MI355X ("The evaluation metrics against exact counts"): largest |AP, AUC - exact| 2.2e-16 in either
form; the rank sums use at most 0.64 of their bound (Q = 1, where a non-zero starting sum adds a second rounding; at most 0.24
from Q = 16 on).  One thing wrong found and fixed: -0.0 and +0.0 were two thresholds (desc_key); on the library before the fix
the five cases that hold a -0.0 fail and no other.  Eight single-line arithmetic defects put into the kernels on a scratch copy
each fail between 5 and 53 of this file's 162 cases."""
import ctypes as C
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_metrics_run_gpu import draw

pytestmark = pytest.mark.gpu

ATOL = 1e-12
SINGLE, SPLIT = 1, 2
MT_THREADS = 1024
SENT = 777.25
SINGLE_B = (1, 2, 3, 511, 512, 513, 1024, 1025, 1536, 2048, 2049, 4096, 4097, 8191, 8192)
SPLIT_B = (8193, 12000, 16383, 16384)
ROUNDS = (None, 1, 3)                          # decimals the draw is rounded to
SINGLE_LAYOUT_B = {1: 300, 2: 1024, 4: 1300, 8: 3000, 16: 8192}   # per -> B; 300: padding follows the last run; 1024, 8192: 2B = n2
RANK_Q = (1, 16, 17, 1024, 1025, 2049)
RANK_C = (1, 2, 64, 65, 66, 129)
ABSENT = 2.0                                   # what an absent entry's probability slot holds here: above every real one


def oracle():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import metrics_exact
    return metrics_exact


def expected_plan(B):
    """(form, n2, per) a case is ABOUT, restated from the kernels' comments, not read from the plan"""
    if B <= 8192:
        n2 = MT_THREADS
        while n2 < 2 * B:
            n2 *= 2
        return SINGLE, n2, n2 // MT_THREADS
    m2 = MT_THREADS
    while m2 < B:
        m2 *= 2
    return SPLIT, 2 * m2, 0


def plan_tag(B):
    form, n2, per = expected_plan(B)
    return "single-B%d-n%d-per%d" % (B, n2, per) if form == SINGLE else "split-B%d-n%d" % (B, n2)


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
def from_levels(mult, seed):
    """mult: [(n_pos, n_neg), ...] per distinct level, DESCENDING.  Distinct float32 levels inside (0.05, 0.95), each class
    shuffled: the sorted position of every run follows from the multiplicities alone (runs())."""
    L = len(mult)
    levels = np.linspace(0.95, 0.05, L).astype(np.float32) if L > 1 else np.array([0.5], np.float32)
    assert L == 1 or np.all(levels[1:] < levels[:-1])
    rng = np.random.RandomState(seed)
    pos = np.repeat(levels, [m[0] for m in mult])
    neg = np.repeat(levels, [m[1] for m in mult])
    rng.shuffle(pos)
    rng.shuffle(neg)
    return pos, neg


def runs(mult):
    """[(start, length, n_pos, n_neg)] of every run in the sorted order of the 2B scores"""
    out, s = [], 0
    for p, q in mult:
        out.append((s, p + q, p, q))
        s += p + q
    return out


def layout(per, B):
    """The single form's constructed input for one chunk length: multiplicities and the index (into them) of every named run.
    With p = per and h = p // 2, sorted positions:
      first      [0, 3p + h)          the first run, over chunks 0 .. 3; its positives lie last (the label is the low key bit),
                                      so chunk 3 begins with positives
      mid        [3p + h, 8p)         starts mid-chunk (p >= 2) behind those positives, covers chunks 4 .. 7 whole and ends at a
                                      chunk's last element
      single     [8p, 8p + 1)         one element at a chunk's first element, directly after the long run
      gap        [8p + 1, 10p)
      aligned    [10p, 12p + 1)       starts at a chunk's first element and ends in chunk 12
      filler     runs of 1, 2, 1, 3, ... elements
      last       [2B - 2p - 1, 2B)    ends at n - 1 after crossing two chunk boundaries
    """
    p, h, n = per, per // 2, 2 * B
    fixed = [("first", 3 * p + h), ("mid", 8 * p - (3 * p + h)), ("single", 1), ("gap", 2 * p - 1), ("aligned", 2 * p + 1)]
    last_len = 2 * p + 1
    used = sum(length for _, length in fixed) + last_len
    assert used + 8 <= n
    mult, names = [], {}
    need_p = need_n = B

    def take(length, n_pos):
        nonlocal need_p, need_n
        mult.append((n_pos, length - n_pos))
        need_p -= n_pos
        need_n -= length - n_pos

    for name, length in fixed:
        names[name] = len(mult)
        take(length, 1 if length == 1 else (length + 1) // 2)          # mixed; `first` has >= h + 1 positives
    last_pos = last_len // 2
    fill = n - used
    cyc, k = (1, 2, 1, 3), 0
    while fill > 0:
        length = min(cyc[k % 4], fill)
        k += 1
        want_p, want_n = need_p - last_pos, need_n - (last_len - last_pos)
        n_pos = min(length, want_p) if want_p >= want_n else length - min(length, want_n)
        if length > 1 and 0 < want_p and 0 < want_n:                   # a mixed run where both classes still have room
            n_pos = min(max(n_pos, 1), length - 1)
        take(length, n_pos)
        fill -= length
    names["last"] = len(mult)
    take(last_len, last_pos)
    assert need_p == 0 and need_n == 0, (need_p, need_n)
    return mult, names


def whole_cases(B):
    """name -> multiplicities of the inputs that are one property from end to end"""
    rng = np.random.RandomState(B)
    lab = rng.permutation(np.arange(2 * B) % 2)
    alt, k, left = [], 0, B
    while left > 0:
        m = min((1, 2, 3)[k % 3], left)
        alt += [(m, 0), (0, m)]
        left -= m
        k += 1
    return {"all_equal": [(B, B)],
            "all_distinct": [(1, 0) if v else (0, 1) for v in lab],
            "alternating": alt}


def split_cases(B):
    """name -> multiplicities for the two-run form"""
    def mixed(n_each, seed):
        """levels of 1 .. 4 scores per class, n_each in total per class"""
        rng, out, a, b = np.random.RandomState(seed), [], n_each, n_each
        while a > 0 or b > 0:
            x, y = min(a, int(rng.randint(0, 4))), min(b, int(rng.randint(0, 4)))
            if x + y:
                out.append((x, y))
            a, b = a - x, b - y
        return out
    alt, k, left = [], 0, B
    while left > 0:
        m = min((1, 2, 3)[k % 3], left)
        alt += [(m, 0), (0, m)]
        left -= m
        k += 1
    return {"pos_above_and_below": [(3, 0), (0, 2)] + mixed(B - 5, 1) + [(0, 3), (2, 0)],      # run_upper = 0 and = B
            "absent_levels": alt,
            "shared_ends": [(2, 3)] + mixed(B - 5, 2) + [(3, 2)],                              # shared at index 0 and at B - 1
            "all_equal": [(B, B)]}


SPECIAL_POOL = np.array([0.0, -0.0, 1.0, 1e-45, 1e-40, -1e-45, -1e-40, 1.17549435e-38, -0.5, 1.5, 2.0, -3.0, 0.25, 0.5, 0.75,
                         0.99999994], np.float32)


def special(name):
    if name == "signed_zero_example":
        return np.array([0.0, 0.5], np.float32), np.array([-0.0, 0.25], np.float32)
    if name == "zeros_only":                   # +0 and -0 within each class and across: one level, AP = AUC = 0.5, acc = 1
        return np.array([0.0, -0.0, -0.0, 0.0, 0.0], np.float32), np.array([-0.0, 0.0, -0.0, -0.0, 0.0], np.float32)
    B = {"pool64": 64, "pool1300": 1300, "pool8200": 8200}[name]
    rng = np.random.RandomState(B)
    pos, neg = SPECIAL_POOL[rng.randint(0, len(SPECIAL_POOL), B)], SPECIAL_POOL[rng.randint(0, len(SPECIAL_POOL), B)]
    k = len(SPECIAL_POOL)
    pos[B - k:], neg[B - k:] = SPECIAL_POOL[rng.permutation(k)], SPECIAL_POOL[rng.permutation(k)]   # every value, both classes
    if name == "pool8200":                     # the four-element example inside a larger batch
        pos[:2], neg[:2] = special("signed_zero_example")
        pos[2:6000], neg[2:6000] = (x[2:6000] for x in draw(6000, False, seed=4))
    return pos.copy(), neg.copy()


def link_case_ids():
    ids = ["random-%s-r%s" % (plan_tag(B), r) for B in SINGLE_B + SPLIT_B for r in ROUNDS]
    ids += ["layout-%s" % plan_tag(B) for B in SINGLE_LAYOUT_B.values()]
    ids += ["whole-%s-%s" % (plan_tag(B), name) for B in SINGLE_LAYOUT_B.values() for name in whole_cases(4)]
    ids += ["levels-%s-%s" % (plan_tag(B), name) for B in (8193, 16384) for name in split_cases(16)]
    ids += ["special-%s-%s" % (plan_tag(len(special(name)[0])), name)
            for name in ("signed_zero_example", "zeros_only", "pool64", "pool1300", "pool8200")]
    return ids


@functools.lru_cache(maxsize=None)
def link_inputs(case):
    """(pos, neg) float32, read-only, of a case id"""
    kind, rest = case.split("-", 1)
    B = int(rest.split("-B")[1].split("-")[0])
    tail = rest.rsplit("-", 1)[1]
    if kind == "random":
        r = None if tail == "rNone" else int(tail[1:])
        pos, neg = draw(B, False, seed=9000 + B)
        if r is not None:
            pos, neg = np.round(pos, r), np.round(neg, r)
    elif kind == "layout":
        pos, neg = from_levels(layout(expected_plan(B)[2], B)[0], B)
    elif kind == "whole":
        pos, neg = from_levels(whole_cases(B)[tail], B + 1)
    elif kind == "levels":
        pos, neg = from_levels(split_cases(B)[tail], B + 2)
    else:
        pos, neg = special(tail)
    assert pos.dtype == np.float32 and neg.dtype == np.float32 and pos.shape == neg.shape == (B,)
    pos.setflags(write=False)
    neg.setflags(write=False)
    return pos, neg


@functools.lru_cache(maxsize=None)
def link_reference(case):
    want = oracle().link_metrics_exact(*link_inputs(case))
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def rank_inputs(Q, Cn, rounded):
    """(prob float32 [Q, C], cand_idx int32 [Q, C] with about 10 % absent).  Absent slots of prob hold ABSENT (above every
    real probability: counted, it moves the rank).  From Q >= 16 and C >= 2 on, the first rows are planted:
      0  a positive of exactly 0.0, candidates of 0.0 and absent ones beside it
      1  an absent positive (skipped: rank 0)
      2  every candidate absent but the positive (rank 1)
      3  every entry equal (rank 1 + (C - 1) / 2)"""
    rng = np.random.RandomState(7000 + 131 * Q + Cn + (1 if rounded else 0))
    prob = rng.uniform(0.0, 1.0, (Q, Cn)).astype(np.float32)
    if rounded:
        prob = np.round(prob, 2)
    ix = rng.randint(0, 1000, (Q, Cn)).astype(np.int32)
    ix[rng.uniform(size=(Q, Cn)) < 0.1] = -1
    if Q >= 16 and Cn >= 2:
        prob[0, 0] = 0.0
        prob[0, 1::3] = 0.0
        ix[0, 0] = 5
        ix[0, 1::2] = -1
        ix[0, Cn - 1] = -1
        ix[1, 0] = -1
        ix[2, 0], ix[2, 1:] = 9, -1
        prob[3, :] = 0.5
        ix[3, :] = 3
    prob[ix < 0] = ABSENT
    prob.setflags(write=False)
    ix.setflags(write=False)
    return prob, ix


def rank_planted(Q, Cn):
    return Q >= 16 and Cn >= 2


# ---------------------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------------------
def carve(arrays, off, fill):
    """The arrays (one dtype) as views of ONE device buffer: `fill` in front (4 + off elements), between and behind; every
    view begins at a multiple of four elements plus `off` (the allocation itself is 256-byte aligned)."""
    starts, o = [], 4 + off
    for a in arrays:
        starts.append(o)
        o = (o + a.size + 3) // 4 * 4 + 4 + off
    host = np.full(o + 8, fill, arrays[0].dtype)
    for a, s in zip(arrays, starts):
        host[s:s + a.size] = a.reshape(-1)
    dev = torch.from_numpy(host).cuda()
    views = [dev[s:s + a.size].view(a.shape) for a, s in zip(arrays, starts)]
    for v in views:
        assert v.data_ptr() % 16 == 4 * off
    return views


def guarded(n, start=None):
    """(buffer, view of n float64 behind and in front of sentinel words)"""
    buf = torch.full((n + 6,), SENT, dtype=torch.float64, device="cuda")
    view = buf[3:3 + n]
    view.copy_(torch.zeros(n, dtype=torch.float64) if start is None else torch.as_tensor(start, dtype=torch.float64))
    return buf, view


def untouched(buf, n):
    h = buf.cpu().numpy()
    return bool(np.all(h[:3] == SENT) and np.all(h[3 + n:] == SENT))


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


WORST = {}


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))
    print("largest error so far, %s: %.3e" % (key, WORST[key]))


# ---------------------------------------------------------------------------------------------------------
# zt_link_metrics
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", link_case_ids())
def test_link_metrics_against_exact_counts(case):
    from zebra_amd import _capi
    from zebra_amd import evaluation as ev
    pos, neg = link_inputs(case)
    B = pos.size
    form, n2, _ = expected_plan(B)
    p = _capi.link_metrics_plan(B)
    assert (p["form"], p["n2"]) == (form, n2)
    want = link_reference(case)
    results = []
    for off in (0, 1):
        dp, dn = carve([pos, neg], off, np.float32("nan"))
        buf, out = guarded(3)
        ev.link_metrics(dp, dn, out=out)                                  # added to zeros: the kernel's own bits
        got = out.cpu().numpy()
        assert untouched(buf, 3)
        results.append(got)
        err = np.abs(got[:2] - want[:2])
        print("%s off=%d  AP %.17g (exact %.17g)  AUC %.17g (exact %.17g)  |err| = %s" % (case, off, got[0], want[0], got[1], want[1], err))
        note("single" if form == SINGLE else "split", err.max())
        assert np.all(err <= ATOL), (got, want)
        assert bits(got[2]) == bits(want[2]), (got[2], want[2])           # accuracy: an integer count over B
        fresh = ev.link_metrics(dp, dn).cpu().numpy()                     # the storing (non-accumulating) call
        assert np.array_equal(bits(fresh), bits(got))
    assert np.array_equal(bits(results[0]), bits(results[1]))             # twice, aligned and one float off: equal bits
    start = np.array([0.375, -2.5, 11.0])
    buf, out = guarded(3, start)
    ev.link_metrics(dp, dn, out=out)
    assert untouched(buf, 3)
    assert np.array_equal(bits(out.cpu().numpy()), bits(start + results[0]))   # out[i] += value: one float64 addition each


# ---------------------------------------------------------------------------------------------------------
# zt_rank_metrics
# ---------------------------------------------------------------------------------------------------------
def run_rank(prob, ix, acc, rank):
    from zebra_amd import _capi
    Q, Cn = prob.shape
    _capi.check(_capi.lib().zt_rank_metrics(_capi.ptr(prob), _capi.ptr(ix), C.c_int64(Q), C.c_int64(Cn), _capi.ptr(rank),
                                            _capi.ptr(acc), _capi.stream_ptr()), "zt_rank_metrics")


@pytest.mark.parametrize("rounded", [True, False])
@pytest.mark.parametrize("Cn", RANK_C)
@pytest.mark.parametrize("Q", RANK_Q)
def test_rank_metrics_against_exact_counts(Q, Cn, rounded):
    prob, ix = rank_inputs(Q, Cn, rounded)
    u = 2.0 ** -53
    for indexed in (False, True):
        # without cand_idx every slot is present: the ABSENT fillers are ordinary (high) scores then
        ref = oracle().rank_exact(prob, ix if indexed else None)
        if rank_planted(Q, Cn) and indexed:
            assert ref["rank"][1] == 0.0 and ref["rank"][2] == 1.0 and ref["rank"][3] == 1.0 + 0.5 * (Cn - 1)
        start = np.array([1.25, 3.0, 0.0, 7.0, 2.0])
        start_exact = [Fraction(float(s)) for s in start]
        results = []
        for off in (0, 1):
            (dprob,) = carve([prob], off, np.float32("nan"))
            dix = carve([ix], off, np.int32(5))[0] if indexed else None
            for begin in (None, start):
                abuf, acc = guarded(5, begin)
                rbuf = torch.full((Q + 6,), SENT, dtype=torch.float32, device="cuda")
                rank = rbuf[3 + off:3 + off + Q]
                run_rank(dprob, dix, acc, rank)
                got, got_rank = acc.cpu().numpy(), rank.cpu().numpy()
                assert untouched(abuf, 5)
                rh = rbuf.cpu().numpy()
                assert np.all(rh[:3 + off] == SENT) and np.all(rh[3 + off + Q:] == SENT)
                assert np.array_equal(got_rank.astype(np.float64), ref["rank"])
                exact = [e + (s if begin is not None else 0) for e, s in zip(ref["exact"], start_exact)]
                err = abs(Fraction(float(got[0])) - exact[0])
                tol = Q * u * max(1.0, float(exact[0]))
                print("Q=%d C=%d rounded=%s indexed=%s off=%d start=%s  sum 1/rank %.17g  |err| = %.3e  bound %.3e"
                      % (Q, Cn, rounded, indexed, off, begin is not None, got[0], float(err), tol))
                note("rank Q=%d C=%d" % (Q, Cn), float(err))
                assert err <= tol, (got[0], float(exact[0]))
                assert [Fraction(float(v)) for v in got[1:]] == exact[1:], (got, exact)   # Hits@1 / @3 / @10 and the count
                if begin is None:
                    results.append((got, got_rank))
        assert np.array_equal(bits(results[0][0]), bits(results[1][0])) and np.array_equal(results[0][1], results[1][1])
