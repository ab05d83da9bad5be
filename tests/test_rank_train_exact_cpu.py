"""The exact cases of the ranking step's scorer without a GPU (tests/helpers_rank_exact.py): every case lies on the seam of
csrc/rank_train.hip's tiling its id names -- the tile constants are read from the sources, so a changed constant fails here
until the list is redrawn --, every planted index has the pair counts it was given and a transpose rank_transpose gets right,
every exact case's sums stay below 2^24 with float32 on the CPU equal to float64 in every bit and the ReLU's z = 0 well
populated, and every random-input case has a seed that meets the margin condition at which torch's float32 composition on the
CPU stays within HALF of the derived bound."""
import numpy as np
import pytest
import torch

import helpers_rank_exact as X
from helpers_rank_train import NEG_INF, check_transpose

S = X.seams()
ALL = X.CASES + X.ABI_CASES[2:]


def test_the_tile_constants_are_read_from_the_sources():
    for name in ("WAVE", "RK_TQ", "RK_GROUP", "RK_NC", "RK_TC", "RK_HC", "RT_SLAB", "RT_CROWS", "RT_CCOLS", "RT_CU",
                 "RANK_MIN_H", "RANK_MAX_H"):
        assert isinstance(S.get(name), int) and S[name] > 0, name
    assert S["RK_TC"] == S["WAVE"] // S["RK_GROUP"] * S["RK_NC"] and S["RT_SLAB"] == 4 * S["RK_GROUP"]
    assert S["RT_CCOLS"] == 4 * S["WAVE"]


def _edges(t, k):
    """both sides of the first k multiples of tile t"""
    return sorted(v for m in range(1, k + 1) for v in (m * t - 1, m * t, m * t + 1))


# family -> (the quantity its cases vary, the values the family must take)
FAMILIES = {
    "cu": (lambda c: c.Q, [S["RT_CU"] - 1, S["RT_CU"], S["RT_CU"] + 1, 2 * S["RT_CU"], 2 * S["RT_CU"] + 1]),
    "crows": (lambda c: c.Nc, [1, S["RT_CROWS"] - 1, S["RT_CROWS"], S["RT_CROWS"] + 1, 2 * S["RT_CROWS"], 2 * S["RT_CROWS"] + 1]),
    "ccols": (lambda c: c.H, [m * S["RT_CCOLS"] + d for m in (1, 2) for d in (-4, 0, 4)]),
    "slab": (lambda c: c.H, [m * S["RT_SLAB"] + d for m in (1, 2) for d in (-4, 0, 4)]),
    "hc": (lambda c: c.H, [S["RK_HC"] - 4, S["RK_HC"], S["RK_HC"] + 4, 2 * S["RK_HC"], 2 * S["RK_HC"] + 4]),
    "widest": (lambda c: c.H, [S["RANK_MAX_H"]]),
    "narrow": (lambda c: c.H, [S["RANK_MIN_H"], 2 * S["RANK_MIN_H"]]),
    "nc": (lambda c: c.C, [1] + _edges(S["RK_NC"], 1) + _edges(S["RK_TC"], 2) + [3 * S["RK_TC"] + 1]),
    "tq": (lambda c: c.Q, [1, S["RK_TQ"] - 1, S["RK_TQ"], S["RK_TQ"] + 1, 2 * S["RK_TQ"], 2 * S["RK_TQ"] + 1, 3 * S["RK_TQ"] + 1]),
}
LADDER = [0, 1, S["RT_CU"] - 1, S["RT_CU"], S["RT_CU"] + 1, 2 * S["RT_CU"] - 1, 2 * S["RT_CU"], 2 * S["RT_CU"] + 1, 3 * S["RT_CU"],
          3 * S["RT_CU"] + 1]


def _family(case):
    return case.id.split("-")[0]


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_case_lies_where_its_id_says(case):
    """from Q, C, H, Nc and the pair counts alone"""
    fam, parts = _family(case), case.id.split("-")
    assert not ("indexed" in parts and not case.indexed) and not ("shared" in parts and case.indexed), case.id
    ix = case.index()
    if fam in FAMILIES and case.id != "cu-ladder":
        value, values = FAMILIES[fam]
        assert value(case) in values, case.id
        named = [p for p in parts if p[0] in "QCHN" and p.lstrip("QCHNc").isdigit()]
        assert named and int(named[0].lstrip("QCHNc")) == value(case), case.id            # the id names the value it takes
    if case.id == "cu-ladder":
        assert sorted(case.n_r) == sorted(LADDER) and case.Nc == len(LADDER)
        flat = ix.reshape(-1)
        r = int(flat[0])
        assert r >= 0 and int(flat[-1]) == r                                              # the first and the last pair id
        assert any(int((ix[q] == rr).sum()) >= 2 for q in range(case.Q) for rr in range(case.Nc))      # twice by one query
    if fam == "cu" and not case.indexed:
        assert case.pair_counts() == [case.Q] * case.Nc
    if "lastunnamed" in parts:
        assert case.n_r[-1] == 0 and min(case.n_r[:-1]) > 0 and case.Nc % S["RT_CROWS"] == 1       # a workgroup of its own
    if "lastlive" in parts:
        TQ = S["RK_TQ"]
        live = (ix >= 0).any(dim=1)
        assert case.Q % TQ == 0 and not bool(live[case.Q - TQ:case.Q - 1].any()) and bool(live[case.Q - 1])
    if fam == "widest" and "small" not in parts:
        assert (case.Q, case.C) == (9, 33) and case.indexed
    if fam == "tq" and case.Q == 3 * S["RK_TQ"] + 1:
        assert -(-case.Q // S["RK_TQ"]) == 4                                              # four partial rows of d_fc2_w
    if case.id == "absent-all":
        assert case.indexed and sum(case.n_r) == 0 and bool((ix == -1).all())
    if case.id == "absent-query":
        assert sum(int(bool((ix[q] == -1).all())) for q in range(case.Q)) == 1
    if case.id == "absent-column":
        assert sum(int(bool((ix[:, c] == -1).all())) for c in range(case.C)) == 1
    if fam == "dlnan":
        assert case.dl_nan and 0 < int((ix == -1).sum()) < ix.numel()
    if fam == "workload":
        assert (case.Q, case.C, case.H) == (200, 101, 300)
    # one parameter at a time: the others stay inside their first tile, the varied one apart
    if fam in ("cu", "crows", "nc", "tq", "absent"):
        assert case.H <= S["RT_SLAB"]
    if fam in ("ccols", "slab", "hc", "narrow"):
        assert case.Q <= 2 * S["RK_TQ"] and case.C <= S["RK_TC"] and case.Nc <= 2 * S["RT_CROWS"]


def test_every_family_takes_every_value_of_its_seam():
    for fam, (value, values) in FAMILIES.items():
        got = sorted(value(c) for c in X.CASES if _family(c) == fam and c.id != "cu-ladder" and "small" not in c.id
                     and "lastunnamed" not in c.id and "lastlive" not in c.id)
        want = sorted(values * 2 if fam in ("crows", "narrow") else values)               # (both forms of the index)
        assert got == want, (fam, got, want)
    for fam in ("nc", "tq", "ccols", "slab", "hc"):                                       # half with an index, half without
        n = [c.indexed for c in X.CASES if _family(c) == fam and "lastlive" not in c.id]
        assert abs(sum(n) - (len(n) - sum(n))) <= 1, fam
    assert {"cu-ladder", "absent-all", "absent-query", "absent-column", "dlnan-holes", "workload-indexed", "workload-shared",
            "crows-indexed-Nc%d-lastunnamed" % (S["RT_CROWS"] + 1), "tq-indexed-Q%d-lastlive" % (2 * S["RK_TQ"]),
            "widest-shared-H%d-small" % S["RANK_MAX_H"]} <= set(X.BY_ID)
    a, b, c = X.ABI_CASES
    assert a.indexed and not b.indexed and c.indexed
    assert (c.Q, c.C, c.H, c.Nc) == (5, 33, 68, 7) and all((c.Q * c.C) % t for t in (2, 4, S["RT_CU"], S["RK_TC"]))


@pytest.mark.parametrize("case", [c for c in ALL if c.indexed], ids=repr)
def test_planted_index_has_its_counts_and_its_transpose(case):
    from zebra_amd.modules import rank_transpose
    ix = case.index()
    assert ix.dtype == torch.int32 and tuple(ix.shape) == (case.Q, case.C)
    flat = ix.reshape(-1).numpy()
    assert np.bincount(flat[flat >= 0], minlength=case.Nc).tolist() == list(case.n_r)
    assert int((flat == -1).sum()) == flat.size - sum(case.n_r) and flat.min() >= -1 and flat.max() < case.Nc
    assert torch.equal(ix, case.index())                                                  # seeded: the same index again
    row_ptr, pairs = rank_transpose(ix, case.Nc)
    check_transpose(ix, case.Nc, row_ptr, pairs)
    assert np.diff(row_ptr.numpy()).tolist() == list(case.n_r)


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_exact_case_cannot_round(case):
    """the four conditions of an exact case, for EVERY case"""
    emb_q, emb_c, ix, dl, wts = case.exact()
    for t in (emb_q, emb_c):
        assert set(np.unique(t.numpy())) <= {-1.0, 0.0, 1.0}
    w1, b1, w2, b2 = wts
    n = min(8, case.H)
    assert set(np.unique(w1)) <= {-1.0, 0.0, 1.0} and set(np.unique(b1)) <= {-1.0, 0.0, 1.0}
    assert bool(((w1[:, :case.H] != 0).sum(1) == n).all()) and bool(((w1[:, case.H:] != 0).sum(1) == n).all())
    assert set(np.unique(w2)) <= {-2.0, -1.0, 1.0, 2.0} and float(b2[0]) == int(b2[0])
    assert set(np.unique(dl.numpy())) <= {-2.0, -1.0, 1.0, 2.0}
    ref, A = X.exact_reference(case.id)
    worst = max(float(torch.where(torch.isfinite(a), a, torch.zeros_like(a)).max()) if a.numel() else 0.0 for a in A)
    assert worst < 2.0 ** 24, worst
    r64 = X.compose64(emb_q, emb_c, ix, dl, wts)
    for name, a, b in zip(X.OUTPUTS, r64, ref):
        fin = torch.isfinite(a)
        assert torch.equal(torch.where(fin, a, torch.zeros_like(a)), torch.where(fin, a, torch.zeros_like(a)).round()), name
        assert torch.equal(b.double(), a), name                                           # the one rounding rounds nothing
    for name, a, b in zip(X.OUTPUTS, X.compose32(emb_q, emb_c, ix, dl, wts), ref):
        assert X.bits_equal(a, b), "float32 on the CPU differs from float64 in %s" % name
    z = X.live_z(emb_q, emb_c, ix, wts)
    if case.id == "absent-all":
        assert z.numel() == 0 and bool((ref[0] == NEG_INF).all()) and all(float(g.abs().max()) == 0.0 for g in ref[1:])
        return
    zero, neg = float((z == 0).double().mean()), float((z < 0).double().mean())
    print("%s: sum of |terms| at most %.3g; z = 0 at %.1f %%, z < 0 at %.1f %% of %d units" % (case.id, worst, 100 * zero, 100 * neg,
                                                                                                 z.numel()))
    assert zero >= 0.02 and neg > 0 and float((z > 0).double().mean()) > 0


def test_the_random_family_is_every_case_the_margin_can_hold():
    left_out = sorted(c.id for c in X.CASES if c not in X.RANDOM_CASES)
    assert left_out == sorted(["absent-all", "widest-indexed-H%d" % S["RANK_MAX_H"], "workload-indexed", "workload-shared"])
    assert any(c.H == S["RANK_MAX_H"] for c in X.RANDOM_CASES)


@pytest.mark.parametrize("case", X.RANDOM_CASES, ids=repr)
def test_random_case_meets_the_margin_and_torch_fits_half_the_bound(case):
    """the first seed of the case that meets the margin condition exists (margin_seed fails otherwise); there torch's float32
    composition on the CPU stays within HALF of L 2^-24 A + ulp elementwise -- a derivation of L that float32 itself cannot
    meet would be wrong -- and the parameter gradients within half of 1e-5 + 1e-4 max|ref|"""
    args, ref, bound = X.random_reference(case.id)
    z = X.live_z(args[0], args[1], args[2], args[4])
    assert X.margin_ok(z) and z.numel() == case.live_units()
    got = X.compose32(*args)
    shares = [X.share_of_bound(g, r, b) for g, r, b in zip(got[:3], ref[:3], bound)]
    print("%s seed %d: torch float32 uses %s of the bound" % (case.id, X.margin_seed(case), ["%.3f" % s for s in shares]))
    assert max(shares) <= 0.5, shares
    for name, g, r in zip(X.OUTPUTS[3:], got[3:], ref[3:]):
        assert float((g.double() - r).abs().max()) <= 0.5 * (1e-5 + 1e-4 * float(r.abs().max())), name
