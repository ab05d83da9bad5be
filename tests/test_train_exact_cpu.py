"""The exact cases of the pair scorer's and the node decoder's training kernels without a GPU (tests/helpers_train_exact.py):
the plan entries (zt_affinity_train_plan, zt_node_decoder_plan) are the restatement written from the kernels' comments; every
case crosses the seam its id names, by both; every seam of the issue's lists has a case; every exact case's sums stay below
2^24, intermediates included, with torch's float32 on the CPU equal to float64 in every bit; every seam row feeds every
gradient a non-zero term; the margin seeds are re-derived; torch's float32 composition stays within the derived bound of the
random family; the six defects the comparison is there for change the bits of the float64 restatement -- and the old
max-norm tolerances accept the first of them at (4096, 300), which is why these files exist."""
import numpy as np
import pytest

import helpers_decoder as hd
import helpers_train_exact as X

SC, DC, GK = X.SC, X.DC, X.GK


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import _capi
    _capi.lib()
    return _capi


def entry_plan(capi, case):
    return capi.score_train_plan(case.n, case.H) if case.kind == "score" else capi.decoder_plan(case.n, case.H, True)


def test_the_tile_constants_are_read_from_the_sources():
    for name in ("SCORE_MAX_H", "SCORE_WAVES", "SCORE_THREADS", "ST_MAX_SPLIT", "GK"):
        assert isinstance(SC.get(name), int) and SC[name] > 0, name
    for name in ("DEC_MIN_H", "DEC_MAX_H", "DEC_KC", "DEC_MAX_SPLIT", "GK", "FIN_THREADS", "FIN_WAVES"):
        assert isinstance(DC.get(name), int) and DC[name] > 0, name
    assert SC["GK"] == DC["GK"] == 64 and SC["SCORE_THREADS"] == 64 * SC["SCORE_WAVES"]
    assert X.FIN_OUTS == 901 and X.cdiv(X.FIN_OUTS, 64) == 15 and X.FIN_OUTS - 14 * 64 == 5     # the last sum workgroup: five sums


# ---- the plan entries ------------------------------------------------------------------------------------------------------
def test_score_plan_entry_is_the_restatement_on_a_grid(capi):
    """every field, every accepted width's class and every batch size up to 20 steps, then the large ones"""
    widths = sorted(set([4, 20, 60, 64, 68, 256, 260, 320, 324, 388, 512, 516, 764, 768] +
                        [X._first_reaching(X.score_max_split, m, X.score_widths()) for m in X.split_values(X.score_max_split, X.score_widths())]))
    for H in widths:
        for B in list(range(1, 20 * GK // 2 + 2)) + [1000, 4095, 4096, 4097, 65536]:
            got, want = capi.score_train_plan(B, H), X.score_plan(B, H)
            assert all(got[k] == want[k] for k in got), (B, H, got, want)
    for H in X.score_widths():
        assert capi.score_train_plan(4096, H)["max_split"] == X.score_max_split(H)
    for H in (0, 2, 50, 772):
        with pytest.raises(ValueError):
            capi.score_train_plan(17, H)
    with pytest.raises(ValueError):
        capi.score_train_plan(-1, 20)
    assert capi.score_train_plan(0, 20)["split"] == 1


def test_decoder_plan_entry_is_the_restatement_on_a_grid(capi):
    for H in sorted(set([4, 20, 2048, 2052, 2304, 2308, 4352] + [X._first_reaching(X.dec_max_split, m, X.dec_widths())
                                                                   for m in X.split_values(X.dec_max_split, X.dec_widths())])):
        for N in list(range(1, 20 * GK + 2)) + [4096, 4097, 65536]:
            got, want = capi.decoder_plan(N, H, True), X.dec_plan(N, H)
            assert (got["split"], got["k_per"]) == (want["split"], want["k_per"]), (N, H)
            assert (want["split"], want["k_per"]) == hd.expected_split(N, H)


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_case_crosses_the_seam_its_id_names(capi, case):
    """by the restatement (crossed reads nothing else) and by the plan entry, which must be the restatement's"""
    got, want = entry_plan(capi, case), case.plan()
    assert all(got[k] == want[k] for k in got if k in want), (got, want)
    assert got["split"] == want["split"] and got["k_per"] == want["k_per"]
    assert X.crossed(case), case.id
    parts = X.parts_of(case.K, want)
    assert parts[0][0] == 0 and parts[-1][1] == case.K and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert all(end > beg for beg, end in parts) and all((end - beg) % GK == 0 for beg, end in parts[:-1])
    assert str(case.n) in case.id and "H%d" % case.H in case.id


def _family(kind, fam):
    return [c for c in X.CASES if c.kind == kind and c.id.split("-")[1] == fam]


def test_every_seam_of_the_lists_has_a_case():
    ids = set(X.BY_ID)
    n = lambda kind, fam: sorted(c.n for c in _family(kind, fam))
    h = lambda kind, fam: sorted(c.H for c in _family(kind, fam))
    # scoring_train.hip
    assert n("score", "tile16") == [1, 15, 16, 17, 33]
    assert h("score", "hmin") == [4] and sorted(H % 16 for H in h("score", "hmod16")) == [0, 4, 8, 12]
    assert h("score", "colgroup") == [60, 64, 68] and h("score", "dxitems") == [320, 324]
    assert h("score", "ntile") == [256, 260, 512, 516, SC["SCORE_MAX_H"]]
    values = X.split_values(X.score_max_split, X.score_widths())
    assert values[0] == SC["ST_MAX_SPLIT"] and values[-1] == 1 and len(values) >= 3, values
    for m in values:
        kinds = sorted(c.id.split("-")[2] for c in X.SCORE_CASES if c.id.split("-")[1] == "maxsplit%d" % m)
        assert kinds == (["capped"] if m == 1 else ["below", "reached"]), (m, kinds)
    assert {"score-steps3-B96-H20", "score-steps4-B97-H20", "score-lowered-raggedpart-B529-H20", "score-rowB-stepedge-B64-H20",
            "score-rowB-partedge-B128-H20", "score-rowB-straddle-B100-H20"} <= ids
    assert h("score", "workload") == [40, 300, SC["SCORE_MAX_H"]] and n("score", "workload") == [4096] * 3
    assert n("score", "finrows") == [63, 64, 65, 129] and n("score", "finthreads") == [511, 512, 513]
    # decoder.hip
    assert n("dec", "tile16") == [1, 15, 16, 17, 63, 64, 65]
    assert h("dec", "hmin") == [4] and sorted(H % 16 for H in h("dec", "hmod16")) == [0, 4, 8, 12]
    assert h("dec", "kchunk") == [252, 256, 260, 512, 516] and h("dec", "widest") == [DC["DEC_MAX_H"]]
    values = X.split_values(X.dec_max_split, X.dec_widths())
    assert values[0] == DC["DEC_MAX_SPLIT"] and len(values) >= 3, values
    seen = []
    for m in values:
        cs = [c for c in X.DEC_CASES if c.id.split("-")[1] == "maxsplit%d" % m]
        assert sorted(c.id.split("-")[2] for c in cs) == ["below", "reached"], m
        seen.append(cs[0].H)
    assert seen[:3] == [2048, 2052, 2308] and X.dec_max_split(DC["DEC_MAX_H"]) == values[-1]
    for s in range(1, DC["DEC_MAX_SPLIT"] + 1):
        assert "dec-split%d-N%d-H12" % (s, 2 * GK * s) in ids and "dec-split%d-below-N%d-H12" % (s, 2 * GK * s - GK) in ids
    assert 513 <= X.BY_ID["dec-lowered3-N545-H20"].n <= 576 and 1025 <= X.BY_ID["dec-lowered6-N1057-H20"].n <= 1088
    assert {"dec-lastpart-step-and-row-N4097-H20", "dec-largest-N4097-H4352", "dec-finrows-N129-H20"} <= ids
    assert sorted((c.n, c.H) for c in X.DEC_CASES if c.p == 0.5) == [(17, 20), (200, 300), (1025, 516)]
    assert all(c.p in (0.0, 0.5) for c in X.CASES)
    # the calls with outputs left out: one product and partial products, both kernels; dropout among them
    assert {c.plan()["split"] > 1 for c in X.OPTIONAL_CASES if c.kind == "score"} == {False, True}
    assert {c.plan()["split"] > 1 for c in X.OPTIONAL_CASES if c.kind == "dec"} == {False, True}
    assert any(c.p for c in X.OPTIONAL_CASES)
    assert max((c.n, c.H) for c in X.SCORE_CASES) == (4096, 768) and max((c.n, c.H) for c in X.DEC_CASES) == (4097, 4352)


# ---- the exact cases -------------------------------------------------------------------------------------------------------
def _values(a):
    return set(np.unique(a).tolist())


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_exact_case_cannot_round(case):
    """the inputs are what the helper says, the composition on absolute values stays below 2^24 in every output and every
    intermediate, the float64 composition is integral, and torch's float32 on the CPU has its bits"""
    d = X.exact_reference(case.id)
    assert d["worst"] < 2.0 ** 24, d["worst"]
    H = case.H
    if case.kind == "score":
        w1, b1, w2, b2 = d["wts"]
        unit, n = 2.0 ** d["e"], min(8, H)
        assert _values(d["emb"]) <= {-1.0, 0.0, 1.0} and _values(w1) <= {-1.0, 0.0, 1.0} and _values(b1) <= {-1.0, 0.0, 1.0}
        assert bool(((w1[:, :H] != 0).sum(1) == n).all()) and bool(((w1[:, H:] != 0).sum(1) == n).all())
        assert _values(w2 * unit) <= {-2.0, -1.0, 1.0, 2.0} and float(b2[0] * unit) == int(b2[0] * unit) and abs(b2[0] * unit) <= 3
        assert _values(d["prob"]) <= {0.25, 0.5, 0.75} and _values(d["dprob"]) <= {-32.0, -16.0, 16.0, 32.0}
        assert 0 <= d["e"] <= 10 and float(np.abs(d["s64"]).max()) <= 8.0
        assert d["e"] == 0 or float(np.abs(d["s64"]).max()) > 4.0                        # the smallest such power
        ds32 = (d["dprob"] * d["prob"]) * (np.float32(1) - d["prob"])                     # the kernel's order, in float32
        assert _values(np.abs(ds32)) <= {3.0, 4.0, 6.0, 8.0}
        assert np.array_equal(d["z64"], np.round(d["z64"])) and np.array_equal(d["s64"] * unit, np.round(d["s64"] * unit))
        for k, (name, o) in enumerate(zip(X.SCORE_OUT, d["out64"])):
            u = 1.0 if k in (3, 4) else unit
            assert np.array_equal(o * u, np.round(o * u)), name
            assert np.array_equal(d["out"][k].astype(np.float64), o), name               # the one rounding rounds nothing
        hid32, s32 = X.score_forward32(d["emb"], d["wts"])
        assert X.np_bits_equal(hid32, d["hid"]) and np.array_equal(s32.astype(np.float64), d["s64"])
        for name, a, b in zip(X.SCORE_OUT, X.score_backward32(d["emb"], d["wts"], d["prob"], d["hid"], d["dprob"]), d["out"]):
            assert X.np_bits_equal(a, b), "float32 on the CPU differs from float64 in %s" % name
        z = d["z64"]
    else:
        P = d["P"]
        assert _values(d["x"]) <= {-1.0, 0.0, 1.0} and _values(d["dz"]) <= {-2.0, -1.0, 1.0, 2.0}
        for k in ("fc_1.weight", "fc_1.bias", "fc_2.weight", "fc_2.bias"):
            assert _values(P[k]) <= {-1.0, 0.0, 1.0}, k
        assert bool(((P["fc_1.weight"] != 0).sum(1) == min(8, H)).all()) and bool(((P["fc_2.weight"] != 0).sum(1) == 8).all()) and bool(((P["fc_2.weight"] != 0).sum(0) == 1).all())
        assert _values(P["fc_3.weight"]) <= {-2.0, -1.0, 1.0, 2.0} and float(P["fc_3.bias"][0]) == int(P["fc_3.bias"][0])
        if case.p:
            assert _values(d["m1"]) == {0.0, 2.0} and _values(d["m2"]) <= {0.0, 2.0}
            assert 0.3 < float((d["m1"] == 0).mean()) < 0.7
        else:
            assert d["m1"] is None and d["m2"] is None
        f = d["fwd64"]
        for k in ("pre1", "h1", "pre2", "h2", "z"):
            assert np.array_equal(f[k], np.round(f[k])), k
        for k, (name, o) in enumerate(zip(X.DEC_OUT, d["out64"])):
            assert np.array_equal(o, np.round(o)), name
            assert np.array_equal(d["out"][k].astype(np.float64), o), name
        # helpers_decoder.backward64, which the reference's fixture pins, gives the same sums
        g = hd.backward64(P, d["x"], f, d["dz"], d["m1"], d["m2"])
        for name, o in zip(X.DEC_OUT, d["out64"]):
            assert np.array_equal(g[name].reshape(o.shape), o), name
        h1, h2, logit = X.dec_forward32(P, d["x"], d["m1"], d["m2"])
        assert X.np_bits_equal(h1, d["h1"]) and X.np_bits_equal(h2, d["h2"]) and X.np_bits_equal(logit, d["logit"])
        for name, a, b in zip(X.DEC_OUT, X.dec_backward32(P, d["x"], d["h1"], d["h2"], d["dz"], d["m1"], d["m2"]), d["out"]):
            assert X.np_bits_equal(a, b), "float32 on the CPU differs from float64 in %s" % name
        z = f["pre1"]
        # the last of the fifteen sum workgroups carries d_fc3_w[6..9] and d_fc3_b: non-zero here, so that a lost sum shows
        if case.id.startswith("dec-finrows"):
            assert np.all(d["out64"][5][0, 6:] != 0) and d["out64"][6][0] != 0
    assert all(np.any(o != 0) for o in d["out64"]), "an output that is all zero cannot show a lost sum"
    zero, neg, pos = float((z == 0).mean()), float((z < 0).mean()), float((z > 0).mean())
    print("%s: sum of |terms| at most %.3g; z = 0 at %.1f %%, z < 0 at %.1f %% of %d units" % (case.id, d["worst"], 100 * zero, 100 * neg, z.size))
    assert zero >= 0.02 and neg > 0 and pos > 0                                          # z > 0 is pinned at z = 0 by every case


@pytest.mark.parametrize("case", X.CASES, ids=repr)
def test_seam_rows_count(case):
    """every seam row of the K dimension has a live unit and non-zero inputs: its own term is non-zero in at least one element
    of every gradient it feeds"""
    d = X.exact_reference(case.id)
    rows = case.seam_rows()
    parts = X.parts_of(case.K, case.plan())
    assert all(end - 1 in rows and beg in rows for beg, end in parts) and case.K - 1 in rows
    if case.kind == "score":
        B = case.n
        assert {B - 1, B, 2 * B - 1} <= set(rows)
        assert X.score_seam_rows_missing(case, d, d["hid"]) == []
    else:
        assert X.dec_seam_rows_missing(case, d, d["h1"], d["h2"]) == []


# ---- the random family -----------------------------------------------------------------------------------------------------
def test_the_random_family_is_every_case_the_margin_can_hold():
    assert [c.id for c in X.RANDOM_CASES] == [c.id for c in X.CASES if c.units() <= X.MARGIN_MAX_UNITS]
    assert any(c.H == SC["SCORE_MAX_H"] for c in X.RANDOM_CASES) and any(c.H == DC["DEC_MAX_H"] for c in X.RANDOM_CASES)
    assert any(c.plan()["split"] == 8 for c in X.RANDOM_CASES if c.kind == "score") and any(c.p for c in X.RANDOM_CASES)
    assert set(X.MARGIN_SEEDS) <= set(c.id for c in X.RANDOM_CASES) and 0 not in X.MARGIN_SEEDS.values()


@pytest.mark.parametrize("case", X.RANDOM_CASES, ids=repr)
def test_margin_seed_is_rederived_and_torch_stays_within_the_bound(case):
    """the committed seed is the first that meets the margin condition; there torch's float32 composition on the CPU stays within
    L 2^-24 A + ulp elementwise -- a count of L that float32 itself cannot meet would be wrong"""
    assert X.derive_margin_seed(case) == X.margin_seed(case)
    d = X.random_reference(case.id)
    if case.kind == "score":
        hid32, s32 = X.score_forward32(d["emb"], d["wts"])
        fwd = dict(hid=hid32)
        p32 = 1.0 / (1.0 + np.exp(-s32.astype(np.float32)))
        assert float((np.abs(p32.astype(np.float64) - hd.sigmoid64(d["s64"])) / hd.prob_bound(d["s64"])).max()) <= 1.0
        out = X.score_backward32(d["emb"], d["wts"], d["prob"], d["hid"], d["dprob"])
        names = X.SCORE_OUT
    else:
        fwd = dict(zip(("h1", "h2", "logit"), X.dec_forward32(d["P"], d["x"], d["m1"], d["m2"])))
        out = X.dec_backward32(d["P"], d["x"], d["h1"], d["h2"], d["dz"], d["m1"], d["m2"])
        names = X.DEC_OUT
    shares = {k: X.share_of_bound(v, d["fwd64"][k], d["fwd_bound"][k]) for k, v in fwd.items()}
    shares.update({k: X.share_of_bound(g, r, b) for k, g, r, b in zip(names, out, d["out64"], d["bound"])})
    print("%s seed %d: torch float32 uses %s of the bound" % (case.id, X.margin_seed(case), ", ".join("%s %.3f" % kv for kv in shares.items())))
    assert max(shares.values()) <= 1.0, shares


# ---- the comparison rejects what it is there for ---------------------------------------------------------------------------
MUT_CASES = [c for c in X.CASES if c.K <= 1100 and c.H <= 1000] + [X.BY_ID["score-workload-B4096-H300"], X.BY_ID["dec-lastpart-step-and-row-N4097-H20"]]


def _mutated(case, mut):
    d = X.exact_reference(case.id)
    if case.kind == "score":
        return d, X.score_backward64(d["emb"], d["wts"], d["prob"], d["hid"], d["dprob"], case.plan(), mut=mut)
    return d, X.dec_backward64(d["P"], d["x"], d["h1"], d["h2"], d["dz"], d["m1"], d["m2"], case.plan(), mut=mut)


# defect -> (the outputs it must change, the families whose cases name the seam it sits on)
WHERE = {"row_out": ((1,), ("maxsplit", "split", "steps", "lowered", "rowB", "lastpart", "workload")),
         "part_twice": ((1,), ("maxsplit", "split", "steps", "lowered", "rowB", "lastpart", "workload")),
         "swap_dst_neg": ((1,), ("rowB", "tile16", "workload")),
         "mask_ge": ((0, 1, 2), ("tile16", "hmin", "hmod16")),
         "kstep_out": ((0,), ("hmin", "hmod16", "dxitems", "kchunk", "ntile")),
         "no_scale": ((0, 1, 2), ("dropout",))}


@pytest.mark.parametrize("mut", X.MUTATIONS)
def test_a_wrong_result_changes_the_bits(mut):
    """the defect applied to the float64 restatement changes the bits of EVERY case it applies to (of those small enough to
    recompute here), the cases that name its seam among them"""
    outputs, families = WHERE[mut]
    hit = set()
    for case in MUT_CASES:
        if not X.mutation_applies(mut, case):
            continue
        d, got = _mutated(case, mut)
        for k in outputs:
            assert not X.np_bits_equal(X.f32(got[k]), d["out"][k]), "%s: %s leaves %s as it was" % (case.id, mut, k)
        fam = case.id.split("-")[1]
        hit.add(next((stem for stem in ("maxsplit", "split", "steps", "lowered") if fam.startswith(stem)), fam))
    assert set(families) <= hit, (mut, sorted(hit))


def test_the_old_tolerances_accept_a_dropped_row_at_4096_300():
    """tests/test_scoring_train_gpu.py's own inputs at (4096, 300) in float64: the last pair row, the ragged end of the last K-part, left out of
    d fc1.weight stays inside 1e-5 + 1e-4 max|ref|, and an all-zero d_emb inside 1e-5.  The exact case of the same shape
    rejects the same defect (test_a_wrong_result_changes_the_bits)."""
    case = X.BY_ID["score-workload-B4096-H300"]
    emb, dprob, wts = X.score_random_at(case, 0)
    plan = case.plan()
    assert plan["split"] > 1
    fwd = X.score_forward64(emb, wts)
    prob = hd.sigmoid64(fwd["s"])
    ref = X.score_backward64(emb, wts, prob, fwd["hid"], dprob, plan)
    bad = X.score_backward64(emb, wts, prob, fwd["hid"], dprob, plan, mut="row_out")
    err, mx = float(np.abs(bad[1] - ref[1]).max()), float(np.abs(ref[1]).max())
    print("one pair row left out of d fc1.weight: %.3g against an allowed %.3g; max|d_emb| %.3g against 1e-5"
          % (err, X.OLD_ABS + X.OLD_REL * mx, float(np.abs(ref[0]).max())))
    assert 0 < err <= X.OLD_ABS + X.OLD_REL * mx
    assert 0 < float(np.abs(ref[0]).max()) <= X.OLD_ABS
