"""What tests/test_count_exact_gpu.py rests on, checked without a GPU: every planted case of tests/helpers_count_planted.py
reaches the plan fields its id names (zt_affinity_count_plan is host code), the plan's bounds hold over a sweep of shapes and
workspaces, and the host expectation agrees with a brute-force count in numpy."""
import ctypes as C

import numpy as np
import pytest

import helpers_count_planted as K


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import _capi
    return _capi


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_case_reaches_the_seam_its_id_names(case, capi):
    plan = case.plan(capi)
    for field, want in case.reach.items():
        assert plan[field] == want, "%s: plan[%s] = %d, the case is built for %d" % (case.id, field, plan[field], want)
    if case.id.startswith("slab32") or "slab32" in case.id:
        assert plan["n_slabs"] > 1 and plan["slab_rows"] == 32
    if "span" in case.id and "slab" not in case.id:
        assert plan["n_spans"] > 1
    if case.id == "width-H1028":
        assert plan["h_chunks"] > 1
    # the restated plan of the helper (the seam columns of the cases come from it) is the library's
    slab, n_slabs, span_cols, n_spans = K.plan_of(case.Q, case.C, case.H, case.ws_rows)
    assert (plan["slab_rows"], plan["n_slabs"], plan["span_cols"], plan["n_spans"]) == (slab, n_slabs, span_cols, n_spans)


def test_the_cases_cover_the_seams_the_kernel_has():
    ids = set(K.BY_ID)
    for Q in (1, 4, 5, 9):
        for C_ in (0, 1, 31, 32, 33, 127, 128, 129):
            assert "tiles-Q%d-C%d" % (Q, C_) in ids
    assert {"slab32-C33", "slab32-C65", "slab32-C100", "width-H20", "width-H1024", "width-H1028", "spans2-C1500"} <= ids
    by_skip = {0: 0, 1: 0, 2: 0, 4: 0}
    for case in K.CASES:
        d = case.data()
        if case.id.startswith("skip"):
            n = 0 if d["skip"] is None else d["skip"].shape[1]
            by_skip[n] += 1
            if n:
                slab, _, span_cols, _ = K.plan_of(case.Q, case.C, case.H, case.ws_rows)
                named = set(d["skip"].reshape(-1).tolist())
                assert {0, case.C - 1} <= named and any(c >= case.C for c in named)      # first, last, and one outside the call
                seam = slab if case.ws_rows else span_cols
                assert {seam - 1, seam} & named, case.id
    assert all(v >= 2 for v in by_skip.values())
    d = K.BY_ID["bits-C100"].data()
    assert d["mask"][:, [0, 31, 32, 63, 99]].all() and d["mask"][3].all() and not d["mask"][0].all()
    assert K.BY_ID["bits-slab32-with-skips"].data()["skip"].shape[1] == 2
    a, b = K.BY_ID["pieces-forward"], K.BY_ID["pieces-shuffled"]
    assert sorted(a.pieces) == sorted(b.pieces) and a.pieces != b.pieces and len(a.pieces) == 3 and a.idx_base > 0
    assert (a.incoming[0] + a.incoming[1] > 0).all()


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_host_expectation_agrees_with_brute_force(case):
    d = case.data()
    got, want = K.expected(case, d), K.brute_force(case, d)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case.id
    if case.id == "thr-all-equal":
        assert (got[0] == 0).all() and (got[1] == case.C).all()
    if case.id in ("thr-zero", "thr-negzero"):
        assert (got[1] >= case.C - 21).all() and (got[0] >= 20).all() and (got[0] + got[1] == case.C).all()
    if case.id == "thr-one":
        assert (got[0] == 0).all() and (got[1] == 10 + np.arange(case.Q)).all()
    if case.id == "thr-nan-and-half":
        assert got[0][0] == got[1][0] == got[0][3] == got[1][3] == 0 and got[0][2] == case.C and got[1][2] == 0
    if case.id.startswith("tiles") and case.C >= 31:
        assert (got[1] > 0).any()                                       # columns equal to the threshold exist


def test_pack_bits_is_the_format_of_absent_columns():
    import torch
    from zebra_amd.tgn import TGN, absent_columns
    rng = np.random.RandomState(5)
    for C_ in (1, 31, 32, 33, 100):
        mask = rng.random_sample((6, C_)) < 0.4
        mask[:, C_ - 1] = True                                          # (bit 31 of a word: the sign of an int32)
        bits = K.pack_bits(mask)
        assert np.array_equal(absent_columns(torch.from_numpy(bits.view(np.int32)), C_).numpy(), mask)
        assert np.array_equal(TGN._pack_absent(torch.from_numpy(mask)).numpy().view(np.uint32), bits)


SWEEP_Q = (0, 1, 4, 5, 200, 4097, 100000)
SWEEP_NC = (0, 1, 31, 32, 33, 511, 512, 513, 1023, 1024, 5000, 9228, 100000, 1000000, 3000000)
SWEEP_H = (4, 20, 200, 300, 1024, 1028, 4352)


def test_plan_bounds_over_a_sweep(capi):
    lib = capi.lib()
    for H in SWEEP_H:
        for Q in SWEEP_Q:
            least = int(lib.zt_affinity_count_workspace_bytes(C.c_int64(Q), C.c_int64(32), C.c_int32(H)))
            with pytest.raises(ValueError):
                capi.count_plan(Q, 1000, H, least - 1)
            for Nc in SWEEP_NC:
                rec = int(lib.zt_affinity_count_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H)))
                assert rec >= least
                for ws in sorted({least, least + 31 * H * 4, least + 32 * H * 4, rec, rec + 12345}):
                    p = capi.count_plan(Q, Nc, H, ws)
                    assert p["min_bytes"] == least and p["q_tiles"] == (Q + 3) // 4 and p["h_chunks"] == (H + 1023) // 1024
                    assert p["slab_rows"] >= 32 and p["slab_rows"] % 32 == 0
                    assert p["pc_offset"] % 256 == 0 and p["pc_offset"] >= 256 + Q * H * 4
                    assert p["pc_offset"] + p["slab_rows"] * H * 4 <= ws                    # the slab fits the workspace
                    assert p["slab_rows"] * H * 4 <= max(128 << 20, 32 * H * 4) and p["slab_rows"] <= 1 << 18
                    assert p["n_slabs"] >= 1 and p["n_slabs"] * p["slab_rows"] >= Nc
                    assert (p["n_slabs"] - 1) * p["slab_rows"] < max(Nc, 1)
                    assert p["span_cols"] % 128 == 0 and p["span_cols"] >= 128
                    assert p["n_spans"] >= 1 and p["n_spans"] * p["span_cols"] >= min(p["slab_rows"], Nc)
                    assert (p["n_spans"] - 1) * p["span_cols"] < max(min(p["slab_rows"], Nc), 1)
                    assert p["grid"] == p["q_tiles"] * p["n_spans"] and p["grid"] < 2 ** 31
                # the recommended size stops growing with the pool
                if Nc >= 1 << 18:
                    assert rec == int(lib.zt_affinity_count_workspace_bytes(C.c_int64(Q), C.c_int64(10 * Nc), C.c_int32(H)))


def test_plan_and_workspace_refusals(capi):
    lib = capi.lib()
    ws = lib.zt_affinity_count_workspace_bytes
    for Q, Nc, H in ((-1, 10, 20), (10, -1, 20), (10, 10, 0), (10, 10, 22), (10, 10, 4356), (10, 10, -4)):
        assert int(ws(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H))) == -1
    out = (C.c_int64 * len(capi.COUNT_PLAN_FIELDS))()
    big = C.c_int64(1 << 30)
    call = lib.zt_affinity_count_plan
    assert call(C.c_int64(5), C.c_int64(10), C.c_int32(20), big, None) == capi.ZT_ERR_ARG
    assert call(C.c_int64(-1), C.c_int64(10), C.c_int32(20), big, out) == capi.ZT_ERR_ARG
    assert call(C.c_int64(5), C.c_int64(-1), C.c_int32(20), big, out) == capi.ZT_ERR_ARG
    assert call(C.c_int64(5), C.c_int64(10), C.c_int32(20), C.c_int64(-5), out) == capi.ZT_ERR_ARG
    for H in (0, 2, 22, 4356):
        assert call(C.c_int64(5), C.c_int64(10), C.c_int32(H), big, out) == capi.ZT_ERR_UNSUPPORTED
    assert call(C.c_int64(5), C.c_int64(10), C.c_int32(20), big, out) == capi.ZT_OK
    assert len(capi.COUNT_PLAN_FIELDS) == 9 and capi.COUNT_MAX_SKIP == K.MAX_SKIP
