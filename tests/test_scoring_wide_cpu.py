"""The eval link scorer's widths and kernel plan without a GPU (csrc/scoring.hip: zt::affinity_kernel_plan through the
zt_test_affinity_plan hook, zt_affinity's checks, ZT_CHOICE_SCORE): the eval scorer takes exactly the hidden widths the
training scorer takes, widths 200 / 300 keep the specialised kernels with the launch parameters they always had, every other
width takes the two generic kernels, and a pinned form that cannot take the width falls back to the library's pick."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED, LATENCY, TILED, GEN_LATENCY, GEN_TILED = 0, 1, 2, 3, 4
GEN_TILED_MIN = 512            # the committed switch between the two generic forms


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def plan(capi, B, H, choice=0):
    """dict(form, KC, ET, gx, gy, threads, lds) of affinity_kernel_plan(B, H, choice)"""
    out = (C.c_int64 * 7)()
    assert capi.hooks_lib().zt_test_affinity_plan(C.c_int64(B), C.c_int32(H), C.c_int32(choice), out) == capi.ZT_OK
    return dict(zip(("form", "KC", "ET", "gx", "gy", "threads", "lds"), [int(v) for v in out]))


def round_up16(x):
    return (x + 15) // 16 * 16


def test_eval_scorer_takes_the_training_scorers_widths(capi):
    lib = capi.lib()
    ws, ws_train = lib.zt_affinity_workspace_bytes, lib.zt_affinity_train_workspace_bytes
    for H in (4, 20, 196, 200, 300, 344, 512, 516, 768):
        assert ws(C.c_int64(200), C.c_int32(H)) > 0, H
    for H in (0, -4, 2, 50, 342, 772, 1024):
        assert ws(C.c_int64(200), C.c_int32(H)) == -1, H
    for H in range(0, 800):
        assert (ws(C.c_int64(200), C.c_int32(H)) > 0) == (ws_train(C.c_int64(16), C.c_int32(H)) > 0), H
    for H in (200, 516, 768):
        assert ws(C.c_int64(4096), C.c_int32(H)) > ws(C.c_int64(200), C.c_int32(H)), H
        # the packed W_a / W_b, bias and fc2's weight, the tile counters and the N-tiles' partial scores all fit
        Hp, tiles = round_up16(H), (4096 + 15) // 16
        assert ws(C.c_int64(4096), C.c_int32(H)) >= (2 * Hp * Hp + 2 * Hp) * 4 + tiles * 4 + (Hp // 16) * 2 * tiles * 16 * 4, H


def test_checks_come_before_any_device_call(capi):
    """A refused width: ZT_ERR_UNSUPPORTED with a text that names H and the bound; B = 0: ZT_OK, nothing touched; the new
    selector takes its values.  All before the first HIP call (this process has no GPU to call)."""
    lib = capi.lib()
    p = C.c_void_p(1 << 20)                        # never dereferenced: every call below returns from its checks
    wt = capi.AffinityWeights(p, p, p, p)
    aff = lambda B, H, max_b=16: lib.zt_affinity(p, C.c_int64(B), C.c_int32(H), C.byref(wt), p, p, C.c_int64(max_b), C.c_int32(0),
                                                  None)
    for H in (50, 772):
        assert aff(16, H) == capi.ZT_ERR_UNSUPPORTED, H
        msg = lib.zt_last_error()
        assert (b"H=%d" % H) in msg and b"768" in msg and b"% 4" in msg, msg
    for H in (200, 344, 516, 768):
        assert aff(0, H) == capi.ZT_OK, H
    assert aff(32, 516, max_b=16) == capi.ZT_ERR_ARG                             # workspace sized for fewer edges
    try:
        for v in range(5):
            assert lib.zt_set_kernel_choice(C.c_int32(7), C.c_int32(v)) == capi.ZT_OK, v
    finally:
        assert lib.zt_set_kernel_choice(C.c_int32(7), C.c_int32(0)) == capi.ZT_OK
    assert lib.zt_set_kernel_choice(C.c_int32(99), C.c_int32(0)) == capi.ZT_ERR_ARG
    assert lib.zt_set_kernel_choice(C.c_int32(8), C.c_int32(0)) == capi.ZT_ERR_ARG


@pytest.mark.parametrize("H", [196, 200, 208, 292, 300, 304])
def test_specialised_widths_keep_their_kernels_and_launch_parameters(capi, H):
    """round_up16(H) in {208, 304}: k_affinity<KC> below 512 edges (grid (min(tiles, 160), KC), one wave), k_affinity_tiled<KC, 16>
    to 8192 edges and <KC, 32> beyond, with the LDS bytes those launches always had -- the same kernels, hence the same bits."""
    KC = round_up16(H) // 16
    assert KC in (13, 19)
    lds16, lds32 = {13: (41216, 82432), 19: (59648, 119296)}[KC]
    for B in (1, 200, 511):
        tiles = (B + 15) // 16
        assert plan(capi, B, H) == dict(form=LATENCY, KC=KC, ET=0, gx=min(tiles, 160), gy=KC, threads=64, lds=0), B
    for B in (512, 8192):
        assert plan(capi, B, H) == dict(form=TILED, KC=KC, ET=16, gx=(B + 15) // 16, gy=1, threads=256, lds=lds16), B
    assert plan(capi, 8193, H) == dict(form=TILED, KC=KC, ET=32, gx=(8193 + 31) // 32, gy=1, threads=256, lds=lds32)
    assert plan(capi, 2560, H)["gx"] == 160 and plan(capi, 2560, H, LATENCY)["gx"] == 160      # (the latency grid's cap)


@pytest.mark.parametrize("H", [4, 20, 344, 512, 516, 768])
def test_generic_widths_take_the_generic_kernels(capi, H):
    NT = round_up16(H) // 16
    lds = (48 * (round_up16(H) + 4) + 512) * 4
    assert lds <= 163840
    if H == 768:
        assert lds == 150272
    for B in (1, 17, 200, GEN_TILED_MIN - 1):
        tiles = (B + 15) // 16
        assert plan(capi, B, H) == dict(form=GEN_LATENCY, KC=0, ET=0, gx=min(tiles, 160), gy=NT, threads=64, lds=0), B
    for B in (GEN_TILED_MIN, 4096, 8200):
        assert plan(capi, B, H) == dict(form=GEN_TILED, KC=0, ET=0, gx=(B + 15) // 16, gy=1, threads=1024, lds=lds), B


def test_the_plan_refuses_what_the_library_refuses(capi):
    for H in (0, -4, 2, 50, 342, 772, 1024):
        for choice in range(5):
            assert plan(capi, 200, H, choice)["form"] == REFUSED, (H, choice)
    assert plan(capi, -1, 300)["form"] == REFUSED


def test_score_choice_pins_a_form_where_the_shape_allows(capi):
    for H in (200, 300):
        for B in (17, 200, 1000, 8200):
            for choice in (LATENCY, TILED, GEN_LATENCY, GEN_TILED):
                got = plan(capi, B, H, choice)
                assert got["form"] == choice, (H, B, choice)
            assert plan(capi, B, H, TILED)["ET"] == (16 if B <= 8192 else 32)
            assert plan(capi, B, H, GEN_TILED)["lds"] == (48 * (round_up16(H) + 4) + 512) * 4
            assert plan(capi, B, H, GEN_LATENCY)["gy"] == round_up16(H) // 16
    # no specialised kernel at this width: the library's pick
    for H in (344, 516, 768):
        for B in (17, 200, 1000):
            for choice in (LATENCY, TILED):
                assert plan(capi, B, H, choice) == plan(capi, B, H, 0), (H, B, choice)
            assert plan(capi, B, H, GEN_LATENCY)["form"] == GEN_LATENCY
            assert plan(capi, B, H, GEN_TILED)["form"] == GEN_TILED
    assert plan(capi, 200, 516, 99) == plan(capi, 200, 516, 0)


def test_selector_is_declared_and_mirrored(capi):
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(ZT_[A-Z_0-9]+)\s+(\d+)\b", hdr))
    assert defs["ZT_CHOICE_SCORE"] == 7 == capi.CHOICE_SCORE
    assert defs["ZT_CHOICE_COUNT"] == 8
    for name, val in (("LATENCY", LATENCY), ("TILED", TILED), ("GENERIC_LATENCY", GEN_LATENCY), ("GENERIC_TILED", GEN_TILED)):
        assert defs["ZT_SCORE_" + name] == val == getattr(capi, "SCORE_" + name), name
    hooks = open(os.path.join(ROOT, "zebra_amd", "csrc", "test_hooks.h")).read()
    assert "zt_test_affinity_plan" in hooks
