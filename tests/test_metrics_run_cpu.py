"""The link-metrics kernel plan and the argument checks of the step's metrics tail without a GPU (csrc/scoring.hip:
zt::link_metrics_plan through zt_link_metrics_plan; csrc/pipeline.hip: zt_pipeline_set_metrics, zt_pipeline_metrics): up to
8192 pairs the single-kernel form with the launch parameters zt_link_metrics always computed, from 8193 to 16384 pairs the
two-run form within the 160 KB of LDS, refused beyond; every refusal is answered before the first device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED, SINGLE, SPLIT = 0, 1, 2
LDS_PER_WORKGROUP = 163840     # gfx950


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def pow2_at_least(x):
    n = 1
    while n < x:
        n <<= 1
    return n


@pytest.mark.parametrize("B", [1, 512, 513, 4096, 8192])
def test_up_to_8192_pairs_keep_the_single_kernel_and_its_launch(capi, B):
    """The values zt_link_metrics computed before the plan existed: one workgroup of 1024 threads, n2 = the next power of two
    >= max(1024, 2B) u64 keys, 8 bytes of LDS each."""
    n2 = pow2_at_least(max(1024, 2 * B))
    assert capi.link_metrics_plan(B) == dict(form=SINGLE, threads=1024, n2=n2, lds_bytes=8 * n2)


def test_single_form_padded_lengths():
    assert [pow2_at_least(max(1024, 2 * B)) for B in (1, 512, 513, 4096, 8192)] == [1024, 1024, 2048, 8192, 16384]


@pytest.mark.parametrize("B", [8193, 12000, 16384])
def test_beyond_8192_pairs_take_the_two_run_form_within_lds(capi, B):
    p = capi.link_metrics_plan(B)
    assert p["form"] == SPLIT
    assert p["threads"] == 1024
    assert p["n2"] == 2 * pow2_at_least(B) and p["n2"] >= 2 * B          # both runs fit, padding included
    assert p["lds_bytes"] == 4 * p["n2"]                                 # 32-bit keys
    assert 0 < p["lds_bytes"] <= LDS_PER_WORKGROUP


@pytest.mark.parametrize("B", [0, -1, 16385])
def test_plan_refuses_no_pairs_and_more_than_16384(capi, B):
    assert capi.link_metrics_plan(B) == dict(form=REFUSED, threads=0, n2=0, lds_bytes=0)


def test_plan_wants_somewhere_to_write(capi):
    assert capi.lib().zt_link_metrics_plan(C.c_int64(200), None) == capi.ZT_ERR_ARG


def test_checks_come_before_any_device_call(capi):
    """This process has no GPU to call: every answer below comes from the checks."""
    lib = capi.lib()
    p = C.c_void_p(1 << 20)                        # never dereferenced
    assert lib.zt_pipeline_set_metrics(None, p, p, C.c_int64(8)) == capi.ZT_ERR_ARG
    assert lib.zt_pipeline_set_metrics(None, None, None, C.c_int64(0)) == capi.ZT_ERR_ARG
    n = C.c_int64(-7)
    assert lib.zt_pipeline_metrics(None, None, C.byref(n)) == capi.ZT_ERR_ARG
    assert n.value == -7
    assert lib.zt_link_metrics(p, p, C.c_int64(16385), p, C.c_int32(0), None) == capi.ZT_ERR_UNSUPPORTED
    msg = lib.zt_last_error()
    assert b"16385" in msg and b"16384" in msg, msg
    assert lib.zt_link_metrics(p, p, C.c_int64(0), p, C.c_int32(0), None) == capi.ZT_ERR_ARG
    assert lib.zt_link_metrics(None, p, C.c_int64(16), p, C.c_int32(0), None) == capi.ZT_ERR_ARG


def test_forms_are_declared_and_mirrored(capi):
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(ZT_[A-Z_0-9]+)\s+(\d+)\b", hdr))
    assert defs["ZT_METRICS_FORM_REFUSED"] == REFUSED == capi.METRICS_FORM_REFUSED
    assert defs["ZT_METRICS_FORM_SINGLE"] == SINGLE == capi.METRICS_FORM_SINGLE
    assert defs["ZT_METRICS_FORM_SPLIT"] == SPLIT == capi.METRICS_FORM_SPLIT
    assert defs["ZT_METRICS_MAX_B"] == 16384 == capi.METRICS_MAX_B
    assert defs["ZT_METRICS_PLAN_FIELDS"] == 4
    for name in ("zt_link_metrics_plan", "zt_pipeline_set_metrics", "zt_pipeline_metrics"):
        assert name in capi.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr), name
