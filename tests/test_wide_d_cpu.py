"""CPU-side checks of the memory / embedding widths 128 < D <= 256 (D % 4 == 0): the embed workspace is offered, the plans
(zt::embed_kernel_plan, zt::memory_kernel_plan through the test hooks) pin the kernel each wide shape gets, the widths
that stay refused keep their refusal kinds, and the new instantiations keep within the chip's limits (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

AGG = {"unsupported": 0, "reg": 1, "wide": 2, "d100": 3, "tiled_table": 4, "tiled_full": 5, "tiled_table_big": 6,
       "tiled_full_big": 7, "split": 8}
OUT_TILED = 0
REFUSAL = {"none": 0, "arg": 1, "d_large": 2, "msg_wide": 3}
GRU = {"none": 0, "tile": 1, "split": 2}


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def hooks(capi):
    return capi.hooks_lib()


def _ws(capi, N, D, F, T, M, k):
    return capi.lib().zt_embed_workspace_bytes(C.c_int64(N), C.c_int32(D), C.c_int32(F), C.c_int32(T), C.c_int32(M),
                                               C.c_int32(k))


def plan(hooks, N, D, F, T, M, k, table, training=False):
    a, o, lds = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    rc = hooks.zt_test_embed_plan(C.c_int64(N), C.c_int32(D), C.c_int32(F), C.c_int32(T), C.c_int32(M), C.c_int32(k),
                                  C.c_int32(int(table)), C.c_int32(int(training)), C.c_int32(0), C.c_int32(0), C.byref(a),
                                  C.byref(o), C.byref(lds))
    assert rc == 0
    return a.value, o.value, lds.value


@pytest.mark.parametrize("D", [132, 172, 200, 256])
@pytest.mark.parametrize("F", [1, 172])
@pytest.mark.parametrize("k", [20, 100, 255])
def test_wide_shapes_have_kernels_and_workspace(capi, hooks, D, F, k):
    """Every wide shape has an eval kernel with the table and without it and a training kernel (each refused before), and
    the workspace for them."""
    for table, training in ((False, False), (True, False), (False, True)):
        assert plan(hooks, 1000, D, F, 100, 2, k, table, training)[0] != AGG["unsupported"], (table, training)
    assert _ws(capi, 1000, D, F, 100, 2, k) >= 0


def _train_ok(capi, N, D, F, T, M, k):
    return capi.lib().zt_agg_train_supported(C.c_int64(N), C.c_int32(D), C.c_int32(F), C.c_int32(T), C.c_int32(M),
                                             C.c_int32(k))


# (D, F, k) at N = 600, T = 100, M = 2 -> zt_agg_train_supported: the forward's training plan and the backward's tile both
# take the shape (modules.py: the fused path where 1, the torch composition where 0)
TRAIN_SUPPORT = [
    ((100, 1, 20), 1), ((100, 172, 255), 1), ((128, 172, 100), 1),
    ((132, 1, 20), 1), ((172, 172, 20), 1), ((172, 1, 100), 1), ((172, 172, 255), 1), ((200, 172, 100), 1), ((256, 172, 20), 1),
    ((256, 1, 255), 1),
    ((129, 1, 20), 0), ((130, 172, 20), 0), ((257, 1, 20), 0), ((260, 172, 20), 0),
    ((100, 1, 256), 0),          # k beyond ZT_MAX_K_WIDE: refused although the table path offers a workspace (eval only)
    ((172, 1, 256), 0),
]


@pytest.mark.parametrize("shape,want", TRAIN_SUPPORT, ids=[str(s) for s, _ in TRAIN_SUPPORT])
def test_fused_training_support(capi, shape, want):
    D, F, k = shape
    assert _train_ok(capi, 600, D, F, 100, 2, k) == want
    assert _train_ok(capi, 0, D, F, 100, 2, k) == want          # (N = 0: the shape alone)


def test_training_support_is_the_exact_gate(capi):
    """A shape that only the table path takes has an embed workspace, but no training kernel: the query says so."""
    assert _ws(capi, 1000, 100, 1, 100, 2, 256) >= 0
    assert _train_ok(capi, 1000, 100, 1, 100, 2, 256) == 0
    assert _train_ok(capi, 1000, 172, 172, 100, 0, 20) == 0       # bad argument


# (D, F, k) at N = 600, T = 100, M = 2 -> (eval without the table, eval with it, training); the output layers are the tiled
# kernel for every wide shape (the latency and persistent forms keep their widths)
PLANS = [
    ((132, 1, 20), (("tiled_full", 79760), ("tiled_full", 79760), ("tiled_full", 79760))),
    ((132, 172, 100), (("split", 0), ("tiled_table_big", 125840), ("split", 0))),
    ((172, 1, 20), (("tiled_full", 95120), ("tiled_full", 95120), ("tiled_full", 95120))),       # F + T < D: no table path
    ((172, 1, 100), (("tiled_full_big", 133008), ("tiled_full_big", 133008), ("split", 0))),
    ((172, 1, 255), (("split", 0), ("split", 0), ("split", 0))),
    ((172, 172, 20), (("tiled_full", 146320), ("tiled_table", 90000), ("tiled_full", 146320))),
    ((172, 172, 100), (("split", 0), ("tiled_table_big", 125840), ("split", 0))),
    ((200, 1, 100), (("tiled_full_big", 140176), ("tiled_full_big", 140176), ("split", 0))),
    ((256, 1, 20), (("tiled_full", 120720), ("tiled_full", 120720), ("tiled_full", 120720))),
    ((256, 1, 100), (("split", 0), ("split", 0), ("split", 0))),
    ((256, 172, 20), (("tiled_full", 137616), ("tiled_table", 90000), ("tiled_full", 137616))),
    ((256, 172, 100), (("split", 0), ("tiled_table_big", 125840), ("split", 0))),
    ((256, 172, 255), (("split", 0), ("split", 0), ("split", 0))),
]


@pytest.mark.parametrize("shape,want", PLANS, ids=[str(s) for s, _ in PLANS])
def test_wide_embed_kernel_choice(hooks, shape, want):
    D, F, k = shape
    for (table, training), (agg, lds) in zip(((False, False), (True, False), (False, True)), want):
        assert plan(hooks, 600, D, F, 100, 2, k, table, training) == (AGG[agg], OUT_TILED, lds), (table, training)


@pytest.mark.parametrize("D", [129, 130, 131, 257, 260])
def test_widths_that_stay_refused(capi, hooks, D):
    for F, k, table in ((1, 20, True), (172, 20, False), (172, 100, True), (1, 255, False)):
        assert plan(hooks, 600, D, F, 100, 2, k, table)[0] == AGG["unsupported"]
        assert plan(hooks, 600, D, F, 100, 2, k, False, training=True)[0] == AGG["unsupported"]
        assert _ws(capi, 1000, D, F, 100, 2, k) == -1
    for rows in (0, 400):
        p = memory_plan(hooks, rows, D, 2 * D + 272)
        assert (p["refusal"], p["gru"]) == (REFUSAL["d_large"], GRU["none"])


def memory_plan(hooks, rows, D, msg, F=172, T=100):
    out = (C.c_int64 * 14)(*([-1] * 14))
    rc = hooks.zt_test_memory_plan(C.c_int64(rows), C.c_int32(D), C.c_int32(msg), C.c_int32(F), C.c_int32(T), C.c_int32(0),
                                   C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0),
                                   C.c_int32(0), C.c_int64(0), C.c_int32(0), out)
    assert rc == 0
    keys = ("refusal", "msg", "gru", "out", "lds", "lds2", "lds_f", "gru_tiles", "NTg")
    return dict(zip(keys, list(out)))


# (rows, D, F) with msg = 2 D + F + 100 -> (GRU form, its dynamic LDS, 16-row tiles, hidden N-tiles): always the tile (the
# split stays at Hp <= 112); one workgroup owns every column of its 16 rows
MEMORY = [((r, D, F), (r + 15) // 16) for r in (1, 400, 8192) for D in (132, 172, 256) for F in (1, 172)]
MEM_LDS = {(132, 1): 33152, (132, 172): 44416, (172, 1): 40320, (172, 172): 51584, (256, 1): 56704, (256, 172): 66944}


@pytest.mark.parametrize("shape,tiles", MEMORY, ids=[str(s) for s, _ in MEMORY])
def test_wide_memory_kernel_choice(hooks, shape, tiles):
    rows, D, F = shape
    p = memory_plan(hooks, rows, D, 2 * D + F + 100, F=F)
    assert (p["refusal"], p["msg"], p["gru"], p["out"]) == (REFUSAL["none"], 0, GRU["tile"], 0)
    assert (p["lds"], p["gru_tiles"], p["NTg"]) == (MEM_LDS[(D, F)], tiles, (D + 15) // 16)


def _notes(capi, tmp_path, obj_name):
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), obj_name)
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(obj) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("no built object / no LLVM tools here")
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "k.co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, obj, str(tmp_path / "unused.o")],
                   check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co], check=True)
    return subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                          text=True).stdout


# the wide instantiations, by a fragment of their mangled names
WIDE_KERNELS = [
    ("aggregate.o", "k_fc1_aggILb0ELi5ELi4E"), ("aggregate.o", "k_fc1_aggILb1ELi5ELi4E"),
    ("aggregate.o", "k_fc1_aggILb0ELi8ELi4E"), ("aggregate.o", "k_fc1_aggILb1ELi8ELi4E"),
    ("aggregate.o", "k_embed_outILi1ELi4E"), ("aggregate.o", "k_project_rowsILi4E"),
    ("aggregate_split.o", "k_fc1_agg_splitILi4E"), ("aggregate_bwd.o", "k_fc1_agg_bwdILi4E"),
    ("memory_update.o", "k_gruILi0ELi2E"), ("memory_update.o", "k_gruILi1ELi2E"),
]


@pytest.mark.parametrize("obj,kernel", WIDE_KERNELS)
def test_wide_kernels_use_no_scratch(capi, tmp_path, obj, kernel):
    notes = _notes(capi, tmp_path, obj)
    meta = None
    for b in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(\S+)", b)
        if m and kernel in m.group(1) and not m.group(1).endswith(".kd"):
            meta = b
            break
    assert meta is not None, "%s not found in %s" % (kernel, obj)
    priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    grp = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
    assert priv and int(priv.group(1)) == 0, "%s spills to scratch" % kernel
    assert grp and int(grp.group(1)) <= 160 * 1024
