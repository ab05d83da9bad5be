"""CPU-side checks of the row-split aggregation (csrc/aggregate_split.hip and the chunked tiles of k_fc1_agg_bwd):
the embed workspace is offered for query rows wider than one LDS tile (F = 172 past k = 136), and the new kernel's
code object keeps within the chip's limits (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def _ws(capi, N, D, F, T, M, k):
    return capi.lib().zt_embed_workspace_bytes(C.c_int64(N), C.c_int32(D), C.c_int32(F), C.c_int32(T), C.c_int32(M),
                                               C.c_int32(k))


@pytest.mark.parametrize("k", [137, 160, 200, 255])
def test_embed_workspace_for_wide_edge_features_past_one_tile(capi, k):
    """Wikipedia / Reddit widths (D = T = 100, F = 172): no tile holds such a query row, the row split does."""
    assert _ws(capi, 1000, 100, 172, 100, 2, k) >= 0


@pytest.mark.parametrize("F,k", [(1, 80), (1, 255), (4, 128), (172, 40), (172, 128)])
def test_embed_workspace_of_the_shapes_that_ran_before(capi, F, k):
    assert _ws(capi, 1000, 100, F, 100, 2, k) >= 0


def test_embed_workspace_still_refuses_what_no_kernel_takes(capi):
    assert _ws(capi, 1000, 100, 172, 100, 2, 256) == -1             # beyond ZT_MAX_K_WIDE
    assert _ws(capi, 1000, 100, 172, 100, 2, 0) == -1


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


def _kernel_meta(notes, name):
    """The metadata block of the kernel whose mangled name contains `name`."""
    blocks = re.split(r"\n\s+- \.", notes)
    for b in blocks:
        m = re.search(r"\.name:\s+(\S+)", b)
        if m and name in m.group(1) and not m.group(1).endswith(".kd"):
            return b
    return None


@pytest.mark.parametrize("obj,kernel", [("aggregate_split.o", "k_fc1_agg_split"), ("aggregate_bwd.o", "k_fc1_agg_bwd")])
def test_row_split_kernels_use_no_scratch(capi, tmp_path, obj, kernel):
    notes = _notes(capi, tmp_path, obj)
    meta = _kernel_meta(notes, kernel)
    assert meta is not None, "%s not found in %s" % (kernel, obj)
    priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
    grp = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
    assert priv and int(priv.group(1)) == 0, "%s spills to scratch" % kernel
    assert grp and int(grp.group(1)) <= 160 * 1024
