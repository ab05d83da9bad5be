"""Top-K link scoring without a GPU: the numpy restatement of the selection rule on hand-made arrays, zt_affinity_topk's
argument checks (all before any device call), its workspace size and its host-side plan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers_topk import select_topk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zt_affinity_topk_workspace_bytes", "zt_affinity_topk", "zt_affinity_topk_plan")


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


# ---- 1. the selection rule ----------------------------------------------------------------------------------------------
def test_select_topk_on_hand_made_arrays():
    A = -1
    nan = np.float32("nan")
    # exact ties: ascending column among equals
    p = np.array([[0.5, 0.9, 0.5, 0.9, 0.1]], np.float32)
    i, v = select_topk(p, None, 3)
    assert i.tolist() == [[1, 3, 0]] and v.tolist() == [[np.float32(0.9), np.float32(0.9), np.float32(0.5)]]
    assert i.dtype == np.int32 and v.dtype == np.float32
    # an all-equal row: the first K columns
    i, v = select_topk(np.full((1, 6), 0.25, np.float32), None, 4)
    assert i.tolist() == [[0, 1, 2, 3]] and (v == np.float32(0.25)).all()
    # K above the number present: -1 and 0 behind; an all-absent row
    p = np.array([[0.3, 0.8, 0.6], [0.7, 0.7, 0.7]], np.float32)
    ix = np.array([[4, A, 9], [A, A, A]], np.int32)
    i, v = select_topk(p, ix, 4)
    assert i.tolist() == [[2, 0, A, A], [A, A, A, A]]
    assert v.tolist() == [[np.float32(0.6), np.float32(0.3), 0.0, 0.0], [0.0] * 4]
    # skip names a GLOBAL column (idx_base + column); -1 skips nothing
    p = np.array([[0.1, 0.9, 0.5], [0.1, 0.9, 0.5]], np.float32)
    i, v = select_topk(p, None, 2, skip=np.array([11, -1]), idx_base=10)
    assert i.tolist() == [[12, 10], [11, 12]] and v[0].tolist() == [np.float32(0.5), np.float32(0.1)]
    i, _ = select_topk(p, None, 2, skip=np.array([1, 1]), idx_base=10)       # column 1 + 10 is not 1: nothing skipped
    assert i.tolist() == [[11, 12], [11, 12]]
    # a NaN is never selected
    i, v = select_topk(np.array([[nan, 0.2, nan, 0.0]], np.float32), None, 3)
    assert i.tolist() == [[1, 3, A]] and v.tolist() == [[np.float32(0.2), 0.0, 0.0]]
    # C = 1
    i, v = select_topk(np.array([[0.4]], np.float32), None, 1)
    assert i.tolist() == [[0]] and v.tolist() == [[np.float32(0.4)]]
    i, v = select_topk(np.array([[0.4]], np.float32), np.array([[A]], np.int32), 2)
    assert i.tolist() == [[A, A]] and v.tolist() == [[0.0, 0.0]]


# ---- 2. the C-ABI: symbols, argument checks, workspace, plan ---------------------------------------------------------------
def test_topk_symbols_are_declared_exported_and_listed(capi):
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    declared = set(re.findall(r"\b(zt_[a-z_0-9]+)\s*\(", hdr))
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    for sname in NEW_SYMBOLS:
        assert sname in declared and sname in exported and sname in capi.SYMBOLS, sname
    assert int(re.search(r"#define ZT_TOPK_MAX_K (\d+)", hdr).group(1)) == capi.TOPK_MAX_K == 256
    assert int(re.search(r"#define ZT_TOPK_PLAN_FIELDS (\d+)", hdr).group(1)) == len(capi.TOPK_PLAN_FIELDS)


def _ws(capi, Q, Nc, H, K):
    return capi.lib().zt_affinity_topk_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H), C.c_int32(K))


def test_topk_checks_its_arguments_first(capi):
    """NULL pointers, bad K and H, C != Nc without indices, a workspace below the minimum, the int32 overflow of the indices
    and Q = 0 all return from the host-side checks (this process has no GPU to call); the pointers are never dereferenced."""
    lib = capi.lib()
    p = C.c_void_p(1 << 20)
    wt = capi.AffinityWeights(p, p, p, p)
    i64, i32 = C.c_int64, C.c_int32
    big = 1 << 40

    def topk(Q=8, Nc=8, C_=8, H=300, K=10, eq=p, ec=p, ix=p, w=C.byref(wt), skip=None, base=0, acc=0, ti=p, tp=p, ws=p,
             ws_bytes=big):
        return lib.zt_affinity_topk(eq, i64(Q), ec, i64(Nc), ix, i64(C_), i32(H), w, i32(K), skip, i64(base), i32(acc), ti, tp, ws,
                                    i64(ws_bytes), None)

    for kw in (dict(eq=None), dict(ec=None), dict(w=None), dict(ti=None), dict(tp=None), dict(ws=None), dict(Q=-1), dict(Nc=-1),
               dict(C_=-1), dict(base=-1)):
        assert topk(**kw) == capi.ZT_ERR_ARG, kw
    assert topk(K=0) == capi.ZT_ERR_ARG and topk(K=-3) == capi.ZT_ERR_ARG
    assert b"K=0" in lib.zt_last_error() or b"K=-3" in lib.zt_last_error()
    assert topk(K=257) == capi.ZT_ERR_UNSUPPORTED
    msg = lib.zt_last_error()
    assert b"K=257" in msg and b"256" in msg, msg
    for H in (50, 4356):
        assert topk(H=H) == capi.ZT_ERR_UNSUPPORTED, H
        msg = lib.zt_last_error()
        assert (b"H=%d" % H) in msg and b"4352" in msg, msg
    assert topk(ix=None, Nc=8, C_=7) == capi.ZT_ERR_ARG                       # no cand_idx: C is Nc
    # the workspace: the size for Nc = 32 is the smallest accepted, whatever this call's Nc
    least = _ws(capi, 8, 32, 300, 10)
    assert _ws(capi, 8, 8, 300, 10) == least and _ws(capi, 8, 33, 300, 10) > least
    assert topk(Q=0, ws_bytes=_ws(capi, 0, 32, 300, 10) - 1) == capi.ZT_ERR_ARG
    assert topk(ws_bytes=least - 1) == capi.ZT_ERR_ARG
    assert b"workspace" in lib.zt_last_error()
    assert topk(Q=0, ws_bytes=_ws(capi, 0, 32, 300, 10)) == capi.ZT_OK
    # idx_base + C beyond int32
    assert topk(base=2 ** 31 - 8) == capi.ZT_ERR_ARG
    assert b"idx_base" in lib.zt_last_error()
    assert topk(Q=0, base=2 ** 31 - 9) == capi.ZT_OK
    for H, K in ((4, 1), (772, 64), (4352, 256)):
        assert topk(Q=0, H=H, K=K) == capi.ZT_OK
        assert topk(Q=0, Nc=0, C_=0, ix=None, H=H, K=K) == capi.ZT_OK


def test_topk_workspace_bytes(capi):
    for H in (0, 2, 50, 4356, -4):
        assert _ws(capi, 200, 1000, H, 10) == -1, H
    for K in (0, -1, 257):
        assert _ws(capi, 200, 1000, 300, K) == -1, K
    assert _ws(capi, -1, 10, 300, 10) == -1 and _ws(capi, 10, -1, 300, 10) == -1
    for H, K in ((4, 1), (300, 10), (300, 64), (300, 65), (4352, 256)):
        a, b = _ws(capi, 200, 10 ** 6, H, K), _ws(capi, 200, 10 ** 8, H, K)
        assert a == b > 0, (H, K)                               # the pool no longer shows beyond the slab cap
        assert a <= 256 + 200 * H * 4 + (128 << 20) + (64 << 20), (H, K)
        sizes = [_ws(capi, Q, 5000, H, K) for Q in (0, 1, 4, 5, 200, 4096, 100000)]
        assert all(x > 0 for x in sizes) and sizes == sorted(sizes), (H, K, sizes)
        assert _ws(capi, 200, 5000, H, K) >= 256 + (200 + min(5000, (128 << 20) // (4 * H))) * H * 4
    # the other scorers' sizes are untouched
    lib = capi.lib()
    assert lib.zt_affinity_rank_workspace_bytes(C.c_int64(200), C.c_int64(1000), C.c_int32(772)) == 256 + 1200 * 772 * 4
    assert lib.zt_affinity_workspace_bytes(C.c_int64(200), C.c_int32(772)) == -1
    assert lib.zt_affinity_train_workspace_bytes(C.c_int64(200), C.c_int32(772)) == -1


def test_topk_plan(capi):
    H = 300
    for Q, Nc, K in ((200, 100000, 10), (17, 2500, 65), (4096, 10000, 50), (1, 1, 1), (5, 31, 256)):
        full = _ws(capi, Q, Nc, H, K)
        pl = capi.topk_plan(Q, Nc, Nc, H, K, False, full)
        assert pl["form"] == (capi.TOPK_FORM_LANE if K <= 64 else capi.TOPK_FORM_LANE4)
        assert pl["wave_queries"] == 4 and pl["q_tiles"] == (Q + 3) // 4
        assert pl["slab_rows"] % 32 == 0 and pl["slab_rows"] >= min(Nc, 32)
        assert pl["n_slabs"] == 1 and pl["slab_rows"] >= Nc                    # the recommended size holds this pool whole
        assert pl["n_spans"] * pl["span_cols"] >= min(Nc, pl["slab_rows"]) and pl["span_cols"] % 128 == 0
        assert pl["grid_pairs"] == pl["q_tiles"] * pl["n_spans"] and pl["grid_merge"] == (Q + 3) // 4
        assert 256 + Q * H * 4 <= pl["lists_offset"] < pl["pc_offset"] and pl["pc_offset"] % 256 == 0
        assert pl["pc_offset"] + pl["slab_rows"] * H * 4 <= full
        assert pl["min_bytes"] == _ws(capi, Q, 32, H, K) == pl["pc_offset"] + 32 * H * 4
        # slab rows shrink with the workspace, the slabs still cover the pool, the lists stay where they are
        least = capi.topk_plan(Q, Nc, Nc, H, K, False, pl["min_bytes"])
        assert least["slab_rows"] == 32 and least["n_slabs"] == max(1, (Nc + 31) // 32)
        assert least["n_slabs"] * least["slab_rows"] >= Nc
        assert (least["lists_offset"], least["pc_offset"], least["form"]) == (pl["lists_offset"], pl["pc_offset"], pl["form"])
        mid = capi.topk_plan(Q, Nc, Nc, H, K, False, pl["min_bytes"] + 100 * H * 4)
        assert mid["slab_rows"] == 128 and mid["n_slabs"] * mid["slab_rows"] >= Nc
        with pytest.raises(ValueError, match="workspace"):
            capi.topk_plan(Q, Nc, Nc, H, K, False, pl["min_bytes"] - 1)
        # indexed: a wave per query, the spans cut the C index columns
        ip = capi.topk_plan(Q, Nc, 777, H, K, True, full)
        assert ip["wave_queries"] == 1 and ip["span_cols"] % 32 == 0 and ip["n_spans"] * ip["span_cols"] >= 777
        assert ip["form"] == pl["form"] and ip["slab_rows"] == pl["slab_rows"]
    # beyond the slab cap: several slabs at the recommended size too
    pl = capi.topk_plan(200, 10 ** 6, 10 ** 6, H, 10, False, _ws(capi, 200, 10 ** 6, H, 10))
    assert pl["n_slabs"] > 1 and pl["n_slabs"] * pl["slab_rows"] >= 10 ** 6 and pl["slab_rows"] * H * 4 <= 128 << 20
    # K = 64 and K = 65 are the two forms' edge
    assert capi.topk_plan(8, 64, 64, H, 64, False, 1 << 30)["form"] == capi.TOPK_FORM_LANE
    assert capi.topk_plan(8, 64, 64, H, 65, False, 1 << 30)["form"] == capi.TOPK_FORM_LANE4
    with pytest.raises(ValueError):
        capi.topk_plan(8, 64, 63, H, 10, False, 1 << 30)                       # no indices: C is Nc
    with pytest.raises(ValueError, match="K=257"):
        capi.topk_plan(8, 64, 64, H, 257, False, 1 << 30)
    with pytest.raises(ValueError, match="H=50"):
        capi.topk_plan(8, 64, 64, 50, 10, False, 1 << 30)
