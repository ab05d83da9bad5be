"""Read-only queries and ranking without a GPU: the row emission of zt_tppr_query restated in numpy and held against the
reference's stream fixtures through the CPU oracle; the rank definition on hand-made arrays; the host-side checks of the four
new entry points (symbols, widths, workspace sizes, refusals -- all before any device call)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import inputs as I
from conftest import golden
from helpers_query import comparable, emit_rows, rank_cases, rank_of_positive, rank_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zt_tppr_query", "zt_affinity_rank_workspace_bytes", "zt_affinity_rank", "zt_rank_metrics")


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


# ---- 1. the emission, pinned to the reference's fixtures ---------------------------------------------------------------
@pytest.mark.parametrize("name,floor,exact", [("tiny_general", 0.75, False), ("bs1_single", 1.0, True), ("gen_m3", 0.75, False)])
def test_row_emission_restatement_matches_the_reference(oracle, name, floor, exact):
    """Before each batch, the oracle's dictionaries of [src | dst | neg] emitted by the restatement at the batch's times are
    the fixture's rows, bit for bit, wherever the row's node is not an endpoint of an earlier edge of the batch."""
    kind, N, E, seed, bs, k, al, be, full = I.STREAM_CASES[name]
    assert full
    g = golden("g1_stream_" + name)
    src, dst, neg, ts, eidx = I.make_stream(kind, N, E, seed)
    o = oracle.TpprOracle(N, k, len(al), al, be)
    rows_seen = rows_cmp = 0
    for b in range((E + bs - 1) // bs):
        s, e = b * bs, min(E, (b + 1) * bs)
        nodes = np.concatenate([src[s:e], dst[s:e], neg[s:e]])
        t3 = np.concatenate([ts[s:e]] * 3)
        ok = comparable(src[s:e], dst[s:e], neg[s:e])
        for m in range(len(al)):
            got = emit_rows(o.export_rows(m, nodes), t3)
            for a, key in zip(got, ("nodes", "eidx", "dt", "w")):
                want = g["b%d_%s" % (b, key)][m]
                assert a.dtype == want.dtype
                assert np.array_equal(a[ok].view(np.uint32), want[ok].view(np.uint32)), (name, b, m, key)
        rows_seen += len(ok)
        rows_cmp += int(ok.sum())
        o.streaming_topk(nodes, t3, eidx[s:e])
    share = rows_cmp / rows_seen
    print("%s: %d of %d rows compared (%.3f)" % (name, rows_cmp, rows_seen, share))
    assert share == 1.0 if exact else share >= floor


# ---- 2. the rank definition -----------------------------------------------------------------------------------------------
def test_rank_definition_on_hand_made_arrays():
    for prob, idx, want in rank_cases():
        got = rank_of_positive(prob, idx)
        assert got.dtype == np.float32 and got.tolist() == want, (prob, idx)
    # the mean of the optimistic and the pessimistic rank
    p = np.array([[0.5, 0.5, 0.5, 0.7, 0.1]], np.float32)
    opt, pes = 1 + (p[0, 1:] > 0.5).sum(), 1 + (p[0, 1:] >= 0.5).sum()
    assert rank_of_positive(p)[0] == (opt + pes) / 2 == 3.0
    # the sums: a skipped query is not counted; Hits@n counts rank <= n
    s = rank_sums(np.array([1.0, 2.5, 0.0, 10.5, 10.0, 3.0], np.float32))
    assert s.tolist() == [1 + 1 / 2.5 + 1 / 10.5 + 1 / 10.0 + 1 / 3.0, 1.0, 3.0, 4.0, 5.0]


# ---- 3. the library, before any device call -------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_listed(capi):
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    declared = set(re.findall(r"\b(zt_[a-z_0-9]+)\s*\(", hdr))
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    for sname in NEW_SYMBOLS:
        assert sname in declared and sname in exported and sname in capi.SYMBOLS, sname
        assert hasattr(capi.lib(), sname)


def test_rank_workspace_and_widths(capi):
    lib = capi.lib()
    ws = lambda Q, Nc, H: lib.zt_affinity_rank_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H))
    for H in (4, 20, 300, 516, 772, 860, 4352):
        assert ws(200, 1000, H) > 0, H
        assert ws(200, 1000, H) >= (200 + 1000) * H * 4, H
        assert ws(0, 0, H) > 0, H
    for H in (0, 2, 50, 4356, -4):
        assert ws(200, 1000, H) == -1, H
    assert ws(-1, 10, 300) == -1 and ws(10, -1, 300) == -1
    assert (capi.RANK_MIN_H, capi.RANK_MAX_H) == (4, 4352)
    # the pair scorers keep their own bound
    assert lib.zt_affinity_workspace_bytes(C.c_int64(200), C.c_int32(772)) == -1
    assert lib.zt_affinity_train_workspace_bytes(C.c_int64(200), C.c_int32(772)) == -1


def test_new_entry_points_check_their_arguments_first(capi):
    """NULL pointers, negative sizes, unsupported widths and empty calls all return from the host-side checks (this process
    has no GPU to call); the pointers below are never dereferenced."""
    lib = capi.lib()
    p = C.c_void_p(1 << 20)
    wt = capi.AffinityWeights(p, p, p, p)
    i64, i32 = C.c_int64, C.c_int32

    def rank(Q=8, Nc=8, C_=8, H=300, eq=p, ec=p, ix=p, w=C.byref(wt), prob=p, ws=p):
        return lib.zt_affinity_rank(eq, i64(Q), ec, i64(Nc), ix, i64(C_), i32(H), w, prob, ws, None)

    for kw in (dict(eq=None), dict(ec=None), dict(w=None), dict(prob=None), dict(ws=None), dict(Q=-1), dict(Nc=-1), dict(C_=-1)):
        assert rank(**kw) == capi.ZT_ERR_ARG, kw
    assert rank(ix=None, Nc=8, C_=7) == capi.ZT_ERR_ARG             # no cand_idx: C is Nc
    for H in (0, 2, 50, 4356, -4):
        assert rank(H=H) == capi.ZT_ERR_UNSUPPORTED, H
        msg = lib.zt_last_error()
        assert (b"H=%d" % H) in msg and b"4352" in msg, msg
    for H in (4, 772, 4352):
        assert rank(Q=0, H=H) == capi.ZT_OK and rank(C_=0, H=H) == capi.ZT_OK
        assert rank(Q=0, Nc=0, C_=0, ix=None, H=H) == capi.ZT_OK

    met = lambda Q=4, C_=4, prob=p, acc=p: lib.zt_rank_metrics(prob, None, i64(Q), i64(C_), None, acc, None)
    assert met(prob=None) == capi.ZT_ERR_ARG and met(acc=None) == capi.ZT_ERR_ARG
    assert met(Q=-1) == capi.ZT_ERR_ARG and met(C_=-1) == capi.ZT_ERR_ARG
    assert met(Q=0) == capi.ZT_OK and met(C_=0) == capi.ZT_OK

    # zt_tppr_query: the argument checks that need no handle, then a NULL handle
    qry = lambda h=p, nodes=p, ts=p, N=4, on=p, oe=p, od=p, ow=p: lib.zt_tppr_query(h, nodes, ts, i64(N), i32(-1), on, oe, od,
                                                                                    ow, None, None)
    for kw in (dict(h=None), dict(nodes=None), dict(ts=None), dict(on=None), dict(oe=None), dict(od=None), dict(ow=None),
               dict(N=-1)):
        assert qry(**kw) == capi.ZT_ERR_ARG, kw
    assert qry(N=0) == capi.ZT_OK                                   # nothing enqueued, the handle is not looked at
