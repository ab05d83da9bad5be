"""Filtered top-K without a GPU: the three new entry points are declared, exported and check their arguments before any device
call; TGN.topk_scores(absent=...) on CPU tensors; the plan and the workspace do not know the mask; the numpy restatement of
"seen" against NeighborFinder.find_before."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import inputs as I
from helpers_filtered import adjacency, bits_to_mask, mark_bits, mask_to_bits, masked_idx, seen_ranges
from helpers_topk import select_topk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zt_affinity_topk_masked", "zt_csr_seen_ranges", "zt_exclude_mark")


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def test_filtered_symbols_are_declared_exported_and_listed(capi):
    hdr = open(os.path.join(ROOT, "include", "zebra_amd.h")).read()
    declared = set(re.findall(r"\b(zt_[a-z_0-9]+)\s*\(", hdr))
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in nm.splitlines() if line.strip())
    for sname in NEW_SYMBOLS:
        assert sname in declared and sname in exported and sname in capi.SYMBOLS, sname
    from zebra_amd import build
    assert "seen.hip" in build.SOURCES


def _masked(capi, Q=8, Nc=8, C_=8, H=300, K=10, ix="p", ws_bytes=1 << 40, absent="p", words=1, **null):
    """zt_affinity_topk_masked (absent given) or zt_affinity_topk (absent None) on pointers that are never dereferenced"""
    lib = capi.lib()
    p = C.c_void_p(1 << 20)
    wt = capi.AffinityWeights(p, p, p, p)
    i64, i32 = C.c_int64, C.c_int32
    a = dict(eq=p, ec=p, w=C.byref(wt), ti=p, tp=p, ws=p)
    a.update(null)
    args = (a["eq"], i64(Q), a["ec"], i64(Nc), p if ix == "p" else ix, i64(C_), i32(H), a["w"], i32(K), None, i64(0), i32(0),
            a["ti"], a["tp"], a["ws"], i64(ws_bytes))
    if absent is None:
        return lib.zt_affinity_topk(*args, None)
    return lib.zt_affinity_topk_masked(*args, p if absent == "p" else absent, i64(words), None)


def test_masked_topk_checks_its_arguments_first(capi):
    lib = capi.lib()
    # absent_words below ceil(C / 32): ZT_ERR_ARG; NULL absent: any count goes (it is zt_affinity_topk)
    for C_, words, ok in ((8, 0, False), (32, 1, True), (33, 1, False), (33, 2, True), (2500, 78, False), (2500, 79, True),
                          (2500, 200, True)):
        rc = _masked(capi, Q=0, Nc=C_, C_=C_, words=words)
        assert rc == (capi.ZT_OK if ok else capi.ZT_ERR_ARG), (C_, words)
        if not ok:
            assert b"absent_words" in lib.zt_last_error()
        assert _masked(capi, Q=0, Nc=C_, C_=C_, absent=C.c_void_p(None), words=0) == capi.ZT_OK
    assert _masked(capi, Q=0, words=-1) == capi.ZT_ERR_ARG
    # every other refusal is zt_affinity_topk's: the same code and the same text
    cases = [dict(eq=None), dict(ec=None), dict(w=None), dict(ti=None), dict(tp=None), dict(ws=None), dict(Q=-1), dict(Nc=-1),
             dict(C_=-1), dict(K=0), dict(K=-3), dict(K=257), dict(H=50), dict(H=4356), dict(ix=None, Nc=8, C_=7),
             dict(ws_bytes=1000)]
    for kw in cases:
        plain = _masked(capi, absent=None, **kw)
        text = lib.zt_last_error()
        assert plain in (capi.ZT_ERR_ARG, capi.ZT_ERR_UNSUPPORTED), kw
        assert _masked(capi, **kw) == plain and lib.zt_last_error() == text, kw
    assert _masked(capi, K=257) == capi.ZT_ERR_UNSUPPORTED and b"K=257" in lib.zt_last_error()
    assert _masked(capi, H=50) == capi.ZT_ERR_UNSUPPORTED and b"H=50" in lib.zt_last_error()


def test_the_plan_and_the_workspace_do_not_know_the_mask(capi):
    """there is one plan and one workspace size: the masked call accepts exactly the workspaces the plain call accepts -- the
    plan's min_bytes, to the byte -- and quotes the same minimum when it refuses"""
    lib = capi.lib()
    for Q, Nc, H, K, indexed in ((200, 100000, 300, 10, False), (17, 2500, 300, 65, True), (5, 31, 4, 256, False)):
        full = lib.zt_affinity_topk_workspace_bytes(C.c_int64(Q), C.c_int64(Nc), C.c_int32(H), C.c_int32(K))
        pl = capi.topk_plan(Q, Nc, Nc, H, K, indexed, full)
        kw = dict(Q=Q, Nc=Nc, C_=Nc, H=H, K=K, ix="p" if indexed else None, words=(Nc + 31) // 32)
        texts = []
        for absent in (None, "p"):
            assert _masked(capi, ws_bytes=pl["min_bytes"] - 1, absent=absent, **kw) == capi.ZT_ERR_ARG
            texts.append(lib.zt_last_error())
            assert (b"%d" % pl["min_bytes"]) in texts[-1]
        assert texts[0] == texts[1]
        # (at min_bytes both pass the plan and stop at the next host-side check: the workspace pointer's alignment)
        odd = C.c_void_p((1 << 20) + 4)
        for absent in (None, "p"):
            assert _masked(capi, ws_bytes=pl["min_bytes"], absent=absent, ws=odd, **kw) == capi.ZT_ERR_ARG
            assert b"aligned" in lib.zt_last_error()


def test_seen_ranges_and_exclude_mark_check_their_arguments_first(capi):
    lib = capi.lib()
    p = C.c_void_p(1 << 20)
    i64 = C.c_int64

    def ranges(c=p, nodes=p, ts=p, Q=4, begin=p, length=p, status=p):
        return lib.zt_csr_seen_ranges(c, nodes, ts, i64(Q), begin, length, status, None)

    for kw in (dict(c=None), dict(nodes=None), dict(ts=None), dict(begin=None), dict(length=None), dict(status=None), dict(Q=-1)):
        assert ranges(**kw) == capi.ZT_ERR_ARG, kw
        assert b"zt_csr_seen_ranges" in lib.zt_last_error()
    assert ranges(Q=0) == capi.ZT_OK

    def mark(c=None, ids=p, begin=p, length=p, Q=4, id_lo=0, srt=None, col=None, stride=0, C_=64, absent=p, words=2):
        return lib.zt_exclude_mark(c, ids, begin, length, i64(Q), i64(id_lo), srt, col, i64(stride), i64(C_), absent, i64(words), None)

    for kw in (dict(ids=None), dict(begin=None), dict(length=None), dict(absent=None), dict(Q=-1), dict(C_=-1), dict(words=-1),
               dict(words=1), dict(C_=65), dict(srt=p), dict(srt=p, col=p, stride=5), dict(srt=p, col=p, stride=-64)):
        assert mark(**kw) == capi.ZT_ERR_ARG, kw
        assert b"zt_exclude_mark" in lib.zt_last_error()
    for kw in (dict(Q=0), dict(Q=0, c=p, ids=None), dict(Q=0, srt=p, col=p), dict(Q=0, srt=p, col=p, stride=64), dict(C_=0, words=0),
               dict(Q=0, words=50)):
        assert mark(**kw) == capi.ZT_OK, kw


# ---- the torch path of topk_scores honours the bits ----------------------------------------------------------------------
def test_topk_scores_on_cpu_tensors_honours_absent_bits():
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN, absent_columns
    H, Q, C_, Nc, K = 20, 7, 70, 40, 10
    rng = np.random.RandomState(11)
    torch.manual_seed(3)
    cpu = types.SimpleNamespace(affinity_score=MergeLayer(H, H, H, 1), device=torch.device("cpu"))
    cpu.rank_scores = types.MethodType(TGN.rank_scores, cpu)
    eq = torch.from_numpy((rng.standard_normal((Q, H)) * 0.7).astype(np.float32))
    for shared in (True, False):
        n_rows = C_ if shared else Nc
        ec = torch.from_numpy((rng.standard_normal((n_rows, H)) * 0.7).astype(np.float32))
        idx = None
        if not shared:
            idx = rng.randint(0, Nc, (Q, C_)).astype(np.int32)
            idx[rng.random_sample((Q, C_)) < 0.15] = -1
        ix = None if shared else torch.from_numpy(idx)
        prob = cpu.rank_scores(eq, ec, ix).numpy()
        mask = rng.random_sample((Q, C_)) < 0.3
        mask[1] = False                     # a query with nothing masked
        mask[2] = True                      # ... and one with everything masked
        mask[3, 64:] = True                 # (bits of the third word)
        skip = np.full(Q, -1, np.int32)
        skip[4] = 100 + int(select_topk(prob, masked_idx(idx, mask), 1)[0][4, 0])
        for W in (3, 5):                    # spare words are never read
            bits = mask_to_bits(mask, W)
            assert np.array_equal(bits_to_mask(bits, C_), mask) and not bits[:, 3:].any()
            absent = torch.from_numpy(bits.view(np.int32))
            assert np.array_equal(absent_columns(absent, C_).numpy(), mask)
            got = TGN.topk_scores(cpu, eq, ec, K, cand_idx=ix, skip=torch.from_numpy(skip), idx_base=100, absent=absent)
            wi, wp = select_topk(prob, masked_idx(idx, mask), K, skip=skip, idx_base=100)
            assert np.array_equal(got[0].numpy(), wi) and np.array_equal(got[1].numpy().view(np.uint32), wp.view(np.uint32))
            assert (wi[2] == -1).all() and not wp[2].any()
        plain = TGN.topk_scores(cpu, eq, ec, K, cand_idx=ix)
        none = TGN.topk_scores(cpu, eq, ec, K, cand_idx=ix, absent=torch.zeros((Q, 3), dtype=torch.int32))
        assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
        for bad in (torch.zeros((Q, 2), dtype=torch.int32), torch.zeros((Q + 1, 3), dtype=torch.int32),
                    torch.zeros((Q, 3), dtype=torch.int64)):
            with pytest.raises(ValueError, match="absent"):
                TGN.topk_scores(cpu, eq, ec, K, cand_idx=ix, absent=bad)


# ---- the restatements ----------------------------------------------------------------------------------------------------
def test_seen_restatement_agrees_with_find_before():
    """helpers_filtered's adjacency and seen_ranges against NeighborFinder.find_before (host arrays alone: the finder is given
    the adjacency without a device handle), on the stream of the model-level tests: it has timestamp ties, also inside one
    node's entries, and queries AT an entry's timestamp"""
    from zebra_amd.tppr import NeighborFinder
    src, dst, _, ts, _ = I.make_stream("general", 80, 250, 61)
    N = int(max(src.max(), dst.max())) + 1
    assert len(ts) - len(np.unique(ts)) >= 10                                 # ties in the stream
    indptr, nbr, ats = adjacency(src, dst, ts, N)
    assert indptr[-1] == 2 * len(src) and all((np.diff(ats[indptr[v]:indptr[v + 1]]) >= 0).all() for v in range(N))
    nf = NeighborFinder.__new__(NeighborFinder)
    nf.num_nodes, nf._indptr, nf._nbr, nf._ts = N, indptr, nbr, ats
    nf._eid = np.zeros(len(nbr), np.int32)
    tied_inside = 0
    nodes, times = [], []
    for v in range(N):
        own = ats[indptr[v]:indptr[v + 1]]
        tied_inside += len(own) - len(np.unique(own))
        for t in list(np.unique(own)) + [own.min() - 1 if len(own) else 0.0, own.max() + 1 if len(own) else 1.0]:
            nodes.append(v)
            times.append(float(t))
    assert tied_inside > 0
    begin, length = seen_ranges(indptr, ats, np.array(nodes), np.array(times))
    for q, (v, t) in enumerate(zip(nodes, times)):
        want = nf.find_before(v, t)[0]
        assert begin[q] == indptr[v] and np.array_equal(nbr[begin[q]:begin[q] + length[q]], want), (v, t)
        assert t not in ats[begin[q]:begin[q] + length[q]]                    # an entry AT t is not seen
    assert seen_ranges(indptr, ats, np.array([-1, N]), np.array([1e9, 1e9]))[1].tolist() == [0, 0]


def test_mark_bits_on_hand_made_lists():
    ids = np.array([7, 3, 3, 99, -1, 0, 5], np.int32)
    begin, length = np.array([0, 4, 7]), np.array([4, 3, 0])
    # range: ids 3 .. 8 are columns 0 .. 5
    b = mark_bits(ids, begin, length, 6, 2, id_lo=3)
    assert b.tolist() == [[0b10001, 0], [0b100, 0], [0, 0]]
    # a shared list with a repeat and a -1 entry: every column of an excluded id; -1 never matches the list's -1
    cand = np.array([3, -1, 7, 3, 5, 0], np.int32)
    b = mark_bits(ids, begin, length, 6, 1, cand=cand)
    assert b.tolist() == [[0b001101], [0b110000], [0]]
    per = np.stack([cand, cand[::-1], cand])
    b = mark_bits(ids, begin, length, 6, 1, cand=per)
    assert b.tolist() == [[0b001101], [0b000011], [0]]
    assert bits_to_mask(mask_to_bits(np.eye(3, 40, 33, dtype=bool)), 40)[1, 34]
