"""The negative sampler without a GPU: Philox4x32-10 against Random123's known answers, the numpy restatement of
zt_neg_sample's rule (tests/helpers_negsample.py) held to the rule's own invariants on every case of the table, what each case
reaches shown from its trace, zt_neg_sample_plan's table and the argument errors, which return before any device call."""
import ctypes as C

import numpy as np
import pytest

import helpers_negsample as H
from helpers_negsample import ALL, CASES, DISTINCT, EXCLUDE_SOURCE, FILTER, REACHES, case_expected, case_inputs, sample_rows


def test_philox_known_answers():
    hexes = lambda words: " ".join("%08x" % int(w) for w in words)
    assert hexes(H.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes(H.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexes(H.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) \
        == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays of counters give the scalar answers element by element
    got = H.philox4x32_10((np.array([0, 0xffffffff]), np.array([0, 0xffffffff]), np.array([0, 0xffffffff]),
                           np.array([0, 0xffffffff])), (np.array([0, 0xffffffff]), np.array([0, 0xffffffff])))
    assert [int(w[0]) for w in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w[1]) for w in got] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # the rule's counter and key: (row lo, row hi, slot, round) and (seed lo, seed hi)
    row, seed = (0x85a308d3 << 32) | 0x243f6a88, (0x299f31d0 << 32) | 0xa4093822
    assert H.draw_words(seed, row, [0x13198a2e], 0x03707344) == [0xd16cfe09]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_keeps_the_rules_invariants(name):
    a = case_inputs(name)
    neg, count, tr = case_expected(name)
    assert neg.shape == (a.rows, a.K) and neg.dtype == np.int32 and count.shape == (a.rows, 2)
    pool = set(a.pool.tolist())
    for q in range(a.rows):
        b, n = (0, 0) if a.ids is None else H.clip_range(a.begin[q], a.length[q], a.n_ids)
        members = set(int(v) for v in a.ids[b:b + n] if v >= 0) if n else set()
        live = neg[q] >= 0
        got = neg[q][live].tolist()
        assert int(a.dst[q]) not in got and (neg[q][~live] == -1).all()
        if a.flags & EXCLUDE_SOURCE:
            assert int(a.src[q]) not in got
        kind = tr["kind"][q]
        assert ((kind > 0) == live).all() and ((tr["round"][q] >= 0) == live).all()
        from_pool, from_list = neg[q][kind == 2].tolist(), neg[q][kind == 1].tolist()
        assert all(v in pool for v in from_pool) and all(v in members for v in from_list)
        if a.flags & FILTER:
            assert not any(v in members for v in from_pool)
        if a.flags & DISTINCT:
            assert len(set(got)) == len(got)
        assert count[q].tolist() == [len(from_list), len(from_pool)]
        assert not (kind[a.K_hist:] == 1).any()                            # a pool slot never reads the list
        assert (tr["round"][q] < a.rounds).all()


def test_split_invariance():
    """Q = 10 at row_base = 100 equals rows 100 .. 103 followed by rows 104 .. 109"""
    a = case_inputs("K65")
    args = lambda lo, hi: dict(src=a.src[lo:hi], dst=a.dst[lo:hi], pool=a.pool, ids=a.ids, begin=a.begin[lo:hi],
                               length=a.length[lo:hi], n_ids=a.n_ids)
    desc = (a.K, a.K_hist, a.rounds, a.hist_rounds, a.flags)
    whole = sample_rows(a.seed, 100, *desc, **args(0, 10))
    head = sample_rows(a.seed, 100, *desc, **args(0, 4))
    tail = sample_rows(a.seed, 104, *desc, **args(4, 10))
    assert np.array_equal(whole[0], np.concatenate([head[0], tail[0]])) and np.array_equal(whole[1], np.concatenate([head[1], tail[1]]))
    moved = sample_rows(a.seed, 101, *desc, **args(0, 10))             # another base: other draws
    assert not np.array_equal(whole[0], moved[0])
    reseeded = sample_rows(a.seed + 1, 100, *desc, **args(0, 10))
    assert not np.array_equal(whole[0], reseeded[0])


@pytest.mark.parametrize("name", sorted(REACHES))
def test_case_reaches_what_its_id_names(name):
    a = case_inputs(name)
    neg, count, tr = case_expected(name)
    total = lambda rule: sum(r[rule] for r in tr["rejects"])
    what = REACHES[name]
    if what == "last_round_accept":
        assert a.rounds == 8 and (tr["round"] == a.rounds - 1).any()
    elif what == "same_round":
        assert total("same_round") > 0
    elif what == "earlier":
        assert total("earlier") > 0
    elif what == "filter":
        assert total("filter") > 0
    elif what == "ends_empty":
        assert ((neg < 0).any(axis=1)).any() and (neg >= 0).any()
    elif what == "hist_slot_from_pool":
        assert a.K_hist > 0 and (tr["kind"][:, :a.K_hist] == 2).any() and (tr["kind"][:, :a.K_hist] == 1).any()
    else:
        raise AssertionError(what)


def test_named_cases_are_what_they_say():
    w = H.world()
    # the histories' lengths, with duplicate partners
    a = case_inputs("K65")
    assert a.length[:8].tolist() == [0, 1, 255, 256, 257, 1000, 500, int(np.diff(w.indptr)[a.src[7]])]
    for q in (2, 3, 4, 5):
        lst = a.ids[a.begin[q]:a.begin[q] + a.length[q]]
        assert len(set(lst.tolist())) < len(lst)
    assert a.dst[3] == H.OUTSIDE and H.OUTSIDE not in a.pool and int(a.src[7]) in a.pool
    assert any(int(a.dst[q]) in set(a.ids[a.begin[q]:a.begin[q] + a.length[q]].tolist()) for q in range(a.rows))
    # the full cases hold no -1 at all
    for name in ("full-random", "full-mixed", "full-historical"):
        assert (case_expected(name)[0] >= 0).all(), name
    assert case_expected("full-random")[1][:, 0].sum() == 0 and case_expected("full-mixed")[1][:, 0].sum() > 0
    # a list that covers the whole pool under FILTER: every slot of such a row is -1
    for name in ("covered-pool", "covered-pool-undistinct"):
        a = case_inputs(name)
        neg, count, _ = case_expected(name)
        rows = [q for q in range(a.rows) if a.src[q] == 6 and a.ts[q] == w.t_end]
        assert len(rows) >= 3
        for q in rows:
            assert set(a.pool.tolist()) <= set(a.ids[a.begin[q]:a.begin[q] + a.length[q]].tolist())
            assert (neg[q] == -1).all() and count[q].tolist() == [0, 0]
        assert (neg >= 0).any()
    # a pool of 40 and K = 32: rows collide (duplicates rejected) and run dry
    a = case_inputs("dry-pool40-K32")
    assert len(a.pool) == 40 and a.K == 32 and (case_expected("dry-pool40-K32")[0] < 0).any()
    # the source flag: with it off the source of row 7, a pool member, is drawn; with it on it never is
    off, on = case_expected("source-off-pool40")[0], case_expected("source-on-pool40")[0]
    src7 = int(case_inputs("source-off-pool40").src[7])
    assert src7 in off[7].tolist() and src7 not in on[7].tolist() and sum(r["source"] for r in case_expected("source-on-pool40")[2]["rejects"]) > 0
    # the caller's lists hold negative ids, and historical slots draw them
    a = case_inputs("own-lists-negative")
    assert (a.ids < 0).any() and a.n_ids is None and sum(r["negative"] for r in case_expected("own-lists-negative")[2]["rejects"]) > 0
    # clipped ranges: three entries left, none, a negative begin, a negative length, a begin beyond the array
    a = case_inputs("clipped")
    assert [H.clip_range(a.begin[q], a.length[q], a.n_ids)[1] for q in range(5)] == [3, 0, 0, 0, 0]
    assert case_expected("clipped")[1][0, 0] > 0
    # without flags nothing but the destination is rejected
    rej = case_expected("flags-none")[2]["rejects"]
    assert all(r[k] == 0 for r in rej for k in r if k != "destination") and (case_expected("flags-none")[0] >= 0).all()


def test_pool_draws_are_uniform():
    """50 000 pool draws over 50 ids at a fixed seed: chi-square with 49 degrees of freedom, bound 85.4 (p = 0.001)"""
    n_pool, rows, slots = 50, 50, 1000
    counts = np.zeros(n_pool, np.int64)
    for row in range(rows):
        x = np.array(H.draw_words(20221, row, np.arange(slots), 0), np.uint64)
        counts += np.bincount(((x * np.uint64(n_pool)) >> np.uint64(32)).astype(np.int64), minlength=n_pool)
    assert counts.sum() == 50000
    expected = counts.sum() / n_pool
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print("chi-square over 50 ids:", chi2)
    assert chi2 < 85.4
    # ... and the restatement's unflagged pool rows are those draws
    pool = np.arange(1000, 1050, dtype=np.int32)
    neg, _ = sample_rows(20221, 0, slots, 0, 1, 0, 0, np.zeros(2, np.int32), np.zeros(2, np.int32), pool)
    x = np.array(H.draw_words(20221, 1, np.arange(slots), 0), np.uint64)
    assert np.array_equal(neg[1], pool[((x * np.uint64(50)) >> np.uint64(32)).astype(np.int64)])


def test_plan_table():
    from zebra_amd import _capi
    want = {1: (1, 64, 64), 63: (1, 64, 64), 64: (1, 64, 64), 65: (1, 64, 128), 128: (1, 64, 128), 129: (2, 256, 256),
            256: (2, 256, 256), 257: (2, 256, 512), 1000: (2, 256, 1024), 1024: (2, 256, 1024), 1025: (2, 1024, 2048),
            2048: (2, 1024, 2048), 2049: (2, 1024, 4096), 4096: (2, 1024, 4096)}
    for K, (form, threads, n2) in want.items():
        p = _capi.neg_sample_plan(K)
        assert (p["form"], p["threads"], p["n2"]) == (form, threads, n2), K
        assert p["lds_bytes"] == 14 * n2 + 16 and p["lds_bytes"] <= 64 * 1024 and p["n2"] >= K
    for K in (0, -1, 4097, 2 ** 31 - 1):                                    # refused in field 0, not failed
        assert _capi.neg_sample_plan(K) == dict(form=0, threads=0, n2=0, lds_bytes=0)
    assert _capi.lib().zt_neg_sample_plan(C.c_int32(5), None) == _capi.ZT_ERR_ARG
    assert _capi.NEG_MAX_K == 4096 and _capi.NEG_MAX_ROUNDS == 8
    assert (_capi.NEG_FILTER, _capi.NEG_DISTINCT, _capi.NEG_EXCLUDE_SOURCE) == (FILTER, DISTINCT, EXCLUDE_SOURCE)
    # every K of the table's seam cases is a seam of the plan or beside one
    assert {64, 65, 128, 129, 1024, 1025, 4096} <= set(H.K_SEAMS)


def test_bad_arguments_fail_without_a_device():
    """every ZT_ERR_ARG of zt_neg_sample returns before any device call (host addresses stand in for the device pointers:
    none is read)"""
    from zebra_amd import _capi
    lib = _capi.lib()
    buf = np.zeros(64, np.int64)
    p = _capi.ptr(buf)

    def call(d=True, src=p, dst=p, Q=4, pool=p, n_pool=10, c=None, ids=None, begin=None, length=None, neg=p, **desc):
        f = dict(seed=1, row_base=0, K=8, K_hist=4, rounds=4, hist_rounds=2, flags=ALL)
        f.update(desc)
        nd = _capi.NegDesc(**f)
        return lib.zt_neg_sample(C.byref(nd) if d else None, src, dst, C.c_int64(Q), pool, C.c_int64(n_pool), c, ids, begin,
                                 length, neg, None, None)

    bad = [dict(d=False), dict(src=None), dict(dst=None), dict(pool=None), dict(neg=None), dict(Q=-1), dict(n_pool=0),
           dict(n_pool=-3), dict(K=0), dict(K=4097), dict(K=-1), dict(K_hist=-1), dict(K_hist=9), dict(rounds=0), dict(rounds=9),
           dict(hist_rounds=-1), dict(hist_rounds=5), dict(flags=8), dict(flags=-1), dict(begin=p, ids=p), dict(length=p, ids=p),
           dict(begin=p, length=p)]
    for kw in bad:
        assert call(**kw) == _capi.ZT_ERR_ARG, kw
        assert b"zt_neg_sample" in lib.zt_last_error()
    assert call(n_pool=2 ** 31) == _capi.ZT_ERR_UNSUPPORTED
    # Q = 0: ZT_OK, nothing touched -- also with an empty pool
    assert call(Q=0) == _capi.ZT_OK and call(Q=0, n_pool=0) == _capi.ZT_OK and not buf.any()
    with pytest.raises(ValueError):
        _capi.check(call(K=0), "zt_neg_sample")


def test_sampler_object_refuses_what_it_cannot_draw():
    """the Python layer's own checks, which come before any device call (the pool goes to the device in __init__: only what
    fails before that is checked here)"""
    from zebra_amd.sampling import NegativeSampler
    import zebra_amd
    assert zebra_amd.NegativeSampler is NegativeSampler
    for kw in (dict(strategy="popular"), dict(hist_ratio=1.5), dict(rounds=0), dict(rounds=9)):
        with pytest.raises(ValueError):
            NegativeSampler(np.arange(5), 3, **kw)
    with pytest.raises(ValueError):
        NegativeSampler(np.arange(5), None)
    with pytest.raises(ValueError):
        NegativeSampler(np.zeros(0, np.int32), 3)
