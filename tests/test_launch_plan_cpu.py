"""CPU-side pin of the embedding's kernel choice (zt::embed_kernel_plan, csrc/aggregate.hip; through the test hook
zt_test_embed_plan).  Every kernel of a family gives the same bits, so the GPU suite cannot tell a shape sent to the wrong
kernel; this table can.  Each row is the kernel the shape took before the choice moved into one function, read off the
predicates of embed_impl / zt_agg_train_forward as they were:
  tab    = a projected table is given and its [ef | time] tile holds a query row (mt2 > 0)
  split  = no tab and no [memory | ef | time] tile holds a query row (mt = 0); refused where no 16-row chunk fits either
  wide   = tab, D = T = 100, F = 172, k in {20, 40}                       (not under ZT_AGG_GENERIC)
  reg    = tab, D = T = 100, F <= 4 (K2p = 112), k in {20, 40}            (not under ZT_AGG_GENERIC)
  d100   = tab, D = T = 100, mt2 = 5, k in {10, 20, 40}                   (not under ZT_AGG_GENERIC)
  then the tiled kernel over the table's tile or the full one, the MAX_MT_BIG instantiation for k > 80.
  training: the full tile for k <= 80 where it fits, else the row split.
  output layers: latency where D % 4 == 0, Dp in {112, 128} and (ZT_OUT_LATENCY, or no choice and N <= 1024); else persist
  where Dp = 112 and (ZT_OUT_PERSIST, or no choice and N >= 8192); else tiled."""
import ctypes as C

import pytest

AGG = {"unsupported": 0, "reg": 1, "wide": 2, "d100": 3, "tiled_table": 4, "tiled_full": 5, "tiled_table_big": 6,
       "tiled_full_big": 7, "split": 8}
OUT = {"tiled": 0, "latency": 1, "persist": 2}
GENERIC = 1                                      # ZT_AGG_GENERIC
TILED, LATENCY, PERSIST = 1, 2, 3                # ZT_OUT_*


@pytest.fixture(scope="module")
def hooks():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi.hooks_lib()


def plan(hooks, N, D, F, T, M, k, table, training=False, agg_choice=0, out_choice=0):
    a, o, lds = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    rc = hooks.zt_test_embed_plan(C.c_int64(N), C.c_int32(D), C.c_int32(F), C.c_int32(T), C.c_int32(M), C.c_int32(k),
                                  C.c_int32(int(table)), C.c_int32(int(training)), C.c_int32(agg_choice),
                                  C.c_int32(out_choice), C.byref(a), C.byref(o), C.byref(lds))
    assert rc == 0
    return a.value, o.value, lds.value


# (N, D, F, T, M, k, table, ZT_CHOICE_AGGREGATE, ZT_CHOICE_EMBED_OUT) -> (aggregation, output layers, LDS of the tiled launch)
EVAL = [
    # BASELINE C1 - C3 (Wikipedia / Reddit widths: F = 172, k = 20; N = 3 bs), with the projected table and without
    ((600, 100, 172, 100, 1, 20, True, 0, 0), ("wide", "latency", 0)),
    ((600, 100, 172, 100, 1, 20, False, 0, 0), ("tiled_full", "latency", 125840)),
    ((600, 100, 172, 100, 2, 20, True, 0, 0), ("wide", "latency", 0)),
    ((600, 100, 172, 100, 2, 20, False, 0, 0), ("tiled_full", "latency", 125840)),
    ((1800, 100, 172, 100, 2, 20, True, 0, 0), ("wide", "tiled", 0)),
    ((1800, 100, 172, 100, 2, 20, False, 0, 0), ("tiled_full", "tiled", 125840)),
    # C4 (k = 40) and C5 (12 288 rows): F <= 4
    ((3000, 100, 1, 100, 2, 40, True, 0, 0), ("reg", "tiled", 0)),
    ((3000, 100, 1, 100, 2, 40, False, 0, 0), ("tiled_full", "tiled", 69520)),
    ((12288, 100, 1, 100, 2, 20, True, 0, 0), ("reg", "persist", 0)),
    ((12288, 100, 1, 100, 2, 20, False, 0, 0), ("tiled_full", "persist", 69520)),
    # k = 10: d100 (mt2 = 5) where the table is given
    ((600, 100, 172, 100, 2, 10, True, 0, 0), ("d100", "latency", 90000)),
    ((600, 100, 1, 100, 2, 10, True, 0, 0), ("d100", "latency", 38800)),
    ((600, 100, 1, 100, 2, 10, False, 0, 0), ("tiled_full", "latency", 69520)),
    # ZT_AGG_GENERIC: the tiled kernel over the table's tile instead of wide / reg / d100
    ((600, 100, 172, 100, 2, 20, True, GENERIC, 0), ("tiled_table", "latency", 90000)),
    ((12288, 100, 1, 100, 2, 20, True, GENERIC, 0), ("tiled_table", "persist", 38800)),
    ((3000, 100, 1, 100, 2, 40, True, GENERIC, 0), ("tiled_table", "tiled", 38800)),
    ((600, 100, 1, 100, 2, 10, True, GENERIC, 0), ("tiled_table", "latency", 38800)),
    # 80 < k at F = 1: the big tile; at k = 255 the full one no longer fits and the row split takes it
    ((600, 100, 1, 100, 2, 81, True, 0, 0), ("tiled_table_big", "latency", 123280)),
    ((600, 100, 1, 100, 2, 81, False, 0, 0), ("tiled_full_big", "latency", 152464)),
    ((600, 100, 1, 100, 2, 100, True, 0, 0), ("tiled_table_big", "latency", 100240)),
    ((600, 100, 1, 100, 2, 100, False, 0, 0), ("tiled_full_big", "latency", 97168)),
    ((600, 100, 1, 100, 2, 255, True, 0, 0), ("tiled_table_big", "latency", 123280)),
    ((600, 100, 1, 100, 2, 255, False, 0, 0), ("split", "latency", 0)),
    # F = 172 past one tile: no tile holds a query row, with or without the table
    ((600, 100, 172, 100, 2, 136, True, 0, 0), ("split", "latency", 0)),
    ((600, 100, 172, 100, 2, 136, False, 0, 0), ("split", "latency", 0)),
    ((600, 100, 172, 100, 2, 137, True, 0, 0), ("split", "latency", 0)),
    ((600, 100, 172, 100, 2, 137, False, 0, 0), ("split", "latency", 0)),
    ((600, 100, 172, 100, 2, 160, True, 0, 0), ("split", "latency", 0)),
    ((600, 100, 172, 100, 2, 160, False, 0, 0), ("split", "latency", 0)),
    ((600, 100, 172, 100, 2, 255, True, 0, 0), ("split", "latency", 0)),
    ((600, 100, 172, 100, 2, 255, False, 0, 0), ("split", "latency", 0)),
    # D = 128: the table's tile cannot stage the hidden rows (K2p < Dp + 1); Dp = 128 has no persistent form
    ((1024, 128, 1, 100, 2, 20, True, 0, 0), ("tiled_full", "latency", 79760)),
    ((8192, 128, 1, 100, 2, 20, True, 0, 0), ("tiled_full", "tiled", 79760)),
    # partial-sum groups (k = 40: hg = 10) in the latency and persistent forms
    ((1024, 100, 172, 100, 2, 40, True, 0, 0), ("wide", "latency", 0)),
    ((8192, 100, 172, 100, 2, 40, True, 0, 0), ("wide", "persist", 0)),
    # widths the fast output layers do not take: Dp = 64; D % 4 != 0
    ((8192, 64, 1, 100, 2, 20, True, 0, 0), ("tiled_table", "tiled", 38800)),
    ((1024, 98, 1, 100, 2, 20, True, 0, 0), ("tiled_table", "tiled", 38800)),
]
# the output layers around the two switch points, under each ZT_CHOICE_EMBED_OUT value (C5's widths, table given: reg)
for _N, _want in [(1024, ("latency", "tiled", "latency", "persist")), (1025, ("tiled", "tiled", "latency", "persist")),
                  (8191, ("tiled", "tiled", "latency", "persist")), (8192, ("persist", "tiled", "latency", "persist"))]:
    for _oc, _o in zip((0, TILED, LATENCY, PERSIST), _want):
        EVAL.append(((_N, 100, 1, 100, 2, 20, True, 0, _oc), ("reg", _o, 0)))


@pytest.mark.parametrize("shape,want", EVAL, ids=[str(s) for s, _ in EVAL])
def test_embed_kernel_choice(hooks, shape, want):
    N, D, F, T, M, k, table, ac, oc = shape
    assert plan(hooks, N, D, F, T, M, k, table, agg_choice=ac, out_choice=oc) == (AGG[want[0]], OUT[want[1]], want[2])


@pytest.mark.parametrize("shape", [(600, 100, 172, 100, 2, 256, True), (600, 100, 172, 100, 2, 256, False),
                                   (600, 129, 172, 100, 2, 20, True), (600, 129, 1, 100, 2, 20, False)])
def test_embed_refuses_what_no_kernel_takes(hooks, shape):
    """k beyond ZT_MAX_K_WIDE; D > 128"""
    assert plan(hooks, *shape)[0] == AGG["unsupported"]


# zt_agg_train_forward: (D, F, T, k) at N = 600, M = 2 -> (aggregation, LDS)
TRAIN = [
    ((100, 1, 100, 20), ("tiled_full", 69520)),
    ((100, 1, 100, 80), ("tiled_full", 69520)),
    ((100, 1, 100, 81), ("split", 0)),
    ((100, 1, 100, 100), ("split", 0)),
    ((100, 1, 100, 255), ("split", 0)),
    ((100, 172, 100, 20), ("tiled_full", 125840)),
    ((100, 172, 100, 40), ("tiled_full", 125840)),
    ((100, 172, 100, 100), ("split", 0)),
    ((100, 172, 100, 136), ("split", 0)),
    ((100, 172, 100, 137), ("split", 0)),
    ((100, 172, 100, 255), ("split", 0)),
    ((100, 172, 100, 256), ("unsupported", 0)),
    ((100, 1, 100, 256), ("unsupported", 0)),
    ((129, 1, 100, 20), ("unsupported", 0)),
]


@pytest.mark.parametrize("shape,want", TRAIN, ids=[str(s) for s, _ in TRAIN])
def test_train_forward_kernel_choice(hooks, shape, want):
    D, F, T, k = shape
    for table in (False, True):                   # (the training forward has no table)
        a, _, lds = plan(hooks, 600, D, F, T, 2, k, table, training=True)
        assert (a, lds) == (AGG[want[0]], want[1])
