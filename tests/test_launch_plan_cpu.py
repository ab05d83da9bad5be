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


# ---------------------------------------------------------------------------------------------------------------------
# The memory update (zt::memory_kernel_plan, csrc/memory_update.hip; through the test hook zt_test_memory_plan).  Each row is
# the kernel the shape took before the choice moved into one function, read off the predicates of gru_update_ex and
# store_messages_ex as they were (Xp, Hp = msg, D rounded up to 16; rows = the ids given to the update):
#   refused: D <= 0 or msg <= 0 (bad argument), then D > 128, then -- only where rows > 0 -- a message too wide for
#            k_gru<2>'s two 16-row tiles of [message | memory] in 150 KB of LDS: 2 * 16 * (Xp + Hp + 4) * 4 + 128 > 153 600
#   fits  = rows <= 8192 and (Xp + Hp) / 16 <= 40 and 16 (msg + D) <= 37 * 256 and 16 Hp <= 7 * 256
#           (the chunk bound never decides alone: the staging bound fails from 39 chunks on)
#   split = fits and (ZT_GRU_SPLIT, or no choice and rows <= 512); else the tile
#   held-back output layers over the table updated: fused with the tile where they are tiled with hg in {1, 5, 10}; fused with
#           the split where they are latency-organised, hg in {1, 5, 10}, their N-tiles are the GRU's and NTg in {7, 8};
#           in front of the GRU kernel otherwise (and on the way out of a refused or empty update)
#   messages: two positions per wave unless ZT_MSG_ONE, D > 128, T > 128 or F > 256
REFUSAL = {"none": 0, "arg": 1, "d_large": 2, "msg_wide": 3}
MSGK = {"one": 0, "two": 1}
GRU = {"none": 0, "tile": 1, "split": 2}
HELD = {"none": 0, "front": 1, "fused_tile": 2, "fused_split": 3}
GRU_TILE, GRU_SPLIT = 1, 2                       # ZT_GRU_*
MSG_ONE, MSG_TWO = 1, 2                          # ZT_MSG_*


def memory_plan(hooks, rows, D, msg, F=172, T=100, gru_choice=0, msg_choice=0, held=None):
    """held: (form, hg, D, M, gx, N, same memory) of output layers held back by embed_ex, or None"""
    form, hg, hD, hM, gx, hN, same = held if held else ("tiled", 0, 0, 0, 0, 0, False)
    out = (C.c_int64 * 14)(*([-1] * 14))
    rc = hooks.zt_test_memory_plan(C.c_int64(rows), C.c_int32(D), C.c_int32(msg), C.c_int32(F), C.c_int32(T),
                                   C.c_int32(gru_choice), C.c_int32(msg_choice), C.c_int32(int(held is not None)),
                                   C.c_int32(OUT[form]), C.c_int32(hg), C.c_int32(hD), C.c_int32(hM), C.c_int32(gx),
                                   C.c_int64(hN), C.c_int32(int(same)), out)
    assert rc == 0
    keys = ("refusal", "msg", "gru", "out", "lds", "lds2", "lds_f", "gru_tiles", "NTg", "n_src_wgs", "n_nb_wgs",
            "out_tiles", "target", "participants")
    return dict(zip(keys, list(out)))


# (rows, D, msg, ZT_CHOICE_GRU) -> (form, dynamic LDS of its launch, 16-row tiles, N-tiles)
GRU_ROWS = [
    # BASELINE C2 - C5 (D = 100; messages 2 D + F + T: F = 172 for C2 / C3, 1 for C4 / C5)
    ((400, 100, 472, 0), ("split", 54656, 25, 7)),
    ((1200, 100, 472, 0), ("tile", 38272, 75, 7)),
    ((2000, 100, 301, 0), ("tile", 27008, 125, 7)),
    ((8192, 100, 301, 0), ("tile", 27008, 512, 7)),
    # the row switch
    ((512, 100, 472, 0), ("split", 54656, 32, 7)),
    ((513, 100, 472, 0), ("tile", 38272, 33, 7)),
    # the split pinned: up to GS_MAX_ROWS, beyond it the tile
    ((8192, 100, 301, GRU_SPLIT), ("split", 43392, 512, 7)),
    ((8193, 100, 301, GRU_SPLIT), ("tile", 27008, 513, 7)),
    ((1200, 100, 472, GRU_SPLIT), ("split", 54656, 75, 7)),
    # the tile pinned
    ((400, 100, 472, GRU_TILE), ("tile", 38272, 25, 7)),
    # the staging bound 16 (msg + D) <= 37 * 256
    ((400, 100, 492, 0), ("split", 55680, 25, 7)),
    ((400, 100, 493, 0), ("tile", 39296, 25, 7)),
    # the chunk bound: 38 chunks fit, 39 do not (there the staging bound fails)
    ((400, 1, 577, 0), ("split", 55680, 25, 1)),
    ((400, 1, 593, 0), ("tile", 40320, 25, 1)),
    # 16 Hp <= 7 * 256: D = 112 against 113, also pinned (the split that does not fit falls back)
    ((400, 112, 100, 0), ("split", 31104, 25, 7)),
    ((400, 113, 100, 0), ("tile", 15744, 25, 8)),
    ((400, 113, 100, GRU_SPLIT), ("tile", 15744, 25, 8)),
    # the widest messages taken (D = 100: 1 072; D = 128: 1 056)
    ((400, 100, 1072, 0), ("tile", 76160, 25, 7)),
    ((400, 100, 1072, GRU_SPLIT), ("tile", 76160, 25, 7)),
    ((400, 128, 1056, 0), ("tile", 76160, 25, 8)),
    ((400, 64, 236, 0), ("split", 36224, 25, 4)),
]


@pytest.mark.parametrize("shape,want", GRU_ROWS, ids=[str(s) for s, _ in GRU_ROWS])
def test_gru_kernel_choice(hooks, shape, want):
    rows, D, msg, gc = shape
    p = memory_plan(hooks, rows, D, msg, gru_choice=gc)
    assert (p["refusal"], p["out"]) == (REFUSAL["none"], HELD["none"])
    lds = p["lds2"] if want[0] == "split" else p["lds"]
    assert (p["gru"], lds, p["gru_tiles"], p["NTg"]) == (GRU[want[0]], want[1], want[2], want[3])


# (rows, D, msg) -> refusal; nothing is launched
REFUSED = [
    ((400, 100, 1073), "msg_wide"),
    ((400, 128, 1057), "msg_wide"),
    ((400, 129, 472), "d_large"),
    ((0, 129, 472), "d_large"),
    ((400, 0, 472), "arg"),
    ((400, 100, 0), "arg"),
    ((0, 100, 2000), "none"),          # no rows: nothing to do, whatever the message width
]


@pytest.mark.parametrize("shape,want", REFUSED, ids=[str(s) for s, _ in REFUSED])
def test_gru_refusals(hooks, shape, want):
    p = memory_plan(hooks, *shape)
    assert (p["refusal"], p["gru"]) == (REFUSAL[want], GRU["none"])


# (D, F, T, ZT_CHOICE_MESSAGES) -> positions per wave
MESSAGES = [
    ((100, 172, 100, 0), "two"),
    ((100, 1, 100, 0), "two"),
    ((128, 172, 100, 0), "two"),
    ((129, 172, 100, 0), "one"),
    ((100, 172, 128, 0), "two"),
    ((100, 172, 129, 0), "one"),
    ((100, 256, 100, 0), "two"),
    ((100, 257, 100, 0), "one"),
    ((100, 172, 100, MSG_ONE), "one"),
    ((100, 172, 100, MSG_TWO), "two"),
    ((129, 172, 100, MSG_TWO), "one"),
]


@pytest.mark.parametrize("shape,want", MESSAGES, ids=[str(s) for s, _ in MESSAGES])
def test_message_kernel_choice(hooks, shape, want):
    D, F, T, mc = shape
    assert memory_plan(hooks, 400, D, 2 * D + F + T, F=F, T=T, msg_choice=mc)["msg"] == MSGK[want]


# (rows, D, msg, ZT_CHOICE_GRU, held: (form, hg, D, M, gx, N, same memory)) ->
#   (output layers, lds_f, n_src_wgs, n_nb_wgs, out_tiles, gate target, gate participants)
FRONT = ("front", 0, 0, 0, 0, 0, 0)
FUSE = [
    # C2: the split beside latency-organised output layers, hg = 1, 5, 10 (gx = 38 tiles per path)
    ((400, 100, 472, 0, ("latency", 1, 100, 2, 38, 600, True)), ("fused_split", 54656, 67, 133, 0, 266, 441)),
    ((400, 100, 472, 0, ("latency", 5, 100, 2, 38, 600, True)), ("fused_split", 54656, 67, 133, 0, 266, 441)),
    ((400, 100, 472, 0, ("latency", 10, 100, 2, 38, 600, True)), ("fused_split", 54656, 67, 133, 0, 266, 441)),
    ((400, 100, 472, 0, ("latency", 2, 100, 2, 38, 600, True)), FRONT),
    ((400, 100, 472, 0, ("latency", 1, 100, 2, 38, 600, False)), FRONT),
    ((400, 100, 472, 0, ("tiled", 1, 100, 2, 38, 600, True)), FRONT),
    ((400, 100, 472, 0, ("persist", 1, 100, 2, 38, 600, True)), FRONT),
    ((1200, 100, 472, GRU_SPLIT, ("latency", 5, 100, 2, 38, 1800, True)), ("fused_split", 54656, 67, 133, 0, 266, 791)),
    # NTg: 7 at D = 112 (one model); output layers of other N-tiles; NTg = 4; NTg = 8 never fits the split
    ((400, 112, 100, 0, ("latency", 1, 112, 1, 10, 300, True)), ("fused_split", 31104, 18, 18, 0, 70, 245)),
    ((400, 100, 472, 0, ("latency", 1, 128, 2, 38, 600, True)), FRONT),
    ((400, 64, 236, 0, ("latency", 1, 64, 2, 38, 600, True)), FRONT),
    ((400, 128, 100, 0, ("latency", 1, 128, 2, 38, 600, True)), FRONT),
    # C3 / C4: the tile beside tiled output layers, hg = 1, 5, 10
    ((1200, 100, 472, 0, ("tiled", 1, 100, 2, 0, 1800, True)), ("fused_tile", 38272, 0, 0, 57, 57, 132)),
    ((1200, 100, 472, 0, ("tiled", 5, 100, 2, 0, 1800, True)), ("fused_tile", 38272, 0, 0, 57, 57, 132)),
    ((1200, 100, 472, 0, ("tiled", 10, 100, 2, 0, 1800, True)), ("fused_tile", 38272, 0, 0, 57, 57, 132)),
    ((1200, 100, 472, 0, ("tiled", 2, 100, 2, 0, 1800, True)), FRONT),
    ((1200, 100, 472, 0, ("tiled", 1, 100, 2, 0, 1800, False)), FRONT),
    ((1200, 100, 472, 0, ("latency", 1, 100, 2, 38, 1800, True)), FRONT),
    ((2000, 100, 301, 0, ("tiled", 10, 128, 2, 0, 3000, True)), ("fused_tile", 33920, 0, 0, 94, 94, 219)),
    ((400, 100, 472, GRU_TILE, ("tiled", 1, 100, 2, 0, 600, True)), ("fused_tile", 38272, 0, 0, 19, 19, 44)),
    # C5: the persistent output layers are never fused
    ((8192, 100, 301, 0, ("persist", 1, 100, 2, 0, 12288, True)), FRONT),
    # no rows, a refused update: the output layers still run
    ((0, 100, 472, 0, ("tiled", 1, 100, 2, 0, 600, True)), FRONT),
    ((400, 100, 1073, 0, ("tiled", 1, 100, 2, 0, 600, True)), FRONT),
]


@pytest.mark.parametrize("shape,want", FUSE, ids=[str(s) for s, _ in FUSE])
def test_held_back_output_layers(hooks, shape, want):
    rows, D, msg, gc, held = shape
    p = memory_plan(hooks, rows, D, msg, gru_choice=gc, held=held)
    got = (p["out"], p["lds_f"], p["n_src_wgs"], p["n_nb_wgs"], p["out_tiles"], p["target"], p["participants"])
    assert got == (HELD[want[0]],) + want[1:]


# ---------------------------------------------------------------------------------------------------------------------
# One step of the pipeline (zt::pipeline_step_plan / zt::pipeline_group_plan, csrc/pipeline.hip; through the test hooks
# zt_test_step_plan / zt_test_group_plan).  Every gate form releases the same rows, so the GPU suite cannot tell a step that took
# the wrong one, or that added a packet; this table can.  Each row is what the step did before the choice moved into one
# function, read off the predicates of zt_pipeline_step_ahead / make_group as they were (whole = rows [0, 3B); n = row_hi - row_lo):
#   this member's gate: carried  = its slot is released by member and its bit of Slot::tail_gated is set: nothing is enqueued
#                       inside   = by member, masked and whole and 0 < n <= 2048 and no avg_topk: offered to embed_ex
#                       front    = by member otherwise: k_member_gate in front of the aggregation
#                                  (inside / front: behind the slot's `filled` unless the slot was waited for already)
#                       event    = not by member (a group of one, pruning, the release by launch, by launch-full): the main
#                                  stream waits for the launch's event unless the slot was waited for already
#   gather   = streaming and not whole;  k_avg_topk = avg_topk and whole;  scored = n > 0 and scoring and whole;
#   measured = scored and metrics;  late zt_project_memory = proj_table and no padded W_m yet;  exchange = one is attached
#   the GRU update is the main stream's last item = not scored, no late zt_project_memory, no exchange
#   tail offer = that, and whole and n > 0 and not ZT_RELEASE_MEMBER_FRONT and a valid batch follows whose slot exists, is by
#                member and launched, whose bit is not set yet and which does not ride inside ITS aggregation (masked and
#                3 next_B <= 2048 and no avg_topk); behind that slot's `filled` unless it was waited for already
#   make_group: by member = streaming and the release is neither ZT_RELEASE_LAUNCH nor ZT_RELEASE_LAUNCH_FULL (a slot is then
#                released by member where it holds more than one batch); at most min(want, 8) batches, except under
#                ZT_RELEASE_LAUNCH with n_more <= want followers in sight: n_more - 1, at least 1; pruning: always 1
GATE = {"carried": 0, "event": 1, "front": 2, "inside": 3}
MEMBER, LAUNCH, LAUNCH_FULL, MEMBER_FRONT = 1, 2, 3, 4           # ZT_RELEASE_*
STEP_KEYS = ("gate", "wait_filled", "wait_launch", "gather", "avg_topk", "scored", "measured", "gru_is_last", "tail_offer",
             "tail_wait_filled", "late_project", "exchange")
# the batch that follows, as the slots show it in the steady state: in a launched slot released by member, waited for
NEXT = dict(B=1024, in_slot=True, by_member=True, launched=True, waited=True, tail_gated=False)


def step_plan(hooks, streaming=True, masked=True, release=0, B=1024, rows=None, scoring=False, metrics=False, exchange=False,
              avg_topk=False, proj_table=True, wm_ready=True, by_member=True, tail_gated=False, waited=False, nxt=None):
    """rows: (row_lo, row_hi), None = the whole batch; nxt: the batch that follows (NEXT's keys), None = nothing in sight"""
    lo, hi = rows if rows is not None else (0, 3 * B)
    n = nxt or dict(B=0, in_slot=False, by_member=False, launched=False, waited=False, tail_gated=False)
    out = (C.c_int64 * 12)(*([-1] * 12))
    i32 = lambda v: C.c_int32(int(v))
    rc = hooks.zt_test_step_plan(i32(streaming), i32(masked), i32(release), C.c_int64(B), C.c_int64(lo), C.c_int64(hi),
                                 i32(scoring), i32(metrics), i32(exchange), i32(avg_topk), i32(proj_table), i32(wm_ready),
                                 i32(by_member), i32(tail_gated), i32(waited), i32(nxt is not None), C.c_int64(n["B"]),
                                 i32(n["in_slot"]), i32(n["by_member"]), i32(n["launched"]), i32(n["waited"]),
                                 i32(n["tail_gated"]), out)
    assert rc == 0
    return dict(zip(STEP_KEYS, list(out)))


# facts -> (gate form, wait for `filled`, wait for the launch's event).  Only a whole batch qualifies and 3 B is never 2048:
# B = 682 is the largest whole batch of at most 2048 rows (2046), B = 683 the smallest beyond (2049)
GATES = [
    (dict(B=682), ("inside", 1, 0)),
    (dict(B=683), ("front", 1, 0)),
    (dict(B=682, masked=False), ("front", 1, 0)),
    (dict(B=683, masked=False), ("front", 1, 0)),
    (dict(B=200), ("inside", 1, 0)),                                          # C2
    (dict(B=4096), ("front", 1, 0)),                                          # C5
    (dict(B=682, avg_topk=True), ("front", 1, 0)),
    (dict(B=682, rows=(341, 2041)), ("front", 1, 0)),                         # a shard
    (dict(B=682, rows=(0, 2045)), ("front", 1, 0)),
    (dict(B=682, rows=(1, 2046)), ("front", 1, 0)),
    (dict(B=682, rows=(0, 0)), ("front", 1, 0)),                              # n_rows = 0
    (dict(B=682, rows=(2046, 2046)), ("front", 1, 0)),
    (dict(B=682, tail_gated=True), ("carried", 0, 0)),
    (dict(B=4096, tail_gated=True), ("carried", 0, 0)),
    (dict(B=4096, tail_gated=True, waited=True), ("carried", 0, 0)),
    (dict(B=682, waited=True), ("inside", 0, 0)),
    (dict(B=4096, waited=True), ("front", 0, 0)),
    # the release by launch and by launch-full: make_group gives no slot by_member
    (dict(B=682, release=LAUNCH, by_member=False), ("event", 0, 1)),
    (dict(B=682, release=LAUNCH_FULL, by_member=False), ("event", 0, 1)),
    (dict(B=4096, release=LAUNCH, by_member=False, waited=True), ("event", 0, 0)),
    (dict(B=4096, release=LAUNCH_FULL, by_member=False, waited=True), ("event", 0, 0)),
    # ZT_RELEASE_MEMBER_FRONT moves no gate of the step's own
    (dict(B=682, release=MEMBER_FRONT), ("inside", 1, 0)),
    (dict(B=4096, release=MEMBER_FRONT), ("front", 1, 0)),
    (dict(B=4096, release=MEMBER), ("front", 1, 0)),
    # a group of one (a batch nobody queried ahead, group = 1) whatever the release; the tail bit of such a slot is never read
    (dict(B=682, by_member=False), ("event", 0, 1)),
    (dict(B=682, by_member=False, waited=True), ("event", 0, 0)),
    (dict(B=682, by_member=False, tail_gated=True), ("event", 0, 1)),
    (dict(B=4096, by_member=False, masked=False), ("event", 0, 1)),
    # pruning: one batch per query, never by member
    (dict(B=1000, streaming=False, masked=False, by_member=False), ("event", 0, 1)),
    (dict(B=1000, streaming=False, masked=False, by_member=False, rows=(1000, 2000)), ("event", 0, 1)),
]


@pytest.mark.parametrize("facts,want", GATES, ids=[str(f) for f, _ in GATES])
def test_step_gate_form(hooks, facts, want):
    p = step_plan(hooks, **facts)
    assert (p["gate"], p["wait_filled"], p["wait_launch"]) == (GATE[want[0]], want[1], want[2])
    assert p["tail_offer"] == 0 and p["tail_wait_filled"] == 0           # nothing in sight: nothing to carry


# facts -> (gather, k_avg_topk, scored, measured, late zt_project_memory, exchange, the GRU update is the last item)
ITEMS = [
    (dict(), (0, 0, 0, 0, 0, 0, 1)),
    (dict(proj_table=False, wm_ready=False), (0, 0, 0, 0, 0, 0, 1)),
    (dict(wm_ready=False), (0, 0, 0, 0, 1, 0, 0)),                            # the first step: W_m is padded by its aggregation
    (dict(scoring=True), (0, 0, 1, 0, 0, 0, 0)),
    (dict(scoring=True, metrics=True), (0, 0, 1, 1, 0, 0, 0)),
    (dict(metrics=True), (0, 0, 0, 0, 0, 0, 1)),
    (dict(scoring=True, metrics=True, rows=(0, 3071)), (1, 0, 0, 0, 0, 0, 1)),    # a shard is not scored
    (dict(scoring=True, rows=(0, 0)), (1, 0, 0, 0, 0, 0, 1)),
    (dict(avg_topk=True), (0, 1, 0, 0, 0, 0, 1)),
    (dict(avg_topk=True, rows=(0, 1536)), (1, 0, 0, 0, 0, 0, 1)),
    (dict(exchange=True, rows=(1536, 3072)), (1, 0, 0, 0, 0, 1, 0)),
    (dict(exchange=True), (0, 0, 0, 0, 0, 1, 0)),
    (dict(exchange=True, wm_ready=False, rows=(0, 1536)), (1, 0, 0, 0, 1, 1, 0)),
    (dict(streaming=False, by_member=False, rows=(0, 1536)), (0, 0, 0, 0, 0, 0, 1)),   # pruning queries the shard's rows only
    (dict(streaming=False, by_member=False, scoring=True, metrics=True), (0, 0, 1, 1, 0, 0, 0)),
]


@pytest.mark.parametrize("facts,want", ITEMS, ids=[str(f) for f, _ in ITEMS])
def test_step_items(hooks, facts, want):
    p = step_plan(hooks, **facts)
    got = tuple(p[k] for k in ("gather", "avg_topk", "scored", "measured", "late_project", "exchange", "gru_is_last"))
    assert got == want


# facts (the batch that follows: NEXT unless given) -> (the tail gate is offered, behind the next slot's `filled`)
TAIL = [
    (dict(), (1, 0)),                                                         # the case where it is made (C5's steady state)
    (dict(nxt=dict(NEXT, waited=False)), (1, 1)),                             # the first member of a new group
    (dict(B=4096, nxt=dict(NEXT, B=4096)), (1, 0)),
    (dict(masked=False, B=20, nxt=dict(NEXT, B=20)), (1, 0)),                 # unmasked: no gate rides inside an aggregation
    (dict(proj_table=False, wm_ready=False), (1, 0)),
    (dict(by_member=False), (1, 0)),                                          # a batch queried alone in front of a group
    (dict(tail_gated=True, waited=True), (1, 0)),
    (dict(avg_topk=True, B=200, nxt=dict(NEXT, B=200)), (1, 0)),              # the statistics keep the next gate out of its aggregation
    # each single reason that withdraws it
    (dict(scoring=True), (0, 0)),
    (dict(exchange=True), (0, 0)),
    (dict(wm_ready=False), (0, 0)),                                           # proj_table without a ready W_m
    (dict(rows=(0, 3071)), (0, 0)),                                           # a shard
    (dict(rows=(1024, 3072)), (0, 0)),
    (dict(rows=(0, 0)), (0, 0)),                                              # n_rows = 0
    (dict(release=MEMBER_FRONT), (0, 0)),
    (dict(nxt=None), (0, 0)),                                                 # no next batch
    (dict(nxt=dict(NEXT, in_slot=False, by_member=False, launched=False, waited=False)), (0, 0)),
    (dict(nxt=dict(NEXT, launched=False, waited=False)), (0, 0)),
    (dict(nxt=dict(NEXT, by_member=False)), (0, 0)),
    (dict(nxt=dict(NEXT, tail_gated=True)), (0, 0)),
    (dict(nxt=dict(NEXT, B=682)), (0, 0)),                                    # the next batch rides inside its aggregation
    (dict(B=200, nxt=dict(NEXT, B=200, waited=False)), (0, 0)),               # C2
    (dict(nxt=dict(NEXT, B=683)), (1, 0)),
    (dict(release=LAUNCH, by_member=False, nxt=dict(NEXT, by_member=False)), (0, 0)),
]


@pytest.mark.parametrize("facts,want", TAIL, ids=[str(f) for f, _ in TAIL])
def test_step_tail_offer(hooks, facts, want):
    facts = dict(facts)
    facts.setdefault("nxt", NEXT)
    p = step_plan(hooks, **facts)
    assert (p["tail_offer"], p["tail_wait_filled"]) == want
    if want[0]:
        assert p["gru_is_last"] == 1


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("avg_topk", [False, True])
@pytest.mark.parametrize("B", [682, 683, 1024])
def test_tail_offer_and_next_gate_agree(hooks, masked, avg_topk, B):
    """Step b's view of batch b + 1 against batch b + 1's own plan: the same batch gets exactly one gate.  If b offers the tail
    gate, b + 1 (its bit set by the GRU kernel that took the offer) passes none; if b + 1 waits inside its aggregation, b offers
    nothing; and where b offers nothing, b + 1 (bit clear) passes a gate of its own."""
    for release in (0, MEMBER, MEMBER_FRONT):
        for waited in (False, True):
            b = step_plan(hooks, masked=masked, avg_topk=avg_topk, release=release, B=B, waited=True,
                          nxt=dict(NEXT, B=B, waited=waited))
            own = step_plan(hooks, masked=masked, avg_topk=avg_topk, release=release, B=B, waited=waited or bool(b["tail_offer"]))
            after_offer = step_plan(hooks, masked=masked, avg_topk=avg_topk, release=release, B=B, tail_gated=True, waited=True)
            if b["tail_offer"]:
                assert after_offer["gate"] == GATE["carried"]
                assert own["gate"] == GATE["front"]                  # what the offer replaces: never a gate inside the aggregation
                assert b["tail_wait_filled"] == int(not waited)      # the wait for `filled` moves with the gate, once per group
            if own["gate"] == GATE["inside"]:
                assert not b["tail_offer"]
            assert own["gate"] in (GATE["front"], GATE["inside"])    # bit clear: a gate of its own, one
            assert bool(b["tail_offer"]) == (release != MEMBER_FRONT and own["gate"] == GATE["front"])


def group_plan(hooks, streaming, release, want, n_more):
    out = (C.c_int64 * 2)(-1, -1)
    assert hooks.zt_test_group_plan(C.c_int32(int(streaming)), C.c_int32(release), C.c_int32(want), C.c_int32(n_more), out) == 0
    return out[0], out[1]


# ZT_RELEASE_LAUNCH: (want, n_more) -> batches the group may take (the taper: n_more - 1 where n_more <= want, at least 1)
TAPER = {
    (1, 0): 1, (1, 1): 1, (1, 2): 1,
    (2, 0): 1, (2, 1): 1, (2, 2): 1, (2, 3): 2,
    (4, 0): 1, (4, 1): 1, (4, 2): 1, (4, 3): 2, (4, 4): 3, (4, 5): 4,
    (8, 0): 1, (8, 1): 1, (8, 2): 1, (8, 7): 6, (8, 8): 7, (8, 9): 8,
}


@pytest.mark.parametrize("want", [1, 2, 4, 8])
def test_group_size_and_release(hooks, want):
    for n_more in sorted({0, 1, 2, want - 1, want, want + 1}):
        for release in (0, MEMBER, MEMBER_FRONT):
            assert group_plan(hooks, True, release, want, n_more) == (1, want)           # by member: full whatever is in sight
        assert group_plan(hooks, True, LAUNCH_FULL, want, n_more) == (0, want)           # the event without the taper
        assert group_plan(hooks, True, LAUNCH, want, n_more) == (0, TAPER[(want, n_more)])
        for release in (0, MEMBER, LAUNCH, LAUNCH_FULL, MEMBER_FRONT):                    # pruning: always 1, never by member
            assert group_plan(hooks, False, release, want, n_more) == (0, 1)


def test_group_size_is_capped(hooks):
    """ZT_MAX_GROUP = 8 (zt_pipeline_set_group refuses more; make_group clamped all the same)"""
    assert group_plan(hooks, True, 0, 9, 20) == (1, 8)
    assert group_plan(hooks, True, LAUNCH, 9, 20) == (0, 8)
    assert group_plan(hooks, True, LAUNCH, 9, 9) == (0, 8)     # (the clamp comes first: 9 followers against a want of 8)
    assert group_plan(hooks, True, LAUNCH, 9, 8) == (0, 7)


# The gate forms the GPU tests reach (every form by at least one): test -> configuration of its steps -> form
REACH = [
    # test_tail_gate_gpu.py: CU-masked, bs 1024 (a last batch of 700: 2100 rows), groups of 4 and 8
    ("tail_gate: the library's pick, first member of a group", dict(B=1024), "front"),
    ("tail_gate: the library's pick, a later member", dict(B=1024, tail_gated=True, waited=True), "carried"),
    ("tail_gate: the ragged last batch", dict(B=700, tail_gated=True, waited=True), "carried"),
    ("tail_gate: ZT_RELEASE_MEMBER_FRONT", dict(B=1024, release=MEMBER_FRONT, waited=True), "front"),
    ("tail_gate: ZT_RELEASE_LAUNCH", dict(B=1024, release=LAUNCH, by_member=False), "event"),
    ("tail_gate: blind (every batch alone)", dict(B=1024, by_member=False), "event"),
    # test_grouped_tppr_launches_match_sequential: bs 20, groups of 2 .. 8; unmasked, and one CU-masked case
    ("grouped: whole batches", dict(B=20, masked=False), "front"),
    ("grouped: whole batches, a later member", dict(B=20, masked=False, tail_gated=True, waited=True), "carried"),
    ("grouped: row shards", dict(B=20, masked=False, rows=(10, 55)), "front"),
    ("grouped: ZT_RELEASE_LAUNCH", dict(B=20, masked=False, release=LAUNCH, by_member=False), "event"),
    ("grouped: CU-masked, whole batches", dict(B=20, masked=True), "inside"),
    ("grouped: CU-masked, row shards", dict(B=20, masked=True, rows=(10, 55)), "front"),
    # test_pipelined_step_matches_sequential: one batch per launch
    ("pipelined: streaming", dict(B=20, masked=False, by_member=False), "event"),
    ("pipelined: streaming, CU-masked", dict(B=20, masked=True, by_member=False), "event"),
    ("pipelined: pruning", dict(B=20, streaming=False, masked=False, by_member=False), "event"),
    # test_bench_path_vs_oracle_c5_launch_shapes: CU-masked, bs 4096; groups of 2 by launch, groups of 4 by member
    ("c5 launch shapes: groups of 2", dict(B=4096, release=LAUNCH, by_member=False), "event"),
    ("c5 launch shapes: groups of 4, first member", dict(B=4096), "front"),
    ("c5 launch shapes: groups of 4, a later member", dict(B=4096, tail_gated=True, waited=True), "carried"),
]


@pytest.mark.parametrize("name,facts,want", REACH, ids=[r[0] for r in REACH])
def test_gate_forms_the_gpu_tests_reach(hooks, name, facts, want):
    assert step_plan(hooks, **facts)["gate"] == GATE[want]


def test_gpu_tests_reach_every_gate_form():
    assert {r[2] for r in REACH} == set(GATE)
