"""CPU-side pin of where the neighbour half of the persistent output layers runs in the GRU update's grid (k_nbr_gru,
csrc/memory_update.hip), through the same hooks as tests/test_launch_plan_cpu.py and with that file's answers untouched.

The form has two ends.  zt::embed_kernel_plan keeps answering `persist` for C5's shape; what a caller that can hold output layers
back (the pipeline) does with it -- source half launched at once, neighbour half handed on -- is the plan's `nbr_later`, which
that hook does not report and zt_test_embed_divided does: true for the library's own pick exactly from 8 192 rows on (C5's
pipeline), never under ZT_OUT_WHOLE or a pinned form, at any batch size under ZT_OUT_NBR_GRU, never with partial-sum groups.
What zt::embed_ex then hands to the memory update is an OutForm of its own (3, the persistent form's neighbour half).
zt::memory_kernel_plan answers for that form: behind the tile's workgroups in one grid (4) wherever the
tile runs, which such held-back layers make it do at any row count unless the split is pinned; in front otherwise.
ZT_CHOICE_EMBED_OUT: ZT_OUT_NBR_GRU = the persistent form at any batch size (and nbr_later), ZT_OUT_WHOLE = the pick by shape with
the output layers never divided; a pinned ZT_OUT_PERSIST is k_embed_out3 whole, as it was."""
import ctypes as C
import os

import pytest

AGG = {"reg": 1}
OUT = {"tiled": 0, "latency": 1, "persist": 2, "persist_nbr": 3}
REFUSAL = {"none": 0, "msg_wide": 3}
GRU = {"none": 0, "tile": 1, "split": 2}
HELD = {"none": 0, "front": 1, "fused_tile": 2, "fused_split": 3, "fused_nbr": 4}
GRU_TILE, GRU_SPLIT = 1, 2                                      # ZT_GRU_*
TILED, LATENCY, PERSIST, NBR_GRU, WHOLE = 1, 2, 3, 4, 5          # ZT_OUT_*
EO3_NBR_LDS = 7 * 7 * 256 * 4                                   # fc2 in fragment order


@pytest.fixture(scope="module")
def hooks():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi.hooks_lib()


def plan(hooks, N, D, F, T, M, k, table, out_choice=0):
    a, o, lds = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    rc = hooks.zt_test_embed_plan(C.c_int64(N), C.c_int32(D), C.c_int32(F), C.c_int32(T), C.c_int32(M), C.c_int32(k),
                                  C.c_int32(int(table)), C.c_int32(0), C.c_int32(0), C.c_int32(out_choice), C.byref(a),
                                  C.byref(o), C.byref(lds))
    assert rc == 0
    return a.value, o.value, lds.value


def held_plan(hooks, rows, D, msg, gru_choice, held):
    """held: (form, hg, D, M, gx, N, same memory) of the output layers embed_ex held back"""
    form, hg, hD, hM, gx, hN, same = held
    out = (C.c_int64 * 14)(*([-1] * 14))
    rc = hooks.zt_test_memory_plan(C.c_int64(rows), C.c_int32(D), C.c_int32(msg), C.c_int32(1), C.c_int32(100),
                                   C.c_int32(gru_choice), C.c_int32(0), C.c_int32(1), C.c_int32(OUT[form]), C.c_int32(hg),
                                   C.c_int32(hD), C.c_int32(hM), C.c_int32(gx), C.c_int64(hN), C.c_int32(int(same)), out)
    assert rc == 0
    keys = ("refusal", "msg", "gru", "out", "lds", "lds2", "lds_f", "gru_tiles", "NTg", "n_src_wgs", "n_nb_wgs",
            "out_tiles", "target", "participants")
    return dict(zip(keys, list(out)))


def test_header_values_match():
    from zebra_amd import _capi
    assert (_capi.OUT_NBR_GRU, _capi.OUT_WHOLE) == (NBR_GRU, WHOLE)
    with open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "zebra_amd.h")) as fh:
        text = fh.read()
    assert "#define ZT_OUT_NBR_GRU 4" in text and "#define ZT_OUT_WHOLE 5" in text


# ---- the embedding's end: (N, ZT_CHOICE_EMBED_OUT) -> output layers, at C5's widths with the table (aggregation: reg) ----
EMBED = [
    # the library's pick: unchanged (these three rows repeat test_launch_plan_cpu.py's)
    ((12288, 0), "persist"), ((8191, 0), "tiled"), ((1024, 0), "latency"),
    # forced: the persistent form at any batch size
    ((12288, NBR_GRU), "persist"), ((8191, NBR_GRU), "persist"), ((1025, NBR_GRU), "persist"), ((600, NBR_GRU), "persist"),
    ((16, NBR_GRU), "persist"), ((1, NBR_GRU), "persist"),
    # forbidden: the pick by shape
    ((12288, WHOLE), "persist"), ((8192, WHOLE), "persist"), ((8191, WHOLE), "tiled"), ((1025, WHOLE), "tiled"),
    ((1024, WHOLE), "latency"), ((600, WHOLE), "latency"),
    # the pinned forms are what they were
    ((600, PERSIST), "persist"), ((12288, TILED), "tiled"), ((12288, LATENCY), "latency"),
]


@pytest.mark.parametrize("shape,want", EMBED, ids=[str(s) for s, _ in EMBED])
def test_output_layer_choice_values(hooks, shape, want):
    N, oc = shape
    assert plan(hooks, N, 100, 1, 100, 2, 20, True, out_choice=oc) == (AGG["reg"], OUT[want], 0)


def test_forced_form_needs_the_persistent_kernels_width(hooks):
    """Dp = 128, D % 4 != 0: no persistent form, forced or not -- the library's pick"""
    for D, want in ((128, "tiled"), (98, "tiled")):
        for oc in (0, NBR_GRU, WHOLE):
            assert plan(hooks, 8192, D, 1, 100, 2, 20, True, out_choice=oc)[1] == OUT[want]


# ---- the division itself: (N, F, ZT_CHOICE_EMBED_OUT) -> does a caller that holds output layers back get the form divided ----
def divided(hooks, N, F, out_choice, D=100, table=True):
    v = C.c_int32(-1)
    rc = hooks.zt_test_embed_divided(C.c_int64(N), C.c_int32(D), C.c_int32(F), C.c_int32(100), C.c_int32(2), C.c_int32(20),
                                     C.c_int32(int(table)), C.c_int32(out_choice), C.byref(v))
    assert rc == 0
    assert v.value in (0, 1)
    return bool(v.value)


DIVIDED = [
    # the library's own pick: divided exactly where the persistent form is its answer -- C5's pipeline (12 288 rows), from 8 192 on
    ((12288, 1, 0), True), ((8192, 1, 0), True), ((8191, 1, 0), False), ((1025, 1, 0), False), ((1024, 1, 0), False),
    ((600, 1, 0), False), ((1, 1, 0), False),
    # forbidden: the same pick of kernels by shape, never divided
    ((12288, 1, WHOLE), False), ((8192, 1, WHOLE), False), ((8191, 1, WHOLE), False), ((600, 1, WHOLE), False),
    # the pinned forms are what they were: k_embed_out3 whole, the tiled and the latency-organised layers
    ((12288, 1, PERSIST), False), ((600, 1, PERSIST), False), ((12288, 1, TILED), False), ((12288, 1, LATENCY), False),
    # forced: at any batch size
    ((12288, 1, NBR_GRU), True), ((8191, 1, NBR_GRU), True), ((600, 1, NBR_GRU), True), ((16, 1, NBR_GRU), True),
    ((1, 1, NBR_GRU), True),
    # partial-sum groups in H (F = 172: k_fc1_agg_wide, five groups a row): the persistent form, whole
    ((12288, 172, 0), False), ((12288, 172, NBR_GRU), False), ((600, 172, NBR_GRU), False),
]


@pytest.mark.parametrize("shape,want", DIVIDED, ids=[str(s) for s, _ in DIVIDED])
def test_where_the_persistent_form_is_divided(hooks, shape, want):
    N, F, oc = shape
    assert divided(hooks, N, F, oc) is want


def test_division_follows_the_persistent_form(hooks):
    """divided => the plan's output layers are the persistent ones; the F = 172 shapes above are persistent and whole"""
    for N in (1, 600, 1024, 1025, 8191, 8192, 12288):
        for F in (1, 172):
            for oc in (0, TILED, LATENCY, PERSIST, NBR_GRU, WHOLE):
                out = plan(hooks, N, 100, F, 100, 2, 20, True, out_choice=oc)[1]
                if divided(hooks, N, F, oc):
                    assert out == OUT["persist"], (N, F, oc)
    for N, oc in ((12288, 0), (12288, NBR_GRU), (600, NBR_GRU)):
        assert plan(hooks, N, 100, 172, 100, 2, 20, True, out_choice=oc)[1] == OUT["persist"]
    # other widths have no persistent form to divide, forced or not
    for D in (128, 98):
        for oc in (0, NBR_GRU):
            assert not divided(hooks, 8192, 1, oc, D=D)


# ---- the memory update's end: (rows, D, msg, ZT_CHOICE_GRU, held) -> (output layers, GRU form, lds_f, n_nb_wgs, gru_tiles) ----
C5 = ("persist_nbr", 1, 100, 2, 0, 12288, True)
NBR = [
    # C5's pipeline: 8 192 endpoints, 12 288 output rows of two models = 1 536 units, two to a wave of eight: 96 workgroups
    ((8192, 100, 301, 0, C5), ("fused_nbr", "tile", EO3_NBR_LDS, 96, 512)),
    ((8192, 100, 301, GRU_TILE, C5), ("fused_nbr", "tile", EO3_NBR_LDS, 96, 512)),
    # a wide message: the tile's own LDS is the larger need
    ((1200, 100, 1072, 0, ("persist_nbr", 1, 100, 2, 0, 1800, True)), ("fused_nbr", "tile", 76160, 15, 75)),
    # held-back neighbour paths draw the update to the tile at any row count ...
    ((400, 100, 472, 0, ("persist_nbr", 1, 100, 2, 0, 600, True)), ("fused_nbr", "tile", EO3_NBR_LDS, 5, 25)),
    ((16, 100, 301, 0, ("persist_nbr", 1, 100, 1, 0, 1, True)), ("fused_nbr", "tile", EO3_NBR_LDS, 1, 1)),
    ((16, 100, 301, 0, ("persist_nbr", 1, 100, 1, 0, 16 * 16, True)), ("fused_nbr", "tile", EO3_NBR_LDS, 1, 1)),
    ((16, 100, 301, 0, ("persist_nbr", 1, 100, 1, 0, 16 * 16 + 1, True)), ("fused_nbr", "tile", EO3_NBR_LDS, 2, 1)),
    # ... unless the split is pinned: then in front, by themselves
    ((400, 100, 472, GRU_SPLIT, ("persist_nbr", 1, 100, 2, 0, 600, True)), ("front", "split", 0, 0, 25)),
    ((8193, 100, 301, GRU_SPLIT, C5), ("fused_nbr", "tile", EO3_NBR_LDS, 96, 513)),      # (beyond the split's reach: the tile)
    # they read nothing of the memory table: whose table the update rewrites does not matter
    ((8192, 100, 301, 0, ("persist_nbr", 1, 100, 2, 0, 12288, False)), ("fused_nbr", "tile", EO3_NBR_LDS, 96, 512)),
    # partial-sum groups, other widths: in front
    ((8192, 100, 472, 0, ("persist_nbr", 10, 100, 2, 0, 12288, True)), ("front", "tile", 0, 0, 512)),
    ((8192, 100, 301, 0, ("persist_nbr", 1, 128, 2, 0, 12288, True)), ("front", "tile", 0, 0, 512)),
    # no rows, a refused update: they still run, in front
    ((0, 100, 301, 0, C5), ("front", "none", 0, 0, 0)),
]


@pytest.mark.parametrize("shape,want", NBR, ids=[str(s) for s, _ in NBR])
def test_neighbour_half_beside_the_gru_tiles(hooks, shape, want):
    rows, D, msg, gc, held = shape
    p = held_plan(hooks, rows, D, msg, gc, held)
    assert p["refusal"] == REFUSAL["none"]
    assert (p["out"], p["gru"], p["lds_f"], p["n_nb_wgs"], p["gru_tiles"]) == (HELD[want[0]], GRU[want[1]]) + want[2:]
    # no gate, no source-path workgroups, no tiled rows: nothing of the other fused forms
    assert (p["n_src_wgs"], p["out_tiles"], p["target"], p["participants"]) == (0, 0, 0, 0)


def test_refused_update_keeps_them_in_front(hooks):
    p = held_plan(hooks, 400, 100, 1073, 0, ("persist_nbr", 1, 100, 2, 0, 600, True))
    assert (p["refusal"], p["out"], p["gru"]) == (REFUSAL["msg_wide"], HELD["front"], GRU["none"])


def test_the_whole_persistent_form_is_still_never_fused(hooks):
    """what test_launch_plan_cpu.py pins for C5 (`persist`, 2): in front, under every ZT_CHOICE_GRU value"""
    for gc in (0, GRU_TILE, GRU_SPLIT):
        p = held_plan(hooks, 8192, 100, 301, gc, ("persist", 1, 100, 2, 0, 12288, True))
        assert (p["out"], p["lds_f"], p["n_nb_wgs"]) == (HELD["front"], 0, 0)


def test_hook_refuses_a_fifth_form(hooks):
    out = (C.c_int64 * 14)()
    i32 = C.c_int32
    assert hooks.zt_test_memory_plan(C.c_int64(8192), i32(100), i32(301), i32(1), i32(100), i32(0), i32(0), i32(1), i32(4), i32(1),
                                     i32(100), i32(2), i32(0), C.c_int64(12288), i32(1), out) != 0
