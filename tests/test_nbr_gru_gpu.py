"""The neighbour half of the persistent output layers in the GRU update's grid (k_nbr_gru, csrc/memory_update.hip) behind a
source-only launch (k_embed_src3, csrc/aggregate.hip), held bit for bit against the kernels it replaces on C5's path --
k_embed_out3 whole + k_gru -- and against the tiled pair in one launch (k_out_gru).  D = T = 100, F = 1, k = 20.

Directly (the hook zt_test_embed_gru: the two calls of a pipeline step without the pipeline; its max_wgs is the most persistent
workgroups each launch of the divided form may take, so that the seams of a small grid sit at small sizes):
  * output rows N = 1, 15, 16, 17, 3 16 + 5, and N whose (16 rows, model) units are fewer than, as many as and one more than the
    striding waves of the neighbour workgroups (one workgroup of eight waves under a limit of 1: 7, 8, 9 units; M = 2: 8 units);
    17 units under a limit of 2: a second neighbour workgroup, and a wave of the first with a second unit;
  * the library's own pick: 8 192 output rows are divided (k_nbr_gru), 8 191 are not (k_out_gru), and ZT_OUT_WHOLE keeps 8 192
    whole (k_embed_out3 in the embed call) -- all three the same bits;
  * M = 1 and 2; GRU rows 0, 1, 16, 17, 2 16 + 3 -- more tiles than the neighbour workgroups allowed, and fewer; no rows at all (the
    neighbour half then runs by itself, k_embed_nbr3);
  * the output rows draw their node ids from a small pool, with repeats, and the GRU rows are ids of the same pool: the source
    path reads rows the update rewrites; the last model's neighbourhoods are empty (S = 0); both cells.
Through the pipeline: twelve steps at bs 64 (CU masks and launch groups as synth.pipeline_settings gives them) with the form
forced, forbidden (the library's pick of output layers, other kernels altogether, beside the GRU tile) and as C5's pair, k_embed_out3 +
k_gru, against each other bit for
bit and against ProtocolOracle at tests/test_tail_gate_gpu.py's tolerance; and at bs 700 (2 100 rows: the gate is a kernel in
front, so the GRU kernel is offered the next batch's gate) forced against the pair: the same bits and the same number of gates
carried at the tail -- the offer survives the move into k_nbr_gru.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn

pytestmark = pytest.mark.gpu
TOL = 1e-4
D = T = 100
F, K = 1, 20
MSG = 2 * D + F + T
NODES, EDGES, POOL = 300, 500, 40                # tables of the direct cases; the ids in play
CELL_GRU, CELL_RNN = 0, 1
NBR_GRU, WHOLE, PERSIST, TILED = 4, 5, 3, 1      # ZT_OUT_*
GRU_TILE = 1
# what became of the held-back layers (zt_test_memory_plan's values)
NOT_HELD, FRONT, FUSED_TILE, FUSED_NBR = 0, 1, 2, 4


@pytest.fixture(scope="module")
def libs():
    from zebra_amd import _capi
    return _capi, _capi.lib(), _capi.hooks_lib()


@pytest.fixture(scope="module")
def tables():
    """The weights and the tables every direct case starts from (made once, never changed: a case works on clones)."""
    rng = np.random.RandomState(1515)
    dev = "cuda"
    w = I.model_weights(D, F, T, 2, 1516)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s = 1.0 / np.sqrt(D)
    return dict(
        w={kk: t(v) for kk, v in w.items()}, time_w=t(I.time_encode_weights(T)),
        rnn={"w_ih": t(rng.uniform(-s, s, (D, MSG)).astype(np.float32)), "w_hh": t(rng.uniform(-s, s, (D, D)).astype(np.float32)),
             "b_ih": t(rng.uniform(-s, s, D).astype(np.float32)), "b_hh": t(rng.uniform(-s, s, D).astype(np.float32))},
        memory=t((rng.standard_normal((NODES, D)) * 0.5).astype(np.float32)),
        last_update=t(rng.uniform(0, 100, NODES).astype(np.float32)),
        messages=t(rng.standard_normal((NODES, MSG)).astype(np.float32)),
        msg_ts=t(rng.uniform(100, 200, NODES).astype(np.float32)),
        efeat=t(np.zeros((EDGES, F), np.float32)))


def direct(libs, tables, N, M, gru_rows, max_rows, cell, max_wgs, out_choice, gru_choice):
    """One embed + update under the given choices, from fresh clones of the tables; every input is drawn from the case's own seed,
    the same for every form."""
    _capi, lib, hooks = libs
    ptr = _capi.ptr
    dev = "cuda"
    rng = np.random.RandomState(1000 * N + 10 * gru_rows + M)
    nodes = torch.from_numpy(rng.randint(1, POOL, N).astype(np.int32)).to(dev)           # repeats among the output rows
    nbr = rng.randint(1, NODES, (M, N, K)).astype(np.int32)
    eix = rng.randint(1, EDGES, (M, N, K)).astype(np.int32)
    dt = rng.uniform(0, 1000, (M, N, K)).astype(np.float32)
    wt = rng.uniform(0.01, 1, (M, N, K)).astype(np.float32)
    wt[:, N // 2] = 0                                                                    # one row without neighbours in every model
    if M > 1:
        nbr[M - 1], eix[M - 1], dt[M - 1], wt[M - 1] = 0, 0, 0, 0                        # the last model: S = 0 throughout
    nbr, eix, dt, wt = (torch.from_numpy(x).to(dev) for x in (nbr, eix, dt, wt))
    rows = torch.from_numpy(rng.permutation(np.arange(1, POOL))[:gru_rows].astype(np.int32)).to(dev)   # distinct ids of the pool
    memory, last_update = tables["memory"].clone(), tables["last_update"].clone()
    flags = torch.zeros(NODES, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((N, D * (M + 1)), float("nan"), dtype=torch.float32, device=dev)
    w = tables["w"]
    ew = _capi.EmbedWeights(*[ptr(w[n]) for n in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc1s_w", "fc1s_b", "fc2s_w", "fc2s_b")],
                            ptr(tables["time_w"]))
    g = w if cell == CELL_GRU else tables["rnn"]
    gw = _capi.GruWeights(ptr(g["w_ih"]), ptr(g["w_hh"]), ptr(g["b_ih"]), ptr(g["b_hh"]))
    i32, i64 = C.c_int32, C.c_int64
    ews = torch.zeros(int(lib.zt_embed_workspace_bytes(i64(N), i32(D), i32(F), i32(T), i32(M), i32(K))), dtype=torch.uint8, device=dev)
    gws = torch.zeros(int(lib.zt_gru_workspace_bytes(i64(max(1, max_rows)), i32(D), i32(MSG))), dtype=torch.uint8, device=dev)
    off = int(lib.zt_gru_rows_offset(i32(D), i32(MSG)))
    gws[:4].view(torch.int32)[0] = gru_rows
    if gru_rows:
        gws[off:off + 4 * gru_rows].view(torch.int32).copy_(rows)
    table = torch.zeros(int(lib.zt_project_table_bytes(i64(NODES), i32(D))) // 4, dtype=torch.float32, device=dev)
    st = _capi.stream_ptr()
    _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, out_choice)
    _capi.set_kernel_choice(_capi.CHOICE_GRU, gru_choice)
    try:
        # the projected table of the memory as it stands (pads the weights into the embed workspace)
        _capi.check(lib.zt_project_memory(ptr(memory), i64(NODES), i32(D), i32(F), i32(T), C.byref(ew), i32(0), None, None, i64(0),
                                          ptr(table), ptr(ews), i64(N), i32(M), i32(K), st), "zt_project_memory")
        launch = i32(-1)
        _capi.check(hooks.zt_test_embed_gru(ptr(memory), ptr(tables["efeat"]), i64(NODES), i64(EDGES), i32(D), i32(F), i32(T),
                                            ptr(nodes), i64(N), i32(M), i32(K), ptr(nbr), ptr(eix), ptr(dt), ptr(wt), C.byref(ew),
                                            ptr(out), ptr(ews), ptr(status), ptr(table), i32(1), ptr(last_update),
                                            ptr(tables["messages"]), ptr(tables["msg_ts"]), ptr(flags), i32(MSG), i64(max_rows),
                                            C.byref(gw), ptr(gws), i32(0), i32(cell), i32(max_wgs), C.byref(launch), st), "zt_test_embed_gru")
        torch.cuda.synchronize()
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, 0)
        _capi.set_kernel_choice(_capi.CHOICE_GRU, 0)
    assert int(status.item()) == 0
    cnt = int(gws[:4].view(torch.int32)[0].item())
    return dict(launch=launch.value, out=out.cpu().numpy(), memory=memory.cpu().numpy(), last_update=last_update.cpu().numpy(),
                P=table.cpu().numpy(), rows=gws[off:off + 4 * gru_rows].view(torch.int32).cpu().numpy().copy(), count=cnt,
                want_rows=rows.cpu().numpy())


def same(a, b, what):
    for kk in ("out", "memory", "last_update", "P", "rows"):
        assert np.array_equal(a[kk], b[kk]), "%s: %s" % (what, kk)
    assert a["count"] == b["count"], what


# (N, M, GRU rows, the most persistent workgroups).  Under a limit of 1 the neighbour half is one workgroup: eight striding waves
SHAPES = [
    (1, 1, 0, 2), (1, 2, 1, 2), (15, 2, 1, 2), (16, 1, 16, 2), (16, 2, 17, 2), (17, 2, 17, 2), (17, 1, 35, 2), (53, 2, 35, 2),
    (53, 1, 16, 2),
    (7 * 16, 1, 35, 1), (8 * 16, 1, 17, 1), (8 * 16 + 1, 1, 16, 1), (4 * 16, 2, 35, 1), (4 * 16 + 1, 2, 1, 1), (3 * 16 + 5, 2, 0, 1),
    # 17 units, two to a wave of eight: two neighbour workgroups asked for and allowed (the stride across workgroups)
    (17 * 16, 1, 17, 2),
]


@pytest.mark.parametrize("cell", [CELL_GRU, CELL_RNN], ids=["gru", "rnn"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_same_bits_as_the_separate_kernels_and_the_tiled_pair(libs, tables, shape, cell):
    N, M, gru_rows, cap = shape
    max_rows = max(gru_rows, 16)                 # (0 rows: the kernel runs and its one tile finds nothing to do)
    new = direct(libs, tables, N, M, gru_rows, max_rows, cell, cap, NBR_GRU, 0)
    assert new["launch"] == FUSED_NBR
    assert not np.isnan(new["out"]).any()
    assert np.array_equal(new["rows"], new["want_rows"]) and new["count"] == gru_rows     # the row list is the caller's, untouched
    pair = direct(libs, tables, N, M, gru_rows, max_rows, cell, cap, PERSIST, GRU_TILE)
    assert pair["launch"] == NOT_HELD            # k_embed_out3 ran whole inside the embed call, k_gru by itself
    same(new, pair, "k_embed_src3 + k_nbr_gru against k_embed_out3 + k_gru")
    tiled = direct(libs, tables, N, M, gru_rows, max_rows, cell, cap, TILED, GRU_TILE)
    assert tiled["launch"] == FUSED_TILE
    same(new, tiled, "k_embed_src3 + k_nbr_gru against k_out_gru")
    # the update did something: the listed rows moved, nothing else did
    moved = np.flatnonzero((new["memory"] != tables["memory"].cpu().numpy()).any(axis=1))
    assert set(moved) <= set(new["want_rows"].tolist()) and (gru_rows == 0 or len(moved) > 0)


@pytest.mark.parametrize("shape", [(17, 2, 2), (8 * 16 + 1, 1, 1), (17 * 16, 1, 2)], ids=str)
def test_without_an_update_the_neighbour_half_runs_by_itself(libs, tables, shape):
    """no ids to update: no GRU kernel is launched, and the held-back half goes out on the way (k_embed_nbr3)"""
    N, M, cap = shape
    new = direct(libs, tables, N, M, 0, 0, CELL_GRU, cap, NBR_GRU, 0)
    assert new["launch"] == FRONT
    pair = direct(libs, tables, N, M, 0, 0, CELL_GRU, cap, PERSIST, GRU_TILE)
    same(new, pair, "k_embed_src3 + k_embed_nbr3 against k_embed_out3")
    assert not np.isnan(new["out"]).any()
    assert np.array_equal(new["memory"], tables["memory"].cpu().numpy())


def test_the_librarys_own_pick_divides_from_8192_rows_on(libs, tables):
    """ZT_CHOICE_EMBED_OUT = 0: the persistent form's threshold is the division's; ZT_OUT_WHOLE forbids it there"""
    own = direct(libs, tables, 8192, 1, 17, 17, CELL_GRU, 0, 0, GRU_TILE)
    assert own["launch"] == FUSED_NBR
    assert not np.isnan(own["out"]).any()
    whole = direct(libs, tables, 8192, 1, 17, 17, CELL_GRU, 0, WHOLE, GRU_TILE)
    assert whole["launch"] == NOT_HELD           # k_embed_out3 ran whole inside the embed call
    same(own, whole, "the library's pick against ZT_OUT_WHOLE at 8 192 rows")
    pinned = direct(libs, tables, 8192, 1, 17, 17, CELL_GRU, 0, PERSIST, GRU_TILE)
    assert pinned["launch"] == NOT_HELD
    same(own, pinned, "the library's pick against ZT_OUT_PERSIST at 8 192 rows")
    below = direct(libs, tables, 8191, 1, 17, 17, CELL_GRU, 0, 0, GRU_TILE)
    assert below["launch"] == FUSED_TILE         # the tiled pair in one launch, as before
    forced = direct(libs, tables, 8191, 1, 17, 17, CELL_GRU, 0, NBR_GRU, GRU_TILE)
    assert forced["launch"] == FUSED_NBR
    same(below, forced, "the library's pick against ZT_OUT_NBR_GRU at 8 191 rows")
    # forbidden at a size where it can be forced: the latency-organised layers, held back for the GRU launch, never k_nbr_gru
    small = direct(libs, tables, 600, 1, 17, 17, CELL_GRU, 0, WHOLE, GRU_TILE)
    assert small["launch"] == FRONT
    same(small, direct(libs, tables, 600, 1, 17, 17, CELL_GRU, 0, NBR_GRU, GRU_TILE), "ZT_OUT_WHOLE against ZT_OUT_NBR_GRU at 600 rows")


# ---------------------------------------------------------------------------------------------------------------------
NB = 12


def make_world(oracle, bs, n_nodes, with_oracle):
    from zebra_amd import synth
    wl = dict(synth.WORKLOADS["c5"], n_nodes=n_nodes, n_edges=(NB + 1) * bs, bs=bs)
    E = wl["n_edges"]
    src, dst, ts, eidx = synth.power_law_stream(n_nodes, E, bipartite=None, seed=3030, perm_seed=9)
    neg = synth.negatives(dst, E, seed=3031)
    M = len(wl["alpha"])
    w = I.model_weights(D, F, T, M, 505)
    efeat = synth.edge_features(E + 1, F, seed=506)
    cuts = [(b * bs, (b + 1) * bs) for b in range(NB)]
    world = dict(wl=wl, stream=(src, dst, neg, ts, eidx), w=w, efeat=efeat, cuts=cuts, n_nodes=n_nodes)
    if with_oracle:
        p = oracle.ProtocolOracle(n_nodes + 1, D, F, T, K, wl["alpha"], wl["beta"], w, efeat, I.time_encode_weights(T), "streaming",
                                  None, 10, 2, n_threads=8)
        world["ref_emb"] = [p.batch(src[a:b], dst[a:b], neg[a:b], ts[a:b], eidx[a:b], False)[0] for a, b in cuts]
        world["ref_memory"], world["ref_last_update"] = p.mem.memory.copy(), p.mem.last_update.copy()
    return world


@pytest.fixture(scope="module")
def small_world(oracle):
    return make_world(oracle, 64, 2000, True)


@pytest.fixture(scope="module")
def gated_world(oracle):
    return make_world(oracle, 700, 20_000, False)


def run_pipeline(world, out_choice, gru_choice):
    from zebra_amd import _capi, synth
    wl = world["wl"]
    M, bs = len(wl["alpha"]), wl["bs"]
    _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, out_choice)
    _capi.set_kernel_choice(_capi.CHOICE_GRU, gru_choice)
    try:
        tgn = build_tgn(world["n_nodes"] + 1, len(world["efeat"]), D, F, T, K, wl["alpha"], wl["beta"], world["w"], world["efeat"]).eval()
        cus, group = synth.pipeline_settings(wl, NB)
        tgn.enable_pipeline(tppr_cus=cus, max_batch=bs, group=group)
        dev = tgn.device
        t = [torch.from_numpy(x).to(dev) for x in world["stream"]]
        batches = [tuple(x[a:b] for x in t) for a, b in world["cuts"]]
        with torch.cuda.stream(tgn.main_stream):
            out = torch.zeros((NB, 3 * bs, D * (M + 1)), dtype=torch.float32, device=dev)
            tgn.run_device(tgn.prepare_run(batches), out=out)
        torch.cuda.synchronize()
        tgn.check_status()
        res = dict(carried=tgn.pipeline_tail_gates(), embs=out.cpu().numpy(), memory=tgn.memory.memory.cpu().numpy(),
                   last_update=tgn.memory.last_update.cpu().numpy())
        tgn.enable_pipeline(False)
        return res
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, 0)
        _capi.set_kernel_choice(_capi.CHOICE_GRU, 0)


def same_run(a, b, what):
    for q in range(NB):
        assert np.array_equal(a["embs"][q], b["embs"][q]), "%s: embeddings of step %d" % (what, q)
    assert np.array_equal(a["memory"], b["memory"]), "%s: memory" % what
    assert np.array_equal(a["last_update"], b["last_update"]), "%s: last_update" % what


def test_pipeline_forced_against_forbidden_and_the_oracle(small_world):
    forced = run_pipeline(small_world, NBR_GRU, 0)
    for q, ref in enumerate(small_world["ref_emb"]):
        d = float(np.abs(forced["embs"][q] - ref).max())
        assert d <= TOL, "embeddings of step %d differ from the oracle by %g" % (q, d)
    assert float(np.abs(forced["memory"] - small_world["ref_memory"]).max()) <= TOL
    assert np.array_equal(forced["last_update"], small_world["ref_last_update"])
    # (forbidden: the library's pick of output layers for 192 rows, the latency-organised ones.  The GRU tile is pinned beside it:
    #  held-back neighbour paths draw the update to the tile, the library's pick for 128 rows would be the split, and the split's
    #  four waves divide K and add their partial gate sums afterwards -- the two GRU forms agree to rounding, 2e-6 in
    #  tests/test_embed_gpu.py, not to the bit (csrc/common.hpp, at MemoryPlan).  The pin changes nothing at the sizes the
    #  library divides by itself: from 8 192 output rows on, the pipeline's update has 5 462 rows and more, the tile's)
    forbidden = run_pipeline(small_world, WHOLE, GRU_TILE)
    same_run(forced, forbidden, "forced against forbidden (the library's pick)")
    assert forced["carried"] == forbidden["carried"], (forced["carried"], forbidden["carried"])
    pair = run_pipeline(small_world, PERSIST, GRU_TILE)
    same_run(forced, pair, "forced against k_embed_out3 + k_gru")
    assert forced["carried"] == pair["carried"], (forced["carried"], pair["carried"])


def test_pipeline_tail_offer_survives_the_move(gated_world):
    forced = run_pipeline(gated_world, NBR_GRU, 0)
    pair = run_pipeline(gated_world, PERSIST, GRU_TILE)
    same_run(forced, pair, "forced against k_embed_out3 + k_gru")
    # every step but the last has a batch in sight whose gate its GRU kernel can carry (the very first may not: its GRU kernel is
    # followed by the first refresh of the projected table) -- in k_gru and in k_nbr_gru alike
    assert NB - 2 <= pair["carried"] <= NB - 1, pair["carried"]
    assert forced["carried"] == pair["carried"], (forced["carried"], pair["carried"])
