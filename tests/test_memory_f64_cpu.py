"""oracle/memory_f64.py, the float64 restatement tests/test_memory_f64_gpu.py holds the memory path to, checked without
a GPU: cell_update against torch's GRUCell / RNNCell in float64 and against the C oracle's gru_update, store_messages
against the C oracle's; the conditions on the GPU file's inputs that its tolerances rely on (torch float32 within half the
tolerance of float64 on every plain case, the stress rows as saturated as they are said to be, the batches as awkward);
a listed shape for every residue of the k-step count; and, through zt_test_memory_plan, that every GPU case reaches the
kernel its name says -- a pinned split silently falls back where it does not fit (D = 113)."""
import numpy as np
import pytest
import torch

import inputs as I
import test_launch_plan_cpu as LP
import test_memory_f64_gpu as G
from test_launch_plan_cpu import hooks          # noqa: F401  (the fixture)

M64 = G.oracle()


def _flags(il):
    f = np.zeros(G.NN, np.uint8)
    f[il["flagged"]] = 1
    return f


# ----------------------------------------------------------------------------------------------- the restatement's pins --
@pytest.mark.parametrize("cell", G.CELLS)
@pytest.mark.parametrize("D,msg", [(100, 472), (4, 13), (132, 465), (1, 577)])
def test_cell_update_is_torch_float64(D, msg, cell):
    x = G.make_cell_inputs(cell, D, msg)
    for kind in ("plain", "awkward", "all"):
        ref = G.cell_reference(cell, D, msg, False, 40, kind, 0)
        rows = ref["rows"]
        c = G.torch_cell(cell, D, msg, x, dtype=torch.float64)
        with torch.no_grad():
            want = c(G._t(x["messages"][rows]).double(), G._t(x["memory"][rows]).double()).numpy()
        assert ref["memory"].dtype == np.float64 and len(rows) > 0
        assert np.abs(ref["memory"][rows] - want).max() <= 1e-12
        other = np.ones(G.NN, bool)
        other[rows] = False
        assert np.array_equal(ref["memory"][other], x["memory"][other].astype(np.float64))
        assert np.array_equal(ref["last_update"][rows], x["timestamps"][rows])
        assert np.array_equal(ref["last_update"][other], x["last_update"][other])
        h = np.tanh(ref["pre"]["n"])
        if cell == "gru":
            z = 1.0 / (1.0 + np.exp(-ref["pre"]["z"]))
            h = (1.0 - z) * h + z * x["memory"][rows]
        assert np.abs(h - want).max() <= 1e-12                               # the pre-activations are the cell's


@pytest.mark.parametrize("D,msg", [(100, 472), (20, 59), (128, 456)])
def test_cell_update_is_the_c_oracle_gru(oracle, D, msg):
    """MemoryOracle.gru_update refuses ids out of range, so the awkward list goes in without its two: repeats, unflagged
    ids, node 0 and node NN - 1, flags beside the list.  Within the oracle's own float32: 1e-5 max(1, max|ref|)."""
    x = G.make_cell_inputs("gru", D, msg)                                    # (20, 59): nothing a multiple of 16
    il = G.id_list(x["perm"], 40, "awkward")
    ids = il["ids"][: il["n_dev"]]
    ids = ids[(ids >= 0) & (ids < G.NN)]
    flags = _flags(il)
    ref = M64.cell_update("gru", x["memory"], x["last_update"], x["messages"], x["timestamps"], flags, ids, len(ids),
                          x["w_ih"], x["w_hh"], x["b_ih"], x["b_hh"])
    mo = oracle.MemoryOracle(G.NN, D, msg)
    mo.memory[:], mo.last_update[:], mo.messages[:], mo.timestamps[:] = x["memory"], x["last_update"], x["messages"], x["timestamps"]
    mo.flags[:] = flags
    assert mo.gru_update({kk: x[kk] for kk in ("w_ih", "w_hh", "b_ih", "b_hh")}, ids) == len(ref["rows"])
    assert len(ref["rows"]) < len(np.unique(ids)) < len(ids)                 # unflagged ids and repeats went in
    assert np.abs(mo.memory - ref["memory"]).max() <= 1e-5 * max(1.0, np.abs(ref["memory"]).max())
    assert np.array_equal(mo.last_update, ref["last_update"])
    assert np.array_equal(mo.flags, ref["flags"]) and ref["flags"].sum() >= 50


@pytest.mark.parametrize("B", G.STORE_B)
@pytest.mark.parametrize("D,F,T", G.STORE_SHAPES, ids=["%d-%d-%d" % s for s in G.STORE_SHAPES])
def test_store_messages_is_the_c_oracle(oracle, D, F, T, B):
    """Copy columns, timestamps, flags: equal.  Time columns: the oracle's cosf of the same float32 product, within two
    units in the last place of 1 (2^-22) of float64's cos."""
    x = G.make_store_inputs(D, F, T, B)
    ref = G.store_reference(D, F, T, B, True)
    mo = oracle.MemoryOracle(G.NN, D, 2 * D + F + T)
    mo.memory[:], mo.last_update[:], mo.messages[:], mo.timestamps[:] = x["memory"], x["last_update"], x["messages"], x["timestamps"]
    mo.flags[:] = x["flags"]
    assert mo.store_messages(x["efeat"], I.time_encode_weights(T), x["src"], x["dst"], x["ts"], x["eidx"]) == len(ref["nodes"])
    nodes, C = ref["nodes"], 2 * D + F
    assert len(set(nodes.tolist())) == len(nodes) and set(nodes.tolist()) == set(x["src"].tolist()) | set(x["dst"].tolist())
    assert np.array_equal(mo.messages[nodes][:, :C], ref["rows"][:, :C].astype(np.float32))
    assert np.array_equal(ref["rows"][:, :C].astype(np.float32).astype(np.float64), ref["rows"][:, :C])
    assert np.abs(mo.messages[nodes][:, C:] - ref["rows"][:, C:]).max() <= 2.0 ** -22
    assert np.array_equal(mo.timestamps[nodes], ref["ts"])
    want = x["flags"].copy()
    want[nodes] = 1
    assert np.array_equal(mo.flags, want)
    other = np.ones(G.NN, bool)
    other[nodes] = False
    assert np.array_equal(mo.messages[other], x["messages"][other])
    # a shard: the same rows, of the winners whose position falls into it
    lo, hi = G.store_shard(B)
    part = G.store_reference(D, F, T, B, False)
    keep = (ref["pos"] >= lo) & (ref["pos"] < hi)
    assert np.array_equal(part["nodes"], nodes[keep]) and np.array_equal(part["rows"], ref["rows"][keep])
    assert np.array_equal(part["winner"], ref["winner"])
    if B >= 7:
        assert 0 < keep.sum() < len(keep)


def test_run_batches_is_store_then_update():
    """The composition against its two parts called by hand (float32 tables between them: within float32's rounding)."""
    D, F, T, B = 20, 7, 12, 7
    x = G.make_store_inputs(D, F, T, B, 3)
    w = G.make_cell_inputs("gru", D, 2 * D + F + T)
    tw = I.time_encode_weights(T)
    batches = [tuple(x[kk][b * B:(b + 1) * B] for kk in ("src", "dst", "ts", "eidx")) for b in range(3)]
    out = M64.run_batches("gru", x["memory"], x["last_update"], x["efeat"], tw, batches, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"])
    mem, lu = x["memory"].copy(), x["last_update"].copy()
    messages, ts, flags = np.zeros((G.NN, 2 * D + F + T), np.float32), np.zeros(G.NN, np.float32), np.zeros(G.NN, np.uint8)
    for b, (src, dst, t, e) in enumerate(batches):
        s = M64.store_messages(mem, lu, x["efeat"], tw, src, dst, t, e)
        messages[s["nodes"]], ts[s["nodes"]], flags[s["nodes"]] = s["rows"], s["ts"], 1
        ids = np.concatenate([src, dst])
        u = M64.cell_update("gru", mem, lu, messages, ts, flags, ids, len(ids), w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"])
        mem, lu, flags = u["memory"].astype(np.float32), u["last_update"], u["flags"]
        assert np.abs(out[b]["memory"] - mem).max() <= 1e-6 * max(1.0, np.abs(mem).max())
        assert np.array_equal(out[b]["last_update"], lu) and np.array_equal(out[b]["rows"], u["rows"])
        assert not out[b]["flags"].any()


# ------------------------------------------------------------------------------------- conditions on the GPU file's inputs --
def test_a_listed_shape_for_every_residue_of_the_k_step_count():
    steps = [G.chunk_steps(D, msg) for D, msg, _ in G.CELL_SHAPES]
    assert steps == [37, 26, 38, 38, 38, 39, 34, 35, 37, 74, 74, 19, 2, 6, 39, 50, 67, 61]
    assert {s % G.GRU_CH for s in steps} == set(range(G.GRU_CH))


def test_awkward_id_list_is_what_it_says():
    perm = G.make_cell_inputs("gru", 4, 13)["perm"]
    assert 0 not in perm and G.NN - 1 not in perm and len(set(perm.tolist())) == G.NN - 2
    prev = None
    for n in G.ROWS + (G.ROWS_PAST_SWITCH,):
        il = G.id_list(perm, n, "awkward")
        ids, flagged = il["ids"], set(il["flagged"].tolist())
        assert il["n_ids"] == len(ids) == n + 3 and il["n_dev"] == n
        assert ids[0] == 0 and 0 in flagged
        assert all(int(v) in flagged for v in ids[n:])                       # the tail is flagged, and must be ignored
        if prev is not None:
            assert np.array_equal(ids[: len(prev)], prev)                    # a smaller n is a prefix of a larger one
        prev = ids[:n].copy()
        if n >= 16:
            head = ids[:n]
            assert head[1] == G.NN - 1 and G.NN - 1 in flagged and head[2] < 0 and head[3] >= G.NN
            assert all(head[i] == head[i - 4] for i in range(4, n, 5))
            unfl = [int(v) for v in head[7::10]]
            assert unfl and not any(v in flagged for v in unfl) and len(unfl) >= n // 10
        plain = G.id_list(perm, n, "plain")
        assert len(set(plain["ids"].tolist())) == n and set(plain["ids"].tolist()) < set(plain["flagged"].tolist())
    assert not set(G.id_list(perm, 40, "plain", 700)["ids"].tolist()) & set(G.id_list(perm, 40, "plain")["ids"].tolist())


@pytest.mark.parametrize("cell", G.CELLS)
@pytest.mark.parametrize("D,msg", [s[:2] for s in G.CELL_SHAPES], ids=["%d-%d" % s[:2] for s in G.CELL_SHAPES])
def test_torch_float32_is_within_half_the_tolerance(D, msg, cell):
    """The condition the plain tolerance rests on: torch's float32 cell (here on the CPU) within half of it, on every plain
    case and every call of it."""
    x = G.make_cell_inputs(cell, D, msg)
    assert np.abs(x["memory"]).min() > 0 and np.abs(x["last_update"]).min() > 0 and np.abs(x["timestamps"]).min() > 0
    worst = 0.0
    for n, kind in G._cases(D, msg):
        for step, (_, changed) in enumerate(G.cell_steps(n, kind)):
            ref = G.cell_reference(cell, D, msg, False, n, kind, step)
            rows = ref["rows"]
            c = G.torch_cell(cell, D, msg, x["w2"] if changed else x)
            with torch.no_grad():
                got = c(G._t(x["messages"][rows]), G._t(x["memory"][rows])).numpy()
            e = float(np.abs(got - ref["memory"][rows]).max())
            worst = max(worst, e)
            assert e <= 0.5 * G.plain_tolerance(ref), (n, kind, step, e)
            assert np.isfinite(ref["memory"]).all()
    print("%s D=%d msg=%d: torch float32 on the CPU %.2e" % (cell, D, msg, worst))


@pytest.mark.parametrize("cell", G.CELLS)
@pytest.mark.parametrize("D,msg", G.STRESS_SHAPES, ids=["%d-%d" % s for s in G.STRESS_SHAPES])
def test_stress_rows_are_what_they_say(D, msg, cell):
    x, plain = G.make_cell_inputs(cell, D, msg, True), G.make_cell_inputs(cell, D, msg)
    rows = x["perm"][: G.STRESS_ROWS]
    assert msg >= (3 if cell == "gru" else 1) * D                            # the least-norm message exists
    assert np.abs(x["messages"][rows[:10]]).max() > 200 and np.abs(x["memory"][rows[10:20]]).max() > 15
    ref = G.cell_reference(cell, D, msg, True, G.STRESS_ROWS, "plain", 0)
    pos = {int(v): i for i, v in enumerate(ref["rows"])}
    sat = np.array([pos[int(v)] for v in rows[G.SAT]])
    assert min(np.abs(p[sat]).min() for p in ref["pre"].values()) > 40.0
    limit = M64.saturated_limit(cell, {k: p[sat] for k, p in ref["pre"].items()}, x["memory"][ref["rows"]][sat].astype(np.float64))
    assert np.abs(ref["memory"][ref["rows"]][sat] - limit).max() <= 1e-12
    if cell == "gru":                                                        # both limits occur
        assert (ref["pre"]["z"][sat] > 0).any() and (ref["pre"]["z"][sat] < 0).any()
    assert np.isfinite(ref["memory"]).all()
    c = G.torch_cell(cell, D, msg, x)
    with torch.no_grad():
        got = c(G._t(x["messages"][ref["rows"]]), G._t(x["memory"][ref["rows"]])).numpy()
    print("%s D=%d msg=%d stress: torch float32 on the CPU %.2e" % (cell, D, msg, np.abs(got - ref["memory"][ref["rows"]]).max()))
    assert np.isfinite(got).all() and plain is not x


@pytest.mark.parametrize("D,F,T", G.STORE_SHAPES, ids=["%d-%d-%d" % s for s in G.STORE_SHAPES])
def test_store_inputs_are_what_they_say(D, F, T):
    for B in G.STORE_B:
        x = G.make_store_inputs(D, F, T, B)
        assert np.abs(x["efeat"]).min() > 0 and np.abs(x["memory"]).min() > 0 and np.abs(x["last_update"]).min() > 0
        assert x["eidx"][0] == 0 and x["ts"].dtype == np.float64 and x["ts"].min() > 2 ** 24
        assert (x["ts"].astype(np.float32).astype(np.float64) != x["ts"]).all()          # .float() rounds every one
        ref = G.store_reference(D, F, T, B, True)
        i = np.where(ref["pos"] < B, ref["pos"], ref["pos"] - B)
        dt = x["ts"][i].astype(np.float32) - x["last_update"][ref["nodes"]]
        assert (dt == 0).any() and dt.min() >= 0
        if B >= 7:
            both = np.concatenate([x["src"], x["dst"]])
            assert (both == 11).sum() >= 3 and (x["src"] == x["dst"]).any()
            assert x["dst"][1] == 13 and x["src"][5] == 13 and ref["winner"][13] == B + 1
            assert (dt < 4e6).any() and (dt > 4e6).any() and 3e8 <= dt.max() < 3.1e8
        if B == 600:
            assert (dt[dt > 0] < 4e6).sum() > 100 and (dt > 4e6).sum() > 100


# ---------------------------------------------------------------------------------------- the kernel each GPU case reaches --
@pytest.mark.parametrize("D,msg", [s[:2] for s in G.CELL_SHAPES], ids=["%d-%d" % s[:2] for s in G.CELL_SHAPES])
def test_cell_cases_reach_the_kernel_their_name_says(hooks, D, msg):
    perm = G.make_cell_inputs("gru", D, msg)["perm"]
    seen = set()
    cases = G._cases(D, msg) + ([(G.STRESS_ROWS, "plain"), (G.STRESS_ROWS, "awkward")] if (D, msg) in G.STRESS_SHAPES else [])
    for n, kind in cases:
        il = G.id_list(perm, n, kind)
        rows = G.NN if il["ids"] is None else il["n_ids"]
        for form, choice in G.FORMS:
            p = LP.memory_plan(hooks, rows, D, msg, gru_choice=choice)
            want, ntw = G.expected_form(D, msg, rows, choice)
            assert p["refusal"] == LP.REFUSAL["none"] and p["gru"] == LP.GRU[want], (n, kind, form)
            assert p["NTg"] == (D + 15) // 16 and (p["NTg"] > 8) == (ntw == 2)
            assert p["gru_tiles"] == (rows + 15) // 16
            seen.add(want)
    split_ok = {(d, m): ok for d, m, ok in G.CELL_SHAPES}[(D, msg)]
    assert seen == ({"tile", "split"} if split_ok else {"tile"})


def test_both_sides_of_every_seam_are_listed(hooks):
    """The pairs the GPU list is built around do part ways in the plan (were a bound to move, a pair would no longer
    straddle it)."""
    form = lambda D, msg, rows=40, c=0: LP.memory_plan(hooks, rows, D, msg, gru_choice=c)["gru"]
    S, Tl = LP.GRU["split"], LP.GRU["tile"]
    assert (form(100, 492), form(100, 493)) == (S, Tl)                       # the staging bound
    assert (form(1, 577), form(1, 593)) == (S, Tl)                           # the chunk bound
    assert (form(112, 425), form(113, 427), form(113, 427, c=LP.GRU_SPLIT)) == (S, Tl, Tl)
    assert (form(100, 472, 512), form(100, 472, 513), form(100, 472, 516)) == (S, Tl, Tl)    # the row switch
    assert LP.memory_plan(hooks, 40, 100, 1073)["refusal"] == LP.REFUSAL["msg_wide"]
    assert LP.memory_plan(hooks, 40, 128, 1057)["refusal"] == LP.REFUSAL["msg_wide"]
    assert LP.memory_plan(hooks, 40, 129, 400)["refusal"] == LP.REFUSAL["d_large"]


@pytest.mark.parametrize("D,F,T", G.STORE_SHAPES + G.COMPOSED, ids=["%d-%d-%d" % s for s in G.STORE_SHAPES + G.COMPOSED])
def test_message_cases_reach_the_kernel_their_name_says(hooks, D, F, T):
    two = D <= 128 and T <= 128 and F <= 256
    msg = 2 * D + F + T
    assert LP.memory_plan(hooks, 40, D, msg, F=F, T=T)["msg"] == LP.MSGK["two" if two else "one"]
    assert LP.memory_plan(hooks, 40, D, msg, F=F, T=T, msg_choice=LP.MSG_ONE)["msg"] == LP.MSGK["one"]
    if (D, F, T) in G.COMPOSED:                                              # 2 B ids to the update
        p = LP.memory_plan(hooks, 2 * G.COMPOSED_B, D, msg, F=F, T=T)
        assert p["refusal"] == LP.REFUSAL["none"] and p["gru"] == LP.GRU["split" if D <= 112 else "tile"]


def test_message_seams_are_straddled():
    kinds = {(D <= 128, F <= 256, T <= 128) for D, F, T in G.STORE_SHAPES}
    assert kinds == {(True, True, True), (False, True, True), (True, False, True), (True, True, False)}
    assert (128, 256, 128) in G.STORE_SHAPES                                 # the last width of each that takes two positions


# test_fused_output_and_gru_launch_matches_separate_kernels (tests/test_embed_gpu.py) at D = 128: (F, bs)
@pytest.mark.parametrize("F,bs,want", [(16, 400, "fused_tile"), (16, 150, "front")])
def test_one_launch_forms_at_d128(hooks, F, bs, want):
    """What the pipelined step of that test reaches at D = 128 (2 bs ids to the update, 3 bs output rows).  bs = 400: the
    tile beside the tiled output layers, ONE launch (k_out_gru).  bs = 150: Hp = 128 does not fit the split's commit
    (16 Hp <= 7 * 256), so the update is the tile, the output layers are latency-organised, and they run in front of it:
    no width reaches k_out_gru2's NTg = 8 instantiation (at D <= 112, NTg = 7: the one-launch split of the test's
    D = 100 cases)."""
    D, T, M, k = 128, 100, 2, 20
    _, out, _ = LP.plan(hooks, 3 * bs, D, F, T, M, k, True)
    form = {v: kk for kk, v in LP.OUT.items()}[out]
    assert form == ("tiled" if bs == 400 else "latency")
    p = LP.memory_plan(hooks, 2 * bs, D, 2 * D + F + T, F=F, T=T, held=(form, 1, D, M, 38, 3 * bs, True))
    assert p["refusal"] == LP.REFUSAL["none"] and p["gru"] == LP.GRU["tile"] and p["NTg"] == 8
    assert p["out"] == LP.HELD[want]
    if bs == 150:      # the same rows at D = 100 do take the one-launch split
        q = LP.memory_plan(hooks, 2 * bs, 100, 300 + F, F=F, T=T, held=("latency", 1, 100, M, 38, 3 * bs, True))
        assert (q["gru"], q["out"], q["NTg"]) == (LP.GRU["split"], LP.HELD["fused_split"], 7)
