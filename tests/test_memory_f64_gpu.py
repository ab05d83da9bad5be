"""The eval-time memory path -- zt_store_messages (k_last_pos, k_build_messages, k_build_messages2) and zt_gru_update /
zt_rnn_update (k_select_flagged, k_pack_gates, k_gru<CELL, 1 | 2>, k_gru_split) -- against the plain float64 restatement
oracle/memory_f64.py (pinned to torch's float64 cells and to the C oracle in tests/test_memory_f64_cpu.py), at every
width where zt::memory_kernel_plan or a kernel's own loop changes.

Inputs: this file's own seeded generators (make_cell_inputs, make_store_inputs), NOT inputs.random_tables: edge features
are non-zero at every F, row 0 included; memory and last_update are non-zero; the edge times are float64 above 2^24, so
.float() rounds; dt = f32(t) - last_update falls on both sides of the cosine's 4e6 switch, reaches 3e8 and is 0 once.  The
special rows sit at fixed positions from row 0 on: a smaller n is a prefix of a larger one.

The cell.  GRUMemoryUpdater / RNNMemoryUpdater.update_device over a bare Memory (no TGN: the message width need not be
2 D + F + T) of NN = 3001 nodes (not a multiple of 4: the last flag word is partial), the tile pinned, the split pinned, and
the library's pick, on n = 1, 16, 17, 40 ids (one row, a full tile, a tile plus one, a ragged third tile; 513 once, past the
row switch).  Each with the plain list and with an awkward one: node 0 and node NN - 1, both flagged; every fifth id a
repeat; a tenth of the ids unflagged; one negative id and one >= NN; and a count on the device smaller than n_ids, whose
tail must be ignored.  Per case three calls on ONE workspace: the first packs the weights, the second (other ids and flags)
finds them packed, the third follows a weight changed in place.
The shapes (D, msg) in CELL_SHAPES: (Xp + Hp) / 16, the number of 16-column k-steps of [message | memory], takes every
residue modulo GRU_CH = 6 across them -- 37 26 38 38 38 39 34 35 37 74 74 19 2 6 39 50 67 61, residues 1 2 2 2 2 3 4 5 1 2 2
1 2 0 3 2 1 1 (asserted in the CPU file).

Tolerances against float64, none fitted to the kernels:
  plain cases   1e-5 max(1, max|ref|): the number test_gru_kernels_agree and test_hip_gru_rows_against_float64 assert for
                this cell.  torch's float32 cell on the device, same inputs, is held to HALF of it (what shows the reference
                method has room); torch float32 on the CPU within half is a condition on the inputs, asserted in the CPU file.
                The D = 1 rows draw their weights in +- 1/4 (at +- 1 torch float32 itself reaches 5.3e-6).
  stress cases  messages x 100 on some rows, memory x 30 on others, a block of rows whose float64 pre-activations all
                exceed 40: four times the error torch's float32 cell on the device makes against float64 on the same case
                (another summation order over up to 1 172 terms), the plain tolerance as floor; every output finite; on
                the saturated rows h' within 1e-6 max(1, |h|) of the limit float64 gives.
  messages      memory and edge-feature columns and the timestamps equal to the bit; time columns within 2e-6, the bound
                test_time_encode_through_message_kernel asserts.

Measured on an MI355X (max |error| against float64; per shape in DESIGN.md, "The memory path against float64"): plain cases --
kernels 1.2e-07 ... 3.6e-06 (the RNN at (100, 1072)), torch 9.7e-08 ... 3.1e-06 (the RNN at (1, 593)), tolerance 1e-5 at every shape
(max|ref| <= 1); torch float32 on the CPU 1.1e-07 ... 2.7e-06, so no case needed its messages scaled down (MSG_SCALE is empty).
Stress cases -- kernels 2.1e-05 ... 8.8e-05, torch 1.2e-05 ... 8.7e-05, the kernels at most 1.8 times torch.  Messages -- time columns
6.8e-08 ... 2.8e-07.  Composition -- 2.1e-07 ... 1.7e-06.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

NN = 3001                                   # nodes: not a multiple of 4
E1 = 2000                                   # edge-feature rows
GRU_CH = 6                                  # csrc/memory_update.hip: k-steps of weight fragments in flight
CELLS = ("gru", "rnn")
ROWS = (1, 16, 17, 40)
ROWS_PAST_SWITCH = 513                      # once, at (100, 472): the library's pick turns from the split to the tile
TOL = 1e-5
MSG_SCALE = {}                              # (D, msg) -> constant on the messages of a case, were torch on the device to miss its half
# (D, msg, the split takes it -- else a pinned split falls back to the tile)
CELL_SHAPES = [
    (100, 472, True), (100, 301, True),                  # C2 / C3, C4 / C5
    (100, 492, True), (100, 493, False),                 # the staging bound: 16 (msg + D) = 37 * 256, and one more
    (1, 577, True), (1, 593, False),                     # the chunk bound
    (112, 425, True), (113, 427, False), (128, 456, False),      # 16 Hp <= 7 * 256; Hp = 128: no padded column
    (128, 1056, False), (100, 1072, False),              # the widest messages taken
    (64, 236, True), (4, 13, True), (16, 80, True),
    (132, 465, False), (172, 616, False), (252, 805, False), (256, 712, False),     # k_gru<CELL, 2>: 9, 11, 16, 16 N-tiles
]
STRESS_SHAPES = [(100, 472), (128, 456), (172, 616)]
STRESS_ROWS = 40
SAT = slice(20, 30)                         # the rows of the stress list whose pre-activations all exceed 40
# (D, F, T): C4 / C5, C2 / C3, then a seam each -- D = 128 | 132, F = 256 | 257, T = 128 | 129 -- and small odd ones
STORE_SHAPES = [(100, 1, 100), (100, 172, 100), (128, 256, 128), (132, 4, 100), (100, 257, 100), (100, 4, 129),
                (20, 7, 12), (4, 1, 4)]
STORE_B = (1, 7, 600)
COMPOSED = [(100, 1, 100), (128, 16, 128), (172, 172, 172)]


def oracle():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import memory_f64
    return memory_f64


def _t(a):
    """a tensor over a copy (the generators hand out read-only arrays)"""
    return torch.from_numpy(np.array(a))


def chunk_steps(D, msg):
    """(Xp + Hp) / 16: the 16-column k-steps of a [message | memory] row."""
    return ((msg + 15) // 16 * 16 + (D + 15) // 16 * 16) // 16


def expected_form(D, msg, rows, choice):
    """The kernel a case's name says: choice 0 (the library's pick), 1 (ZT_GRU_TILE), 2 (ZT_GRU_SPLIT); rows = the ids
    handed to the update.  (form, N-tiles per wave of k_gru)"""
    split_ok = {(d, m): ok for d, m, ok in CELL_SHAPES}[(D, msg)]
    split = split_ok and (choice == 2 or (choice == 0 and rows <= 512))
    return ("split" if split else "tile"), (2 if D > 128 else 1)


# ------------------------------------------------------------------------------------------------------------ the cell --
@functools.lru_cache(maxsize=4)
def make_cell_inputs(cell, D, msg, stress=False):
    """The one seeded generator of the cell's cases (numpy, float32): weights in torch's own init range +- 1 / sqrt(D)
    (D = 1: +- 1 / 4), randn messages, memory x 0.3, timestamps and last_update non-zero; perm: the node order the id
    lists are cut from (nodes 1 .. NN - 2: nodes 0 and NN - 1 enter through the awkward list alone)."""
    rng = np.random.RandomState(9000 + 131 * D + msg + (7 if cell == "rnn" else 0) + (100003 if stress else 0))
    G = 3 if cell == "gru" else 1
    s = 0.25 if D == 1 else 1.0 / np.sqrt(D)
    x = {"w_ih": rng.uniform(-s, s, (G * D, msg)).astype(np.float32),
         "w_hh": rng.uniform(-s, s, (G * D, D)).astype(np.float32),
         "b_ih": rng.uniform(-s, s, G * D).astype(np.float32), "b_hh": rng.uniform(-s, s, G * D).astype(np.float32)}
    x["messages"] = (rng.standard_normal((NN, msg)) * MSG_SCALE.get((D, msg), 1.0)).astype(np.float32)
    x["memory"] = (rng.standard_normal((NN, D)) * 0.3).astype(np.float32)
    x["memory"][x["memory"] == 0] = 0.25
    x["timestamps"] = (rng.rand(NN) * 1.0e6 + 1.0).astype(np.float32)
    x["last_update"] = (rng.rand(NN) * 9.0e4 + 1.0).astype(np.float32)
    x["perm"] = rng.permutation(np.arange(1, NN - 1))
    # the weights a case's third call runs with
    x["w2"] = {"w_ih": (x["w_ih"] * np.float32(-0.5)).astype(np.float32), "w_hh": x["w_hh"][::-1].copy(),
               "b_ih": (x["b_ih"] + np.float32(0.05)).astype(np.float32), "b_hh": x["b_hh"][::-1].copy()}
    if stress:
        rows = x["perm"][:STRESS_ROWS]
        x["messages"][rows[0:10]] *= 100.0
        x["memory"][rows[10:20]] *= 30.0
        # saturated rows: the least-norm message with W_ih x = t, |t| in 50 .. 70 with random signs (msg >= G D at these
        # shapes); biases and the memory part (memory x 0.3) move a pre-activation by a few units at most
        t = rng.uniform(50.0, 70.0, (10, G * D)) * rng.choice([-1.0, 1.0], (10, G * D))
        sol = np.linalg.lstsq(x["w_ih"].astype(np.float64), t.T, rcond=None)[0]
        x["messages"][rows[SAT]] = sol.T.astype(np.float32)
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


def id_list(perm, n, kind, shift=0):
    """kind "plain": n distinct flagged ids.  "awkward": n considered ids -- position 0: node 0, 1: node NN - 1 (both
    flagged), 2: a negative id, 3: an id >= NN, every position 4 mod 5: a repeat of the id four places before, every
    position 7 mod 10: unflagged -- followed by three FLAGGED ids beyond the count on the device.  "all": ids = None.
    Beside the list, flags are set on nodes the list does not name.  shift: another cut of perm (a case's second call).
    Returns ids (int32 or None), n_ids, n_dev (None: no count on the device) and flagged (the nodes whose flag is set)."""
    base = perm[shift: shift + n].astype(np.int64)
    unlisted = perm[2000:2050]
    if kind == "plain":
        return {"ids": base.astype(np.int32), "n_ids": n, "n_dev": None, "flagged": np.concatenate([base, unlisted])}
    if kind == "all":
        return {"ids": None, "n_ids": 0, "n_dev": None, "flagged": np.concatenate([base, [0, NN - 1]])}
    a = base.copy()
    for i, v in enumerate((0, NN - 1, -7, NN + 5)):
        if i < n:
            a[i] = v
    for i in range(4, n):
        if i % 5 == 4:
            a[i] = a[i - 4]
    unflagged = a[7::10]
    tail = perm[2100:2103]
    ok = a[(a >= 0) & (a < NN)]
    flagged = np.concatenate([np.setdiff1d(ok, unflagged), unlisted, tail])
    return {"ids": np.concatenate([a, tail]).astype(np.int32), "n_ids": n + 3, "n_dev": n, "flagged": flagged}


def cell_steps(n, kind):
    """The three calls of a case: (id list's cut of perm, second weight set)"""
    return [(0, False), (700, False), (0, True)]


def cell_reference(cell, D, msg, stress, n, kind, step):
    """float64; a test computes it once per case and shares it among the three forms: every call starts from the
    generator's tables."""
    x = make_cell_inputs(cell, D, msg, stress)
    shift, changed = cell_steps(n, kind)[step]
    il = id_list(x["perm"], n, kind, shift)
    flags = np.zeros(NN, np.uint8)
    flags[il["flagged"]] = 1
    w = x["w2"] if changed else x
    n_considered = il["n_dev"] if il["n_dev"] is not None else il["n_ids"]
    ref = oracle().cell_update(cell, x["memory"], x["last_update"], x["messages"], x["timestamps"], flags, il["ids"],
                               n_considered, w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"])
    ref["flags_before"] = flags
    ref["il"] = il
    return ref


def torch_cell(cell, D, msg, w, device="cpu", dtype=torch.float32):
    c = (torch.nn.GRUCell if cell == "gru" else torch.nn.RNNCell)(msg, D)
    with torch.no_grad():
        for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            getattr(c, name).copy_(_t(w[key]))
    return c.to(device=device, dtype=dtype)


def plain_tolerance(ref):
    rows = ref["rows"]
    return TOL * max(1.0, float(np.abs(ref["memory"][rows]).max()) if len(rows) else 1.0)


class _Device:
    """A bare Memory and its updater on the device, with the generator's tables beside them."""

    def __init__(self, cell, D, msg, x):
        from zebra_amd.modules import GRUMemoryUpdater, Memory, RNNMemoryUpdater
        self.cell, self.x = cell, x
        self.m = Memory(n_nodes=NN, memory_dimension=D, input_dimension=msg, message_dimension=msg, device="cuda")
        self.upd = (GRUMemoryUpdater if cell == "gru" else RNNMemoryUpdater)(msg, D, "cuda").to("cuda")
        self.mem0 = _t(x["memory"]).cuda()
        self.lu0 = _t(x["last_update"]).cuda()
        self.m.messages.copy_(_t(x["messages"]).cuda())
        self.m.timestamps.copy_(_t(x["timestamps"]).cuda())
        self.current = None
        self.set_weights(False)

    def set_weights(self, changed):
        if self.current == changed:
            return
        w = self.x["w2"] if changed else self.x
        g = self.upd.memory_updater
        with torch.no_grad():                           # in place: the parameters keep their storage, their version moves
            for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
                getattr(g, name).copy_(_t(w[key]))
        self.current = changed

    def run(self, il):
        """One update_device from the generator's tables; what it left, on the host."""
        m = self.m
        m.memory.copy_(self.mem0)
        m.last_update.copy_(self.lu0)
        m._flag_buf.zero_()
        m._flag_buf[_t(il["flagged"]).cuda()] = 1
        ids_d = _t(il["ids"]).cuda() if il["ids"] is not None else None
        n_dev = torch.tensor([il["n_dev"]], dtype=torch.int32, device="cuda") if il["n_dev"] is not None else None
        self.upd.update_device(m, ids_d, il["n_ids"], n_dev)
        torch.cuda.synchronize()
        rows, count = self.upd.last_rows()
        return {"memory": m.memory.cpu().numpy(), "last_update": m.last_update.cpu().numpy(),
                "flags": m._flag_buf.cpu().numpy(), "rows": rows[: int(count.item())].cpu().numpy()}

    def torch_rows(self, rows):
        """torch's float32 cell on the device, on the same rows of the same tables"""
        r = _t(rows).cuda()
        with torch.no_grad():
            return self.upd.memory_updater(self.m.messages[r], self.mem0[r]).cpu().numpy()


def check_update(got, ref, x, tol, what):
    """Everything but the new rows' values against float64; returns the kernels' max |error| on them."""
    rows, il = ref["rows"], ref["il"]
    assert np.array_equal(np.sort(got["rows"]), rows), what                 # exactly the oracle's rows, each once
    untouched = np.ones(NN, bool)
    untouched[rows] = False
    assert np.array_equal(got["memory"][untouched], x["memory"][untouched]), what      # unflagged, beyond the count, not listed
    assert np.array_equal(got["last_update"], ref["last_update"]), what
    assert np.array_equal(got["flags"][:NN], ref["flags"]), what            # considered: cleared; every other flag: as it was
    assert not got["flags"][NN:].any(), what
    if il["ids"] is not None:
        assert ref["flags"].sum() >= 50, what                                # (flags outside the list were there to be kept)
    err = float(np.abs(got["memory"][rows] - ref["memory"][rows]).max()) if len(rows) else 0.0
    assert np.isfinite(got["memory"]).all(), what
    assert err <= tol, (what, err, tol)
    return err


def _cases(D, msg):
    cases = [(n, kind) for n in ROWS for kind in ("plain", "awkward")]
    if (D, msg) == (100, 472):
        cases += [(ROWS_PAST_SWITCH, "plain"), (ROWS_PAST_SWITCH, "awkward")]
    if D == 100 and msg in (472, 301):
        cases.append((40, "all"))                                            # ids = None: every node is considered
    return cases


FORMS = (("tile", 1), ("split", 2), ("auto", 0))                             # ZT_GRU_TILE, ZT_GRU_SPLIT, the library's pick


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("D,msg", [s[:2] for s in CELL_SHAPES], ids=["%d-%d" % s[:2] for s in CELL_SHAPES])
def test_cell_against_float64(D, msg, cell):
    from zebra_amd import _capi
    x = make_cell_inputs(cell, D, msg)
    dev = _Device(cell, D, msg, x)
    worst, worst_torch, worst_tol = 0.0, 0.0, np.inf
    try:
        for n, kind in _cases(D, msg):
            refs = [cell_reference(cell, D, msg, False, n, kind, step) for step in range(3)]
            for step, ref in enumerate(refs):                                # torch float32 on the device: half the tolerance
                dev.set_weights(cell_steps(n, kind)[step][1])
                tol = plain_tolerance(ref)
                e = float(np.abs(dev.torch_rows(ref["rows"]) - ref["memory"][ref["rows"]]).max())
                worst_torch, worst_tol = max(worst_torch, e), min(worst_tol, tol)
                assert e <= 0.5 * tol, ("torch", n, kind, step, e, tol)
            for form, choice in FORMS:
                _capi.set_kernel_choice(_capi.CHOICE_GRU, choice)
                for step, ref in enumerate(refs):
                    dev.set_weights(cell_steps(n, kind)[step][1])
                    got = dev.run(ref["il"])
                    worst = max(worst, check_update(got, ref, x, plain_tolerance(ref), (form, n, kind, step)))
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_GRU, 0)
    print("%s D=%d msg=%d: kernels %.2e torch %.2e tolerance >= %.2e" % (cell, D, msg, worst, worst_torch, worst_tol))


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("D,msg", STRESS_SHAPES, ids=["%d-%d" % s for s in STRESS_SHAPES])
def test_cell_stress_rows(D, msg, cell):
    from zebra_amd import _capi
    x = make_cell_inputs(cell, D, msg, True)
    dev = _Device(cell, D, msg, x)
    worst, worst_torch = 0.0, 0.0
    try:
        for kind in ("plain", "awkward"):
            ref = cell_reference(cell, D, msg, True, STRESS_ROWS, kind, 0)
            rows = ref["rows"]
            pos = {int(v): i for i, v in enumerate(rows)}
            sat = np.array([pos[int(v)] for v in x["perm"][:STRESS_ROWS][SAT] if int(v) in pos])
            assert len(sat) >= 5
            assert min(np.abs(p[sat]).min() for p in ref["pre"].values()) > 40.0
            assert max(np.abs(p).max() for p in ref["pre"].values()) > 200.0                 # the scaled rows reach far
            h = x["memory"][rows].astype(np.float64)
            limit = oracle().saturated_limit(cell, {k: p[sat] for k, p in ref["pre"].items()}, h[sat])
            assert np.abs(ref["memory"][rows][sat] - limit).max() <= 1e-12                  # float64 is at its limit there
            tq = dev.torch_rows(rows)
            e_torch = float(np.abs(tq - ref["memory"][rows]).max())
            tol = max(4.0 * e_torch, plain_tolerance(ref))
            worst_torch = max(worst_torch, e_torch)
            for form, choice in FORMS:
                _capi.set_kernel_choice(_capi.CHOICE_GRU, choice)
                got = dev.run(ref["il"])
                worst = max(worst, check_update(got, ref, x, tol, (form, kind)))
                new = got["memory"][rows][sat].astype(np.float64)
                assert (np.abs(new - limit) <= 1e-6 * np.maximum(1.0, np.abs(h[sat]))).all(), (form, kind)
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_GRU, 0)
    print("%s D=%d msg=%d stress: kernels %.2e torch %.2e" % (cell, D, msg, worst, worst_torch))


# -------------------------------------------------------------------------------------------------------- the messages --
@functools.lru_cache(maxsize=8)
def make_store_inputs(D, F, T, B, batches=1):
    """The one seeded generator of the message cases (numpy).  Edge features non-zero at every F, row 0 included (edge 0
    is named at position 0); memory, last_update, and the tables' contents before the call non-zero.  Edge times float64
    above 2^24 (3e8 and up: .float() rounds); last_update puts dt below 4e6 on half the nodes and up to 3e8 on the others,
    dt = 0 on node 19, the destination of edge 0, dt = f32(t) - 1.5 ~ 3e8 on node 13.  From B = 7 on: node 11 at many
    positions, self-loops, and node 13, a destination at edge 1 and a source at edge 5 -- its LAST position in
    [src | dst] is the destination's, although the source's edge is the later one.  batches > 1: B edges each, the
    times running on."""
    rng = np.random.RandomState(5000 + 131 * D + 17 * F + 5 * T + B)
    x = {"memory": rng.standard_normal((NN, D)).astype(np.float32), "efeat": rng.standard_normal((E1, F)).astype(np.float32),
         "messages": rng.standard_normal((NN, 2 * D + F + T)).astype(np.float32),
         "timestamps": (rng.rand(NN) * 1.0e5 + 1.0).astype(np.float32)}
    x["memory"][x["memory"] == 0] = 0.25
    x["efeat"][x["efeat"] == 0] = 0.25
    x["flags"] = (rng.rand(NN) < 0.1).astype(np.uint8)
    n = B * batches
    src, dst = rng.randint(0, NN, n).astype(np.int32), rng.randint(0, NN, n).astype(np.int32)
    for a in (src, dst):
        a[(a == 11) | (a == 13) | (a == 19)] = 17
    dst[0] = 19                                                           # node 19: this once, the winner of position B
    eidx = rng.randint(0, E1, n).astype(np.int64)
    eidx[0] = 0
    ts = 3.0e8 + np.cumsum(rng.rand(n) * 50.0) + 0.37
    for b in range(batches):
        s, d = src[b * B:(b + 1) * B], dst[b * B:(b + 1) * B]
        if B >= 7:
            s[::3] = 11
            d[6::50] = 11
            d[1], s[5] = 13, 13
            d[2::11] = s[2::11]
    lu = (np.float32(3.0e8) - rng.rand(NN) * 3.9e6).astype(np.float32)
    far = rng.rand(NN) < 0.5
    lu[far] = (rng.rand(int(far.sum())) * 2.9e8 + 1.0).astype(np.float32)
    lu[13] = 1.5
    lu[19] = np.float32(ts[0])                                            # dt = 0
    x.update(src=src, dst=dst, eidx=eidx, ts=ts, last_update=lu)
    for v in x.values():
        v.setflags(write=False)
    return x


def store_shard(B):
    return (B // 3, 2 * B - max(1, B // 5))


@functools.lru_cache(maxsize=8)
def store_reference(D, F, T, B, whole):
    import inputs as I
    x = make_store_inputs(D, F, T, B)
    return oracle().store_messages(x["memory"], x["last_update"], x["efeat"], I.time_encode_weights(T), x["src"], x["dst"],
                                   x["ts"], x["eidx"], pos_range=None if whole else store_shard(B))


def _store_tgn(D, F, T, efeat):
    import inputs as I
    from helpers import build_tgn
    tgn = build_tgn(NN, E1, D, F, T, 20, [0.1, 0.1], [0.5, 0.95], I.model_weights(D, F, T, 2, 5), efeat).eval()
    assert np.array_equal(tgn.time_encoder.w.weight.detach().cpu().numpy().ravel(), I.time_encode_weights(T))
    return tgn


def check_store(m, scratch, x, ref, D, F, what):
    """The tables after a store against the oracle's rows; returns the max |error| of the time columns."""
    nodes = ref["nodes"]
    msg, ts, flags = m.messages.cpu().numpy(), m.timestamps.cpu().numpy(), m._flag_buf.cpu().numpy()
    C = 2 * D + F
    assert np.array_equal(msg[nodes][:, :C], ref["rows"][:, :C].astype(np.float32)), what        # copies: to the bit
    assert np.array_equal(ts[nodes], ref["ts"]), what
    err = float(np.abs(msg[nodes][:, C:] - ref["rows"][:, C:]).max()) if len(nodes) else 0.0
    assert err <= 2e-6, (what, err)
    untouched = np.ones(NN, bool)
    untouched[nodes] = False                                                # the winners are the oracle's, no node more
    assert np.array_equal(msg[untouched], x["messages"][untouched]), what
    assert np.array_equal(ts[untouched], x["timestamps"][untouched]), what
    want = x["flags"].copy()
    want[nodes] = 1
    assert np.array_equal(flags[:NN], want) and not flags[NN:].any(), what
    assert bool((scratch == -1).all()), what
    return err


@pytest.mark.parametrize("B", STORE_B)
@pytest.mark.parametrize("D,F,T", STORE_SHAPES, ids=["%d-%d-%d" % s for s in STORE_SHAPES])
def test_messages_against_float64(D, F, T, B):
    from zebra_amd import _capi
    x = make_store_inputs(D, F, T, B)
    tgn = _store_tgn(D, F, T, x["efeat"])
    m = tgn.memory
    args = [_t(x[kk]).cuda() for kk in ("src", "dst", "ts", "eidx")]
    if B >= 7:                                                               # the batch is what the generator says it is
        both = np.concatenate([x["src"], x["dst"]])
        w = store_reference(D, F, T, B, True)["winner"]
        assert (both == 11).sum() >= 3 and (x["src"] == x["dst"]).any() and w[13] == B + 1 and x["src"][5] == 13
        dt = np.float32(x["ts"][np.where(w[w >= 0] < B, w[w >= 0], w[w >= 0] - B)]) - x["last_update"][w >= 0]
        assert (dt == 0).any() and (np.abs(dt) < 4e6).any() and (dt > 4e6).any() and dt.max() >= 3e8
    assert (np.float32(x["ts"]) != x["ts"]).all()
    worst = 0.0
    try:
        for mode, choice in (("auto", 0), ("one", _capi.MSG_ONE)):
            _capi.set_kernel_choice(_capi.CHOICE_MESSAGES, choice)
            for whole in (True, False):
                m.memory.copy_(_t(x["memory"]).cuda())
                m.last_update.copy_(_t(x["last_update"]).cuda())
                m.messages.copy_(_t(x["messages"]).cuda())
                m.timestamps.copy_(_t(x["timestamps"]).cuda())
                m._flag_buf.zero_()
                m._flag_buf[:NN] = _t(x["flags"]).cuda()
                tgn.store_messages_device(*args, pos_range=None if whole else store_shard(B))
                torch.cuda.synchronize()
                assert int(tgn._status.item()) == 0
                ref = store_reference(D, F, T, B, whole)
                worst = max(worst, check_store(m, tgn._scratch, x, ref, D, F, (mode, whole)))
                assert np.array_equal(m.memory.cpu().numpy(), x["memory"])
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_MESSAGES, 0)
    print("D=%d F=%d T=%d B=%d: time columns %.2e" % (D, F, T, B, worst))


# ----------------------------------------------------------------------------------------------------- the composition --
COMPOSED_B = 150


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("D,F,T", COMPOSED, ids=["%d-%d-%d" % s for s in COMPOSED])
def test_store_then_update_over_three_batches(D, F, T, cell):
    """zt_store_messages then the cell on the batch's endpoints, three batches running: from the second on the messages
    are built from rows the update before wrote.  Against the float64 composition, at the cell's tolerance."""
    import inputs as I
    from zebra_amd.modules import GRUMemoryUpdater, RNNMemoryUpdater
    B = COMPOSED_B
    x = make_store_inputs(D, F, T, B, 3)
    w = make_cell_inputs(cell, D, 2 * D + F + T)
    tgn = _store_tgn(D, F, T, x["efeat"])
    m = tgn.memory
    upd = (GRUMemoryUpdater if cell == "gru" else RNNMemoryUpdater)(2 * D + F + T, D, "cuda").to("cuda")
    with torch.no_grad():
        for name, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            getattr(upd.memory_updater, name).copy_(_t(w[key]))
    mem0 = (x["memory"] * np.float32(0.3)).astype(np.float32)
    batches = [tuple(x[kk][b * B:(b + 1) * B] for kk in ("src", "dst", "ts", "eidx")) for b in range(3)]
    refs = oracle().run_batches(cell, mem0, x["last_update"], x["efeat"], I.time_encode_weights(T), batches, w["w_ih"],
                                w["w_hh"], w["b_ih"], w["b_hh"])
    m.memory.copy_(_t(mem0).cuda())
    m.last_update.copy_(_t(x["last_update"]).cuda())
    worst = 0.0
    for b, (src, dst, ts, eidx) in enumerate(batches):
        tgn.store_messages_device(*[_t(a).cuda() for a in (src, dst, ts, eidx)])
        ids = _t(np.concatenate([src, dst])).cuda()
        upd.update_device(m, ids, ids.numel())
        torch.cuda.synchronize()
        assert int(tgn._status.item()) == 0
        ref = refs[b]
        tol = TOL * max(1.0, float(np.abs(ref["memory"]).max()))
        err = float(np.abs(m.memory.cpu().numpy() - ref["memory"]).max())
        worst = max(worst, err)
        assert err <= tol, (b, err, tol)
        assert np.array_equal(m.last_update.cpu().numpy(), ref["last_update"]), b
        assert np.array_equal(m.timestamps.cpu().numpy(), ref["timestamps"]), b
        assert np.array_equal(m._flag_buf.cpu().numpy()[:NN], ref["flags"]) and not ref["flags"].any(), b
        rows, count = upd.last_rows()
        assert np.array_equal(np.sort(rows[: int(count.item())].cpu().numpy()), ref["rows"]), b
        assert np.abs(m.messages.cpu().numpy() - ref["messages"]).max() <= tol, b
    assert len(np.intersect1d(refs[0]["rows"], np.concatenate(batches[2][:2]))) > 0          # later batches read updated rows
    print("%s D=%d F=%d T=%d composed: %.2e" % (cell, D, F, T, worst))
