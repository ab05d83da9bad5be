"""The fused neighbour aggregation -- every form behind zt::embed_kernel_plan and the three output-layer forms (zt_embed),
zt_agg_train_forward / zt_agg_train_backward -- against the plain float64 restatement oracle/aggregate_f64.py
(pinned to TorchCpuP23.embed in tests/test_aggregate_f64_cpu.py).

Inputs: this file's own seeded generator (make_inputs), NOT inputs.random_tables: edge features are non-zero at every F,
F = 1 included, so the edge-feature columns of every kernel multiply something; ids include 0 and repeat within a
row; dt on both sides of the cosine's 4e6 switch, up to 3e8; query rows without any weight (S = 0) and short ones.

Tolerances against float64, each one a number the project already asserts, none fitted to the kernels:
  embeddings  2e-5 max(1, max|ref|)             (test_specialised_aggregate_equals_generic, between two forms)
  H           1e-5 max(1, max|ref|)             (test_row_split_aggregate_forward_backward)
  gradients   1e-5 + 1e-5 max|ref| per tensor, EVERY element (test_hip_gru_rows_against_float64), plus the ReLU-switch
              allowance below
torch's own float32 composition on the device, on the same inputs, is held to HALF of each (the gradients: half the
tolerance plus the same allowance -- a switch is one whole term or none, in either float32 method), which is what shows
that the reference method has room.

ReLU switches.  From the float64 pre-activations z a unit is undecided where it is live (kept by the mask, normalised
weight > 0) and |z| <= TAU = 2e-5: torch float32's z is off by up to 2.7e-6 on these inputs, and the kernels' cosine can add
at most eps_cos sum_c |W1[j, D+F+c]| ~ 1e-5 with eps_cos = 2e-6, the bound test_time_encode_through_embed_kernel asserts.
A gradient element's allowance is the sum of |term| the undecided units would contribute to it (aggregate_f64, in
float64), added to that element's tolerance; nothing else is excluded.  It is a bound, not a skip: undecided units are at
most 1e-4 of the live ones (asserted here and, for every training case, without a GPU in test_aggregate_f64_cpu.py).

How much the allowance covers.  ONE undecided unit (m, n, kk, j) reaches db1[j], the whole row dW1[j, :] and, where its
neighbour is an overlay row, the whole row d_overlay[u, :]: 1 / D of db1 and dW1, 1 / 30 of d_overlay.  At the share
expected (2e-5 of 1.2e5 ... 1.5e6 live units: 2 ... 30 units) "99 % of each gradient's elements carry no allowance"
cannot hold at D = 100 for any seed, and an allowance of |G| wn |x| ~ 1e-2 would leave those rows unchecked at 1e-4.
So the rows that carry an allowance are checked a second time AT THE BARE TOLERANCE: a ReLU's derivative is 0 or 1, so
a correct backward equals float64 with each undecided unit of the row wholly in or wholly out; every such choice is tried
(at most MAX_FLIPS = 12 units per row, 2^12 choices) and the best one must leave every element of the row within the
tolerance.  Only rows with more undecided units than that are left to the allowance alone, and those must be under 1 % of
each gradient's elements -- the form of the 99 % rule that can be met (no case here has such a row: the CPU test asserts
it).  This asks more than the allowance does, never less: every in-or-out choice lies inside it.

Measured on an MI355X (max |error| against float64; the tables per form and per case are in DESIGN.md): embeddings -- kernels
<= 2.0e-6, torch <= 2.0e-6, tolerance >= 6.0e-5; H -- kernels <= 1.1e-6, torch <= 1.2e-6, tolerance >= 1.6e-5; dW1 -- kernels
<= 9.7e-6, torch <= 3.5e-5, against 1.2e-4 ... 1.9e-4; db1 -- 5.7e-6 and 2.1e-6; d_overlay -- 1.9e-7 and 1.7e-7 against
1.2e-5 ... 2.9e-5.  Undecided units: 0 ... 25 per case, 0 ... 3.05e-5 of the live ones, at most 2 in one gradient row; none fell
on the other side, for the kernels or for torch.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import inputs as I
import test_launch_plan_cpu as LP
from conftest import ROOT

pytestmark = pytest.mark.gpu

NN, E1, M = 600, 2000, 2                   # memory rows, edge-feature rows, models
TAU = 2e-5
UNDECIDED_CAP = 1e-4                       # share of the live units
EVAL_N = (1, 37, 257)                      # one row; less than a tile; several workgroups and a ragged last tile
TRAIN_N, U = 37, 30
DROP_SEED = 0x0BADC0DE12345678
MAX_FLIPS = 12                             # undecided units of one gradient row tried in and out (2^12 choices)

# (form, D, F, T, k, projected table given)
EVAL_CASES = [
    ("reg", 100, 1, 100, 20, True), ("reg", 100, 4, 100, 40, True),
    ("wide", 100, 172, 100, 20, True), ("wide", 100, 172, 100, 40, True),
    ("d100", 100, 172, 100, 10, True), ("d100", 100, 64, 100, 20, True),
    ("tiled_table", 100, 172, 100, 5, True), ("tiled_table", 20, 7, 20, 5, True),
    ("tiled_full", 100, 172, 100, 20, False), ("tiled_full", 100, 172, 100, 40, False),
    ("tiled_full", 100, 1, 100, 20, False), ("tiled_full", 100, 4, 100, 40, False),
    ("tiled_full", 20, 7, 12, 5, False),                                   # K1 = 39: nothing is a multiple of 16
    ("tiled_table_big", 100, 1, 100, 81, True), ("tiled_table_big", 100, 1, 100, 255, True),
    ("tiled_full_big", 100, 1, 100, 81, False),
    ("split", 100, 172, 100, 160, False), ("split", 100, 1, 100, 255, False),
    # the wide widths (Dp = D: no padded column), with the table and without
    ("tiled_table", 172, 172, 172, 20, True), ("tiled_full", 172, 172, 172, 20, False),
    ("tiled_table_big", 256, 1, 256, 100, True), ("split", 256, 1, 256, 100, False),
    ("tiled_table", 128, 16, 128, 20, True), ("tiled_full", 128, 16, 128, 20, False),
]
# (D, F, T, k): one 80-row tile, the chunked tiles at 81 and 255, BW_NTW (D <= 128) and BW_NTW_WIDE, T != D
TRAIN_CASES = [(100, 1, 100, 20), (100, 172, 100, 20), (100, 172, 100, 80), (100, 172, 100, 81), (100, 1, 100, 255),
               (128, 16, 128, 20), (172, 172, 172, 20), (256, 1, 256, 100), (20, 7, 12, 5)]


def _oracle():
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import aggregate_f64
    return aggregate_f64


def make_inputs(D, F, T, k, n, overlay=False, M=M):
    """The one seeded generator of this file and of test_aggregate_f64_cpu.py (CPU tensors).  The special rows sit at
    fixed positions from row 0 on, so the first rows of a draw are a smaller case of the same kind: the eval cases draw
    257 rows once and run their first 1, 37 and 257.  M models (tests/test_many_models_gpu.py runs 3, 4 and 16): the
    model count enters the seed only where it is not 2, so the cases of this file draw what they always drew."""
    g = torch.Generator().manual_seed(7000 + 131 * D + 17 * F + 5 * T + k + (1 if overlay else 0)
                                      + (100003 * M if M != 2 else 0))
    x = {"w": I.model_weights(D, F, T, M, 61), "tw": I.time_encode_weights(T)}
    x["memory"] = torch.randn((NN, D), generator=g)
    x["efeat"] = torch.randn((E1, F), generator=g)                      # non-zero at every F, row 0 included
    on = torch.randint(0, NN, (M, n, k), generator=g, dtype=torch.int32)
    oe = torch.randint(0, E1, (M, n, k), generator=g, dtype=torch.int32)
    if overlay:                                                          # test_row_split_aggregate_forward_backward's
        ids = torch.randperm(NN, generator=g)[:U]
        x["ids"] = ids.to(torch.int32)
        x["overlay"] = torch.randn((U, D), generator=g)
        row_map = torch.full((NN,), -1, dtype=torch.int32)
        row_map[ids] = torch.arange(U, dtype=torch.int32)
        x["row_map"] = row_map
        on[:, :, ::3] = ids[torch.randint(0, U, (M, n, (k + 2) // 3), generator=g)].to(torch.int32)   # repeated overlay rows
    on[:, :, k - 1] = on[:, :, k // 2 - 1]                              # a repeat within every row
    oe[:, :, k - 2] = oe[:, :, 0]
    on[:, ::3, 1] = 0                                                    # id 0
    oe[:, 1::3, 1] = 0
    od = torch.rand((M, n, k), generator=g) * 3.0e6
    od[:, ::7] *= 100.0                                                  # both sides of the 4e6 switch, up to 3e8
    ow = torch.rand((M, n, k), generator=g)
    ow[:, 2::5] = 0.0                                                    # S = 0 rows
    ow[:, 3::5, k // 2:] = 0.0                                           # short dictionaries
    x.update(on=on, oe=oe, od=od.float(), ow=ow.float(), G=torch.randn((M, n, D), generator=g))
    return x


def train_mask(D, k, p, M=M):
    """The kernels' keep-mask for a training case (its definition: zebra_amd.modules.dropout_mask), or None."""
    if p == 0:
        return None
    from zebra_amd.modules import dropout_mask
    return dropout_mask(DROP_SEED, p, (M, TRAIN_N, k), D)


def train_reference(D, F, T, k, p, overlay=True, M=M):
    x = make_inputs(D, F, T, k, TRAIN_N, overlay=overlay, M=M)
    ref = _oracle().aggregate_f64(x["w"]["fc1_w"], x["w"]["fc1_b"], x["memory"], x["efeat"], x["tw"], x["on"], x["oe"],
                                  x["od"], x["ow"], x["G"], overlay=x.get("overlay"), row_map=x.get("row_map"),
                                  mask=train_mask(D, k, p, M), tau=TAU)
    return x, ref


@functools.lru_cache(maxsize=None)
def _eval_reference(D, F, T, k, M=M):
    x = make_inputs(D, F, T, k, max(EVAL_N), M=M)
    nodes = torch.randint(0, NN, (max(EVAL_N),), generator=torch.Generator().manual_seed(D + F + k), dtype=torch.int32)
    nodes[1] = 0
    out, H, S = _oracle().embed_f64(x["w"], x["memory"].numpy(), x["efeat"].numpy(), x["tw"], nodes.numpy(),
                                    x["on"].numpy(), x["oe"].numpy(), x["od"].numpy(), x["ow"].numpy())
    return x, nodes, out, S


def _tgn(x, D, F, T, k, M=M):
    from helpers import build_tgn
    al, be = ([0.1, 0.1, 0.2, 0.0] * 4)[:M], ([0.5, 0.95, 0.8, 0.25] * 4)[:M]     # (the aggregation reads neither)
    tgn = build_tgn(NN, E1, D, F, T, k, al, be, x["w"], x["efeat"].numpy())
    tgn.memory.memory.copy_(x["memory"].to(tgn.device))
    return tgn


def _wn(ow):
    ws = ow.sum(dim=-1, keepdim=True)
    return torch.where(ws == 0, torch.zeros_like(ow), ow / torch.where(ws == 0, torch.ones_like(ws), ws)), ws.squeeze(-1) != 0


def _torch_embed(em, memory, nodes, on, oe, od, ow):
    """torch's float32 composition of the eval forward on the device (TorchCpuP23.embed's ops)."""
    lin = torch.nn.functional.linear
    with torch.no_grad():
        outs = [em.fc2_source(torch.relu(em.fc1_source(memory[nodes.long()])))]
        tw = em.time_encoder.w.weight.view(-1)
        for m in range(on.shape[0]):
            xx = torch.cat([memory[on[m].long()], em.edge_features[oe[m].long()], torch.cos(od[m].unsqueeze(-1) * tw)], dim=2)
            h = lin(torch.relu(lin(xx, em.fc1.weight, em.fc1.bias)), em.fc2.weight, em.fc2.bias)
            outs.append((h * _wn(ow[m])[0].unsqueeze(-1)).sum(dim=1))
        return torch.cat(outs, dim=1)


def _check_eval(form, D, F, T, k, table, out_choice=0, Ns=EVAL_N, M=M):
    from zebra_amd import _capi
    x, nodes, want, S = _eval_reference(D, F, T, k, M)
    hooks = _capi.hooks_lib()
    tgn = _tgn(x, D, F, T, k, M).eval()
    em, dev = tgn.embedding_module, tgn.device
    tol = 2e-5 * max(1.0, np.abs(want).max())
    assert (S == 0).any() and (S == 1).any()
    for n in Ns:
        a, o, _ = LP.plan(hooks, n, D, F, T, M, k, table, out_choice=out_choice)
        assert a == LP.AGG[form], "N = %d: the plan sends this shape to form %d, not to %s" % (n, a, form)
        args = [x[kk][:, :n].contiguous().to(dev) for kk in ("on", "oe", "od", "ow")]
        nd = nodes[:n].contiguous().to(dev)
        got = em.embed_device(tgn.memory.memory, nd, *args, memory_obj=tgn.memory if table else None)
        assert int(em._status.item()) == 0
        ref32 = _torch_embed(em, tgn.memory.memory, nd, *args)
        assert (em._proj is not None and em._proj["key"] is not None) == table     # the projected table was what it read
        d_hip = np.abs(got.cpu().numpy().astype(np.float64) - want[:n])
        d_torch = np.abs(ref32.cpu().numpy().astype(np.float64) - want[:n])
        e_hip, e_torch = float(d_hip.max()), float(d_torch.max())
        print("eval %-15s M=%d D=%d F=%d T=%d k=%d table=%d out=%d/%d N=%d: models' columns hip %.2e torch %.2e, source columns "
              "hip %.2e torch %.2e (tol %.2e)" % (form, M, D, F, T, k, table, out_choice, o, n, d_hip[:, D:].max(),
                                                  d_torch[:, D:].max(), d_hip[:, :D].max(), d_torch[:, :D].max(), tol))
        assert got.shape == (n, D * (M + 1))
        assert e_torch <= 0.5 * tol, "torch float32 itself is %.3g from float64 at N = %d" % (e_torch, n)
        assert e_hip <= tol, "N = %d: %.3g from float64" % (n, e_hip)
    return o


@pytest.mark.parametrize("form,D,F,T,k,table", EVAL_CASES,
                         ids=["%s-%d-%d-%d-%d-%s" % (c[0], c[1], c[2], c[3], c[4], "tab" if c[5] else "notab") for c in EVAL_CASES])
def test_embed_against_float64(form, D, F, T, k, table):
    """embed_device (zt_embed) against embed_f64 at N = 1, 37, 257, the library's own choice of output layers; before each
    run zt_test_embed_plan must name the aggregation form the case is listed under, so that a plan change that reroutes a
    shape fails here and cannot silently lose the form's coverage.  Every shape of the list takes its form as listed."""
    _check_eval(form, D, F, T, k, table)


@pytest.mark.parametrize("form,D,F,T,k,table", [("reg", 100, 1, 100, 20, True), ("tiled_full", 128, 16, 128, 20, False)],
                         ids=["Dp112", "Dp128"])
def test_output_layers_against_float64(form, D, F, T, k, table):
    """The three output-layer forms pinned one after the other (k_embed_out, k_embed_out2, k_embed_out3), one shape per
    padded width: Dp = 112 takes all three, Dp = 128 has no persistent form and the plan answers it with the tiled one."""
    from zebra_amd import _capi
    want = {_capi.OUT_TILED: "tiled", _capi.OUT_LATENCY: "latency", _capi.OUT_PERSIST: "persist" if D == 100 else "tiled"}
    try:
        for choice in (_capi.OUT_TILED, _capi.OUT_LATENCY, _capi.OUT_PERSIST):
            _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, choice)
            assert _check_eval(form, D, F, T, k, table, out_choice=choice, Ns=(37, 257)) == LP.OUT[want[choice]]
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, 0)


def flip_groups(ref, name):
    """{row of the gradient: signed terms [u, C] of the undecided units that reach it} for d_overlay / dW1 / db1."""
    und = ref["undecided"]
    rows = und["slot"] if name == "d_overlay" else und["j"]
    terms = np.asarray(und[name], np.float64).reshape(len(rows), -1 if len(rows) else 1)
    return {int(r): terms[rows == r] for r in np.unique(rows[rows >= 0])}


def _grad_check(name, got, want, ref, half, what):
    """Every element within the tolerance plus its allowance; then the rows that carry an allowance once more at the
    bare tolerance, against float64 with each of the row's undecided units wholly in or wholly out (a ReLU derivative
    is 0 or 1: nothing in between can come out of a correct backward).  Returns the worst error left after the best
    such choice, the tolerance, and the number of units found on the other side."""
    allow = ref[{"d_overlay": "allow_overlay", "dW1": "allow_W1", "db1": "allow_b1"}[name]]
    base = (0.5 if half else 1.0) * (1e-5 + 1e-5 * np.abs(want).max())
    err = got.astype(np.float64) - want
    over = np.abs(err) > base + allow
    assert not over.any(), "%s %s: %d elements beyond tolerance + allowance, the worst by %.3g (tolerance %.3g)" \
        % (what, name, int(over.sum()), float((np.abs(err) - base - allow).max()), base)
    err2, worst, flipped = err.reshape(len(err), -1).copy(), 0.0, 0
    for r, terms in flip_groups(ref, name).items():
        if len(terms) > MAX_FLIPS:
            continue                                                    # (held to the allowance alone; counted by the caller)
        best = None
        for bits in range(1 << len(terms)):
            sel = np.array([(bits >> i) & 1 for i in range(len(terms))], np.float64)
            left = err2[r] - sel @ terms
            if best is None or np.abs(left).max() < np.abs(best[0]).max():
                best = (left, int(sel.sum()))
        assert np.abs(best[0]).max() <= base, "%s %s row %d: %.3g from float64 with its %d undecided units in or out, " \
            "whichever fits best (tolerance %.3g)" % (what, name, r, np.abs(best[0]).max(), len(terms), base)
        err2[r], flipped = best[0], flipped + best[1]
    rest = np.ones(len(err2), bool)
    rest[[r for r, t in flip_groups(ref, name).items() if len(t) > MAX_FLIPS]] = False
    if rest.any():
        worst = float(np.abs(err2[rest]).max())
    return worst, base, flipped


def allowance_only_share(ref, name):
    """The share of a gradient's elements that only the allowance covers: rows with more than MAX_FLIPS undecided units."""
    n = len(ref[name])
    return sum(1 for t in flip_groups(ref, name).values() if len(t) > MAX_FLIPS) / n


def _check_train(D, F, T, k, p, overlay=True, M=M):
    from zebra_amd import _capi
    from zebra_amd.modules import _NeighbourAggregate
    x, ref = train_reference(D, F, T, k, p, overlay, M)
    form = LP.plan(_capi.hooks_lib(), TRAIN_N, D, F, T, M, k, False, training=True)[0]
    assert form == LP.AGG["tiled_full" if k <= 80 else "split"]      # one tile up to k = 80, the row split beyond
    tgn = _tgn(x, D, F, T, k, M)
    em, dev = tgn.embedding_module, tgn.device
    mem = tgn.memory.memory.detach()
    on, oe, od, ow, G = [x[kk].to(dev) for kk in ("on", "oe", "od", "ow", "G")]
    seed = DROP_SEED if p > 0 else 0
    if overlay:
        ov = x["overlay"].to(dev).requires_grad_(True)
        row_map, ids32 = x["row_map"].to(dev), x["ids"].to(dev)
    else:
        ov = torch.zeros((1, D), device=dev, requires_grad=True)
        row_map, ids32 = torch.full((NN,), -1, dtype=torch.int32, device=dev), None
    fc1_w = em.fc1.weight.detach().clone().requires_grad_(True)
    fc1_b = em.fc1.bias.detach().clone().requires_grad_(True)
    leaves = (ov, fc1_w, fc1_b)

    def grads():
        return [t.grad.detach().cpu().numpy().copy() if t.grad is not None else None for t in leaves]

    def fused():
        for t in leaves:
            t.grad = None
        H, S = _NeighbourAggregate.apply(ov, fc1_w, fc1_b, em, mem, row_map, ids32, on, oe, od, ow, p, seed)
        (H * G).sum().backward()
        if overlay:
            row_map[ids32.long()] = torch.arange(U, dtype=torch.int32, device=dev)   # (the backward resets the shared map)
        return H.detach().cpu().numpy(), S.cpu().numpy(), grads()

    def composed():
        for t in leaves:
            t.grad = None
        rows = mem[on.long()]
        if overlay:
            slot = row_map[on.long()]
            rows = torch.where((slot >= 0).unsqueeze(-1), ov[slot.long().clamp(min=0)], rows)
        tw = em.time_encoder.w.weight.view(-1)
        xx = torch.cat([rows, em.edge_features[oe.long()], torch.cos(od.unsqueeze(-1) * tw)], dim=-1)
        h = torch.relu(torch.nn.functional.linear(xx, fc1_w, fc1_b))
        if p > 0:
            h = h * torch.from_numpy(train_mask(D, k, p, M)).to(dev)
        wn, nz = _wn(ow)
        H = (h * wn.unsqueeze(-1)).sum(dim=2)
        (H * G).sum().backward()
        return H.detach().cpu().numpy(), nz.float().cpu().numpy(), grads()

    Hf, Sf, gf = fused()
    Hc, Sc, gc = composed()
    what = "%sD=%d F=%d T=%d k=%d p=%g%s" % ("" if M == 2 else "M=%d " % M, D, F, T, k, p, "" if overlay else " no overlay")
    share = ref["n_undecided"] / ref["n_live"]
    print("train %s: undecided %d of %d live units (%.2e)" % (what, ref["n_undecided"], ref["n_live"], share))
    assert share <= UNDECIDED_CAP
    assert np.array_equal(Sf, ref["S"]) and np.array_equal(Sc, ref["S"]) and (ref["S"] == 0).any() and (ref["S"] == 1).any()
    tolH = 1e-5 * max(1.0, np.abs(ref["H"]).max())
    eH, eHt = np.abs(Hf - ref["H"]).max(), np.abs(Hc - ref["H"]).max()
    print("train %s: H hip %.2e torch %.2e (tol %.2e)" % (what, eH, eHt, tolH))
    assert eHt <= 0.5 * tolH, "torch float32's H is %.3g from float64" % eHt
    assert eH <= tolH, "H is %.3g from float64" % eH
    assert np.abs(Hf[ref["S"] == 0]).max() == 0.0
    for name, a, b in zip(("d_overlay", "dW1", "db1"), gf, gc):
        if name == "d_overlay" and not overlay:
            assert a is None or np.abs(a).max() == 0.0                       # nothing flows into a buffer nobody read
            continue
        want = ref[name]
        assert allowance_only_share(ref, name) < 0.01
        wt, tol_t, ft = _grad_check(name, b, want, ref, True, what + " torch float32")
        wh, tol_h, fh = _grad_check(name, a, want, ref, False, what)
        print("train %s: %-9s hip %.2e (tol %.2e, %d units on the other side) torch %.2e (tol %.2e, %d units); max|ref| "
              "%.3g, rows with undecided units %d of %d" % (what, name, wh, tol_h, fh, wt, tol_t, ft, np.abs(want).max(),
                                                            len(flip_groups(ref, name)), len(want)))
        assert np.abs(a).max() > 0
    H2, _, _ = fused()
    assert np.array_equal(Hf, H2), "the forward is not deterministic"
    assert (int(em._status.item()) if em._status is not None else 0) == 0


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("D,F,T,k", TRAIN_CASES, ids=["%d-%d-%d-%d" % c for c in TRAIN_CASES])
def test_train_aggregate_against_float64(D, F, T, k, p):
    """_NeighbourAggregate forward + backward (zt_agg_train_forward / zt_agg_train_backward) against aggregate_f64: M = 2,
    n = 37, a random cotangent, 30 overlay rows that repeat within and across query rows, the kernels' dropout mask at
    p = 0.1: H, S exactly, d_overlay / dW1 / db1 element by element, the same H bits from two runs, status 0."""
    _check_train(D, F, T, k, p)


def test_train_aggregate_without_overlay_against_float64():
    """ids32 = None: no overlay pointer, no row map; dW1 and db1 as above."""
    _check_train(100, 172, 100, 20, 0.0, overlay=False)
