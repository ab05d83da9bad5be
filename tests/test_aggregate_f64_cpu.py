"""oracle/aggregate_f64.py, the float64 restatement tests/test_aggregate_f64_gpu.py holds the aggregation kernels to,
checked without a GPU: embed_f64 against TorchCpuP23.embed (itself held to the C port and the reference's fixtures in
test_oracle_golden.py), aggregate_f64's H against embed_f64's, and the GPU file's input generator against the caps its
ReLU-switch allowance relies on, so that a cap can never be the reason a GPU case goes slack."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import test_aggregate_f64_gpu as G
import test_many_models_gpu as MM

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import aggregate_f64
import torch_cpu


def _embed_args(x, n):
    nodes = np.arange(3, 3 + n) % G.NN
    return nodes, [x[kk].numpy() for kk in ("on", "oe", "od", "ow")]


@pytest.mark.parametrize("D,F,T,k", [(100, 172, 100, 20), (20, 7, 12, 5)])
def test_embed_f64_matches_torch_cpu_oracle(D, F, T, k):
    n = 37
    x = G.make_inputs(D, F, T, k, n)
    nodes, args = _embed_args(x, n)
    memory = x["memory"].numpy()
    mem = types.SimpleNamespace(memory=memory, D=D, last_update=np.zeros(G.NN, np.float32),
                                messages=np.zeros((G.NN, 1), np.float32), timestamps=np.zeros(G.NN, np.float32),
                                flags=np.zeros(G.NN, np.uint8))
    want = torch_cpu.TorchCpuP23(mem, x["w"], x["efeat"].numpy(), x["tw"]).embed(nodes, *args)
    out, H, S = aggregate_f64.embed_f64(x["w"], memory, x["efeat"].numpy(), x["tw"], nodes, *args)
    assert out.dtype == np.float64 and out.shape == want.shape == (n, D * (G.M + 1))
    assert H.shape == (G.M, n, D) and S.shape == (G.M, n)
    assert (S == 0).any() and (S == 1).any() and np.abs(H[S == 0]).max() == 0.0
    assert np.abs(out - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("overlay", [False, True])
@pytest.mark.parametrize("D,F,T,k", [(100, 1, 100, 20), (20, 7, 12, 5)])
def test_aggregate_f64_forward_is_embed_f64(D, F, T, k, overlay):
    x = G.make_inputs(D, F, T, k, G.TRAIN_N, overlay=overlay)
    nodes, args = _embed_args(x, G.TRAIN_N)
    memory = x["memory"].numpy().copy()
    if overlay:
        memory[x["ids"].long().numpy()] = x["overlay"].numpy()
        assert (x["row_map"][x["on"].long()] >= 0).float().mean() > 0.3       # the overlay is read, and often
    _, H, S = aggregate_f64.embed_f64(x["w"], memory, x["efeat"].numpy(), x["tw"], nodes, *args)
    r = aggregate_f64.aggregate_f64(x["w"]["fc1_w"], x["w"]["fc1_b"], x["memory"], x["efeat"], x["tw"], x["on"], x["oe"],
                                    x["od"], x["ow"], x["G"], overlay=x.get("overlay"), row_map=x.get("row_map"))
    assert np.array_equal(r["S"], S)
    assert np.abs(r["H"] - H).max() <= 1e-12
    assert (r["d_overlay"] is not None) == overlay


def test_generator_covers_what_it_says():
    x = G.make_inputs(100, 1, 100, 20, 257)
    assert np.abs(x["efeat"].numpy()).min() > 0                               # F = 1: no zero edge feature
    assert (x["on"] == 0).any() and (x["oe"] == 0).any()
    assert all(len(set(r.tolist())) < len(r) for r in x["on"][0])             # a repeat in every row
    od, ow = x["od"].numpy(), x["ow"].numpy()
    assert (od < 4e6).any() and (od > 4e6).any() and 1e8 < od.max() <= 3e8
    s = ow.sum(axis=-1)
    assert (s == 0).any() and ((ow[..., 10:] == 0).all(axis=-1) & (s > 0)).any()
    s37 = s[:, :37]                                                           # the first 37 rows: the same kinds of row
    assert (s37 == 0).any() and (s37 > 0).any() and (od[:, :37] > 4e6).any() and s[0, 0] > 0


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("D,F,T,k", G.TRAIN_CASES, ids=["%d-%d-%d-%d" % c for c in G.TRAIN_CASES])
def test_undecided_units_stay_under_their_cap(D, F, T, k, p):
    """Every training case of the GPU file: the units within TAU of zero are at most 1e-4 of the live ones, and no row of
    a gradient has more of them than the GPU test tries in and out (so no element is left to the allowance alone)."""
    _undecided_under_cap(D, F, T, k, p, G.M)


def _undecided_under_cap(D, F, T, k, p, M):
    x, ref = G.train_reference(D, F, T, k, p, M=M)
    assert ref["n_live"] > 0.3 * M * G.TRAIN_N * k * D * (1 - p)
    print("M=%d D=%d F=%d T=%d k=%d p=%g: %d of %d live units undecided (%.2e)"
          % (M, D, F, T, k, p, ref["n_undecided"], ref["n_live"], ref["n_undecided"] / ref["n_live"]))
    assert ref["n_undecided"] <= G.UNDECIDED_CAP * ref["n_live"]
    for name, an in (("d_overlay", "allow_overlay"), ("dW1", "allow_W1"), ("db1", "allow_b1")):
        groups = G.flip_groups(ref, name)
        assert G.allowance_only_share(ref, name) == 0.0, name      # every row's units can be tried in and out
        carrying = np.zeros(len(ref[name]), bool)
        carrying[list(groups)] = True                                # the allowance sits on exactly the rows with such units
        assert np.array_equal((ref[an].reshape(len(carrying), -1) != 0).any(axis=1), carrying)
        assert sum(len(t) for t in groups.values()) == (ref["undecided"]["slot"] >= 0).sum() if name == "d_overlay" \
            else sum(len(t) for t in groups.values()) == ref["n_undecided"]
    for kk in ("H", "z", "dW1", "db1", "d_overlay"):
        assert ref[kk].dtype == np.float64 and np.isfinite(ref[kk]).all()


@pytest.mark.parametrize("M,D,F,T,k,p", MM.TRAIN_MANY, ids=["M%d-%d-%d-%d-%d-p%g" % c for c in MM.TRAIN_MANY])
def test_undecided_units_stay_under_their_cap_many_models(M, D, F, T, k, p):
    """The same for the three- and four-model training cases of tests/test_many_models_gpu.py."""
    _undecided_under_cap(D, F, T, k, p, M)


def _broken(x, mask):
    """float64 gradients of a backward that lost what ``mask`` zeroes (a keep-mask is exactly such a loss)."""
    return aggregate_f64.aggregate_f64(x["w"]["fc1_w"], x["w"]["fc1_b"], x["memory"], x["efeat"], x["tw"], x["on"], x["oe"],
                                       x["od"], x["ow"], x["G"], overlay=x["overlay"], row_map=x["row_map"], mask=mask)


def _rejected(name, got, ref):
    try:
        G._grad_check(name, got.astype(np.float32), ref[name], ref, False, "broken")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("D,F,T,k", [(100, 172, 100, 81), (100, 1, 100, 255)])
def test_gradient_check_rejects_broken_backwards(D, F, T, k):
    """What the GPU test's gradient check (tolerance + allowance, then in-or-out at the bare tolerance) does with wrong
    gradients made in float64: one neighbour entry lost, the last 16-row chunk of one query row lost, one query row lost,
    ONE decided ReLU unit lost (a single term of dW1's row and of db1) -- all rejected, in every gradient they reach;
    an undecided unit wholly on the other side -- accepted, that is the allowance; HALF of that unit's term -- inside
    the allowance, and rejected all the same, because no choice of in or out explains it."""
    x, ref = G.train_reference(D, F, T, k, 0.0)
    ones = lambda: np.ones((G.M, G.TRAIN_N, k, D), np.float32)
    assert not any(_rejected(name, ref[name], ref) for name in ("d_overlay", "dW1", "db1"))
    wn_pos = x["ow"].numpy() / np.where(x["ow"].numpy().sum(-1, keepdims=True) == 0, 1, x["ow"].numpy().sum(-1, keepdims=True)) > 0
    slot = x["row_map"][x["on"].long()].numpy()
    m, n = [int(v[0]) for v in np.nonzero(wn_pos[:, :, k - 1] & (slot[:, :, k - 1] >= 0))]   # a full row ending on an overlay row
    for lost in ((m, n, k - 1), (m, n, slice(16 * ((k - 1) // 16), k)), (m, n)):
        mask = ones()
        mask[lost] = 0
        br = _broken(x, mask)
        for name in ("d_overlay", "dW1", "db1"):
            assert _rejected(name, br[name], ref), (lost, name)
    j = int(np.argmax(ref["z"][m, n, k - 1]))                                  # a unit far from zero, open
    assert ref["z"][m, n, k - 1, j] > 100 * G.TAU
    mask = ones()
    mask[m, n, k - 1, j] = 0
    br = _broken(x, mask)
    assert (br["dW1"] != ref["dW1"]).any(axis=1).sum() == 1                    # one row of dW1, one element of db1
    for name in ("d_overlay", "dW1", "db1"):
        assert _rejected(name, br[name], ref), name
    und = ref["undecided"]
    assert ref["n_undecided"] > 0
    for name in ("dW1", "db1"):
        u = int(np.argmax(np.abs(und["db1"])))                                 # the undecided unit that weighs most
        term = np.zeros_like(ref[name]).reshape(len(ref[name]), -1)
        term[und["j"][u]] = und[name].reshape(len(und["j"]), -1)[u]
        term = term.reshape(ref[name].shape)
        assert np.abs(term).max() > 4 * (1e-5 + 1e-5 * np.abs(ref[name]).max())    # half of it: twice the bare tolerance
        assert not _rejected(name, ref[name] + term, ref)                      # the unit on the other side
        assert (np.abs(0.5 * term) <= ref["allow_W1" if name == "dW1" else "allow_b1"]).all()
        assert _rejected(name, ref[name] + 0.5 * term, ref)                    # half a ReLU: within the allowance, and wrong
