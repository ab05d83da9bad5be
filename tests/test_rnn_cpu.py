"""CPU-side checks of the RNN memory updater (RNNMemoryUpdater, zt_rnn_update, zt_pipeline_set_cell; the reference's
`--memory_updater rnn`, modules/memory_updater.py:100-103): the Python surface, the C-ABI's argument checks (no GPU
needed) and the reference-generated fixtures g11_rnn_* themselves."""
import ctypes as C

import numpy as np
import pytest
import torch

import inputs as I
from conftest import golden


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def test_rnn_updater_state_dict_matches_the_reference(capi):
    """get_memory_updater("rnn") is the reference's RNNMemoryUpdater as far as a checkpoint can tell: the same keys
    (the dead layer_norm included) with the same shapes, so torch.save((tgn.state_dict(), tgn.memory)) files load
    both ways."""
    from zebra_amd.modules import RNNMemoryUpdater, get_memory_updater
    g = golden("g11_rnn_state_dict")
    u = get_memory_updater("rnn", int(g["message_dimension"]), int(g["memory_dimension"]), "cpu")
    assert isinstance(u, RNNMemoryUpdater)
    assert isinstance(u.memory_updater, torch.nn.RNNCell) and u.memory_updater.nonlinearity == "tanh"
    sd = u.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    for k in sd:
        assert tuple(sd[k].shape) == tuple(g["shape_" + k]), k
    assert u.cell == capi.CELL_RNN and u.update_symbol == "zt_rnn_update"


def test_other_memory_updaters_are_still_refused(capi):
    from zebra_amd.modules import GRUMemoryUpdater, get_memory_updater
    assert isinstance(get_memory_updater("gru", 67, 20, "cpu"), GRUMemoryUpdater)
    for kind in ("lstm", "RNN", ""):
        with pytest.raises(ValueError):
            get_memory_updater(kind, 67, 20, "cpu")


def test_rnn_update_validates_its_arguments_without_gpu(capi):
    """zt_rnn_update takes zt_gru_update's arguments and refuses what it refuses: NULL tables with ZT_ERR_ARG, D > 128
    with ZT_ERR_UNSUPPORTED (both before any device call)."""
    lib = capi.lib()
    buf = np.zeros(1 << 16, np.float32)
    flags = np.zeros(64, np.uint8)
    p, pf = capi.ptr(buf), capi.ptr(flags)
    wt = capi.GruWeights(p, p, p, p)

    def call(memory, D, weights=wt, msg=67):
        return lib.zt_rnn_update(memory, p, p, p, pf, C.c_int64(16), C.c_int32(D), C.c_int32(msg), None, C.c_int64(0),
                                 None, C.byref(weights) if weights is not None else None, p, C.c_int32(0), None)

    assert call(None, 20) == capi.ZT_ERR_ARG
    assert call(p, 20, weights=None) == capi.ZT_ERR_ARG
    assert call(p, 0) == capi.ZT_ERR_ARG
    assert call(p, 129) == capi.ZT_ERR_UNSUPPORTED
    assert "zt_rnn_update" in lib.zt_last_error().decode()
    # the GRU's bounds, the same numbers
    assert lib.zt_gru_update(p, p, p, p, pf, C.c_int64(16), C.c_int32(129), C.c_int32(67), None, C.c_int64(0), None,
                             C.byref(wt), p, C.c_int32(0), None) == capi.ZT_ERR_UNSUPPORTED
    for name in ("zt_rnn_train_forward", "zt_rnn_train_backward"):
        assert hasattr(lib, name)
    assert lib.zt_rnn_train_forward(None, p, p, C.c_int64(4), C.c_int32(20), C.c_int32(67), C.byref(wt), p, p, p,
                                    None) == capi.ZT_ERR_ARG
    assert lib.zt_rnn_train_backward(p, p, p, p, C.c_int64(4), C.c_int32(20), C.c_int32(67), p, None, p, p, p, p,
                                     None) == capi.ZT_ERR_ARG


def test_pipeline_set_cell_refuses_bad_arguments(capi):
    lib = capi.lib()
    assert lib.zt_pipeline_set_cell(None, C.c_int32(capi.CELL_RNN)) == capi.ZT_ERR_ARG
    assert lib.zt_pipeline_set_cell(None, C.c_int32(capi.CELL_GRU)) == capi.ZT_ERR_ARG
    # an unknown cell is refused before the handle is looked at: any non-NULL handle will do
    fake = C.c_void_p(8)
    assert lib.zt_pipeline_set_cell(fake, C.c_int32(7)) == capi.ZT_ERR_ARG
    assert lib.zt_pipeline_set_cell(fake, C.c_int32(-1)) == capi.ZT_ERR_ARG


@pytest.mark.parametrize("name", ["d20_f7", "d100_f172"])
def test_rnn_fixture_last_memory_rows_are_the_cell(name):
    """Sanity of the generator: in the eval protocol the last batch's endpoints get memory = RNNCell(message, memory
    after the batch before), with the messages the batch stored.  A float64 NumPy restatement of nn.RNNCell on the
    fixture's own inputs gives those rows to 1e-5; every other row is the previous memory."""
    N, E, D, F, T, k, al, be, seed, bs, nb = I.EMBED_CASES[name]
    g = golden("g11_rnn_embed_" + name)
    src, dst, _, _, _ = I.make_stream("general", N, E, seed)
    s, e = (nb - 1) * bs, nb * bs
    ids = np.unique(np.concatenate([src[s:e], dst[s:e]]))
    prev = g["eval_b%d_memory" % (nb - 2)].astype(np.float64)
    msg = g["eval_b%d_messages" % (nb - 1)].astype(np.float64)
    w_ih, w_hh = g["rnn_w_ih"].astype(np.float64), g["rnn_w_hh"].astype(np.float64)
    b_ih, b_hh = g["rnn_b_ih"].astype(np.float64), g["rnn_b_hh"].astype(np.float64)
    assert w_ih.shape == (D, 2 * D + F + T) and w_hh.shape == (D, D)
    want = prev.copy()
    want[ids] = np.tanh(msg[ids] @ w_ih.T + b_ih + prev[ids] @ w_hh.T + b_hh)
    got = g["eval_b%d_memory" % (nb - 1)]
    assert np.abs(got - want).max() <= 1e-5
    assert np.abs(want[ids] - prev[ids]).max() > 1e-3                 # the rows did change
    assert not g["eval_b%d_flags" % (nb - 1)].any()
