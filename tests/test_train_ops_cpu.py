"""The host side of csrc/train_ops.hip: the workspace's size and what zt_gemm_f32, zt_colsum_f32 and the GRU / RNN
training pairs refuse.  Every refusal is decided before any device call, so nothing here needs a GPU: the pointers
handed over are host addresses that a refused call never follows."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def _i64(*v):
    return [C.c_int64(x) for x in v]


def _i32(*v):
    return [C.c_int32(x) for x in v]


def _refused(capi, name, rc):
    assert rc == capi.ZT_ERR_ARG, "%s: status %d" % (name, rc)
    msg = capi.lib().zt_last_error().decode()
    assert name in msg, msg
    return msg


@pytest.mark.parametrize("U,D,msg", [(1, 20, 67), (37, 100, 472), (64, 100, 301), (65, 172, 616), (600, 256, 812), (3, 1, 1)])
def test_gru_train_workspace_is_four_regions_of_256_byte_multiples(capi, U, D, msg):
    """zt_gru_train_workspace_bytes: the gathered messages [U][msg], the gathered memory [U][D] and the two gate
    products [U][3 D], float32, each region rounded up to 256 bytes; U = 0 is sized as U = 1."""
    lib = capi.lib()
    up = lambda b: (b + 255) // 256 * 256
    want = up(U * msg * 4) + up(U * D * 4) + 2 * up(U * 3 * D * 4)
    assert lib.zt_gru_train_workspace_bytes(C.c_int64(U), C.c_int32(D), C.c_int32(msg)) == want
    assert want % 256 == 0
    assert (lib.zt_gru_train_workspace_bytes(C.c_int64(0), C.c_int32(D), C.c_int32(msg))
            == lib.zt_gru_train_workspace_bytes(C.c_int64(1), C.c_int32(D), C.c_int32(msg)) > 0)


@pytest.mark.parametrize("U,D,msg", [(-1, 100, 472), (5, 0, 472), (5, -3, 472), (5, 100, 0), (5, 100, -1)])
def test_gru_train_workspace_refuses_bad_sizes(capi, U, D, msg):
    assert capi.lib().zt_gru_train_workspace_bytes(C.c_int64(U), C.c_int32(D), C.c_int32(msg)) == -1


def _gemm(capi, A, B, Cm, M, N, K, lda, ldb, ldc, ta=0, tb=0, acc=0):
    return capi.lib().zt_gemm_f32(A, B, Cm, *_i64(M, N, K, lda, ldb, ldc), *_i32(ta, tb, acc), None)


def test_gemm_refuses_bad_sizes_and_missing_operands(capi):
    """Negative M / N / K, a NULL C with something to write, a NULL A or B with something to read."""
    buf = np.zeros(64, np.float32)
    p = capi.ptr(buf)
    for M, N, K in ((-1, 4, 4), (4, -1, 4), (4, 4, -1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        _refused(capi, "zt_gemm_f32", _gemm(capi, p, p, p, M, N, K, 8, 8, 8))
    _refused(capi, "zt_gemm_f32", _gemm(capi, p, p, None, 4, 4, 4, 4, 4, 4))
    _refused(capi, "zt_gemm_f32", _gemm(capi, p, p, None, 4, 4, 0, 4, 4, 4))
    _refused(capi, "zt_gemm_f32", _gemm(capi, None, p, p, 4, 4, 4, 4, 4, 4))
    _refused(capi, "zt_gemm_f32", _gemm(capi, p, None, p, 4, 4, 4, 4, 4, 4))
    assert not buf.any()


# (M, N, K) = (5, 7, 3): the rows are K = 3 | M = 5 wide for A, N = 7 | K = 3 for B, N = 7 for C
@pytest.mark.parametrize("ta,tb,lda,ldb,ldc", [
    (0, 0, 2, 7, 7), (1, 0, 4, 7, 7), (1, 0, 3, 7, 7),          # lda: below K; below M when transposed (3 = K would pass untransposed)
    (0, 0, 3, 6, 7), (0, 1, 3, 2, 7), (1, 1, 5, 2, 7),          # ldb: below N; below K when transposed
    (0, 0, 3, 7, 6), (1, 1, 5, 3, 6), (0, 1, 3, 3, 0),          # ldc: below N
    (0, 0, -1, 7, 7), (0, 0, 3, -1, 7), (0, 0, 3, 7, -1),
])
def test_gemm_refuses_a_leading_dimension_below_its_row(capi, ta, tb, lda, ldb, ldc):
    """lda < (trans_a ? M : K), ldb < (trans_b ? K : N) or ldc < N: rows that overlap.  Refused before any launch, and the
    message says which call and why."""
    buf = np.zeros(64, np.float32)
    p = capi.ptr(buf)
    msg = _refused(capi, "zt_gemm_f32", _gemm(capi, p, p, p, 5, 7, 3, lda, ldb, ldc, ta, tb))
    assert "leading dimension" in msg
    assert not buf.any()


def test_colsum_refusals(capi):
    """Negative sizes, a NULL out or X with something to write or read, ldx below the row."""
    lib = capi.lib()
    buf = np.zeros(64, np.float32)
    p = capi.ptr(buf)
    call = lambda X, rows, cols, ldx, out, acc=0: lib.zt_colsum_f32(X, *_i64(rows, cols, ldx), out, C.c_int32(acc), None)
    for rows, cols in ((-1, 4), (4, -1), (-1, 0), (0, -1)):
        _refused(capi, "zt_colsum_f32", call(p, rows, cols, 8, p))
    _refused(capi, "zt_colsum_f32", call(p, 4, 4, 4, None))
    _refused(capi, "zt_colsum_f32", call(p, 0, 4, 4, None))
    _refused(capi, "zt_colsum_f32", call(None, 4, 4, 4, p))
    for ldx in (3, 0, -1):
        assert "leading dimension" in _refused(capi, "zt_colsum_f32", call(p, 4, 4, ldx, p))
        assert "leading dimension" in _refused(capi, "zt_colsum_f32", call(p, 4, 4, ldx, p, 1))
    assert "leading dimension" in _refused(capi, "zt_colsum_f32", call(None, 0, 4, 3, p))
    assert not buf.any()


@pytest.mark.parametrize("cell", ["gru", "rnn"])
def test_train_pairs_refuse_missing_tables_weights_and_outputs(capi, cell):
    """zt_gru_train_forward / zt_rnn_train_forward: NULL tables, NULL weights, bad sizes, NULL outputs with rows to write;
    the backwards: a NULL gradient output (they are written even at U = 0), NULL tables, NULL inputs with rows to read."""
    lib = capi.lib()
    fname, bname = "zt_%s_train_forward" % cell, "zt_%s_train_backward" % cell
    fwd, bwd = getattr(lib, fname), getattr(lib, bname)
    buf = np.zeros(64, np.float32)
    p = capi.ptr(buf)
    wt = capi.GruWeights(p, p, p, p)
    U, D, msg = 2, 4, 3

    def f(messages=p, memory=p, ids=p, U=U, D=D, msg=msg, w=C.byref(wt), h=p, saved=p, ws=p):
        return fwd(messages, memory, ids, C.c_int64(U), C.c_int32(D), C.c_int32(msg), w, h, saved, ws, None)

    for kw in (dict(messages=None), dict(memory=None), dict(w=None), dict(U=-1), dict(D=0), dict(msg=0), dict(ids=None),
               dict(h=None), dict(saved=None), dict(ws=None), dict(messages=None, U=0), dict(w=None, U=0)):
        _refused(capi, fname, f(**kw))

    def b(dh=p, messages=p, memory=p, ids=p, U=U, D=D, msg=msg, saved=p, g0=p, g1=p, g2=p, g3=p, ws=p):
        return bwd(dh, messages, memory, ids, C.c_int64(U), C.c_int32(D), C.c_int32(msg), saved, g0, g1, g2, g3, ws, None)

    for q in range(4):
        _refused(capi, bname, b(**{"g%d" % q: None}))
        _refused(capi, bname, b(**{"g%d" % q: None, "U": 0}))
    for kw in (dict(messages=None), dict(memory=None), dict(U=-1), dict(D=0), dict(msg=-2), dict(dh=None), dict(ids=None),
               dict(saved=None), dict(ws=None)):
        _refused(capi, bname, b(**kw))
    assert not buf.any()
