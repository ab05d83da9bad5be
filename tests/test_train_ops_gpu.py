"""The dense operators of a training step (csrc/train_ops.hip) on their own, each against a float64 reference on the CPU
computed from the same float32 inputs: zt_gemm_f32 in its four transpose forms and zt_colsum_f32 through the C-ABI --
tile edges, leading dimensions wider than the row, accumulate, K = 0, guards around every operand --, _HipLinear and
_HipGruRows under autograd (the GRU with torch's own float32 GRUCell held to HALF the tolerances on the same inputs, so that
the reference method has room of its own), the rule that the GRU's backward reads the forward's workspace and not the
tables, bit-equal repeats, U = 0, and _OverlayRows at the memory widths its own test does not run."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                       # float32's unit roundoff
SENTINEL = 0x5EA7BEEF                  # the bits every guard and padding element of an output starts with (6.0e18 as a float)


def _sentinel(shape):
    return np.full(shape, SENTINEL, np.uint32).view(np.float32)


def _framed(body, pad, fill):
    """[rows + 1][width + pad] float32: `body` [rows][width] top left, the padding columns and one guard row after the last
    row filled with `fill` (a float, or None for the sentinel bits)"""
    rows, width = body.shape
    out = _sentinel((rows + 1, width + pad)) if fill is None else np.full((rows + 1, width + pad), fill, np.float32)
    out[:rows, :width] = body
    return out


def _frame_untouched(got, rows, width):
    """every element of a _framed(..., None) buffer outside [rows][width] still holds the sentinel bits"""
    bits = got.view(np.uint32).copy()
    bits[:rows, :width] = SENTINEL
    return bool((bits == SENTINEL).all())


def _bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------
# 1. zt_gemm_f32
# ---------------------------------------------------------------------------------------------------------
def _zt_gemm(A, B, Cm, M, N, K, lda, ldb, ldc, ta, tb, acc):
    from zebra_amd._capi import check, lib, ptr, stream_ptr
    check(lib().zt_gemm_f32(ptr(A), ptr(B), ptr(Cm), C.c_int64(M), C.c_int64(N), C.c_int64(K), C.c_int64(lda), C.c_int64(ldb),
                            C.c_int64(ldc), C.c_int32(ta), C.c_int32(tb), C.c_int32(acc), stream_ptr()), "zt_gemm_f32")


# the smallest shapes that cross the 64 x 64 tile in M and N and the 64-column K step; the last two: a GRU gate product
# and a weight gradient in miniature
GEMM_SHAPES = [(1, 1, 1), (63, 65, 64), (64, 64, 65), (65, 63, 63), (129, 70, 130), (5, 300, 600), (300, 67, 37)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_against_float64(ta, tb, M, N, K):
    """C = op(A) op(B) (+ C0) against the float64 product, element by element within the forward bound of K float32
    products summed in any order, fused or not, plus the accumulate add: (K + 2) 2^-24 (|A| |B| + |C0|)[i, j].  Leading
    dimensions equal to the rows and 3 wider; A's and B's padding columns and a guard row after each are NaN (a read
    outside the logical operand poisons the result), C's padding and guard row must come back bit-equal to the sentinel
    they held; with accumulate = 0 C starts as NaN (it must not be read); two calls give the same bits."""
    rng = np.random.RandomState(1000 * M + 10 * N + K + 2 * ta + tb)
    worst = 0.0
    for pad in (0, 3):
        for acc in (0, 1):
            a = rng.standard_normal((M, K)).astype(np.float32)
            b = rng.standard_normal((K, N)).astype(np.float32)
            c0 = rng.standard_normal((M, N)).astype(np.float32)
            hA = _framed(a.T if ta else a, pad, np.nan)
            hB = _framed(b.T if tb else b, pad, np.nan)
            hC = _framed(c0 if acc else np.full((M, N), np.nan, np.float32), pad, None)
            dA, dB = _dev(hA), _dev(hB)
            got = []
            for _ in range(2):
                dC = _dev(hC)
                _zt_gemm(dA, dB, dC, M, N, K, hA.shape[1], hB.shape[1], hC.shape[1], ta, tb, acc)
                got.append(dC.cpu().numpy())
            what = "pad %d accumulate %d" % (pad, acc)
            assert _frame_untouched(got[0], M, N), what
            assert _bits_equal(got[0], got[1]), what
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            ref = a64 @ b64
            bound = np.abs(a64) @ np.abs(b64)
            if acc:
                ref += c0
                bound += np.abs(c0)
            bound *= (K + 2) * EPS
            err = np.abs(got[0][:M, :N].astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), "%s: %d of %d elements over the bound, worst %.3g of it" % (
                what, int((~(err <= bound)).sum()), M * N, float(np.nanmax(err / bound)))
    print("gemm ta=%d tb=%d %dx%dx%d: worst error %.3g of the bound" % (ta, tb, M, N, K, worst))


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_with_nothing_to_sum_or_to_write(ta, tb):
    """K = 0 with A and B NULL: zeros with accumulate = 0 (C preloaded with NaN), C0 bit-unchanged with accumulate = 1;
    padding and guard untouched.  M = 0 or N = 0: ZT_OK and nothing written."""
    M, N = 65, 70
    rng = np.random.RandomState(7 + 2 * ta + tb)
    c0 = rng.standard_normal((M, N)).astype(np.float32)
    lda, ldb = (M if ta else 0) + 3, (0 if tb else N) + 3
    for acc in (0, 1):
        hC = _framed(c0 if acc else np.full((M, N), np.nan, np.float32), 3, None)
        dC = _dev(hC)
        _zt_gemm(None, None, dC, M, N, 0, lda, ldb, N + 3, ta, tb, acc)
        got = dC.cpu().numpy()
        assert _frame_untouched(got, M, N), acc
        assert _bits_equal(got[:M, :N], c0 if acc else np.zeros((M, N), np.float32)), acc
    hC = _sentinel((4, 80))
    a = _dev(np.full((80, 80), np.nan, np.float32))
    for m, n in ((0, 70), (3, 0), (0, 0)):
        for acc in (0, 1):
            dC = _dev(hC)
            _zt_gemm(a, a, dC, m, n, 5, 80, 80, 80, ta, tb, acc)
            assert _bits_equal(dC.cpu().numpy(), hC), (m, n, acc)


# ---------------------------------------------------------------------------------------------------------
# 2. zt_colsum_f32
# ---------------------------------------------------------------------------------------------------------
# sixteen waves with eight rows in flight each: a row period of 128; 64 columns per workgroup
COLSUM_SHAPES = [(0, 5), (1, 1), (15, 64), (16, 65), (17, 63), (127, 300), (128, 516), (129, 768), (600, 100)]


@pytest.mark.parametrize("rows,cols", COLSUM_SHAPES)
def test_colsum_against_float64(rows, cols):
    """out (+)= column sums of X against float64 within (rows + 1) 2^-24 (sum_r |x[r, c]| + |out0[c]|); ldx = cols and
    cols + 3 with X's padding and a guard row NaN, a sentinel after out; accumulate onto random out0, and accumulate = 0
    onto NaN; rows = 0: zeros, or out0's bits; two calls give the same bits."""
    from zebra_amd._capi import check, lib, ptr, stream_ptr
    rng = np.random.RandomState(100 * rows + cols)
    worst = 0.0
    for pad in (0, 3):
        for acc in (0, 1):
            x = rng.standard_normal((rows, cols)).astype(np.float32)
            out0 = rng.standard_normal((1, cols)).astype(np.float32)
            hX = _framed(x, pad, np.nan)
            hO = _framed(out0 if acc else np.full((1, cols), np.nan, np.float32), 5, None)      # [2][cols + 5]: out, then guards
            dX = _dev(hX)
            got = []
            for _ in range(2):
                dO = _dev(hO)
                check(lib().zt_colsum_f32(ptr(dX), C.c_int64(rows), C.c_int64(cols), C.c_int64(cols + pad), ptr(dO), C.c_int32(acc),
                                          stream_ptr()), "zt_colsum_f32")
                got.append(dO.cpu().numpy())
            what = "pad %d accumulate %d" % (pad, acc)
            assert _frame_untouched(got[0], 1, cols), what
            assert _bits_equal(got[0], got[1]), what
            if rows == 0:
                assert _bits_equal(got[0][:1, :cols], out0 if acc else np.zeros((1, cols), np.float32)), what
                continue
            x64 = x.astype(np.float64)
            ref, bound = x64.sum(0), np.abs(x64).sum(0)
            if acc:
                ref += out0[0]
                bound += np.abs(out0[0])
            bound *= (rows + 1) * EPS
            err = np.abs(got[0][0, :cols].astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), "%s: %d of %d columns over the bound, worst %.3g of it" % (
                what, int((~(err <= bound)).sum()), cols, float(np.nanmax(err / bound)))
    print("colsum %dx%d: worst error %.3g of the bound" % (rows, cols, worst))


# ---------------------------------------------------------------------------------------------------------
# 3. _HipLinear
# ---------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(0, 100, 100), (1, 20, 20), (37, 67, 20), (65, 100, 100), (600, 172, 172), (129, 256, 100)]


def _within(got, ref, bound, what):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, "%s: shape %s for %s" % (what, got.shape, ref.shape)
    ok = np.abs(got - ref) <= bound                     # (a NaN fails it; a bound of zero asks for exact zeros)
    assert ok.all(), "%s: %d of %d elements over the bound" % (what, int((~ok).sum()), ok.size)


@pytest.mark.parametrize("x_grad", [True, False], ids=["dx", "nodx"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n,k,o", LINEAR_SHAPES)
def test_hip_linear_against_float64(n, k, o, bias, x_grad):
    """_HipLinear under autograd against float64 F.linear: y within (k + 3) 2^-24 (|x| |w|^T + |b|), dx within
    (o + 2) 2^-24 |dy| |w|, dW within (n + 2) 2^-24 |dy|^T |x|, db within (n + 1) 2^-24 sum |dy| -- the GEMM's and the column
    sum's bounds product by product.  With and without a bias (b = None is fc2's use), with x.requires_grad False (dx is
    None), with a contiguous cotangent and a column slice of a wider one; n = 0: an empty y, all-zero dW and db."""
    from zebra_amd.modules import _HipLinear
    g = torch.Generator().manual_seed(10000 * n + 100 * k + o)
    x = torch.randn((n, k), generator=g)
    w = (torch.rand((o, k), generator=g) * 2 - 1) / np.sqrt(k)
    b = (torch.rand(o, generator=g) * 2 - 1) / np.sqrt(k) if bias else None
    wide = torch.randn((n, o + 5), generator=g)
    dy = wide[:, 2:2 + o]
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    torch.nn.functional.linear(xr, wr, br).backward(dy.double())
    X, W, DY = np.abs(x.double().numpy()), np.abs(w.double().numpy()), np.abs(dy.double().numpy())
    y_ref = torch.nn.functional.linear(x.double(), w.double(), b.double() if bias else None).numpy()
    y_bound = (k + 3) * EPS * (X @ W.T + (np.abs(b.double().numpy()) if bias else 0.0))
    for kind in ("contiguous", "slice"):
        xc = x.cuda().requires_grad_(x_grad)
        wc = w.cuda().requires_grad_(True)
        bc = b.cuda().requires_grad_(True) if bias else None
        y = _HipLinear.apply(xc, wc, bc)
        cot = wide.cuda()[:, 2:2 + o]
        if kind == "contiguous":
            cot = cot.contiguous()
        elif n > 1:
            assert not cot.is_contiguous()
        y.backward(cot)
        _within(y, y_ref, y_bound, "y (%s)" % kind)
        if x_grad:
            _within(xc.grad, xr.grad.numpy(), (o + 2) * EPS * (DY @ W), "dx (%s)" % kind)
        else:
            assert xc.grad is None
        _within(wc.grad, wr.grad.numpy(), (n + 2) * EPS * (DY.T @ X), "dW (%s)" % kind)
        if bias:
            _within(bc.grad, br.grad.numpy(), (n + 1) * EPS * DY.sum(0), "db (%s)" % kind)
        if n == 0:
            assert tuple(y.shape) == (0, o) and not wc.grad.any() and (not bias or not bc.grad.any())


# ---------------------------------------------------------------------------------------------------------
# 4. _HipGruRows
# ---------------------------------------------------------------------------------------------------------
# U straddles the K step of the weight-gradient GEMMs; 3 D = 60, 300, 516, 768: below one tile, ragged, an exact multiple
GRU_SHAPES = [(1, 20, 67), (37, 100, 472), (63, 100, 301), (64, 100, 301), (65, 172, 616), (129, 256, 812), (600, 100, 301)]
GRU_PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")


def _gru_case(U, D, msg):
    """weights uniform in +-1/sqrt(D), messages randn, memory 0.5 randn, ids a random subset of a table of 2 U + 5 rows, a
    random cotangent -- CPU float32 tensors"""
    g = torch.Generator().manual_seed(1000 * U + D)
    N = 2 * U + 5
    s = 1.0 / np.sqrt(D)
    u = lambda *shape: (torch.rand(shape, generator=g) * 2 - 1) * s
    wts = [u(3 * D, msg), u(3 * D, D), u(3 * D), u(3 * D)]
    messages = torch.randn((N, msg), generator=g)
    memory = torch.randn((N, D), generator=g) * 0.5
    ids = torch.randperm(N, generator=g)[:U].to(torch.int32)
    dh = torch.randn((U, D), generator=g)
    return wts, messages, memory, ids, dh


def _gru_cell(wts, dtype, device):
    D, msg = wts[1].shape[1], wts[0].shape[1]
    cell = torch.nn.GRUCell(msg, D).to(dtype)
    with torch.no_grad():
        for p, w in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), wts):
            p.copy_(w.to(dtype))
    return cell.to(device)


def _hip_gru(wts, messages, memory, ids, dh, between=None):
    """(h, saved, the four gradients) of one forward + backward of _HipGruRows; between(messages, memory) runs after the
    forward on the device tables the op was given"""
    from zebra_amd.modules import _HipGruRows
    params = [w.cuda().requires_grad_(True) for w in wts]
    messages, memory = messages.cuda(), memory.cuda()
    h = _HipGruRows.apply(*params, messages, memory, ids.cuda())
    saved = h.grad_fn.saved_tensors[0].clone()
    if between is not None:
        between(messages, memory)
    h.backward(dh.cuda())
    torch.cuda.synchronize()
    return h.detach(), saved, [p.grad for p in params]


def _cell_run(cell, x, hx, dh):
    h = cell(x, hx)
    h.backward(dh)
    return h.detach(), [p.grad for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)]


def _max_err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max())


@pytest.mark.parametrize("U,D,msg", GRU_SHAPES)
def test_hip_gru_rows_against_float64(U, D, msg):
    """_HipGruRows (zt_gru_train_forward / _backward) against a float64 nn.GRUCell under autograd on the CPU: h within 1e-5,
    the four parameter gradients within 1e-5 + 1e-5 max|ref| (test_hip_rnn_rows_forward_and_backward's numbers); what the
    forward saves for the backward -- r, z, n and W_hn h + b_hn -- within 1e-5 of the float64 gates; torch's float32
    GRUCell on the device, same inputs, within HALF of each."""
    wts, messages, memory, ids, dh = _gru_case(U, D, msg)
    x, hx = messages[ids.long()], memory[ids.long()]
    ref_h, ref_g = _cell_run(_gru_cell(wts, torch.float64, "cpu"), x.double(), hx.double(), dh.double())
    w_ih, w_hh, b_ih, b_hh = [w.double() for w in wts]
    gi, gh = x.double() @ w_ih.T + b_ih, hx.double() @ w_hh.T + b_hh
    r, z = torch.sigmoid(gi[:, :D] + gh[:, :D]), torch.sigmoid(gi[:, D:2 * D] + gh[:, D:2 * D])
    hn = gh[:, 2 * D:]
    n = torch.tanh(gi[:, 2 * D:] + r * hn)
    assert float(((1 - z) * n + z * hx.double() - ref_h).abs().max()) <= 1e-12         # the gates below are the cell's
    hip_h, saved, hip_g = _hip_gru(wts, messages, memory, ids, dh)
    tor_h, tor_g = _cell_run(_gru_cell(wts, torch.float32, "cuda"), x.cuda(), hx.cuda(), dh.cuda())
    hip = [_max_err(hip_h, ref_h)] + [_max_err(a, b) for a, b in zip(hip_g, ref_g)]
    tor = [_max_err(tor_h, ref_h)] + [_max_err(a, b) for a, b in zip(tor_g, ref_g)]
    mx = [float(q.abs().max()) for q in ref_g]
    gates = _max_err(saved, torch.cat([r, z, n, hn], dim=1))
    fmt = lambda e: "h %.3g " % e[0] + " ".join("d%s %.3g" % (pn, v) for pn, v in zip(GRU_PARAMS, e[1:]))
    print("U=%d D=%d msg=%d hip: %s gates %.3g | torch: %s | max|ref| %s"
          % (U, D, msg, fmt(hip), gates, fmt(tor), " ".join("%.3g" % v for v in mx)))
    assert tuple(saved.shape) == (U, 4 * D)
    for name, e, scale in (("torch", tor, 0.5), ("hip", hip, 1.0)):
        assert e[0] <= scale * 1e-5, "%s h: %g" % (name, e[0])
        for pn, err, m in zip(GRU_PARAMS, e[1:], mx):
            assert err <= scale * (1e-5 + 1e-5 * m), "%s d%s: %g (max |ref| %g)" % (name, pn, err, m)
    assert gates <= 1e-5, "saved gates: %g" % gates


def test_hip_gru_backward_reads_the_forward_workspace_not_the_tables():
    """A training step updates the memory and stores new messages between the forward and loss.backward(): the backward
    must use the rows the forward gathered.  With both tables overwritten by NaN after the forward, the four gradients are
    the bits of a run that left them alone."""
    case = _gru_case(37, 100, 472)

    def poison(messages, memory):
        messages.fill_(float("nan"))
        memory.fill_(float("nan"))

    _, _, clean = _hip_gru(*case)
    _, _, dirty = _hip_gru(*case, between=poison)
    for pn, a, b in zip(GRU_PARAMS, clean, dirty):
        assert not torch.isnan(b).any(), pn
        assert torch.equal(a, b), pn


@pytest.mark.parametrize("U,D,msg", [(37, 100, 472), (129, 256, 812), (600, 100, 301)])
def test_hip_gru_rows_are_bit_equal_across_runs(U, D, msg):
    """Two forward + backward runs on the same inputs: the same h, the same saved gates, the same gradients."""
    case = _gru_case(U, D, msg)
    a, b = _hip_gru(*case), _hip_gru(*case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for pn, p, q in zip(GRU_PARAMS, a[2], b[2]):
        assert torch.equal(p, q), pn


@pytest.mark.parametrize("cell,gates", [("gru", 3), ("rnn", 1)])
def test_train_pairs_with_no_row(cell, gates):
    """U = 0 through the C-ABI: the backward turns its four gradient buffers, preloaded with NaN, into zeros ("written,
    not accumulated") and writes nothing after their ends; the forward returns ZT_OK and leaves h_out alone."""
    from zebra_amd import _capi
    from zebra_amd._capi import check, lib, ptr, stream_ptr
    D, msg, G = 20, 67, 8
    messages, memory = torch.zeros((5, msg)).cuda(), torch.zeros((5, D)).cuda()
    sizes = [gates * D * msg, gates * D * D, gates * D, gates * D]
    host = [np.concatenate([np.full(s, np.nan, np.float32), _sentinel(G)]) for s in sizes]
    bufs = [_dev(h) for h in host]
    check(getattr(lib(), "zt_%s_train_backward" % cell)(None, ptr(messages), ptr(memory), None, C.c_int64(0), C.c_int32(D),
                                                        C.c_int32(msg), None, *[ptr(t) for t in bufs], None, stream_ptr()),
          "backward")
    for s, t in zip(sizes, bufs):
        got = t.cpu().numpy()
        assert _bits_equal(got[:s], np.zeros(s, np.float32)) and _bits_equal(got[s:], _sentinel(G))
    wts = [torch.zeros(s).cuda() for s in sizes]
    wt = _capi.GruWeights(*[ptr(t) for t in wts])
    h_out = _dev(_sentinel(G))
    check(getattr(lib(), "zt_%s_train_forward" % cell)(ptr(messages), ptr(memory), None, C.c_int64(0), C.c_int32(D), C.c_int32(msg),
                                                       C.byref(wt), ptr(h_out), None, None, stream_ptr()), "forward")
    assert _bits_equal(h_out.cpu().numpy(), _sentinel(G))


# ---------------------------------------------------------------------------------------------------------
# 5. _OverlayRows at the other memory widths
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [20, 172, 256])
def test_overlay_rows_at_other_widths(D):
    """test_overlay_rows_forward_and_backward's construction (D = 100 there) at the other memory widths: repeated overlay
    rows, rows without an overlay, and use_map = False; forward bit-equal to torch's index / where composition, the
    gradient within that test's 1e-5.  n = 601: n D is no multiple of the kernels' 256 threads at D = 20 and 172 (at
    D = 256 every n D is one), so their last workgroup is a partial one."""
    from zebra_amd.modules import _OverlayRows
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5 + D)
    N, U, n = 500, 37, 601
    assert D == 256 or (n * D) % 256
    memory = torch.randn((N, D), generator=g).to(dev)
    ids = torch.randperm(N, generator=g)[:U].to(dev)
    row_map = torch.full((N,), -1, dtype=torch.int32, device=dev)
    row_map[ids] = torch.arange(U, dtype=torch.int32, device=dev)
    nodes = torch.randint(0, N, (n,), generator=g).to(dev)
    nodes[:50] = ids[torch.randint(0, U, (50,), generator=g).to(dev)]          # repeated overlay rows
    cot = torch.randn((n, D), generator=g).to(dev)
    ov_a = torch.randn((U, D), generator=g).to(dev).requires_grad_(True)
    ov_b = ov_a.detach().clone().requires_grad_(True)
    out = _OverlayRows.apply(ov_a, memory, row_map, nodes.to(torch.int32), True)
    (out * cot).sum().backward()
    m = row_map[nodes].long()
    ref = torch.where((m >= 0).unsqueeze(1), ov_b[m.clamp(min=0)], memory[nodes])
    (ref * cot).sum().backward()
    assert torch.equal(out, ref)
    assert (m >= 0).sum() >= 50 and (m < 0).sum() > 0
    assert tuple(ov_a.grad.shape) == (U, D)
    assert torch.allclose(ov_a.grad, ov_b.grad, rtol=0, atol=1e-5)           # (sums of a few float32 terms in another order)
    none = _OverlayRows.apply(torch.zeros((1, D), device=dev), memory, row_map, nodes.to(torch.int32), False)
    assert torch.equal(none, memory[nodes])
