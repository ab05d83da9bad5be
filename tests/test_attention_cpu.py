"""The attention layer without a GPU (csrc/attention.hip): zt::attention_plan through the zt_test_attention_plan hook -- which
shapes are taken, how many query rows and 16-row M-tiles a workgroup gets and how much dynamic LDS the launch asks for --,
oracle/attention_np.py against torch's float64 layer at every shape tests/test_attention_f64_gpu.py runs, and the conditions
that file's tolerances rely on: torch's float32 layer meets half of each on these inputs, and every mask holds the rows it says.

The table's numbers are worked out by hand from attention_plan's arithmetic (Ep, Ekp, E2p, Hp, Op = E, Ek, E + D, hidden, out
rounded up to 16; lda = Ekp + 4, ldk = Ep + 4, ldq = max(E2p, Ep, Hp, Op) + 4;
bytes(mt) = 4 (16 mt lda + max(16 mt ldk, 16 ldq)) + 128 ldq + 256 mt + 64), not read from the hook."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_attention_f64_gpu as G

LDS_BOUND = 158 * 1024
REFUSED = None
# (D, F, T, heads, hidden, out, k) -> (rq, mt, LDS bytes or None where only the tile is pinned) or REFUSED
S4, S2, W = (20, 4, 12, 4, 20, 20), (20, 4, 12, 2, 20, 20), (100, 172, 100, 2, 100, 100)
PLAN_TABLE = [
    (S4 + (1,), (16, 1, 16704)), (S4 + (3,), (16, 3, 26432)), (S4 + (5,), (16, 5, 38208)), (S4 + (6,), (13, 5, 38208)),
    (S2 + (16,), (5, 5, None)), (S2 + (17,), (4, 5, None)), (S2 + (40,), (2, 5, None)), (S2 + (41,), (1, 3, 26432)),
    (S2 + (80,), (1, 5, 38208)), (S2 + (81,), REFUSED),
    ((20, 7, 13, 3, 20, 70, 5), (16, 5, 45376)),                  # Op = 80 decides ldq = 84
    ((20, 0, 12, 1, 20, 20, 5), (16, 5, 33088)),
    (W + (20,), (2, 3, 155456)), (W + (48,), (1, 3, 155456)), (W + (49,), REFUSED),
    ((100, 1, 100, 2, 100, 100, 40), (1, 3, 121664)), ((100, 1, 100, 2, 100, 100, 80), REFUSED),
    ((128, 16, 128, 2, 128, 128, 20), (2, 3, 153408)),
    ((172, 172, 172, 2, 172, 172, 16), (1, 1, 136512)), ((172, 172, 172, 2, 172, 172, 17), REFUSED),
    ((224, 1, 224, 2, 224, 224, 10), (1, 1, 160064)),
    # one M-tile is already over the bound: accepted (and then a HIP error at the launch) before the plan checked the tile
    # it ends with -- 163 136, 171 328, 182 592 and 192 832 bytes
    ((228, 1, 228, 2, 228, 228, 10), REFUSED), ((240, 1, 240, 2, 240, 240, 10), REFUSED),
    ((256, 1, 256, 2, 256, 256, 10), REFUSED), ((256, 172, 256, 2, 256, 256, 1), REFUSED),
    ((20, 4, 12, 5, 20, 20, 5), REFUSED),                         # heads > 4
    ((20, 4, 12, 3, 20, 20, 5), REFUSED),                         # E = 32 is no multiple of 3
    ((20, 4, 12, 0, 20, 20, 5), REFUSED), ((20, 4, 12, 2, 20, 20, 0), REFUSED), ((0, 4, 12, 2, 20, 20, 5), REFUSED),
    ((20, -1, 12, 2, 20, 20, 5), REFUSED), ((20, 4, 0, 2, 20, 20, 5), REFUSED), ((20, 4, 12, 2, 0, 20, 5), REFUSED),
    ((20, 4, 12, 2, 20, 0, 5), REFUSED),
]


@pytest.fixture(scope="module")
def capi():
    from zebra_amd import build
    build.build()
    from zebra_amd import _capi
    return _capi


def plan7(capi, D, F, T, heads, hidden, out, k):
    o = (C.c_int64 * 4)()
    assert capi.hooks_lib().zt_test_attention_plan(*[C.c_int32(v) for v in (D, F, T, heads, hidden, out, k)], o) == capi.ZT_OK
    return [int(v) for v in o]


def workspace(capi, *shape):
    return int(capi.lib().zt_attention_workspace_bytes(*[C.c_int32(v) for v in shape]))


@pytest.mark.parametrize("shape,want", PLAN_TABLE, ids=[G.ident(s) for s, _ in PLAN_TABLE])
def test_plan_table(capi, shape, want):
    got = plan7(capi, *shape)
    if want is REFUSED:
        assert got == [0, 0, 0, 0]
        assert workspace(capi, *shape) == -1
        return
    assert got[0] == 1 and tuple(got[1:3]) == want[:2]
    if want[2] is not None:
        assert got[3] == want[2]
    assert got[3] <= LDS_BOUND
    D, F, T, _, hidden, out, _ = shape
    r16 = lambda v: (v + 15) // 16 * 16
    E, Ek = r16(D + T), r16(D + F + T)
    # the six zero-padded weight matrices, each on a 256-byte boundary
    ws = sum((4 * a * b + 255) // 256 * 256 for a, b in ((E, E), (E, Ek), (E, Ek), (E, E), (r16(hidden), r16(D + T + D)),
                                                         (r16(out), r16(hidden))))
    assert workspace(capi, *shape) == ws


@pytest.mark.parametrize("base", [S2[:3], W[:3]], ids=G.ident)
def test_plan_sweep_over_k(capi, base):
    D, F, T = base
    taken = []
    for k in range(1, 82):
        shape = (D, F, T, 2, D, D, k)
        ok, rq, mt, lds = plan7(capi, *shape)
        assert (workspace(capi, *shape) >= 0) == (ok == 1), k
        if ok:
            taken.append(k)
            assert 1 <= rq <= 16, k
            assert rq * k <= 16 * mt <= 80, k
            assert mt == (rq * k + 15) // 16, k                     # no M-tile without a key row in it
            assert lds <= LDS_BOUND, k
    assert taken == list(range(1, 81 if D == 20 else 49))          # 5 M-tiles hold 80 key rows, 3 hold 48


def test_refusal_comes_before_any_device_call(capi):
    """ZT_ERR_UNSUPPORTED for the shapes one M-tile cannot hold, from host code: this process has no GPU to call."""
    lib = capi.lib()
    p = C.c_void_p(1 << 20)                        # never dereferenced
    wt = capi.AttnWeights(*([p] * 10))
    for D, F, T, heads, hidden, out, k in [s for s, want in PLAN_TABLE if want is REFUSED and min(s[0], s[2], s[6]) > 0 and s[1] >= 0]:
        rc = lib.zt_temporal_attention(p, p, p, p, p, p, C.c_int64(3), C.c_int32(k), C.c_int32(D), C.c_int32(F), C.c_int32(T),
                                       C.c_int32(heads), C.c_int32(hidden), C.c_int32(out), C.byref(wt), p, p, p, None)
        assert rc == capi.ZT_ERR_UNSUPPORTED, (D, F, T, heads, hidden, out, k)
        assert b"unsupported shape" in lib.zt_last_error()


def test_hook_is_declared(capi):
    import os
    hooks = open(os.path.join(G.ROOT, "zebra_amd", "csrc", "test_hooks.h")).read()
    common = open(os.path.join(G.ROOT, "zebra_amd", "csrc", "common.hpp")).read()
    assert "zt_test_attention_plan" in hooks and "attention_plan(" in common


def test_gpu_cases_are_the_accepted_rows(capi):
    """The GPU file runs every accepted row of the table (the stress shape (100, 1, 100) at k = 40 as a stress case), with the
    row count its docstring gives, and refuses every refused row a layer's widths can have."""
    accepted = {s[:4] + s[5:] for s, want in PLAN_TABLE if want is not REFUSED}
    assert set(G.CASES) | {c for c, _ in G.STRESS} == accepted
    assert all(s[4] == s[0] for s, _ in PLAN_TABLE if s[4] > 0 and s[0] > 0)    # hidden = D: what the module builds
    refused = {s[:4] + s[5:] for s, want in PLAN_TABLE if want is REFUSED and min(s[:1] + s[2:]) > 0 and s[1] >= 0}
    assert set(G.REFUSED) == refused
    for case in G.CASES + [c for c, _ in G.STRESS]:
        c = G.make_case(*case)
        rq = dict((s[:4] + s[5:], want) for s, want in PLAN_TABLE)[case][0]
        assert c["rq"] == rq and c["N"] == (2 * rq + 1 if rq > 1 else 5) and c["N"] <= 70
    assert set(G.FAMILIES) <= set(G.CASES) and {c[:3] for c in G.FAMILIES} == {c[:3] for c in G.CASES}


ALL = [(c, 1.0) for c in G.CASES] + G.STRESS


@pytest.mark.parametrize("case,scale", ALL, ids=[G.ident(c) + "-x%g" % s for c, s in ALL])
def test_inputs_hold_what_the_gpu_file_says(case, scale):
    D, F, T, heads, out_dim, k = case
    c = G.make_case(*case, scale)
    src, src_t, nbr, nbr_t, edge, mask = c["x"]
    N, rq, sp = c["N"], c["rq"], c["special"]
    assert src.shape == (N, D) and src_t.shape == (N, 1, T) and nbr.shape == (N, k, D) and edge.shape == (N, k, F)
    assert nbr_t.shape == (N, k, T) and mask.shape == (N, k) and mask.dtype == bool
    assert F == 0 or np.abs(edge).min() > 0                                     # every edge column multiplies something
    assert np.abs(src_t).max() <= 1 and src_t.std() > 0.3 and (src_t < 0).any()  # not cos(0)
    key_row = sp["none_last_of_tile_key_1e3"]
    rest = np.ones(N, bool)
    rest[key_row] = False
    assert np.abs(nbr_t[rest]).max() <= 1 and np.abs(nbr_t[key_row, 1:]).max(initial=0) <= 1
    assert np.abs(nbr[key_row, 0]).max() > 100 * scale and np.abs(nbr[rest]).max() < 6 * scale
    # the rows without any neighbour: the last row of a full tile, the first of a full tile, the first of the ragged one
    none = mask.all(axis=1)
    assert none[key_row] and key_row % rq == rq - 1 and key_row + 1 < N
    assert none[N - 1] and sp["none_at_end"] == N - 1 and (N - 1) % rq == 0
    if rq >= 3:
        r = sp["none_first_of_tile"]
        assert none[r] and r % rq == 0 and r + rq <= N
    assert len(set(sp.values())) == len(sp)
    assert not mask[sp["all_neighbours"]].any()
    if k == 1:
        assert none.sum() >= 2 and (~none).sum() >= 2
    else:
        r = sp["only_slot0_masked"]
        assert mask[r, 0] and not mask[r, 1:].any()
        r = sp["one_neighbour_last_slot"]
        assert mask[r, :k - 1].all() and not mask[r, k - 1]
        assert (~none & mask.any(axis=1)).sum() >= 2


@pytest.mark.parametrize("case,scale", ALL, ids=[G.ident(c) + "-x%g" % s for c, s in ALL])
def test_oracle_is_torch_float64_and_float32_has_room(case, scale):
    """attention_np against forward_torch in float64 within 1e-12 max(1, max|ref|); rows without a neighbour give the merger
    of [0 | src] and exact zeros; torch's float32 layer on the CPU is within half of each tolerance of the GPU file (the plain
    cases; the stress cases are held to torch on the device there)."""
    c = G.make_case(*case, scale)
    ref_out, ref_aw = G.reference(*case, scale)
    t_out, t_aw = G.torch_forward(G.build_layer(*case[:5], c["w"], torch.float64), c["x"], dtype=torch.float64)
    top = max(1.0, np.abs(t_out).max())
    assert G.err(ref_out, t_out) <= 1e-12 * top and G.err(ref_aw, t_aw) <= 1e-12
    none = c["x"][5].all(axis=1)
    assert np.all(ref_aw[none] == 0.0) and G.err(ref_out[none], G.merger_of_zero(c)[none]) <= 1e-12 * top
    assert np.abs(ref_aw[~none].sum(axis=1) - 1).max() <= 1e-12
    f_out, f_aw = G.torch_forward(G.build_layer(*case[:5], c["w"]), c["x"])
    e_out, e_aw = G.err(f_out, ref_out), G.err(f_aw, ref_aw)
    print("attention %s x%g on the CPU: torch float32 out %.2e (max|ref| %.2f) attn_w %.2e; max attn_w %.4f"
          % (G.ident(case), scale, e_out, np.abs(ref_out).max(), e_aw, ref_aw.max()))
    if scale == 1.0:
        assert e_out <= 0.5 * G.OUT_TOL * top
        assert e_aw <= 0.5 * G.AW_TOL
    else:
        # scores in the tens: among the rows with several neighbours, one key holds a whole head's worth of weight
        several = (~c["x"][5]).sum(axis=1) >= 2
        assert np.isfinite(f_out).all() and ref_aw[several].max() * case[3] > 0.95
