"""What tests/test_scoring_f64_gpu.py relies on, checked without a GPU: oracle/score_f64.py against torch's float64 MergeLayer
and against the C oracle's scorer; through zt_test_affinity_plan, that every GPU case reaches the form, the grid and the ET its
id names, and that the case lists straddle every seam of the kernels (a seam missing from a list fails HERE, so an edit of a
constant in scoring.hip, or of a list, shows up); that on every case's inputs the float32 composition on the CPU -- the
reference's concatenated form and the kernels' split one -- stays within half the bound; and that the bound rejects float64-made
wrong results of the kinds it is meant to catch, the first of which the old 1e-4 accepts.

Measured here over every shape of the lists: the float32 composition uses at most 0.061 of the bound, max |dp| 3.1e-7; at the
stress scales (x 4, x 30, x 400) at most 0.50 of the plain bound, taken where p64 lies within 2^-24 of 1."""
import re

import numpy as np
import pytest
import torch

import test_scoring_f64_gpu as G
from conftest import ROOT

S64 = G.oracle64()
ALL_H = sorted(set(H for _, _, H in G.CASES))
SHAPES = sorted(set((B, H) for _, B, H in G.CASES) | set(G.CROSS))


@pytest.fixture(scope="module", autouse=True)
def built():
    from zebra_amd import build
    build.build()


def _merge64(H):
    from zebra_amd.modules import MergeLayer
    m = MergeLayer(H, H, H, 1).double()
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), G.weights(H)):
            p.copy_(G._t(w).double())
    return m


# ----------------------------------------------------------------------------------------------- the restatement's pins --
@pytest.mark.parametrize("B,H", [(1, 4), (17, 20), (33, 204), (40, 300), (17, 516), (5, 768)])
def test_merge_layer_f64_is_torch_float64(B, H):
    e = G.embeddings(B, H)
    z, p = S64.merge_layer_f64(e, *G.weights(H))
    assert z.dtype == p.dtype == np.float64 and z.shape == p.shape == (2 * B,)
    t = G._t(e).double()
    with torch.no_grad():
        want = _merge64(H)(torch.cat([t[:B], t[:B]]), t[B:]).squeeze(1)
    assert np.abs(z - want.numpy()).max() <= 1e-12
    assert np.abs(p - want.sigmoid().numpy()).max() <= 1e-12


@pytest.mark.parametrize("Q,Cn,H", [(3, 31, 300), (5, 33, 1028), (1, 1, 20)])
def test_rank_f64_is_torch_float64(Q, Cn, H):
    m = _merge64(H)
    for shared in (True, False):
        emb_q, emb_c, idx, z, p = G.rank_inputs(Q, Cn, H, shared)
        assert z.shape == p.shape == (Q, Cn)
        ix = np.tile(np.arange(Cn), (Q, 1)) if shared else idx
        live = ix >= 0
        if not shared and Q > 1:
            assert (~live).any() and live[Q - 1].all() and emb_c.shape[0] != Cn
        q, c = np.nonzero(live)
        with torch.no_grad():
            want = m(G._t(emb_q).double()[q], G._t(emb_c).double()[ix[q, c]]).squeeze(1)
        assert np.abs(z[live] - want.numpy()).max() <= 1e-12
        assert np.abs(p[live] - want.sigmoid().numpy()).max() <= 1e-12
        assert np.all(p[~live] == 0.0) and np.all(np.isneginf(z[~live]))


@pytest.mark.parametrize("B,H", [(17, 20), (33, 204), (40, 300), (17, 516)])
def test_restatements_are_the_c_oracle(oracle, B, H):
    """zo_affinity (float32, ends with the sigmoid) at the tolerance tests/test_oracle_golden.py holds it to the reference with"""
    from test_oracle_golden import EMB_TOL
    e = G.embeddings(B, H)
    w = dict(zip(("fc1_w", "fc1_b", "fc2_w", "fc2_b"), G.weights(H)))
    _, p = S64.merge_layer_f64(e, *G.weights(H))
    assert np.abs(oracle.affinity(np.concatenate([e[:B], e[:B]]), e[B:], w) - p).max() <= EMB_TOL
    idx = np.stack([np.arange(B), np.arange(B) + B], axis=1)                 # edge i against its dst and its neg
    _, pr = S64.rank_f64(e[:B], e[B:], idx, G.weights(H))
    assert np.abs(pr.T.reshape(-1) - p).max() <= 1e-14                       # the two restatements are one function
    want = oracle.affinity(np.repeat(e[:B], 2, axis=0), e[B:][idx.reshape(-1)], w)
    assert np.abs(want - pr.reshape(-1)).max() <= EMB_TOL


# ------------------------------------------------------------------------------------------------------- plan coverage --
@pytest.mark.parametrize("case", G.CASES, ids=G.ident)
def test_case_reaches_what_its_id_names(case):
    form, B, H = case
    got = G.plan(B, H, form)
    assert got["form"] == form and G.FORM_NAMES[form] == G.ident(case).split("-")[0]
    m = re.search(r"-H(\d+)-B(\d+)-grid(\d+)x(\d+)(?:-ET(\d+))?$", G.ident(case))
    assert (int(m.group(1)), int(m.group(2))) == (H, B)
    assert (got["gx"], got["gy"], got["ET"]) == (int(m.group(3)), int(m.group(4)), int(m.group(5) or 0))
    if form in (G.LATENCY, G.TILED):
        assert got["KC"] == G.round_up16(H) // 16 and got["KC"] in (13, 19)


def test_other_lists_reach_their_forms():
    for B, H in G.CROSS:
        assert G.forms_of(H) == (G.LATENCY, G.TILED, G.GEN_LATENCY, G.GEN_TILED)
    for H in set(h for h, _ in G.STRESS) | set(G.NONFINITE_H):
        for B in (G.STRESS_B, G.NONFINITE_B):
            for form in G.forms_of(H):
                got, want = G.plan(B, H, form), G.expected_launch(form, B, H)
                assert {k: got[k] for k in want} == want, (H, B, form)
            for form in set((G.LATENCY, G.TILED)) - set(G.forms_of(H)):          # no specialised kernel: the library's pick
                assert G.plan(B, H, form) == G.plan(B, H, 0)
    assert G.NONFINITE_B % 16 != 0 and G.NONFINITE_B > 32
    for H in G.NONFINITE_H:
        assert H % 16 != 0                     # a ragged last k-chunk: the float4 after a row's end is the next row's first
        _, _, plants = G.nonfinite_case(H)
        assert len(set(edge for _, edge in plants)) == 6 and all(16 <= edge < 32 for _, edge in plants)
        assert sorted(blk for blk, _ in plants) == [0, 0, 1, 1, 2, 2]


def _source(name):
    return open("%s/zebra_amd/csrc/%s" % (ROOT, name)).read()


def test_the_seams_are_the_sources_constants():
    """The numbers the lists below are built around, read from the sources: an edit there fails here first"""
    s, f, r = _source("scoring.hip"), _source("scoring_fwd.hpp"), _source("rank_pair.hpp")
    assert "constexpr int AG_U = 8;" in s and "q0 += 8" in s
    assert "SPEC_TILED_MIN = 512, SPEC_ET32_MIN = 8192 + 1, GEN_TILED_MIN = 512" in s
    assert "tiles < 160 ? tiles : 160" in s and "Hp == 208 || Hp == 304" in s
    assert "constexpr int SCORE_WAVES = 16;" in f and "c + 4 <= NT; c += 4" in f and "constexpr int SCORE_MAX_H = 768;" in f
    assert "RK_TQ = 4;" in r and "RK_HC = 1024;" in r and "RANK_MAX_H = 4352;" in r and "RK_TC = (WAVE / RK_GROUP) * RK_NC;" in r
    assert "RK_GROUP = 16;" in r and "RK_NC = 8;" in r


def _of(form):
    return [(B, H) for f, B, H in G.CASES if f == form]


def test_lists_straddle_every_seam():
    NT = lambda H: G.round_up16(H) // 16
    tiles = lambda B: (B + 15) // 16
    # every H of both specialised padded widths, in both specialised forms; whole and ragged tiles; the pick's B seams
    spec = tuple(H for H in range(4, 769, 4) if G.round_up16(H) in (208, 304))
    assert spec == G.SPEC_H
    for form in (G.LATENCY, G.TILED):
        assert set(H for _, H in _of(form)) == set(spec)
        for H in spec:
            Bs = set(B for B, h in _of(form) if h == H)
            assert {1, 17, 511, 512} <= Bs, (form, H)
    assert all({15, 16, 17, 33} <= set(B for B, h in _of(G.LATENCY) if h == H) for H in spec)
    # the grid-stride loop of both latency forms: 160 | 161 tiles and a ragged last tile beyond; the specialised form at both
    # padded widths
    for form, Hs in ((G.LATENCY, (204, 300)), (G.GEN_LATENCY, (132,))):
        for H in Hs:
            t = set(tiles(B) for B, h in _of(form) if h == H)
            assert {160, 161} <= t and max(t) > 161, (form, H)
            assert any(tiles(B) > 161 and B % 16 for B, h in _of(form) if h == H), (form, H)
    assert set(G.round_up16(H) for H in (204, 300)) == {208, 304} and 204 % 16 and 300 % 16
    # ET 16 | 32, and ragged 32-edge tiles, at a ragged last chunk and at a whole one
    for H in (204, 304):
        Bs = set(B for B, h in _of(G.TILED) if h == H)
        assert {8192, 8193} <= Bs and any(B > 8193 and B % 32 not in (0, 1) for B in Bs), H
        assert G.plan(8192, H, G.TILED)["ET"] == 16 and G.plan(8193, H, G.TILED)["ET"] == 32
    assert 204 % 16 and 304 % 16 == 0
    # the generic forms: rounds of 8 (latency) and of 4 plus a remainder (tiled), a wave's N-tiles w, w + 16, w + 32
    nts = {form: set(NT(H) for _, H in _of(form)) for form in (G.GEN_LATENCY, G.GEN_TILED)}
    assert {1, 8, 9, 16, 17, 32, 33, 48} <= nts[G.GEN_LATENCY]
    assert {1, 4, 5, 16, 17, 32, 33, 48} <= nts[G.GEN_TILED]
    assert set(n % 4 for n in nts[G.GEN_TILED]) == {0, 1, 2, 3} and {1, 2, 3, 4} <= nts[G.GEN_TILED]
    assert set(n % 8 for n in nts[G.GEN_LATENCY]) >= {0, 1}
    for form in (G.GEN_LATENCY, G.GEN_TILED):
        assert set(H % 16 for _, H in _of(form)) == {0, 4, 8, 12}, form
        assert 768 in set(H for _, H in _of(form)) and 764 in set(H for _, H in _of(form))          # the widest, whole and ragged
    assert 764 % 16 == 12 and NT(764) == 48
    # more than one tile, a ragged tile and one edge, at every width of every form
    for form in G.FORM_NAMES:
        for H in set(h for _, h in _of(form)):
            Bs = set(B for B, h in _of(form) if h == H)
            assert 1 in Bs and 17 in Bs and max(Bs) >= 200, (form, H)
    # the pick's B seams, all four forms on both sides
    assert set(G.CROSS) == set((B, H) for H in (200, 300) for B in (511, 512, 8192, 8193))
    for B, H in G.CROSS:
        side = G.plan(B, H, 0)
        assert (side["form"], side["ET"]) == {511: (G.LATENCY, 0), 512: (G.TILED, 16), 8192: (G.TILED, 16), 8193: (G.TILED, 32)}[B]
    # the one-vs-many scorer's 4 x 32 tile, its chunks of 1024 columns, its widest width
    rk = set(G.RANK_CASES)
    assert set((Q, Cn) for Q, Cn, H in rk if H == 300) == set((Q, Cn) for Q in (3, 4, 5) for Cn in (31, 32, 33))
    assert {1024, 1028, 2048, 2052, 4352} <= set(H for _, _, H in rk) and (1, 1, 4352) in rk


# ------------------------------------------------------------------------------------- the bound is fit for its inputs --
@pytest.mark.parametrize("H", ALL_H)
def test_weights_have_nothing_small_where_a_bias_could_hide(H):
    """b2, b1 of the last real column and that column's fc2 weight: a kernel that dropped one of them must move a logit by
    far more than TOL_Z, or no case could see it.  (|b1 w2| and |b2| against ten times 1e-5.)"""
    W1, b1, W2, b2 = G.weights(H)
    assert abs(float(b2[0])) >= 1e-4, b2
    assert abs(float(b1[H - 1]) * float(W2[0, H - 1])) >= 1e-4, (b1[H - 1], W2[0, H - 1])


@pytest.mark.parametrize("B,H", SHAPES, ids=["H%d-B%d" % (H, B) for B, H in SHAPES])
def test_float32_composition_has_room(B, H):
    e = G.embeddings(B, H)
    z64, p64 = G.reference(B, H)
    assert np.isfinite(z64).all() and 0.0 < p64.min() and p64.max() < 1.0
    w = tuple(G._t(a) for a in G.weights(H))
    for name, p in zip(("cat", "split"), G.torch_compositions(G._t(e), w)):
        err, share = G.used(p.numpy(), z64, p64)
        assert share <= 0.5, (name, err, share)


@pytest.mark.parametrize("H,scale", G.STRESS, ids=["H%d-x%g" % c for c in G.STRESS])
def test_float32_composition_has_room_under_stress(H, scale):
    """The stress inputs do what they are for (|z| in the tens at x 4, beyond 100 at x 30 for the wide layers, exact ones among
    the float32 results) and the float32 composition stays within the PLAIN bound there."""
    B = G.STRESS_B
    e = G.embeddings(B, H, scale)
    z64, p64 = G.reference(B, H, scale)
    assert np.abs(z64).max() >= (4.0 if scale == 4.0 else 30.0)
    w = tuple(G._t(a) for a in G.weights(H))
    for p in G.torch_compositions(G._t(e), w):
        p = p.numpy()
        err, share = G.used(p, z64, p64)
        assert share <= 1.0, (err, share)
        assert np.all(p[z64 >= 18.0] == 1.0) and np.all(p[z64 <= -104.0] == 0.0)


def test_stress_cases_reach_both_saturations():
    ones = zeros = 0
    for H, scale in G.STRESS:
        z64, _ = G.reference(G.STRESS_B, H, scale)
        ones, zeros = ones + int((z64 >= 18.0).sum()), zeros + int((z64 <= -104.0).sum())
        if scale == 400.0:
            assert (z64 >= 18.0).any() and (z64 <= -104.0).any() and np.abs(z64).max() >= 300.0, H
    assert ones >= 100 and zeros >= 100


# ---------------------------------------------------------------------------------------- the bound rejects wrong outputs --
MUT_B = 17


def _parts(H):
    """float64 pieces of the scorer on the (MUT_B, H) inputs: x [2B][2H], W1, b1, W2 [H], b2"""
    e = G.embeddings(MUT_B, H).astype(np.float64)
    W1, b1, W2, b2 = [np.asarray(a, np.float64) for a in G.weights(H)]
    x = np.concatenate([np.concatenate([e[:MUT_B], e[:MUT_B]]), e[MUT_B:]], axis=1)
    return x, W1, b1, W2[0], b2[0]


def _p(z):
    return 1.0 / (1.0 + np.exp(-z))


def _rejected(H, z_wrong):
    z64, p64 = G.reference(MUT_B, H)
    return bool((np.abs(_p(z_wrong) - p64) > G.bound(z64, p64)).any())


def _accepted_by_old(H, z_wrong):
    _, p64 = G.reference(MUT_B, H)
    return bool(np.abs(_p(z_wrong) - p64).max() <= G.OLD_TOL)


def test_parts_are_the_reference():
    for H in (20, 204, 516):
        x, W1, b1, W2, b2 = _parts(H)
        assert np.abs(np.maximum(x @ W1.T + b1, 0) @ W2 + b2 - G.reference(MUT_B, H)[0]).max() <= 1e-12


@pytest.mark.parametrize("H", ALL_H)
def test_bound_rejects_one_dropped_k_column_of_one_unit(H):
    """fc1's weight of ONE unit on the last column of the dst / neg half left out, for every unit in turn.  A unit that is
    dead on all 34 pairs, or whose weight on that column is nearly 0, cannot show; measured, the bound rejects 0.965 .. 1.0 of
    the units at every width, the last real unit among them.  At H >= 300 the old 1e-4 accepts 0.19 .. 0.37 of these wrong
    results (0.09 .. 0.22 from H = 196): that is the point of the new bound."""
    x, W1, b1, W2, b2 = _parts(H)
    z64, p64 = G.reference(MUT_B, H)
    hid, k = x @ W1.T + b1, 2 * H - 1
    dz = (np.maximum(hid - np.outer(x[:, k], W1[:, k]), 0) - np.maximum(hid, 0)) * W2            # [2B][H]: unit u's drop
    err = np.abs(_p(z64[:, None] + dz) - p64[:, None])
    rejected = (err > G.bound(z64, p64)[:, None]).any(axis=0)
    old_accepts = err.max(axis=0) <= G.OLD_TOL
    assert rejected[H - 1] and rejected.mean() >= 0.95, rejected.mean()
    W = W1.copy()                                                         # (the vectorised form above is the plain one)
    W[H - 1, k] = 0.0
    assert np.abs(np.maximum(x @ W.T + b1, 0) @ W2 + b2 - (z64 + dz[:, H - 1])).max() <= 1e-12
    if H >= 300:
        assert (old_accepts & rejected).mean() >= 0.1, (old_accepts & rejected).mean()


@pytest.mark.parametrize("H", [h for h in ALL_H if h % 16])
def test_bound_rejects_a_dropped_ragged_k_chunk(H):
    x, W1, b1, W2, b2 = _parts(H)
    k0 = H // 16 * 16
    xw = x.copy()
    xw[:, k0:H] = 0.0
    xw[:, H + k0:] = 0.0
    assert H not in (204, 764) or H - k0 == 12
    assert _rejected(H, np.maximum(xw @ W1.T + b1, 0) @ W2 + b2)


@pytest.mark.parametrize("H", ALL_H)
def test_bound_rejects_a_dropped_bias_of_the_last_real_column(H):
    x, W1, b1, W2, b2 = _parts(H)
    b = b1.copy()
    b[H - 1] = 0.0
    assert _rejected(H, np.maximum(x @ W1.T + b, 0) @ W2 + b2)
    assert _rejected(H, np.maximum(x @ W1.T + b1, 0) @ W2)                   # and fc2's


@pytest.mark.parametrize("H", [h for h in ALL_H if h > 16])
def test_bound_rejects_a_left_out_last_n_tile(H):
    """the last N-tile's partial score never added: 132 and 260 (four real units in it) among the widths"""
    x, W1, b1, W2, b2 = _parts(H)
    n0 = (G.round_up16(H) // 16 - 1) * 16
    hid = np.maximum(x @ W1.T + b1, 0)
    assert H not in (132, 260) or H - n0 == 4
    assert _rejected(H, hid[:, :n0] @ W2[:n0] + b2)


@pytest.mark.parametrize("H", ALL_H)
def test_bound_rejects_w_b_applied_to_src_for_one_edge(H):
    """each edge of the tile in turn.  From 16 units on no pair has all of them dead before and after (2^-16 each); below
    that a pair can, and then the two results are equal: most edges still show."""
    x, W1, b1, W2, b2 = _parts(H)
    n = 0
    for edge in range(MUT_B):
        xw = x.copy()
        xw[edge, H:] = xw[edge, :H]                                           # the positive pair of the edge
        n += _rejected(H, np.maximum(xw @ W1.T + b1, 0) @ W2 + b2)
    assert n == MUT_B if H >= 16 else n > MUT_B // 2, n
