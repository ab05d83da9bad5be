"""The workspace form of the pruning query (csrc/tppr_prune.hip: k_pruned_topk_ws) -- walks whose candidate list or frontier
does not fit LDS (the reference bounds neither --n_degree nor --n_layer, train.py:25,28) -- bit for bit against the CPU
oracle and against fixtures the reference itself produced, through every layer that reaches the LDS form: the finder's
public calls, the multi-model device call, TGN directly and through the native pipeline."""
import types

import numpy as np
import pytest

import inputs as I
from conftest import golden
from helpers import build_tgn

pytestmark = pytest.mark.gpu
LDS_STATES = 1280
DTYPES = (np.int32, np.int32, np.float32, np.float32)
NAMES = ("nodes", "eidx", "dt", "w")
# shape -> (largest walk: states emitted, largest dictionary: distinct states) over the 120 queries, computed on the CPU
SHAPES = {(36, 2): (1332, 1304), (11, 3): (1463, 1413), (20, 3): (8420, 7078), (6, 5): (9330, 7423), (3000, 1): (3000, 2942),
          (1281, 1): (1281, 1265)}


def _outs(n, k, fill=0):
    return [np.full((n, k), fill, dt) for dt in DTYPES]


def _same(a, b, what=""):
    for x, y, nm in zip(a, b, NAMES):
        assert np.array_equal(x, y), "%s differs %s" % (nm, what)


class Env:
    def __init__(self, zt, oracle):
        self.src, self.dst, self.neg, self.ts, self.eidx = I.make_stream("hub", 400, 24000, 305)
        self.data = types.SimpleNamespace(sources=self.src, destinations=self.dst, edge_idxs=self.eidx, timestamps=self.ts)
        self.zt = zt
        self.nf = zt.get_neighbor_finder(self.data)
        self.csr = oracle.CsrOracle(self.src, self.dst, self.eidx, self.ts, self.nf.num_nodes)
        self.q = np.concatenate([self.src[-40:], self.dst[-40:], self.neg[-40:]]).astype(np.int32)
        self.qt = np.concatenate([self.ts[-40:]] * 3)
        self._ref = {}

    def finder(self):
        return self.zt.get_neighbor_finder(self.data)

    def ref(self, width, depth, alpha, beta, k, q=None, qt=None, tag="std"):
        """the oracle's answer, computed once per case and never written to afterwards"""
        key = (width, depth, alpha, beta, k, tag)
        if key not in self._ref:
            q, qt = (self.q, self.qt) if q is None else (q, qt)
            o = _outs(len(q), k)
            self.csr.get_pruned_topk(q, qt, width, depth, alpha, beta, k, *o)
            for a in o:
                a.setflags(write=False)
            self._ref[key] = o
        return self._ref[key]


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from zebra_amd import tppr
    return Env(tppr, oracle)


def _walk_sizes(nf, q, qt, width, depth):
    """(largest walk, largest dictionary) over the queries: states emitted and distinct states, from the exported CSR"""
    indptr, nbr, eid, ts = nf._indptr, nf._nbr, nf._eid, nf._ts
    big_walk = big_dict = 0
    for node, t in zip(q, qt):
        front, states = [(int(node), float(t))], []
        for _ in range(depth):
            new = []
            for v, tv in front:
                lo, hi = indptr[v], indptr[v + 1]
                n = int(np.searchsorted(ts[lo:hi], tv))
                c = min(n, width)
                sl = slice(lo + n - c, lo + n)
                new += list(zip(eid[sl][::-1].tolist(), nbr[sl][::-1].tolist(), ts[sl][::-1].tolist()))
            if not new:
                break
            states += new
            front = [(s[1], s[2]) for s in new]
        big_walk, big_dict = max(big_walk, len(states)), max(big_dict, len(set(states)))
    return big_walk, big_dict


@pytest.mark.parametrize("width,depth", list(SHAPES))
def test_fixture_walks_are_beyond_the_lds_form(env, width, depth):
    """A fixture that quietly fell back into LDS-sized lists would test nothing."""
    walk, dic = _walk_sizes(env.nf, env.q, env.qt, width, depth)
    print("%d x %d: largest walk %d, largest dictionary %d" % (width, depth, walk, dic))
    assert (walk, dic) == SHAPES[(width, depth)]
    assert walk > LDS_STATES
    assert walk > dic                                              # duplicate states to merge
    if (width, depth) != (1281, 1):                                # (its dictionary alone would fit: 1 265)
        assert dic > LDS_STATES
    assert env.nf.pruning_plan(width, depth, 1, 20)["form"] == "workspace"


CASES = [(w, d, 20, b) for (w, d) in SHAPES for b in (0.5, 0.95)] + \
        [(w, d, k, b) for (w, d) in ((20, 3), (3000, 1)) for k in (100, 255) for b in (0.5, 0.95)]


@pytest.mark.parametrize("width,depth,k,beta", CASES)
def test_wide_walk_vs_oracle(env, width, depth, k, beta):
    """get_pruned_topk on a finder that holds a workspace: all four outputs equal the oracle's, bit for bit.  beta = 0.5
    makes exact ties at the cut (the literal quicksort replay), 0.95 none (radix select + ranks)."""
    plan = env.nf.reserve_pruning(width, depth, 1, k)
    assert plan["form"] == "workspace" and plan["slabs"] >= 1
    got = _outs(len(env.q), k)
    assert env.nf.get_pruned_topk(env.q, env.qt, width, depth, 0.1, beta, k, *got) is None
    want = env.ref(width, depth, 0.1, beta, k)
    _same(got, want, "(%d x %d, k=%d, beta=%g)" % (width, depth, k, beta))
    if k <= 100:                                                   # (beyond, the smallest kept weights are below float32)
        assert (np.count_nonzero(want[3], axis=1) == k).any()      # some rows are full


# the LDS form at the top of its range, on the same queries: shape -> (largest walk, largest dictionary), computed on the CPU
LDS_SHAPES = {(35, 2): (1260, 1243), (2, 9): (1022, 980)}


@pytest.mark.parametrize("width,depth", list(LDS_SHAPES))
def test_lds_form_below_the_switch(env, width, depth):
    """The walk the two forms share, held to the oracle on the LDS side of the switch too: 35 x 2 fills 1 260 of the LDS
    form's 1 280 states (36 x 2 is the workspace's first shape), 2 x 9 walks nine levels with a frontier of 256."""
    import torch
    k = 20
    assert env.nf.pruning_plan(width, depth, 1, k)["form"] == "lds"
    walk, dic = _walk_sizes(env.nf, env.q, env.qt, width, depth)
    print("%d x %d: largest walk %d, largest dictionary %d" % (width, depth, walk, dic))
    assert (walk, dic) == LDS_SHAPES[(width, depth)]
    for beta in (0.5, 0.95):
        got = _outs(len(env.q), k)
        assert env.nf.get_pruned_topk(env.q, env.qt, width, depth, 0.1, beta, k, *got) is None
        _same(got, env.ref(width, depth, 0.1, beta, k), "(%d x %d, beta=%g)" % (width, depth, beta))
    if (width, depth) == (35, 2):                                  # two models in one call, against the single-model answers
        dev = torch.device("cuda")
        q, qt = torch.from_numpy(env.q).to(dev), torch.from_numpy(env.qt).to(dev)
        on = torch.zeros((2, len(env.q), k), dtype=torch.int32, device=dev)
        oe, od = torch.zeros_like(on), torch.zeros((2, len(env.q), k), dtype=torch.float32, device=dev)
        ow = torch.zeros_like(od)
        env.nf.pruned_topk_multi_device(q, qt, width, depth, [0.1, 0.1], [0.5, 0.95], k, on, oe, od, ow)
        for m, beta in enumerate((0.5, 0.95)):
            got = [x[m].cpu().numpy() for x in (on, oe, od, ow)]
            _same(got, env.ref(width, depth, 0.1, beta, k), "(model %d of 2)" % m)


@pytest.mark.parametrize("M", [2, 5])
@pytest.mark.parametrize("width,depth", [(11, 3), (20, 3)])
def test_models_share_one_walk(env, M, width, depth):
    """pruned_topk_multi_device: every (alpha, beta) model equals the oracle's single-model call; five models are more than
    one launch carries."""
    import torch
    k = 20
    al = [0.1, 0.1, 0.2, 0.0, 0.3][:M]
    be = [0.5, 0.95, 0.7, 0.5, 0.9][:M]
    env.nf.reserve_pruning(width, depth, M, k)
    dev = torch.device("cuda")
    q, qt = torch.from_numpy(env.q).to(dev), torch.from_numpy(env.qt).to(dev)
    on = torch.zeros((M, len(env.q), k), dtype=torch.int32, device=dev)
    oe, od = torch.zeros_like(on), torch.zeros((M, len(env.q), k), dtype=torch.float32, device=dev)
    ow = torch.zeros_like(od)
    env.nf.pruned_topk_multi_device(q, qt, width, depth, al, be, k, on, oe, od, ow)
    for m in range(M):
        got = [x[m].cpu().numpy() for x in (on, oe, od, ow)]
        _same(got, env.ref(width, depth, al[m], be[m], k), "(model %d of %d)" % (m, M))
    # the single-model public call gives the same bits as the oracle too (M = 1)
    got = _outs(len(env.q), k)
    env.nf.get_pruned_topk(env.q, env.qt, width, depth, al[1], be[1], k, *got)
    _same(got, env.ref(width, depth, al[1], be[1], k))


@pytest.mark.parametrize("width,depth", [(11, 3), (20, 3)])
def test_emit_edges(env, width, depth):
    """Empty rows, rows with fewer than k states, node 0, and an id out of range."""
    k = 20
    q = np.concatenate([env.q, env.src[[0, 4, 49]], env.dst[[0, 4, 49]], [0, 0]]).astype(np.int32)
    qt = np.concatenate([env.qt, env.ts[[0, 4, 49]], env.ts[[0, 4, 49]], [env.ts[0], env.ts[-1]]])
    want = env.ref(width, depth, 0.1, 0.5, k, q, qt, tag="edges")
    empty = (want[3] == 0).all(axis=1) & (want[0] == 0).all(axis=1) & (want[2] == 0).all(axis=1)
    nstates = np.count_nonzero(want[3], axis=1)
    assert empty.any() and ((nstates > 0) & (nstates < k)).any() and (nstates == k).any()
    nf = env.finder()
    nf.reserve_pruning(width, depth, 1, k)
    got = _outs(len(q), k, fill=7)
    nf.get_pruned_topk(q, qt, width, depth, 0.1, 0.5, k, *got)
    for x, y, nm in zip(got, want, NAMES):
        assert (x[empty] == 7).all(), nm                            # rows with an empty dictionary are left untouched
        assert np.array_equal(x[~empty], y[~empty]), nm
    bad = q.copy()
    bad[5] = nf.num_nodes + 3
    with pytest.raises(IndexError):
        nf.get_pruned_topk(bad, qt, width, depth, 0.1, 0.5, k, *_outs(len(q), k))
    again = _outs(len(env.q), k)
    nf.get_pruned_topk(env.q, env.qt, width, depth, 0.1, 0.5, k, *again)
    _same(again, env.ref(width, depth, 0.1, 0.5, k), "(after an out-of-range id)")


def test_slab_reuse(env):
    """One slab (a grid of one: every query reuses it), three slabs, the default budget: the same bits."""
    width, depth, k = 20, 3, 20
    want = env.ref(width, depth, 0.1, 0.5, k)
    nf = env.finder()
    one = nf.pruning_plan(width, depth, 1, k)["slab_bytes"]
    for budget, slabs in ((one, 1), (3 * one + 17, 3), (None, None)):
        plan = nf.reserve_pruning(width, depth, 1, k, budget) if budget else nf.reserve_pruning(width, depth, 1, k)
        if slabs:
            assert plan["slabs"] == slabs == plan["grid"]
        else:
            assert plan["slabs"] == min((1 << 30) // one, 768)
        got = _outs(len(env.q), k)
        nf.get_pruned_topk(env.q, env.qt, width, depth, 0.1, 0.5, k, *got)
        _same(got, want, "(%s slabs)" % plan["slabs"])
    with pytest.raises(ValueError, match=str(one)):
        nf.reserve_pruning(width, depth, 1, k, one - 1)
    # a reservation covers narrower walks, at any k and number of models
    got = _outs(len(env.q), 100)
    nf.get_pruned_topk(env.q, env.qt, 11, 3, 0.1, 0.95, 100, *got)
    _same(got, env.ref(11, 3, 0.1, 0.95, 100))


def test_without_a_reservation_wide_walks_are_refused(env):
    nf = env.finder()
    with pytest.raises(ValueError, match="zt_csr_reserve_pruning"):
        nf.get_pruned_topk(env.q, env.qt, 36, 2, 0.1, 0.5, 20, *_outs(len(env.q), 20))
    plain = _outs(len(env.q), 40)
    nf.get_pruned_topk(env.q, env.qt, 10, 2, 0.1, 0.5, 40, *plain)
    assert nf.reserve_pruning(10, 2, 1, 40)["form"] == "lds"       # reserves nothing
    with pytest.raises(ValueError):
        nf.get_pruned_topk(env.q, env.qt, 36, 2, 0.1, 0.5, 20, *_outs(len(env.q), 20))
    nf.reserve_pruning(36, 2, 1, 20)
    got = _outs(len(env.q), 20)
    nf.get_pruned_topk(env.q, env.qt, 36, 2, 0.1, 0.5, 20, *got)
    _same(got, env.ref(36, 2, 0.1, 0.5, 20))
    with pytest.raises(ValueError):                                # covers 36 x 2 only
        nf.get_pruned_topk(env.q, env.qt, 20, 3, 0.1, 0.5, 20, *_outs(len(env.q), 20))
    # the LDS form is untouched by a reservation: 10 x 2 gives the bits it gave without one
    held = _outs(len(env.q), 40)
    nf.get_pruned_topk(env.q, env.qt, 10, 2, 0.1, 0.5, 40, *held)
    _same(held, plain, "(10 x 2 with and without a reservation)")
    _same(held, env.ref(10, 2, 0.1, 0.5, 40))
    nf.release_pruning()
    with pytest.raises(ValueError):
        nf.get_pruned_topk(env.q, env.qt, 36, 2, 0.1, 0.5, 20, *_outs(len(env.q), 20))
    nf.release_pruning()                                           # twice is fine


def test_two_runs_give_the_same_bits(env):
    nf = env.finder()
    nf.reserve_pruning(6, 5, 1, 20)
    a, b = _outs(len(env.q), 20), _outs(len(env.q), 20)
    nf.get_pruned_topk(env.q, env.qt, 6, 5, 0.1, 0.5, 20, *a)
    nf.get_pruned_topk(env.q, env.qt, 6, 5, 0.1, 0.5, 20, *b)
    _same(a, b)


@pytest.mark.parametrize("name,width,depth", [("w36d2_k20", 36, 2), ("w11d3_k20", 11, 3)])
def test_wide_walk_golden(env, name, width, depth):
    """The kernel against the reference's own get_pruned_topk (tests/golden/gen_golden_wide_prune.py)."""
    g = golden("g13_prune_" + name)
    nf = env.finder()
    for v in g["probe"]:
        nb, ei, tt = nf.find_before(int(v), np.inf)
        assert np.array_equal(nb, g["adj%d_nbr" % v]) and np.array_equal(ei, g["adj%d_eid" % v])
        assert np.array_equal(tt, g["adj%d_ts" % v])
    nq, k = g["nodes"].shape
    nf.reserve_pruning(width, depth, 1, k)
    got = _outs(nq, k)
    nf.get_pruned_topk(g["q_nodes"], g["q_ts"], width, depth, 0.1, 0.5, k, *got)
    _same(got, [g[nm] for nm in NAMES], "from the reference")


def test_tgn_with_a_wide_walk(oracle):
    """A TGN whose pruning strategy walks 11 x 3 (what a reference checkout run with --n_degree 11 --n_layer 3 asks for):
    nobody reserves anything by hand.  Four eval batches directly and through the native pipeline: bit-equal to each other,
    and within the tolerance test_configs_gpu.py holds C4 to (1e-4) of the protocol oracle; then one training step."""
    import torch
    from zebra_amd.tppr import get_neighbor_finder
    TOL = 1e-4
    N, E, D, F, T, k, al, be, seed, bs, nb = 300, 3000, 20, 7, 100, 20, [0.1, 0.1], [0.5, 0.95], 77, 20, 4
    width, depth = 11, 3
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, seed)
    w = I.model_weights(D, F, T, len(al), seed)
    _, efeat = I.random_tables(N, E + 1, D, F, seed)
    tw = I.time_encode_weights(T)
    data = types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts)
    first = E - nb * bs
    t = [torch.from_numpy(x).cuda() for x in (src, dst, neg, ts, eidx)]
    batches = [tuple(x[first + b * bs:first + (b + 1) * bs] for x in t) for b in range(nb)]
    outs = {}
    for mode in ("seq", "pipe"):
        nf = get_neighbor_finder(data)
        assert getattr(nf, "_reserved", None) is None               # the constructor reserves nothing
        tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat, strategy="pruning", nf=nf, width=width, depth=depth).eval()
        if mode == "pipe":
            tgn.enable_pipeline(tppr_cus=0, max_batch=bs)
        try:
            embs = []
            with torch.cuda.stream(getattr(tgn, "main_stream", None) or torch.cuda.current_stream()):
                for b, cur in enumerate(batches):
                    embs.append((tgn.step_device(*cur, ahead=batches[b + 1:b + 4]) if mode == "pipe"
                                 else tgn.step_device(*cur)).clone())
            torch.cuda.synchronize()
        finally:
            if mode == "pipe":
                tgn.enable_pipeline(False)
        assert nf._reserved["form"] == "workspace" and nf._reserved["cap_c"] == 1463
        m = tgn.memory
        outs[mode] = (torch.stack(embs), m.memory.clone(), m.last_update.clone(), m.messages.clone())
        st = tgn.embedding_module._status
        assert st is None or int(st.item()) == 0
    for q in range(4):
        assert torch.equal(outs["seq"][q], outs["pipe"][q]), q
    p = oracle.ProtocolOracle(N, D, F, T, k, al, be, w, efeat, tw, "pruning", oracle.CsrOracle(src, dst, eidx, ts, N),
                              width, depth, n_threads=8)
    for b in range(nb):
        s, e = first + b * bs, first + (b + 1) * bs
        ref, _ = p.batch(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], False)
        d = float(np.abs(outs["seq"][0][b].cpu().numpy() - ref).max())
        assert d <= TOL, "embeddings of batch %d differ from the oracle by %g" % (b, d)
    assert np.abs(outs["seq"][1].cpu().numpy() - p.mem.memory).max() <= TOL
    assert np.array_equal(outs["seq"][2].cpu().numpy(), p.mem.last_update)
    assert outs["seq"][0].abs().max() > 0 and outs["seq"][1].abs().max() > 0
    # one training step
    nf = get_neighbor_finder(data)
    tgn = build_tgn(N, E + 1, D, F, T, k, al, be, w, efeat, strategy="pruning", nf=nf, width=width, depth=depth).train()
    s, e = first, first + bs
    pos, negp = tgn.compute_edge_probabilities(src[s:e], dst[s:e], neg[s:e], ts[s:e], eidx[s:e], 10, True)
    crit = torch.nn.BCELoss()
    loss = crit(pos.squeeze(), torch.ones(bs, device=pos.device)) + crit(negp.squeeze(), torch.zeros(bs, device=pos.device))
    loss.backward()
    grads = [pp.grad for pp in tgn.parameters() if pp.requires_grad and pp.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)
    assert nf._reserved["form"] == "workspace"
