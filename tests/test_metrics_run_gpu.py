"""Per-batch AP / AUC / accuracy inside the native step loop (csrc/scoring.hip: the two-run form of the metrics kernel for
8193 .. 16384 pairs; csrc/pipeline.hip: zt_pipeline_set_metrics / zt_pipeline_metrics; TGN.enable_metrics / metrics;
evaluation.eval_edge_prediction(native=True)) against the float64 torch composition of zebra_amd.evaluation on the CPU (what
tests/test_evaluation_cpu.py holds against exact counts), against the exact counts of oracle/metrics_exact.py, against
scikit-learn where it imports, and against the same batches stepped one by one."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import inputs as I
from conftest import ROOT
from helpers import build_tgn

pytestmark = pytest.mark.gpu
ATOL = 1e-12


def composition(pos, neg):
    """(AP, AUC, accuracy) by zebra_amd.evaluation's torch ops on CPU float64 copies of the scores"""
    from zebra_amd import evaluation as ev
    p = torch.as_tensor(np.asarray(pos.detach().cpu() if torch.is_tensor(pos) else pos)).to(torch.float64)
    n = torch.as_tensor(np.asarray(neg.detach().cpu() if torch.is_tensor(neg) else neg)).to(torch.float64)
    return np.array([float(ev.average_precision(p, n)), float(ev.roc_auc(p, n)), float(ev.accuracy(p, n))])


def exact_metrics(pos, neg):
    """(AP, AUC, accuracy) from integer counts: oracle/metrics_exact.py"""
    p = os.path.join(ROOT, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import metrics_exact
    return metrics_exact.link_metrics_exact(pos, neg)


def draw(B, ties, seed=None):
    """the scores of test_link_metrics_kernel_matches_sklearn: clipped normals, rounded to one decimal for heavy ties"""
    rng = np.random.RandomState(B + (7 if ties else 0) if seed is None else seed)
    pos = np.clip(rng.normal(0.65, 0.2, B), 0, 1).astype(np.float32)
    neg = np.clip(rng.normal(0.4, 0.2, B), 0, 1).astype(np.float32)
    if ties:
        pos, neg = np.round(pos, 1), np.round(neg, 1)
    return pos, neg


def kernel(pos, neg, out=None):
    from zebra_amd import evaluation as ev
    return ev.link_metrics(torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), out=out)


# ---------------------------------------------------------------------------------------------------------
# the kernel beyond 8192 pairs
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8193, 12000, 16384])
@pytest.mark.parametrize("ties", [False, True])
def test_wide_form_matches_the_float64_composition(B, ties):
    """zt_link_metrics on 8193 .. 16384 pairs (positives and negatives sorted as two runs of 32-bit keys) against the CPU float64
    composition to 1e-12; the accumulating call twice gives twice the value to 1e-11; the same input twice gives equal bits."""
    from zebra_amd import _capi
    assert _capi.link_metrics_plan(B)["form"] == _capi.METRICS_FORM_SPLIT
    pos, neg = draw(B, ties)
    got = kernel(pos, neg)
    want = composition(pos, neg)
    g = got.cpu().numpy()
    print("B=%d ties=%s |kernel - composition| = %s" % (B, ties, np.abs(g - want)))
    assert np.allclose(g, want, rtol=0, atol=ATOL), (g, want)
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    kernel(pos, neg, out=acc)
    kernel(pos, neg, out=acc)
    assert np.allclose(acc.cpu().numpy(), 2 * want, rtol=0, atol=1e-11)
    again = kernel(pos, neg)
    assert torch.equal(got, again)


@pytest.mark.parametrize("B", [8193, 12000, 16384])
@pytest.mark.parametrize("ties", [False, True])
def test_wide_form_matches_sklearn(B, ties):
    """against the exact counts of oracle/metrics_exact.py always, and against scikit-learn where it imports"""
    pos, neg = draw(B, ties)
    got = kernel(pos, neg).cpu().numpy()
    want = exact_metrics(pos, neg)
    assert want[2] == float(np.mean(pos >= neg))
    assert np.allclose(got, want, rtol=0, atol=ATOL), (got, want)
    try:
        import sklearn.metrics as sk
    except ImportError:
        return
    y = np.concatenate([np.ones(B), np.zeros(B)])
    sc = np.concatenate([pos, neg]).astype(np.float64)
    want = [sk.average_precision_score(y, sc), sk.roc_auc_score(y, sc), float(np.mean(pos >= neg))]
    assert np.allclose(got, want, rtol=0, atol=ATOL), (got, want)


@pytest.mark.parametrize("case", ["all_equal", "separated", "inverted"])
def test_wide_form_degenerate_inputs(case):
    B = 8193
    if case == "all_equal":                       # one threshold
        pos, neg = np.full(B, 0.5, np.float32), np.full(B, 0.5, np.float32)
        exact = [0.5, 0.5, 1.0]
    elif case == "separated":                     # every positive above every negative
        rng = np.random.RandomState(3)
        pos, neg = rng.uniform(0.6, 1.0, B).astype(np.float32), rng.uniform(0.0, 0.4, B).astype(np.float32)
        exact = [1.0, 1.0, 1.0]
    else:                                         # positives all 0, negatives all 1
        pos, neg = np.zeros(B, np.float32), np.ones(B, np.float32)
        exact = [0.5, 0.0, 0.0]
    got = kernel(pos, neg).cpu().numpy()
    want = composition(pos, neg)
    assert np.allclose(want, exact, rtol=0, atol=ATOL), want
    assert np.allclose(got, want, rtol=0, atol=ATOL), (got, want)
    assert torch.equal(kernel(pos, neg), kernel(pos, neg))


@pytest.mark.parametrize("ties", [False, True])
def test_seam_between_the_two_forms(ties):
    """8192 pairs (the single sort of u64 words) and the same input extended by one pair (the two-run form)"""
    from zebra_amd import _capi
    pos, neg = draw(8193, ties, seed=811 + ties)
    for B, form in ((8192, _capi.METRICS_FORM_SINGLE), (8193, _capi.METRICS_FORM_SPLIT)):
        assert _capi.link_metrics_plan(B)["form"] == form
        got = kernel(pos[:B].copy(), neg[:B].copy()).cpu().numpy()
        want = composition(pos[:B], neg[:B])
        assert np.allclose(got, want, rtol=0, atol=ATOL), (B, got, want)


def test_python_routes_up_to_16384_pairs_to_the_library():
    """CUDA float32 scores of up to 16384 pairs take the kernel (float64 [3] on the device, bits repeat); beyond, and for other
    dtypes, the torch composition answers -- to the same values."""
    from zebra_amd import evaluation as ev
    pos, neg = draw(16385, False)
    p, n = torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda()
    beyond = ev.link_metrics(p, n).cpu().numpy()
    assert np.allclose(beyond, composition(pos, neg), rtol=0, atol=1e-9)
    dbl = ev.link_metrics(p[:9000].double(), n[:9000].double()).cpu().numpy()
    assert np.allclose(dbl, ev.link_metrics(p[:9000], n[:9000]).cpu().numpy(), rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------
# the tail of the native step
# ---------------------------------------------------------------------------------------------------------
D = T = 100
N, E, F, BS, K, AL, BE, SEED = 3000, 4070, 1, 400, 20, [0.1, 0.1], [0.5, 0.95], 77


@pytest.fixture(scope="module")
def world():
    from zebra_amd.tppr import get_neighbor_finder
    src, dst, neg, ts, eidx = I.make_stream("general", N, E, SEED)
    w = I.model_weights(D, F, T, 2, SEED)
    _, efeat = I.random_tables(N, E + 1, D, F, SEED)
    nf = get_neighbor_finder(types.SimpleNamespace(sources=src, destinations=dst, edge_idxs=eidx, timestamps=ts))
    return dict(stream=(src, dst, neg, ts, eidx), w=w, efeat=efeat, nf=nf, cache={})


def model(world, strategy, group, max_batch=512):
    tgn = build_tgn(N, E + 1, D, F, T, K, AL, BE, world["w"], world["efeat"], strategy=strategy,
                    nf=world["nf"] if strategy == "pruning" else None).eval()
    tgn.enable_pipeline(tppr_cus=0, max_batch=max_batch, group=group)
    tgn.enable_scoring()
    t = [torch.from_numpy(x).to(tgn.device) for x in world["stream"]]
    batches = [tuple(x[s0:s0 + BS] for x in t) for s0 in range(0, E, BS)]                # eleven; the last one has 70 edges
    return tgn, batches


def state(tgn, strategy):
    torch.cuda.synchronize()
    tgn.check_status()
    st = [tgn.embedding_module.tppr_finder.export_state(m) for m in range(2)] if strategy == "streaming" else []
    return (tgn.memory.memory.clone(), tgn.memory.messages.clone(), tgn.memory.last_update.clone()), st


def stepped(world, strategy, group, n, change_at=None):
    """Batches 0 .. n-1 stepped one by one, no metrics tail: per batch the embeddings, the probabilities and
    evaluation.link_metrics of them (the same kernel on the same scores); the state afterwards.  Computed once per case."""
    key = (strategy, group, n, change_at)
    if key not in world["cache"]:
        from zebra_amd import evaluation as ev
        tgn, batches = model(world, strategy, group)
        embs, probs, rows = [], [], []
        with torch.cuda.stream(tgn.main_stream):
            for q, cur in enumerate(batches[:n]):
                if q == change_at:
                    with torch.no_grad():
                        tgn.affinity_score.fc1.bias.add_(0.1)
                embs.append(tgn.step_device(*cur, ahead=batches[q + 1: min(n, q + 1 + 3 * group)]).clone())
                B = cur[0].numel()
                prob = tgn.last_prob()
                rows.append(ev.link_metrics(prob[:B], prob[B:]).clone())
                probs.append(prob.clone())
        st = state(tgn, strategy)
        tgn.enable_pipeline(False)
        world["cache"][key] = dict(embs=embs, probs=[p.cpu() for p in probs], rows=torch.stack(rows).cpu(), state=st)
    return world["cache"][key]


def same_state(a, b):
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        for kk in x:
            assert np.array_equal(x[kk], y[kk]), kk


@pytest.mark.parametrize("strategy,group", [("streaming", 1), ("streaming", 3), ("pruning", 1)])
def test_tail_matches_stepping_and_disturbs_nothing(world, strategy, group):
    ref = stepped(world, strategy, group, 11)
    res = {}
    for mode in ("metrics", "plain"):
        tgn, batches = model(world, strategy, group)
        if mode == "metrics":
            tgn.enable_metrics(per_batch=11)
        out = torch.zeros((11, 3 * BS, 300), dtype=torch.float32, device=tgn.device)
        with torch.cuda.stream(tgn.main_stream):
            tgn.run_device(tgn.prepare_run(batches), out=out)
            if mode == "metrics":
                total, n, rows = tgn.metrics()
                total, rows = total.clone(), rows.clone()
        st = state(tgn, strategy)
        if mode == "metrics":
            assert n == 11
            res["sum"], res["rows"] = total.cpu(), rows.cpu()
        res[mode] = (out.cpu(), st)
        tgn.enable_pipeline(False)
    rows = res["rows"]
    assert rows.shape == (11, 3)
    assert torch.equal(rows, ref["rows"])                                 # the same kernel on the same probabilities
    acc = torch.zeros(3, dtype=torch.float64)
    for q in range(11):
        acc += rows[q]                                                    # first to last: the order of the message stream
    assert torch.equal(res["sum"], acc)
    for q in range(11):
        B = ref["probs"][q].numel() // 2
        want = composition(ref["probs"][q][:B], ref["probs"][q][B:])
        assert np.allclose(rows[q].numpy(), want, rtol=0, atol=ATOL), (q, rows[q], want)
    # the tail disturbs nothing: embeddings and state of a run without it, and of the stepped batches
    assert torch.equal(res["metrics"][0], res["plain"][0])
    for q in range(11):
        B3 = ref["embs"][q].shape[0]
        assert torch.equal(res["metrics"][0][q, :B3], ref["embs"][q].cpu()), q
    same_state(res["metrics"][1], res["plain"][1])
    same_state(res["metrics"][1], ref["state"])


def test_a_half_is_measured_before_the_scorer_rewrites_it(world):
    """Two runs of four batches with the scorer's fc1.bias changed in place between them: rows 0-3 are those of the old weights,
    rows 4-7 those of the new ones -- each metrics kernel read its half of the probabilities before the scorer of two steps
    later rewrote it, and after its own scorer had written it."""
    ref = stepped(world, "streaming", 1, 8, change_at=4)
    old = stepped(world, "streaming", 1, 8)
    tgn, batches = model(world, "streaming", 1)
    tgn.enable_metrics(per_batch=8)
    with torch.cuda.stream(tgn.main_stream):
        tgn.run_device(tgn.prepare_run(batches[:4]))
        with torch.no_grad():
            tgn.affinity_score.fc1.bias.add_(0.1)
        tgn.run_device(tgn.prepare_run(batches[4:8]))
        total, n, rows = tgn.metrics()
        rows = rows.clone()
    torch.cuda.synchronize()
    tgn.check_status()
    tgn.enable_pipeline(False)
    rows = rows.cpu()
    assert n == 8
    assert torch.equal(rows, ref["rows"])
    assert torch.equal(rows[:4], old["rows"][:4])
    for q in range(4, 8):
        assert not torch.equal(ref["probs"][q], old["probs"][q]), q         # (the change moves every later batch's scores)


def test_one_wide_batch_through_the_pipeline():
    """Batches of 8200 edges: the step's tail takes the two-run form of the kernel"""
    n_nodes, bs = 3000, 8200
    src, dst, neg, ts, eidx = I.make_stream("general", n_nodes, 2 * bs, 78)
    w = I.model_weights(D, F, T, 2, 78)
    _, efeat = I.random_tables(n_nodes, 2 * bs + 1, D, F, 78)
    got = {}
    for mode in ("run", "step"):
        tgn = build_tgn(n_nodes, 2 * bs + 1, D, F, T, K, AL, BE, w, efeat).eval()
        tgn.enable_pipeline(tppr_cus=0, max_batch=bs, group=1)
        tgn.enable_scoring()
        t = [torch.from_numpy(x).to(tgn.device) for x in (src, dst, neg, ts, eidx)]
        batches = [tuple(x[s0:s0 + bs] for x in t) for s0 in (0, bs)]
        with torch.cuda.stream(tgn.main_stream):
            if mode == "run":
                tgn.enable_metrics(per_batch=2)
                tgn.run_device(tgn.prepare_run(batches))
                _, n, rows = tgn.metrics()
                assert n == 2
                got[mode] = rows.clone()
            else:
                probs = []
                for q, cur in enumerate(batches):
                    tgn.step_device(*cur, ahead=batches[q + 1:])
                    probs.append(tgn.last_prob().clone())
                got[mode] = probs
        torch.cuda.synchronize()
        tgn.check_status()
        tgn.enable_pipeline(False)
        del tgn
    rows = got["run"].cpu().numpy()
    for q in range(2):
        want = composition(got["step"][q][:bs], got["step"][q][bs:])
        assert np.allclose(rows[q], want, rtol=0, atol=ATOL), (q, rows[q], want)


# ---------------------------------------------------------------------------------------------------------
# the validation pass
# ---------------------------------------------------------------------------------------------------------
class Sampler:                       # RandEdgeSampler's interface (utils/util.py:54-84)
    def __init__(self, dsts, seed):
        self.seed, self.dst_list = seed, np.unique(dsts)
        self.random_state = np.random.RandomState(seed)

    def reset_random_state(self):
        self.random_state = np.random.RandomState(self.seed)

    def sample(self, size):
        i = self.random_state.randint(0, len(self.dst_list), size)
        return self.dst_list[i], self.dst_list[self.random_state.randint(0, len(self.dst_list), size)]


def test_native_validation_pass_matches_the_stepwise_one():
    from zebra_amd import evaluation as ev
    n_nodes, n_edges, d, f, t_dim, k, al, be, seed, _, _ = I.EMBED_CASES["d100_f1"]
    src, dst, neg, ts, eidx = I.make_stream("general", n_nodes, n_edges, seed)
    w = I.model_weights(d, f, t_dim, len(al), seed)
    _, efeat = I.random_tables(n_nodes, n_edges + 1, d, f, seed)
    data = types.SimpleNamespace(sources=src, destinations=dst, timestamps=ts, edge_idxs=eidx, n_interactions=len(src))
    batch = 150
    assert math.ceil(len(src) / batch) == 3 and len(src) % batch != 0                         # a ragged last batch
    res = {}
    for native in (False, True):
        tgn = build_tgn(n_nodes, n_edges + 1, d, f, t_dim, k, al, be, w, efeat)
        tgn.enable_pipeline(tppr_cus=0, max_batch=256)
        if not native:
            tgn.enable_scoring()                  # (native=True turns scoring and metrics on itself)
        got = ev.eval_edge_prediction(tgn, Sampler(dst, 7), data, 10, batch, native=native)
        torch.cuda.synchronize()
        st = [tgn.embedding_module.tppr_finder.export_state(m) for m in range(len(al))]
        res[native] = (got, (tgn.memory.memory.clone(), tgn.memory.messages.clone(), tgn.memory.last_update.clone()), st)
        tgn.enable_pipeline(False)
    print("native=False %r native=True %r" % (res[False][0], res[True][0]))
    assert np.allclose(res[True][0], res[False][0], rtol=0, atol=ATOL), (res[True][0], res[False][0])
    assert all(0.0 <= v <= 1.0 for v in res[True][0])
    same_state(res[True][1:], res[False][1:])
    plain = build_tgn(n_nodes, n_edges + 1, d, f, t_dim, k, al, be, w, efeat)
    with pytest.raises(RuntimeError):
        ev.eval_edge_prediction(plain, Sampler(dst, 7), data, 10, batch, native=True)


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------
def test_metrics_need_a_pipeline_and_scoring(world):
    tgn = build_tgn(N, E + 1, D, F, T, K, AL, BE, world["w"], world["efeat"]).eval()
    with pytest.raises(RuntimeError):
        tgn.enable_metrics()
    tgn.enable_pipeline(tppr_cus=0, max_batch=512)
    with pytest.raises(RuntimeError):
        tgn.enable_metrics()
    with pytest.raises(RuntimeError):
        tgn.metrics()
    tgn.enable_scoring()
    tgn.enable_metrics()
    total, n, rows = tgn.metrics()
    assert n == 0 and rows is None and float(total.abs().sum()) == 0.0
    tgn.enable_scoring(False)                      # turning scoring off turns the tail off
    with pytest.raises(RuntimeError):
        tgn.metrics()
    tgn.enable_pipeline(False)


def test_metrics_refuse_batches_the_kernel_cannot_take(world):
    tgn = build_tgn(N, E + 1, D, F, T, K, AL, BE, world["w"], world["efeat"]).eval()
    tgn.enable_pipeline(tppr_cus=0, max_batch=20000)
    tgn.enable_scoring()
    with pytest.raises(ValueError, match="16384"):
        tgn.enable_metrics()
    tgn.enable_pipeline(False)


def test_a_batch_beyond_the_table_is_refused_before_it_is_enqueued(world):
    ref = stepped(world, "streaming", 1, 8)
    tgn, batches = model(world, "streaming", 1)
    tgn.enable_metrics(per_batch=8)
    with torch.cuda.stream(tgn.main_stream):
        with pytest.raises(ValueError, match="8 rows"):
            tgn.run_device(tgn.prepare_run(batches[:9]))
        total, n, rows = tgn.metrics()
        total, rows = total.clone(), rows.clone()
    torch.cuda.synchronize()
    assert n == 8
    assert torch.equal(rows.cpu(), ref["rows"])
    acc = torch.zeros(3, dtype=torch.float64)
    for q in range(8):
        acc += ref["rows"][q]
    assert torch.equal(total.cpu(), acc)
    # the state is that of eight steps: nothing of the ninth was enqueued on the main stream
    for x, y in zip((tgn.memory.memory, tgn.memory.messages, tgn.memory.last_update), ref["state"][0]):
        assert torch.equal(x, y)
    tgn.enable_pipeline(False)
