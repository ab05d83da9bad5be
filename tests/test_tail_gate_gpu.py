"""The gate of the release by member at the tail of the GRU kernel (pipeline.hip, "the gate at the tail of the GRU"): where a
step's GRU kernel is the last thing it puts on the main stream, one thread of that kernel waits for the NEXT batch's T-PPR
rows and the next step passes no gate of its own.

C5's shape made small -- 20 000 nodes, bs 1024 (3 B > 2048 rows: the gate is the one-wave form, not the wait inside the
aggregation kernel), k 20, two models, CU-masked streams, launch groups of 4 and 8 -- run three times over the same 12 batches:
with the library's pick, with every gate in front of its own step (ZT_RELEASE_MEMBER_FRONT) and with the release by launch
(ZT_RELEASE_LAUNCH).  C5's 12 288 rows take the persistent output layers (k_embed_out3) and the plain k_gru behind them; 3 072 rows
would take the tiled output layers fused with the GRU update (k_out_gru), which carries no gate, so the runs pin C5's form
(ZT_CHOICE_EMBED_OUT = ZT_OUT_PERSIST) -- and one case leaves the library's own form, where nothing may be carried.  Every step's embeddings, the memory, last_update and the T-PPR rows must be the same bits in the three
and within 1e-4 of the protocol oracle (reference model/tgn_model.py:124-174, utils/util.py:473-576).
"""
import numpy as np
import pytest
import torch

import inputs as I
from helpers import build_tgn

pytestmark = pytest.mark.gpu
TOL = 1e-4
D = T = 100
BS, NB, RAGGED = 1024, 12, 700               # 11 batches of 1024 and a last one of 700 (still more than 2048 rows)
N_NODES = 20_000


@pytest.fixture(scope="module")
def world(oracle):
    """The stream, the weights and the oracle's answers for the 12 batches (computed once, never changed)."""
    from zebra_amd import synth
    wl = dict(synth.WORKLOADS["c5"], n_nodes=N_NODES, n_edges=(NB + 1) * BS, bs=BS)
    E = wl["n_edges"]
    src, dst, ts, eidx = synth.power_law_stream(N_NODES, E, bipartite=None, seed=2020, perm_seed=7)
    neg = synth.negatives(dst, E, seed=2021)
    M, F, k = len(wl["alpha"]), wl["F"], wl["k"]
    w = I.model_weights(D, F, T, M, 404)
    efeat = synth.edge_features(E + 1, F, seed=405)
    tw = I.time_encode_weights(T)
    cuts = [(b * BS, (b + 1) * BS) for b in range(NB - 1)] + [((NB - 1) * BS, (NB - 1) * BS + RAGGED)]
    extra = (NB * BS, NB * BS + BS)          # one more batch: the step that shows the pipeline's latch is clear
    p = oracle.ProtocolOracle(N_NODES + 1, D, F, T, k, wl["alpha"], wl["beta"], w, efeat, tw, "streaming", None, 10, 2, n_threads=8)
    ref = [p.batch(src[a:b], dst[a:b], neg[a:b], ts[a:b], eidx[a:b], False) for a, b in cuts]
    ids = np.unique(np.concatenate([x[:cuts[-1][1]] for x in (src, dst, neg)])).astype(np.int64)
    state = [p.tppr.export_rows(m, ids) for m in range(M)]
    return dict(wl=wl, stream=(src, dst, neg, ts, eidx), w=w, efeat=efeat, cuts=cuts, extra=extra, ids=ids,
                ref_emb=[r[0] for r in ref], ref_state=state,
                ref_memory=p.mem.memory.copy(), ref_last_update=p.mem.last_update.copy())


def run(world, release, group, loop, scoring, out_form):
    """loop: 'native' (zt_pipeline_run), 'python' (step_device with the batches ahead in sight) or 'blind' (step_device with an
    empty ``ahead``)."""
    from zebra_amd import _capi
    wl = world["wl"]
    M, F, k = len(wl["alpha"]), wl["F"], wl["k"]
    _capi.set_kernel_choice(_capi.CHOICE_GROUP_RELEASE, release)
    _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, out_form)
    try:
        tgn = build_tgn(N_NODES + 1, len(world["efeat"]), D, F, T, k, wl["alpha"], wl["beta"], world["w"], world["efeat"]).eval()
        tgn.enable_pipeline(tppr_cus=64, max_batch=BS, group=group)
        if scoring:
            tgn.enable_scoring()
        dev = tgn.device
        t = [torch.from_numpy(x).to(dev) for x in world["stream"]]
        batches = [tuple(x[a:b] for x in t) for a, b in world["cuts"]]
        extra = tuple(x[world["extra"][0]:world["extra"][1]] for x in t)
        probs = []
        with torch.cuda.stream(tgn.main_stream):
            if loop == "native" and not scoring:
                out = torch.zeros((NB, 3 * BS, D * (M + 1)), dtype=torch.float32, device=dev)
                tgn.run_device(tgn.prepare_run(batches), out=out)
                embs = [out[q, :3 * b[0].numel()].clone() for q, b in enumerate(batches)]
            else:
                embs = []
                look = 3 * group + 1
                for q, cur in enumerate(batches):
                    embs.append(tgn.step_device(*cur, ahead=batches[q + 1: q + 1 + look] if loop != "blind" else []).clone())
                    if scoring:
                        probs.append(tgn.last_prob().clone())
        torch.cuda.synchronize()
        tgn.check_status()                                     # the T-PPR handle's latch and the steps' status words
        f = tgn.embedding_module.tppr_finder
        res = dict(carried=tgn.pipeline_tail_gates(), embs=[e.cpu().numpy() for e in embs], probs=[x.cpu().numpy() for x in probs],
                   memory=tgn.memory.memory.cpu().numpy(), last_update=tgn.memory.last_update.cpu().numpy(),
                   state=[f.export_rows(m, world["ids"]) for m in range(M)])
        # the pipeline's latch: a step call fails with what an earlier step's kernel latched -- this one must go through
        with torch.cuda.stream(tgn.main_stream):
            tgn.step_device(*extra, check_status=True)
        torch.cuda.synchronize()
        tgn.enable_pipeline(False)
        return res
    finally:
        _capi.set_kernel_choice(_capi.CHOICE_GROUP_RELEASE, 0)
        _capi.set_kernel_choice(_capi.CHOICE_EMBED_OUT, 0)


def against_oracle(world, r):
    for q, (e, ref) in enumerate(zip(r["embs"], world["ref_emb"])):
        d = float(np.abs(e - ref).max())
        assert e.shape == ref.shape and d <= TOL, "embeddings of batch %d differ from the oracle by %g" % (q, d)
    assert float(np.abs(r["memory"] - world["ref_memory"]).max()) <= TOL
    assert np.array_equal(r["last_update"], world["ref_last_update"])
    for m, (a, b) in enumerate(zip(r["state"], world["ref_state"])):
        for kk in a:
            assert np.array_equal(a[kk], b[kk]), "T-PPR state %s of model %d differs from the oracle" % (kk, m)


def same_bits(a, b, what):
    assert len(a["embs"]) == len(b["embs"])
    for q, (x, y) in enumerate(zip(a["embs"], b["embs"])):
        assert np.array_equal(x, y), "%s: embeddings of batch %d" % (what, q)
    for q, (x, y) in enumerate(zip(a["probs"], b["probs"])):
        assert np.array_equal(x, y), "%s: probabilities of batch %d" % (what, q)
    assert np.array_equal(a["memory"], b["memory"]), "%s: memory" % what
    assert np.array_equal(a["last_update"], b["last_update"]), "%s: last_update" % what
    for m, (x, y) in enumerate(zip(a["state"], b["state"])):
        for kk in x:
            assert np.array_equal(x[kk], y[kk]), "%s: T-PPR state %s of model %d" % (what, kk, m)


PERSIST, OWN = 3, 0                           # ZT_OUT_PERSIST (C5's output layers) / the library's pick for 3 072 rows (tiled, fused with the GRU)


@pytest.mark.parametrize("group,loop,scoring,out_form", [
    (4, "native", False, PERSIST),   # the batch loop bench.py times: the gates of batches 1 .. 11 ride on the GRU kernels before them --
                                     # batches 4 and 8 open a new launch group, batch 11 is ragged and has nothing ahead
    (8, "native", False, PERSIST),   # one launch group of eight, one of three
    (4, "python", False, PERSIST),   # the same steps from Python, the batches ahead in sight
    (4, "python", True, PERSIST),    # the scorer follows the GRU kernel: nothing is carried
    (4, "blind", False, PERSIST),    # an empty `ahead`: every batch is queried alone, no gate at all
    (4, "native", False, OWN),       # the GRU update shares its launch with the output layers: nothing is carried
])
def test_tail_gate_same_bits_as_front_gate_and_release_by_launch(world, group, loop, scoring, out_form):
    from zebra_amd import _capi
    pick = run(world, 0, group, loop, scoring, out_form)
    against_oracle(world, pick)
    # the path under test must have run: with the batches ahead in sight every step but the last carries the next batch's gate
    # (every launch group here has more than one member; the very first step may not, its GRU kernel is followed by the first
    # refresh of the projected table), and nothing is carried where the scorer follows the GRU or no batch is in sight
    if loop == "blind" or scoring or out_form == OWN:
        assert pick["carried"] == 0, pick["carried"]
    else:
        assert NB - 2 <= pick["carried"] <= NB - 1, pick["carried"]
    front = run(world, _capi.RELEASE_MEMBER_FRONT, group, loop, scoring, out_form)
    assert front["carried"] == 0, front["carried"]
    same_bits(pick, front, "library's pick against ZT_RELEASE_MEMBER_FRONT")
    launch = run(world, _capi.RELEASE_LAUNCH, group, loop, scoring, out_form)
    assert launch["carried"] == 0, launch["carried"]
    same_bits(pick, launch, "library's pick against ZT_RELEASE_LAUNCH")
