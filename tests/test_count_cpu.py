"""The parts of the full-pool rank that need no GPU: TGN.count_scores on CPU tensors (its torch composition) against a numpy
brute force, the argument checks of evaluation.rank_metrics_counts, and eval_edge_ranking_full's ValueErrors."""
import types

import numpy as np
import pytest
import torch

import helpers_count_planted as K


def _holder(H, seed):
    from zebra_amd.modules import MergeLayer
    from zebra_amd.tgn import TGN
    torch.manual_seed(seed)
    holder = types.SimpleNamespace(affinity_score=MergeLayer(H, H, H, 1), device=torch.device("cpu"))
    for name in ("rank_scores", "count_scores"):
        setattr(holder, name, types.MethodType(getattr(TGN, name), holder))
    return holder


@pytest.mark.parametrize("H", [20, 22])
def test_count_scores_on_cpu_tensors_against_numpy(H):
    Q, C_, base = 5, 150, 300
    rk = _holder(H, H)
    rng = np.random.RandomState(H)
    eq = torch.from_numpy(rng.standard_normal((Q, H)).astype(np.float32))
    emb_c = rng.standard_normal((C_, H)).astype(np.float32)
    emb_c[100:110] = emb_c[1]                                  # ties with query 1's threshold
    emb_c[33, 2] = np.nan
    ec = torch.from_numpy(emb_c)
    prob = rk.rank_scores(eq, ec).numpy()
    assert np.isnan(prob[:, 33]).all()
    thr = prob[np.arange(Q), np.arange(Q)].copy()
    thr[4] = np.nan
    mask = rng.random_sample((Q, C_)) < 0.3
    skip = np.stack([base + rng.randint(0, C_, Q), np.full(Q, -1), base + np.arange(Q) + 100, np.full(Q, 5)], axis=1).astype(np.int32)

    def brute(use_mask, use_skip):
        above, equal = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
        for q in range(Q):
            for c in range(C_):
                if np.isnan(prob[q, c]) or np.isnan(emb_c[c]).any() or (use_mask and mask[q, c]):
                    continue
                if use_skip and base + c in skip[q].tolist():
                    continue
                above[q] += prob[q, c] > thr[q]
                equal[q] += prob[q, c] == thr[q]
        return above, equal

    bits = torch.from_numpy(K.pack_bits(mask).view(np.int32))
    t = torch.from_numpy(thr)
    for use_mask in (False, True):
        for use_skip in (False, True):
            a, e = rk.count_scores(eq, ec, t, idx_base=base, absent=bits if use_mask else None,
                                   skip=torch.from_numpy(skip) if use_skip else None)
            wa, we = brute(use_mask, use_skip)
            assert a.dtype == torch.int32 and a.shape == (Q,) and not a.is_cuda
            assert np.array_equal(a.numpy(), wa) and np.array_equal(e.numpy(), we), (use_mask, use_skip)
    wa, we = brute(False, False)
    assert we[1] == 11 and wa[4] == we[4] == 0 and wa.max() > 20
    # the pool in pieces, backwards, under accumulate, onto incoming counts
    out = (torch.full((Q,), 3, dtype=torch.int32), torch.full((Q,), 4, dtype=torch.int32))
    for b, e_ in ((90, 150), (0, 33), (33, 90)):
        got = rk.count_scores(eq, ec[b:e_], t, idx_base=base + b, out=out, skip=torch.from_numpy(skip),
                              absent=torch.from_numpy(K.pack_bits(mask[:, b:e_]).view(np.int32)))
        assert got[0] is out[0] and got[1] is out[1]
    wa, we = brute(True, True)
    assert np.array_equal(out[0].numpy(), wa + 3) and np.array_equal(out[1].numpy(), we + 4)
    # empties, and the checks
    a, e = rk.count_scores(eq, ec[:0], t)
    assert a.tolist() == [0] * Q and e.tolist() == [0] * Q
    a, e = rk.count_scores(eq[:0], ec, t[:0])
    assert a.shape == (0,) and e.shape == (0,)
    for kw in (dict(skip=torch.zeros((Q, 5), dtype=torch.int32)), dict(skip=torch.zeros(Q - 1, dtype=torch.int32)),
               dict(absent=bits[:, :4]), dict(absent=bits[:-1]), dict(absent=bits.float()), dict(idx_base=-1),
               dict(idx_base=0x7fffffff - C_ + 1), dict(out=(out[0], out[1].long())), dict(out=(out[0][:-1], out[1][:-1]))):
        with pytest.raises(ValueError):
            rk.count_scores(eq, ec, t, **kw)
    with pytest.raises(ValueError):
        rk.count_scores(eq, ec, t[:-1])


def test_rank_metrics_counts_argument_checks():
    from zebra_amd import evaluation as ev
    thr = torch.zeros(4)
    cnt = torch.zeros(4, dtype=torch.int32)
    for args in ((thr, cnt, cnt), (thr.numpy(), cnt, cnt), (thr.double(), cnt, cnt), (thr.reshape(2, 2), cnt, cnt)):
        with pytest.raises(ValueError, match="thresholds"):                # CPU tensors, arrays, other dtypes and shapes
            ev.rank_metrics_counts(*args)


def test_eval_edge_ranking_full_value_errors():
    from zebra_amd import evaluation as ev
    model = types.SimpleNamespace(neighbor_finder=None)
    data = types.SimpleNamespace(n_interactions=0)
    with pytest.raises(ValueError, match="finder"):
        ev.eval_edge_ranking_full(model, data, 10, filtered=True)
    with pytest.raises(ValueError, match="batch_size"):
        ev.eval_edge_ranking_full(model, data, 10, batch_size=0)
