"""Link-prediction scoring without a per-batch host round trip.

The reference's ``eval_edge_prediction`` (evaluation/evaluation.py:7-48) copies the probabilities
of every batch to the host and calls scikit-learn three times per batch.  Here the batch stays on
the device: the metrics below are torch ops (float64, the arithmetic scikit-learn does) on whatever
device the scores live on, the per-batch values are accumulated there, and the host reads three
numbers at the end.  Definitions follow scikit-learn exactly, ties included:

  average_precision  sum over distinct thresholds of (R_n - R_{n-1}) * P_n
                     (sklearn.metrics.average_precision_score)
  roc_auc            trapezoid under the ROC curve over distinct thresholds
                     (sklearn.metrics.roc_auc_score; equals P(pos > neg) + P(pos == neg) / 2)
  accuracy           np.argmax(np.hstack([pos, neg]), axis=1) == 0, i.e. pos >= neg
                     (evaluation/evaluation.py:40-45)
"""
import math

import numpy as np
import torch


def _curve(pos, neg):
    """Scores descending: cumulative true / false positives, the mask of the last element of every run
    of equal scores (= the distinct thresholds) and, per element, the index before its run starts
    (-1 for the first run).  Everything is a fixed-shape device op: no host synchronisation."""
    score = torch.cat([pos.reshape(-1), neg.reshape(-1)]).to(torch.float64)
    label = torch.cat([torch.ones(pos.numel(), dtype=torch.float64, device=score.device),
                       torch.zeros(neg.numel(), dtype=torch.float64, device=score.device)])
    order = torch.argsort(score, descending=True, stable=True)
    score, label = score[order], label[order]
    tps = torch.cumsum(label, 0)
    fps = torch.cumsum(1.0 - label, 0)
    idx = torch.arange(score.numel(), device=score.device)
    first = torch.ones_like(score, dtype=torch.bool)
    first[1:] = score[1:] != score[:-1]
    last = torch.ones_like(score, dtype=torch.bool)
    last[:-1] = first[1:]
    before = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), 0).values - 1
    return tps, fps, last, before


def _at(x, before):
    """x[before], 0 where before == -1."""
    return torch.where(before >= 0, x[before.clamp(min=0)], torch.zeros_like(x))


def average_precision(pos, neg):
    tps, fps, last, before = _curve(pos, neg)
    recall = tps / float(pos.numel())
    precision = tps / (tps + fps)
    term = (recall - _at(recall, before)) * precision
    return torch.sum(torch.where(last, term, torch.zeros_like(term)))


def roc_auc(pos, neg):
    tps, fps, last, before = _curve(pos, neg)
    tpr, fpr = tps / float(pos.numel()), fps / float(neg.numel())
    term = (fpr - _at(fpr, before)) * (tpr + _at(tpr, before)) * 0.5
    return torch.sum(torch.where(last, term, torch.zeros_like(term)))


def accuracy(pos, neg):
    return (pos.reshape(-1) >= neg.reshape(-1)).to(torch.float64).mean()


def link_metrics(pos, neg, out=None):
    """(average_precision, roc_auc, accuracy) of one batch as a float64[3] tensor on the scores' device.  CUDA scores of
    up to 16384 pairs go through ONE HIP kernel (zt_link_metrics, csrc/scoring.hip: bitonic sort in LDS + the two curve
    sums, in the form zt_link_metrics_plan picks -- one sort of (key | label) words up to 8192 pairs, the positives and the
    negatives as two sorted runs beyond; ``out`` given: the values are ADDED to it there, no extra op); anything else through
    the torch ops above -- the same definitions; the tests hold both to exact integer counts (oracle/metrics_exact.py).
    -0.0 and +0.0 are one threshold; NaN scores are outside the contract."""
    pos, neg = pos.reshape(-1), neg.reshape(-1)
    if pos.is_cuda and pos.dtype == torch.float32 and neg.dtype == torch.float32 and 0 < pos.numel() == neg.numel() <= 16384:
        import ctypes as C
        from ._capi import check, lib, ptr, stream_ptr
        acc = out if out is not None else torch.zeros(3, dtype=torch.float64, device=pos.device)
        check(lib().zt_link_metrics(ptr(pos.contiguous()), ptr(neg.contiguous()), C.c_int64(pos.numel()), ptr(acc),
                                    C.c_int32(1 if out is not None else 0), stream_ptr()), "zt_link_metrics")
        return acc
    m = torch.stack([average_precision(pos, neg), roc_auc(pos, neg), accuracy(pos, neg)])
    if out is not None:
        out += m
        return out
    return m


@torch.no_grad()
def eval_edge_prediction(model, negative_edge_sampler, data, n_neighbors, batch_size, native=False):
    """evaluation/evaluation.py:7-48 with the same protocol and return value (mean AP, mean AUC, mean
    accuracy over the batches); probabilities and metrics stay on the device, the host reads once.

    ``native=True``: the whole pass as ONE native call (TGN.run_device with the scorer and the metrics tail of the step,
    zt_pipeline_set_metrics) instead of a Python iteration, a staging copy and a host synchronisation per batch.  It needs a
    model with ``enable_pipeline()`` (RuntimeError otherwise; batches of at most the pipeline's ``max_batch``) and turns
    scoring and metrics on if they are off.  The negatives are drawn batch by batch first, in the same order (the sampler's
    RandomState sequence is the loop's); the T-PPR and step status words are checked once at the end.  The ``average_topk``
    statistics the stepwise pass collects for the embedding module are not collected in this mode."""
    if native:
        return _eval_edge_prediction_native(model, negative_edge_sampler, data, batch_size)
    assert negative_edge_sampler.seed is not None
    negative_edge_sampler.reset_random_state()
    model = model.eval()
    n = data.n_interactions
    nb = math.ceil(n / batch_size)
    acc = None
    for b in range(nb):
        s, e = b * batch_size, min(n, (b + 1) * batch_size)
        _, negatives = negative_edge_sampler.sample(e - s)
        pos, neg = model.compute_edge_probabilities(data.sources[s:e], data.destinations[s:e], negatives,
                                                    data.timestamps[s:e], data.edge_idxs[s:e], n_neighbors, train=False)
        if acc is None:
            acc = torch.zeros(3, dtype=torch.float64, device=pos.device)
        link_metrics(pos, neg, out=acc)
    out = (acc / nb).cpu().numpy()
    return float(out[0]), float(out[1]), float(out[2])


@torch.no_grad()
def _eval_edge_prediction_native(model, negative_edge_sampler, data, batch_size):
    from . import _capi
    assert negative_edge_sampler.seed is not None
    negative_edge_sampler.reset_random_state()
    model = model.eval()
    if getattr(model, "_pipe", None) is None:
        raise RuntimeError("eval_edge_prediction(native=True) needs a model with enable_pipeline()")
    n = data.n_interactions
    nb = math.ceil(n / batch_size)
    if nb == 0:
        return float("nan"), float("nan"), float("nan")
    cuts = [(b * batch_size, min(n, (b + 1) * batch_size)) for b in range(nb)]
    negatives = np.concatenate([np.asarray(negative_edge_sampler.sample(e - s)[1]) for s, e in cuts])
    if not getattr(model, "_score_on", False):
        model.enable_scoring()
    if not getattr(model, "_met_on", False):
        model.enable_metrics()
    with torch.cuda.stream(model.main_stream):
        model.metrics(reset=True)
        split = _capi.to_device(model.device, [np.ascontiguousarray(data.sources[:n], np.int32),
                                               np.ascontiguousarray(data.destinations[:n], np.int32),
                                               np.ascontiguousarray(negatives, np.int32),
                                               np.ascontiguousarray(data.timestamps[:n], np.float64),
                                               np.ascontiguousarray(data.edge_idxs[:n], np.int64)])
        batches = [tuple(x[s:e] for x in split) for s, e in cuts]        # the ragged last one included
        model.run_device(model.prepare_run(batches), out=None)
        total, measured, _ = model.metrics()
        out = (total / nb).cpu().numpy()                                 # (the one host synchronisation of the pass)
    model.check_status()
    if measured != nb:
        raise RuntimeError("%d of %d batches were measured" % (measured, nb))
    return float(out[0]), float(out[1]), float(out[2])


# ---------------------------------------------------------------------------------------------------------------------
# Node classification (evaluation/evaluation.py:51-79)
# ---------------------------------------------------------------------------------------------------------------------
def node_auc(prob, labels):
    """sklearn.metrics.roc_auc_score(labels, prob) for binary labels (1 / 0) as a float64 scalar tensor on the scores' device:
    ``roc_auc`` above on prob[labels == 1] and prob[labels == 0].  ValueError when only one class is present, as scikit-learn
    raises (that check reads two counts from the device)."""
    prob = torch.as_tensor(prob).reshape(-1)
    labels = torch.as_tensor(labels).reshape(-1).to(prob.device)
    if labels.numel() != prob.numel():
        raise ValueError("node_auc takes one label per score")
    is_pos = labels == 1
    pos, neg = prob[is_pos], prob[labels == 0]
    if pos.numel() + neg.numel() != prob.numel():
        raise ValueError("node_auc takes binary labels (0 / 1)")
    if pos.numel() == 0 or neg.numel() == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return roc_auc(pos, neg)


@torch.no_grad()
def eval_node_classification(tgn, decoder, data, batch_size, n_neighbors):
    """evaluation/evaluation.py:51-79 with the same protocol and return value (ROC-AUC of the decoder's probabilities on the
    source embeddings over the whole split): the TGN is stepped in eval mode with each batch's destinations as negatives, the
    probabilities of every batch are written into one device vector, the AUC is computed there (``roc_auc``, float64: a split can
    exceed what zt_link_metrics sorts, and labels are not paired) and the host reads it once."""
    decoder.eval()
    tgn.eval()
    n = len(data.sources)
    nb = math.ceil(n / batch_size)
    # the labels are host data: the two classes' positions are found there, so the device is read once, for the result
    lab = np.asarray(data.labels[:n])
    pos_i, neg_i = np.nonzero(lab == 1)[0], np.nonzero(lab == 0)[0]
    if len(pos_i) + len(neg_i) != n:
        raise ValueError("eval_node_classification takes binary labels (0 / 1)")
    if len(pos_i) == 0 or len(neg_i) == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    prob = torch.empty(n, dtype=torch.float32, device=tgn.device)
    for b in range(nb):
        s, e = b * batch_size, min(n, (b + 1) * batch_size)
        src_emb, _, _ = tgn.compute_temporal_embeddings(data.sources[s:e], data.destinations[s:e], data.destinations[s:e],
                                                        data.timestamps[s:e], data.edge_idxs[s:e], n_neighbors, train=False)
        prob[s:e] = decoder.predict(src_emb)
    from ._capi import to_device
    pos_d, neg_d = to_device(tgn.device, [pos_i.astype(np.int64), neg_i.astype(np.int64)])
    return float(roc_auc(prob.index_select(0, pos_d), prob.index_select(0, neg_d)).item())


# ---------------------------------------------------------------------------------------------------------------------
# Evaluation by rank: one positive against many negatives (MRR, Hits@k)
# ---------------------------------------------------------------------------------------------------------------------
def rank_metrics(prob, cand_idx=None, out=None, ranks=False):
    """zt_rank_metrics on float32 CUDA probabilities [Q, C]: column 0 is the positive, rank = 1 + #{c >= 1 present : p_c > p_0}
    + 0.5 #{c >= 1 present : p_c == p_0} -- the mean of the optimistic and the pessimistic rank; ``cand_idx`` [Q, C] (or None:
    all present) marks absent entries with -1, and a query whose positive is absent is skipped.  ADDS (sum of 1 / rank, Hits@1,
    Hits@3, Hits@10, queries counted) to the float64 [5] tensor ``out`` (None: a fresh one of zeros) and returns it -- with
    ``ranks=True`` (out, rank [Q]; 0 for a skipped query).  No host synchronisation."""
    import ctypes as C
    from ._capi import check, lib, ptr, stream_ptr
    if not (prob.is_cuda and prob.dtype == torch.float32 and prob.dim() == 2):
        raise ValueError("rank_metrics takes a float32 CUDA tensor [Q, C]")
    Q, Cn = prob.shape
    acc = out if out is not None else torch.zeros(5, dtype=torch.float64, device=prob.device)
    rk = torch.zeros(Q, dtype=torch.float32, device=prob.device) if ranks else None
    ix = None if cand_idx is None else cand_idx.to(prob.device, torch.int32).contiguous()
    if Q == 0 or Cn == 0:
        return (acc, rk) if ranks else acc
    check(lib().zt_rank_metrics(ptr(prob.contiguous()), ptr(ix), C.c_int64(Q), C.c_int64(Cn), ptr(rk), ptr(acc), stream_ptr()),
          "zt_rank_metrics")
    return (acc, rk) if ranks else acc


def rank_metrics_counts(thr, above, equal, out=None, ranks=False):
    """zt_rank_metrics_counts: ``rank_metrics`` from counts taken over a whole pool (TGN.count_scores / rank_of(counts=True)) --
    ``thr`` float32 [Q] the thresholds they were taken at, ``above`` / ``equal`` int32 [Q], all CUDA.  rank = 1 + above +
    0.5 equal in float64; a query whose threshold is NaN is skipped.  ADDS (sum of 1 / rank, Hits@1, Hits@3, Hits@10, queries
    counted) to the float64 [5] tensor ``out`` (None: a fresh one of zeros) and returns it -- with ``ranks=True`` (out, rank [Q]
    float64; 0 for a skipped query).  No host synchronisation."""
    import ctypes as C
    from ._capi import check, lib, ptr, stream_ptr
    if not (torch.is_tensor(thr) and thr.is_cuda and thr.dtype == torch.float32 and thr.dim() == 1):
        raise ValueError("rank_metrics_counts takes float32 CUDA thresholds [Q]")
    Q = thr.numel()
    for t in (above, equal):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.shape == (Q,)):
            raise ValueError("rank_metrics_counts takes int32 CUDA counts above [Q] and equal [Q]")
    if out is not None and not (out.is_cuda and out.dtype == torch.float64 and out.shape == (5,) and out.is_contiguous()):
        raise ValueError("rank_metrics_counts: out is a contiguous float64 CUDA tensor [5]")
    acc = out if out is not None else torch.zeros(5, dtype=torch.float64, device=thr.device)
    rk = torch.zeros(Q, dtype=torch.float64, device=thr.device) if ranks else None
    if Q == 0:
        return (acc, rk) if ranks else acc
    check(lib().zt_rank_metrics_counts(ptr(thr.contiguous()), ptr(above.contiguous()), ptr(equal.contiguous()), C.c_int64(Q),
                                       ptr(rk), ptr(acc), stream_ptr()), "zt_rank_metrics_counts")
    return (acc, rk) if ranks else acc


@torch.no_grad()
def eval_edge_ranking_full(model, data, n_neighbors, batch_size=200, filtered=False, finder=None, candidates=None,
                           pool_chunk=65536):
    """Link prediction by rank against the WHOLE pool: what ``TGN.recommend`` would have answered, measured.  Per batch, t0 is
    the batch's first timestamp; every source ranks its true destination among all node ids but its own (``candidates``: a 1-D
    list instead) read-only from the state BEFORE the batch -- ``TGN.rank_of(sources, t0, destinations, counts=True)``: the
    fused count kernel, prob[B, pool] never exists --, zt_rank_metrics_counts accumulates on the device; then the state advances
    with the ordinary eval step, whose single negative is the destination.  Returns dict(mrr, hits1, hits3, hits10) from one
    host read at the end.  The model runs without the native pipeline.
    THE PROTOCOL: this evaluates ``recommend`` as it answers -- everyone, sources and candidates, is embedded at t0, not at
    each edge's own time, and no edge of the batch is known to the state.  ``batch_size=1`` is the per-edge protocol, at the
    price of one embedding of the pool per edge.
    ``filtered=True``: a candidate does not count where it is a partner of the source strictly before the EDGE'S OWN timestamp
    in ``finder`` (None: ``model.neighbor_finder``; ValueError if there is none) -- embedded at t0, filtered at each edge's
    time.  The destination itself always has its rank."""
    if filtered and finder is None and model.neighbor_finder is None:
        raise ValueError("eval_edge_ranking_full(filtered=True) needs a finder: the model has no neighbor_finder")
    if int(batch_size) <= 0:
        raise ValueError("eval_edge_ranking_full takes batch_size > 0")
    model = model.eval()
    if not model.test_mode:                                      # (as the eval step begins)
        model.update_memory_in_test(model.memory)
        model.test_mode = True
    n = data.n_interactions
    acc = torch.zeros(5, dtype=torch.float64, device=model.device)
    exclude = None if not filtered else (finder if finder is not None else "seen")
    for s in range(0, n, batch_size):
        e = min(n, s + batch_size)
        above, equal, prob = model.rank_of(data.sources[s:e], float(data.timestamps[s]), data.destinations[s:e],
                                           candidates=candidates, pool_chunk=pool_chunk, exclude=exclude,
                                           exclude_timestamps=data.timestamps[s:e], counts=True)
        dst_d = torch.from_numpy(np.ascontiguousarray(data.destinations[s:e], np.int32)).to(model.device)
        thr = torch.where(dst_d >= 0, prob, torch.full_like(prob, float("nan")))
        rank_metrics_counts(thr, above, equal, out=acc)
        model.compute_temporal_embeddings(data.sources[s:e], data.destinations[s:e], data.destinations[s:e],
                                          data.timestamps[s:e], data.edge_idxs[s:e], n_neighbors, False)
    a = acc.cpu().numpy()                                        # (the one host read of the pass)
    q = a[4] if a[4] > 0 else float("nan")
    return dict(mrr=float(a[0] / q), hits1=float(a[1] / q), hits3=float(a[2] / q), hits10=float(a[3] / q))


@torch.no_grad()
def eval_edge_ranking(model, negative_edge_sampler, data, n_neighbors, batch_size=200, n_negatives=100, filtered=False,
                      finder=None):
    """Link prediction by rank, what temporal-graph benchmarks report: per batch, ``B * n_negatives`` negatives from ONE
    ``sampler.sample`` call, reshaped [B, n_negatives]; every source ranks [destination | its negatives] read-only from the
    state BEFORE the batch (TGN.rank_candidates), zt_rank_metrics accumulates on the device; then the state advances with the
    ordinary eval step, whose single negative is the first column.  Returns dict(mrr, hits1, hits3, hits10) from one host
    read at the end.  The model runs without the native pipeline.
    ``filtered=True`` is the filtered protocol: a negative does not count where it is one of the source's true partners --
    a partner strictly before the edge's timestamp in ``finder`` (None: ``model.neighbor_finder``; ValueError if there is
    none), or the edge's own destination.  The positive, column 0, always counts.  The absent columns are marked on the device
    (TGN.absent_bits) and reach zt_rank_metrics as cand_idx = -1; still one host read at the end.
    A sampler that has ``sample_for`` (zebra_amd.sampling.NegativeSampler) draws per edge on the device instead: it is called
    with the batch's sources, destinations and timestamps and ``row_base`` = the batch's position in the split, and its rows
    [B, n_negatives] are used as they are -- a -1 is an absent column, never ranked against; ``filtered`` ORs its masks on top."""
    assert negative_edge_sampler.seed is not None
    if filtered and finder is None and model.neighbor_finder is None:
        raise ValueError("eval_edge_ranking(filtered=True) needs a finder: the model has no neighbor_finder")
    negative_edge_sampler.reset_random_state()
    model = model.eval()
    if not model.test_mode:                                      # (as the eval step begins)
        model.update_memory_in_test(model.memory)
        model.test_mode = True
    n = data.n_interactions
    acc = torch.zeros(5, dtype=torch.float64, device=model.device)
    on_device = hasattr(negative_edge_sampler, "sample_for")      # zebra_amd.sampling.NegativeSampler
    for s in range(0, n, batch_size):
        e = min(n, s + batch_size)
        if on_device:
            # per-edge negatives drawn on the device, row s + b of the split: the rows are used as they are, a -1 is an absent
            # column for rank_candidates and for zt_rank_metrics; the eval step's single negative is the first column, or
            # the edge's destination where that is -1 (its one read-back per batch, beside the step's own status read)
            neg_d, _ = negative_edge_sampler.sample_for(data.sources[s:e], data.destinations[s:e], data.timestamps[s:e],
                                                        n_negatives, row_base=s)
            neg_d = neg_d.to(model.device)
            dst_d = torch.from_numpy(np.ascontiguousarray(data.destinations[s:e], np.int32)).to(model.device)
            cand_d = torch.cat([dst_d.reshape(-1, 1), neg_d], dim=1).contiguous()
            prob = model.rank_candidates(data.sources[s:e], data.timestamps[s:e], cand_d)
            gone = cand_d < 0
            if filtered:
                from .tgn import absent_columns
                bits = model.absent_bits(data.sources[s:e], data.timestamps[s:e], finder if finder is not None else "seen",
                                         candidates=cand_d)
                gone = gone | absent_columns(bits, cand_d.shape[1]) | (cand_d == cand_d[:, :1])
                gone[:, 0] = False                                   # the positive is never filtered
            rank_metrics(prob.float(), -gone.to(torch.int32), out=acc)
            first = torch.where(neg_d[:, 0] >= 0, neg_d[:, 0], dst_d).cpu().numpy()
            model.compute_temporal_embeddings(data.sources[s:e], data.destinations[s:e], first, data.timestamps[s:e],
                                              data.edge_idxs[s:e], n_neighbors, False)
            continue
        _, negatives = negative_edge_sampler.sample((e - s) * n_negatives)
        negatives = np.asarray(negatives).reshape(e - s, n_negatives)
        cands = np.concatenate([np.asarray(data.destinations[s:e]).reshape(-1, 1), negatives], axis=1)
        prob = model.rank_candidates(data.sources[s:e], data.timestamps[s:e], cands)
        cand_idx = None
        if filtered:
            from .tgn import absent_columns
            cand_d = torch.from_numpy(np.ascontiguousarray(cands, np.int32)).to(model.device)
            bits = model.absent_bits(data.sources[s:e], data.timestamps[s:e], finder if finder is not None else "seen",
                                     candidates=cand_d)
            gone = absent_columns(bits, cand_d.shape[1]) | (cand_d == cand_d[:, :1])
            gone[:, 0] = False                                       # the positive is never filtered
            cand_idx = -gone.to(torch.int32)                         # 0: present, -1: absent
        rank_metrics(prob.float(), cand_idx, out=acc)
        model.compute_temporal_embeddings(data.sources[s:e], data.destinations[s:e], negatives[:, 0], data.timestamps[s:e],
                                          data.edge_idxs[s:e], n_neighbors, False)
    a = acc.cpu().numpy()                                        # (the one host read of the pass)
    q = a[4] if a[4] > 0 else float("nan")
    return dict(mrr=float(a[0] / q), hits1=float(a[1] / q), hits3=float(a[2] / q), hits10=float(a[3] / q))
