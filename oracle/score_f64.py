"""Plain float64 restatement of the link scorers: the reference's MergeLayer (utils/util.py:14-26) as
compute_edge_probabilities applies it (model/tgn_model.py:185-188), in its CONCATENATION form -- one product of
[x1 | x2] with fc1.weight as it lies -- not the split form W_a x1 + W_b x2 the kernels compute.

TEST INFRASTRUCTURE ONLY (like everything under oracle/): imported by tests/, never by zebra_amd/, and it imports
nothing from zebra_amd/.  Every entry point takes the float32 / int arrays the kernels get and computes in float64 from
them.  Non-finite inputs follow IEEE arithmetic and numpy's maximum (NaN stays NaN), as torch's composition does.

merge_layer_f64   a batch's B positive pairs (src, dst) and B negative pairs (src, neg) from its [3B][H] embeddings
rank_f64          Q queries against C candidates each (rows of emb_c named by cand_idx; -1: absent, probability 0)
Both return (z, p): the logit fc2(relu(fc1(.))) and the probability 1 / (1 + exp(-z)).
"""
import numpy as np


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).astype(np.float64)


def _merge(x, fc1_w, fc1_b, fc2_w, fc2_b):
    """x float64 [n][2H] -> (z [n], p [n])"""
    W1, b1, W2, b2 = _f64(fc1_w), _f64(fc1_b), _f64(fc2_w).reshape(-1), _f64(fc2_b).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        hid = np.maximum(x @ W1.T + b1, 0.0)
        z = hid @ W2 + b2[0]
        p = 1.0 / (1.0 + np.exp(-z))
    return z, p


def merge_layer_f64(emb, fc1_w, fc1_b, fc2_w, fc2_b):
    """emb float32 [3B][H] = [src | dst | neg]; fc1_w [H][2H], fc1_b [H], fc2_w [1][H], fc2_b [1] in torch layout.
    Returns (z float64 [2B], p float64 [2B]): the B positive pairs, then the B negative ones."""
    e = _f64(emb)
    B = e.shape[0] // 3
    assert e.shape[0] == 3 * B
    x = np.concatenate([np.concatenate([e[:B], e[:B]]), e[B:]], axis=1)
    return _merge(x, fc1_w, fc1_b, fc2_w, fc2_b)


def rank_f64(emb_q, emb_c, cand_idx, weights):
    """emb_q float32 [Q][H], emb_c float32 [Nc][H]; cand_idx int [Q][C] names rows of emb_c (-1: absent) or is None: every
    query takes all Nc rows in order; weights = (fc1_w, fc1_b, fc2_w, fc2_b).  Returns (z, p) float64 [Q][C]; an absent
    entry has p = 0 exactly and z = -inf."""
    eq, ec = _f64(emb_q), _f64(emb_c)
    Q, Nc = eq.shape[0], ec.shape[0]
    idx = np.tile(np.arange(Nc, dtype=np.int64), (Q, 1)) if cand_idx is None else np.asarray(cand_idx).astype(np.int64)
    assert idx.shape[0] == Q and idx.min(initial=0) >= -1 and idx.max(initial=-1) < Nc
    z = np.full(idx.shape, -np.inf)
    p = np.zeros(idx.shape)
    for q in range(Q):
        live = idx[q] >= 0
        rows = ec[idx[q][live]]
        x = np.concatenate([np.broadcast_to(eq[q], rows.shape), rows], axis=1)
        z[q, live], p[q, live] = _merge(x, *weights)
    return z, p
