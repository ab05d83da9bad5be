"""Float64 restatements for the ranking step's tests (tests/test_rank_train_cpu.py, tests/test_rank_train_gpu.py): the
one-vs-many scorer as torch composes it (MergeLayer over [emb_q[q] | emb_c[cand_idx[q, c]]], -inf where the index is -1), the
two listwise losses, inputs for both, and the check of an index matrix's transpose."""
import numpy as np
import torch

NEG_INF = float("-inf")


def scorer_weights(H, seed):
    """[fc1.weight [H, 2H], fc1.bias [H], fc2.weight [1, H], fc2.bias [1]] (float32 numpy) for ANY width, drawn as
    tests/golden/inputs.py: model_weights draws a scorer's"""
    rng = np.random.RandomState(seed)

    def lin(o, i):
        return ((rng.standard_normal((o, i)) * np.sqrt(2.0 / (o + i))).astype(np.float32),
                (rng.uniform(-1, 1, o) / np.sqrt(i)).astype(np.float32))

    w1, b1 = lin(H, 2 * H)
    w2, b2 = lin(1, H)
    return [w1, b1, w2, b2]


def merge_layer(H, wts, dtype, device):
    from zebra_amd.modules import MergeLayer
    m = MergeLayer(H, H, H, 1).to(dtype)
    with torch.no_grad():
        for p, w in zip((m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias), wts):
            p.copy_(torch.from_numpy(w).to(dtype))
    return m.to(device)


def composed_logits(m, emb_q, emb_c, cand_idx, chunk=None):
    """logits [Q, C] of MergeLayer ``m`` under autograd, in m's dtype, on its device: -inf where cand_idx is -1.  The hidden
    layer [Q, C, H] IS materialised here (a chunk of queries at a time): this is the reference, not the product."""
    Q, H = emb_q.shape
    Nc = emb_c.shape[0]
    C_ = Nc if cand_idx is None else cand_idx.shape[1]
    chunk = chunk or max(1, (1 << 23) // max(1, C_ * 2 * H))
    out = []
    for s in range(0, Q, chunk):
        q = emb_q[s:s + chunk]
        if cand_idx is None:
            ec = emb_c.unsqueeze(0).expand(q.shape[0], Nc, H)
        else:
            ix = cand_idx[s:s + chunk].long()
            ec = emb_c[ix.clamp(min=0)]
        x = torch.cat([q.unsqueeze(1).expand(-1, C_, -1), ec], dim=2).reshape(-1, 2 * H)
        lg = m(x[:, :H], x[:, H:]).reshape(q.shape[0], C_)
        if cand_idx is not None:
            lg = lg.masked_fill(ix < 0, NEG_INF)
        out.append(lg)
    return torch.cat(out)


def composed_scorer(m, emb_q, emb_c, cand_idx, dl):
    """[logits, d_emb_q, d_emb_c, d fc1.weight, d fc1.bias, d fc2.weight, d fc2.bias] of the composition at
    d(loss)/d(logit) = dl (ignored at absent pairs)"""
    m.zero_grad()
    eq, ec = emb_q.clone().requires_grad_(True), emb_c.clone().requires_grad_(True)
    lg = composed_logits(m, eq, ec, cand_idx)
    live = lg != NEG_INF
    (torch.where(live, lg, torch.zeros_like(lg)) * torch.where(live, dl, torch.zeros_like(dl))).sum().backward()
    zero = lambda g, like: g if g is not None else torch.zeros_like(like)
    return [lg.detach(), zero(eq.grad, eq), zero(ec.grad, ec)] + [zero(p.grad, p).clone() for p in
                                                                   (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)]


def rank_loss_f64(logits, target=None, mode="softmax"):
    """The listwise loss restated in float64 under autograd -> (loss, d loss / d logits) as float64 CPU tensors.  A column is
    absent where the logit is -inf; a query whose target column is absent is skipped; no live query: (0, zeros).
      softmax: mean over live q of logsumexp over present c - logit[q, t_q]
      bce:     mean over live q of -max(log sigmoid(logit[q, t_q]), -100)
               + mean over the present non-target pairs of live q of -max(log(1 - sigmoid(logit)), -100)
    (autograd cuts the gradient where the clamp is active, the kernels' is sigma - y throughout, as BCELoss's own backward:
    the tests compare gradients where no clamp is active, |logit| < 100)."""
    lg = logits.detach().double().cpu().clone()
    Q, C = lg.shape
    t = torch.zeros(Q, dtype=torch.long) if target is None else target.detach().cpu().long()
    present = lg != NEG_INF
    live = present[torch.arange(Q), t]
    x = torch.where(present, lg, torch.zeros_like(lg)).requires_grad_(True)
    if not bool(live.any()):
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(lg)
    onehot = torch.zeros_like(present)
    onehot[torch.arange(Q), t] = True
    if mode == "softmax":
        masked = torch.where(present, x, torch.full_like(x, NEG_INF))
        per_q = torch.logsumexp(masked[live], dim=1) - x[live][onehot[live]]
        loss = per_q.mean()
    else:
        logsig = lambda v: -torch.nn.functional.softplus(-v)
        pos = x[onehot & live.unsqueeze(1)]
        negm = present & ~onehot & live.unsqueeze(1)
        loss = (-logsig(pos).clamp(min=-100)).mean()
        if bool(negm.any()):
            loss = loss + (-logsig(-x[negm]).clamp(min=-100)).mean()
    loss.backward()
    return loss.detach(), torch.where(present, x.grad, torch.zeros_like(lg))


def check_transpose(cand_idx, Nc, row_ptr, pairs):
    """Asserts that (row_ptr, pairs) is the transpose of cand_idx [Q, C]: every present pair exactly once, under the row it
    names, ascending within a row; a row nobody names has an empty range."""
    ix = np.asarray(cand_idx.cpu())
    row_ptr, pairs = np.asarray(row_ptr.cpu()), np.asarray(pairs.cpu())
    flat = ix.reshape(-1)
    assert row_ptr.shape == (Nc + 1,) and row_ptr[0] == 0 and row_ptr[-1] == pairs.size
    assert np.all(np.diff(row_ptr) >= 0)
    assert pairs.size == int((flat >= 0).sum())
    assert np.unique(pairs).size == pairs.size                      # each pair once
    for r in range(Nc):
        seg = pairs[row_ptr[r]:row_ptr[r + 1]]
        assert np.all(flat[seg] == r), r
        assert np.all(np.diff(seg) > 0), r                          # ascending pair id
        assert seg.size == int((flat == r).sum()), r                # (an unreferenced row: empty)


def scorer_inputs(Q, C, H, Nc=None, seed=0):
    """(emb_q [Q, H], emb_c [Nc, H], dl [Q, C], weights): embeddings randn * 0.7 as tests/test_scoring_train_gpu.py draws them;
    dl at the scale a mean loss gives -- O(1 / Q) per row, spread over the C columns: the positive's -(c / Q), the others'
    +(c / Q) / max(C - 1, 1), c in 1/4 .. 3/4 (that file's _inputs explains the constant)."""
    Nc = C if Nc is None else Nc
    g = torch.Generator().manual_seed(100003 * H + 1009 * Q + C + seed)
    emb_q = torch.randn((Q, H), generator=g) * 0.7
    emb_c = torch.randn((Nc, H), generator=g) * 0.7
    c = (0.25 + 0.5 * torch.rand((Q, C), generator=g)) / Q
    dl = c / max(C - 1, 1)
    dl[:, 0] = -c[:, 0]
    return emb_q, emb_c, dl, scorer_weights(H, 7 + H)
