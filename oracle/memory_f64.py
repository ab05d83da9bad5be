"""Plain float64 restatement of the eval-time memory path: the raw-message store and the memory update.

TEST INFRASTRUCTURE ONLY (like everything under oracle/): imported by tests/, never by zebra_amd/, and it imports
nothing from zebra_amd/.  Every entry point takes the float32 / int arrays the kernels get and computes in float64 from
them, with the exceptions the reference model itself defines (model/tgn_model.py:204-226): the edge time is .float()ed,
the difference to last_update and its product with the frequencies are FLOAT32 (model/time_encoding.py:18-28 multiplies
float32 tensors), and the cosine is float64 cos of that float32 product -- the convention of aggregate_f64.time_encode_f64
and of test_time_encode_through_message_kernel.

store_messages  "the last message wins" (np.unique on the flipped batch in the reference): over the positions
                [src | dst] the LAST occurrence of a node writes [memory[v] | memory[partner] | efeat[e] | cos(dt w)]
cell_update     torch.nn.GRUCell / RNNCell (modules/memory_updater.py:29-57,95-103) on the flagged subset of ids[:n],
                Memory.clear_messages on every id considered
run_batches     the two composed over a run of batches: store, then update, per batch
"""
import numpy as np

CELL_GRU, CELL_RNN = "gru", "rnn"


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).astype(np.float64)


def store_messages(memory, last_update, efeat, time_w, src, dst, ts, eidx, pos_range=None):
    """memory [N, D], last_update [N], efeat [E, F], time_w [T]: float32 (memory may be float64: run_batches);
    src / dst int[B], ts float64[B], eidx int[B]; pos_range = (lo, hi): only winners at positions lo .. hi - 1 of
    [src | dst] write (every node's winner is still its last position in the WHOLE batch).

    Returns a dict: nodes int64[W] (the nodes written, in the order of their winning positions), pos int64[W],
    rows float64[W, 2 D + F + T], ts float32[W] (the .float()ed edge time) and winner int64[N] (the last position of
    every node in the batch, -1 where it does not occur).  The flags after the call are the flags before with
    flags[nodes] = 1; messages[nodes] = rows; timestamps[nodes] = ts."""
    mem = np.asarray(memory, np.float64)
    lu = np.asarray(last_update, np.float32)
    ef = _f64(efeat)
    tw = np.asarray(time_w, np.float32).reshape(-1)
    src, dst = np.asarray(src).astype(np.int64), np.asarray(dst).astype(np.int64)
    eidx = np.asarray(eidx).astype(np.int64)
    B = len(src)
    lo, hi = pos_range if pos_range is not None else (0, 2 * B)
    both = np.concatenate([src, dst])
    winner = np.full(len(mem), -1, np.int64)
    for p in range(2 * B):                                             # later positions overwrite earlier ones
        winner[both[p]] = p
    pos = np.sort(winner[winner >= 0])
    pos = pos[(pos >= lo) & (pos < hi)]
    i = np.where(pos < B, pos, pos - B)
    v = both[pos]
    partner = np.where(pos < B, dst[i], src[i])
    tf = np.asarray(ts, np.float64)[i].astype(np.float32)              # edge_times .float()
    delta = (tf - lu[v]).astype(np.float32)                            # float32 difference
    x = (delta[:, None] * tw[None, :]).astype(np.float32)              # float32 product
    rows = np.concatenate([mem[v], mem[partner], ef[eidx[i]], np.cos(x.astype(np.float64))], axis=1)
    return {"nodes": v, "pos": pos, "rows": rows, "ts": tf, "winner": winner}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def cell_update(cell, memory, last_update, messages, msg_ts, flags, ids, n, w_ih, w_hh, b_ih, b_hh):
    """cell: "gru" (weights [3 D, msg] / [3 D, D], gates r, z, n) or "rnn" ([D, msg] / [D, D], tanh).  ids: int[..] of
    which the first n are considered, or None: every node.  A duplicated id is applied once; ids < 0 or >= N and
    unflagged ids are ignored; the flag of every considered id in range is cleared; last_update[v] = msg_ts[v].

    Returns a dict: memory float64[N, D] (rows not updated: the input's values), last_update float32[N], flags uint8[N],
    rows int64[R] (the rows updated, ascending, each once) and pre: the float64 pre-activations of those rows --
    "r", "z", "n" [R, D] for the GRU (n = gi_n + b_in + r (gh_n + b_hn), the tanh's argument), "n" for the RNN."""
    mem = np.asarray(memory, np.float64).copy()
    lu = np.asarray(last_update, np.float32).copy()
    fl = np.asarray(flags, np.uint8).copy()
    N, D = mem.shape
    if ids is None:
        considered = np.arange(N, dtype=np.int64)
    else:
        considered = np.asarray(ids).astype(np.int64)[: int(n)]
        considered = np.unique(considered[(considered >= 0) & (considered < N)])
    rows = considered[fl[considered] != 0]
    fl[considered] = 0
    # (float64 messages -- run_batches -- are taken as they are: their float32 roundings would be another input)
    msgs = np.asarray(messages)
    x, h = (msgs if msgs.dtype == np.float64 else _f64(msgs))[rows], mem[rows]
    Wi, Wh, bi, bh = _f64(w_ih), _f64(w_hh), _f64(b_ih), _f64(b_hh)
    gi, gh = x @ Wi.T + bi, h @ Wh.T + bh
    if cell == CELL_RNN:
        pre = {"n": gi + gh}
        new = np.tanh(pre["n"])
    elif cell == CELL_GRU:
        r_pre, z_pre = gi[:, :D] + gh[:, :D], gi[:, D:2 * D] + gh[:, D:2 * D]
        r, z = _sigmoid(r_pre), _sigmoid(z_pre)
        n_pre = gi[:, 2 * D:] + r * gh[:, 2 * D:]
        pre = {"r": r_pre, "z": z_pre, "n": n_pre}
        new = (1.0 - z) * np.tanh(n_pre) + z * h
    else:
        raise ValueError("cell %r" % (cell,))
    mem[rows] = new
    lu[rows] = np.asarray(msg_ts, np.float32)[rows]
    return {"memory": mem, "last_update": lu, "flags": fl, "rows": rows, "pre": pre}


def saturated_limit(cell, pre, h):
    """The value h' tends to on rows whose gates are saturated: the GRU's h where z -> 1 and sign(n) where z -> 0,
    the RNN's sign(n).  pre: cell_update's pre-activations, h float64[R, D] the old rows."""
    n = np.sign(pre["n"])
    return n if cell == CELL_RNN else np.where(pre["z"] > 0, h, n)


def run_batches(cell, memory, last_update, efeat, time_w, batches, w_ih, w_hh, b_ih, b_hh):
    """batches: [(src, dst, ts, eidx), ..].  Per batch: the batch's messages are stored, then the cell runs on the
    flagged subset of the batch's endpoints [src | dst] -- so every batch after the first builds its messages from rows
    the update before it wrote.  The memory and the messages stay float64 across the batches; last_update and the
    timestamps are the float32 values the reference keeps.
    Returns a list with one dict per batch, the state after its update: memory, last_update, messages, timestamps,
    flags, and rows (the rows that update wrote)."""
    mem = _f64(memory)
    lu = np.asarray(last_update, np.float32).copy()
    N, D = mem.shape
    msg_dim = 2 * D + np.asarray(efeat).shape[1] + len(np.asarray(time_w).reshape(-1))
    messages = np.zeros((N, msg_dim), np.float64)
    timestamps = np.zeros(N, np.float32)
    flags = np.zeros(N, np.uint8)
    out = []
    for src, dst, ts, eidx in batches:
        s = store_messages(mem, lu, efeat, time_w, src, dst, ts, eidx)
        messages, timestamps, flags = messages.copy(), timestamps.copy(), flags.copy()
        messages[s["nodes"]] = s["rows"]
        timestamps[s["nodes"]] = s["ts"]
        flags[s["nodes"]] = 1
        ids = np.concatenate([np.asarray(src), np.asarray(dst)])
        u = cell_update(cell, mem, lu, messages, timestamps, flags, ids, len(ids), w_ih, w_hh, b_ih, b_hh)
        mem, lu, flags = u["memory"], u["last_update"], u["flags"]
        out.append({"memory": mem, "last_update": lu, "messages": messages, "timestamps": timestamps, "flags": flags,
                    "rows": u["rows"]})
    return out
