"""Plain float64 restatement of the fused neighbour aggregation, eval and training halves.

TEST INFRASTRUCTURE ONLY (like everything under oracle/): imported by tests/, never by zebra_amd/, and it imports
nothing from zebra_amd/.  Both entry points take the float32 inputs the kernels get and compute in float64 from them,
with the one exception the reference model itself defines: the cosine's argument is the FLOAT32 product
f32(dt) * f32(w) (model/time_encoding.py:18-28 multiplies float32 tensors), converted to float64 before cos.  With dt up
to 3e8 a float64 product would be a different function.

embed_f64       numpy; modules/embedding_module.py:243-276,320-328 in eval mode -- what oracle/torch_cpu.py's
                TorchCpuP23.embed writes in float32 (tests/test_aggregate_f64_cpu.py pins one to the other)
aggregate_f64   torch float64 under autograd; the training half (_NeighbourAggregate: overlay rows, a keep-mask after
                the ReLU), H / S / pre-activations and d_overlay / dW1 / db1 for a given cotangent, and -- for a
                threshold tau -- the bound on what ReLU units within tau of zero can add to each gradient element
"""
import numpy as np
import torch


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).astype(np.float64)


def time_encode_f64(dt, time_w):
    """cos of the float32 product, in float64: [..., T]."""
    dt = np.asarray(dt, np.float32)
    tw = np.asarray(time_w, np.float32).reshape(-1)
    return np.cos((dt[..., None] * tw).astype(np.float32).astype(np.float64))


def _normalised(ow):
    """wn = w / sum(w) (0 where the sum is 0) and S = [sum(w) != 0], from float32 weights [..., k]."""
    wt = _f64(ow)
    s = wt.sum(axis=-1, keepdims=True)
    nz = s != 0
    return np.where(nz, wt / np.where(nz, s, 1.0), 0.0), nz[..., 0].astype(np.float64)


def embed_f64(w, memory, efeat, time_w, nodes, on, oe, od, ow):
    """w: dict of torch-layout float32 arrays (fc1_w [D, D+F+T], fc1_b, fc2_*, fc1s_*, fc2s_*); memory [nodes, D];
    efeat [edges, F]; nodes int[N]; on / oe / od / ow: [M, N, k].
    Returns out [N, D (M + 1)] = [source transform | model 0 | ...], H [M, N, D], S [M, N]."""
    W = {kk: _f64(v) for kk, v in w.items() if kk.startswith("fc")}
    mem, ef = _f64(memory), _f64(efeat)
    nodes = np.asarray(nodes).astype(np.int64)
    src = np.maximum(mem[nodes] @ W["fc1s_w"].T + W["fc1s_b"], 0.0) @ W["fc2s_w"].T + W["fc2s_b"]       # :243-246
    outs, Hs, Ss = [src], [], []
    for m in range(len(on)):
        x = np.concatenate([mem[np.asarray(on[m]).astype(np.int64)], ef[np.asarray(oe[m]).astype(np.int64)],
                            time_encode_f64(od[m], time_w)], axis=2)                                     # :264
        h = np.maximum(x @ W["fc1_w"].T + W["fc1_b"], 0.0)                                               # :320-321
        wn, S = _normalised(ow[m])                                                                       # :268-272
        H = (h * wn[..., None]).sum(axis=1)
        outs.append(H @ W["fc2_w"].T + W["fc2_b"] * S[:, None])       # fc2 is linear: sum_k wn (fc2 h) = fc2 H + b2 S
        Hs.append(H)
        Ss.append(S)
    return np.concatenate(outs, axis=1), np.stack(Hs), np.stack(Ss)


def aggregate_f64(fc1_w, fc1_b, memory, efeat, time_w, on, oe, od, ow, cotangent, overlay=None, row_map=None, mask=None,
                  tau=None):
    """fc1_w [D, D+F+T], fc1_b [D]; memory [nodes, D]; overlay [U, D] with row_map int[nodes] (-1: the memory row),
    or neither; on / oe / od / ow [M, N, k]; mask: keep-mask [M, N, k, D] multiplied in after the ReLU, or None;
    cotangent [M, N, D] (dL/dH).  All float32 (numpy or CPU tensors), computed in float64.

    Returns a dict: H [M, N, D], S [M, N], z [M, N, k, D] (pre-activations), d_overlay [U, D] (None without an overlay),
    dW1, db1.  With tau also n_live / n_undecided -- a unit (m, n, kk, j) is live where its mask and its normalised
    weight are non-zero, undecided where it is live and |z| <= tau -- and allow_overlay / allow_W1 / allow_b1: per
    gradient element, the sum of |term| the undecided units would contribute to it with their ReLU open, i.e. the
    most that element can move when every undecided unit falls on the other side -- and "undecided": per such unit its
    fc1 row j, its overlay row (slot, -1: none) and its signed term in db1 [u], dW1's row j [u, K] and d_overlay's
    row slot [u, D], the change of that gradient when this one unit falls on the other side."""
    t64 = lambda a: torch.from_numpy(_f64(a.detach().cpu().numpy() if torch.is_tensor(a) else a))
    idx = lambda a: torch.from_numpy(np.asarray(a.cpu() if torch.is_tensor(a) else a).astype(np.int64))
    W1, b1 = t64(fc1_w).requires_grad_(True), t64(fc1_b).requires_grad_(True)
    mem, ef = t64(memory), t64(efeat)
    on_l, oe_l = idx(on), idx(oe)
    D = mem.shape[1]
    if overlay is not None:
        ov = t64(overlay).requires_grad_(True)
        slot = idx(row_map)[on_l]                                                        # [M, N, k]
        rows = torch.where((slot >= 0).unsqueeze(-1), ov[slot.clamp(min=0)], mem[on_l])
    else:
        ov, slot, rows = None, None, mem[on_l]
    od_np = np.asarray(od.cpu() if torch.is_tensor(od) else od, np.float32)
    ow_np = np.asarray(ow.cpu() if torch.is_tensor(ow) else ow, np.float32)
    x = torch.cat([rows, ef[oe_l], torch.from_numpy(time_encode_f64(od_np, time_w))], dim=-1)            # [M, N, k, K]
    z = torch.nn.functional.linear(x, W1, b1)
    h = torch.relu(z)
    mk = t64(mask) if mask is not None else None
    if mk is not None:
        h = h * mk
    wn_np, S = _normalised(ow_np)
    wn = torch.from_numpy(wn_np)
    H = (h * wn.unsqueeze(-1)).sum(dim=2)
    G = t64(cotangent)
    (H * G).sum().backward()
    res = {"H": H.detach().numpy(), "S": S, "z": z.detach().numpy(), "dW1": W1.grad.numpy(), "db1": b1.grad.numpy(),
           "d_overlay": ov.grad.numpy() if ov is not None else None}
    if tau is None:
        return res
    zd, xd, W1d = res["z"], x.detach().numpy(), W1.detach().numpy()
    live = np.broadcast_to(wn_np[..., None] > 0, zd.shape)
    if mk is not None:
        live = live & (mk.numpy() != 0)
    und = live & (np.abs(zd) <= tau)
    res["n_live"], res["n_undecided"] = int(live.sum()), int(und.sum())
    # the undecided units one by one: term = the signed change of the gradients when the unit falls on the other side
    # (open in float64, z > 0: its term leaves; closed: its term comes in)
    um, un, uk, uj = np.nonzero(und)
    Gd = G.numpy()
    dz =Gd[um, un, uj] * wn_np[um, un, uk] * (mk.numpy()[um, un, uk, uj] if mk is not None else 1.0)
    dz = np.where(zd[um, un, uk, uj] > 0, -dz, dz)
    uslot = slot.numpy()[um, un, uk] if ov is not None else np.full(len(um), -1, np.int64)
    res["undecided"] = {"j": uj, "slot": uslot, "db1": dz, "dW1": dz[:, None] * xd[um, un, uk],
                        "d_overlay": dz[:, None] * W1d[uj, :D]}
    aW, ab = np.zeros_like(res["dW1"]), np.zeros_like(res["db1"])
    ao = np.zeros_like(res["d_overlay"]) if ov is not None else None
    np.add.at(ab, uj, np.abs(dz))
    np.add.at(aW, uj, np.abs(res["undecided"]["dW1"]))
    if ov is not None:
        np.add.at(ao, uslot[uslot >= 0], np.abs(res["undecided"]["d_overlay"][uslot >= 0]))
    res["allow_W1"], res["allow_b1"], res["allow_overlay"] = aW, ab, ao
    return res
