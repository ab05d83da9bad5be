"""The quicksort replay without its rank pass in LDS (csrc/numba_sort.hpp, topk_ties_reg: final position = rank + entries
of the same rank to the left; tests/test_replay_identity_cpu.py restates it) on lists shaped like a hub hop's candidates:
n = 21 .. 41 entries for k = 20, two ascending runs (the hub's row, the partner's unmatched entries) and a new key, one to
five tie groups of two to five members that reach the kept ranks, every third list with a group that straddles the cut.
Both forms of the replay are driven through the test hook -- sel[] (modes 0 and 4) and the per-lane slot of ties_order
(modes 5 and 6: candidates in adjacent lanes / split over the wave's halves as the merge lays them out) -- and compared
with the oracle's restatement of numba's argsort.  (The hub chains' own form, ties_order_at, answers by list position from
the same replay; the streaming goldens and the soaks run it.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 20
CASES = 240


def hub_list(rng, n, k, straddle):
    """(values in list order, tie groups that reach the kept ranks, does one straddle the cut)"""
    drop = n - k
    w = np.sort(rng.random_sample(n))
    taken = np.zeros(n, bool)
    groups, straddles = 0, False
    for gi in range(int(rng.randint(1, 6))):
        s = int(rng.randint(2, 6))
        for attempt in range(6):
            if gi == 0 and straddle:
                a = int(rng.randint(max(0, drop - s + 1), drop))      # starts below the cut, ends at or above it
            else:
                a = int(rng.randint(max(0, drop - s + 1), n - s + 1)) # ends at or above the cut
            if not taken[max(0, a - 1):a + s + 1].any():              # keep the groups apart: sizes stay 2 .. 5
                break
        else:
            continue
        taken[a:a + s] = True
        w[a:a + s] = w[a]
        groups += 1
        straddles = straddles or a < drop
    perm = rng.permutation(n)
    n1 = int(rng.randint(1, min(k, n - 1) + 1))                       # the hub's row holds at most k entries
    n1 = max(n1, n - 1 - k)                                           # ... and so does the partner's
    vals = np.concatenate([np.sort(w[perm[:n1]]), np.sort(w[perm[n1:n - 1]]), w[perm[n - 1:]]])
    return vals, groups, straddles


@pytest.mark.parametrize("n", list(range(21, 42)))
def test_hub_shaped_lists(oracle, n):
    import torch
    from zebra_amd import _capi
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    rng = np.random.RandomState(4100 + n)
    vals = np.empty((CASES, n), np.float64)
    n_groups = np.zeros(CASES, int)
    n_straddle = 0
    for c in range(CASES):
        vals[c], n_groups[c], st = hub_list(rng, n, K, c % 3 == 0)
        n_straddle += int(st)
    assert n_groups.min() >= 1 and n_groups.max() >= 3 and n_straddle >= CASES // 3
    want = np.stack([oracle.numba_argsort(v)[-K:] for v in vals])
    dv = torch.from_numpy(vals).cuda()
    for mode in (0, 4, 5, 6):
        sel = torch.full((CASES, K), -1, dtype=torch.int32, device="cuda")
        path = torch.full((CASES,), -1, dtype=torch.int32, device="cuda")
        _capi.check(_capi.hooks_lib().zt_test_topk(_capi.ptr(dv), C.c_int32(n), C.c_int32(K), C.c_int32(CASES),
                                                   C.c_int32(mode), _capi.ptr(sel), _capi.ptr(path), _capi.stream_ptr()))
        got = sel.cpu().numpy()
        bad = np.where((got != want).any(axis=1))[0]
        assert len(bad) == 0, "mode %d: %d/%d lists differ, first %d: %s -> %s, want %s" % (
            mode, len(bad), CASES, bad[0], vals[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
        assert ((path.cpu().numpy() & 0xff) == 4).all()               # every list needs the replay
