"""The quicksort replay places entries without a rank pass inside the finished segments (csrc/numba_sort.hpp,
topk_ties_reg).  After the partitions every position left of a segment holds a rank <= every rank inside it and every
position right of it a rank >=, whether the segment was finished (fewer than 16 entries) or left alone because it lies
below the cut.  numba's insertion sort with strict < is stable inside a segment, so the entry at current position p
with rank r (r = number of strictly smaller entries) ends at

    f = r + (number of entries of rank r at current positions < p)

This file restates the replay that way in Python -- partitions as oracle/numba_semantics.py runs them, only on
segments of 16 or more entries that reach the kept ranks, then the identity, with the tie groups read top-down from
the ranks nobody claimed exactly as the kernel does -- and holds it against numba_argsort on seeded lists."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from numba_semantics import SMALL_QUICKSORT, numba_argsort  # noqa: E402


def _partition(key, r, low, high):
    """numba's partition of r[low..high] on key (no NaN: lt(a, b) is a < b).  Returns the pivot's place."""
    mid = (low + high) >> 1
    if key[r[mid]] < key[r[low]]:
        r[low], r[mid] = r[mid], r[low]
    if key[r[high]] < key[r[mid]]:
        r[high], r[mid] = r[mid], r[high]
    if key[r[mid]] < key[r[low]]:
        r[low], r[mid] = r[mid], r[low]
    pivot = key[r[mid]]
    r[high], r[mid] = r[mid], r[high]
    i, j = low, high - 1
    while True:
        while i < high and key[r[i]] < pivot:
            i += 1
        while j >= low and pivot < key[r[j]]:
            j -= 1
        if i >= j:
            break
        r[i], r[j] = r[j], r[i]
        i += 1
        j -= 1
    r[i], r[high] = r[high], r[i]
    return i


def replay_by_identity(values, k):
    """np.argsort(values)[-k:] under numba's quicksort, the way topk_ties_reg computes it."""
    v = [float(x) for x in values]
    n = len(v)
    drop = n - k
    lt = [sum(1 for y in v if y < x) for x in v]          # rank: equal values <=> equal ranks
    r = list(range(n))                                    # candidate at every position
    stack = [(0, n - 1)]
    while stack:
        low, high = stack.pop()
        # a segment wholly below the cut is neither partitioned nor ordered; one of fewer than 16 entries is finished
        while high >= drop and high - low >= SMALL_QUICKSORT:
            i = _partition(lt, r, low, high)
            stack.append((i + 1, high))
            high = i - 1
    key = [lt[c] for c in r]                              # rank at every current position
    f = list(key)                                         # an entry whose rank is unique already has f = r
    claimed = 0
    for x in key:
        claimed |= 1 << x
    unclaimed = ~claimed & ((1 << n) - 1)
    groups = 0
    while unclaimed >> drop:                              # tie groups that reach the kept ranks, from the top
        t = unclaimed.bit_length() - 1                    # last rank of the group
        g = (claimed & ((1 << t) - 1)).bit_length() - 1   # its members' rank: the highest claimed one below
        before = 0
        for p in range(n):
            if key[p] == g:
                f[p] = g + before
                before += 1
        assert g + before - 1 == t
        unclaimed &= (1 << g) - 1
        groups += 1
    # every entry of a group that was not visited lies wholly below the cut
    for p in range(n):
        direct = key[p] + sum(1 for q in range(p) if key[q] == key[p])
        assert (f[p] >= drop) == (direct >= drop) and (f[p] < drop or f[p] == direct)
    sel = [-1] * k
    for p in range(n):
        if f[p] >= drop:
            assert sel[f[p] - drop] == -1
            sel[f[p] - drop] = r[p]
    return np.asarray(sel, dtype=np.int64), groups


def _two_runs(rng, n, levels):
    """Two ascending runs and a new key behind them: the candidate list of a hub hop (the hub's row in dictionary order,
    the partner's unmatched entries, the new key).  `levels` distinct weights: few levels, many ties."""
    n1 = int(rng.randint(1, n - 1))
    w = 0.5 ** rng.randint(1, levels + 1, n).astype(np.float64)
    return np.concatenate([np.sort(w[:n1]), np.sort(w[n1:n - 1]), w[n - 1:]])


def _straddling(rng, n, k):
    """Distinct weights but for one group that straddles the cut n - k (and perhaps another one above it)."""
    w = np.sort(rng.random_sample(n))
    drop = n - k
    a = int(rng.randint(max(0, drop - 4), drop))
    b = int(rng.randint(drop, min(n - 1, drop + 4) + 1))
    w[a:b + 1] = w[a]
    if b + 3 < n and rng.randint(2):
        w[b + 1:b + 3] = w[b + 1]
    n1 = int(rng.randint(1, n - 1))
    perm = rng.permutation(n)
    return np.concatenate([np.sort(w[perm[:n1]]), np.sort(w[perm[n1:n - 1]]), w[perm[n - 1:]]])


def _lists(k, seed, count):
    rng = np.random.RandomState(seed)
    for c in range(count):
        kind = c % 6
        n = int(rng.randint(k + 1, min(2 * k + 2, 64) + 1))
        if kind == 0:
            yield _two_runs(rng, n, 3)                    # many ties
        elif kind == 1:
            yield _two_runs(rng, n, 12)                   # few ties
        elif kind == 2:
            yield _straddling(rng, n, k)
        elif kind == 3:
            yield rng.randint(0, max(2, n // 3), n) * 0.125           # arbitrary order
        elif kind == 4:
            yield 0.5 ** rng.randint(1, 6, n).astype(np.float64)      # arbitrary order, powers of beta = 0.5
        else:
            yield np.full(n, 1.0)                         # one group


@pytest.mark.parametrize("k", [5, 10, 20, 31])
def test_identity_places_like_numba(k):
    seen_groups = 0
    for vals in _lists(k, 7000 + k, 1500):
        got, groups = replay_by_identity(vals, k)
        want = numba_argsort(vals)[-k:]
        assert np.array_equal(got, want), (vals.tolist(), got.tolist(), want.tolist())
        seen_groups += groups
    assert seen_groups > 1500                             # the lists do carry ties into the kept ranks


@pytest.mark.parametrize("n,k", [(6, 5), (11, 5), (15, 10), (15, 14), (12, 3), (2, 1)])
def test_identity_on_lists_shorter_than_16(n, k):
    """No partition at all: the identity is the stable rank of the whole list."""
    rng = np.random.RandomState(n * 31 + k)
    for c in range(400):
        vals = rng.randint(0, 1 + c % 5, n) * 0.25
        got, _ = replay_by_identity(vals, k)
        assert np.array_equal(got, numba_argsort(vals)[-k:]), vals.tolist()


def test_group_straddling_the_cut():
    """A group that starts below the cut: its upper members are kept, in the order the partitions left them."""
    rng = np.random.RandomState(99)
    n_straddle = 0
    for c in range(1500):
        k = (5, 10, 20, 31)[c % 4]
        n = int(rng.randint(max(k + 1, 16), min(max(2 * k + 2, 24), 64) + 1))
        vals = _straddling(rng, n, k)
        srt = np.sort(vals)
        n_straddle += int(srt[n - k - 1] == srt[n - k])
        got, _ = replay_by_identity(vals, k)
        assert np.array_equal(got, numba_argsort(vals)[-k:]), vals.tolist()
    assert n_straddle == 1500
