// What the two forms of the pruning query (tppr_prune.hip: k_pruned_topk in LDS, k_pruned_topk_ws over a slab of device
// memory) have in common: the per-query list and its layout, the level-by-level walk of the adjacency, the left-to-right sum
// of duplicate states and the row writers.  Each is written over a "group" -- the threads that answer one query together:
// a wavefront (WaveGroup) or a workgroup (BlockGroup).  A group gives its SIZE, the caller's rank(), a barrier sync() and an
// exclusive scan with total, scan_excl(); nothing here asks a group which of the two it is.  The merge and the selection are
// different algorithms in the two forms and stay with their kernels.
//
// Needs u64, WAVE, lane_id() and wave_sync() (common.hpp) in scope and nothing else of the library, so that
// tools/exp/prune_ws_emu.cpp can include it as host code over its own stand-ins; includes nothing and opens no namespace:
// tppr_prune.hip includes it inside its unnamed namespace.  Everything is __forceinline__: the kernels must keep seeing which
// address space (LDS / global) the list's plain pointers point into.
#pragma once

constexpr int PR_MAX_MODELS = 4;      // (alpha, beta) models sharing one walk; more run as several launches
constexpr int WS_THREADS = 256;       // the workspace form's workgroup
constexpr int WS_WAVES = WS_THREADS / WAVE;

struct PruneModels {
    int M;
    double alpha[PR_MAX_MODELS], beta[PR_MAX_MODELS];
};

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// The list of one query: the candidate states in BFS (= dictionary insertion) order and the frontier's per-entry scratch.
// LDS form: one per wave, followed by sel / stk / SortLds; workspace form: one per slab, followed by the hash table.
struct PruneList {
    u64 *key;               // [cap_c] (edge << 32) | node
    double *ts;             // [cap_c]
    double *w;              // [M][cap_c] weight of every occurrence, per model (model stride wst)
    int *perm;              // [cap_c] owner frontier entry of a new state (walk) / first occurrence (merge) / sort scratch
    int *f_cnt;             // [cap_f] per frontier entry: number of states it emits
    int *f_off;             // [cap_f] exclusive scan of f_cnt
    int *f_ngh;             // [cap_f] find_before count
    long long *f_lo;        // [cap_f] start of the entry's adjacency
    double *f_base;         // [M][cap_f] weight of the entry's most recent neighbour (model stride bst)
    size_t wst, bst;        // model strides, in doubles
};

__host__ __device__ inline size_t prune_list_bytes(int cap_c, int cap_f, int M)
{
    return (2 + (size_t)M) * align16((size_t)cap_c * 8) + align16((size_t)cap_c * 4) + 3 * align16((size_t)cap_f * 4) +
           (1 + (size_t)M) * align16((size_t)cap_f * 8);
}

// the list at `base` (16-byte aligned); what a form appends starts at base + prune_list_bytes(cap_c, cap_f, M)
__device__ __forceinline__ PruneList carve_list(char *base, int cap_c, int cap_f, int M)
{
    PruneList L;
    L.wst = align16((size_t)cap_c * 8) / 8;
    L.bst = align16((size_t)cap_f * 8) / 8;
    char *p = base;
    L.key = reinterpret_cast<u64 *>(p); p += L.wst * 8;
    L.ts = reinterpret_cast<double *>(p); p += L.wst * 8;
    L.w = reinterpret_cast<double *>(p); p += (size_t)M * L.wst * 8;
    L.perm = reinterpret_cast<int *>(p); p += align16((size_t)cap_c * 4);
    L.f_cnt = reinterpret_cast<int *>(p); p += align16((size_t)cap_f * 4);
    L.f_off = reinterpret_cast<int *>(p); p += align16((size_t)cap_f * 4);
    L.f_ngh = reinterpret_cast<int *>(p); p += align16((size_t)cap_f * 4);
    L.f_lo = reinterpret_cast<long long *>(p); p += L.bst * 8;
    L.f_base = reinterpret_cast<double *>(p);
    return L;
}

// the caller's output arrays, [M][nq][k] with model stride `stride`
struct PruneOut {
    int *nodes, *eidx;
    float *dt, *w;
    long long stride;
};

__device__ __forceinline__ int wave_scan_incl(int v)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

struct WaveGroup {
    static constexpr int SIZE = WAVE;
    __device__ __forceinline__ int rank() const { return lane_id(); }
    __device__ __forceinline__ void sync() const { wave_sync(); }
    __device__ __forceinline__ int scan_excl(int v, int *total) const
    {
        const int inc = wave_scan_incl(v);
        *total = __shfl(inc, WAVE - 1);
        return inc - v;
    }
};

struct BlockGroup {
    static constexpr int SIZE = WS_THREADS;
    int *wt;                // WS_WAVES ints of LDS
    __device__ __forceinline__ int rank() const { return threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // (thread order; two barriers)
    __device__ __forceinline__ int scan_excl(int v, int *total) const
    {
        const int wv = threadIdx.x / WAVE;
        const int inc = wave_scan_incl(v);
        if (lane_id() == WAVE - 1) wt[wv] = inc;
        __syncthreads();
        int base = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < WS_WAVES; ++q) { const int t = wt[q]; base += q < wv ? t : 0; tot += t; }
        __syncthreads();
        *total = tot;
        return base + inc - v;
    }
};

// numba pow(float64, int64) (numba/cpython/numbers.py:207-243)
__device__ __forceinline__ double numba_int_pow(double a, long long b)
{
    if (b > 0x10000) return pow(a, (double)b);
    double r = 1.0;
    long long e = b;
    while (e != 0) {
        if (e & 1) r *= a;
        e >>= 1;
        a *= a;
    }
    return r;
}

// The walk of NeighborFinder.get_pruned_topk (utils/util.py:185-236) for every (alpha, beta) model at once -- which states
// are reached depends on (node, time) only, so the adjacency is walked once and one weight per model is carried along.
// Fills L.key / ts / w with every occurrence in BFS order and returns their number (<= cap_c).  Uniform over the group.
//   find_before (np.searchsorted, :152-154): a P-ary search by P lanes of one wavefront per frontier entry (P = 64 for the
//     single entry of level 0, 8 when a level has many) -- log_P(degree) dependent round trips instead of log_2;
//   the <= width most recent neighbours of all entries of a level (:211-232): one lane per (entry, z) pair, so the tails
//     come in as one coalesced round of loads.
template <class G>
__device__ __forceinline__ int prune_walk(const G &grp, const long long *__restrict__ indptr, const int *__restrict__ nbr,
                                          const int *__restrict__ eid, const double *__restrict__ ats, int qn, double qt,
                                          int width, int depth, const PruneModels &pm, int cap_c, int cap_f, const PruneList &L)
{
    const int rank = grp.rank(), M = pm.M;
    // frontier of level `dep` = the states level dep-1 appended: candidates [fr_lo, fr_lo + nf); level 0: the query
    int n_cand = 0, fr_lo = 0, nf = 1;
    for (int dep = 0; dep < depth; ++dep) {
        // ---- find_before of every frontier entry: P lanes per entry ----
        const int P = nf == 1 ? 64 : (nf == 2 ? 32 : (nf <= 4 ? 16 : 8));
        const int epc = G::SIZE / P;                                // entries per pass
        const int g = rank / P, gl = lane_id() / P, j = rank % P;   // the entry; its bit field in the wave's ballot; the probe
        const u64 gmask = P == 64 ? ~0ull : ((1ull << P) - 1ull);
        for (int f0 = 0; f0 < nf; f0 += epc) {
            const int f = f0 + g;
            const bool act = f < nf;
            const int node = !act ? 0 : (dep == 0 ? qn : (int)(unsigned)(L.key[fr_lo + f] & 0xffffffffull));
            const double t = !act ? 0.0 : (dep == 0 ? qt : L.ts[fr_lo + f]);
            const long long lo0 = act ? indptr[node] : 0, hi0 = act ? indptr[node + 1] : 0;
            long long lo = lo0, hi = hi0;                           // the answer (first index with ts >= t) is in [lo, hi]
            while (__ballot(lo < hi) != 0ull) {
                const long long n = hi - lo;
                const bool open = lo < hi;
                const bool pred = open && ats[lo + (n * j) / P] < t;               // probes at lo + floor(n * j / P)
                const int c = __popcll((__ballot(pred) >> (gl * P)) & gmask);      // true for a prefix of the probes
                if (open) {
                    if (c == 0) hi = lo;
                    else {
                        const long long nlo = lo + (n * (c - 1)) / P + 1;
                        hi = c < P ? lo + (n * c) / P : hi;
                        lo = nlo;
                    }
                }
            }
            if (act && j == 0) {
                const long long n_ngh = lo - lo0;
                L.f_ngh[f] = (int)n_ngh;                            // < 2^31: entries of one node
                L.f_lo[f] = lo0;
                L.f_cnt[f] = (int)(n_ngh < width ? n_ngh : width);
            }
        }
        grp.sync();
        // ---- exclusive scan of f_cnt ----
        int n_new = 0;
        for (int f0 = 0; f0 < nf; f0 += G::SIZE) {
            const int f = f0 + rank;
            int tot;
            const int ex = grp.scan_excl(f < nf ? L.f_cnt[f] : 0, &tot);
            if (f < nf) L.f_off[f] = n_new + ex;
            n_new += tot;
        }
        if (n_new == 0) break;                                      // :234-235
        if (n_cand + n_new > cap_c || nf > cap_f) break;            // (cannot happen: the plan's caps are sums of width^d)
        grp.sync();
        // ---- per entry and model: weight of its most recent neighbour (:208-209); who owns which new state ----
        for (int f = rank; f < nf; f += G::SIZE) {
            const int c = L.f_cnt[f], o = n_cand + L.f_off[f];
            if (c > 0) {
                const long long n_ngh = L.f_ngh[f];
                for (int m = 0; m < M; ++m) {
                    const double alpha = pm.alpha[m], beta = pm.beta[m];
                    const double qw = dep == 0 ? 1.0 : L.w[m * L.wst + fr_lo + f];
                    const double norm = beta / (1.0 - beta) * (1.0 - numba_int_pow(beta, n_ngh));   // :208
                    L.f_base[m * L.bst + f] = (alpha != 0.0 && dep == 0) ? qw * (1.0 - alpha) * beta / norm * alpha
                                                                         : qw * (1.0 - alpha) * beta / norm;   // :209
                }
                for (int z = 0; z < c; ++z) L.perm[o + z] = f;
            }
        }
        grp.sync();
        // ---- the new states, most recent first (:211-232): one lane per (entry, z) ----
        for (int i = rank; i < n_new; i += G::SIZE) {
            const int f = L.perm[n_cand + i];
            const int z = i - L.f_off[f];
            const long long p = L.f_lo[f] + L.f_ngh[f] - (z + 1);
            L.key[n_cand + i] = ((u64)(unsigned)eid[p] << 32) | (u64)(unsigned)nbr[p];
            L.ts[n_cand + i] = ats[p];
            for (int m = 0; m < M; ++m) {
                const double beta = pm.beta[m];
                double weight = L.f_base[m * L.bst + f];
                for (int q = 0; q < z; ++q) weight = weight * beta;                 // weight *= beta after every state
                L.w[m * L.wst + n_cand + i] = weight;
            }
        }
        grp.sync();
        fr_lo = n_cand;
        nf = n_new;
        n_cand += n_new;
    }
    return n_cand;
}

// dict[state] += weight in occurrence order (:222-225), given perm[c] = first occurrence of c's state: a leader's value is
// the left-to-right sum of its occurrences.  ONE wavefront, all of its lanes, walks the list in index order, lane m adding for
// model m (a lane's accesses to one address execute in program order).
__device__ __forceinline__ void sum_duplicates(const PruneList &L, int n_cand, int M)
{
    const int lane = lane_id();
    for (int c0 = 0; c0 < n_cand; c0 += WAVE) {
        const int c = c0 + lane;
        const int pc = c < n_cand ? L.perm[c] : c;
        u64 dm = __ballot(pc != c);
        while (dm != 0ull) {
            const int sl = __ffsll((long long)dm) - 1;
            dm &= dm - 1ull;
            const int cc = c0 + sl;
            const int lead = __shfl(pc, sl);
            if (lane < M) L.w[lane * L.wst + lead] = L.w[lane * L.wst + lead] + L.w[lane * L.wst + cc];
        }
    }
}

// ---- row writers: row qi of every model / of model m ----
// A row nobody else writes: an id out of range, an empty dictionary (:241-242).  The reference leaves such a row untouched;
// zero_empty callers (pipeline.hip) do not clear their output arrays beforehand -- a memset in front of every query is a packet
// on the T-PPR stream, ~6 us of every C4 step -- and the aggregation of the step, whose caller may never look at the status
// word, would consume the previous group's neighbours: an empty row instead.
template <class G>
__device__ __forceinline__ void zero_row(const G &grp, const PruneOut &O, int M, long long qi, int k)
{
    for (int m = 0; m < M; ++m) {
        const long long ob = (long long)m * O.stride + qi * k;
        for (int j = grp.rank(); j < k; j += G::SIZE) { O.nodes[ob + j] = 0; O.eidx[ob + j] = 0; O.w[ob + j] = 0.f; O.dt[ob + j] = 0.f; }
    }
}

// nd <= k: the whole dictionary in insertion order, then padding
template <class G>
__device__ __forceinline__ void emit_all(const G &grp, const PruneOut &O, const PruneList &L, int m, long long qi, int k,
                                         int nd, double qt)
{
    const long long ob = (long long)m * O.stride + qi * k;
    const double *wm = L.w + m * L.wst;
    for (int j = grp.rank(); j < k; j += G::SIZE) {
        const bool a = j < nd;
        O.nodes[ob + j] = a ? (int)(unsigned)(L.key[j] & 0xffffffffull) : 0;
        O.eidx[ob + j] = a ? (int)(unsigned)(L.key[j] >> 32) : 0;
        O.w[ob + j] = a ? (float)wm[j] : 0.f;
        const float tsf = a ? (float)L.ts[j] : 0.f;
        O.dt[ob + j] = (float)(qt - (double)tsf);
    }
}

// the k list indices sel[0..k) in that order
template <class G>
__device__ __forceinline__ void emit_selected(const G &grp, const PruneOut &O, const PruneList &L, int m, long long qi, int k,
                                              const int *sel, double qt)
{
    const long long ob = (long long)m * O.stride + qi * k;
    const double *wm = L.w + m * L.wst;
    for (int j = grp.rank(); j < k; j += G::SIZE) {
        const int c = sel[j];
        O.nodes[ob + j] = (int)(unsigned)(L.key[c] & 0xffffffffull);
        O.eidx[ob + j] = (int)(unsigned)(L.key[c] >> 32);
        O.w[ob + j] = (float)wm[c];
        O.dt[ob + j] = (float)(qt - (double)(float)L.ts[c]);
    }
}
