// Static adjacency (CSR) + pruning T-PPR ("PPI", reference utils/util.py:90-276).
// Compile with -ffp-contract=off (bit-exact float64, see tppr_stream.hip).
//
// One query row = one walk of the adjacency for all (alpha, beta) models, a merge of duplicate states that keeps the
// reference's dictionary order (first occurrence) and its left-to-right float64 summation order, and a selection with the
// exact numba argsort semantics.  Two kernels answer it; prune_plan decides between them:
//   k_pruned_topk     the LDS form: one wavefront per query, the list in LDS;
//   k_pruned_topk_ws  the workspace form, for walks that do not fit LDS: one workgroup per slab of device memory the
//                     handle reserves.
// The list layout, the walk, the duplicate sum and the row writers are the same code for both (prune_walk.hpp, over a
// wavefront or a workgroup); each kernel has its own merge (all pairs / hash table) and selection (numba_sort.hpp's
// wave-parallel argsort / radix select), which are different algorithms for different sizes.
#include "csr_handle.hpp"
#include "numba_sort.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace zt;

namespace {

#include "prune_walk.hpp"     // (in here: its names are this file's own)

constexpr int PR_WAVES = 4;           // queries per workgroup
constexpr int MAX_CAND = 1280;        // sum_{d<=depth} width^d
constexpr int MAX_FRONT = 512;        // width^(depth-1)

// Per-wave LDS block, carved from dynamic shared memory: the list, then sel, stk and the sort's scratch; sized at launch
// from the actual (width, depth, models) so that small configurations keep occupancy high.
// (sel: 64 entries for k <= ZT_MAX_K -- the tuned configurations keep their LDS footprint --, 256 for the wider k)
__host__ __device__ inline size_t prune_sel_words(int k) { return k <= 64 ? 64 : 256; }
__host__ __device__ inline size_t prune_lds_bytes(int cap_c, int cap_f, int M, int k)
{
    return prune_list_bytes(cap_c, cap_f, M) + align16(prune_sel_words(k) * 4) + align16(96 * 4) + align16(sizeof(SortLds));
}

// The LDS form: ONE wavefront per query row.  The walk, then
//   duplicate states (dict[state] += w in occurrence order, :222-225): first occurrences by an all-pairs scan with
//     broadcast reads;
//   exact numba argsort selection (:240-276) per model.
__global__ __launch_bounds__(WAVE * PR_WAVES) void k_pruned_topk(
    const long long *__restrict__ indptr, const int *__restrict__ nbr, const int *__restrict__ eid,
    const double *__restrict__ ats, long long num_nodes, const int *__restrict__ q_nodes,
    const double *__restrict__ q_ts, long long nq, int width, int depth, PruneModels pm, int k,
    int *out_nodes, int *out_eidx, float *out_dt, float *out_w, long long out_stride, int *status, int cap_c, int cap_f,
    int dbg_stop, int zero_empty)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = pm.M;
    char *blk = smem + (threadIdx.x / WAVE) * prune_lds_bytes(cap_c, cap_f, M, k);
    const PruneList L = carve_list(blk, cap_c, cap_f, M);
    int *sel = reinterpret_cast<int *>(blk + prune_list_bytes(cap_c, cap_f, M));   // 64 (k <= ZT_MAX_K) or 256
    int *stk = sel + prune_sel_words(k);                                           // 96
    SortLds *sort = reinterpret_cast<SortLds *>(stk + 96);      // wave-parallel exact argsort scratch (n <= 128)
    const WaveGroup grp;
    const PruneOut O = {out_nodes, out_eidx, out_dt, out_w, out_stride};
    const size_t wst = L.wst;
    const int lane = lane_id();
    const long long qi = (long long)blockIdx.x * PR_WAVES + threadIdx.x / WAVE;
    if (qi >= nq) return;
    const int qn = q_nodes[qi];
    const double qt = q_ts[qi];
    if (qn < 0 || qn >= num_nodes) {
        if (lane == 0) atomicExch(status, ZT_ERR_RANGE);
        if (zero_empty) zero_row(grp, O, M, qi, k);
        return;
    }
    const int n_cand = prune_walk(grp, indptr, nbr, eid, ats, qn, qt, width, depth, pm, cap_c, cap_f, L);
    if (n_cand == 0) {                                              // :241-242, row untouched
        if (zero_empty) zero_row(grp, O, M, qi, k);
        return;
    }
    if (dbg_stop == 1) { if (lane == 0) out_nodes[qi * k] = n_cand; return; }      // (diagnostic: ZT_PRUNE_STOP)

    // ---- merge duplicate states: dict[state] += weight in occurrence order (:222-225) ----
    // perm[c] = first occurrence of c's state (= c for a leader); every lane walks the list front to back with
    // broadcast reads.  The frontier above needed the un-merged weights; from here on only leaders matter.
    bool any_dup = false;
    for (int c0 = 0; c0 < n_cand; c0 += WAVE) {
        const int c = c0 + lane;
        const bool in = c < n_cand;
        const u64 kc = in ? L.key[c] : 0ull;
        const double tc = in ? L.ts[c] : 0.0;
        int fi = c;
        const int qmax = c0 + WAVE - 1 < n_cand ? c0 + WAVE - 1 : n_cand - 1;      // nobody looks beyond its own index
        // first earlier entry with the same (edge, node): four broadcast reads in flight per step
        for (int q0 = 0; q0 < qmax; q0 += 4) {
            u64 kq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) kq[u] = L.key[q0 + u < n_cand ? q0 + u : n_cand - 1];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (in && q0 + u < c && fi == c && kq[u] == kc) fi = q0 + u;
        }
        // the dictionary key is (edge, node, time): equal (edge, node) with different times cannot come out of one
        // adjacency, but if it ever does, redo this chunk comparing the time on every hit
        if (__ballot(in && fi != c && L.ts[fi] != tc) != 0ull) {
            fi = c;
            for (int q = 0; q < qmax; ++q)
                if (in && q < c && fi == c && L.key[q] == kc && L.ts[q] == tc) fi = q;
        }
        if (in) L.perm[c] = fi;
        any_dup = any_dup || __ballot(in && fi != c) != 0ull;
    }
    wave_sync();
    int nd = n_cand;
    if (any_dup) {
        sum_duplicates(L, n_cand, M);
        wave_sync();
        // compact the leaders in order (dictionary insertion order)
        nd = 0;
        for (int c0 = 0; c0 < n_cand; c0 += WAVE) {
            const int c = c0 + lane;
            const bool lead = c < n_cand && L.perm[c] == c;
            const u64 kc = lead ? L.key[c] : 0;
            const double tc = lead ? L.ts[c] : 0.0;
            double wc[PR_MAX_MODELS];
#pragma unroll
            for (int m = 0; m < PR_MAX_MODELS; ++m) wc[m] = (lead && m < M) ? L.w[m * wst + c] : 0.0;
            const u64 bm = __ballot(lead);
            wave_sync();   // all reads of this chunk done before it may be overwritten
            if (lead) {
                const int pos = nd + __popcll(bm & lanemask_lt());   // pos <= c: never clobbers unread chunks
                L.key[pos] = kc; L.ts[pos] = tc;
#pragma unroll
                for (int m = 0; m < PR_MAX_MODELS; ++m) if (m < M) L.w[m * wst + pos] = wc[m];
            }
            nd += __popcll(bm);
            wave_sync();
        }
    }

    if (dbg_stop == 2) { if (lane == 0) out_nodes[qi * k] = nd; return; }
    // ---- select and emit (:240-276), model by model ----
    // (k <= ZT_MAX_K: one pass, lane j = entry j; wider k -- the reference puts no bound on --topk, train.py:46 -- strides)
    for (int m = 0; m < M; ++m) {
        if (nd <= k) { emit_all(grp, O, L, m, qi, k, nd, qt); continue; }
        const double *wm = L.w + m * wst;
        if (dbg_stop == 4 || (dbg_stop == 3 && nd > WAVE)) { if (lane < k) sel[lane] = lane; wave_sync(); }   // (diagnostic)
        else if (k <= ZT_MAX_K) topk_select_wave(wm, nd, k, sel, *sort, L.perm, stk);
        else topk_select_any(wm, nd, k, sel, *sort, L.perm, stk);            // kept sets wider than a wavefront: correct first
        emit_selected(grp, O, L, m, qi, k, sel, qt);
        wave_sync();
    }
}

// ---------------------------------------------------------------------------
// The workspace form: the same query with its list in a slab of device memory (zt_csr_reserve_pruning), for walks that do
// not fit LDS (the reference bounds neither --n_degree nor --n_layer).  Persistent: worker = one WORKGROUP of WS_THREADS
// threads, one slab each, queries worker, worker + grid, ...  A workgroup rather than a wavefront: a walk of 10^4..10^5
// states is latency-bound on global memory, and four waves keep four times the loads in flight per slab (slabs are megabytes
// each, so slabs, not lanes, are what a budget runs out of); the barrier between stages and a 256-bin LDS histogram for the
// selection come with it.  The walk, the duplicate sum and the row writers are prune_walk.hpp's, over the workgroup; what
// differs from k_pruned_topk is how the two quadratic steps are done:
//   merge   first occurrences through a hash table in the slab: a slot is claimed for a (edge, node) key by compare-and-swap
//           and keeps the SMALLEST list index of its key (atomicMin), which does not depend on who inserts first;
//   select  the cut (k-th largest value) by an 8-bit-per-pass radix select on the float64 patterns -- weights are positive
//           and finite, where pattern order is value order --, then ranks by counting among the k candidates at or above
//           it.  A tie group that reaches the kept ranks (or a NaN / negative pattern) takes the literal replay
//           numba_argsort_seq over all n, on one lane: n log n, correct first.
// A slab is reused from query to query: every array is written before it is read within a query (the hash table is
// cleared over the slots this query uses).
// ---------------------------------------------------------------------------
struct WsLds {                                // k_pruned_topk_ws's LDS: the selection's scratch
    double cval[256];                         // the candidates at or above the cut: value,
    int cidx[256];                            // list index
    int sel[256];                             // the kept set, in output order
    int hist[256];                            // radix select: one pass's bins
    int stk[96];                              // numba_argsort_seq's stack
    int wt[WS_WAVES];                         // BlockGroup::scan_excl
    int bin, want, cnt;
};
constexpr int WS_STATIC_LDS = (int)sizeof(WsLds);
constexpr u64 WS_EMPTY = ~0ull;              // no (edge, node) key: edge ids are < 2^31

__host__ __device__ inline size_t ws_table_slots(long long n)           // power of two, load factor <= 1/2
{
    size_t t = 64;
    while (t < 2 * (size_t)n) t <<= 1;
    return t;
}
// a slab: the list, then the merge's hash table -- h_key [slots]: the key that owns the slot, h_first [slots]: the smallest
// list index of that key
__host__ __device__ inline size_t ws_slab_bytes(int cap_c, int cap_f, int M)
{
    const size_t b = prune_list_bytes(cap_c, cap_f, M) + align16(ws_table_slots(cap_c) * 8) + align16(ws_table_slots(cap_c) * 4);
    return (b + 255) & ~(size_t)255;
}

__global__ __launch_bounds__(WS_THREADS) void k_pruned_topk_ws(
    const long long *__restrict__ indptr, const int *__restrict__ nbr, const int *__restrict__ eid,
    const double *__restrict__ ats, long long num_nodes, const int *__restrict__ q_nodes,
    const double *__restrict__ q_ts, long long nq, int width, int depth, PruneModels pm, int k,
    int *out_nodes, int *out_eidx, float *out_dt, float *out_w, long long out_stride, int *status, int cap_c, int cap_f,
    int slab_models, char *slabs, long long slab_bytes, int zero_empty)
{
    __shared__ WsLds S;
    const int M = pm.M;
    char *slab = slabs + (size_t)blockIdx.x * (size_t)slab_bytes;
    const PruneList L = carve_list(slab, cap_c, cap_f, slab_models);
    u64 *h_key = reinterpret_cast<u64 *>(slab + prune_list_bytes(cap_c, cap_f, slab_models));
    int *h_first = reinterpret_cast<int *>(h_key + ws_table_slots(cap_c));
    const BlockGroup grp = {S.wt};
    const PruneOut O = {out_nodes, out_eidx, out_dt, out_w, out_stride};
    const size_t wst = L.wst;
    const int tid = threadIdx.x;
    for (long long qi = blockIdx.x; qi < nq; qi += gridDim.x) {        // (every branch below is uniform over the workgroup)
        __syncthreads();                                               // the previous query's LDS and slab reads are done
        const int qn = q_nodes[qi];
        const double qt = q_ts[qi];
        if (qn < 0 || qn >= num_nodes) {
            if (tid == 0) atomicExch(status, ZT_ERR_RANGE);
            if (zero_empty) zero_row(grp, O, M, qi, k);
            continue;
        }
        const int n_cand = prune_walk(grp, indptr, nbr, eid, ats, qn, qt, width, depth, pm, cap_c, cap_f, L);
        if (n_cand == 0) {                                              // :241-242, row untouched
            if (zero_empty) zero_row(grp, O, M, qi, k);
            continue;
        }

        // ---- merge duplicate states: dict[state] += weight in occurrence order (:222-225) ----
        // perm[c] = first occurrence of c's state.  The table's words are written by atomics and read back past the L1.
        {
            const int tsz = (int)ws_table_slots(n_cand);
            const unsigned hmask = (unsigned)tsz - 1u;
            for (int s = tid; s < tsz; s += WS_THREADS) { st_agent(&h_key[s], WS_EMPTY); st_agent(&h_first[s], 0x7fffffff); }
            __syncthreads();
            for (int c = tid; c < n_cand; c += WS_THREADS) {
                const u64 kc = L.key[c];
                unsigned h = (unsigned)((kc * 0x9E3779B97F4A7C15ull) >> 40) & hmask;
                for (;;) {
                    const u64 prev = atomicCAS(&h_key[h], WS_EMPTY, kc);
                    if (prev == WS_EMPTY || prev == kc) break;
                    h = (h + 1u) & hmask;
                }
                atomicMin(&h_first[h], c);
                L.perm[c] = (int)h;
            }
            __syncthreads();
        }
        int dup = 0, mis = 0;
        for (int c = tid; c < n_cand; c += WS_THREADS) {
            const int fi = ld_agent(&h_first[L.perm[c]]);
            mis |= (fi != c && L.ts[fi] != L.ts[c]) ? 1 : 0;
            dup |= fi != c ? 1 : 0;
            L.perm[c] = fi;
        }
        mis = __syncthreads_or(mis);
        if (mis) {
            // the dictionary key is (edge, node, time): equal (edge, node) with different times cannot come out of one
            // adjacency, but if it ever does, redo the search comparing the time on every hit (the LDS form's fallback)
            dup = 0;
            for (int c = tid; c < n_cand; c += WS_THREADS) {
                const u64 kc = L.key[c];
                const double tc = L.ts[c];
                int fi = c;
                for (int q = 0; q < c; ++q)
                    if (L.key[q] == kc && L.ts[q] == tc) { fi = q; break; }
                L.perm[c] = fi;
                dup |= fi != c ? 1 : 0;
            }
        }
        const bool any_dup = __syncthreads_or(dup) != 0;
        int nd = n_cand;
        if (any_dup) {
            if (tid < WAVE) sum_duplicates(L, n_cand, M);
            __syncthreads();
            // compact the leaders in order (dictionary insertion order): a chunk's reads come before the scan's barriers, its
            // writes after them, and land at or below the chunk (pos <= c)
            nd = 0;
            for (int c0 = 0; c0 < n_cand; c0 += WS_THREADS) {
                const int c = c0 + tid;
                const bool lead = c < n_cand && L.perm[c] == c;
                const u64 kc = lead ? L.key[c] : 0;
                const double tc = lead ? L.ts[c] : 0.0;
                double wc[PR_MAX_MODELS];
#pragma unroll
                for (int m = 0; m < PR_MAX_MODELS; ++m) wc[m] = (lead && m < M) ? L.w[m * wst + c] : 0.0;
                int tot;
                const int ex = grp.scan_excl(lead ? 1 : 0, &tot);
                if (lead) {
                    const int pos = nd + ex;
                    L.key[pos] = kc; L.ts[pos] = tc;
#pragma unroll
                    for (int m = 0; m < PR_MAX_MODELS; ++m) if (m < M) L.w[m * wst + pos] = wc[m];
                }
                nd += tot;
            }
            __syncthreads();
        }

        // ---- select and emit (:240-276), model by model ----
        for (int m = 0; m < M; ++m) {
            if (nd <= k) { emit_all(grp, O, L, m, qi, k, nd, qt); continue; }
            const double *wm = L.w + m * wst;
            // np.argsort(values)[-k:] in numba's order (topk_select_any's contract, numba_sort.hpp)
            const int drop = nd - k;
            int odd = 0;                                                // a pattern whose order is not its value's: negative, NaN
            for (int c = tid; c < nd; c += WS_THREADS) {
                const double v = wm[c];
                odd |= ((u64)__double_as_longlong(v) >> 63) != 0ull || v != v ? 1 : 0;
            }
            bool slow = __syncthreads_or(odd) != 0;
            if (!slow) {
                // the cut: the k-th largest pattern, eight bits per pass
                u64 prefix = 0ull, pmask = 0ull;
                int want = k, eq_cut = 0;
                for (int shift = 56; shift >= 0; shift -= 8) {
                    S.hist[tid] = 0;
                    __syncthreads();
                    for (int c = tid; c < nd; c += WS_THREADS) {
                        const u64 b = (u64)__double_as_longlong(wm[c]);
                        if ((b & pmask) == prefix) atomicAdd(&S.hist[(int)((b >> shift) & 255ull)], 1);
                    }
                    __syncthreads();
                    if (tid == 0) {
                        int acc = 0, b = 255;
                        for (; b > 0; --b) {
                            if (acc + S.hist[b] >= want) break;
                            acc += S.hist[b];
                        }
                        S.bin = b; S.want = want - acc;
                    }
                    __syncthreads();
                    prefix |= (u64)S.bin << shift;
                    pmask |= 255ull << shift;
                    want = S.want;
                    eq_cut = S.hist[S.bin];
                    __syncthreads();
                }
                // `want` of the eq_cut values equal to the cut are kept: more than one of them is a tie group that reaches the
                // kept ranks
                slow = eq_cut > 1;
                if (!slow) {
                    if (tid == 0) S.cnt = 0;
                    __syncthreads();
                    for (int c = tid; c < nd; c += WS_THREADS) {
                        const double v = wm[c];
                        if ((u64)__double_as_longlong(v) >= prefix) {   // exactly k of them
                            const int pos = atomicAdd(&S.cnt, 1);
                            if (pos < 256) { S.cidx[pos] = c; S.cval[pos] = v; }
                        }
                    }
                    __syncthreads();
                    int tie = 0;
                    if (tid < k) {
                        const double v = S.cval[tid];
                        int lt = 0, eq = 0;
                        for (int q = 0; q < k; ++q) { const double x = S.cval[q]; lt += x < v ? 1 : 0; eq += x == v ? 1 : 0; }
                        tie = eq > 1 ? 1 : 0;
                        if (!tie) S.sel[lt] = S.cidx[tid];               // rank among all nd = drop + lt
                    }
                    slow = __syncthreads_or(tie) != 0;
                }
            }
            if (slow) {
                if (tid == 0) numba_argsort_seq(wm, nd, L.perm, S.stk);
                __syncthreads();
                for (int q = tid; q < k; q += WS_THREADS) S.sel[q] = L.perm[drop + q];
                __syncthreads();
            }
            emit_selected(grp, O, L, m, qi, k, S.sel, qt);
            __syncthreads();
        }
    }
}

}  // namespace

static int csr_upload(zt_csr *c)
{
    const int64_t n2 = c->E2;
    ZT_HIP(hipMalloc(&c->indptr, sizeof(long long) * (c->N + 1)));
    ZT_HIP(hipMalloc(&c->nbr, sizeof(int) * (n2 > 0 ? n2 : 1)));
    ZT_HIP(hipMalloc(&c->eid, sizeof(int) * (n2 > 0 ? n2 : 1)));
    ZT_HIP(hipMalloc(&c->ts, sizeof(double) * (n2 > 0 ? n2 : 1)));
    ZT_HIP(hipMemcpy(c->indptr, c->h_indptr.data(), sizeof(long long) * (c->N + 1), hipMemcpyHostToDevice));
    if (n2 > 0) {
        ZT_HIP(hipMemcpy(c->nbr, c->h_nbr.data(), sizeof(int) * n2, hipMemcpyHostToDevice));
        ZT_HIP(hipMemcpy(c->eid, c->h_eid.data(), sizeof(int) * n2, hipMemcpyHostToDevice));
        ZT_HIP(hipMemcpy(c->ts, c->h_ts.data(), sizeof(double) * n2, hipMemcpyHostToDevice));
    }
    return ZT_OK;
}

extern "C" int zt_csr_build(zt_csr **out, const int32_t *src, const int32_t *dst, const int64_t *eidx,
                            const double *ts, int64_t E, int64_t num_nodes)
{
    if (!out || E < 0 || num_nodes <= 0 || (E > 0 && (!src || !dst || !eidx || !ts))) {
        set_error("zt_csr_build: bad argument");
        return ZT_ERR_ARG;
    }
    for (int64_t i = 0; i < E; ++i) {
        if (src[i] < 0 || src[i] >= num_nodes || dst[i] < 0 || dst[i] >= num_nodes || eidx[i] < 0 ||
            eidx[i] > 0x7fffffffll) {
            set_error("zt_csr_build: id out of range at edge %lld", (long long)i);
            return ZT_ERR_RANGE;
        }
    }
    zt_csr *c = new zt_csr();
    c->N = num_nodes;
    c->E2 = 2 * E;
    c->h_indptr.assign(num_nodes + 1, 0);
    for (int64_t i = 0; i < E; ++i) { c->h_indptr[src[i] + 1]++; c->h_indptr[dst[i] + 1]++; }
    for (int64_t v = 0; v < num_nodes; ++v) c->h_indptr[v + 1] += c->h_indptr[v];
    // adjacency in stream order (both directions per edge, utils/util.py:94-96),
    // then a stable sort by timestamp per node (:103)
    std::vector<long long> cur(c->h_indptr.begin(), c->h_indptr.end() - 1);
    std::vector<int64_t> pos(2 * E);            // slot -> (edge index * 2 + direction)
    for (int64_t i = 0; i < E; ++i) { pos[cur[src[i]]++] = 2 * i; pos[cur[dst[i]]++] = 2 * i + 1; }
    for (int64_t v = 0; v < num_nodes; ++v)
        std::stable_sort(pos.begin() + c->h_indptr[v], pos.begin() + c->h_indptr[v + 1],
                         [&](int64_t a, int64_t b) { return ts[a >> 1] < ts[b >> 1]; });
    c->h_nbr.resize(2 * E); c->h_eid.resize(2 * E); c->h_ts.resize(2 * E);
    for (int64_t p = 0; p < 2 * E; ++p) {
        const int64_t i = pos[p] >> 1;
        c->h_nbr[p] = (pos[p] & 1) ? src[i] : dst[i];
        c->h_eid[p] = (int)eidx[i];
        c->h_ts[p] = ts[i];
    }
    {
        int rc = csr_upload(c);
        if (rc != ZT_OK) { delete c; return rc; }
    }
    *out = c;
    return ZT_OK;
}

extern "C" int zt_csr_from_sorted(zt_csr **out, const int64_t *indptr, const int32_t *nbr, const int32_t *eid,
                                  const double *ts, int64_t num_nodes)
{
    if (!out || !indptr || num_nodes <= 0) { set_error("zt_csr_from_sorted: bad argument"); return ZT_ERR_ARG; }
    const int64_t n2 = indptr[num_nodes];
    if (indptr[0] != 0 || n2 < 0) { set_error("zt_csr_from_sorted: bad indptr"); return ZT_ERR_ARG; }
    for (int64_t v = 0; v < num_nodes; ++v)
        if (indptr[v + 1] < indptr[v]) { set_error("zt_csr_from_sorted: indptr not monotone"); return ZT_ERR_ARG; }
    for (int64_t p = 0; p < n2; ++p)
        if (nbr[p] < 0 || nbr[p] >= num_nodes || eid[p] < 0) {
            set_error("zt_csr_from_sorted: id out of range at entry %lld", (long long)p);
            return ZT_ERR_RANGE;
        }
    zt_csr *c = new zt_csr();
    c->N = num_nodes;
    c->E2 = n2;
    c->h_indptr.assign(indptr, indptr + num_nodes + 1);
    c->h_nbr.assign(nbr, nbr + n2);
    c->h_eid.assign(eid, eid + n2);
    c->h_ts.assign(ts, ts + n2);
    int rc = csr_upload(c);
    if (rc != ZT_OK) { delete c; return rc; }
    *out = c;
    return ZT_OK;
}

extern "C" int zt_csr_size(const zt_csr *c, int64_t *num_nodes, int64_t *num_entries)
{
    if (!c) return ZT_ERR_ARG;
    if (num_nodes) *num_nodes = c->N;
    if (num_entries) *num_entries = c->E2;
    return ZT_OK;
}

extern "C" int zt_csr_export(const zt_csr *c, int64_t *indptr, int32_t *nbr, int32_t *eid, double *ts)
{
    if (!c) return ZT_ERR_ARG;
    if (indptr) for (int64_t v = 0; v <= c->N; ++v) indptr[v] = c->h_indptr[v];
    if (nbr) memcpy(nbr, c->h_nbr.data(), sizeof(int) * c->E2);
    if (eid) memcpy(eid, c->h_eid.data(), sizeof(int) * c->E2);
    if (ts) memcpy(ts, c->h_ts.data(), sizeof(double) * c->E2);
    return ZT_OK;
}

extern "C" int zt_csr_destroy(zt_csr *c)
{
    if (!c) return ZT_OK;
    (void)zt_csr_release_pruning(c);
    (void)hipFree(c->indptr); (void)hipFree(c->nbr); (void)hipFree(c->eid); (void)hipFree(c->ts);
    delete c;
    return ZT_OK;
}

extern "C" int zt_csr_find_before(const zt_csr *c, int32_t v, double t, int64_t *count, int32_t *nbr_host,
                                  int32_t *eid_host, double *ts_host, int64_t cap)
{
    if (!c || !count) return ZT_ERR_ARG;
    if (v < 0 || v >= c->N) { set_error("zt_csr_find_before: node id out of range"); return ZT_ERR_RANGE; }
    const long long lo = c->h_indptr[v], hi = c->h_indptr[v + 1];
    const long long n = std::lower_bound(c->h_ts.begin() + lo, c->h_ts.begin() + hi, t) - (c->h_ts.begin() + lo);
    *count = n;
    const long long m = n < cap ? n : cap;
    if (nbr_host) memcpy(nbr_host, c->h_nbr.data() + lo, sizeof(int) * m);
    if (eid_host) memcpy(eid_host, c->h_eid.data() + lo, sizeof(int) * m);
    if (ts_host) memcpy(ts_host, c->h_ts.data() + lo, sizeof(double) * m);
    return ZT_OK;
}

// Which form a pruning query of this shape takes and what it needs: the ONE place that decides (pruned_launch, the
// reservation and zt_prune_plan all come here).  Host code, no GPU call.
struct PrunePlan {
    int form;                    // ZT_PRUNE_FORM_*
    long long cap_c, cap_f;      // states a query may emit (sum width^d), widest frontier (width^(depth-1))
    int models;                  // per launch
    long long slab_bytes, slabs;
    int grid, threads;
    long long lds;
};

static PrunePlan prune_plan(int width, int depth, int n_models, int k, long long max_bytes)
{
    PrunePlan p = {};
    long long cap = 0, lvl = 1, front = 1;
    for (int d = 0; d < depth; ++d) {
        front = lvl; lvl *= width; cap += lvl;
        if (cap > ZT_PRUNE_WS_MAX_STATES) { cap = (long long)ZT_PRUNE_WS_MAX_STATES + 1; break; }
    }
    p.cap_c = cap; p.cap_f = front;
    if (k > ZT_MAX_K_WIDE || cap > ZT_PRUNE_WS_MAX_STATES) {
        set_error("zt_pruned_topk: k=%d width=%d depth=%d exceeds what the pruning query takes "
                  "(k<=%d, sum width^d<=%d)", k, width, depth, ZT_MAX_K_WIDE, (int)ZT_PRUNE_WS_MAX_STATES);
        p.form = ZT_PRUNE_FORM_REFUSED;
        return p;
    }
    if (cap <= MAX_CAND && front <= MAX_FRONT) {
        // as many models per launch as the workgroup's LDS allows (at least one)
        int mm = n_models < PR_MAX_MODELS ? n_models : PR_MAX_MODELS;
        while (mm > 1 && prune_lds_bytes((int)cap, (int)front, mm, k) * PR_WAVES > 64 * 1024) --mm;
        p.form = ZT_PRUNE_FORM_LDS;
        p.models = mm;
        p.threads = WAVE * PR_WAVES;
        p.lds = (long long)(prune_lds_bytes((int)cap, (int)front, mm, k) * PR_WAVES);
        return p;
    }
    p.form = ZT_PRUNE_FORM_WORKSPACE;
    p.models = n_models < PR_MAX_MODELS ? n_models : PR_MAX_MODELS;
    p.slab_bytes = (long long)ws_slab_bytes((int)cap, (int)front, p.models);
    p.slabs = max_bytes / p.slab_bytes;
    if (p.slabs > ZT_PRUNE_WS_MAX_SLABS) p.slabs = ZT_PRUNE_WS_MAX_SLABS;
    p.grid = (int)p.slabs;
    p.threads = WS_THREADS;
    p.lds = (long long)WS_STATIC_LDS;
    if (p.slabs == 0) {
        set_error("zt_csr_reserve_pruning: width=%d depth=%d models=%d needs %lld bytes for one slab, the budget is %lld",
                  width, depth, p.models, p.slab_bytes, max_bytes);
        p.form = ZT_PRUNE_FORM_REFUSED;
    }
    return p;
}

extern "C" int zt_prune_plan(int32_t width, int32_t depth, int32_t n_models, int32_t k, int64_t max_bytes, int64_t *out)
{
    if (width <= 0 || depth <= 0 || n_models <= 0 || k <= 0 || max_bytes < 0 || !out) {
        set_error("zt_prune_plan: bad argument");
        return ZT_ERR_ARG;
    }
    const PrunePlan p = prune_plan(width, depth, n_models, k, max_bytes);
    out[0] = p.form; out[1] = p.cap_c; out[2] = p.cap_f; out[3] = p.models; out[4] = p.slab_bytes; out[5] = p.slabs;
    out[6] = p.grid; out[7] = p.threads; out[8] = p.lds; out[9] = p.cap_c;
    return ZT_OK;
}

extern "C" int zt_csr_release_pruning(zt_csr *c)
{
    if (!c) return ZT_OK;
    if (c->ws) {
        if (c->ws_used) ZT_HIP(hipEventSynchronize(c->ws_event));      // the launches that use it
        ZT_HIP(hipFree(c->ws));
    }
    if (c->ws_event) ZT_HIP(hipEventDestroy(c->ws_event));
    c->ws = nullptr; c->ws_event = nullptr; c->ws_stream = nullptr; c->ws_used = false;
    c->ws_slab_bytes = 0; c->ws_slabs = c->ws_cap_c = c->ws_cap_f = c->ws_models = 0;
    return ZT_OK;
}

extern "C" int zt_csr_reserve_pruning(zt_csr *c, int32_t width, int32_t depth, int32_t n_models, int32_t k, int64_t max_bytes)
{
    if (!c || width <= 0 || depth <= 0 || n_models <= 0 || k <= 0 || max_bytes < 0) {
        set_error("zt_csr_reserve_pruning: bad argument");
        return ZT_ERR_ARG;
    }
    const PrunePlan p = prune_plan(width, depth, n_models, k, max_bytes);
    if (p.form == ZT_PRUNE_FORM_REFUSED) return ZT_ERR_UNSUPPORTED;
    if (p.form == ZT_PRUNE_FORM_LDS) return ZT_OK;                     // nothing to reserve
    int rc = zt_csr_release_pruning(c);
    if (rc != ZT_OK) return rc;
    ZT_HIP(hipMalloc(&c->ws, (size_t)p.slabs * (size_t)p.slab_bytes));
    if (hipEventCreateWithFlags(&c->ws_event, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(c->ws); c->ws = nullptr; c->ws_event = nullptr;
        set_error("zt_csr_reserve_pruning: hipEventCreateWithFlags failed");
        return ZT_ERR_HIP;
    }
    c->ws_slab_bytes = p.slab_bytes; c->ws_slabs = (int)p.slabs;
    c->ws_cap_c = (int)p.cap_c; c->ws_cap_f = (int)p.cap_f; c->ws_models = p.models;
    return ZT_OK;
}

// out arrays are [M][nq][k]; one launch per group of models, in either form
static int pruned_launch(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t nq, int32_t width,
                         int32_t depth, int M, const double *alpha, const double *beta, int32_t k, int32_t *on, int32_t *oe,
                         float *od, float *ow, int32_t *status_dev, hipStream_t s, bool zero_empty = false)
{
    PrunePlan plan = prune_plan(width, depth, M, k, 0x7fffffffffffffffll);
    if (plan.form == ZT_PRUNE_FORM_REFUSED) return ZT_ERR_UNSUPPORTED;
    const bool ws = plan.form == ZT_PRUNE_FORM_WORKSPACE;
    if (ws) {
        if (!c->ws || plan.cap_c > c->ws_cap_c || plan.cap_f > c->ws_cap_f) {
            set_error("zt_pruned_topk: k=%d width=%d depth=%d exceeds the LDS-resident limits (k<=%d, sum width^d<=%d) and the "
                      "handle holds no workspace that covers it: use a narrower walk or reserve a workspace: "
                      "zt_csr_reserve_pruning", k, width, depth, ZT_MAX_K_WIDE, MAX_CAND);
            return ZT_ERR_UNSUPPORTED;
        }
        // the workspace serves one launch at a time: behind the previous one, on whatever stream that ran
        if (c->ws_used && c->ws_stream != s) ZT_HIP(hipStreamWaitEvent(s, c->ws_event, 0));
    }
#ifdef ZT_DIAG
    static const int dbg_stop = getenv("ZT_PRUNE_STOP") ? atoi(getenv("ZT_PRUNE_STOP")) : 0;   // diagnostic builds only (WRONG results): 1 walk only, 2 + merge
#else
    constexpr int dbg_stop = 0;
#endif
    for (int m0 = 0; m0 < M;) {
        // The models that remain are planned like a call of their own.  The form does not depend on M, and a launch's bytes
        // are monotone in its models, so a group is min(remaining, the first plan's models) of them; a last group of fewer
        // models asks for the LDS of that many.  A workspace carries the models it was reserved for.
        if (m0 > 0) plan = prune_plan(width, depth, M - m0, k, 0x7fffffffffffffffll);
        const int mm = ws && c->ws_models < plan.models ? c->ws_models : plan.models;
        PruneModels pm;
        pm.M = mm;
        for (int q = 0; q < mm; ++q) { pm.alpha[q] = alpha[m0 + q]; pm.beta[q] = beta[m0 + q]; }
        const size_t o = (size_t)m0 * nq * k;
        if (!ws) ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_pruned_topk), (size_t)plan.lds));
        ZT_PROF_BEGIN(s, P_PRUNE);
        if (ws)
            k_pruned_topk_ws<<<(int)(nq < c->ws_slabs ? nq : c->ws_slabs), plan.threads, 0, s>>>(
                c->indptr, c->nbr, c->eid, c->ts, c->N, q_nodes_dev, q_ts_dev, nq, width, depth, pm, k, on + o, oe + o, od + o,
                ow + o, (long long)nq * k, status_dev, c->ws_cap_c, c->ws_cap_f, c->ws_models, (char *)c->ws, c->ws_slab_bytes,
                zero_empty ? 1 : 0);
        else
            k_pruned_topk<<<(int)((nq + PR_WAVES - 1) / PR_WAVES), plan.threads, (size_t)plan.lds, s>>>(
                c->indptr, c->nbr, c->eid, c->ts, c->N, q_nodes_dev, q_ts_dev, nq, width, depth, pm, k, on + o, oe + o, od + o,
                ow + o, (long long)nq * k, status_dev, (int)plan.cap_c, (int)plan.cap_f, dbg_stop, zero_empty ? 1 : 0);
        ZT_PROF_END(s, P_PRUNE);
        ZT_LAUNCH_CHECK();
        m0 += mm;
    }
    if (ws) {
        ZT_HIP(hipEventRecord(c->ws_event, s));
        c->ws_stream = s; c->ws_used = true;
    }
    return ZT_OK;
}

extern "C" int zt_pruned_topk(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t nq,
                              int32_t width, int32_t depth, double alpha, double beta, int32_t k,
                              int32_t *out_nodes_dev, int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev,
                              int32_t *status_dev, void *stream)
{
    if (!c || nq < 0 || width <= 0 || depth <= 0 || k <= 0 || !status_dev) {
        set_error("zt_pruned_topk: bad argument");
        return ZT_ERR_ARG;
    }
    if (nq == 0) return ZT_OK;
    return pruned_launch(c, q_nodes_dev, q_ts_dev, nq, width, depth, 1, &alpha, &beta, k, out_nodes_dev, out_eidx_dev,
                         out_dt_dev, out_w_dev, status_dev, (hipStream_t)stream);
}

// zero_empty: the output arrays were NOT cleared, rows with an empty dictionary are written as zeros by the kernel
static int pruned_multi(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t nq, int32_t width,
                        int32_t depth, int32_t n_models, const double *alpha_host, const double *beta_host, int32_t k,
                        int32_t *out_nodes_dev, int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev, int32_t *status_dev,
                        void *stream, bool zero_empty)
{
    if (!c || nq < 0 || width <= 0 || depth <= 0 || k <= 0 || !status_dev || n_models <= 0 || !alpha_host || !beta_host) {
        set_error("zt_pruned_topk_multi: bad argument");
        return ZT_ERR_ARG;
    }
    if (nq == 0) return ZT_OK;
    return pruned_launch(c, q_nodes_dev, q_ts_dev, nq, width, depth, n_models, alpha_host, beta_host, k, out_nodes_dev,
                         out_eidx_dev, out_dt_dev, out_w_dev, status_dev, (hipStream_t)stream, zero_empty);
}

int zt::pruned_topk_multi_fill(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t nq, int32_t width,
                               int32_t depth, int32_t n_models, const double *alpha_host, const double *beta_host, int32_t k,
                               int32_t *out_nodes_dev, int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev,
                               int32_t *status_dev, void *stream)
{
    return pruned_multi(c, q_nodes_dev, q_ts_dev, nq, width, depth, n_models, alpha_host, beta_host, k, out_nodes_dev,
                        out_eidx_dev, out_dt_dev, out_w_dev, status_dev, stream, true);
}

extern "C" int zt_pruned_topk_multi(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t nq,
                                    int32_t width, int32_t depth, int32_t n_models, const double *alpha_host,
                                    const double *beta_host, int32_t k, int32_t *out_nodes_dev, int32_t *out_eidx_dev,
                                    float *out_dt_dev, float *out_w_dev, int32_t *status_dev, void *stream)
{
    return pruned_multi(c, q_nodes_dev, q_ts_dev, nq, width, depth, n_models, alpha_host, beta_host, k, out_nodes_dev,
                        out_eidx_dev, out_dt_dev, out_w_dev, status_dev, stream, false);
}
