// Top-K link scoring over a large candidate pool ("Read-only queries and ranking"):
//   zt_affinity_topk   for each query the K present candidates with the largest probability -- zt_affinity_rank's probabilities,
//                      bit for bit (rank_pair.hpp) -- without ever writing prob[Q][C].  The pool goes through the workspace in
//                      SLABS of P_c rows, so memory does not grow with it.  Per slab two launches:
//     k_topk_pairs     a workgroup takes RK_TQ queries and a SPAN of candidate columns (rank_walk.hpp's rk_span_walk, shared
//                      with rank_count.hip); every wave keeps a running top-K in registers and leaves one list per
//                      (query, span) in the workspace;
//     k_topk_merge     a wave per query merges the spans' lists -- and the list already in the output, from the slabs before or
//                      from the caller (accumulate) -- and writes the K results.
//   zt_affinity_topk_masked  the same with ABSENT BITS absent[Q][W] (seen.hip writes them): a set bit takes local column c out of
//                      query q's candidates.  k_topk_pairs<., ., true> folds the bit into `present`; the plan, the workspace and
//                      the merge are the unmasked call's.
//   No workgroup waits for another, no atomics but atomicExch on the status word, every loop bounded by its arguments.
// A candidate is a 64-bit key (probability bits << 32) | ~index: probabilities are >= +0, so the bits order as unsigned, and
// among equal probabilities the smaller index has the larger key.  Keys are distinct (indices are), the order is strict and
// the K largest of a union are the K largest of the K largest of its parts: no tiling, slab size or grid changes a bit.
// Key 0 is the empty slot (~index >= 0x80000000 for every index a call can name).
#include <algorithm>

#include "common.hpp"
#include "rank_walk.hpp"

using namespace zt;

namespace {

constexpr int TK_MAX_K = ZT_TOPK_MAX_K;
constexpr int TK_WAVES = 4;                          // waves per workgroup, both kernels
constexpr long long TK_TARGET_WGS = 2048;            // workgroups of k_topk_pairs worth cutting spans for: 8 per compute unit
constexpr int TK_MIN_STEPS = 8;                      // steps of a workgroup per span at least: the list's warm-up is paid per span

struct TopkPlan {
    int form, nq;                     // ZT_TOPK_FORM_*; queries per wave: RK_TQ (shared pool) or 1 (indexed)
    long long q_tiles, slab_rows, n_slabs, span_cols, n_spans, grid1, grid2;
    long long off_part, off_pc, min_bytes, max_spans;
};

// byte offsets of the partial lists and of the slab's P_c behind the status word and P_q
inline void topk_layout(long long Q, int H, int K, TopkPlan &p)
{
    p.q_tiles = (Q + RK_TQ - 1) / RK_TQ;
    p.max_spans = rank_max_spans(TK_TARGET_WGS, p.q_tiles);
    p.off_part = rank_layout_head(Q, H);
    // Q * max_spans lists at most: below RK_TQ * (TK_TARGET_WGS + q_tiles), which -- unlike the product -- grows with Q
    p.off_pc = p.off_part + round_up_ll((TK_TARGET_WGS + p.q_tiles) * RK_TQ * K * 8, 256);
    p.min_bytes = p.off_pc + 32ll * H * 4;
}

// Pure host code: the form, the slab rows, the spans and the grids of one call -- the one place that decides them.
// false: the workspace is below the minimum.
bool topk_plan(long long Q, long long Nc, long long C, int H, int K, bool indexed, long long workspace_bytes, TopkPlan &p)
{
    topk_layout(Q, H, K, p);
    p.form = K <= 64 ? ZT_TOPK_FORM_LANE : ZT_TOPK_FORM_LANE4;
    p.nq = indexed ? 1 : RK_TQ;
    if (workspace_bytes < p.min_bytes) return false;
    p.slab_rows = rank_slab_rows(H, workspace_bytes - p.off_pc);
    p.n_slabs = std::max(1ll, (Nc + p.slab_rows - 1) / p.slab_rows);
    // columns a launch walks: the slab's rows (shared pool) or all C index columns; a step of a workgroup takes step_cols
    const long long cols = indexed ? C : std::min(p.slab_rows, std::max(Nc, 1ll));
    rank_cut_spans(cols, indexed ? RK_TC : (long long)TK_WAVES * RK_TC, TK_MIN_STEPS, p.max_spans, p.span_cols, p.n_spans);
    p.grid1 = p.q_tiles * p.n_spans;
    p.grid2 = (Q + TK_WAVES - 1) / TK_WAVES;
    return true;
}

struct TopkArgs : RkWalkArgs {
    const int *skip;                  // [Q] or NULL
    int K;
    u64 *part;                        // [Q][n_spans][K]
};

__device__ __forceinline__ u64 tk_readlane(u64 v, int src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 tk_shfl(u64 v, int src)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, WAVE), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, WAVE);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 tk_key(float p, long long index) { return ((u64)__float_as_uint(p) << 32) | (unsigned)~(unsigned)index; }

// A wave's list: position i = 64 r + lane in m[r], descending, positions >= K and empty slots 0.  Wave-uniform control flow,
// every lane active, in all three.
template <int NR>
__device__ __forceinline__ u64 tk_kth(const u64 (&m)[NR], int K)
{
    const int rk = (K - 1) >> 6;
    u64 v = m[0];
#pragma unroll
    for (int r = 1; r < NR; ++r)
        if (rk == r) v = m[r];
    return tk_readlane(v, (K - 1) & 63);
}

template <int NR>
__device__ __forceinline__ void tk_insert(u64 (&m)[NR], u64 x, int K, int lane)
{
    int pos = 0;                                       // keys above x: where x goes
#pragma unroll
    for (int r = 0; r < NR; ++r) pos += __popcll(__ballot(m[r] > x));
#pragma unroll
    for (int r = NR - 1; r >= 0; --r) {                // (descending: m[r - 1] is still the old one)
        u64 up = tk_shfl(m[r], (lane + 63) & 63);      // the key one position above
        if (r > 0) {
            const u64 carry = tk_readlane(m[r - 1], 63);
            if (lane == 0) up = carry;
        }
        const int p = r * 64 + lane;
        const u64 nv = p < pos ? m[r] : (p == pos ? x : up);
        m[r] = p < K ? nv : 0ull;
    }
}

// every lane offers one key (0: none): tested against the K-th key by one ballot, the survivors inserted one by one
template <int NR>
__device__ __forceinline__ void tk_offer(u64 (&m)[NR], u64 &kth, u64 key, int K, int lane)
{
    u64 mask = __ballot(key > kth);
    while (mask != 0) {                                // at most 64 rounds
        const int src = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        const u64 x = tk_readlane(key, src);
        if (x > kth) {
            tk_insert<NR>(m, x, K, lane);
            kth = tk_kth<NR>(m, K);
        }
    }
}

// One workgroup: RK_TQ queries against one span of candidate columns -- rank_walk.hpp's span walk (rk_span_walk: the steps, the
// rows, the NaN rule, the absent bits, the pair sum), whose every probability is offered to a running top-K.
//   NQ = RK_TQ (shared pool): every wave keeps four lists, one per query of the tile; at the end wave w merges the four waves'
//        lists of query w through LDS.
//   NQ = 1 (indexed): wave w owns query q0 + w and keeps its one list.
// NR: u64 registers per lane and list (1: K <= 64; 4: K <= 256).
// MASKED: the walk folds the bits of a.absent into `present`.  false: none of this is compiled in.
template <int NQ, int NR, bool MASKED = false>
__global__ __launch_bounds__(WAVE * TK_WAVES) void k_topk_pairs(const TopkArgs a)
{
    __shared__ RkTileLds s_t;
    __shared__ u64 s_list[NQ == 1 ? 1 : TK_WAVES][NQ][WAVE * NR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool shared = NQ != 1;
    const long long qt = blockIdx.x / a.n_spans, span = blockIdx.x - qt * a.n_spans;
    const long long q0 = qt * RK_TQ;
    const int K = a.K;

    u64 m[NQ][NR], kth[NQ];
    long long skipc[NQ];                                                // the global column query qi leaves out, or -1
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
        for (int r = 0; r < NR; ++r) m[qi][r] = 0ull;
        kth[qi] = 0ull;
        const long long q = q0 + (shared ? qi : wave);
        skipc[qi] = (a.skip != nullptr && q < a.Q) ? (long long)a.skip[q] : -1ll;
    }
    rk_span_walk<NQ, MASKED, TK_WAVES>(a, s_t, q0, span, [&](int qi, float p, bool present, long long gcol) {
        tk_offer<NR>(m[qi], kth[qi], present && gcol != skipc[qi] ? tk_key(p, gcol) : 0ull, K, lane);
    });

    if (!shared) {
        const long long q = q0 + wave;
        if (q < a.Q) {
            u64 *out = a.part + (q * a.n_spans + span) * K;
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (r * 64 + lane < K) out[r * 64 + lane] = m[0][r];
        }
        return;
    }
    // the four waves' lists of query w into wave w's
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
        for (int r = 0; r < NR; ++r) s_list[wave][qi][r * 64 + lane] = m[qi][r];
    __syncthreads();
    const long long q = q0 + wave;
    if (q >= a.Q) return;
    u64 f[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) f[r] = s_list[0][wave][r * 64 + lane];        // wave 0's: a list already
    u64 fk = tk_kth<NR>(f, K);
    for (int v = 1; v < TK_WAVES; ++v)
#pragma unroll
        for (int r = 0; r < NR; ++r) tk_offer<NR>(f, fk, s_list[v][wave][r * 64 + lane], K, lane);
    u64 *out = a.part + (q * a.n_spans + span) * K;
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r * 64 + lane < K) out[r * 64 + lane] = f[r];
}

// A wave per query: the n_spans lists of the launch before, with the K entries already in the output where `accumulate` says so
// (-1: an empty slot), into the output: descending, equal probabilities in ascending index, empty slots -1 and 0.
template <int NR>
__global__ __launch_bounds__(WAVE * TK_WAVES) void k_topk_merge(const u64 *__restrict__ part, long long Q, long long n_spans, int K,
                                                                int accumulate, int *top_idx, float *top_prob)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * TK_WAVES + wave;
    if (q >= Q) return;
    u64 m[NR], kth = 0ull;
#pragma unroll
    for (int r = 0; r < NR; ++r) m[r] = 0ull;
    if (accumulate) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int pos = r * 64 + lane;
            u64 key = 0ull;
            if (pos < K) {
                const int ix = top_idx[q * K + pos];
                const float p = top_prob[q * K + pos];
                if (ix >= 0 && p == p) key = tk_key(p, ix);
            }
            tk_offer<NR>(m, kth, key, K, lane);
        }
    }
    const long long n = n_spans * K;
    const u64 *src = part + q * n;
    for (long long i0 = 0; i0 < n; i0 += WAVE) {
        const long long i = i0 + lane;
        tk_offer<NR>(m, kth, i < n ? src[i] : 0ull, K, lane);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int pos = r * 64 + lane;
        if (pos < K) {
            const u64 key = m[r];
            top_idx[q * K + pos] = key != 0ull ? (int)~(unsigned)key : -1;
            top_prob[q * K + pos] = key != 0ull ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
        }
    }
}

__global__ void k_topk_fill_empty(long long n, int *top_idx, float *top_prob)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        top_idx[i] = -1;
        top_prob[i] = 0.f;
    }
}

// the checks zt_affinity_topk, its plan and its workspace size share; ZT_OK or the code, with the message set
int topk_check_shape(const char *who, int H, int K)
{
    if (K <= 0) {
        set_error("%s: K=%d (1 <= K <= %d)", who, K, TK_MAX_K);
        return ZT_ERR_ARG;
    }
    if (K > TK_MAX_K) {
        set_error("%s: K=%d unsupported (1 <= K <= %d)", who, K, TK_MAX_K);
        return ZT_ERR_UNSUPPORTED;
    }
    return rank_width_ok(H) ? ZT_OK : rank_width_refused(who, H);
}

}  // namespace

extern "C" int64_t zt_affinity_topk_workspace_bytes(int64_t Q, int64_t Nc, int32_t H, int32_t K)
{
    if (Q < 0 || Nc < 0 || !rank_width_ok(H) || K <= 0 || K > TK_MAX_K) return -1;
    TopkPlan p;
    topk_layout(Q, H, K, p);
    return p.off_pc + rank_pool_rows(Nc, H) * (long long)H * 4;
}

extern "C" int zt_affinity_topk_plan(int64_t Q, int64_t Nc, int64_t C, int32_t H, int32_t K, int32_t indexed,
                                     int64_t workspace_bytes, int64_t *plan_out)
{
    if (!plan_out || Q < 0 || Nc < 0 || C < 0 || (!indexed && C != Nc)) {
        set_error("zt_affinity_topk_plan: bad argument");
        return ZT_ERR_ARG;
    }
    const int rc = topk_check_shape("zt_affinity_topk_plan", H, K);
    if (rc != ZT_OK) return rc;
    TopkPlan p;
    if (!topk_plan(Q, Nc, C, H, K, indexed != 0, workspace_bytes, p)) {
        set_error("zt_affinity_topk_plan: workspace of %lld bytes, at least %lld needed (zt_affinity_topk_workspace_bytes for Nc = 32)",
                  (long long)workspace_bytes, p.min_bytes);
        return ZT_ERR_ARG;
    }
    const long long v[ZT_TOPK_PLAN_FIELDS] = {p.form, p.nq, p.q_tiles, p.slab_rows, p.n_slabs, p.span_cols, p.n_spans, p.grid1,
                                              p.grid2, p.off_part, p.off_pc, p.min_bytes};
    for (int i = 0; i < ZT_TOPK_PLAN_FIELDS; ++i) plan_out[i] = v[i];
    return ZT_OK;
}

// zt_affinity_topk and zt_affinity_topk_masked (absent_dev NULL: the former exactly)
static int topk_run(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc, const int32_t *cand_idx_dev, int64_t C,
                    int32_t H, const zt_affinity_weights *w, int32_t K, const int32_t *skip_dev, int64_t idx_base,
                    int32_t accumulate, int32_t *top_idx_dev, float *top_prob_dev, void *workspace_dev, int64_t workspace_bytes,
                    const uint32_t *absent_dev, int64_t absent_words, void *stream)
{
    if (!emb_q_dev || !emb_c_dev || !w || !top_idx_dev || !top_prob_dev || !workspace_dev || Q < 0 || Nc < 0 || C < 0 || idx_base < 0) {
        set_error("zt_affinity_topk: bad argument");
        return ZT_ERR_ARG;
    }
    if (absent_dev != nullptr && absent_words < (C + 31) / 32) {
        set_error("zt_affinity_topk_masked: absent_words=%lld, C=%lld columns need %lld", (long long)absent_words, (long long)C,
                  (long long)((C + 31) / 32));
        return ZT_ERR_ARG;
    }
    int rc = topk_check_shape("zt_affinity_topk", H, K);
    if (rc != ZT_OK) return rc;
    if (cand_idx_dev == nullptr && C != Nc) {
        set_error("zt_affinity_topk: without cand_idx every query takes all Nc=%lld candidates, C=%lld given", (long long)Nc,
                  (long long)C);
        return ZT_ERR_ARG;
    }
    if (idx_base > 0x7fffffffll - C) {
        set_error("zt_affinity_topk: idx_base=%lld + C=%lld exceeds the int32 indices of the result", (long long)idx_base, (long long)C);
        return ZT_ERR_ARG;
    }
    TopkPlan p;
    if (!topk_plan(Q, Nc, C, H, K, cand_idx_dev != nullptr, workspace_bytes, p)) {
        set_error("zt_affinity_topk: workspace of %lld bytes, at least %lld needed (zt_affinity_topk_workspace_bytes for Nc = 32)",
                  (long long)workspace_bytes, p.min_bytes);
        return ZT_ERR_ARG;
    }
    if (p.grid1 > 0x7fffffffll || p.grid2 > 0x7fffffffll) {
        set_error("zt_affinity_topk: Q=%lld queries exceed one launch's workgroups", (long long)Q);
        return ZT_ERR_UNSUPPORTED;
    }
    if (Q == 0) return ZT_OK;
    hipStream_t s = (hipStream_t)stream;
    if (C == 0) {
        if (!accumulate) {
            k_topk_fill_empty<<<(unsigned)((Q * K + 255) / 256), 256, 0, s>>>(Q * K, top_idx_dev, top_prob_dev);
            ZT_LAUNCH_CHECK();
        }
        return ZT_OK;
    }
    if (!rank_weights_ok("zt_affinity_topk", w, workspace_dev)) return ZT_ERR_ARG;
    char *ws = reinterpret_cast<char *>(workspace_dev);
    int *status = reinterpret_cast<int *>(ws);
    float *Pq = reinterpret_cast<float *>(ws + RK_HEAD), *Pc = reinterpret_cast<float *>(ws + p.off_pc);
    u64 *part = reinterpret_cast<u64 *>(ws + p.off_part);
    ZT_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    rc = rank_project(emb_q_dev, w, false, Pq, Q, H, stream);
    if (rc != ZT_OK) return rc;
    TopkArgs a;
    a.Pq = Pq; a.Pc = Pc; a.cand_idx = cand_idx_dev; a.skip = skip_dev;
    a.Q = Q; a.Nc = Nc; a.C = C; a.idx_base = idx_base;
    a.n_spans = p.n_spans; a.span_cols = p.span_cols;
    a.H = H; a.K = K;
    a.b1 = w->fc1_b; a.w2 = w->fc2_w; a.b2 = w->fc2_b;
    a.part = part; a.status = status;
    a.absent = absent_dev; a.absent_words = absent_words;
    const bool masked = absent_dev != nullptr;
    for (long long slab = 0; slab < p.n_slabs; ++slab) {       // P_c a slab at a time
        a.r0 = slab * p.slab_rows;
        a.rows = std::min<long long>(p.slab_rows, Nc - a.r0);
        rc = rank_project(emb_c_dev + a.r0 * H, w, true, Pc, a.rows, H, stream);
        if (rc != ZT_OK) return rc;
        ZT_PROF_BEGIN(s, P_SCORE);
        const unsigned g1 = (unsigned)p.grid1, g2 = (unsigned)p.grid2, th = WAVE * TK_WAVES;
        const int acc = (accumulate != 0 || slab > 0) ? 1 : 0;
        if (p.form == ZT_TOPK_FORM_LANE) {
            if (masked) {
                if (p.nq == 1) k_topk_pairs<1, 1, true><<<g1, th, 0, s>>>(a);
                else k_topk_pairs<RK_TQ, 1, true><<<g1, th, 0, s>>>(a);
            } else if (p.nq == 1) k_topk_pairs<1, 1><<<g1, th, 0, s>>>(a);
            else k_topk_pairs<RK_TQ, 1><<<g1, th, 0, s>>>(a);
            ZT_LAUNCH_CHECK();
            k_topk_merge<1><<<g2, th, 0, s>>>(part, Q, p.n_spans, K, acc, top_idx_dev, top_prob_dev);
        } else {
            if (masked) {
                if (p.nq == 1) k_topk_pairs<1, 4, true><<<g1, th, 0, s>>>(a);
                else k_topk_pairs<RK_TQ, 4, true><<<g1, th, 0, s>>>(a);
            } else if (p.nq == 1) k_topk_pairs<1, 4><<<g1, th, 0, s>>>(a);
            else k_topk_pairs<RK_TQ, 4><<<g1, th, 0, s>>>(a);
            ZT_LAUNCH_CHECK();
            k_topk_merge<4><<<g2, th, 0, s>>>(part, Q, p.n_spans, K, acc, top_idx_dev, top_prob_dev);
        }
        ZT_LAUNCH_CHECK();
        ZT_PROF_END(s, P_SCORE);
    }
    return ZT_OK;
}

extern "C" int zt_affinity_topk(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                                const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w, int32_t K,
                                const int32_t *skip_dev, int64_t idx_base, int32_t accumulate, int32_t *top_idx_dev,
                                float *top_prob_dev, void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    return topk_run(emb_q_dev, Q, emb_c_dev, Nc, cand_idx_dev, C, H, w, K, skip_dev, idx_base, accumulate, top_idx_dev, top_prob_dev,
                    workspace_dev, workspace_bytes, nullptr, 0, stream);
}

extern "C" int zt_affinity_topk_masked(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                                       const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w, int32_t K,
                                       const int32_t *skip_dev, int64_t idx_base, int32_t accumulate, int32_t *top_idx_dev,
                                       float *top_prob_dev, void *workspace_dev, int64_t workspace_bytes,
                                       const uint32_t *absent_dev, int64_t absent_words, void *stream)
{
    return topk_run(emb_q_dev, Q, emb_c_dev, Nc, cand_idx_dev, C, H, w, K, skip_dev, idx_base, accumulate, top_idx_dev, top_prob_dev,
                    workspace_dev, workspace_bytes, absent_dev, absent_words, stream);
}
