// Top-K link scoring over a large candidate pool ("Read-only queries and ranking"):
//   zt_affinity_topk   for each query the K present candidates with the largest probability -- zt_affinity_rank's probabilities,
//                      bit for bit (rank_pair.hpp) -- without ever writing prob[Q][C].  The pool goes through the workspace in
//                      SLABS of P_c rows, so memory does not grow with it.  Per slab two launches:
//     k_topk_pairs     a workgroup takes RK_TQ queries and a SPAN of candidate columns; every wave keeps a running top-K in
//                      registers and leaves one list per (query, span) in the workspace;
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
#include "rank_pair.hpp"

using namespace zt;

namespace {

constexpr int TK_MAX_K = ZT_TOPK_MAX_K;
constexpr int TK_WAVES = 4;                          // waves per workgroup, both kernels
constexpr long long TK_SLAB_BYTES = 128ll << 20;     // P_c of one slab at most: half the Infinity Cache
constexpr long long TK_SLAB_ROWS = 1ll << 18;        // ... and its rows at most (narrow H): launches are long paid for by then
constexpr long long TK_TARGET_WGS = 2048;            // workgroups of k_topk_pairs worth cutting spans for: 8 per compute unit
constexpr int TK_MIN_STEPS = 8;                      // steps of a workgroup per span at least: the list's warm-up is paid per span

struct TopkPlan {
    int form, nq;                     // ZT_TOPK_FORM_*; queries per wave: RK_TQ (shared pool) or 1 (indexed)
    long long q_tiles, slab_rows, n_slabs, span_cols, n_spans, grid1, grid2;
    long long off_part, off_pc, min_bytes, max_spans;
};

inline long long round_up_ll(long long x, long long m) { return (x + m - 1) / m * m; }
inline long long topk_cap_rows(int H) { return std::max(32ll, std::min(TK_SLAB_ROWS, TK_SLAB_BYTES / ((long long)H * 4) / 32 * 32)); }
inline long long topk_max_spans(long long q_tiles) { return std::max(1ll, (TK_TARGET_WGS + q_tiles - 1) / std::max(1ll, q_tiles)); }
// byte offsets of the partial lists and of the slab's P_c behind the status word and P_q
inline void topk_layout(long long Q, int H, int K, TopkPlan &p)
{
    p.q_tiles = (Q + RK_TQ - 1) / RK_TQ;
    p.max_spans = topk_max_spans(p.q_tiles);
    p.off_part = (long long)RK_HEAD + round_up_ll(Q * (long long)H * 4, 256);
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
    p.slab_rows = std::min(topk_cap_rows(H), (workspace_bytes - p.off_pc) / ((long long)H * 4) / 32 * 32);
    p.n_slabs = std::max(1ll, (Nc + p.slab_rows - 1) / p.slab_rows);
    // columns a launch walks: the slab's rows (shared pool) or all C index columns; a step of a workgroup takes step_cols
    const long long cols = indexed ? C : std::min(p.slab_rows, std::max(Nc, 1ll));
    const long long step_cols = indexed ? RK_TC : (long long)TK_WAVES * RK_TC;
    long long n = std::min(p.max_spans, std::max(1ll, cols / (step_cols * TK_MIN_STEPS)));
    p.span_cols = round_up_ll((std::max(cols, 1ll) + n - 1) / n, step_cols);
    p.n_spans = std::max(1ll, (cols + p.span_cols - 1) / p.span_cols);
    p.grid1 = p.q_tiles * p.n_spans;
    p.grid2 = (Q + TK_WAVES - 1) / TK_WAVES;
    return true;
}

struct TopkArgs {
    const float *Pq, *Pc;             // [Q][H]; the slab's rows [r0, r0 + rows) of P_c
    const int *cand_idx, *skip;       // [Q][C] or NULL; [Q] or NULL
    long long Q, Nc, C, r0, rows, idx_base;
    long long n_spans, span_cols;
    int H, K;
    const float *b1, *w2, *b2;
    u64 *part;                        // [Q][n_spans][K]
    int *status;
    const unsigned *absent;           // [Q][absent_words] or NULL: read by the MASKED instantiations alone
    long long absent_words;
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

// One workgroup: RK_TQ queries against one span of candidate columns, in steps.
//   NQ = RK_TQ (shared pool): every wave scores all RK_TQ queries against ITS 32 candidates of the step -- a candidate row's
//        float4s are loaded into registers once and run against the four query rows from LDS -- and keeps four lists; at the
//        end wave w merges the four waves' lists of query w through LDS.
//   NQ = 1 (indexed): wave w owns query q0 + w and walks the span's index columns 32 at a time, as k_rank_pairs does; rows
//        outside the slab are passed over (another slab's launch takes them).
// NR: u64 registers per lane and list (1: K <= 64; 4: K <= 256).
// MASKED: a candidate is present only if its bit of a.absent is clear -- bit c of row q, c the LOCAL column of the call
//        (a.r0 + mycol in the shared form: the slab's offset counts; mycol in the indexed form); every query of a wave tests
//        its own row.  The word is loaded ahead of the pair sum, once per wave.  false: none of this is compiled in.
// The (P_q + b1) rows and w2 lie in LDS a chunk of RK_HC columns at a time: H <= RK_HC loads them once, wider rows once per
// step and chunk.  The pair sum is rank_pair.hpp's.
template <int NQ, int NR, bool MASKED = false>
__global__ __launch_bounds__(WAVE * TK_WAVES) void k_topk_pairs(const TopkArgs a)
{
    __shared__ float4 s_q[RK_TQ][RK_HC / 4];
    __shared__ float4 s_w[RK_HC / 4];
    __shared__ u64 s_list[NQ == 1 ? 1 : TK_WAVES][NQ][WAVE * NR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, gl = lane & 15;
    const bool shared = NQ != 1;
    const long long qt = blockIdx.x / a.n_spans, span = blockIdx.x - qt * a.n_spans;
    const long long q0 = qt * RK_TQ;
    const int H = a.H, K = a.K;
    const long long cols = shared ? a.rows : a.C;                       // what the spans cut
    const long long lo = min(cols, span * a.span_cols), hi = min(cols, lo + a.span_cols);
    const long long step_cols = shared ? (long long)TK_WAVES * RK_TC : RK_TC;
    const long long nsteps = (hi - lo + step_cols - 1) / step_cols;     // the same for the four waves (barriers below)
    const int nchunks = (H + RK_HC - 1) / RK_HC;
    const float bias2 = a.b2[0];

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

    auto load_chunk = [&](int h0, int hn) {
        for (int v = tid; v < (RK_TQ + 1) * (hn / 4); v += WAVE * TK_WAVES) {
            const int r = v / (hn / 4), c4 = v - r * (hn / 4);
            const float4 b = *reinterpret_cast<const float4 *>((r < RK_TQ ? a.b1 : a.w2) + h0 + 4 * c4);
            if (r == RK_TQ) { s_w[c4] = b; continue; }
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q0 + r < a.Q) p = *reinterpret_cast<const float4 *>(a.Pq + (q0 + r) * H + h0 + 4 * c4);
            s_q[r][c4] = rk_query_bias(p, b);
        }
    };
    if (nchunks == 1) {
        load_chunk(0, H);
        __syncthreads();
    }

    const int myj = rk_fold_pair(gl);                                   // the pair of its group whose sum this lane ends with
    for (long long t = 0; t < nsteps; ++t) {
        // this lane's own candidate: column, local row in the slab (-1: nothing to read)
        const long long mycol = lo + t * step_cols + (shared ? wave * RK_TC : 0) + grp * RK_NC + myj;
        int myrow = -1;
        if (mycol < hi) {
            if (shared) {
                myrow = (int)mycol;
            } else if (q0 + wave < a.Q) {
                const long long r = (long long)a.cand_idx[(q0 + wave) * a.C + mycol];
                if (r < -1 || r >= a.Nc) atomicExch(a.status, (int)ZT_ERR_RANGE);
                else if (r >= a.r0 && r < a.r0 + a.rows) myrow = (int)(r - a.r0);
            }
        }
        // a NaN anywhere in a candidate's embedding makes its whole projected row NaN; the pair sum's relu (fmaxf) would drop
        // it and zt_affinity_rank writes a finite number there -- here such a candidate is a NaN candidate: never selected
        const bool nan_row = myrow >= 0 && a.Pc[(long long)myrow * H] != a.Pc[(long long)myrow * H];
        // MASKED: the wave's RK_TC = 32 columns of this step lie in ONE word of a query's bits -- spans begin at multiples of
        // the step and slabs at multiples of 32 rows (topk_plan) --, so the word's address is the same in every lane
        unsigned gone[NQ];
        if (MASKED) {
            static_assert(RK_TC == 32, "one word of absent bits per wave and step");
            const long long wcol = lo + t * step_cols + (shared ? __builtin_amdgcn_readfirstlane(wave) * RK_TC : 0);
            const long long word = ((shared ? a.r0 : 0) + wcol) >> 5;      // < ceil(C / 32) wherever wcol < hi
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                const long long q = q0 + (shared ? qi : __builtin_amdgcn_readfirstlane(wave));
                gone[qi] = (wcol < hi && q < a.Q) ? a.absent[q * a.absent_words + word] : 0u;
            }
        }
        int row[RK_NC];
#pragma unroll
        for (int j = 0; j < RK_NC; ++j)          // pair j's row from the lane of this group that owns it (bit 0 of gl clear)
            row[j] = __shfl(myrow, (lane & 48) | ((j & 4) << 1) | ((j & 2) << 1) | ((j & 1) << 1), WAVE);

        float acc[NQ][RK_NC];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
            for (int j = 0; j < RK_NC; ++j) acc[qi][j] = 0.f;

        for (int h0 = 0; h0 < H; h0 += RK_HC) {
            const int hn = min(RK_HC, H - h0);                 // a multiple of 4
            if (nchunks > 1) {
                __syncthreads();                               // the chunk before has been read
                load_chunk(h0, hn);
                __syncthreads();
            }
            for (int c4 = gl; c4 < hn / 4; c4 += RK_GROUP) {
                float4 pc[RK_NC];
#pragma unroll
                for (int j = 0; j < RK_NC; ++j) {
                    pc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (row[j] >= 0) pc[j] = *reinterpret_cast<const float4 *>(a.Pc + (long long)row[j] * H + h0 + 4 * c4);
                }
                const float4 w = s_w[c4];
#pragma unroll
                for (int qi = 0; qi < NQ; ++qi) {
                    const float4 pq = s_q[shared ? qi : wave][c4];
#pragma unroll
                    for (int j = 0; j < RK_NC; ++j) acc[qi][j] = rk_pair_step(acc[qi][j], w, pq, pc[j]);
                }
            }
        }
        const long long gcol = (shared ? a.r0 : 0) + mycol + a.idx_base;   // the index this lane's candidate is returned under
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            const float p = rk_prob(rk_fold16x8(acc[qi], gl), bias2);
            bool present = myrow >= 0 && !nan_row && (gl & 1) == 0 && p == p && q0 + (shared ? qi : wave) < a.Q && gcol != skipc[qi];
            if (MASKED) present = present && ((gone[qi] >> (mycol & 31)) & 1u) == 0u;
            tk_offer<NR>(m[qi], kth[qi], present ? tk_key(p, gcol) : 0ull, K, lane);
        }
    }

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
    if (!rank_width_ok(H)) {
        set_error("%s: H=%d unsupported (H %% 4 == 0 and %d <= H <= %d)", who, H, RANK_MIN_H, RANK_MAX_H);
        return ZT_ERR_UNSUPPORTED;
    }
    return ZT_OK;
}

}  // namespace

extern "C" int64_t zt_affinity_topk_workspace_bytes(int64_t Q, int64_t Nc, int32_t H, int32_t K)
{
    if (Q < 0 || Nc < 0 || !rank_width_ok(H) || K <= 0 || K > TK_MAX_K) return -1;
    TopkPlan p;
    topk_layout(Q, H, K, p);
    const long long rows = std::min(topk_cap_rows(H), round_up_ll(std::max<long long>(Nc, 32), 32));
    return p.off_pc + rows * (long long)H * 4;
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
    if (!w->fc1_w || !w->fc1_b || !w->fc2_w || !w->fc2_b || ((uintptr_t)workspace_dev & 15) || ((uintptr_t)w->fc1_b & 15) ||
        ((uintptr_t)w->fc2_w & 15)) {
        set_error("zt_affinity_topk: NULL weight, or workspace / fc1 bias / fc2 weight not 16-byte aligned");
        return ZT_ERR_ARG;
    }
    char *ws = reinterpret_cast<char *>(workspace_dev);
    int *status = reinterpret_cast<int *>(ws);
    float *Pq = reinterpret_cast<float *>(ws + RK_HEAD), *Pc = reinterpret_cast<float *>(ws + p.off_pc);
    u64 *part = reinterpret_cast<u64 *>(ws + p.off_part);
    ZT_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    // W_a = columns [0, H) of fc1.weight [H][2H], W_b = columns [H, 2H): the GEMM calls of zt_affinity_rank, P_c a slab at a time
    rc = zt_gemm_f32(emb_q_dev, w->fc1_w, Pq, Q, H, H, H, 2 * (int64_t)H, H, 0, 1, 0, stream);
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
    for (long long slab = 0; slab < p.n_slabs; ++slab) {
        a.r0 = slab * p.slab_rows;
        a.rows = std::min<long long>(p.slab_rows, Nc - a.r0);
        rc = zt_gemm_f32(emb_c_dev + a.r0 * H, w->fc1_w + H, Pc, a.rows, H, H, H, 2 * (int64_t)H, H, 0, 1, 0, stream);
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
