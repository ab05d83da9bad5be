// Where a probability stands in a large candidate pool ("Read-only queries and ranking"):
//   zt_affinity_count  for each query the number of present candidates of a shared pool whose probability -- zt_affinity_rank's,
//                      bit for bit (rank_pair.hpp) -- is ABOVE the query's threshold and the number EQUAL to it, without ever
//                      writing prob[Q][C]: the two integers a full-pool rank needs.  The walk is rank_walk.hpp's, as
//                      rank_topk.hip's is: the pool goes through the workspace in SLABS of P_c rows, per slab one launch of
//     k_count_pairs    a workgroup takes RK_TQ queries and a SPAN of candidate columns; every wave scores its 32 candidates of a
//                      step against the four query rows from LDS and keeps 2 x RK_TQ counters fed by ballots (wave-uniform
//                      integers); at the end the four waves' counters are added through LDS and ONE integer atomicAdd per
//                      (query, counter, workgroup) goes into the outputs.
//   Integer sums commute: the counts are a function of the inputs alone, whatever the slab, span, grid or workspace.  No float
//   atomics, no workgroup waits for another, every loop bounded by its arguments.  The shared pool only: a per-query candidate
//   table is small and goes through zt_affinity_rank + zt_rank_metrics.
#include <algorithm>

#include "common.hpp"
#include "rank_walk.hpp"

using namespace zt;

namespace {

constexpr int CN_WAVES = 4;                          // waves per workgroup
constexpr int CN_MAX_SKIP = ZT_COUNT_MAX_SKIP;
constexpr long long CN_TARGET_WGS = 2048;            // workgroups worth cutting spans for: 8 per compute unit
constexpr int CN_MIN_STEPS = 4;                      // steps of a workgroup per span at least: a span pays one load of the query
                                                     // tile into LDS and 2 x RK_TQ atomics, no list warm-up as the top-K's
constexpr long long CN_STEP_COLS = (long long)CN_WAVES * RK_TC;      // 128 columns a workgroup takes per step

struct CountPlan {
    long long q_tiles, slab_rows, n_slabs, span_cols, n_spans, grid, h_chunks, off_pc, min_bytes;
};

// byte offset of the slab's P_c behind the status word and P_q
inline void count_layout(long long Q, int H, CountPlan &p)
{
    p.q_tiles = (Q + RK_TQ - 1) / RK_TQ;
    p.off_pc = rank_layout_head(Q, H);
    p.min_bytes = p.off_pc + 32ll * H * 4;
    p.h_chunks = (H + RK_HC - 1) / RK_HC;
}

// Pure host code: the slab rows, the spans and the grid of one call -- the one place that decides them.
// false: the workspace is below the minimum.
bool count_plan(long long Q, long long Nc, int H, long long workspace_bytes, CountPlan &p)
{
    count_layout(Q, H, p);
    if (workspace_bytes < p.min_bytes) return false;
    p.slab_rows = rank_slab_rows(H, workspace_bytes - p.off_pc);
    p.n_slabs = std::max(1ll, (Nc + p.slab_rows - 1) / p.slab_rows);
    const long long cols = std::min(p.slab_rows, std::max(Nc, 1ll));            // columns a launch walks: a slab's rows
    rank_cut_spans(cols, CN_STEP_COLS, CN_MIN_STEPS, rank_max_spans(CN_TARGET_WGS, p.q_tiles), p.span_cols, p.n_spans);
    p.grid = p.q_tiles * p.n_spans;
    return true;
}

struct CountArgs : RkWalkArgs {      // (cand_idx, Nc, C, status: the indexed form's, unset here)
    const float *thr;                 // [Q]
    const int *skip;                  // [Q][n_skip] or NULL
    int n_skip;
    int *above, *equal;               // [Q], added to
};

// One workgroup: RK_TQ queries against one span of the slab's columns -- rank_walk.hpp's span walk in its shared-pool form
// (rk_span_walk<RK_TQ, MASKED, .>: the steps of CN_STEP_COLS, the NaN rule, the absent bits, the pair sum), here with up to
// CN_MAX_SKIP skipped columns per query.  What happens to a present candidate's probability: two compares against the query's
// threshold and two ballots.  Every lane of a wave takes every ballot (wave-uniform control flow), so the counters are
// wave-uniform.
template <bool MASKED>
__global__ __launch_bounds__(WAVE * CN_WAVES) void k_count_pairs(const CountArgs a)
{
    __shared__ RkTileLds s_t;
    __shared__ int s_cnt[CN_WAVES][2 * RK_TQ];
    __shared__ int s_skip[RK_TQ][CN_MAX_SKIP];                                  // the global columns query qi leaves out, or -1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long qt = blockIdx.x / a.n_spans, span = blockIdx.x - qt * a.n_spans;
    const long long q0 = qt * RK_TQ;

    float thr[RK_TQ];
    int n_above[RK_TQ], n_equal[RK_TQ];
#pragma unroll
    for (int qi = 0; qi < RK_TQ; ++qi) {
        thr[qi] = q0 + qi < a.Q ? a.thr[q0 + qi] : 0.f;
        n_above[qi] = n_equal[qi] = 0;
    }
    if (tid < RK_TQ * CN_MAX_SKIP) {                                            // (read after the barrier every path of the walk has)
        const int qi = tid / CN_MAX_SKIP, j = tid - qi * CN_MAX_SKIP;
        s_skip[qi][j] = (j < a.n_skip && q0 + qi < a.Q) ? a.skip[(q0 + qi) * a.n_skip + j] : -1;
    }
    rk_span_walk<RK_TQ, MASKED, CN_WAVES>(a, s_t, q0, span, [&](int qi, float p, bool present, long long gcol) {
#pragma unroll
        for (int j = 0; j < CN_MAX_SKIP; ++j) present = present && gcol != (long long)s_skip[qi][j];
        n_above[qi] += __popcll(__ballot(present && p > thr[qi]));              // IEEE compares: a NaN threshold counts nothing,
        n_equal[qi] += __popcll(__ballot(present && p == thr[qi]));             // -0.0 equals +0.0
    });

    // the four waves' counters through LDS, then one atomicAdd per query and counter: integer sums, any order gives the number
    if (lane == 0) {
#pragma unroll
        for (int qi = 0; qi < RK_TQ; ++qi) {
            s_cnt[wave][qi] = n_above[qi];
            s_cnt[wave][RK_TQ + qi] = n_equal[qi];
        }
    }
    __syncthreads();
    if (tid < 2 * RK_TQ) {
        int n = 0;
#pragma unroll
        for (int v = 0; v < CN_WAVES; ++v) n += s_cnt[v][tid];
        const int qi = tid < RK_TQ ? tid : tid - RK_TQ;
        if (n != 0 && q0 + qi < a.Q) atomicAdd((tid < RK_TQ ? a.above : a.equal) + q0 + qi, n);
    }
}

}  // namespace

extern "C" int64_t zt_affinity_count_workspace_bytes(int64_t Q, int64_t Nc, int32_t H)
{
    if (Q < 0 || Nc < 0 || !rank_width_ok(H)) return -1;
    CountPlan p;
    count_layout(Q, H, p);
    return p.off_pc + rank_pool_rows(Nc, H) * (long long)H * 4;
}

extern "C" int zt_affinity_count_plan(int64_t Q, int64_t Nc, int32_t H, int64_t workspace_bytes, int64_t *plan_out)
{
    if (!plan_out || Q < 0 || Nc < 0) {
        set_error("zt_affinity_count_plan: bad argument");
        return ZT_ERR_ARG;
    }
    if (!rank_width_ok(H)) return rank_width_refused("zt_affinity_count_plan", H);
    CountPlan p;
    if (!count_plan(Q, Nc, H, workspace_bytes, p)) {
        set_error("zt_affinity_count_plan: workspace of %lld bytes, at least %lld needed (zt_affinity_count_workspace_bytes for Nc = 32)",
                  (long long)workspace_bytes, p.min_bytes);
        return ZT_ERR_ARG;
    }
    const long long v[ZT_COUNT_PLAN_FIELDS] = {p.q_tiles, p.slab_rows, p.n_slabs, p.span_cols, p.n_spans, p.grid, p.h_chunks,
                                               p.off_pc, p.min_bytes};
    for (int i = 0; i < ZT_COUNT_PLAN_FIELDS; ++i) plan_out[i] = v[i];
    return ZT_OK;
}

extern "C" int zt_affinity_count(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc, int32_t H,
                                 const zt_affinity_weights *w, const float *thr_dev, const int32_t *skip_dev, int32_t n_skip,
                                 int64_t idx_base, int32_t accumulate, int32_t *above_dev, int32_t *equal_dev,
                                 void *workspace_dev, int64_t workspace_bytes, const uint32_t *absent_dev, int64_t absent_words,
                                 void *stream)
{
    if (!emb_q_dev || !emb_c_dev || !w || !thr_dev || !above_dev || !equal_dev || !workspace_dev || Q < 0 || Nc < 0 || idx_base < 0) {
        set_error("zt_affinity_count: bad argument");
        return ZT_ERR_ARG;
    }
    if (n_skip < 0 || n_skip > CN_MAX_SKIP || (n_skip > 0 && !skip_dev)) {
        set_error("zt_affinity_count: n_skip=%d (0 <= n_skip <= %d, with skip_dev [Q][n_skip])", n_skip, CN_MAX_SKIP);
        return ZT_ERR_ARG;
    }
    if (absent_dev != nullptr && absent_words < (Nc + 31) / 32) {
        set_error("zt_affinity_count: absent_words=%lld, C=%lld columns need %lld", (long long)absent_words, (long long)Nc,
                  (long long)((Nc + 31) / 32));
        return ZT_ERR_ARG;
    }
    if (!rank_width_ok(H)) return rank_width_refused("zt_affinity_count", H);
    if (idx_base > 0x7fffffffll - Nc) {
        set_error("zt_affinity_count: idx_base=%lld + C=%lld exceeds int32 columns", (long long)idx_base, (long long)Nc);
        return ZT_ERR_ARG;
    }
    CountPlan p;
    if (!count_plan(Q, Nc, H, workspace_bytes, p)) {
        set_error("zt_affinity_count: workspace of %lld bytes, at least %lld needed (zt_affinity_count_workspace_bytes for Nc = 32)",
                  (long long)workspace_bytes, p.min_bytes);
        return ZT_ERR_ARG;
    }
    if (p.grid > 0x7fffffffll) {
        set_error("zt_affinity_count: Q=%lld queries exceed one launch's workgroups", (long long)Q);
        return ZT_ERR_UNSUPPORTED;
    }
    if (Q == 0) return ZT_OK;
    if (!rank_weights_ok("zt_affinity_count", w, workspace_dev)) return ZT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) {                         // the kernels add: a fresh call starts from zeros
        ZT_HIP(hipMemsetAsync(above_dev, 0, Q * sizeof(int32_t), s));
        ZT_HIP(hipMemsetAsync(equal_dev, 0, Q * sizeof(int32_t), s));
    }
    if (Nc == 0) return ZT_OK;
    char *ws = reinterpret_cast<char *>(workspace_dev);
    float *Pq = reinterpret_cast<float *>(ws + RK_HEAD), *Pc = reinterpret_cast<float *>(ws + p.off_pc);
    int rc = rank_project(emb_q_dev, w, false, Pq, Q, H, stream);
    if (rc != ZT_OK) return rc;
    CountArgs a = {};
    a.Pq = Pq; a.Pc = Pc; a.thr = thr_dev; a.skip = n_skip > 0 ? skip_dev : nullptr;
    a.Q = Q; a.idx_base = idx_base;
    a.n_spans = p.n_spans; a.span_cols = p.span_cols;
    a.H = H; a.n_skip = n_skip;
    a.b1 = w->fc1_b; a.w2 = w->fc2_w; a.b2 = w->fc2_b;
    a.above = above_dev; a.equal = equal_dev;
    a.absent = absent_dev; a.absent_words = absent_words;
    for (long long slab = 0; slab < p.n_slabs; ++slab) {       // P_c a slab at a time
        a.r0 = slab * p.slab_rows;
        a.rows = std::min<long long>(p.slab_rows, Nc - a.r0);
        rc = rank_project(emb_c_dev + a.r0 * H, w, true, Pc, a.rows, H, stream);
        if (rc != ZT_OK) return rc;
        ZT_PROF_BEGIN(s, P_SCORE);
        if (absent_dev != nullptr) k_count_pairs<true><<<(unsigned)p.grid, WAVE * CN_WAVES, 0, s>>>(a);
        else k_count_pairs<false><<<(unsigned)p.grid, WAVE * CN_WAVES, 0, s>>>(a);
        ZT_LAUNCH_CHECK();
        ZT_PROF_END(s, P_SCORE);
    }
    return ZT_OK;
}
