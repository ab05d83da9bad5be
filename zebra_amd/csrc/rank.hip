// Ranking a source against many candidates ("Read-only queries and ranking"):
//   zt_affinity_rank   prob[q][c] = sigmoid(fc2(relu(fc1([emb_q[q] | emb_c[idx[q][c]]])))) -- MergeLayer as
//                      compute_edge_probabilities applies it (model/tgn_model.py:185-188, utils/util.py:14-26) -- for Q x C
//                      pairs.  fc1 splits over its two halves, P_q = emb_q W_a^T and P_c = emb_c W_b^T (two launches of the f32
//                      MFMA GEMM of train_ops.hip into the workspace); what is left per pair is
//                          s = b2 + sum_h w2[h] relu((P_q[q][h] + b1[h]) + P_c[idx][h]),
//                      which is no GEMM (the relu sits inside the sum over h): k_rank_pairs, whose body -- tiling, rows, pair
//                      sum -- is rank_walk.hpp's rk_tile_pairs.
//   zt_rank_metrics    rank of column 0 among the present candidates of each query, and MRR / Hits@1,3,10 sums.
//   zt_rank_metrics_counts  the same sums from counts taken elsewhere (rank_count.hip: above and equal over a whole pool).
#include "common.hpp"
#include "rank_walk.hpp"

using namespace zt;

namespace {

// rank_walk.hpp's tile body (rk_tile_pairs: the tiling, the rows, the pair sum and its fold); what is written is the probability,
// 0 for an absent pair
__global__ __launch_bounds__(WAVE * RK_TQ) void k_rank_pairs(const float *__restrict__ Pq, const float *__restrict__ Pc,
                                                             const int *__restrict__ cand_idx, long long Q, long long Nc,
                                                             long long C, int H, long long ctiles,
                                                             const float *__restrict__ b1, const float *__restrict__ w2,
                                                             const float *__restrict__ b2, float *__restrict__ prob, int *status)
{
    __shared__ RkTileLds s_t;
    rk_tile_pairs(s_t, Pq, Pc, cand_idx, Q, Nc, C, H, ctiles, b1, w2, b2, prob, status,
                  [](bool present, float s, float bias2) { return present ? rk_prob(s, bias2) : 0.f; });
}

// One workgroup of sixteen waves.  A wave takes one query at a time and counts, over the present candidates c >= 1, those above
// and those equal to column 0 (integers: exact); the ranks of 1024 queries go to LDS, then ONE lane adds them to the five
// running sums first to last in float64 -- the sums start from acc's own values, so a pass accumulates over its batches in one
// fixed order.
constexpr int RM_WAVES = 16, RM_CHUNK = 1024;
__global__ __launch_bounds__(WAVE * RM_WAVES) void k_rank_metrics(const float *__restrict__ prob, const int *__restrict__ cand_idx,
                                                                  long long Q, long long C, float *__restrict__ rank_out,
                                                                  double *__restrict__ acc)
{
    __shared__ float s_rank[RM_CHUNK];          // 0: the query is skipped (its positive is absent)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x == 0)
        for (int i = 0; i < 5; ++i) sum[i] = acc[i];
    for (long long qc = 0; qc < Q; qc += RM_CHUNK) {
        const int nq = (int)min((long long)RM_CHUNK, Q - qc);
        for (int qi = wave; qi < nq; qi += RM_WAVES) {
            const long long q = qc + qi;
            const float *p = prob + q * C;
            const int *ix = cand_idx != nullptr ? cand_idx + q * C : nullptr;
            float rank = 0.f;
            if (ix == nullptr || ix[0] >= 0) {
                const float p0 = p[0];
                int gt = 0, eq = 0;
                for (long long cb = 1; cb < C; cb += WAVE) {          // (wave-uniform bounds: every lane takes every ballot)
                    const long long c = cb + lane;
                    const bool live = c < C && (ix == nullptr || ix[c] >= 0);
                    const float v = live ? p[c] : 0.f;
                    gt += __popcll(__ballot(live && v > p0));
                    eq += __popcll(__ballot(live && v == p0));
                }
                rank = 1.f + (float)gt + 0.5f * (float)eq;
            }
            if (lane == 0) {
                s_rank[qi] = rank;
                if (rank_out != nullptr) rank_out[q] = rank;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int qi = 0; qi < nq; ++qi) {
                const float r = s_rank[qi];
                if (r == 0.f) continue;
                sum[0] += 1.0 / (double)r;
                sum[1] += r <= 1.f ? 1.0 : 0.0;
                sum[2] += r <= 3.f ? 1.0 : 0.0;
                sum[3] += r <= 10.f ? 1.0 : 0.0;
                sum[4] += 1.0;
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int i = 0; i < 5; ++i) acc[i] = sum[i];
}

// k_rank_metrics' sums from counts: rank = 1 + above + 0.5 equal in float64 (a pool of ten million ids does not fit a float32
// rank; below 2^23 the rank, its reciprocal and the compares are the ones k_rank_metrics forms from its float32 rank), 0 for
// a query whose threshold is NaN.  One workgroup, a query per thread and chunk; ONE lane adds first to last.
__global__ __launch_bounds__(RM_CHUNK) void k_rank_metrics_counts(const float *__restrict__ thr, const int *__restrict__ above,
                                                                  const int *__restrict__ equal, long long Q,
                                                                  double *__restrict__ rank_out, double *__restrict__ acc)
{
    __shared__ double s_rank[RM_CHUNK];         // 0: the query is skipped
    double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x == 0)
        for (int i = 0; i < 5; ++i) sum[i] = acc[i];
    for (long long qc = 0; qc < Q; qc += RM_CHUNK) {
        const int nq = (int)min((long long)RM_CHUNK, Q - qc);
        if ((int)threadIdx.x < nq) {
            const long long q = qc + threadIdx.x;
            const float t = thr[q];
            const double rank = t == t ? 1.0 + (double)above[q] + 0.5 * (double)equal[q] : 0.0;
            s_rank[threadIdx.x] = rank;
            if (rank_out != nullptr) rank_out[q] = rank;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int qi = 0; qi < nq; ++qi) {
                const double r = s_rank[qi];
                if (r == 0.0) continue;
                sum[0] += 1.0 / r;
                sum[1] += r <= 1.0 ? 1.0 : 0.0;
                sum[2] += r <= 3.0 ? 1.0 : 0.0;
                sum[3] += r <= 10.0 ? 1.0 : 0.0;
                sum[4] += 1.0;
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int i = 0; i < 5; ++i) acc[i] = sum[i];
}

}  // namespace

extern "C" int64_t zt_affinity_rank_workspace_bytes(int64_t Q, int64_t Nc, int32_t H)
{
    if (Q < 0 || Nc < 0 || !rank_width_ok(H)) return -1;
    return (int64_t)RK_HEAD + (Q + Nc) * (int64_t)H * 4;
}

extern "C" int zt_affinity_rank(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                                const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w,
                                float *prob_dev, void *workspace_dev, void *stream)
{
    if (!emb_q_dev || !emb_c_dev || !w || !prob_dev || !workspace_dev || Q < 0 || Nc < 0 || C < 0) {
        set_error("zt_affinity_rank: bad argument");
        return ZT_ERR_ARG;
    }
    if (!rank_width_ok(H)) return rank_width_refused("zt_affinity_rank", H);
    if (cand_idx_dev == nullptr && C != Nc) {
        set_error("zt_affinity_rank: without cand_idx every query takes all Nc=%lld candidates, C=%lld given", (long long)Nc,
                  (long long)C);
        return ZT_ERR_ARG;
    }
    if (Q == 0 || C == 0) return ZT_OK;
    if (!rank_weights_ok("zt_affinity_rank", w, workspace_dev)) return ZT_ERR_ARG;
    const long long ctiles = (C + RK_TC - 1) / RK_TC, qtiles = (Q + RK_TQ - 1) / RK_TQ;
    if (ctiles > 0x7fffffffll / qtiles) {
        set_error("zt_affinity_rank: Q=%lld x C=%lld pairs exceed one launch", (long long)Q, (long long)C);
        return ZT_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace_dev);
    int *status = reinterpret_cast<int *>(ws);
    float *Pq = reinterpret_cast<float *>(ws + RK_HEAD), *Pc = Pq + Q * (int64_t)H;
    ZT_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    int rc = rank_project(emb_q_dev, w, false, Pq, Q, H, stream);
    if (rc == ZT_OK) rc = rank_project(emb_c_dev, w, true, Pc, Nc, H, stream);
    if (rc != ZT_OK) return rc;
    ZT_PROF_BEGIN(s, P_SCORE);
    k_rank_pairs<<<(unsigned)(qtiles * ctiles), WAVE * RK_TQ, 0, s>>>(Pq, Pc, cand_idx_dev, Q, Nc, C, H, ctiles, w->fc1_b, w->fc2_w,
                                                                      w->fc2_b, prob_dev, status);
    ZT_LAUNCH_CHECK();
    ZT_PROF_END(s, P_SCORE);
    return ZT_OK;
}

extern "C" int zt_rank_metrics(const float *prob_dev, const int32_t *cand_idx_dev, int64_t Q, int64_t C, float *rank_dev,
                               double *acc_dev, void *stream)
{
    if (!prob_dev || !acc_dev || Q < 0 || C < 0) {
        set_error("zt_rank_metrics: bad argument");
        return ZT_ERR_ARG;
    }
    if (Q == 0 || C == 0) return ZT_OK;
    k_rank_metrics<<<1, WAVE * RM_WAVES, 0, (hipStream_t)stream>>>(prob_dev, cand_idx_dev, Q, C, rank_dev, acc_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_rank_metrics_counts(const float *thr_dev, const int32_t *above_dev, const int32_t *equal_dev, int64_t Q,
                                      double *rank_dev, double *acc_dev, void *stream)
{
    if (!thr_dev || !above_dev || !equal_dev || !acc_dev || Q < 0) {
        set_error("zt_rank_metrics_counts: bad argument");
        return ZT_ERR_ARG;
    }
    if (Q == 0) return ZT_OK;
    k_rank_metrics_counts<<<1, RM_CHUNK, 0, (hipStream_t)stream>>>(thr_dev, above_dev, equal_dev, Q, rank_dev, acc_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
