// Ranking a source against many candidates ("Read-only queries and ranking"):
//   zt_affinity_rank   prob[q][c] = sigmoid(fc2(relu(fc1([emb_q[q] | emb_c[idx[q][c]]])))) -- MergeLayer as
//                      compute_edge_probabilities applies it (model/tgn_model.py:185-188, utils/util.py:14-26) -- for Q x C
//                      pairs.  fc1 splits over its two halves, P_q = emb_q W_a^T and P_c = emb_c W_b^T (two launches of the f32
//                      MFMA GEMM of train_ops.hip into the workspace); what is left per pair is
//                          s = b2 + sum_h w2[h] relu((P_q[q][h] + b1[h]) + P_c[idx][h]),
//                      which is no GEMM (the relu sits inside the sum over h): k_rank_pairs.
//   zt_rank_metrics    rank of column 0 among the present candidates of each query, and MRR / Hits@1,3,10 sums.
//   zt_rank_metrics_counts  the same sums from counts taken elsewhere (rank_count.hip: above and equal over a whole pool).
#include "common.hpp"
#include "rank_pair.hpp"

using namespace zt;

namespace {

// One workgroup: RK_TQ queries x RK_TC candidate slots.  Wave w owns query q0 + w; each of its four 16-lane groups owns RK_NC
// slots.  The (P_q + b1) rows of the tile and w2 lie in LDS one chunk of RK_HC columns at a time; a lane walks the chunk in
// steps of 64 columns, its float4 of the query row and of w2 from LDS (the four groups of a wave read the same address: a
// broadcast) against one 16-byte vector of each of its candidates' rows from memory.  A pair's sum: lane l of its group adds
// columns 4l .. 4l + 3 of every 64 in ascending order into one accumulator, then the sixteen lanes are folded by xor 8, 4, 2, 1
// -- one association whatever the tile, no atomics: the same bits on every run.  The arithmetic is rank_pair.hpp's, shared with
// the top-K scorer (rank_topk.hip).
__global__ __launch_bounds__(WAVE * RK_TQ) void k_rank_pairs(const float *__restrict__ Pq, const float *__restrict__ Pc,
                                                             const int *__restrict__ cand_idx, long long Q, long long Nc,
                                                             long long C, int H, long long ctiles,
                                                             const float *__restrict__ b1, const float *__restrict__ w2,
                                                             const float *__restrict__ b2, float *__restrict__ prob, int *status)
{
    __shared__ float4 s_q[RK_TQ][RK_HC / 4];
    __shared__ float4 s_w[RK_HC / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, gl = lane & 15;
    const long long qt = blockIdx.x / ctiles, ct = blockIdx.x - qt * ctiles;
    const long long q0 = qt * RK_TQ, q = q0 + wave;
    const long long c0 = ct * RK_TC + grp * RK_NC;

    long long row[RK_NC];           // row of P_c, or -1: nothing to read (absent, out of range, beyond C or Q)
    bool bad = false;
#pragma unroll
    for (int j = 0; j < RK_NC; ++j) {
        const long long c = c0 + j;
        long long r = -1;
        if (q < Q && c < C) {
            r = cand_idx != nullptr ? (long long)cand_idx[q * C + c] : c;
            if (r < -1 || r >= Nc) { bad = true; r = -1; }
        }
        row[j] = r;
    }
    if (bad && gl == 0) atomicExch(status, (int)ZT_ERR_RANGE);

    float acc[RK_NC];
#pragma unroll
    for (int j = 0; j < RK_NC; ++j) acc[j] = 0.f;

    for (int h0 = 0; h0 < H; h0 += RK_HC) {
        const int hn = min(RK_HC, H - h0);                     // a multiple of 4
        if (h0 > 0) __syncthreads();                           // the chunk before has been read
        for (int v = tid; v < (RK_TQ + 1) * (hn / 4); v += WAVE * RK_TQ) {
            const int r = v / (hn / 4), c4 = v - r * (hn / 4);
            const float4 b = *reinterpret_cast<const float4 *>((r < RK_TQ ? b1 : w2) + h0 + 4 * c4);
            if (r == RK_TQ) { s_w[c4] = b; continue; }
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q0 + r < Q) p = *reinterpret_cast<const float4 *>(Pq + (q0 + r) * H + h0 + 4 * c4);
            s_q[r][c4] = rk_query_bias(p, b);
        }
        __syncthreads();
        for (int c4 = gl; c4 < hn / 4; c4 += RK_GROUP) {
            float4 pc[RK_NC];
#pragma unroll
            for (int j = 0; j < RK_NC; ++j) {
                pc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row[j] >= 0) pc[j] = *reinterpret_cast<const float4 *>(Pc + row[j] * H + h0 + 4 * c4);
            }
            const float4 pq = s_q[wave][c4], w = s_w[c4];
#pragma unroll
            for (int j = 0; j < RK_NC; ++j) acc[j] = rk_pair_step(acc[j], w, pq, pc[j]);
        }
    }
    const float bias2 = b2[0];
#pragma unroll
    for (int j = 0; j < RK_NC; ++j) {
        const float s = rk_fold16(acc[j]);
        const long long c = c0 + j;
        if (gl == 0 && q < Q && c < C) prob[q * C + c] = row[j] >= 0 ? rk_prob(s, bias2) : 0.f;
    }
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
    if (!rank_width_ok(H)) {
        set_error("zt_affinity_rank: H=%d unsupported (H %% 4 == 0 and %d <= H <= %d)", H, RANK_MIN_H, RANK_MAX_H);
        return ZT_ERR_UNSUPPORTED;
    }
    if (cand_idx_dev == nullptr && C != Nc) {
        set_error("zt_affinity_rank: without cand_idx every query takes all Nc=%lld candidates, C=%lld given", (long long)Nc,
                  (long long)C);
        return ZT_ERR_ARG;
    }
    if (Q == 0 || C == 0) return ZT_OK;
    if (!w->fc1_w || !w->fc1_b || !w->fc2_w || !w->fc2_b || ((uintptr_t)workspace_dev & 15) || ((uintptr_t)w->fc1_b & 15) ||
        ((uintptr_t)w->fc2_w & 15)) {
        set_error("zt_affinity_rank: NULL weight, or workspace / fc1 bias / fc2 weight not 16-byte aligned");
        return ZT_ERR_ARG;
    }
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
    // W_a = columns [0, H) of fc1.weight [H][2H], W_b = columns [H, 2H): the same matrix, a pointer offset, ldb = 2H
    int rc = zt_gemm_f32(emb_q_dev, w->fc1_w, Pq, Q, H, H, H, 2 * (int64_t)H, H, 0, 1, 0, stream);
    if (rc == ZT_OK) rc = zt_gemm_f32(emb_c_dev, w->fc1_w + H, Pc, Nc, H, H, H, 2 * (int64_t)H, H, 0, 1, 0, stream);
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
