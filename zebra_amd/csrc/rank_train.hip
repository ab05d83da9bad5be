// The one-vs-many scorer of a RANKING training step, forward and backward ("The scorer of a ranking step"):
//   z[q][c][h]  = (P_q[q][h] + b1[h]) + P_c[row(q, c)][h],   P_q = emb_q W_a^T,  P_c = emb_c W_b^T   (rank.hip's factoring)
//   logit[q][c] = b2 + sum_h w2[h] relu(z[q][c][h])
// zt_affinity_rank_train_forward writes the logits -- rank_walk.hpp's tile body (rk_tile_pairs) over rank_pair.hpp's pair sum,
// k_rank_pairs' too, so sigmoid(logit) computed as rk_prob computes it has the bits zt_affinity_rank writes -- and leaves P_q
// and P_c with the caller, who keeps them for the backward.  No buffer of Q C H elements exists on either side: the backward
// forms z and the ReLU mask again from P_q and P_c.
//
// Backward, from dl = d(loss)/d(logit) [Q][C]:
//   k_rank_bwd_q   one workgroup per RK_TQ queries and 64 columns of H: wave w owns query q0 + w, its four 16-lane groups take
//                  RK_NC candidates each per tile of RK_TC, tiles in ascending order, lane l of a group the columns 4l .. 4l + 3
//                  of the slab.  A lane carries four sums of dP_q[q][h] = sum_c dl w2[h] [z > 0] and four of
//                  d_fc2_w[h] = sum_c dl relu(z); the four groups are folded first to last, the d_fc2_w sums of the four waves
//                  first to last into row (query tile) of a partial matrix [q tiles][H] that zt_colsum_f32 adds up.
//                  sum dl per query tile goes the same way (slab 0 writes it).
//   k_rank_bwd_c   a wave per row r of emb_c and 256 columns: it walks the pairs that name r in ascending pair id q C + c --
//                  every q when there is no index, else the caller's transpose (row_ptr, pairs) -- and adds
//                  dP_c[r][h] = sum dl w2[h] [z > 0] into one accumulator per column.  A row nobody names is written as zeros.
//                  A pair id outside [0, Q C), a pair whose index is not r, or a row range outside the pair list sets the status
//                  word to ZT_ERR_RANGE and is left out: nothing is read or written out of bounds.
// then zt_colsum_f32 (d_fc1_b = colsum dP_q) and four zt_gemm_f32 with leading dimensions (d_emb_q = dP_q W_a, d_emb_c = dP_c W_b,
// d_fc1_w[:, :H] = dP_q^T emb_q, d_fc1_w[:, H:] = dP_c^T emb_c).  Every sum has one fixed association and there is no float
// atomic: two runs give the same bits.
#include "common.hpp"
#include "rank_walk.hpp"

using namespace zt;

namespace {

constexpr int RT_SLAB = 4 * RK_GROUP;        // 64 columns of H per workgroup of the query pass
constexpr int RT_CROWS = 4;                  // rows of emb_c per workgroup of the candidate pass (a wave each)
constexpr int RT_CCOLS = 4 * WAVE;           // 256 columns of H per workgroup of the candidate pass
constexpr int RT_CU = 8;                     // pairs of a row whose loads are in flight together

// rank_walk.hpp's tile body (rk_tile_pairs), k_rank_pairs' too (rank.hip); what is written is the logit, -inf for an absent pair
__global__ __launch_bounds__(WAVE * RK_TQ) void k_rank_train_fwd(const float *__restrict__ Pq, const float *__restrict__ Pc,
                                                                 const int *__restrict__ cand_idx, long long Q, long long Nc,
                                                                 long long C, int H, long long ctiles,
                                                                 const float *__restrict__ b1, const float *__restrict__ w2,
                                                                 const float *__restrict__ b2, float *__restrict__ logit, int *status)
{
    __shared__ RkTileLds s_t;
    rk_tile_pairs(s_t, Pq, Pc, cand_idx, Q, Nc, C, H, ctiles, b1, w2, b2, logit, status,
                  [](bool present, float s, float bias2) { return present ? rk_logit(s, bias2) : -INFINITY; });
}

// the values of the wave's four lane groups at this lane's place in its group, added first to last: every lane receives the sum
__device__ __forceinline__ float fold_groups(float v, int gl)
{
    const float g0 = __shfl(v, gl, WAVE), g1 = __shfl(v, gl + 16, WAVE), g2 = __shfl(v, gl + 32, WAVE), g3 = __shfl(v, gl + 48, WAVE);
    return ((g0 + g1) + g2) + g3;
}

// grid (q tiles, ceil(H / 64)).  part_w [q tiles][H], part_b [q tiles]; dPq [Q][H].
__global__ __launch_bounds__(WAVE * RK_TQ) void k_rank_bwd_q(const float *__restrict__ Pq, const float *__restrict__ Pc,
                                                             const int *__restrict__ cand_idx, const float *__restrict__ dl,
                                                             long long Q, long long Nc, long long C, int H,
                                                             const float *__restrict__ b1, const float *__restrict__ w2,
                                                             float *__restrict__ dPq, float *__restrict__ part_w,
                                                             float *__restrict__ part_b)
{
    __shared__ float s_w[RK_TQ][RT_SLAB];
    __shared__ float s_b[RK_TQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, gl = lane & 15;
    const long long qt = blockIdx.x, q = qt * RK_TQ + wave;
    const int col = (int)blockIdx.y * RT_SLAB + 4 * gl;
    const bool cok = col < H;                                  // H % 4 == 0: all four columns or none
    const bool qok = q < Q;
    float4 pq = make_float4(0.f, 0.f, 0.f, 0.f), w = pq;
    if (cok) {
        w = *reinterpret_cast<const float4 *>(w2 + col);
        if (qok) pq = rk_query_bias(*reinterpret_cast<const float4 *>(Pq + q * H + col), *reinterpret_cast<const float4 *>(b1 + col));
    }
    const float wv[4] = {w.x, w.y, w.z, w.w};
    float ap[4] = {0.f, 0.f, 0.f, 0.f}, aw[4] = {0.f, 0.f, 0.f, 0.f}, ab = 0.f;
    const long long ctiles = (C + RK_TC - 1) / RK_TC;
    for (long long ct = 0; ct < ctiles; ++ct) {                // candidates in ascending tiles
        const long long c0 = ct * RK_TC + grp * RK_NC;
        float d[RK_NC];
        float4 pc[RK_NC];
        bool live[RK_NC];
#pragma unroll
        for (int j = 0; j < RK_NC; ++j) {
            const long long c = c0 + j;
            long long r = -1;
            if (qok && c < C) {
                r = cand_idx != nullptr ? (long long)cand_idx[q * C + c] : c;
                if (r < -1 || r >= Nc) r = -1;                 // (the forward has reported it)
            }
            live[j] = r >= 0;
            d[j] = live[j] ? dl[q * C + c] : 0.f;
            pc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[j] && cok) pc[j] = *reinterpret_cast<const float4 *>(Pc + r * H + col);
        }
#pragma unroll
        for (int j = 0; j < RK_NC; ++j) {
            if (!live[j]) continue;
            float z[4];
            rk_pair_z(pq, pc[j], z);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (z[i] > 0.f) {
                    ap[i] = fmaf(d[j], wv[i], ap[i]);
                    aw[i] = fmaf(d[j], z[i], aw[i]);
                }
            ab += d[j];
        }
    }
    float tp[4], tw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tp[i] = fold_groups(ap[i], gl);
        tw[i] = fold_groups(aw[i], gl);
    }
    const float tb = fold_groups(ab, gl);
    if (grp == 0) {
        if (qok && cok) *reinterpret_cast<float4 *>(dPq + q * H + col) = make_float4(tp[0], tp[1], tp[2], tp[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) s_w[wave][4 * gl + i] = tw[i];
        if (gl == 0) s_b[wave] = tb;
    }
    __syncthreads();
    if (tid < RT_SLAB) {
        const int c = (int)blockIdx.y * RT_SLAB + tid;
        float t = s_w[0][tid];
#pragma unroll
        for (int k = 1; k < RK_TQ; ++k) t += s_w[k][tid];      // the waves first to last
        if (c < H) part_w[qt * H + c] = t;
    }
    if (tid == 0 && blockIdx.y == 0) {
        float t = s_b[0];
#pragma unroll
        for (int k = 1; k < RK_TQ; ++k) t += s_b[k];
        part_b[qt] = t;
    }
}

// grid (ceil(Nc / 4), ceil(H / 256)); a wave per row of emb_c.  cand_idx == NULL: row r is named by pair q C + r of every q.
__global__ __launch_bounds__(WAVE * RT_CROWS) void k_rank_bwd_c(const float *__restrict__ Pq, const float *__restrict__ Pc,
                                                                const int *__restrict__ cand_idx, const float *__restrict__ dl,
                                                                const long long *__restrict__ row_ptr, const int *__restrict__ pairs,
                                                                long long n_pairs, long long Q, long long Nc, long long C, int H,
                                                                const float *__restrict__ b1, const float *__restrict__ w2,
                                                                float *__restrict__ dPc, int *status)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * RT_CROWS + wave;
    if (r >= Nc) return;
    const int col = (int)blockIdx.y * RT_CCOLS + 4 * lane;
    const bool cok = col < H;
    float4 pc = make_float4(0.f, 0.f, 0.f, 0.f), w = pc, b = pc;
    if (cok) {
        pc = *reinterpret_cast<const float4 *>(Pc + r * H + col);
        w = *reinterpret_cast<const float4 *>(w2 + col);
        b = *reinterpret_cast<const float4 *>(b1 + col);
    }
    const float wv[4] = {w.x, w.y, w.z, w.w};
    bool bad = false;
    long long beg = 0, end = Q;
    if (cand_idx != nullptr) {
        beg = row_ptr[r];
        end = row_ptr[r + 1];
        if (beg < 0 || end < beg || end > n_pairs) { bad = true; end = beg = 0; }
    }
    const long long QC = Q * C;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long i0 = beg; i0 < end; i0 += RT_CU) {          // the pairs of the row in ascending pair id
        float d[RT_CU];
        float4 pq[RT_CU];
        bool live[RT_CU];
#pragma unroll
        for (int u = 0; u < RT_CU; ++u) {
            const long long i = i0 + u;
            live[u] = false;
            d[u] = 0.f;
            pq[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i >= end) continue;
            long long p, q;
            if (cand_idx != nullptr) {
                p = (long long)pairs[i];
                if (p < 0 || p >= QC || (long long)cand_idx[p] != r) { bad = true; continue; }
                q = p / C;
            } else {
                q = i;
                p = q * C + r;
            }
            live[u] = true;
            d[u] = dl[p];
            if (cok) pq[u] = rk_query_bias(*reinterpret_cast<const float4 *>(Pq + q * H + col), b);
        }
#pragma unroll
        for (int u = 0; u < RT_CU; ++u) {
            if (!live[u]) continue;
            float z[4];
            rk_pair_z(pq[u], pc, z);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (z[k] > 0.f) acc[k] = fmaf(d[u], wv[k], acc[k]);
        }
    }
    if (cok) *reinterpret_cast<float4 *>(dPc + r * H + col) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    if (bad && lane == 0) atomicExch(status, (int)ZT_ERR_RANGE);
}

struct RankTrainPlan { size_t off_dpq, off_dpc, off_pw, off_pb, total; };
void rt_plan(int64_t Q, int64_t Nc, int H, RankTrainPlan &p)
{
    size_t o = RK_HEAD;                                        // the status word
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t qtiles = (size_t)((Q + RK_TQ - 1) / RK_TQ);
    p.off_dpq = take((size_t)Q * H * 4);
    p.off_dpc = take((size_t)Nc * H * 4);
    p.off_pw = take(qtiles * H * 4);
    p.off_pb = take(qtiles * 4);
    p.total = o;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks the two calls share; ZT_OK with *empty set: nothing to do
int rt_check(const char *who, const float *emb_q, int64_t Q, const float *emb_c, int64_t Nc, const int32_t *cand_idx, int64_t C, int32_t H,
             const zt_affinity_weights *w, const void *ws, bool *empty)
{
    *empty = false;
    if (!emb_q || !emb_c || !w || !ws || Q < 0 || Nc < 0 || C < 0) {
        set_error("%s: bad argument", who);
        return ZT_ERR_ARG;
    }
    if (!rank_width_ok(H)) return rank_width_refused(who, H);
    if (cand_idx == nullptr && C != Nc) {
        set_error("%s: without cand_idx every query takes all Nc=%lld candidates, C=%lld given", who, (long long)Nc, (long long)C);
        return ZT_ERR_ARG;
    }
    if (Q == 0 || C == 0) {
        *empty = true;
        return ZT_OK;
    }
    if (!w->fc1_w || !w->fc1_b || !w->fc2_w || !w->fc2_b || !aligned16(ws) || !aligned16(w->fc1_w) || !aligned16(w->fc1_b) ||
        !aligned16(w->fc2_w) || !aligned16(emb_q) || !aligned16(emb_c)) {
        set_error("%s: NULL weight, or workspace / embeddings / fc1 / fc2 weight not 16-byte aligned", who);
        return ZT_ERR_ARG;
    }
    const long long ctiles = (C + RK_TC - 1) / RK_TC, qtiles = (Q + RK_TQ - 1) / RK_TQ;
    if (ctiles > 0x7fffffffll / qtiles || C > 0x7fffffffll / Q) {      // (a pair id is an int32)
        set_error("%s: Q=%lld x C=%lld pairs exceed one launch", who, (long long)Q, (long long)C);
        return ZT_ERR_UNSUPPORTED;
    }
    if ((Nc + RT_CROWS - 1) / RT_CROWS > 0x7fffffffll) {               // (the candidate pass: a wave per row of emb_c)
        set_error("%s: Nc=%lld rows exceed one launch", who, (long long)Nc);
        return ZT_ERR_UNSUPPORTED;
    }
    return ZT_OK;
}

}  // namespace

extern "C" int64_t zt_affinity_rank_train_workspace_bytes(int64_t Q, int64_t Nc, int64_t C, int32_t H)
{
    if (Q < 0 || Nc < 0 || C < 0 || !rank_width_ok(H)) return -1;
    RankTrainPlan p;
    rt_plan(Q, Nc, H, p);
    return (int64_t)p.total;
}

extern "C" int zt_affinity_rank_train_forward(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                                              const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w,
                                              float *logit_dev, float *pq_dev, float *pc_dev, void *workspace_dev, void *stream)
{
    const char *who = "zt_affinity_rank_train_forward";
    if (!logit_dev || !pq_dev || !pc_dev) {
        set_error("%s: bad argument", who);
        return ZT_ERR_ARG;
    }
    bool empty;
    int rc = rt_check(who, emb_q_dev, Q, emb_c_dev, Nc, cand_idx_dev, C, H, w, workspace_dev, &empty);
    if (rc != ZT_OK || empty) return rc;
    if (!aligned16(pq_dev) || !aligned16(pc_dev)) {
        set_error("%s: P_q / P_c not 16-byte aligned", who);
        return ZT_ERR_ARG;
    }
    const long long ctiles = (C + RK_TC - 1) / RK_TC, qtiles = (Q + RK_TQ - 1) / RK_TQ;
    hipStream_t s = (hipStream_t)stream;
    int *status = reinterpret_cast<int *>(workspace_dev);
    ZT_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    rc = rank_project(emb_q_dev, w, false, pq_dev, Q, H, stream);
    if (rc == ZT_OK) rc = rank_project(emb_c_dev, w, true, pc_dev, Nc, H, stream);
    if (rc != ZT_OK) return rc;
    ZT_PROF_BEGIN(s, P_SCORE);
    k_rank_train_fwd<<<(unsigned)(qtiles * ctiles), WAVE * RK_TQ, 0, s>>>(pq_dev, pc_dev, cand_idx_dev, Q, Nc, C, H, ctiles, w->fc1_b,
                                                                          w->fc2_w, w->fc2_b, logit_dev, status);
    ZT_LAUNCH_CHECK();
    ZT_PROF_END(s, P_SCORE);
    return ZT_OK;
}

extern "C" int zt_affinity_rank_train_backward(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                                               const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w,
                                               const float *pq_dev, const float *pc_dev, const float *dl_dev,
                                               const int64_t *row_ptr_dev, const int32_t *pairs_dev, int64_t n_pairs,
                                               float *d_emb_q_dev, float *d_emb_c_dev, float *d_fc1_w_dev, float *d_fc1_b_dev,
                                               float *d_fc2_w_dev, float *d_fc2_b_dev, void *workspace_dev, void *stream)
{
    const char *who = "zt_affinity_rank_train_backward";
    if (!pq_dev || !pc_dev || !dl_dev || n_pairs < 0 || (cand_idx_dev != nullptr && (!row_ptr_dev || (n_pairs > 0 && !pairs_dev)))) {
        set_error("%s: bad argument (P_q, P_c, dl and, with cand_idx, its transpose expected)", who);
        return ZT_ERR_ARG;
    }
    bool empty;
    int rc = rt_check(who, emb_q_dev, Q, emb_c_dev, Nc, cand_idx_dev, C, H, w, workspace_dev, &empty);
    if (rc != ZT_OK || empty) return rc;
    if (!aligned16(pq_dev) || !aligned16(pc_dev) || !aligned16(d_emb_q_dev) || !aligned16(d_emb_c_dev) || !aligned16(d_fc1_w_dev)) {
        set_error("%s: P_q / P_c / d_emb / d_fc1_w not 16-byte aligned", who);
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    RankTrainPlan p;
    rt_plan(Q, Nc, H, p);
    char *ws = reinterpret_cast<char *>(workspace_dev);
    int *status = reinterpret_cast<int *>(ws);
    float *dPq = reinterpret_cast<float *>(ws + p.off_dpq), *dPc = reinterpret_cast<float *>(ws + p.off_dpc);
    float *part_w = reinterpret_cast<float *>(ws + p.off_pw), *part_b = reinterpret_cast<float *>(ws + p.off_pb);
    const long long qtiles = (Q + RK_TQ - 1) / RK_TQ;
    const int64_t H2 = 2 * (int64_t)H;
    ZT_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    const bool need_c = d_emb_c_dev != nullptr || d_fc1_w_dev != nullptr;
    const bool need_q = d_emb_q_dev != nullptr || d_fc1_w_dev != nullptr || d_fc1_b_dev != nullptr || d_fc2_w_dev != nullptr ||
                        d_fc2_b_dev != nullptr;
    ZT_PROF_BEGIN(s, P_SCORE);
    if (need_q) {
        const dim3 grid((unsigned)qtiles, (unsigned)((H + RT_SLAB - 1) / RT_SLAB));
        k_rank_bwd_q<<<grid, WAVE * RK_TQ, 0, s>>>(pq_dev, pc_dev, cand_idx_dev, dl_dev, Q, Nc, C, H, w->fc1_b, w->fc2_w, dPq, part_w, part_b);
    }
    if (need_c) {
        const dim3 grid((unsigned)((Nc + RT_CROWS - 1) / RT_CROWS), (unsigned)((H + RT_CCOLS - 1) / RT_CCOLS));
        k_rank_bwd_c<<<grid, WAVE * RT_CROWS, 0, s>>>(pq_dev, pc_dev, cand_idx_dev, dl_dev, reinterpret_cast<const long long *>(row_ptr_dev),
                                                      pairs_dev, n_pairs, Q, Nc, C, H, w->fc1_b, w->fc2_w, dPc, status);
    }
    ZT_LAUNCH_CHECK();
    ZT_PROF_END(s, P_SCORE);
    if (d_fc2_w_dev) rc = zt_colsum_f32(part_w, qtiles, H, H, d_fc2_w_dev, 0, stream);
    if (rc == ZT_OK && d_fc2_b_dev) rc = zt_colsum_f32(part_b, qtiles, 1, 1, d_fc2_b_dev, 0, stream);
    if (rc == ZT_OK && d_fc1_b_dev) rc = zt_colsum_f32(dPq, Q, H, H, d_fc1_b_dev, 0, stream);
    if (rc == ZT_OK && d_emb_q_dev) rc = zt_gemm_f32(dPq, w->fc1_w, d_emb_q_dev, Q, H, H, H, H2, H, 0, 0, 0, stream);
    if (rc == ZT_OK && d_emb_c_dev) rc = zt_gemm_f32(dPc, w->fc1_w + H, d_emb_c_dev, Nc, H, H, H, H2, H, 0, 0, 0, stream);
    if (rc == ZT_OK && d_fc1_w_dev) rc = zt_gemm_f32(dPq, emb_q_dev, d_fc1_w_dev, H, H, Q, H, H, H2, 1, 0, 0, stream);
    if (rc == ZT_OK && d_fc1_w_dev) rc = zt_gemm_f32(dPc, emb_c_dev, d_fc1_w_dev + H, H, H, Nc, H, H, H2, 1, 0, 0, stream);
    return rc;
}
