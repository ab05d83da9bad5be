// The pair sum of the one-vs-many scorers, in ONE place so that all give a pair the same bits (the walks around it, and so its
// two call sites, are rank_walk.hpp's: the tile body of rank.hip / rank_train.hip, the span walk of rank_topk.hip / rank_count.hip):
//   s = b2 + sum_h w2[h] relu((P_q[q][h] + b1[h]) + P_c[row][h]),  prob = 1 / (1 + expf(-s)).
// Sixteen lanes share a pair.  Lane l of the group adds columns 4l .. 4l + 3 of every 64 in ascending order into one
// accumulator (rk_pair_step, one call per 64 columns), then the sixteen are folded by xor 8, 4, 2, 1 (rk_fold16, or rk_fold16x8
// for eight pairs at once).  P_q + b1 is formed once per query row (rk_query_bias) and P_c added to it -- that order.
#pragma once

#include "common.hpp"

namespace zt {

constexpr int RANK_MIN_H = 4, RANK_MAX_H = 4352;   // 256 x 17: the widest hidden layer D <= 256 and 16 models give
constexpr int RK_TQ = 4;            // query rows per workgroup
constexpr int RK_GROUP = 16;        // lanes that share one pair: 16 x float4 = 64 consecutive h per step
constexpr int RK_NC = 8;            // candidates per lane group, their loads in flight together
constexpr int RK_TC = (WAVE / RK_GROUP) * RK_NC;   // 32 candidates per wave and step
constexpr int RK_HC = 1024;         // h per chunk: (RK_TQ + 1) x 4 KB of LDS
constexpr size_t RK_HEAD = 256;     // bytes in front of P_q in the workspace: the status word

inline bool rank_width_ok(int H) { return H >= RANK_MIN_H && H <= RANK_MAX_H && H % 4 == 0; }

#if defined(__HIPCC__)

// (P_q + b1) of four columns: what lies in LDS for a query row
__device__ __forceinline__ float4 rk_query_bias(const float4 p, const float4 b)
{
    return make_float4(p.x + b.x, p.y + b.y, p.z + b.z, p.w + b.w);
}

// four columns of one pair into its accumulator, in ascending order
__device__ __forceinline__ float rk_pair_step(float acc, const float4 w, const float4 pq, const float4 pc)
{
    acc = fmaf(w.x, fmaxf(pq.x + pc.x, 0.f), acc);
    acc = fmaf(w.y, fmaxf(pq.y + pc.y, 0.f), acc);
    acc = fmaf(w.z, fmaxf(pq.z + pc.z, 0.f), acc);
    acc = fmaf(w.w, fmaxf(pq.w + pc.w, 0.f), acc);
    return acc;
}

// the sixteen accumulators of a pair folded: every lane of the group receives the sum
__device__ __forceinline__ float rk_fold16(float s)
{
    s += __shfl_xor(s, 8, WAVE);
    s += __shfl_xor(s, 4, WAVE);
    s += __shfl_xor(s, 2, WAVE);
    s += __shfl_xor(s, 1, WAVE);
    return s;
}

// rk_fold16 of RK_NC = 8 pairs with a quarter of the shuffles: at every level a lane keeps the half of the pairs its bit of
// the level names and hands the other half over, so each sum is still own + partner's, level by level -- the bits of rk_fold16.
// Lane gl of the group ends with the sum of pair rk_fold_pair(gl) (both lanes of an xor-1 couple hold it).
__device__ __forceinline__ int rk_fold_pair(int gl) { return ((gl >> 3) & 1) * 4 + ((gl >> 2) & 1) * 2 + ((gl >> 1) & 1); }
__device__ __forceinline__ float rk_fold16x8(const float (&acc)[RK_NC], int gl)
{
    const bool b3 = gl & 8, b2 = gl & 4, b1 = gl & 2;
    float a4[4], a2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float keep = b3 ? acc[i + 4] : acc[i], send = b3 ? acc[i] : acc[i + 4];
        a4[i] = keep + __shfl_xor(send, 8, WAVE);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float keep = b2 ? a4[i + 2] : a4[i], send = b2 ? a4[i] : a4[i + 2];
        a2[i] = keep + __shfl_xor(send, 4, WAVE);
    }
    const float keep = b1 ? a2[1] : a2[0], send = b1 ? a2[0] : a2[1];
    float s = keep + __shfl_xor(send, 2, WAVE);
    s += __shfl_xor(s, 1, WAVE);
    return s;
}

__device__ __forceinline__ float rk_prob(float s, float bias2) { return 1.f / (1.f + expf(-(s + bias2))); }

// the logit rk_prob takes the sigmoid of (rank_train.hip writes it): 1 / (1 + expf(-rk_logit(s, b))) has rk_prob(s, b)'s bits
__device__ __forceinline__ float rk_logit(float s, float bias2) { return s + bias2; }

// z of four columns of one pair, formed as rk_pair_step forms it: the backward's ReLU mask is the forward's
__device__ __forceinline__ void rk_pair_z(const float4 pq, const float4 pc, float (&z)[4])
{
    z[0] = pq.x + pc.x;
    z[1] = pq.y + pc.y;
    z[2] = pq.z + pc.z;
    z[3] = pq.w + pc.w;
}

#endif  // __HIPCC__

}  // namespace zt
