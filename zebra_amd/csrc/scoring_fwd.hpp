// The link scorer's forward over 16 edges per workgroup, shared by the training scorer (scoring_train.hip: k_score_fwd, which
// keeps the hidden rows for its backward) and the eval scorer's generic tiled form (scoring.hip: k_affinity_gen_tiled, which
// does not).  One body, two instantiations: the sums have the same association in both.
#pragma once

#include "common.hpp"

namespace zt {

typedef float score_f32x4 __attribute__((ext_vector_type(4)));

// The widest hidden layer either scorer takes: 48 staged rows x (768 + 4) floats = 148 KB of the CU's 160 KB of LDS
constexpr int SCORE_MAX_H = 768;
constexpr int SCORE_WAVES = 16;
constexpr int SCORE_THREADS = 64 * SCORE_WAVES;

__host__ __device__ inline int score_round_up16(int x) { return (x + 15) / 16 * 16; }
inline bool score_width_ok(int H) { return H >= 4 && H <= SCORE_MAX_H && H % 4 == 0; }
// dynamic LDS of score_fwd_body: the staged rows [48][Hp + 4] and the waves' partial scores [16][2][16]
inline size_t score_fwd_lds(int H) { return ((size_t)48 * (score_round_up16(H) + 4) + SCORE_WAVES * 2 * 16) * 4; }

#if defined(__HIPCC__)

// U k-chunks of 16 of one N-tile of the forward: every weight load of the round issued before the first MFMA
template <int U>
__device__ __forceinline__ void fwd_chunks(int c, bool cok, int g4, int H, const float *__restrict__ wrow, const float *as_p,
                                           const float *ad_p, const float *an_p, score_f32x4 &au, score_f32x4 &ap, score_f32x4 &ang)
{
    const score_f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    score_f32x4 wa[U], wb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // H % 4 == 0: all four columns or none.  The load itself is unconditional, from a clamped address (no branch per load)
        const int k = 16 * (c + u) + 4 * g4;
        const bool kok = cok && k < H;
        const float *wk = wrow + (k < H ? k : H - 4);
        const score_f32x4 va = *reinterpret_cast<const score_f32x4 *>(wk), vb = *reinterpret_cast<const score_f32x4 *>(wk + H);
        wa[u] = kok ? va : zero4;
        wb[u] = kok ? vb : zero4;
    }
    __builtin_amdgcn_sched_barrier(0);                                   // (or the scheduler sinks every load to its first use)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const score_f32x4 as = *reinterpret_cast<const score_f32x4 *>(as_p + 16 * (c + u));
        const score_f32x4 ad = *reinterpret_cast<const score_f32x4 *>(ad_p + 16 * (c + u));
        const score_f32x4 an = *reinterpret_cast<const score_f32x4 *>(an_p + 16 * (c + u));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            au = __builtin_amdgcn_mfma_f32_16x16x4f32(as[j], wa[u][j], au, 0, 0, 0);
            ap = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[j], wb[u][j], ap, 0, 0, 0);
            ang = __builtin_amdgcn_mfma_f32_16x16x4f32(an[j], wb[u][j], ang, 0, 0, 0);
        }
    }
}

// A workgroup of sixteen waves owns the 16 edges from blockIdx.x * 16.  Their 48 embedding rows are staged in LDS once; wave w
// takes the N-tiles w, w + 16, ... of the hidden layer with three accumulators (W_a src, W_b dst, W_b neg), streams its 16 rows
// of fc1.weight (the module's own [H][2H]: W_a is columns [0, H) of a row, W_b columns [H, 2H)) from L2 as 16-byte vectors,
// applies bias and ReLU in the accumulator lanes and carries relu(.) x fc2.weight per lane.  The waves' partial scores meet in
// LDS and are added in wave order.  KEEP_HID: the hidden rows [2B][H] after the ReLU are written to `hid`.
template <bool KEEP_HID>
__device__ __forceinline__ void score_fwd_body(const float *__restrict__ emb, long long B, int H, const float *__restrict__ fc1_w,
                                               const float *__restrict__ fc1_b, const float *__restrict__ fc2_w,
                                               const float *__restrict__ fc2_b, float *__restrict__ prob, float *__restrict__ hid)
{
    extern __shared__ __attribute__((aligned(16))) char score_smem[];
    const int Hp = score_round_up16(H), ld = Hp + 4, NT = Hp / 16, h4 = H / 4, hp4 = Hp / 4;
    float *A = reinterpret_cast<float *>(score_smem);                    // [48][ld]: src rows, dst rows, neg rows of the tile
    float *part = A + 48 * ld;                                           // [16 waves][2][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const long long e0 = (long long)blockIdx.x * 16;
    const score_f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // ---- stage the 48 rows: zero beyond the batch and beyond H ----
    for (int f = tid; f < 48 * hp4; f += SCORE_THREADS) {
        const int row = f / hp4, c4 = f - row * hp4;
        const long long e = e0 + (row & 15);
        const bool ok = c4 < h4 && e < B;
        const score_f32x4 v = ok ? *reinterpret_cast<const score_f32x4 *>(emb + ((size_t)(row >> 4) * B + e) * H + 4 * c4) : zero4;
        *reinterpret_cast<score_f32x4 *>(A + row * ld + 4 * c4) = v;
    }
    __syncthreads();
    float sp[4] = {0.f, 0.f, 0.f, 0.f}, sn[4] = {0.f, 0.f, 0.f, 0.f};
    const float *as_p = A + r16 * ld + 4 * g4, *ad_p = as_p + 16 * ld, *an_p = ad_p + 16 * ld;
    for (int nt = wave; nt < NT; nt += SCORE_WAVES) {
        const int col = 16 * nt + r16;
        const bool cok = col < H;
        const float *wrow = fc1_w + (size_t)(cok ? col : 0) * 2 * H;
        score_f32x4 au = zero4, ap = zero4, ang = zero4;
        // four k-chunks a round: their eight weight loads are in flight together
        int c = 0;
        for (; c + 4 <= NT; c += 4) fwd_chunks<4>(c, cok, g4, H, wrow, as_p, ad_p, an_p, au, ap, ang);
        for (; c < NT; ++c) fwd_chunks<1>(c, cok, g4, H, wrow, as_p, ad_p, an_p, au, ap, ang);
        // lane (column col, edges 4 g4 + j): relu(fc1), kept where asked; x fc2's weight, carried per lane over this wave's N-tiles
        const float b1v = cok ? fc1_b[col] : 0.f, w2v = cok ? fc2_w[col] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float hp = au[j] + ap[j] + b1v, hn = au[j] + ang[j] + b1v;
            hp = hp > 0.f ? hp : 0.f;
            hn = hn > 0.f ? hn : 0.f;
            if constexpr (KEEP_HID) {
                const long long e = e0 + 4 * g4 + j;
                if (cok && e < B) {
                    hid[(size_t)e * H + col] = hp;
                    hid[(size_t)(B + e) * H + col] = hn;
                }
            }
            sp[j] += hp * w2v;
            sn[j] += hn * w2v;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x = sp[j], y = sn[j];
        x += dpp_f<0x128>(x); x += dpp_f<0x124>(x); x += dpp_f<0x122>(x); x += dpp_f<0x121>(x);
        y += dpp_f<0x128>(y); y += dpp_f<0x124>(y); y += dpp_f<0x122>(y); y += dpp_f<0x121>(y);
        if (r16 == 0) {                                                  // (lane 0 of the row: ITS association of the 16 terms)
            part[(wave * 2 + 0) * 16 + 4 * g4 + j] = x;
            part[(wave * 2 + 1) * 16 + 4 * g4 + j] = y;
        }
    }
    __syncthreads();
    if (tid < 32) {
        const int e = tid & 15, which = tid >> 4;
        float sc = part[which * 16 + e];
#pragma unroll
        for (int wv = 1; wv < SCORE_WAVES; ++wv) sc += part[(wv * 2 + which) * 16 + e];
        sc += fc2_b[0];
        if (e0 + e < B) prob[(size_t)which * B + e0 + e] = 1.f / (1.f + expf(-sc));
    }
}

#endif  // __HIPCC__

}  // namespace zt
