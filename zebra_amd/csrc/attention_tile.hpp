// The row tile of TemporalAttentionLayer shared by the eval forward (attention.hip) and the training pair
// (attention_train.hip): the LDS carve-up, the staging of a tile's inputs, the LDS-to-LDS linear layer on exact-f32 MFMA
// and the forward body itself.  attention_forward_tile<false> IS the eval kernel; <true> adds the dropout scale on the
// softmax weights and the stores of what the backward reads -- nothing else differs, so with drop_p = 0 the two give the
// same bits.
//
// attn_w is the head mean of the weights AFTER dropout: nn.MultiheadAttention applies dropout to the softmax output and
// returns that tensor when need_weights is set (torch/nn/functional.py, multi_head_attention_forward: softmax, then
// `if dropout_p > 0.0: attn_output_weights = dropout(attn_output_weights, p=dropout_p)`, then the bmm with v, and for
// average_attn_weights `attn_output_weights.mean(dim=1)` of that same tensor).
#pragma once
#include "common.hpp"

namespace zt {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ATT_THREADS = 256;
constexpr int ATT_WAVES = 4;
constexpr int ATT_MAX_MT = 5;

__host__ __device__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

__global__ void k_pad_w(const float *__restrict__ W, int rows, int cols, int ld_src, int col0, float *__restrict__ Wp,
                        int rows_p, int cols_p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_p * cols_p) return;
    const int r = i / cols_p, c = i % cols_p;
    Wp[i] = (r < rows && c < cols) ? W[(size_t)r * ld_src + col0 + c] : 0.f;
}

// Y[g][col] = act((sum_i X[g][i] * Wp[col][i] + bias[col]) * scale), g < mt*16, col < NT*16 (zero for
// col >= n_out).  X, Y in LDS; Wp zero-padded [NT*16][Kp] in global (L2); wave w owns N-tiles w, w+4, ...
__device__ inline void lds_linear(const float *X, int ldx, int mt, const float *__restrict__ Wp, int Kp, int n_out,
                                  int NT, const float *__restrict__ bias, float scale, bool relu, float *Y, int ldy)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    for (int nt = wave; nt < NT; nt += ATT_WAVES) {
        f32x4 acc[ATT_MAX_MT];
#pragma unroll
        for (int a = 0; a < ATT_MAX_MT; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *bp = Wp + (size_t)(nt * 16 + r16) * Kp + 4 * g4;
        for (int kc = 0; kc < Kp / 16; ++kc) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bp + 16 * kc);
#pragma unroll
            for (int a = 0; a < ATT_MAX_MT; ++a) {
                if (a < mt) {
                    const f32x4 av = *reinterpret_cast<const f32x4 *>(X + (size_t)(a * 16 + r16) * ldx + 16 * kc + 4 * g4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc[a], 0, 0, 0);
                }
            }
        }
        const int col = nt * 16 + r16;
        const float b = (col < n_out && bias) ? bias[col] : 0.f;
#pragma unroll
        for (int a = 0; a < ATT_MAX_MT; ++a) {
            if (a < mt) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = (acc[a][j] + b) * scale;
                    if (relu) v = v > 0.f ? v : 0.f;
                    Y[(size_t)(a * 16 + g4 * 4 + j) * ldy + col] = col < n_out ? v : 0.f;
                }
            }
        }
    }
}

// One workgroup's dynamic LDS (zt::attention_plan sizes it)
struct AttnLds {
    float *A;      // [rows_p][lda]   key rows
    float *KV;     // [rows_p][ldk]   projected K, then V
    float *Xq;     // [16][ldq]       query rows / attention output
    float *Qp;     // [16][ldq]       projected, scaled queries; later scratch
    float *Z;      // [16][ldq]       = KV: [attn_out | src] for the merger (K/V are dead by then)
    float *sc;     // [rows_p][heads] scores -> softmax weights
    int *inv;      // [16]            row has no real neighbour
};

__device__ inline AttnLds attn_carve(char *smem, const AttnDims &d)
{
    const int rows_p = d.mt * 16;
    AttnLds l;
    l.A = reinterpret_cast<float *>(smem);
    l.KV = l.A + (size_t)rows_p * d.lda;
    const size_t kv_words = (size_t)rows_p * d.ldk > (size_t)16 * d.ldq ? (size_t)rows_p * d.ldk : (size_t)16 * d.ldq;
    l.Xq = l.KV + kv_words;
    l.Qp = l.Xq + 16 * d.ldq;
    l.Z = l.KV;
    l.sc = l.Qp + 16 * d.ldq;
    l.inv = reinterpret_cast<int *>(l.sc + rows_p * 4);
    return l;
}

// inv, the tile's key rows [nbr | edge | nbr_time] and its query rows [src | src_time], zero-padded; ends with a barrier.
// The three key arrays are read in place: the concatenation exists in LDS only.
__device__ inline void attn_stage(const AttnDims &d, const AttnLds &l, long long q0, int nq, const float *__restrict__ src,
                                  const float *__restrict__ src_t, const float *__restrict__ nf, const float *__restrict__ ef,
                                  const float *__restrict__ ntf, const unsigned char *__restrict__ mask)
{
    const int tid = threadIdx.x;
    const int rows_p = d.mt * 16, nrow = nq * d.k, k = d.k;
    if (tid < 16) {
        int all = 1;
        if (tid < nq) for (int j = 0; j < k; ++j) all &= mask[(q0 + tid) * k + j] ? 1 : 0;
        l.inv[tid] = (tid < nq) ? all : 1;
    }
    for (int f = tid; f < rows_p * d.lda; f += ATT_THREADS) {
        const int g = f / d.lda, c = f - g * d.lda;
        float v = 0.f;
        if (g < nrow) {
            const size_t row = (size_t)q0 * k + g;
            if (c < d.D) v = nf[row * d.D + c];
            else if (c < d.D + d.F) v = ef[row * d.F + (c - d.D)];
            else if (c < d.Ek) v = ntf[row * d.T + (c - d.D - d.F)];
        }
        l.A[f] = v;
    }
    for (int f = tid; f < 16 * d.ldq; f += ATT_THREADS) {
        const int q = f / d.ldq, c = f - q * d.ldq;
        float v = 0.f;
        if (q < nq) {
            if (c < d.D) v = src[(q0 + q) * d.D + c];
            else if (c < d.E) v = src_t[(q0 + q) * d.T + (c - d.D)];
        }
        l.Xq[f] = v;
    }
    __syncthreads();
}

// The hashed keep-mask of the softmax weights (common.hpp drop_scale at element (n * heads + h) * k + j) and the arrays
// the training forward keeps for the backward; all unused by the eval kernel.
struct AttnDrop {
    unsigned lo, hi, thr;
    float inv_keep;
};
struct AttnSaved {
    float *p;      // [N][k][heads]  softmax weights before dropout
    float *o;      // [N][E]         concatenated heads, before out_proj
    float *y;      // [N][E]         out_proj's output, zero for rows without neighbours
    float *hid;    // [N][hidden]    relu(merger.fc1)
};

__device__ inline float attn_keep(const AttnDrop &dr, const AttnDims &d, long long n, int h, int j)
{
    return drop_scale(dr.lo, dr.hi, dr.thr, dr.inv_keep, ((unsigned long long)n * d.heads + h) * d.k + j);
}

template <bool TRAIN>
__device__ inline void attention_forward_tile(
    char *smem, const AttnDims &d, long long N, const float *__restrict__ src, const float *__restrict__ src_t,
    const float *__restrict__ nf, const float *__restrict__ ef, const float *__restrict__ ntf,
    const unsigned char *__restrict__ mask, const float *__restrict__ Wq, const float *__restrict__ Wk,
    const float *__restrict__ Wv, const float *__restrict__ in_b, const float *__restrict__ Wo,
    const float *__restrict__ out_b, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, float *__restrict__ out, float *__restrict__ attn_w,
    const AttnDrop &dr, const AttnSaved &sv)
{
    const int tid = threadIdx.x;
    const int rows_p = d.mt * 16;
    const AttnLds l = attn_carve(smem, d);
    float *A = l.A, *KV = l.KV, *Xq = l.Xq, *Qp = l.Qp, *Z = l.Z, *sc = l.sc;
    int *inv = l.inv;
    const long long q0 = (long long)blockIdx.x * d.rq;
    const int nq = (int)((N - q0) < d.rq ? (N - q0) : d.rq);
    const int nrow = nq * d.k;
    const int k = d.k, E = d.E;

    // ---- stage inputs ----
    attn_stage(d, l, q0, nq, src, src_t, nf, ef, ntf, mask);
    // ---- q = (Wq x + bq) / sqrt(head_dim);  K = Wk key + bk ----
    lds_linear(Xq, d.ldq, 1, Wq, d.Ep, E, d.Ep / 16, in_b, rsqrtf((float)d.hd), false, Qp, d.ldq);
    lds_linear(A, d.lda, d.mt, Wk, d.Ekp, E, d.Ep / 16, in_b + E, 1.f, false, KV, d.ldk);
    __syncthreads();
    // ---- scores, key-padding mask, softmax over the neighbours ----
    for (int f = tid; f < rows_p * d.heads; f += ATT_THREADS) {
        const int g = f / d.heads, h = f - g * d.heads;
        float s = -INFINITY;
        if (g < nrow) {
            const int q = g / k, j = g - q * k;
            const bool masked = mask[(q0 + q) * k + j] != 0 && !(inv[q] && j == 0);
            if (!masked) {
                s = 0.f;
                const float *qr = Qp + (size_t)q * d.ldq + h * d.hd, *kr = KV + (size_t)g * d.ldk + h * d.hd;
                for (int c = 0; c < d.hd; ++c) s += qr[c] * kr[c];
            }
        }
        sc[f] = s;
    }
    __syncthreads();
    for (int f = tid; f < nq * d.heads; f += ATT_THREADS) {
        const int q = f / d.heads, h = f - q * d.heads;
        float mx = -INFINITY;
        for (int j = 0; j < k; ++j) mx = fmaxf(mx, sc[(q * k + j) * d.heads + h]);
        float sum = 0.f;
        for (int j = 0; j < k; ++j) sum += expf(sc[(q * k + j) * d.heads + h] - mx);
        for (int j = 0; j < k; ++j) sc[(q * k + j) * d.heads + h] = expf(sc[(q * k + j) * d.heads + h] - mx) / sum;
    }
    __syncthreads();
    if constexpr (TRAIN) {
        // keep p for the backward, then p~ = p * m in place (m = 1 exactly without dropout)
        for (int f = tid; f < nrow * d.heads; f += ATT_THREADS) {
            const int g = f / d.heads, h = f - g * d.heads;
            const int q = g / k, j = g - q * k;
            const float p = sc[f];
            sv.p[(size_t)q0 * k * d.heads + f] = p;
            sc[f] = p * attn_keep(dr, d, q0 + q, h, j);
        }
        __syncthreads();
    }
    // attention weights averaged over heads, zero for rows without neighbours (:60-63)
    for (int f = tid; f < nrow; f += ATT_THREADS) {
        const int q = f / k;
        float a = 0.f;
        for (int h = 0; h < d.heads; ++h) a += sc[f * d.heads + h];
        attn_w[(size_t)q0 * k + f] = inv[q] ? 0.f : a / (float)d.heads;
    }
    // ---- V = Wv key + bv (overwrites K), weighted sum over the neighbours ----
    lds_linear(A, d.lda, d.mt, Wv, d.Ekp, E, d.Ep / 16, in_b + 2 * E, 1.f, false, KV, d.ldk);
    __syncthreads();
    for (int f = tid; f < 16 * d.ldq; f += ATT_THREADS) {
        const int q = f / d.ldq, c = f - q * d.ldq;
        float v = 0.f;
        if (q < nq && c < E) {
            const int h = c / d.hd;
            for (int j = 0; j < k; ++j) v += sc[(q * k + j) * d.heads + h] * KV[(size_t)(q * k + j) * d.ldk + c];
            if constexpr (TRAIN) sv.o[(size_t)(q0 + q) * E + c] = v;
        }
        Xq[f] = v;
    }
    __syncthreads();
    // ---- out_proj, zero rows without neighbours, merger([attn_out | src]) ----
    lds_linear(Xq, d.ldq, 1, Wo, d.Ep, E, d.Ep / 16, out_b, 1.f, false, Qp, d.ldq);
    __syncthreads();
    for (int f = tid; f < 16 * d.ldq; f += ATT_THREADS) {
        const int q = f / d.ldq, c = f - q * d.ldq;
        float v = 0.f;
        if (q < nq) {
            if (c < E) {
                v = inv[q] ? 0.f : Qp[f];
                if constexpr (TRAIN) sv.y[(size_t)(q0 + q) * E + c] = v;
            } else if (c < E + d.D) v = src[(q0 + q) * d.D + (c - E)];
        }
        Z[f] = v;
    }
    __syncthreads();
    lds_linear(Z, d.ldq, 1, W1, d.E2p, d.hidden, d.Hp / 16, b1, 1.f, true, Xq, d.ldq);
    __syncthreads();
    lds_linear(Xq, d.ldq, 1, W2, d.Hp, d.out_dim, d.Op / 16, b2, 1.f, false, Qp, d.ldq);
    __syncthreads();
    for (int f = tid; f < nq * d.out_dim; f += ATT_THREADS) {
        const int q = f / d.out_dim, c = f - q * d.out_dim;
        out[(size_t)(q0 + q) * d.out_dim + c] = Qp[(size_t)q * d.ldq + c];
    }
    if constexpr (TRAIN) {
        for (int f = tid; f < nq * d.hidden; f += ATT_THREADS) {
            const int q = f / d.hidden, c = f - q * d.hidden;
            sv.hid[(size_t)(q0 + q) * d.hidden + c] = Xq[(size_t)q * d.ldq + c];
        }
    }
}

}  // namespace
}  // namespace zt
