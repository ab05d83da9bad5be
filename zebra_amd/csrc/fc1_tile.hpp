// The tile steps the neighbour aggregation's general kernels share: k_fc1_agg (aggregate.hip), k_fc1_agg_split
// (aggregate_split.hip) and k_fc1_agg_bwd (aggregate_bwd.hip) gather rows [memory'[nbr] | ef | cos(dt w) | 0] into an LDS tile
// A[rows_p][lda], run fc1 over it on v_mfma_f32_16x16x4f32 -- wave w of the four owns the hidden layer's N-tiles {w, w + 4, ..},
// lane (r16, g4) = (lane & 15, lane >> 4) -- and turn the accumulators into weighted hidden rows.  One text for each step: the
// split kernel gives what a tile holding the whole row would give, and the backward recomputes the forward's pre-activations,
// because they run the same code.  Beside the weight-padding kernel, device functions only; none of them knows which kernel calls it.
#pragma once

#include "common.hpp"

namespace {

using zt::fastdiv;
using zt::fastdiv_magic;
using zt::dense::f32x4;
using zt::dense::AGG_THREADS;
using zt::dense::AGG_WAVES;

// Zero-padded copy of the block W[0..rows)[c0..c0+cols) of a matrix with leading dimension ld -> Wp[rows_p][cols_p].
__global__ void k_pad_matrix(const float *__restrict__ W, int ld, int c0, int rows, int cols, float *__restrict__ Wp,
                             int rows_p, int cols_p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_p * cols_p) return;
    const int r = i / cols_p, c = i % cols_p;
    Wp[i] = (r < rows && c < cols) ? W[(size_t)r * ld + c0 + c] : 0.f;
}

// This wave's N-tiles {wave, wave + 4, ..} of W1p [NT * 16][K1p]: where this lane's weight fragments start, and which of
// the NW tiles exist (a dead one points at tile 0 and is never multiplied).
template <int NW>
struct fc1_weight_cursor {
    const float *bp[NW];
    bool live[NW];
    __device__ __forceinline__ fc1_weight_cursor(const float *__restrict__ W1p, int K1p, int NT)
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            const int nt = wave + b * AGG_WAVES;
            live[b] = nt < NT;
            bp[b] = W1p + (size_t)((live[b] ? nt : 0) * 16 + (lane & 15)) * K1p + 4 * (lane >> 4);
        }
    }
};

// acc[a][b] += A[a-th 16 rows] * W1p[b-th owned N-tile]^T over K1p columns, for the mt first M-tiles of MT.  The weight
// fragments stream from L2 one chunk of 16 columns ahead of their MFMAs (keeping all of them in registers was measured: no
// gain, and it halves the occupancy).  Every accumulator receives its MFMAs in the order kc, j -- whoever calls.
template <int MT, int NW>
__device__ __forceinline__ void fc1_mfma(const float *A, int lda, int mt, const fc1_weight_cursor<NW> &wc, int K1p,
                                         f32x4 (&acc)[MT][NW])
{
    const float *const *bp = wc.bp;
    const bool *live = wc.live;
    const int lane = threadIdx.x & 63, r16 = lane & 15, g4 = lane >> 4;
    const int nchunk = K1p / 16;
    f32x4 bcur[NW], bnext[NW];
#pragma unroll
    for (int b = 0; b < NW; ++b) bcur[b] = *reinterpret_cast<const f32x4 *>(bp[b]);
    for (int kc = 0; kc < nchunk; ++kc) {
        if (kc + 1 < nchunk) {
#pragma unroll
            for (int b = 0; b < NW; ++b) bnext[b] = *reinterpret_cast<const f32x4 *>(bp[b] + 16 * (kc + 1));
        }
        f32x4 av[MT];
#pragma unroll
        for (int a = 0; a < MT; ++a)
            av[a] = a < mt ? *reinterpret_cast<const f32x4 *>(A + (size_t)(a * 16 + r16) * lda + 16 * kc + 4 * g4)
                           : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < NW; ++b)
                    if (a < mt && live[b])
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][j], bcur[b][j], acc[a][b], 0, 0, 0);
#pragma unroll
        for (int b = 0; b < NW; ++b) bcur[b] = bnext[b];
    }
}

// Hs[g][col] = wn[g] * drop(relu(acc + b1[col])) for every row g of the tile's mt M-tiles and this wave's live ones of the a.D
// columns.  The rows past the tile's last entry are written too, without a branch per element: the caller stages wn[g] = 0
// there and reads none of them back.  (A `g < rows` guard, 40 exec-masked stores per wave, cost the tiled kernel 716 -> 690 us
// at 12 288 rows.)  The dropout element of (g, col) is (entry0 + g) * D + col, entry0 the tile's first entry in [M][N][k]; wn:
// the tile's first row's.
template <int MT, int NW>
__device__ __forceinline__ void fc1_hidden_rows(const f32x4 (&acc)[MT][NW], const bool (&live)[NW], int mt,
                                                const zt::FcAggArgs &a, const float *wn, size_t entry0, float *Hs, int ldh)
{
    const int Dout = a.D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g4 = lane >> 4;
#pragma unroll
    for (int b = 0; b < NW; ++b) {
        if (!live[b]) continue;
        const int col = (wave + b * AGG_WAVES) * 16 + r16;
        const float bias = col < Dout ? a.b1[col] : 0.f;
#pragma unroll
        for (int x = 0; x < MT; ++x) {
            if (x >= mt) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = x * 16 + g4 * 4 + j;
                float v = acc[x][b][j] + bias;
                v = v > 0.f ? v : 0.f;
                if (a.drop_thr != 0u)
                    v *= zt::drop_scale(a.drop_lo, a.drop_hi, a.drop_thr, a.drop_inv, (unsigned long long)(entry0 + g) * Dout + col);
                Hs[(size_t)g * ldh + col] = v * wn[g];
            }
        }
    }
}

// Where gathered rows come from.  A staged row id s >= 0 is memory row s, s < 0 overlay row -s - 1.  vecD / vecF: the memory /
// edge-feature rows are whole float4s, 16-byte aligned in HBM (and so in the tile).
struct fc1_row_source {
    const float *memory, *overlay, *efeat, *tw;     // tw: the T time-encoding frequencies (LDS)
    int D, F, K1;
    bool vecD, vecF;
    __device__ __forceinline__ fc1_row_source(const float *memory_, const float *overlay_, const float *efeat_, const float *tw_,
                                              int D_, int F_, int T_)
        : memory(memory_), overlay(overlay_), efeat(efeat_), tw(tw_), D(D_), F(F_), K1(D_ + F_ + T_)
    {
        vecD = (D & 3) == 0 && ((size_t)memory & 15) == 0 && (overlay == nullptr || ((size_t)overlay & 15) == 0);
        vecF = vecD && F > 0 && (F & 3) == 0 && ((size_t)efeat & 15) == 0;
    }
    __device__ __forceinline__ const float *mem_row(int s) const
    {
        return s >= 0 ? memory + (size_t)s * D : overlay + (size_t)(-s - 1) * D;
    }
};

// A[g][0 .. K1p) = [memory'[nb[g]] | ef[ei[g]] | cos(dt[g] w) | 0] for g < rows, zeros for rows <= g < rows_p: four columns
// per element, GU elements' loads in flight per thread before their LDS stores.  nb / ei / dt: the staged entries of the
// tile's first row; mK4 = fastdiv_magic(K1p / 4).
__device__ __forceinline__ void gather_rows_v4(float *A, int lda, int rows, int rows_p, int K1p, unsigned mK4,
                                               const fc1_row_source &src, const int *nb, const int *ei, const float *dt)
{
    constexpr int GU = 8;
    const int K4 = K1p >> 2, D = src.D, F = src.F;
    for (int f0 = threadIdx.x; f0 < rows_p * K4; f0 += AGG_THREADS * GU) {
        f32x4 v[GU];
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int f = f0 + u * AGG_THREADS;
            const int g = fastdiv(f, mK4), col = 4 * (f - g * K4);
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (f >= rows_p * K4 || g >= rows) continue;
            if (src.vecD && col + 4 <= D) {
                v[u] = *reinterpret_cast<const f32x4 *>(src.mem_row(nb[g]) + col);
            } else if (src.vecF && col >= D && col + 4 <= D + F) {
                v[u] = *reinterpret_cast<const f32x4 *>(src.efeat + (size_t)ei[g] * F + (col - D));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = col + e;
                    v[u][e] = c < D ? src.mem_row(nb[g])[c]
                                    : (c < D + F ? src.efeat[(size_t)ei[g] * F + (c - D)]
                                                 : (c < src.K1 ? zt::time_cosf(dt[g] * src.tw[c - D - F]) : 0.f));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int f = f0 + u * AGG_THREADS;
            const int g = fastdiv(f, mK4), c4 = f - g * K4;
            if (f < rows_p * K4) *reinterpret_cast<f32x4 *>(A + (size_t)g * lda + 4 * c4) = v[u];
        }
    }
}

// k_fc1_agg's gather: a [rows_p][n] block of elements V (float, or f32x4: four columns) goes to the tile's columns from
// col0, element f = (row g, element c) = (f / n, f % n) (magic = fastdiv_magic(n)) from src(g, c), zero for g >= rows.  GU
// elements per thread are LOADED, f0 + u * AGG_THREADS, before any is STORED (a row-at-a-time loop serialises on HBM latency:
// 20 rows x ~3 us per wave); the two halves are separate so that a kernel can put other work between them.
template <class V, int GU>
struct batched_copy {
    int n, count;          // elements per row, elements in all (rows_p * n)
    unsigned magic;
    int rows;
    __device__ __forceinline__ batched_copy(int n_, int rows_p, int rows_)
        : n(n_), count(rows_p * n_), magic(fastdiv_magic((unsigned)(n_ > 0 ? n_ : 1))), rows(rows_) {}
    template <class Src>
    __device__ __forceinline__ void load(V (&v)[GU], int f0, Src src) const
    {
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int f = f0 + u * AGG_THREADS;
            const int g = fastdiv(f, magic), c = f - g * n;
            v[u] = (f < count && g < rows) ? src(g, c) : V{};
        }
    }
    __device__ __forceinline__ void store(const V (&v)[GU], int f0, float *A, int lda, int col0) const
    {
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int f = f0 + u * AGG_THREADS;
            const int g = fastdiv(f, magic), c = f - g * n;
            if (f < count) *reinterpret_cast<V *>(A + (size_t)g * lda + col0 + (int)(sizeof(V) / sizeof(float)) * c) = v[u];
        }
    }
    // every element from f0 on, a batch at a time
    template <class Src>
    __device__ __forceinline__ void run(int f0, Src src, float *A, int lda, int col0) const
    {
        for (; f0 < count; f0 += AGG_THREADS * GU) {
            V v[GU];
            load(v, f0, src);
            store(v, f0, A, lda, col0);
        }
    }
};

}  // namespace
