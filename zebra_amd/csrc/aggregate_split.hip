// Row-split neighbour aggregation: fc1 + ReLU (+ dropout) + T-PPR-weighted k-reduction for query rows whose k gathered
// rows do not fit one LDS tile (80 < k <= ZT_MAX_K_WIDE with the memory columns gathered, or F = 172 past k = 136 in
// eval).  Same arithmetic as k_fc1_agg<false> (aggregate.hip):
//   H[m][n][:] = sum_j w_j/sum(w) drop(relu(fc1([memory'[nbr_j] | ef_j | cos(dt_j w)]) )),   S[m][n] = (sum(w) != 0)
// but a workgroup owns ONE (model, query row) and walks its k neighbours in chunks of at most SPLIT_MT 16-row tiles:
//   gather the chunk into LDS -> fc1 on v_mfma_f32_16x16x4f32 -> bias, ReLU, dropout, weight -> add the chunk's rows
//   into per-column accumulators (one register per column, held across the chunks).
// The normaliser sum(w) is formed once per row in entry order j = 0..k-1, and every column is reduced in the same order
// j = 0..k-1, like the one-tile kernel: H is the same from run to run (no atomics), and equal to what a tile holding the
// whole row would give.  The dropout element index stays ((m N + n) k + j) D + col (modules.dropout_mask, aggregate_bwd).
//
// LDS: the chunk tile [cr][K1p + 4] floats + the row's staged ids / dt / weights (4 x 256 words) + the frequencies.
// D = T = 100, F = 172: K1p = 384, 80 rows x 388 floats = 124 KB + 4.4 KB (one workgroup per CU); F = 1: 68 KB.
#include "common.hpp"
#include "embed_out_body.hpp"     // f32x4, AGG_THREADS / AGG_WAVES / NTW / NTW_WIDE

using namespace zt;

namespace {

constexpr int SPLIT_MT = 5;                 // 16-row tiles per chunk (80 gathered rows, the register tile of k_fc1_agg)
constexpr int SPLIT_KMAX = 256;             // staged per-row entries (k <= ZT_MAX_K_WIDE < 256)
constexpr int SPLIT_LDS_BUDGET = 150 * 1024;

static_assert(ZT_MAX_K_WIDE < SPLIT_KMAX && SPLIT_KMAX <= AGG_THREADS, "one staging thread per neighbour");

__host__ __device__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

size_t split_lds(int lda, int mt, int T) { return ((size_t)mt * 16 * lda + 4 * SPLIT_KMAX + T + 4) * 4; }

// NW: N-tiles of the hidden layer per wave (NTW: D <= 128; NTW_WIDE: 128 < D <= 256)
template <int NW>
__global__ __launch_bounds__(AGG_THREADS) void k_fc1_agg_split(
    const float *__restrict__ memory, const float *__restrict__ overlay, const int *__restrict__ row_map,
    const float *__restrict__ efeat, const float *__restrict__ time_w, long long num_nodes, long long num_edges, int D,
    int F, int T, long long N, int k, int cmt, int lda, const int *__restrict__ nbr, const int *__restrict__ eix,
    const float *__restrict__ dt, const float *__restrict__ w, const float *__restrict__ W1p, int K1p,
    const float *__restrict__ b1, float *__restrict__ H, float *__restrict__ S, int *status, unsigned drop_lo,
    unsigned drop_hi, unsigned drop_thr, float drop_inv)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *A = reinterpret_cast<float *>(smem);                        // [cmt*16][lda]   one chunk
    float *wn = A + (size_t)cmt * 16 * lda;                            // [SPLIT_KMAX]    normalised weights of the row
    int *g_nb = reinterpret_cast<int *>(wn + SPLIT_KMAX);              // >= 0: memory row, < 0: -(overlay row) - 1
    int *g_ei = g_nb + SPLIT_KMAX;
    float *g_dt = reinterpret_cast<float *>(g_ei + SPLIT_KMAX);
    float *tw = g_dt + SPLIT_KMAX;                                     // [T]
    float *wsum = tw + T;                                              // [1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    const long long n = blockIdx.x;
    const int m = blockIdx.y;
    const size_t rb = ((size_t)m * N + n) * k;                         // first entry of this row in [M][N][k]
    const int K1 = D + F + T, NT = (D + 15) / 16;

    // ---- the row's k entries (an out-of-range id latches ZT_ERR_RANGE and reads row 0 with weight 0) ----
    if (tid < k) {
        int nb = nbr[rb + tid], ei = eix[rb + tid];
        float wv = w[rb + tid];
        if (nb < 0 || nb >= num_nodes || ei < 0 || ei >= num_edges) {
            atomicExch(status, ZT_ERR_RANGE);
            nb = 0; ei = 0; wv = 0.f;
        }
        if (row_map != nullptr) { const int ov = row_map[nb]; if (ov >= 0) nb = -ov - 1; }
        g_nb[tid] = nb; g_ei[tid] = ei; g_dt[tid] = dt[rb + tid]; wn[tid] = wv;
    }
    for (int c = tid; c < T; c += AGG_THREADS) tw[c] = time_w[c];
    __syncthreads();
    // w / sum(w), 0 where the sum is 0; the sum in entry order like torch.sum(dim=1) and k_fc1_agg
    if (tid == 0) {
        float s = 0.f;
        for (int j = 0; j < k; ++j) s += wn[j];
        *wsum = s;
        S[(size_t)m * N + n] = (s == 0.f) ? 0.f : 1.f;
    }
    __syncthreads();
    {
        const float s = *wsum;
        if (tid < k) wn[tid] = (s == 0.f) ? 0.f : wn[tid] / s;
    }

    const float *bp[NW];
    bool live[NW];
#pragma unroll
    for (int b = 0; b < NW; ++b) {
        const int nt = wave + b * AGG_WAVES;
        live[b] = nt < NT;
        bp[b] = W1p + (size_t)((live[b] ? nt : 0) * 16 + r16) * K1p + 4 * g4;
    }
    auto mem_row = [&](int s) { return s >= 0 ? memory + (size_t)s * D : overlay + (size_t)(-s - 1) * D; };
    const bool vecD = (D & 3) == 0 && ((size_t)memory & 15) == 0 && (overlay == nullptr || ((size_t)overlay & 15) == 0);
    const bool vecF = vecD && F > 0 && (F & 3) == 0 && ((size_t)efeat & 15) == 0;
    const int K4 = K1p >> 2;
    const unsigned mK4 = fastdiv_magic((unsigned)K4);
    const int ldh = NT * 16 + 1;                                       // hidden rows staged in the A region
    float hacc = 0.f;                                                  // H[m][n][tid] (tid < D)

    for (int j0 = 0; j0 < k; j0 += cmt * 16) {
        const int rows = (k - j0) < cmt * 16 ? (k - j0) : cmt * 16;
        const int mt = (rows + 15) / 16, rows_p = mt * 16;
        __syncthreads();                                               // previous chunk's hidden rows consumed (and wn ready)
        // ---- gather [memory'[nbr] | ef | cos(dt w) | 0] of rows j0 .. j0 + rows_p, four columns per element; GU
        // ---- elements' loads in flight per thread before their LDS stores
        constexpr int GU = 8;
        for (int f0 = tid; f0 < rows_p * K4; f0 += AGG_THREADS * GU) {
            f32x4 v[GU];
#pragma unroll
            for (int u = 0; u < GU; ++u) {
                const int f = f0 + u * AGG_THREADS;
                const int g = fastdiv(f, mK4), col = 4 * (f - g * K4);
                v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (f >= rows_p * K4 || g >= rows) continue;
                const int j = j0 + g;
                if (vecD && col + 4 <= D) {
                    v[u] = *reinterpret_cast<const f32x4 *>(mem_row(g_nb[j]) + col);
                } else if (vecF && col >= D && col + 4 <= D + F) {
                    v[u] = *reinterpret_cast<const f32x4 *>(efeat + (size_t)g_ei[j] * F + (col - D));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = col + e;
                        v[u][e] = c < D ? mem_row(g_nb[j])[c]
                                        : (c < D + F ? efeat[(size_t)g_ei[j] * F + (c - D)]
                                                     : (c < K1 ? time_cosf(g_dt[j] * tw[c - D - F]) : 0.f));
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
        __syncthreads();

        // ---- fc1 on f32 MFMA: wave handles N-tiles {wave, wave+4, ..}, all M-tiles of the chunk ----
        f32x4 acc[SPLIT_MT][NW];
#pragma unroll
        for (int a = 0; a < SPLIT_MT; ++a)
#pragma unroll
            for (int b = 0; b < NW; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const int nchunk = K1p / 16;
            f32x4 bcur[NW], bnext[NW];
#pragma unroll
            for (int b = 0; b < NW; ++b) bcur[b] = *reinterpret_cast<const f32x4 *>(bp[b]);
            for (int kc = 0; kc < nchunk; ++kc) {
                if (kc + 1 < nchunk) {
#pragma unroll
                    for (int b = 0; b < NW; ++b) bnext[b] = *reinterpret_cast<const f32x4 *>(bp[b] + 16 * (kc + 1));
                }
                f32x4 av[SPLIT_MT];
#pragma unroll
                for (int a = 0; a < SPLIT_MT; ++a)
                    av[a] = a < mt ? *reinterpret_cast<const f32x4 *>(A + (size_t)(a * 16 + r16) * lda + 16 * kc + 4 * g4)
                                   : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int a = 0; a < SPLIT_MT; ++a)
#pragma unroll
                        for (int b = 0; b < NW; ++b)
                            if (a < mt && live[b])
                                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][j], bcur[b][j], acc[a][b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < NW; ++b) bcur[b] = bnext[b];
            }
        }
        __syncthreads();   // every wave is done reading the A tile: reuse it for the hidden rows

        // ---- bias + ReLU + dropout + weight, staged as Hs[g][col] in the A region ----
        float *Hs = A;
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            if (!live[b]) continue;
            const int col = (wave + b * AGG_WAVES) * 16 + r16;
            const float bias = col < D ? b1[col] : 0.f;
#pragma unroll
            for (int a = 0; a < SPLIT_MT; ++a) {
                if (a >= mt) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int g = a * 16 + g4 * 4 + j;
                    if (g >= rows) continue;
                    float v = acc[a][b][j] + bias;
                    v = v > 0.f ? v : 0.f;
                    if (drop_thr != 0u)
                        v *= drop_scale(drop_lo, drop_hi, drop_thr, drop_inv, (unsigned long long)(rb + j0 + g) * D + col);
                    Hs[(size_t)g * ldh + col] = v * wn[j0 + g];
                }
            }
        }
        __syncthreads();
        // ---- this chunk's rows into the column accumulators, in entry order ----
        if (tid < D)
            for (int g = 0; g < rows; ++g) hacc += Hs[(size_t)g * ldh + tid];
    }
    if (tid < D) H[((size_t)m * N + n) * D + tid] = hacc;
}

}  // namespace

// rows of one chunk (a multiple of 16, at most SPLIT_MT * 16); 0: not even one 16-row tile fits the LDS budget
int zt::fc1_agg_split_rows(int D, int F, int T)
{
    if (!width_supported(D) || F < 0 || T < 0) return 0;
    const int lda = round_up(D + F + T, 16) + 4;
    for (int mt = SPLIT_MT; mt >= 1; --mt)
        if (split_lds(lda, mt, T) <= (size_t)SPLIT_LDS_BUDGET) return mt * 16;
    return 0;
}

size_t zt::fc1_agg_split_lds(int D, int F, int T)
{
    const int cr = fc1_agg_split_rows(D, F, T);
    return cr > 0 ? split_lds(round_up(D + F + T, 16) + 4, cr / 16, T) : 0;
}

int zt::fc1_agg_split_launch(const float *memory, const float *overlay, const int *row_map, const float *efeat,
                             const float *time_w, long long num_nodes, long long num_edges, int D, int F, int T,
                             long long N, int M, int k, const int *nbr, const int *eix, const float *dt, const float *w,
                             const float *W1p, int K1p, const float *b1, float *H, float *S, int *status, float drop_p,
                             unsigned long long drop_seed, hipStream_t s)
{
    const int cr = fc1_agg_split_rows(D, F, T);
    if (cr == 0 || k <= 0 || k > ZT_MAX_K_WIDE || K1p != round_up(D + F + T, 16) || N > 0x7fffffffLL || M > 65535) {
        set_error("row-split aggregation: D=%d F=%d T=%d k=%d M=%d unsupported (D <= 128 or a multiple of 4 up to %d, k <= %d, one "
                  "16-row chunk within %d KB of LDS)", D, F, T, k, M, MAX_D, ZT_MAX_K_WIDE, SPLIT_LDS_BUDGET / 1024);
        return ZT_ERR_UNSUPPORTED;
    }
    if (N == 0) return ZT_OK;
    const size_t lds = fc1_agg_split_lds(D, F, T);
    const auto fn = D > 16 * NTW * AGG_WAVES ? k_fc1_agg_split<NTW_WIDE> : k_fc1_agg_split<NTW>;
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(fn), lds));
    const unsigned thr = drop_threshold(drop_p);
    dim3 grid((unsigned)N, (unsigned)M);
    fn<<<grid, AGG_THREADS, lds, s>>>(memory, overlay, row_map, efeat, time_w, num_nodes, num_edges, D, F, T, N, k,
                                      cr / 16, K1p + 4, nbr, eix, dt, w, W1p, K1p, b1, H, S, status,
                                      (unsigned)drop_seed, (unsigned)(drop_seed >> 32), thr,
                                      thr ? 1.f / (1.f - drop_p) : 1.f);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
