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
#include "fc1_tile.hpp"           // the tile steps shared with k_fc1_agg and k_fc1_agg_bwd

using namespace zt;
using namespace zt::dense;        // f32x4, round_up, AGG_LDS_BUDGET, AGG_THREADS / AGG_WAVES / NTW / NTW_WIDE

namespace {

constexpr int SPLIT_MT = 5;                 // 16-row tiles per chunk (80 gathered rows, the register tile of k_fc1_agg)
constexpr int SPLIT_KMAX = 256;             // staged per-row entries (k <= ZT_MAX_K_WIDE < 256)

static_assert(ZT_MAX_K_WIDE < SPLIT_KMAX && SPLIT_KMAX <= AGG_THREADS, "one staging thread per neighbour");

size_t split_lds(int lda, int mt, int T) { return ((size_t)mt * 16 * lda + 4 * SPLIT_KMAX + T + 4) * 4; }

// NW: N-tiles of the hidden layer per wave (NTW: D <= 128; NTW_WIDE: 128 < D <= 256)
template <int NW>
__global__ __launch_bounds__(AGG_THREADS) void k_fc1_agg_split(FcAggArgs a, int cmt, int lda)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // (a struct member carries no __restrict__: the hot pointers as locals)
    const float *__restrict__ memory = a.memory, *__restrict__ overlay = a.overlay, *__restrict__ efeat = a.efeat;
    const int D = a.D, F = a.F, T = a.T, k = a.k, K1p = a.K1p;
    const long long N = a.N;
    float *A = reinterpret_cast<float *>(smem);                        // [cmt*16][lda]   one chunk
    float *wn = A + (size_t)cmt * 16 * lda;                            // [SPLIT_KMAX]    normalised weights of the row
    int *g_nb = reinterpret_cast<int *>(wn + SPLIT_KMAX);              // >= 0: memory row, < 0: -(overlay row) - 1
    int *g_ei = g_nb + SPLIT_KMAX;
    float *g_dt = reinterpret_cast<float *>(g_ei + SPLIT_KMAX);
    float *tw = g_dt + SPLIT_KMAX;                                     // [T]
    float *wsum = tw + T;                                              // [1]
    const int tid = threadIdx.x;
    const long long n = blockIdx.x;
    const int m = blockIdx.y;
    const size_t rb = ((size_t)m * N + n) * k;                         // first entry of this row in [M][N][k]
    const int NT = (D + 15) / 16;

    // ---- the row's k entries (an out-of-range id latches ZT_ERR_RANGE and reads row 0 with weight 0) ----
    if (tid < k) {
        int nb = a.nbr[rb + tid], ei = a.eix[rb + tid];
        float wv = a.w[rb + tid];
        if (nb < 0 || nb >= a.num_nodes || ei < 0 || ei >= a.num_edges) {
            atomicExch(a.status, ZT_ERR_RANGE);
            nb = 0; ei = 0; wv = 0.f;
        }
        if (a.row_map != nullptr) { const int ov = a.row_map[nb]; if (ov >= 0) nb = -ov - 1; }
        g_nb[tid] = nb; g_ei[tid] = ei; g_dt[tid] = a.dt[rb + tid]; wn[tid] = wv;
    } else if (tid < SPLIT_KMAX) {
        wn[tid] = 0.f;                                                 // the last chunk's rows past k: weight 0 (fc1_hidden_rows)
    }
    for (int c = tid; c < T; c += AGG_THREADS) tw[c] = a.time_w[c];
    __syncthreads();
    // w / sum(w), 0 where the sum is 0; the sum in entry order like torch.sum(dim=1) and k_fc1_agg
    if (tid == 0) {
        float s = 0.f;
        for (int j = 0; j < k; ++j) s += wn[j];
        *wsum = s;
        a.S[(size_t)m * N + n] = (s == 0.f) ? 0.f : 1.f;
    }
    __syncthreads();
    {
        const float s = *wsum;
        if (tid < k) wn[tid] = (s == 0.f) ? 0.f : wn[tid] / s;
    }

    const fc1_weight_cursor<NW> wc(a.W1p, K1p, NT);
    const fc1_row_source from(memory, overlay, efeat, tw, D, F, T);
    const unsigned mK4 = fastdiv_magic((unsigned)(K1p >> 2));
    const int ldh = NT * 16 + 1;                                       // hidden rows staged in the A region
    float hacc = 0.f;                                                  // H[m][n][tid] (tid < D)

    for (int j0 = 0; j0 < k; j0 += cmt * 16) {
        const int rows = (k - j0) < cmt * 16 ? (k - j0) : cmt * 16;
        const int mt = (rows + 15) / 16, rows_p = mt * 16;
        __syncthreads();                                               // previous chunk's hidden rows consumed (and wn ready)
        gather_rows_v4(A, lda, rows, rows_p, K1p, mK4, from, g_nb + j0, g_ei + j0, g_dt + j0);
        __syncthreads();

        // ---- fc1 on f32 MFMA: wave handles N-tiles {wave, wave+4, ..}, all M-tiles of the chunk ----
        f32x4 acc[SPLIT_MT][NW];
#pragma unroll
        for (int x = 0; x < SPLIT_MT; ++x)
#pragma unroll
            for (int b = 0; b < NW; ++b) acc[x][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        fc1_mfma<SPLIT_MT, NW>(A, lda, mt, wc, K1p, acc);
        __syncthreads();   // every wave is done reading the A tile: reuse it for the hidden rows

        // ---- bias + ReLU + dropout + weight, staged as Hs[g][col] in the A region ----
        float *Hs = A;
        fc1_hidden_rows<SPLIT_MT, NW>(acc, wc.live, mt, a, wn + j0, rb + j0, Hs, ldh);
        __syncthreads();
        // ---- this chunk's rows into the column accumulators, in entry order ----
        if (tid < D)
            for (int g = 0; g < rows; ++g) hacc += Hs[(size_t)g * ldh + tid];
    }
    if (tid < D) a.H[((size_t)m * N + n) * D + tid] = hacc;
}

}  // namespace

// rows of one chunk (a multiple of 16, at most SPLIT_MT * 16); 0: not even one 16-row tile fits the LDS budget
int zt::fc1_agg_split_rows(int D, int F, int T)
{
    if (!width_supported(D) || F < 0 || T < 0) return 0;
    const int lda = round_up(D + F + T, 16) + 4;
    for (int mt = SPLIT_MT; mt >= 1; --mt)
        if (split_lds(lda, mt, T) <= (size_t)AGG_LDS_BUDGET) return mt * 16;
    return 0;
}

size_t zt::fc1_agg_split_lds(int D, int F, int T)
{
    const int cr = fc1_agg_split_rows(D, F, T);
    return cr > 0 ? split_lds(round_up(D + F + T, 16) + 4, cr / 16, T) : 0;
}

int zt::fc1_agg_split_launch(const FcAggArgs &a, hipStream_t s)
{
    const int D = a.D, F = a.F, T = a.T, k = a.k, M = a.M;
    const int cr = fc1_agg_split_rows(D, F, T);
    if (cr == 0 || k <= 0 || k > ZT_MAX_K_WIDE || a.K1p != round_up(D + F + T, 16) || a.N > 0x7fffffffLL || M > 65535) {
        set_error("row-split aggregation: D=%d F=%d T=%d k=%d M=%d unsupported (D <= 128 or a multiple of 4 up to %d, k <= %d, one "
                  "16-row chunk within %d KB of LDS)", D, F, T, k, M, MAX_D, ZT_MAX_K_WIDE, AGG_LDS_BUDGET / 1024);
        return ZT_ERR_UNSUPPORTED;
    }
    if (a.N == 0) return ZT_OK;
    const size_t lds = fc1_agg_split_lds(D, F, T);
    const auto fn = D > 16 * NTW * AGG_WAVES ? k_fc1_agg_split<NTW_WIDE> : k_fc1_agg_split<NTW>;
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(fn), lds));
    dim3 grid((unsigned)a.N, (unsigned)M);
    fn<<<grid, AGG_THREADS, lds, s>>>(a, cr / 16, a.K1p + 4);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
