// Training path of the top-k neighbour aggregation: forward with a sparse "updated rows"
// overlay and the fused backward.
//
// Reference (modules/embedding_module.py:227-276, train=True): `memory` is the lazily updated copy of the whole
// memory table (get_updated_memory clones [N, D] every batch, modules/memory_updater.py:79) and autograd flows
//   loss -> embeddings -> fc2 -> sum_k w_k relu(fc1([memory'[nbr] | ef | cos])) -> fc1, memory'[ids] -> GRU weights.
// Here the lazily updated rows live in a compact OVERLAY [U, D] (row_map[v] = overlay row of node v, or -1: the
// stored memory row, which carries no gradient); nothing of size [N, D] or [N, k, 2D+F] is ever materialised.
//
//   zt_agg_train_forward : H[m][n][:] = sum_k w_k relu(fc1(x_k)), S[m][n] = (sum w != 0)     (k_fc1_agg<false> + overlay)
//   zt_agg_train_backward: given dH, recomputes the pre-activations tile by tile and accumulates
//        dW1 += dpre^T x,   db1 += sum dpre,   d_overlay[row_map[nbr]] += dpre W_m      with dpre = w_k dH 1[pre > 0]
//     on f32 MFMA: three products per tile (the recompute and the two gradients), the [D, K1] weight gradient
//     held in registers across the tiles of a persistent workgroup and added to HBM once at the end.
//   A query row wider than one tile (k > 80, or F = 172 past k = 64) is split: a tile is then one chunk of one row's
//   neighbours, (m, n, chunk), and re-reads the row's k weights for the normaliser (forward: aggregate_split.hip).
#include "common.hpp"
#include "fc1_tile.hpp"            // the gather and the fc1 product shared with the forward kernels; k_pad_matrix

using namespace zt;
using namespace zt::dense;         // f32x4, round_up, AGG_LDS_BUDGET, AGG_THREADS / AGG_WAVES / NTW / NTW_WIDE

namespace {

constexpr int BW_MT = 5;           // 16-row tiles of gathered rows per step (80 rows)
constexpr int BW_MAX_OT = 24;      // dW1 output tiles per wave and launch (96 accumulator registers)
constexpr int BW_MT_WIDE = 3;      // ... the NTW_WIDE instantiation: 48 rows per step, 12 dW1 tiles per wave (the accumulators of
constexpr int BW_MAX_OT_WIDE = 12; // its forward recompute are four N-tiles wide: within the register file without scratch)

struct BwdArgs {
    FcAggArgs f;                       // the forward's arguments (H, S, status unused; ldm = D)
    int rq, lda, ldp, Dp;
    const float *dH;                   // [M][N][D]
    float *dW1, *db1, *d_overlay;      // [D][K1], [D], [U][D]  (accumulated with atomics)
    long long n_tiles;                 // tiles of rq query rows per model (row split: N * nch)
    int mt;                            // 16-row tiles per step (<= BW_MT)
    int nch;                           // row split: chunks of mt * 16 gathered rows per query row (rq = 1); 0: whole rows
    int kt_lo, kt_hi;                  // this launch accumulates dW1 column tiles [kt_lo, kt_hi)
    int first;                         // 1: this launch also accumulates db1 and d_overlay
};

template <int NW, int OT, int MT>  // forward N-tiles per wave, dW1 tiles per wave, 16-row tiles per step: NTW / BW_* or NTW_WIDE / BW_*_WIDE
__global__ __launch_bounds__(AGG_THREADS) void k_fc1_agg_bwd(BwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FcAggArgs &f = a.f;
    // (a struct member carries no __restrict__: the hot pointers as locals)
    const float *__restrict__ memory = f.memory, *__restrict__ overlay = f.overlay, *__restrict__ efeat = f.efeat;
    const int D = f.D, F = f.F, T = f.T, k = f.k, lda = a.lda, ldp = a.ldp, K1p = f.K1p, Dp = a.Dp;
    const int K1 = D + F + T;
    const int mt = a.mt, rows_p = mt * 16;
    float *A = reinterpret_cast<float *>(smem);                 // [rows_p][lda]   gathered rows
    float *P = A + (size_t)rows_p * lda;                        // [rows_p][ldp]   dpre
    float *wn = P + (size_t)rows_p * ldp;                       // [rows_p]
    int *g_src = reinterpret_cast<int *>(wn + rows_p);          // >= 0: memory row, < 0: -(overlay row) - 1
    int *g_ei = g_src + rows_p;
    float *g_dt = reinterpret_cast<float *>(g_ei + rows_p);
    float *tw = g_dt + rows_p;                                  // [T]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    const int NT = Dp / 16, KT = a.kt_hi - a.kt_lo;
    const int n_ot = NT * KT;                                   // 16x16 tiles of dW1 handled by this launch
    f32x4 gw[OT];                                        // this wave's dW1 tiles (tile t = wave + 4*q)
#pragma unroll
    for (int q = 0; q < OT; ++q) gw[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gb = 0.f;                                             // db1[tid] (tid < Dp)
    for (int c = tid; c < T; c += AGG_THREADS) tw[c] = f.time_w[c];
    const fc1_weight_cursor<NW> wc(f.W1p, K1p, NT);
    const fc1_row_source from(memory, overlay, efeat, tw, D, F, T);
    const unsigned mK4 = fastdiv_magic((unsigned)(K1p >> 2));

    const long long total = a.n_tiles * f.M;
    for (long long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int m = (int)(tile / a.n_tiles);
        long long q0 = (tile % a.n_tiles) * a.rq;
        int j0 = 0;                                             // (row split: tile = (m, n, chunk), rows j0 .. j0 + rows of row q0)
        if (a.nch > 0) {
            const long long r = tile % a.n_tiles;
            q0 = r / a.nch;
            j0 = (int)(r - q0 * a.nch) * rows_p;
        }
        const int nq = (int)((f.N - q0) < a.rq ? (f.N - q0) : a.rq);
        const int rows = a.nch > 0 ? (k - j0 < rows_p ? k - j0 : rows_p) : nq * k;
        const size_t mb = ((size_t)m * f.N + q0) * k + j0;     // first gathered row of this tile in [M][N][k]
        __syncthreads();                                        // previous tile fully consumed
        for (int g = tid; g < rows_p; g += AGG_THREADS) {
            int src = 0, ei = 0;
            float d = 0.f, wv = 0.f;
            if (g < rows) {
                int nb = f.nbr[mb + g];
                ei = f.eix[mb + g]; d = f.dt[mb + g]; wv = f.w[mb + g];
                if (nb < 0 || nb >= f.num_nodes || ei < 0 || ei >= f.num_edges) { nb = 0; ei = 0; wv = 0.f; }
                const int ov = f.row_map ? f.row_map[nb] : -1;
                src = ov >= 0 ? -ov - 1 : nb;
            }
            g_src[g] = src; g_ei[g] = ei; g_dt[g] = d; wn[g] = wv;
        }
        // row split: the normaliser needs all k weights of the row (checked the same way), staged in the P region
        float *wrow = P;
        if (a.nch > 0 && tid < k) {
            const size_t e = mb - j0 + tid;
            const int nb = f.nbr[e], ei = f.eix[e];
            wrow[tid] = (nb < 0 || nb >= f.num_nodes || ei < 0 || ei >= f.num_edges) ? 0.f : f.w[e];
        }
        __syncthreads();
        float my_sum = 0.f;
        if (tid < rows) {
            if (a.nch > 0) {
                for (int j = 0; j < k; ++j) my_sum += wrow[j];
            } else {
                const int q = tid / k;
                for (int j = 0; j < k; ++j) my_sum += wn[q * k + j];
            }
        }
        __syncthreads();
        if (tid < rows) wn[tid] = (my_sum == 0.f) ? 0.f : wn[tid] / my_sum;
        // ---- gather x = [memory' | ef | cos | 0] into the tile ----
        gather_rows_v4(A, lda, rows, rows_p, K1p, mK4, from, g_src, g_ei, g_dt);
        __syncthreads();
        // ---- recompute pre = x W1^T (f32 MFMA; wave owns N-tiles {wave, wave+4, ..}) ----
        f32x4 acc[MT][NW];
#pragma unroll
        for (int x = 0; x < MT; ++x)
#pragma unroll
            for (int b = 0; b < NW; ++b) acc[x][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        fc1_mfma<MT, NW>(A, lda, mt, wc, K1p, acc);
        // ---- dpre = w_k dH 1[pre > 0] into P ----
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            const int nt = wave + b * AGG_WAVES;
            if (nt >= NT) continue;
            const int col = nt * 16 + r16;
            const float bias = col < D ? f.b1[col] : 0.f;
#pragma unroll
            for (int x = 0; x < MT; ++x)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (x >= mt) continue;
                    const int g = x * 16 + g4 * 4 + j;
                    float dp = 0.f;
                    if (g < rows && col < D && acc[x][b][j] + bias > 0.f) {
                        dp = wn[g] * a.dH[((size_t)m * f.N + q0 + g / k) * D + col];
                        if (f.drop_thr != 0u)
                            dp *= drop_scale(f.drop_lo, f.drop_hi, f.drop_thr, f.drop_inv, (unsigned long long)(mb + g) * D + col);
                    }
                    P[(size_t)g * ldp + col] = dp;
                }
        }
        __syncthreads();
        // ---- db1 ----
        if (a.first && tid < Dp) {
            float s = 0.f;
            for (int g = 0; g < rows; ++g) s += P[(size_t)g * ldp + tid];
            gb += s;
        }
        // ---- dW1[i][c] += sum_g P[g][i] x[g][c]: tiles t = wave, wave+4, ...; tile t = (dt, kt) ----
#pragma unroll
        for (int q = 0; q < OT; ++q) {
            const int t = wave + q * AGG_WAVES;
            if (t >= n_ot) break;
            const int dtile = t / KT, ktile = a.kt_lo + t - dtile * KT;
            f32x4 c4 = gw[q];
            for (int s = 0; s < rows_p / 4; ++s) {
                const int g = 4 * s + g4;
                const float pa = P[(size_t)g * ldp + dtile * 16 + r16];        // A operand: [m = D column][k = g]
                const float xb = A[(size_t)g * lda + ktile * 16 + r16];        // B operand: [k = g][n = input column]
                c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, xb, c4, 0, 0, 0);
            }
            gw[q] = c4;
        }
        // ---- d_overlay[row][c] += sum_col P[g][col] W1[col][c]  (memory columns c < D only) ----
        if (a.first && f.row_map != nullptr) {
            f32x4 dx[MT][NW];
#pragma unroll
            for (int x = 0; x < MT; ++x)
#pragma unroll
                for (int b = 0; b < NW; ++b) dx[x][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < Dp / 4; ++s) {
                const int col = 4 * s + g4;
                float pa[MT], wb[NW];
#pragma unroll
                for (int x = 0; x < MT; ++x) pa[x] = x < mt ? P[(size_t)(x * 16 + r16) * ldp + col] : 0.f;   // [m = row g][k = col]
#pragma unroll
                for (int b = 0; b < NW; ++b) {
                    const int c = (wave + b * AGG_WAVES) * 16 + r16;
                    wb[b] = c < D ? f.W1p[(size_t)col * K1p + c] : 0.f;                           // [k = col][n = c]
                }
#pragma unroll
                for (int x = 0; x < MT; ++x)
#pragma unroll
                    for (int b = 0; b < NW; ++b)
                        if (x < mt) dx[x][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[x], wb[b], dx[x][b], 0, 0, 0);
            }
#pragma unroll
            for (int b = 0; b < NW; ++b) {
                const int c = (wave + b * AGG_WAVES) * 16 + r16;
                if (c >= D) continue;
#pragma unroll
                for (int x = 0; x < MT; ++x)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int g = x * 16 + g4 * 4 + j;
                        if (x >= mt || g >= rows) continue;
                        const int s = g_src[g];
                        if (s < 0 && dx[x][b][j] != 0.f) atomicAdd(a.d_overlay + (size_t)(-s - 1) * D + c, dx[x][b][j]);
                    }
            }
        }
    }
    // ---- flush the accumulated weight gradient ----
#pragma unroll
    for (int q = 0; q < OT; ++q) {
        const int t = wave + q * AGG_WAVES;
        if (t >= n_ot) break;
        const int dtile = t / KT, ktile = a.kt_lo + t - dtile * KT;
        const int c = ktile * 16 + r16;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = dtile * 16 + g4 * 4 + j;
            if (i < D && c < K1 && gw[q][j] != 0.f) atomicAdd(a.dW1 + (size_t)i * K1 + c, gw[q][j]);
        }
    }
    if (a.first && tid < D && gb != 0.f) atomicAdd(a.db1 + tid, gb);
}

// the backward's tile: as many whole query rows as fit max_mt 16-row tiles and 150 KB of LDS, else (a query row does not fit)
// the row split: tiles of one chunk of max_mt (or as many as fit) 16-row tiles, nch chunks per row.  false: refused
size_t bwd_lds(int mt, int K1p, int Dp, int T) { return ((size_t)mt * 16 * (K1p + 4 + Dp + 4) + (size_t)mt * 16 * 4 + T) * 4; }

bool bwd_tile(int D, int F, int T, int k, int &mt, int &rq, int &nch)
{
    if (!zt::width_supported(D) || F < 0 || T < 0 || k <= 0) return false;
    const int Dp = round_up(D, 16), K1p = round_up(D + F + T, 16);
    const int max_mt = Dp > 16 * NTW * AGG_WAVES ? BW_MT_WIDE : BW_MT;
    mt = max_mt;
    while (mt > 1 && bwd_lds(mt, K1p, Dp, T) > AGG_LDS_BUDGET) --mt;
    rq = (mt * 16) / k;
    if (rq < 1) { mt = (k + 15) / 16; rq = 1; }
    nch = 0;
    if ((mt > max_mt || bwd_lds(mt, K1p, Dp, T) > AGG_LDS_BUDGET) && k <= ZT_MAX_K_WIDE) {
        mt = max_mt;
        while (mt > 1 && bwd_lds(mt, K1p, Dp, T) > AGG_LDS_BUDGET) --mt;
        rq = 1;
        nch = (k + mt * 16 - 1) / (mt * 16);
    }
    if (mt > max_mt || bwd_lds(mt, K1p, Dp, T) > AGG_LDS_BUDGET) return false;
    if (nch == 0) mt = (rq * k + 15) / 16;
    return true;
}

}  // namespace

bool zt::agg_backward_supported(int D, int F, int T, int k)
{
    int mt, rq, nch;
    return bwd_tile(D, F, T, k, mt, rq, nch);
}

extern "C" int64_t zt_agg_backward_workspace_bytes(int32_t D, int32_t F, int32_t T)
{
    if (D <= 0 || F < 0 || T < 0) return -1;
    return (int64_t)round_up(D, 16) * round_up(D + F + T, 16) * 4;
}

extern "C" int zt_agg_train_backward(const float *memory_dev, const float *overlay_dev, const int32_t *row_map_dev,
                                     const float *efeat_dev, const float *time_w_dev, int64_t num_nodes, int64_t num_edges,
                                     int32_t D, int32_t F, int32_t T, int64_t N, int32_t M, int32_t k,
                                     const int32_t *nbr_dev, const int32_t *eix_dev, const float *dt_dev, const float *w_dev,
                                     const float *fc1_w_dev, const float *fc1_b_dev, const float *dH_dev, float *dW1_dev,
                                     float *db1_dev, float *d_overlay_dev, void *workspace_dev, float drop_p,
                                     uint64_t drop_seed, void *stream)
{
    if (!memory_dev || !efeat_dev || !time_w_dev || !nbr_dev || !eix_dev || !dt_dev || !w_dev || !fc1_w_dev || !fc1_b_dev ||
        !dH_dev || !dW1_dev || !db1_dev || !workspace_dev || N < 0 || D <= 0 || F < 0 || T < 0 || M <= 0 || k <= 0 ||
        (row_map_dev != nullptr && (!overlay_dev || !d_overlay_dev))) {
        set_error("zt_agg_train_backward: bad argument");
        return ZT_ERR_ARG;
    }
    if (N == 0) return ZT_OK;
    const int K1 = D + F + T, Dp = round_up(D, 16), K1p = round_up(K1, 16);
    const bool wide = Dp > 16 * NTW * AGG_WAVES;
    int mt, rq, nch;
    if (!bwd_tile(D, F, T, k, mt, rq, nch)) {
        set_error("zt_agg_train_backward: D=%d F=%d T=%d k=%d outside the supported shapes (D <= 128, or a multiple of 4 up to %d)",
                  D, F, T, k, zt::MAX_D);
        return ZT_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    float *W1p = reinterpret_cast<float *>(workspace_dev);
    k_pad_matrix<<<(Dp * K1p + 255) / 256, 256, 0, s>>>(fc1_w_dev, K1, 0, D, K1, W1p, Dp, K1p);
    BwdArgs a{};
    FcAggArgs &f = a.f;
    f.memory = memory_dev; f.overlay = overlay_dev; f.row_map = row_map_dev; f.efeat = efeat_dev; f.time_w = time_w_dev;
    f.set_dropout((drop_p > 0.f && drop_p < 1.f) ? drop_p : 0.f, drop_seed);
    f.num_nodes = num_nodes; f.num_edges = num_edges; f.N = N;
    f.D = D; f.F = F; f.T = T; f.k = k; f.M = M; f.ldm = D; f.K1p = K1p;
    f.nbr = nbr_dev; f.eix = eix_dev; f.dt = dt_dev; f.w = w_dev; f.W1p = W1p; f.b1 = fc1_b_dev;
    a.rq = rq; a.lda = K1p + 4; a.ldp = Dp + 4; a.Dp = Dp;
    a.dH = dH_dev; a.dW1 = dW1_dev; a.db1 = db1_dev; a.d_overlay = d_overlay_dev;
    a.n_tiles = nch > 0 ? N * nch : (N + rq - 1) / rq;
    a.mt = mt;
    a.nch = nch;
    const size_t lds = bwd_lds(mt, K1p, Dp, T);
    const auto fn = wide ? k_fc1_agg_bwd<NTW_WIDE, BW_MAX_OT_WIDE, BW_MT_WIDE> : k_fc1_agg_bwd<NTW, BW_MAX_OT, BW_MT>;
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(fn), lds));
    hipDeviceProp_t prop;
    int dev = 0;
    ZT_HIP(hipGetDevice(&dev));
    ZT_HIP(hipGetDeviceProperties(&prop, dev));
    long long grid = a.n_tiles * M;
    if (grid > prop.multiProcessorCount) grid = prop.multiProcessorCount;      // persistent: one weight-gradient flush per CU
    // the weight gradient of one launch lives in registers: BW_MAX_OT (wide D: BW_MAX_OT_WIDE) tiles per wave.  Wide inputs
    // (F = 172; D > 128: at D = 256, windows of 3 column tiles) take several launches over windows of input columns (the
    // recompute is repeated, db1 / d_overlay are not).
    const int NT = Dp / 16, KT = K1p / 16;
    const int win = ((wide ? BW_MAX_OT_WIDE : BW_MAX_OT) * AGG_WAVES) / NT;
    for (int lo = 0; lo < KT; lo += win) {
        a.kt_lo = lo; a.kt_hi = lo + win < KT ? lo + win : KT; a.first = lo == 0 ? 1 : 0;
        fn<<<(unsigned)grid, AGG_THREADS, lds, s>>>(a);
    }
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
