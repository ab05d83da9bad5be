// Top-k neighbour gather + TimeEncode + transform + T-PPR-weighted sum (P2).
//
// Replaces the device half of GraphDiffusionEmbedding.compute_embedding_tppr_ensemble
// (reference modules/embedding_module.py:243-276, transform/transform_source
// :320-328, TimeEncode model/time_encoding.py:23-28), eval forward.
//
// The reference materialises cat[memory[nbr] | edge_feat[eidx] | cos(dt*w)] as
// an [N,k,2D+F] tensor, runs two Linear layers over all N*k rows and then
// reduces over k.  Here:
//   k_fc1_agg   one workgroup per (tile of RQ query rows, model): gathers the
//               RQ*k neighbour rows straight into an LDS tile (the cat is never
//               written to HBM), evaluates the time encoding in-register,
//               runs fc1 on exact-f32 MFMA (v_mfma_f32_16x16x4_f32; weights
//               streamed from L2 as pre-padded fragments), applies bias+ReLU
//               and the normalised T-PPR weight, and reduces over k in LDS.
//               fc2 is linear, so sum_k w_k*fc2(h_k) = fc2(sum_k w_k*h_k) +
//               b2*sum_k w_k: only the [N,D] reduced rows go through fc2.
//   k_embed_out fc2 on the reduced rows, transform_source on memory[nodes]
//               (three D x D layers, also f32 MFMA) and the concat into out[N, D*(M+1)].
// Arithmetic is float32 throughout (parity tolerance for embeddings: 1e-4).
#include "common.hpp"
#include "embed_out_body.hpp"     // small_gemm, the output layers' body (shared with memory_update.hip)
#include "fc1_tile.hpp"           // the fc1 tile steps shared with aggregate_split.hip and aggregate_bwd.hip; k_pad_matrix

using namespace zt;
using namespace zt::dense;        // f32x4, round_up, AGG_LDS_BUDGET, AGG_THREADS / AGG_WAVES / NTW / NTW_WIDE

namespace {

constexpr int MAX_MT = 5;          // M-tiles (16 gathered rows each) per workgroup
constexpr int MAX_MT_BIG = 16;     // ... of the instantiation for 80 < k <= 255 (k_fc1_agg<TAB, MAX_MT_BIG>)
constexpr int MAX_MT_BIG_WIDE = 8; // ... of the one for 128 < D (k_fc1_agg<TAB, MAX_MT_BIG_WIDE, NTW_WIDE>: 80 < k <= 128)

#ifdef ZT_AGG_STAMP
// diagnostic build only: shader-clock time per phase of k_fc1_agg, summed over workgroups
__device__ unsigned long long g_agg[8];
#define AGG_STAMP(i) do { if (threadIdx.x == 0) { const long long t__ = clock64(); atomicAdd(&g_agg[i], (unsigned long long)(t__ - t_prev__)); t_prev__ = t__; } } while (0)
#else
#define AGG_STAMP(i) do { } while (0)
#endif

// ---------------------------------------------------------------------------
// fc1 + ReLU + weighted k-reduction.
//   A tile in LDS: [mt*16][lda] floats, row g = q*k + j holds
//   [memory[nbr] (D) | efeat[eidx] (F) | cos(dt*w_t) (T) | 0-pad].
//   W1p: [Dp][K1p] zero padded (Dp = NT*16, K1p = round_up(K1,16)).
//   H:   [M][N][D] reduced hidden rows;  S: [M][N] = 1 if sum(w) != 0 else 0.
// ---------------------------------------------------------------------------
// TAB = true: the memory columns are not gathered and not multiplied.  fc1 is linear, so
//   fc1([mem | ef | cos]) = W_m mem + W_e ef + W_t cos + b1, and W_m mem[v] is a per-NODE quantity: it is kept in
// a projected table P[v] = W_m memory[v] ([num_nodes][Dp], maintained by k_project_rows whenever a memory row
// changes: at most 2B rows per batch instead of 3B*k*M gathered rows).  The accumulators START from the
// gathered P rows, the tile holds only [ef | cos] and the contraction runs over F + T columns: for F = 1
// half the matrix work and none of the memory-row staging.  `memory` then points at P and D is the row stride Dp.
// MMT: M-tiles a workgroup can hold.  MAX_MT (5: 80 gathered rows) for every k <= 80; MAX_MT_BIG (16) is instantiated for
// 80 < k <= 255 -- a query row of that many neighbours must still fit ONE workgroup's tile (dictionaries wider than a
// wavefront: tppr_wide.hpp; correct first, not tuned).
// NW: N-tiles of the hidden layer per wave.  NTW (Dp <= 128); NTW_WIDE for 128 < D <= 256, D % 4 == 0 (MMT <= MAX_MT_BIG_WIDE:
// the accumulators of MMT x NW tiles stay at the MAX_MT_BIG instantiation's 128 registers).
template <bool TAB, int MMT = MAX_MT, int NW = NTW>
__global__ __launch_bounds__(AGG_THREADS) void k_fc1_agg(FcAggArgs a, int rq, int mt_count, int lda)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // (a struct member carries no __restrict__: the hot pointers as locals)
    const float *__restrict__ memory = a.memory, *__restrict__ efeat = a.efeat, *__restrict__ overlay = a.overlay;
    const int D = a.ldm, F = a.F, T = a.T, k = a.k, Dout = a.D;       // D: the row stride of `memory` (TAB: Dp)
    const long long N = a.N;
    float *A = reinterpret_cast<float *>(smem);                       // [mt*16][lda]
    float *wn = A + (size_t)mt_count * 16 * lda;                      // [mt*16] normalised weights
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = blockIdx.y;
    const long long q0 = (long long)blockIdx.x * rq;
    const int nq = (int)((N - q0) < rq ? (N - q0) : rq);
    const int rows = nq * k, rows_p = mt_count * 16;
    const int CM = TAB ? 0 : D;                                       // memory columns held in the tile
    const int K1 = CM + F + T;
    const size_t mb = ((size_t)m * N + q0) * k;                       // first entry of this tile in [M][N][k]
    const int NT = (Dout + 15) / 16;
    const int r16 = lane & 15, g4 = lane >> 4;
    const fc1_weight_cursor<NW> wc(a.W1p, a.K1p, NT);
#ifdef ZT_AGG_STAMP
    long long t_prev__ = clock64();
#endif

    // per-row gather indices, staged once so that the row loads below are independent
    int *g_nb = reinterpret_cast<int *>(wn + rows_p);                 // [mt*16]
    int *g_ei = g_nb + rows_p;
    float *g_dt = reinterpret_cast<float *>(g_ei + rows_p);
    float *tw = g_dt + rows_p;                                        // [T] time-encoding frequencies

    // ---- stage the per-row scalars (coalesced), then normalise the weights in LDS ----
    for (int g = tid; g < rows_p; g += AGG_THREADS) {
        int nb = 0, ei = 0;
        float d = 0.f, wv = 0.f;
        if (g < rows) {
            nb = a.nbr[mb + g]; ei = a.eix[mb + g]; d = a.dt[mb + g]; wv = a.w[mb + g];
            if (nb < 0 || nb >= a.num_nodes || ei < 0 || ei >= a.num_edges) {
                atomicExch(a.status, ZT_ERR_RANGE);
                nb = 0; ei = 0;
            }
            // training: rows of the lazily updated memory live in a compact overlay (aggregate_bwd.hip)
            if (!TAB && a.row_map != nullptr) { const int ov = a.row_map[nb]; if (ov >= 0) nb = -ov - 1; }
        }
        g_nb[g] = nb; g_ei[g] = ei; g_dt[g] = d; wn[g] = wv;
    }
    for (int c = tid; c < T; c += AGG_THREADS) tw[c] = a.time_w[c];
    __syncthreads();
    // w / sum(w), 0 where the sum is 0 (:267-270); sum in entry order like torch.sum(dim=1)
    float my_sum = 0.f;
    if (tid < rows) {
        const int q = tid / k;
        for (int j = 0; j < k; ++j) my_sum += wn[q * k + j];
    }
    __syncthreads();
    if (tid < rows) {
        wn[tid] = (my_sum == 0.f) ? 0.f : wn[tid] / my_sum;
        if (tid % k == 0) a.S[(size_t)m * N + q0 + tid / k] = (my_sum == 0.f) ? 0.f : 1.f;
    }

    auto mem_row = [&](int s) { return s >= 0 ? memory + (size_t)s * D : overlay + (size_t)(-s - 1) * D; };
    AGG_STAMP(0);
    // accumulators: zero, or (TAB) the projected rows P[nbr[row]][col] -- issued before the staging below so that the
    // memory round trip is hidden behind it; the MFMAs then accumulate on top of them
    f32x4 acc[MMT][NW];
#pragma unroll
    for (int x = 0; x < MMT; ++x)
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            acc[x][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (TAB && x < mt_count && wc.live[b]) {
                const int col = (wave + b * AGG_WAVES) * 16 + r16;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[x][b][j] = memory[(size_t)g_nb[x * 16 + g4 * 4 + j] * D + col];
            }
        }
    // ---- gather: flat (row, column) loops, GU loads in flight per thread before any LDS store (fc1_tile.hpp: batched_copy)
    constexpr int GU = 8;
    const unsigned mT = fastdiv_magic((unsigned)(T > 0 ? T : 1));
    // rows are whole float4s, 16-byte aligned in HBM and in the tile
    const bool vecD = TAB || ((D & 3) == 0 && ((size_t)memory & 15) == 0);
    const bool vecF = vecD && F > 0 && (F & 3) == 0 && ((size_t)efeat & 15) == 0;
    auto mem1 = [&](int g, int c) { return mem_row(g_nb[g])[c]; };
    auto mem4 = [&](int g, int c) { return *reinterpret_cast<const f32x4 *>(mem_row(g_nb[g]) + 4 * c); };
    auto ef1 = [&](int g, int c) { return efeat[(size_t)g_ei[g] * F + c]; };
    auto ef4 = [&](int g, int c) { return *reinterpret_cast<const f32x4 *>(efeat + (size_t)g_ei[g] * F + 4 * c); };
    // cos(dt * w_c) for every (row, frequency); reads only LDS.  A thread keeps ONE frequency in a register and
    // walks down a block of rows, four dt values per (broadcast) LDS read: no dependent LDS read and no index
    // arithmetic per element, and the four cosines of a step are independent instructions.
    auto time_encode = [&]() {
        if (T > AGG_THREADS || T <= 0) {                                // (not a shape the reference uses)
            for (int f = tid; f < rows_p * T; f += AGG_THREADS) {
                const int g = fastdiv(f, mT), c = f - g * T;
                A[g * lda + CM + F + c] = g < rows ? time_cosf(g_dt[g] * tw[c]) : 0.f;
            }
            return;
        }
        const int TC = T <= 64 ? 64 : (T <= 128 ? 128 : 256);          // threads per row block
        const int RG = AGG_THREADS / TC, per = rows_p / RG;             // rows_p is a multiple of 16
        const int c = tid & (TC - 1), g0 = (tid / TC) * per;
        if (c >= T) return;
        const float freq = tw[c];
        float *dst = A + (size_t)g0 * lda + CM + F + c;
        for (int i = 0; i < per; i += 4) {
            const f32x4 d4 = *reinterpret_cast<const f32x4 *>(g_dt + g0 + i);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                dst[(size_t)(i + u) * lda] = (g0 + i + u) < rows ? time_cosf(d4[u] * freq) : 0.f;     // cos(t*w + 0)
        }
    };
    const batched_copy<float, GU> ef_s(F, rows_p, rows);
    if (vecD) {
        // One memory round trip for the whole gather, with the time encoding computed underneath it: the
        // first GU 16-byte loads of every thread (all of them for D = 100, k = 20) and the first batch
        // of edge-feature loads are issued, then the cosines are evaluated, then the loaded values are
        // stored to the tile.  (Memory latency under the gather load is ~3-4 us per dependent access.)
        const batched_copy<f32x4, GU> mem_v(D >> 2, rows_p, rows), ef_v(F >> 2, rows_p, rows);
        f32x4 vm[GU], vf[GU];
        float sf[GU];
        if (!TAB) mem_v.load(vm, tid, mem4);                            // 1. first batch of memory loads
        if (vecF) ef_v.load(vf, tid, ef4);                              // 2. first batch of edge-feature loads
        else ef_s.load(sf, tid, ef1);
        AGG_STAMP(1);
        time_encode();                                                  // 3. the cosines underneath them
        AGG_STAMP(2);
        if (!TAB) mem_v.store(vm, tid, A, lda, 0);                      // 4. the stores
        if (vecF) ef_v.store(vf, tid, A, lda, CM);
        else ef_s.store(sf, tid, A, lda, CM);
        if (!TAB) mem_v.run(tid + AGG_THREADS * GU, mem4, A, lda, 0);   // 5. whatever does not fit the first batch
        if (vecF) ef_v.run(tid + AGG_THREADS * GU, ef4, A, lda, CM);
        else ef_s.run(tid + AGG_THREADS * GU, ef1, A, lda, CM);
    } else {
        batched_copy<float, GU>(D, rows_p, rows).run(tid, mem1, A, lda, 0);
        AGG_STAMP(1);
        ef_s.run(tid, ef1, A, lda, CM);
        AGG_STAMP(2);
        time_encode();
    }
    const int padw = a.K1p - K1;
    const unsigned mP = fastdiv_magic((unsigned)(padw > 0 ? padw : 1));
    for (int f = tid; f < rows_p * padw; f += AGG_THREADS) {
        const int g = fastdiv(f, mP), c = f - g * padw;
        A[(size_t)g * lda + K1 + c] = 0.f;
    }
    AGG_STAMP(3);
    __syncthreads();
    AGG_STAMP(4);

    // ---- fc1 on f32 MFMA: wave handles N-tiles {wave, wave+4, ..}, all M-tiles ----
    fc1_mfma<MMT, NW>(A, lda, mt_count, wc, a.K1p, acc);
    AGG_STAMP(5);
    __syncthreads();   // every wave is done reading the A tile: reuse it for the hidden rows

    // ---- bias + ReLU + dropout + weight, staged as Hs[g][col] in the A region ----
    float *Hs = A;                               // [rows_p][ldh]
    const int ldh = NT * 16 + 1;
    fc1_hidden_rows<MMT, NW>(acc, wc.live, mt_count, a, wn, mb, Hs, ldh);      // (wn = 0 past the last entry: staged above)
    __syncthreads();
    AGG_STAMP(6);
    // ---- reduce over the k neighbours of each query row ----
    const unsigned mDo = fastdiv_magic((unsigned)Dout);
    for (int idx = tid; idx < nq * Dout; idx += AGG_THREADS) {
        const int q = fastdiv(idx, mDo), c = idx - q * Dout;
        float s = 0.f;
        for (int j = 0; j < k; ++j) s += Hs[(size_t)(q * k + j) * ldh + c];
        a.H[((size_t)m * N + q0 + q) * Dout + c] = s;
    }
    AGG_STAMP(7);
}

// ---------------------------------------------------------------------------
// The same kernel (table path) for the reference's default widths -- memory_dim = time_dim = 100
// (train.py:33-36) -- and k in {10, 20, 40}: a tile is exactly 80 gathered rows (5 M-tiles), the hidden layer 7
// N-tiles.  k_fc1_agg<true> spends more SIMD time on vector instructions (index arithmetic, bounds, generic
// loops: ~2400 per wave and tile) than on its 245 MFMAs; with the widths fixed at compile time the vector
// work is ~3x smaller:
//   * every thread owns one time-encoding COLUMN (its frequency stays in a register) and walks down 40 rows,
//     four dt values per broadcast LDS read; the 28 idle column lanes write the zero padding of the tile;
//   * the projected rows are fetched with one 64-bit address per row and immediate offsets per column;
//   * bias / ReLU / weight and the k-reduction use immediate LDS offsets (no divisions anywhere).
// Waves 0-2 own N-tiles {w, w+4}, wave 3 owns tile 3 only (7 tiles): two instantiations of the MFMA loop.
// (Splitting the 35 (M, N) tile pairs 9 / 9 / 9 / 8 instead of 10 / 10 / 10 / 5 was measured: no difference -- the
// kernel is bound by the latency of a workgroup's serial phases at 4 workgroups per CU, not by MFMA issue.)
// ---------------------------------------------------------------------------
template <int NB>
__device__ __forceinline__ void d100_mfma(const float *A, int lda, const float *__restrict__ bp, int K1p, int nchunk, int nrem,
                                          int r16, int g4, f32x4 (&acc)[5][2])
{
    // nchunk whole 16-column chunks (one b128 fragment per lane: k = 16 kc + 4 g4 + j), then nrem single MFMA steps
    // over the last columns (k = 16 nchunk + 4 j + g4, scalar fragments): the contraction is padded to a multiple
    // of 4 columns, not 16 (F + T = 101 -> 26 steps instead of 28).
    f32x4 bcur[NB], bnext[NB];
    float bre[NB][3];
#pragma unroll
    for (int b = 0; b < NB; ++b) bcur[b] = *reinterpret_cast<const f32x4 *>(bp + (size_t)b * 64 * K1p);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            bre[b][j] = j < nrem ? bp[(size_t)b * 64 * K1p - 4 * g4 + 16 * nchunk + 4 * j + g4] : 0.f;
    const float *ap = A + (size_t)r16 * lda + 4 * g4;
    for (int kc = 0; kc < nchunk; ++kc) {
        if (kc + 1 < nchunk) {
#pragma unroll
            for (int b = 0; b < NB; ++b) bnext[b] = *reinterpret_cast<const f32x4 *>(bp + (size_t)b * 64 * K1p + 16 * (kc + 1));
        }
        f32x4 av[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) av[a] = *reinterpret_cast<const f32x4 *>(ap + (size_t)a * 16 * lda + 16 * kc);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int a = 0; a < 5; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][j], bcur[b][j], acc[a][b], 0, 0, 0);
#pragma unroll
        for (int b = 0; b < NB; ++b) bcur[b] = bnext[b];
    }
    const float *ar = A + (size_t)r16 * lda + 16 * nchunk + g4;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j >= nrem) break;
        float av[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) av[a] = ar[(size_t)a * 16 * lda + 4 * j];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bre[b][j], acc[a][b], 0, 0, 0);
    }
}

template <int KK>
__global__ __launch_bounds__(AGG_THREADS, 4) void k_fc1_agg_d100(
    const float *__restrict__ P, const float *__restrict__ efeat, const float *__restrict__ time_w, long long num_nodes,
    long long num_edges, int F, long long N, int lda, const int *__restrict__ nbr, const int *__restrict__ eix,
    const float *__restrict__ dt, const float *__restrict__ w, const float *__restrict__ W1p, int K1p,
    const float *__restrict__ b1, float *__restrict__ H, float *__restrict__ S, int *status)
{
    constexpr int D = 100, T = 100, DP = 112, ROWS = 80, RQ = ROWS / KK, LDH = DP + 1;
    static_assert(ROWS % KK == 0, "a tile holds whole query rows");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *A = reinterpret_cast<float *>(smem);                       // [80][lda]: [ef (F) | cos (T) | 0-pad]
    float *wn = A + (size_t)ROWS * lda;                               // raw T-PPR weights
    float *wnn = wn + ROWS;                                           // w / sum(w)
    int *g_nb = reinterpret_cast<int *>(wnn + ROWS);
    int *g_ei = g_nb + ROWS;
    float *g_dt = reinterpret_cast<float *>(g_ei + ROWS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    const int m = blockIdx.y;
    const long long q0 = (long long)blockIdx.x * RQ;
    const int nq = (int)((N - q0) < RQ ? (N - q0) : RQ);
    const int rows = nq * KK;
    const size_t mb = ((size_t)m * N + q0) * KK;
#ifdef ZT_AGG_STAMP
    long long t_prev__ = clock64();
#endif

    // ---- per-row scalars; a thread's own edge feature (F = 1) and time frequency ride on the same round trip ----
    float ef1 = 0.f;
    if (tid < ROWS) {
        int nb = 0, ei = 0;
        float d = 0.f, wv = 0.f;
        if (tid < rows) {
            nb = nbr[mb + tid]; ei = eix[mb + tid]; d = dt[mb + tid]; wv = w[mb + tid];
            if (nb < 0 || nb >= num_nodes || ei < 0 || ei >= num_edges) {
                atomicExch(status, ZT_ERR_RANGE);
                nb = 0; ei = 0;
            }
            if (F == 1) ef1 = efeat[ei];
        }
        g_nb[tid] = nb; g_ei[tid] = ei; g_dt[tid] = d; wn[tid] = wv;
    }
    const int cc = tid & 127;                                         // this thread's column of the time block
    const float wc = cc < T ? time_w[cc] : 0.f;
    const int col0 = wave * 16 + r16;                                 // this lane's output columns: col0, col0 + 64
    const float bias0 = col0 < D ? b1[col0] : 0.f, bias1 = (wave < 3 && col0 + 64 < D) ? b1[col0 + 64] : 0.f;
    __syncthreads();
    AGG_STAMP(0);

    // ---- accumulators start from the projected rows P[nbr[row]][col]: one address per row ----
    f32x4 acc[5][2];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const int nb4[4] = {g_nb[a * 16 + g4 * 4 + 0], g_nb[a * 16 + g4 * 4 + 1], g_nb[a * 16 + g4 * 4 + 2], g_nb[a * 16 + g4 * 4 + 3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *pr = P + (size_t)nb4[j] * DP + col0;
            acc[a][0][j] = pr[0];
            acc[a][1][j] = pr[wave < 3 ? 64 : 0];                     // wave 3 has no second N-tile: any valid address
        }
    }
    // ---- w / sum(w), 0 where the sum is 0 (:267-270); sum in entry order like torch.sum(dim=1) ----
    if (tid < ROWS) {
        const int q = tid / KK;
        float my_sum = 0.f;
#pragma unroll
        for (int j = 0; j < KK; ++j) my_sum += wn[q * KK + j];
        wnn[tid] = (my_sum == 0.f) ? 0.f : wn[tid] / my_sum;
        if (tid < rows && tid - q * KK == 0) S[(size_t)m * N + q0 + q] = (my_sum == 0.f) ? 0.f : 1.f;
    }
    AGG_STAMP(1);
    // ---- edge features ----
    if (F == 1) {
        if (tid < ROWS) A[(size_t)tid * lda] = ef1;
    } else if (F > 0) {
        constexpr int GU = 8;
        const bool vecF = (F & 3) == 0 && ((size_t)efeat & 15) == 0;
        if (vecF) {
            const int F4 = F >> 2;
            const unsigned mF4 = fastdiv_magic((unsigned)F4);
            for (int f0 = tid; f0 < ROWS * F4; f0 += AGG_THREADS * GU) {
                f32x4 v[GU];
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    const int f = f0 + u * AGG_THREADS;
                    const int g = fastdiv(f, mF4), c = f - g * F4;
                    v[u] = (f < ROWS * F4 && g < rows) ? *reinterpret_cast<const f32x4 *>(efeat + (size_t)g_ei[g] * F + 4 * c)
                                                      : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    const int f = f0 + u * AGG_THREADS;
                    const int g = fastdiv(f, mF4), c = f - g * F4;
                    if (f < ROWS * F4) *reinterpret_cast<f32x4 *>(A + (size_t)g * lda + 4 * c) = v[u];
                }
            }
        } else {
            const unsigned mF = fastdiv_magic((unsigned)F);
            for (int f0 = tid; f0 < ROWS * F; f0 += AGG_THREADS * GU) {
                float v[GU];
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    const int f = f0 + u * AGG_THREADS;
                    const int g = fastdiv(f, mF), c = f - g * F;
                    v[u] = (f < ROWS * F && g < rows) ? efeat[(size_t)g_ei[g] * F + c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    const int f = f0 + u * AGG_THREADS;
                    const int g = fastdiv(f, mF), c = f - g * F;
                    if (f < ROWS * F) A[(size_t)g * lda + c] = v[u];
                }
            }
        }
    }
    // ---- time encoding: column cc of rows [40 * (tid / 128), +40); lanes 100..127 write the zero padding ----
    // The common-range formula of time_cosf runs branch-free; the largest |argument| is tracked on the side and
    // the (rare: dt * w >= 4e6) columns are redone with the full routine afterwards.
    {
        const int g0 = (tid >> 7) * 40;
        const bool is_cos = cc < T;
        if (is_cos || F + cc < K1p) {
            float *dst = A + (size_t)g0 * lda + F + cc;
            float xmax = 0.f;
#pragma unroll 2
            for (int i = 0; i < 40; i += 4) {
                const f32x4 d4 = *reinterpret_cast<const f32x4 *>(g_dt + g0 + i);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float x = d4[u] * wc;
                    xmax = fmaxf(xmax, fabsf(x));
                    dst[(size_t)(i + u) * lda] = time_cosf_fast(x);          // cos(t*w + 0); wc = 0 in the padding: 1 -> fixed below
                }
            }
            if (!is_cos) {
                for (int i = 0; i < 40; ++i) dst[(size_t)i * lda] = 0.f;
            } else if (!(xmax < 4.0e6f)) {
                for (int i = 0; i < 40; ++i) dst[(size_t)i * lda] = time_cosf(g_dt[g0 + i] * wc);
            }
        }
    }
    AGG_STAMP(2);
    AGG_STAMP(3);
    __syncthreads();
    AGG_STAMP(4);

    // ---- fc1 on f32 MFMA ----
    {
        const float *bp = W1p + (size_t)col0 * K1p + 4 * g4;
        const int K4 = (F + T + 3) & ~3, nchunk = K4 >> 4, nrem = (K4 & 15) >> 2;
        if (wave < 3) d100_mfma<2>(A, lda, bp, K1p, nchunk, nrem, r16, g4, acc);
        else          d100_mfma<1>(A, lda, bp, K1p, nchunk, nrem, r16, g4, acc);
    }
    AGG_STAMP(5);
    __syncthreads();   // every wave is done reading the A tile: reuse it for the hidden rows

    // ---- bias + ReLU + weight, staged as Hs[g][col] in the A region ----
    float *Hs = A;
    {
        float *hp = Hs + (size_t)(g4 * 4) * LDH + col0;
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wnn + a * 16 + g4 * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = acc[a][0][j] + bias0;
                v = v > 0.f ? v : 0.f;
                hp[(size_t)(a * 16 + j) * LDH] = v * w4[j];
            }
        }
        if (wave < 3) {
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wnn + a * 16 + g4 * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v1 = acc[a][1][j] + bias1;
                    v1 = v1 > 0.f ? v1 : 0.f;
                    hp[(size_t)(a * 16 + j) * LDH + 64] = v1 * w4[j];
                }
            }
        }
    }
    __syncthreads();
    AGG_STAMP(6);
    // ---- reduce over the k neighbours of each query row ----
    if (cc < D) {
        for (int q = tid >> 7; q < nq; q += 2) {
            const float *hq = Hs + (size_t)(q * KK) * LDH + cc;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KK; ++j) s += hq[(size_t)j * LDH];
            H[((size_t)m * N + q0 + q) * D + cc] = s;
        }
    }
    AGG_STAMP(7);
}

// ---------------------------------------------------------------------------
// k_fc1_agg_reg<KK>: the same computation for the shapes the headline configurations run (D = T = 100, F <= 4
// so that F + T <= 104, k in {20, 40}), built around the matrix pipe instead of around a workgroup's LDS tile:
//   * PERSISTENT waves, each one on its own: a wave owns 80 gathered rows (4 or 2 whole query rows) x all 7 N-tiles
//     of the hidden layer; no workgroup barrier anywhere, nothing but 1.3 KB of per-row scalars in LDS;
//   * fc1's [ef | time] weights stay in REGISTERS for the whole launch (7 N-tiles x 26 k-steps = 182 per lane, one
//     wave per SIMD: 512 registers) -- the MFMA's B operand never touches memory again;
//   * the A operand is never staged either: MFMA 16x16x4 wants A[row = lane & 15][k = 4 s + (lane >> 4)] from each
//     lane, which is cos(dt[row] * w_time[k]) -- the lane evaluates exactly that (one cosine per 7 MFMAs) while the
//     matrix pipe works on the previous step (an MFMA holds the SIMD's vector issue for 8 of its 32 cycles);
//   * the projected rows P[nbr] (fc1 is linear: W_m memory[nbr], see k_fc1_agg) are added in the epilogue of each
//     16-row M-tile, their loads issued when the M-tile starts;
//   * bias + ReLU + w / sum(w) and the reduction over the k neighbours of a query row happen in registers: k is a
//     multiple of 4, so the 4 rows a lane holds of an M-tile belong to one query row; partial sums per (query
//     row, N-tile) are combined across the four 16-lane groups with two cross-lane adds at the end of the tile.
// Time encoding: every argument goes through time_cosf_rev (below), whose reduction is exact enough for any dt the
// stream produces: arguments beyond 4e6 (old neighbours: dt is seconds) are everyday data at stream scale.
// ---------------------------------------------------------------------------
#ifdef ZT_DIAG
__device__ unsigned long long g_regclk[4 * 1024];   // diagnostic builds (-DZT_DIAG, tools/build_diag.sh): per wave: shader cycles, wall start, wall end (100 MHz), tiles
#endif
constexpr int REG_NS = 26;       // MFMA k-steps: F + T <= 104
constexpr int REG_NB = 7;        // N-tiles of the hidden layer (D = 100 -> 112 columns)
constexpr int REG_FRAG_GROUPS = (REG_NB * REG_NS + 3) / 4;      // the weights in fragment order: groups of four values per lane

// fc1's [ef | time] block ([112][K2p], zero padded) in the order the lanes of k_fc1_agg_reg hold it: value q = 26 b + st
// of lane (r16, g4) is W[16 b + r16][4 st + g4]; image[q / 4][lane][q % 4]
__global__ void k_pack_reg_frag(const float *__restrict__ W1t, int K2p, float *__restrict__ image)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= REG_FRAG_GROUPS * 64 * 4) return;
    const int e = i & 3, lane = (i >> 2) & 63, G = i >> 8;
    const int q = 4 * G + e, b = q / REG_NS, st = q % REG_NS;
    image[i] = q < REG_NB * REG_NS ? W1t[(16 * b + (lane & 15)) * K2p + 4 * st + (lane >> 4)] : 0.f;
}

template <int KK, int DBG = 0>     // DBG != 0: only instantiated in diagnostic builds (-DZT_DIAG + ZT_AGG_DBG; WRONG results: 1 no cosine, 2 bare epilogue, 4 no projected rows)
__global__ __launch_bounds__(AGG_THREADS, 1) void k_fc1_agg_reg(
    const float *__restrict__ P, const float *__restrict__ efeat, const float *__restrict__ time_w, long long num_nodes,
    long long num_edges, int F, long long N, int M, const int *__restrict__ nbr, const int *__restrict__ eix,
    const float *__restrict__ dt, const float *__restrict__ w, const float *__restrict__ Wfrag,
    const float *__restrict__ b1, float *__restrict__ H, float *__restrict__ S, int *status,
    const int *gate_word, int gate_target, int *gate_latch)
{
    constexpr int D = 100, T = 100, DP = 112, ROWS = 80, RQ = ROWS / KK;
    static_assert(KK % 4 == 0 && ROWS % KK == 0, "groups of 4 rows must not straddle query rows");
    __shared__ int s_nb[AGG_WAVES][ROWS];
    __shared__ __attribute__((aligned(16))) float s_dt[AGG_WAVES][ROWS];
    __shared__ __attribute__((aligned(16))) float s_w[AGG_WAVES][ROWS];
    __shared__ float s_sum[AGG_WAVES][4];
    __shared__ __attribute__((aligned(16))) float s_ef[AGG_WAVES][ROWS * 4];      // edge-feature columns k < F <= 4 of every row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    int *nb_s = s_nb[wave];
    float *dt_s = s_dt[wave], *w_s = s_w[wave], *sum_s = s_sum[wave], *ef_s = s_ef[wave];
#ifdef ZT_DIAG
    const unsigned long long wall_in = DBG ? __builtin_amdgcn_s_memrealtime() : 0ull;
#endif

    // ---- once per launch: this lane's slice of the weights, the time frequencies and the biases ----
    // The 182 values a lane needs come from an image in FRAGMENT order (k_pack_reg_frag: [46 groups][64 lanes][4]): 46
    // coalesced 16-byte loads per lane, every wave of the launch reading the same 47 KB from L2.  (Round 3 staged the
    // [112][112] matrix through LDS and picked the values with 182 four-byte reads at a stride that puts sixteen lanes on
    // two banks: 10.6 us from kernel entry to the first tile -- 12 % of the kernel at C4's batch.)
    float Breg[REG_NB][REG_NS];
    {
        const f32x4 *Wf = reinterpret_cast<const f32x4 *>(Wfrag) + lane;
        static_assert(REG_FRAG_GROUPS % 2 == 0, "two batches");
        constexpr int HB = REG_FRAG_GROUPS / 2;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            // (all loads of a batch in flight before the first register write: the accumulator-register writes are volatile
            //  asm, and left alone the compiler issues load, wait, four writes, load, wait ... -- 46 L2 round trips in a row)
            f32x4 v[HB];
#pragma unroll
            for (int i = 0; i < HB; ++i) v[i] = Wf[(half * HB + i) * 64];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < HB; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = 4 * (half * HB + i) + e;
                    // defined by an accumulator-register write: the value then LIVES in the accumulator half of the register
                    // file (an MFMA takes its B operand from either half); left to itself the allocator keeps all 182 in
                    // vector registers, runs out of them and spills
                    if (q < REG_NB * REG_NS) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(Breg[q / REG_NS][q % REG_NS]) : "v"(v[i][e]));
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    float freq[REG_NS];
#pragma unroll
    for (int st = 0; st < REG_NS; ++st) {
        const int kc = 4 * st + g4 - F;
        freq[st] = (kc >= 0 && kc < T) ? time_w[kc] : 0.f;
    }
    float bias[REG_NB];
#pragma unroll
    for (int b = 0; b < REG_NB; ++b) bias[b] = (16 * b + r16) < D ? b1[16 * b + r16] : 0.f;

#ifdef ZT_DIAG
    const unsigned long long clk0 = DBG ? __builtin_amdgcn_s_memtime() : 0ull, wall0 = DBG ? __builtin_amdgcn_s_memrealtime() : 0ull;
#endif
    const long long tpm = (N + RQ - 1) / RQ;                           // tiles per model
    const long long n_tiles = tpm * M;
    const long long stride = (long long)gridDim.x * AGG_WAVES;
    long long tile = (long long)blockIdx.x * AGG_WAVES + wave;

    // per-row scalars of a tile: lane l holds rows l and (l < 16) 64 + l; fetched one tile ahead
    int pf_nb[2] = {0, 0}, pf_ei[2] = {0, 0};
    float pf_dt[2] = {0.f, 0.f}, pf_w[2] = {0.f, 0.f};
    auto fetch = [&](long long t) {
        const long long m = t / tpm, q0 = (t - m * tpm) * RQ;
        const int rows = (int)((N - q0) < RQ ? (N - q0) : RQ) * KK;
        const size_t mb = ((size_t)m * N + q0) * KK;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h * 64 + lane;
            const bool in = row < rows && (h == 0 || lane < ROWS - 64);
            pf_nb[h] = in ? nbr[mb + row] : 0;
            pf_ei[h] = in ? eix[mb + row] : 0;
            pf_dt[h] = in ? dt[mb + row] : 0.f;
            pf_w[h] = in ? w[mb + row] : 0.f;
        }
    };
    // ... and, once those edge ids are there, the rows' edge features (second stage, half a tile later)
    float pf_ef[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    auto fetch_ef = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ei = pf_ei[h];
            const bool ok = ei >= 0 && ei < num_edges && (h == 0 || lane < ROWS - 64);
#pragma unroll
            for (int c = 0; c < 4; ++c) pf_ef[h][c] = (ok && c < F) ? efeat[(size_t)ei * F + c] : 0.f;
        }
    };
    // the T-PPR rows of this batch may still be on their way (a launch group released batch by batch: common.hpp,
    // member_gate): the weights above were requested first, the wait is behind them
    member_gate_enter(gate_word, gate_target, status, gate_latch);
    if (tile < n_tiles) { fetch(tile); fetch_ef(); }

#pragma nounroll
    for (; tile < n_tiles; tile += stride) {
        const long long m = tile / tpm, q0 = (tile - m * tpm) * RQ;
        const int nq = (int)((N - q0) < RQ ? (N - q0) : RQ);
        // ---- this tile's scalars: registers -> LDS (the previous tile is done with the buffer) ----
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h * 64 + lane;
            if (h == 0 || lane < ROWS - 64) {
                int nb = pf_nb[h], ei = pf_ei[h];
                if (nb < 0 || nb >= num_nodes || ei < 0 || ei >= num_edges) { atomicExch(status, ZT_ERR_RANGE); nb = 0; ei = 0; }
                nb_s[row] = nb; dt_s[row] = pf_dt[h]; w_s[row] = pf_w[h];
                *reinterpret_cast<f32x4 *>(ef_s + 4 * row) = f32x4{pf_ef[h][0], pf_ef[h][1], pf_ef[h][2], pf_ef[h][3]};
            }
        }
        wave_sync();
        if (lane < RQ) {                                               // sum(w) in entry order, like torch.sum(dim=1)
            // (KK / 4 sixteen-byte reads, all in flight, then the adds in entry order: twenty dependent four-byte reads cost
            //  ~1 500 cycles per tile with nothing beside them)
            f32x4 wv[KK / 4];
#pragma unroll
            for (int j = 0; j < KK / 4; ++j) wv[j] = *reinterpret_cast<const f32x4 *>(w_s + lane * KK + 4 * j);
            float sm = 0.f;
#pragma unroll
            for (int j = 0; j < KK; ++j) sm += wv[j / 4][j % 4];
            sum_s[lane] = sm;
            if (lane < nq) S[(size_t)m * N + q0 + lane] = (sm == 0.f) ? 0.f : 1.f;
        }
        wave_sync();
        // w / sum(w), 0 where the sum is 0 (:267-270): once per row here, not once per use in the M-tiles
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h * 64 + lane;
            if (h == 0 || lane < ROWS - 64) {
                const float qs = sum_s[row / KK];
                w_s[row] = (qs == 0.f) ? 0.f : pf_w[h] / qs;
            }
        }
        wave_sync();
        const bool has_next = tile + stride < n_tiles;
        if (has_next) fetch(tile + stride);                             // in flight while this tile computes

        float Hloc[RQ][REG_NB];
#pragma unroll
        for (int q = 0; q < RQ; ++q)
#pragma unroll
            for (int b = 0; b < REG_NB; ++b) Hloc[q][b] = 0.f;

        // Software pipeline over the five M-tiles (16 rows each): while the matrix pipe runs M-tile a, the vector
        // unit evaluates the NEXT k-step's cosine and, during the first seven steps, the epilogue of M-tile a - 1 (one
        // N-tile per step) from a copy of its accumulators taken at the boundary; the projected rows of M-tile a are
        // requested at step 7, once that epilogue is through with the previous ones (one register set), and used
        // twenty steps later.  A sixth round drains the last epilogue.  sched_barrier between steps keeps the compiler
        // from hoisting five M-tiles' worth of loads and cosines to the top.  Register budget: accumulator half 182
        // weights + 28 accumulators; vector half ~180.
        f32x4 acc[REG_NB];
        float accv[REG_NB][4], Pv[2][REG_NB][4], wn_cur[4], wn_prv[4];
        // the projected rows of M-tile x into register set x & 1: requested TWO M-tiles ahead of their epilogue (a wave
        // has its SIMD to itself: nothing else hides a 2-4 us gather from a multi-gigabyte table)
        auto load_P = [&](int x) {
            const int4 nb4 = *reinterpret_cast<const int4 *>(nb_s + x * 16 + 4 * g4);         // epilogue rows 4 g4 + j
            const float *p0 = P + (size_t)nb4.x * DP + r16, *p1 = P + (size_t)nb4.y * DP + r16,
                        *p2 = P + (size_t)nb4.z * DP + r16, *p3 = P + (size_t)nb4.w * DP + r16;
#pragma unroll
            for (int b = 0; b < REG_NB; ++b) {
                Pv[x & 1][b][0] = p0[16 * b]; Pv[x & 1][b][1] = p1[16 * b]; Pv[x & 1][b][2] = p2[16 * b]; Pv[x & 1][b][3] = p3[16 * b];
            }
        };
        if (!(DBG & 4)) { load_P(0); load_P(1); }
#pragma unroll
        for (int a = 0; a <= 5; ++a) {
            float dta = 0.f, A_next[2] = {0.f, 0.f};
            if (a > 0) {
#pragma unroll
                for (int b = 0; b < REG_NB; ++b)
#pragma unroll
                    for (int j = 0; j < 4; ++j) accv[b][j] = acc[b][j];
#pragma unroll
                for (int j = 0; j < 4; ++j) wn_prv[j] = wn_cur[j];
            }
            if (a < 5) {
                // ---- M-tile a: rows 16 a .. 16 a + 15 ----
                dta = dt_s[a * 16 + r16];                              // A operand: row r16 of the M-tile
                const float ef = ef_s[4 * (a * 16 + r16) + (g4 & 3)];  // k = g4 < F: an edge-feature column
                const f32x4 w4 = *reinterpret_cast<const f32x4 *>(w_s + a * 16 + 4 * g4);   // already w / sum(w)
#pragma unroll
                for (int j = 0; j < 4; ++j) wn_cur[j] = w4[j];
#pragma unroll
                for (int b = 0; b < REG_NB; ++b) acc[b] = f32x4{bias[b], bias[b], bias[b], bias[b]};     // C operand of the first MFMA
                A_next[0] = (DBG & 1) ? dta * freq[0] : time_cosf_rev(dta * freq[0]);
                A_next[1] = (DBG & 1) ? dta * freq[1] : time_cosf_rev(dta * freq[1]);
                if (g4 < F) A_next[0] = ef;
                if (a == 2 && has_next) fetch_ef();                    // the next tile's edge ids have arrived by now
            }
            __builtin_amdgcn_sched_barrier(0);
            // query rows M-tile a - 1 touches (constants once unrolled)
            const int ap = a > 0 ? a - 1 : 0;
            const int q_lo = (16 * ap) / KK, q_hi = (16 * ap + 15) / KK;
            // Two k-steps at a time: 14 MFMAs, the cosines of the NEXT two steps (two independent chains: the f32 MFMA
            // keeps vector instructions off the SIMD while it runs, so what counts is that they issue back to back
            // once they do run) and, in the first rounds, two slices of the previous M-tile's epilogue.
#pragma unroll
            for (int st0 = 0; st0 < REG_NS; st0 += 2) {
                if (a == 5 && st0 >= REG_NB) break;
                const float A_cur[2] = {A_next[0], A_next[1]};
                if (a < 5) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        if (st0 + 2 + u < REG_NS)
                            A_next[u] = (DBG & 1) ? dta * freq[st0 + 2 + u] : time_cosf_rev(dta * freq[st0 + 2 + u]);
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int b = 0; b < REG_NB; ++b)
                            acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(A_cur[u], Breg[b][st0 + u], acc[b], 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int st = st0 + u;
                    if (!(a > 0 && st < REG_NB)) continue;
                    // epilogue of M-tile a - 1, N-tile st: + projected row (the bias went in as the MFMAs' C operand),
                    // ReLU, x w / sum(w); the lane's 4 rows belong to ONE query row
                    const int b = st;
                    float part = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float v = accv[b][j] + ((DBG & 2) ? 0.f : Pv[ap & 1][b][j]);
                        v = v > 0.f ? v : 0.f;
                        part += (DBG & 2) ? v : v * wn_prv[j];
                    }
                    if (DBG & 2) {
                        Hloc[q_lo][b] += part;
                    } else {
                        // The four 16-lane groups hold rows 4 g .. 4 g + 3 of the M-tile.  Every lane gets all four partial
                        // sums (two half-wave swaps + two row swaps, no LDS) and adds them to their query rows in ROW order:
                        // a query row's k / 4 groups are then always summed first to last, wherever in a tile the row falls
                        // -- a row's value must not depend on which shard or tile it is computed in.
                        const int pi = __float_as_int(part);
                        const auto h = __builtin_amdgcn_permlane32_swap(pi, pi, false, false);       // [0]: groups 0,1,0,1   [1]: 2,3,2,3
                        const auto lo = __builtin_amdgcn_permlane16_swap(h[0], h[0], false, false);  // [0]: group 0 everywhere, [1]: group 1
                        const auto hi = __builtin_amdgcn_permlane16_swap(h[1], h[1], false, false);  // [0]: group 2, [1]: group 3
                        const float pg[4] = {__int_as_float(lo[0]), __int_as_float(lo[1]), __int_as_float(hi[0]), __int_as_float(hi[1])};
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int q = (16 * ap + 4 * g) / KK;                   // constant once unrolled
                            if (q < RQ) Hloc[q][b] += pg[g];
                        }
                    }
                    // (an empty side-effecting statement: it pins this arithmetic to THIS round.  Nothing else orders pure
                    //  vector work against the scheduling barriers, and instruction selection otherwise sinks all five
                    //  epilogues to the end of the tile, where their inputs -- 5 x 60 registers -- are still alive)
                    asm volatile("" : "+v"(Hloc[q_lo][b]));
                    if (q_hi != q_lo && q_hi < RQ) asm volatile("" : "+v"(Hloc[q_hi][b]));
                }
                if (a >= 1 && a <= 3 && st0 == REG_NB + 1 && !(DBG & 4)) load_P(a + 1);   // its register set has just been released
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- every lane holds every sum: group g writes query row g ----
#pragma unroll
        for (int q = 0; q < RQ; ++q) {
            if (g4 == (q & 3) && q < nq) {
                float *hrow = H + ((size_t)m * N + q0 + q) * D;
#pragma unroll
                for (int b = 0; b < REG_NB; ++b)
                    if (16 * b + r16 < D) hrow[16 * b + r16] = Hloc[q][b];
            }
        }
        wave_sync();                                                   // all reads of the scalar buffer are done
    }
#ifdef ZT_DIAG
    if (DBG && lane == 0 && blockIdx.x * AGG_WAVES + wave < 1024) {
        unsigned long long *o = g_regclk + 4 * (blockIdx.x * AGG_WAVES + wave);
        o[0] = __builtin_amdgcn_s_memtime() - clk0; o[1] = wall0; o[2] = __builtin_amdgcn_s_memrealtime();
        o[3] = wall_in;                                                         // (100 MHz) at kernel entry: the weight fill is wall0 - this
    }
#endif
}


// ---------------------------------------------------------------------------
// k_embed_out3: the persistent output layers (embed_out_body.hpp: eo3_src_body, eo3_nbr_body) in one grid -- workgroups
// [0, n_src) take the source path, the others fc2 of the M models.  k_embed_src3 / k_embed_nbr3: one path each, for a caller
// that holds the neighbour paths back for the GRU update's launch (embed_ex: `defer`; k_nbr_gru, memory_update.hip) -- the
// neighbour-only launch is what such a caller falls back to where no GRU kernel takes them along.
// ---------------------------------------------------------------------------
template <int HG>
__global__ __launch_bounds__(AGG_THREADS, 1) void k_embed_out3(EmbedOutArgs E, int n_src)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if ((int)blockIdx.x < n_src) eo3_src_body(E, smem, blockIdx.x, n_src);
    else eo3_nbr_body<HG, AGG_WAVES, EO3_NT>(E, smem, (int)blockIdx.x - n_src, (int)gridDim.x - n_src);
}

__global__ __launch_bounds__(AGG_THREADS, 1) void k_embed_src3(EmbedOutArgs E)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    eo3_src_body(E, smem, blockIdx.x, gridDim.x);
}

// (plain rows only: the neighbour paths are never held back where H holds partial-sum groups, KernelPlan::nbr_later)
__global__ __launch_bounds__(AGG_THREADS, 1) void k_embed_nbr3(EmbedOutArgs E)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    eo3_nbr_body<1, AGG_WAVES, EO3_NT>(E, smem, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------
// Projected memory table: P[v][0..Dp) = W_m memory[v] (W_m = the memory columns of fc1, zero padded to
// [Dp][Dp]; columns >= D of P are zero).  rows == nullptr: every node; else the n rows listed (ids < 0 or
// beyond *count are skipped): the rows a batch's GRU update / exchange has just rewritten.
// ---------------------------------------------------------------------------
template <int NW = NTW>
__global__ __launch_bounds__(AGG_THREADS) void k_project_rows(const float *__restrict__ memory, long long num_nodes,
                                                              int D, const float *__restrict__ Wm_p,
                                                              const int *__restrict__ rows, const int *__restrict__ count,
                                                              long long n_max, float *__restrict__ P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Dp = (D + 15) / 16 * 16, ldx = Dp + 4, NT = Dp / 16;
    float *X = reinterpret_cast<float *>(smem);          // [32][ldx]
    int *rid = reinterpret_cast<int *>(X + OUT_ROWS * ldx);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    const long long r0 = (long long)blockIdx.x * OUT_ROWS;
    long long n = n_max;
    if (count != nullptr) { const long long c = *count; n = c < n ? c : n; }
    if (r0 >= n) return;
    if (tid < OUT_ROWS) {
        long long v = -1;
        if (r0 + tid < n) v = rows != nullptr ? (long long)rows[r0 + tid] : r0 + tid;
        rid[tid] = (v >= 0 && v < num_nodes) ? (int)v : -1;
    }
    __syncthreads();
    const unsigned mL = fastdiv_magic((unsigned)ldx);
    for (int f = tid; f < OUT_ROWS * ldx; f += AGG_THREADS) {
        const int g = fastdiv(f, mL), c = f - g * ldx;
        X[f] = (rid[g] >= 0 && c < D) ? memory[(size_t)rid[g] * D + c] : 0.f;
    }
    __syncthreads();
    f32x4 acc[OUT_MT][NW];
    small_gemm(X, ldx, Wm_p, Dp, NT, wave, lane, acc);
#pragma unroll
    for (int b = 0; b < NW; ++b) {
        const int col = (wave + b * AGG_WAVES) * 16 + r16;
        if (col >= Dp) continue;
#pragma unroll
        for (int a = 0; a < OUT_MT; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = a * 16 + g4 * 4 + j;
                if (rid[g] >= 0) P[(size_t)rid[g] * Dp + col] = acc[a][b][j];
            }
    }
}

// The embed workspace for (N, D, F, T, M, k) and the tiles of k_fc1_agg (plan_kernels below picks the kernel)
struct EmbedPlan {
    int Dp, K1p, lda, mt, rq;                   // the [memory | ef | time] tile (mt = 0: none holds a query row)
    size_t lds;
    int K2p, lda2, mt2, rq2;                    // the projected table's [ef | time] tile (mt2 = 0: none)
    size_t lds2;
    size_t off_w1p, off_H, off_S, off_fc2t, off_fc1st, off_fc2st, off_w1t, off_wm, off_wl, off_wfrag, total;
    int hg;                                     // partial-sum groups per query row in H (k_fc1_agg_wide: k / 4; else 1)
};

// tile shape for a contraction over Kp columns: as many whole query rows as fit MAX_MT tiles / the LDS budget
bool tile_shape(int Kp, int Dp, int k, int T, int *lda_out, int *mt_out, int *rq_out, size_t *lds_out, int max_mt = MAX_MT)
{
    const int lda = Kp + 4;
    int mt = max_mt;
    while (mt > 1 && ((size_t)mt * 16 * lda * 4 + (size_t)mt * 16 * 16) > (size_t)AGG_LDS_BUDGET) --mt;
    int rq = (mt * 16) / k;
    if (rq < 1) {
        // one query row must fit: grow to ceil(k/16) tiles if the budget allows
        mt = (k + 15) / 16;
        rq = 1;
        if (mt > max_mt || ((size_t)mt * 16 * lda * 4 + (size_t)mt * 16 * 16) > (size_t)AGG_LDS_BUDGET) return false;
    }
    mt = (rq * k + 15) / 16;
    // the hidden staging [rows_p][Dp+1] reuses the A region: it must fit
    if ((size_t)mt * 16 * (Dp + 1) * 4 > (size_t)mt * 16 * lda * 4) return false;
    *lda_out = lda; *mt_out = mt; *rq_out = rq;
    *lds_out = (size_t)mt * 16 * lda * 4 + (size_t)mt * 16 * 16 + (size_t)T * 4;   // A tile + wn, nbr, eix, dt per row + time_w
    return true;
}

// the row split (aggregate_split.hip) takes a query row in chunks where no tile holds one
bool split_fits(int D, int F, int T, int k) { return k <= ZT_MAX_K_WIDE && fc1_agg_split_rows(D, F, T) > 0; }

bool make_plan(int64_t N, int D, int F, int T, int M, int k, EmbedPlan &p)
{
    if (!width_supported(D)) return false;
    const int K1 = D + F + T;
    p.Dp = round_up(D, 16);
    p.K1p = round_up(K1, 16);
    const bool big = k > MAX_MT * 16;           // the MAX_MT_BIG (wide D: MAX_MT_BIG_WIDE) instantiation
    const int max_mt = big ? (p.Dp > 16 * NTW * AGG_WAVES ? MAX_MT_BIG_WIDE : MAX_MT_BIG) : MAX_MT;
    const bool full_ok = tile_shape(p.K1p, p.Dp, k, T, &p.lda, &p.mt, &p.rq, &p.lds, max_mt);
    // no tile for a query row with its memory columns: the table path's narrower tile (wide k), or the row split
    if (!full_ok) { p.mt = 0; p.rq = 1; p.lda = p.K1p + 4; p.lds = 0; }
    p.K2p = round_up(F + T, 16);
    p.mt2 = 0;                                  // table path unavailable (e.g. F + T < D: the staging would not fit)
    if (!(full_ok || big) || !tile_shape(p.K2p, p.Dp, k, T, &p.lda2, &p.mt2, &p.rq2, &p.lds2, max_mt)) p.mt2 = 0;
    if (p.mt == 0 && p.mt2 == 0 && !split_fits(D, F, T, k)) return false;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    // padded weights first: their offsets depend on (D, F, T) only, so a workspace prepared once serves every N
    p.off_w1p = take((size_t)p.Dp * p.K1p * 4);
    p.off_fc2t = take((size_t)p.Dp * p.Dp * 4);
    p.off_fc1st = take((size_t)p.Dp * p.Dp * 4);
    p.off_fc2st = take((size_t)p.Dp * p.Dp * 4);
    p.off_w1t = take((size_t)p.Dp * p.K2p * 4);
    p.off_wm = take((size_t)p.Dp * p.Dp * 4);
    p.hg = fc1_agg_wide_supported(D, F, T, k) ? k / 4 : 1;
    p.off_wl = take(p.hg > 1 ? fc1_agg_wide_weight_bytes() : 0);
    p.off_wfrag = take((size_t)REG_FRAG_GROUPS * 64 * 4 * 4);      // k_fc1_agg_reg's weights in fragment order (K2p = 112 shapes)
    p.off_H = take((size_t)M * N * D * 4 * p.hg);
    p.off_S = take((size_t)M * N * 4);
    p.total = o;
    return true;
}

// embed_kernel_plan on the workspace layout p it makes
KernelPlan plan_kernels(int64_t N, int D, int F, int T, int M, int k, bool have_table, bool training, int agg_choice,
                        int out_choice, EmbedPlan &p)
{
    KernelPlan kp{AggKernel::unsupported, OutForm::tiled, Refusal::shape, 0, 0, 0, 0, 1, false};
    static_assert(16 * NTW * AGG_WAVES == 128 && 16 * NTW_WIDE * AGG_WAVES == MAX_D, "the N-tiles cover D <= 128 / D <= 256");
    if (!make_plan(N, D, F, T, M, k, p)) return kp;
    const bool big = k > MAX_MT * 16;
    const bool tab = have_table && !training && p.mt2 > 0;
    // the reference's default widths take the specialised kernels (zt_set_kernel_choice(ZT_CHOICE_AGGREGATE, ZT_AGG_GENERIC): the generic one)
    const bool special = tab && agg_choice != ZT_AGG_GENERIC;
    if (training ? (big || p.mt == 0) : (!tab && p.mt == 0)) {
        // a query row wider than any tile (training: than the 80-row one): the row split
        if (!split_fits(D, F, T, k)) { kp.refusal = Refusal::no_split; return kp; }
        kp.agg = AggKernel::split;
    } else if (special && p.hg > 1) {
        kp.agg = AggKernel::wide;               // F = 172, D = T = 100, k in {20, 40}: weights resident in LDS
    } else if (special && D == 100 && T == 100 && F <= 4 && (k == 20 || k == 40) && p.K2p == 112) {
        kp.agg = AggKernel::reg;                // register-resident weights
    } else if (special && D == 100 && T == 100 && p.mt2 == 5 && (k == 10 || k == 20 || k == 40)) {
        kp.agg = AggKernel::d100;
    } else if (tab) {
        kp.agg = big ? AggKernel::tiled_table_big : AggKernel::tiled_table;
    } else {
        kp.agg = big ? AggKernel::tiled_full_big : AggKernel::tiled_full;
    }
    if (kp.agg == AggKernel::d100 || kp.agg == AggKernel::tiled_table || kp.agg == AggKernel::tiled_table_big) {
        kp.lds = p.lds2; kp.rq = p.rq2; kp.mt = p.mt2; kp.lda = p.lda2;
    } else if (kp.agg == AggKernel::tiled_full || kp.agg == AggKernel::tiled_full_big) {
        kp.lds = p.lds; kp.rq = p.rq; kp.mt = p.mt; kp.lda = p.lda;
    }
    kp.hg = kp.agg == AggKernel::wide ? p.hg : 1;
    if (kp.hg != 1 && kp.hg != 5 && kp.hg != 10) { kp.agg = AggKernel::unsupported; kp.refusal = Refusal::groups; return kp; }
    kp.refusal = Refusal::none;
    // small batches: the latency-organised kernel (one wave per tile, path and N-tile; 1 - 2 memory round trips); large ones:
    // the persistent one (weights resident in LDS, a wave per 16 rows x all N-tiles); other widths: the tiled one (weights
    // streamed from L2 per 32-row workgroup).  zt_set_kernel_choice(ZT_CHOICE_EMBED_OUT, ..) pins one; the three give the
    // same results (tests/test_embed_gpu.py).
    // (alone on the chip, tools/exp/p23_kernels.py: 12 288 rows persist 26 us / tiled 32 / latency 53 -- 29 / 38 / 66 on 192 CUs;
    //  3 000 rows 17 / 18 / 23; 1 800 rows with partial-sum groups 19 / 17.5 / 22; 600 rows 16.5 / 17 / 12)
    //  In the pipeline the persistent workgroups (130 KB of LDS, a whole register file per wave) do not fit beside another
    //  stream's kernels: C4 (3 000 rows, no CU masks, k_pruned_topk running beside) 36 us against the tiled kernel's 20; C5
    //  (12 288 rows, the main stream's CUs to itself) 29 against 38.  So: from 8 192 rows on.
    // (ZT_OUT_WHOLE: the library's pick; ZT_OUT_NBR_GRU: the persistent form wherever it exists)
    const bool by_shape = out_choice == 0 || out_choice == ZT_OUT_WHOLE;
    if (D % 4 == 0 && (p.Dp == 112 || p.Dp == 128) && (out_choice == ZT_OUT_LATENCY || (by_shape && N <= 1024)))
        kp.out = OutForm::latency;
    else if (D % 4 == 0 && p.Dp == EO3_DP && (out_choice == ZT_OUT_PERSIST || out_choice == ZT_OUT_NBR_GRU || (by_shape && N >= 8192)))
        kp.out = OutForm::persist;
    // The persistent form's two halves share nothing, and only the source path reads the memory table: where the caller can
    // hold output layers back (the pipeline), the neighbour paths leave the chain aggregation -> output layers -> GRU update
    // and run in the GRU update's grid (k_nbr_gru, memory_update.hip).  Plain rows only (no partial-sum groups); a pinned
    // ZT_OUT_PERSIST stays what it was, k_embed_out3 whole.
    kp.nbr_later = kp.out == OutForm::persist && kp.hg == 1 && (out_choice == 0 || out_choice == ZT_OUT_NBR_GRU);
    return kp;
}

}  // namespace

KernelPlan zt::embed_kernel_plan(int64_t N, int D, int F, int T, int M, int k, bool have_table, bool training, int agg_choice,
                                 int out_choice)
{
    EmbedPlan p;
    return plan_kernels(N, D, F, T, M, k, have_table, training, agg_choice, out_choice, p);
}

#ifdef ZT_AGG_STAMP
extern "C" int zt_debug_agg(unsigned long long *host, int reset)
{
    ZT_HIP(hipDeviceSynchronize());
    ZT_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_agg), sizeof(unsigned long long) * 8));
    if (reset) { unsigned long long z[8] = {0}; ZT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_agg), z, sizeof(z))); }
    return ZT_OK;
}
#endif

#ifdef ZT_DIAG
extern "C" int zt_debug_regclk(unsigned long long *host)
{
    ZT_HIP(hipDeviceSynchronize());
    ZT_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_regclk), sizeof(unsigned long long) * 4 * 1024));
    return ZT_OK;
}
#endif

extern "C" int64_t zt_embed_workspace_bytes(int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k)
{
    EmbedPlan p;
    if (N < 0 || D <= 0 || F < 0 || T < 0 || M <= 0 || k <= 0) return -1;
    if (!make_plan(N > 0 ? N : 1, D, F, T, M, k, p)) return -1;
    return (int64_t)p.total;
}

extern "C" int32_t zt_agg_train_supported(int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k)
{
    if (N < 0 || D <= 0 || F < 0 || T < 0 || M <= 0 || k <= 0) return 0;
    EmbedPlan p;
    const KernelPlan kp = plan_kernels(N > 0 ? N : 1, D, F, T, M, k, false, true, 0, 0, p);
    return kp.refusal == Refusal::none && agg_backward_supported(D, F, T, k) ? 1 : 0;
}

// pads every weight matrix into the workspace (once per weight change: zt_embed's weights_ready = 0)
static void embed_prepare(const zt_embed_weights *wt, int D, int F, int T, const EmbedPlan &p, char *ws, hipStream_t s)
{
    const int K1 = D + F + T;
    auto pad = [&](const float *W, int ld, int c0, int cols, size_t off, int cols_p) {
        k_pad_matrix<<<(p.Dp * cols_p + 255) / 256, 256, 0, s>>>(W, ld, c0, D, cols, reinterpret_cast<float *>(ws + off), p.Dp, cols_p);
    };
    pad(wt->fc1_w, K1, 0, K1, p.off_w1p, p.K1p);
    pad(wt->fc2_w, D, 0, D, p.off_fc2t, p.Dp);
    pad(wt->fc1s_w, D, 0, D, p.off_fc1st, p.Dp);
    pad(wt->fc2s_w, D, 0, D, p.off_fc2st, p.Dp);
    pad(wt->fc1_w, K1, D, F + T, p.off_w1t, p.K2p);       // the [ef | time] columns of fc1 (table path)
    pad(wt->fc1_w, K1, 0, D, p.off_wm, p.Dp);             // W_m: the memory columns of fc1 (k_project_rows)
    if (p.hg > 1) fc1_agg_wide_pack(wt->fc1_w, wt->time_w, wt->fc1_b, reinterpret_cast<float *>(ws + p.off_wl), s);   // LDS image (aggregate_wide.hip)
    if (p.K2p == 112 && p.Dp == 112)
        k_pack_reg_frag<<<(REG_FRAG_GROUPS * 64 * 4 + 255) / 256, 256, 0, s>>>(reinterpret_cast<const float *>(ws + p.off_w1t), p.K2p,
                                                                          reinterpret_cast<float *>(ws + p.off_wfrag));
}

const float *zt::embed_wm_ptr(void *embed_ws, int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k)
{
    EmbedPlan p;
    if (!embed_ws || !make_plan(N > 0 ? N : 1, D, F, T, M, k, p)) return nullptr;
    return reinterpret_cast<const float *>(reinterpret_cast<char *>(embed_ws) + p.off_wm);
}

extern "C" int64_t zt_project_table_bytes(int64_t num_nodes, int32_t D)
{
    if (num_nodes <= 0 || D <= 0) return -1;
    return (int64_t)num_nodes * round_up(D, 16) * 4;
}

extern "C" int zt_project_memory(const float *memory_dev, int64_t num_nodes, int32_t D, int32_t F, int32_t T,
                                 const zt_embed_weights *wt, int32_t weights_ready, const int32_t *rows_dev,
                                 const int32_t *count_dev, int64_t max_rows, float *table_dev, void *workspace_dev,
                                 int64_t ws_N, int32_t ws_M, int32_t ws_k, void *stream)
{
    if (!memory_dev || !wt || !table_dev || !workspace_dev || num_nodes <= 0 || D <= 0 || F < 0 || T < 0 || max_rows < 0) {
        set_error("zt_project_memory: bad argument");
        return ZT_ERR_ARG;
    }
    EmbedPlan p;
    if (!make_plan(ws_N > 0 ? ws_N : 1, D, F, T, ws_M, ws_k, p)) {
        set_error("zt_project_memory: unsupported shape");
        return ZT_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace_dev);
    if (!weights_ready) embed_prepare(wt, D, F, T, p, ws, s);
    const long long n = rows_dev ? max_rows : num_nodes;
    if (n == 0) return ZT_OK;
    const size_t lds = (size_t)OUT_ROWS * (p.Dp + 4) * 4 + OUT_ROWS * 4;
    const auto project = p.Dp > 16 * NTW * AGG_WAVES ? k_project_rows<NTW_WIDE> : k_project_rows<NTW>;
    project<<<(unsigned)((n + OUT_ROWS - 1) / OUT_ROWS), AGG_THREADS, lds, s>>>(
        memory_dev, num_nodes, D, reinterpret_cast<const float *>(ws + p.off_wm), rows_dev, count_dev, n, table_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

// zt_embed; mid_wait (pipeline.hip): an event the stream is told to wait for BETWEEN the aggregation and the output layer
static int embed_impl(const float *memory_dev, const float *efeat_dev, int64_t num_nodes, int64_t num_edges,
                      int32_t D, int32_t F, int32_t T, const int32_t *nodes_dev, int64_t N, int32_t M, int32_t k,
                      const int32_t *nbr_dev, const int32_t *eix_dev, const float *dt_dev, const float *w_dev,
                      const zt_embed_weights *wt, float *out_dev, void *workspace_dev, int32_t *status_dev,
                      const float *proj_table_dev, int32_t weights_ready, void *stream, hipEvent_t mid_wait,
                      zt::embed_out_deferred *defer = nullptr, const zt::member_gate *gate = nullptr)
{
    if (defer) defer->valid = false;
    if (!memory_dev || !efeat_dev || !wt || !status_dev || N < 0 || D <= 0 || F < 0 || T < 0 || M <= 0 || k <= 0) {
        set_error("zt_embed: bad argument");
        return ZT_ERR_ARG;
    }
    if (N == 0) return ZT_OK;
    if (!nodes_dev || !nbr_dev || !eix_dev || !dt_dev || !w_dev || !out_dev || !workspace_dev) {
        set_error("zt_embed: NULL buffer");
        return ZT_ERR_ARG;
    }
    EmbedPlan p;
    const KernelPlan kp = plan_kernels(N, D, F, T, M, k, proj_table_dev != nullptr, false, kernel_choice(ZT_CHOICE_AGGREGATE),
                                       kernel_choice(ZT_CHOICE_EMBED_OUT), p);
    if (kp.refusal == Refusal::shape) {
        set_error("zt_embed: D=%d F=%d T=%d k=%d outside the supported shapes (D <= 128, or a multiple of 4 up to %d; one query "
                  "row of k neighbours must fit the %d KB LDS tile)", D, F, T, k, MAX_D, AGG_LDS_BUDGET / 1024);
        return ZT_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace_dev);
    float *H = reinterpret_cast<float *>(ws + p.off_H);
    float *S = reinterpret_cast<float *>(ws + p.off_S);
    if (!weights_ready) {
        ZT_PROF_BEGIN(s, P_EMBED_PREP);
        embed_prepare(wt, D, F, T, p, ws, s);
        ZT_PROF_END(s, P_EMBED_PREP);
    }
    if (kp.refusal == Refusal::no_split) {
        set_error("zt_embed: k=%d needs the projected table (a query row's [memory | ef | time] tile does not fit %d KB of LDS, "
                  "nor does a chunk of it)", k, AGG_LDS_BUDGET / 1024);
        return ZT_ERR_UNSUPPORTED;
    }
    if (kp.refusal == Refusal::groups) { set_error("zt_embed: %d partial-sum groups per row", kp.hg); return ZT_ERR_UNSUPPORTED; }
    // (a wait for this batch's T-PPR rows: inside the two persistent kernels, a one-wave kernel in front of the others)
    const bool waits_inside = kp.agg == AggKernel::wide || kp.agg == AggKernel::reg;
    if (gate != nullptr && gate->word != nullptr && !waits_inside) {
        const int rc = zt::member_gate_launch(*gate, status_dev, s);
        if (rc != ZT_OK) return rc;
    }
    const dim3 tile_grid((unsigned)(kp.rq > 0 ? (N + kp.rq - 1) / kp.rq : 0), (unsigned)M);
    const bool wide = p.Dp > 16 * NTW * AGG_WAVES;     // the NTW_WIDE instantiations (128 < D <= 256)
    // the general kernels' arguments: the full [memory | ef | time] tile of the stored memory, no overlay, no dropout
    FcAggArgs fa{};
    fa.memory = memory_dev; fa.efeat = efeat_dev; fa.time_w = wt->time_w;
    fa.num_nodes = num_nodes; fa.num_edges = num_edges; fa.N = N;
    fa.D = D; fa.F = F; fa.T = T; fa.M = M; fa.k = k; fa.ldm = D;
    fa.nbr = nbr_dev; fa.eix = eix_dev; fa.dt = dt_dev; fa.w = w_dev;
    fa.W1p = reinterpret_cast<const float *>(ws + p.off_w1p); fa.K1p = p.K1p; fa.b1 = wt->fc1_b;
    fa.H = H; fa.S = S; fa.status = status_dev;
    fa.set_dropout(0.f, 0ull);
    // k_fc1_agg over the plan's tile, of memory rows or (table) of the projected table's: row stride Dp, the [ef | time] weights
    auto tiled = [&](decltype(&k_fc1_agg<false>) fn, bool table) {
        FcAggArgs ta = fa;
        if (table) { ta.memory = proj_table_dev; ta.ldm = p.Dp; ta.W1p = reinterpret_cast<const float *>(ws + p.off_w1t); ta.K1p = p.K2p; }
        ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(fn), kp.lds));
        fn<<<tile_grid, AGG_THREADS, kp.lds, s>>>(ta, kp.rq, kp.mt, kp.lda);
        return ZT_OK;
    };
    // k_fc1_agg_reg: persistent, one workgroup (4 waves) per CU
    auto reg = [&](decltype(&k_fc1_agg_reg<20>) fn) {
        const long long rq = 80 / k, tiles = ((N + rq - 1) / rq) * M;
        long long wgs = (tiles + AGG_WAVES - 1) / AGG_WAVES;
        const int cus = stream_cu_count(s);
        if (wgs > cus) wgs = cus;
        fn<<<(unsigned)wgs, AGG_THREADS, 0, s>>>(proj_table_dev, efeat_dev, wt->time_w, num_nodes, num_edges, F, N, M, nbr_dev, eix_dev,
                                                 dt_dev, w_dev, reinterpret_cast<const float *>(ws + p.off_wfrag), wt->fc1_b, H, S,
                                                 status_dev, gate ? gate->word : nullptr, gate ? gate->target : 0,
                                                 gate ? gate->latch : nullptr);
        return ZT_OK;
    };
    ZT_PROF_BEGIN(s, P_FC1_AGG);
    int rc = ZT_OK;
    switch (kp.agg) {
    case AggKernel::wide:
        rc = fc1_agg_wide_launch(proj_table_dev, efeat_dev, wt->time_w, num_nodes, num_edges, N, M, k, nbr_dev, eix_dev, dt_dev,
                                 w_dev, reinterpret_cast<const float *>(ws + p.off_wl), wt->fc1_b, H, S, status_dev,
                                 stream_cu_count(s), s, gate);
        break;
    case AggKernel::reg:
#ifdef ZT_DIAG
        {
            // diagnostic variants of k = 20 (wrong results; 8: all parts, with the per-wave clocks)
            static const int dbg = getenv("ZT_AGG_DBG") ? atoi(getenv("ZT_AGG_DBG")) : 0;
            if (k == 20 && dispatch<1, 2, 6, 7, 8>(dbg, [&](auto DB) { return reg(k_fc1_agg_reg<20, DB>); }) == ZT_OK) break;
        }
#endif
        rc = dispatch<20, 40>(k, [&](auto KK) { return reg(k_fc1_agg_reg<KK>); });
        break;
    case AggKernel::d100:
        rc = dispatch<10, 20, 40>(k, [&](auto KK) {
            ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_fc1_agg_d100<KK>), kp.lds));
            k_fc1_agg_d100<KK><<<tile_grid, AGG_THREADS, kp.lds, s>>>(proj_table_dev, efeat_dev, wt->time_w, num_nodes, num_edges, F, N,
                                                                     kp.lda, nbr_dev, eix_dev, dt_dev, w_dev,
                                                                     reinterpret_cast<const float *>(ws + p.off_w1t), p.K2p, wt->fc1_b,
                                                                     H, S, status_dev);
            return ZT_OK;
        });
        break;
    case AggKernel::tiled_table: rc = tiled(wide ? k_fc1_agg<true, MAX_MT, NTW_WIDE> : k_fc1_agg<true>, true); break;
    case AggKernel::tiled_table_big: rc = tiled(wide ? k_fc1_agg<true, MAX_MT_BIG_WIDE, NTW_WIDE> : k_fc1_agg<true, MAX_MT_BIG>, true); break;
    case AggKernel::tiled_full: rc = tiled(wide ? k_fc1_agg<false, MAX_MT, NTW_WIDE> : k_fc1_agg<false>, false); break;
    case AggKernel::tiled_full_big: rc = tiled(wide ? k_fc1_agg<false, MAX_MT_BIG_WIDE, NTW_WIDE> : k_fc1_agg<false, MAX_MT_BIG>, false); break;
    case AggKernel::split: rc = fc1_agg_split_launch(fa, s); break;
    case AggKernel::unsupported: break;               // (refused above)
    }
    if (rc != ZT_OK) return rc;
    ZT_PROF_END(s, P_FC1_AGG);
    if (mid_wait != nullptr) ZT_HIP(hipStreamWaitEvent(s, mid_wait, 0));
    const EmbedOutArgs E{memory_dev, num_nodes, nodes_dev, N, D, M, H, S,
                         reinterpret_cast<const float *>(ws + p.off_fc2t), wt->fc2_b,
                         reinterpret_cast<const float *>(ws + p.off_fc1st), wt->fc1s_b,
                         reinterpret_cast<const float *>(ws + p.off_fc2st), wt->fc2s_b, out_dev, status_dev};
    const long long tiles = (N + 15) / 16;
    zt::embed_out_deferred od{true, E, kp.hg, kp.out, kp.out == OutForm::latency ? (int)(tiles < 256 ? tiles : 256) : 0, nullptr};
    if (defer != nullptr && kp.out == OutForm::persist && kp.nbr_later) {
        // the source path by itself, here: it reads the memory rows the GRU update rewrites, and nothing of the aggregation's.
        // One persistent workgroup per compute unit of the stream, as many as there are four-wave loads of 16-row tiles.
        long long wgs = zt::stream_cu_count(s);
        if (defer->max_wgs > 0 && wgs > defer->max_wgs) wgs = defer->max_wgs;
        if (wgs > (tiles + AGG_WAVES - 1) / AGG_WAVES) wgs = (tiles + AGG_WAVES - 1) / AGG_WAVES;
        ZT_PROF_BEGIN(s, P_EMBED_OUT);
        ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_embed_src3), EO3_SRC_LDS));
        k_embed_src3<<<(unsigned)wgs, AGG_THREADS, EO3_SRC_LDS, s>>>(E);
        ZT_PROF_END(s, P_EMBED_OUT);
        od.form = OutForm::persist_nbr;          // what is left: handed on below
    }
    if (defer != nullptr && od.form != OutForm::persist) {
        // held back: the caller launches them beside the GRU update (gru_update_ex) -- or by embed_out_launch
        int *latch = defer->latch;
        const int max_wgs = defer->max_wgs;
        *defer = od;
        defer->latch = latch;
        defer->max_wgs = max_wgs;
        ZT_LAUNCH_CHECK();
        return ZT_OK;
    }
    ZT_PROF_BEGIN(s, P_EMBED_OUT);
    rc = zt::embed_out_launch(od, s);
    if (rc != ZT_OK) return rc;
    ZT_PROF_END(s, P_EMBED_OUT);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_embed(const float *memory_dev, const float *efeat_dev, int64_t num_nodes, int64_t num_edges,
                        int32_t D, int32_t F, int32_t T, const int32_t *nodes_dev, int64_t N, int32_t M, int32_t k,
                        const int32_t *nbr_dev, const int32_t *eix_dev, const float *dt_dev, const float *w_dev,
                        const zt_embed_weights *wt, float *out_dev, void *workspace_dev, int32_t *status_dev,
                        const float *proj_table_dev, int32_t weights_ready, void *stream)
{
    return embed_impl(memory_dev, efeat_dev, num_nodes, num_edges, D, F, T, nodes_dev, N, M, k, nbr_dev, eix_dev, dt_dev, w_dev,
                      wt, out_dev, workspace_dev, status_dev, proj_table_dev, weights_ready, stream, nullptr);
}

int zt::embed_out_launch(const zt::embed_out_deferred &d, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const EmbedOutArgs &E = d.args;
    const int Dp = round_up(E.D, 16);
    int rc;
    if (d.form == OutForm::latency) {
        // one wave per (16 rows, path, N-tile), striding over the row tiles with its weights in registers
        const dim3 grid2((unsigned)d.gx, (unsigned)(E.M + 1), (unsigned)(Dp / 16));
        rc = dispatch<7, 8>(Dp / 16, [&](auto NTV) {
            return dispatch<1, 5, 10>(d.hg, [&](auto HGV) { k_embed_out2<NTV, HGV><<<grid2, 64, 0, s>>>(E); return ZT_OK; });
        });
    } else if (d.form == OutForm::persist) {
        // one workgroup per CU of the stream; the source path's two layers are as many MFMAs per row as M models' fc2
        const long long tiles = (E.N + 15) / 16;
        long long wgs = zt::stream_cu_count(s);
        const long long want = (tiles * (E.M + 2) + AGG_WAVES - 1) / AGG_WAVES;       // (units of 196 MFMAs) / waves
        if (wgs > want) wgs = want;
        if (wgs < 2) wgs = 2;
        int n_src = (int)((2 * wgs + (E.M + 2) / 2) / (E.M + 2));
        if (n_src < 1) n_src = 1;
        if (n_src > wgs - 1) n_src = (int)wgs - 1;
        rc = dispatch<1, 5, 10>(d.hg, [&](auto HGV) {
            ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_embed_out3<HGV>), EO3_SRC_LDS));
            k_embed_out3<HGV><<<(unsigned)wgs, AGG_THREADS, EO3_SRC_LDS, s>>>(E, n_src);
            return ZT_OK;
        });
    } else if (d.form == OutForm::persist_nbr) {
        // the neighbour paths alone (their source path ran in embed_ex; no GRU kernel took them along): (16 rows, model) units
        // over the waves of at most one workgroup per CU
        const long long units = (E.N + 15) / 16 * E.M;
        long long wgs = zt::stream_cu_count(s);
        if (d.max_wgs > 0 && wgs > d.max_wgs) wgs = d.max_wgs;
        if (wgs > (units + AGG_WAVES - 1) / AGG_WAVES) wgs = (units + AGG_WAVES - 1) / AGG_WAVES;
        rc = dispatch<1>(d.hg, [&](auto) {
            ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_embed_nbr3), EO3_NBR_LDS));
            k_embed_nbr3<<<(unsigned)wgs, AGG_THREADS, EO3_NBR_LDS, s>>>(E);
            return ZT_OK;
        });
    } else {
        const size_t lds2 = (size_t)2 * OUT_ROWS * (Dp + 4) * 4 + OUT_ROWS * 4;
        const dim3 grid((unsigned)((E.N + OUT_ROWS - 1) / OUT_ROWS), (unsigned)(E.M + 1));
        if (Dp > 16 * NTW * AGG_WAVES) {
            // 128 < D <= 256: four N-tiles per wave, up to 66 KB of LDS (no partial-sum groups: k_fc1_agg_wide is D = 100 only)
            rc = dispatch<1>(d.hg, [&](auto HGV) {
                ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_embed_out<HGV, NTW_WIDE>), lds2));
                k_embed_out<HGV, NTW_WIDE><<<grid, AGG_THREADS, lds2, s>>>(E);
                return ZT_OK;
            });
        } else {
            rc = dispatch<1, 5, 10>(d.hg, [&](auto HGV) { k_embed_out<HGV><<<grid, AGG_THREADS, lds2, s>>>(E); return ZT_OK; });
        }
    }
    if (rc == ZT_ERR_UNSUPPORTED) set_error("zt_embed: %d partial-sum groups per row", d.hg);      // (no instantiation for it)
    if (rc != ZT_OK) return rc;
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

int zt::embed_ex(const float *memory_dev, const float *efeat_dev, int64_t num_nodes, int64_t num_edges,
                 int32_t D, int32_t F, int32_t T, const int32_t *nodes_dev, int64_t N, int32_t M, int32_t k,
                 const int32_t *nbr_dev, const int32_t *eix_dev, const float *dt_dev, const float *w_dev,
                 const zt_embed_weights *wt, float *out_dev, void *workspace_dev, int32_t *status_dev,
                 const float *proj_table_dev, int32_t weights_ready, void *stream, hipEvent_t mid_wait,
                 zt::embed_out_deferred *defer, const zt::member_gate *gate)
{
    return embed_impl(memory_dev, efeat_dev, num_nodes, num_edges, D, F, T, nodes_dev, N, M, k, nbr_dev, eix_dev, dt_dev, w_dev,
                      wt, out_dev, workspace_dev, status_dev, proj_table_dev, weights_ready, stream, mid_wait, defer, gate);
}

// The wait for one batch's T-PPR rows as a kernel of its own: a wave that polls the batch's counter.  The kernel behind it on
// the stream starts with the acquire every kernel starts with and reads rows that were stored write-through.
namespace {
__global__ void k_member_gate(const int *word, int target, int *status, int *latch)
{
    if (threadIdx.x == 0) (void)member_gate_wait(word, target, status, latch);
}
}  // namespace

int zt::member_gate_launch(const zt::member_gate &g, int32_t *status_dev, void *stream)
{
    if (g.word == nullptr) return ZT_OK;
    // (The command processor could do the waiting itself -- hipStreamWaitValue32 works on plain device memory and on CU-masked
    //  streams, tools/exp/waitvalue_probe.hip, and the runtime implements it as a one-wave kernel of its own: measured, the step
    //  is the same to within the noise.  But that wait has no time limit, and a tool that serialises kernels -- rocprofv3's
    //  counter mode -- turns it into a hang where this kernel gives up after 4 s and reports.  Every wait of the library is
    //  bounded; so is this one.)
    k_member_gate<<<1, 64, 0, (hipStream_t)stream>>>(g.word, g.target, status_dev, g.latch);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

// Training forward of the neighbour half (backward: aggregate_bwd.hip):
//   H[m][n][:] = sum_k w_k/sum(w) relu(fc1([memory'[nbr] | ef | cos(dt w)])),  S[m][n] = (sum_k w != 0)
// where memory'[v] = overlay[row_map[v]] if row_map[v] >= 0 (rows of the lazily updated memory,
// modules/memory_updater.py:61-90) else memory[v].  fc2 and the source transform run on the [N, D] results
// outside (plain GEMMs).  workspace: zt_embed_workspace_bytes(N, D, F, T, M, k).
extern "C" int zt_agg_train_forward(const float *memory_dev, const float *overlay_dev, const int32_t *row_map_dev,
                                    const float *efeat_dev, int64_t num_nodes, int64_t num_edges, int32_t D, int32_t F,
                                    int32_t T, int64_t N, int32_t M, int32_t k, const int32_t *nbr_dev,
                                    const int32_t *eix_dev, const float *dt_dev, const float *w_dev,
                                    const zt_embed_weights *wt, float *H_dev, float *S_dev, void *workspace_dev,
                                    int32_t *status_dev, float drop_p, uint64_t drop_seed, void *stream)
{
    if (!memory_dev || !efeat_dev || !wt || !status_dev || !H_dev || !S_dev || !workspace_dev || N < 0 || D <= 0 || F < 0 ||
        T < 0 || M <= 0 || k <= 0 || (row_map_dev != nullptr && !overlay_dev) || !(drop_p >= 0.f && drop_p < 1.f)) {
        set_error("zt_agg_train_forward: bad argument");
        return ZT_ERR_ARG;
    }
    if (N == 0) return ZT_OK;
    EmbedPlan p;
    const KernelPlan kp = plan_kernels(N, D, F, T, M, k, false, true, 0, 0, p);
    if (kp.refusal == Refusal::shape) {
        set_error("zt_agg_train_forward: unsupported shape");
        return ZT_ERR_UNSUPPORTED;
    }
    if (kp.refusal == Refusal::no_split) {
        set_error("zt_agg_train_forward: D=%d F=%d T=%d k=%d: no 16-row chunk fits %d KB of LDS", D, F, T, k, AGG_LDS_BUDGET / 1024);
        return ZT_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace_dev);
    embed_prepare(wt, D, F, T, p, ws, s);          // the weights change every optimizer step
    FcAggArgs fa{};
    fa.memory = memory_dev; fa.efeat = efeat_dev; fa.time_w = wt->time_w;
    fa.num_nodes = num_nodes; fa.num_edges = num_edges; fa.N = N;
    fa.D = D; fa.F = F; fa.T = T; fa.M = M; fa.k = k; fa.ldm = D;
    fa.nbr = nbr_dev; fa.eix = eix_dev; fa.dt = dt_dev; fa.w = w_dev;
    fa.W1p = reinterpret_cast<const float *>(ws + p.off_w1p); fa.K1p = p.K1p; fa.b1 = wt->fc1_b;
    fa.H = H_dev; fa.S = S_dev; fa.status = status_dev;
    fa.overlay = overlay_dev; fa.row_map = row_map_dev;
    fa.set_dropout(drop_p, drop_seed);
    if (kp.agg == AggKernel::split)                // a query row wider than the 80-row tile: chunks of that tile
        return fc1_agg_split_launch(fa, s);
    const auto fwd = p.Dp > 16 * NTW * AGG_WAVES ? k_fc1_agg<false, MAX_MT, NTW_WIDE> : k_fc1_agg<false>;
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(fwd), kp.lds));
    dim3 grid((unsigned)((N + kp.rq - 1) / kp.rq), (unsigned)M);
    fwd<<<grid, AGG_THREADS, kp.lds, s>>>(fa, kp.rq, kp.mt, kp.lda);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
