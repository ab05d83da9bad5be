// The output layers of the embedding (k_embed_out: fc2 on the reduced rows, transform_source on memory[nodes]) as a device
// function: aggregate.hip launches it as a kernel of its own, memory_update.hip beside the GRU update in ONE launch
// (k_out_gru: the two are independent, each is bound by one workgroup's latency, and a launch boundary between them costs
// more than either's arithmetic at C2-C4's batch sizes).
#pragma once

#include "common.hpp"

namespace {

using zt::fastdiv;
using zt::fastdiv_magic;
using zt::wave_sync;

using zt::dense::f32x4;
using zt::dense::AGG_THREADS;
using zt::dense::AGG_WAVES;
using zt::dense::NTW;
using zt::dense::NTW_WIDE;

// ---------------------------------------------------------------------------
// out[n] = [ fc2s(relu(fc1s(memory[nodes[n]]))) | fc2(H_0[n]) + b2*S_0[n] | ... ]
// Three small D x D layers on f32 MFMA.  One workgroup per 32 rows; the input
// rows sit in LDS, weights ([Dp][Dp], zero padded) stream from L2 as b128
// fragments; wave w owns output N-tiles {w, w+4} (NW = NTW_WIDE: {w, w+4, w+8, w+12}).
// ---------------------------------------------------------------------------
constexpr int OUT_ROWS = 32;
constexpr int OUT_MT = OUT_ROWS / 16;
constexpr int SG_CH = 8;             // k-steps of weight fragments in flight (small_gemm)
constexpr int EO_GU = 8;             // staged elements in flight per thread (k_embed_out)

// acc[a][b] = X[a-th 16 rows] * W[b-th owned N-tile]^T   (X in LDS [32][ldx], W padded [Dp][Dp])
template <int NW>
__device__ __forceinline__ void small_gemm(const float *X, int ldx, const float *__restrict__ Wp, int Dp, int NT,
                                           int wave, int lane, f32x4 (&acc)[OUT_MT][NW])
{
    const int r16 = lane & 15, g4 = lane >> 4;
#pragma unroll
    for (int a = 0; a < OUT_MT; ++a)
#pragma unroll
        for (int b = 0; b < NW; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The weight fragments of SG_CH k-steps are fetched together, before the first MFMA that needs one: a
    // workgroup has one tile of 32 rows, so nothing else hides the L2 round trip of a load issued per k-step.
    const int KC = Dp / 16;
    for (int kc0 = 0; kc0 < KC; kc0 += SG_CH) {
        f32x4 bv[SG_CH][NW];
#pragma unroll
        for (int c = 0; c < SG_CH; ++c)
#pragma unroll
            for (int b = 0; b < NW; ++b) {
                const int nt = wave + b * AGG_WAVES;
                bv[c][b] = (kc0 + c < KC && nt < NT)
                               ? *reinterpret_cast<const f32x4 *>(Wp + (size_t)(nt * 16 + r16) * Dp + 16 * (kc0 + c) + 4 * g4)
                               : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int c = 0; c < SG_CH; ++c) {
            if (kc0 + c >= KC) break;
            f32x4 av[OUT_MT];
#pragma unroll
            for (int a = 0; a < OUT_MT; ++a)
                av[a] = *reinterpret_cast<const f32x4 *>(X + (size_t)(a * 16 + r16) * ldx + 16 * (kc0 + c) + 4 * g4);
#pragma unroll
            for (int b = 0; b < NW; ++b) {
                if (wave + b * AGG_WAVES >= NT) continue;
#pragma unroll
                for (int a = 0; a < OUT_MT; ++a)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][j], bv[c][b][j], acc[a][b], 0, 0, 0);
            }
        }
    }
}

using zt::EmbedOutArgs;          // (common.hpp)

// bx = 32-row tile, path = 0 (source path) or 1 + model; the first AGG_THREADS threads of the workgroup.  src_read != nullptr:
// a source-path workgroup adds 1 there once its memory rows are in LDS (k_out_gru: the GRU half waits for all of them before
// it writes the table).
// NW: N-tiles per wave (NTW: Dp <= 128; NTW_WIDE: Dp <= 256)
template <int HG, int NW = NTW>      // partial-sum groups per query row in H (k_fc1_agg_wide: k / 4; else 1)
__device__ __forceinline__ void embed_out_body(const EmbedOutArgs &E, char *smem, int bx, int path, int *src_read)
{
    const float *__restrict__ memory = E.memory;
    const long long num_nodes = E.num_nodes, N = E.N;
    const int *__restrict__ nodes = E.nodes;
    const int D = E.D, M = E.M;
    const float *__restrict__ H = E.H, *__restrict__ S = E.S, *__restrict__ fc2_p = E.fc2_p, *__restrict__ fc2_b = E.fc2_b;
    const float *__restrict__ fc1s_p = E.fc1s_p, *__restrict__ fc1s_b = E.fc1s_b, *__restrict__ fc2s_p = E.fc2s_p, *__restrict__ fc2s_b = E.fc2s_b;
    float *__restrict__ out = E.out;
    int *status = E.status;
    const int Dp = (D + 15) / 16 * 16, ldx = Dp + 4, NT = Dp / 16;
    float *X = reinterpret_cast<float *>(smem);          // [32][ldx] layer input
    float *Y = X + OUT_ROWS * ldx;                       // [32][ldx] hidden rows of the source path
    int *rid = reinterpret_cast<int *>(Y + OUT_ROWS * ldx);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    const long long r0 = (long long)bx * OUT_ROWS;
    const int nr = (int)((N - r0) < OUT_ROWS ? (N - r0) : OUT_ROWS);
    const int OW = D * (M + 1);
    const unsigned mL = fastdiv_magic((unsigned)ldx);
    f32x4 acc[OUT_MT][NW];

    // blockIdx.y = 0: the source path (two dependent layers); 1 + m: fc2 of model m.  The paths are independent,
    // and the kernel's time is the latency of ONE workgroup (there are fewer workgroups than the chip holds).
    if (path == 0) {
        if (tid < OUT_ROWS) {
            int nd = 0;
            if (tid < nr) {
                nd = nodes[r0 + tid];
                if (nd < 0 || nd >= num_nodes) { atomicExch(status, ZT_ERR_RANGE); nd = 0; }
            }
            rid[tid] = nd;
        }
        __syncthreads();
        // ---- source path: memory[nodes] -> fc1s -> relu -> fc2s ----
        // (EO_GU loads in flight per thread before the first LDS store: a load per iteration was a memory round trip
        //  per iteration, 15 of them in a row)
        for (int f0 = tid; f0 < OUT_ROWS * ldx; f0 += AGG_THREADS * EO_GU) {
            float v[EO_GU];
#pragma unroll
            for (int u = 0; u < EO_GU; ++u) {
                const int f = f0 + u * AGG_THREADS, g = fastdiv(f, mL), c = f - g * ldx;
                v[u] = (f < OUT_ROWS * ldx && g < nr && c < D) ? memory[(size_t)rid[g] * D + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < EO_GU; ++u)
                if (f0 + u * AGG_THREADS < OUT_ROWS * ldx) X[f0 + u * AGG_THREADS] = v[u];
        }
        __syncthreads();
        if (src_read != nullptr && tid == 0) atomicAdd(src_read, 1);      // (the rows are in LDS: every load has returned)
        small_gemm(X, ldx, fc1s_p, Dp, NT, wave, lane, acc);
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            const int col = (wave + b * AGG_WAVES) * 16 + r16;
            if (col >= Dp) continue;
            const float bias = col < D ? fc1s_b[col] : 0.f;
#pragma unroll
            for (int a = 0; a < OUT_MT; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = acc[a][b][j] + bias;
                    Y[(size_t)(a * 16 + g4 * 4 + j) * ldx + col] = (col < D && v > 0.f) ? v : 0.f;
                }
        }
        __syncthreads();
        small_gemm(Y, ldx, fc2s_p, Dp, NT, wave, lane, acc);
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            const int col = (wave + b * AGG_WAVES) * 16 + r16;
            if (col >= D) continue;
            const float bias = fc2s_b[col];
#pragma unroll
            for (int a = 0; a < OUT_MT; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int g = a * 16 + g4 * 4 + j;
                    if (g < nr) out[(size_t)(r0 + g) * OW + col] = acc[a][b][j] + bias;
                }
        }
        return;
    }
    // ---- neighbour path: fc2 on the reduced rows of model m ----
    {
        const int m = path - 1;
        for (int f0 = tid; f0 < OUT_ROWS * ldx; f0 += AGG_THREADS * EO_GU) {
            float v[EO_GU];
#pragma unroll
            for (int u = 0; u < EO_GU; ++u) {
                const int f = f0 + u * AGG_THREADS, g = fastdiv(f, mL), c = f - g * ldx;
                v[u] = 0.f;
                if (f < OUT_ROWS * ldx && g < nr && c < D) {
                    // hg > 1 (k_fc1_agg_wide): H holds the partial sums of every group of four neighbour rows; a query row's
                    // groups are added first to last, whichever tile or shard computed them
                    const float *hp = H + (((size_t)m * N + r0 + g) * HG) * D + c;
                    v[u] = hp[0];
#pragma unroll
                    for (int q = 1; q < HG; ++q) v[u] += hp[(size_t)q * D];
                }
            }
#pragma unroll
            for (int u = 0; u < EO_GU; ++u)
                if (f0 + u * AGG_THREADS < OUT_ROWS * ldx) X[f0 + u * AGG_THREADS] = v[u];
        }
        __syncthreads();
        small_gemm(X, ldx, fc2_p, Dp, NT, wave, lane, acc);
#pragma unroll
        for (int b = 0; b < NW; ++b) {
            const int col = (wave + b * AGG_WAVES) * 16 + r16;
            if (col >= D) continue;
            const float bias = fc2_b[col];
#pragma unroll
            for (int a = 0; a < OUT_MT; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int g = a * 16 + g4 * 4 + j;
                    if (g < nr)
                        out[(size_t)(r0 + g) * OW + (size_t)D * (m + 1) + col] =
                            acc[a][b][j] + bias * S[(size_t)m * N + r0 + g];
                }
        }
    }
}

template <int HG, int NW = NTW>
__global__ __launch_bounds__(AGG_THREADS) void k_embed_out(EmbedOutArgs E)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    embed_out_body<HG, NW>(E, smem, blockIdx.x, blockIdx.y, nullptr);
}

// ---------------------------------------------------------------------------
// k_embed_out2: the same three layers, organised for LATENCY (round 4).  k_embed_out's time was never its arithmetic:
// at C2's batch (600 rows) it ran 27 us for 40 MFLOP -- a chain of dependent memory round trips per workgroup (ids ->
// row staging through LDS in a loop the compiler cannot unroll, one round trip per iteration -> weight fragments per
// k-chunk -> second layer -> ...) on 57 workgroups.  Here one WAVE owns (16 rows, path, one N-tile of the output):
//   * its weight fragments -- fc2's [16 x Dp] slice, for the source path also ALL of fc1s -- are requested first,
//     before anything is looked at, and stay in registers while the wave strides over row tiles;
//   * the A operand comes straight from memory into the MFMA lanes (lane (row r, k-slot g) loads float4 at columns
//     16 c + 4 g -- the k order the padded weights already have), no LDS staging; partial-sum groups (k_fc1_agg_wide)
//     are added first to last as they arrive;
//   * the source path's hidden layer is computed by each of the NT waves of a row tile (0.4 MFLOP, redundant on purpose:
//     sharing it would cost a barrier and a round trip through LDS or memory) and turned from the MFMA's output layout
//     into its input layout through 7 KB of the wave's own LDS.
// One memory round trip for the neighbour paths, two for the source path (ids, then rows).  D % 4 == 0.
// ---------------------------------------------------------------------------
// ONE WAVE's work: (bx of gx) = the tiles it strides over, path, b = its N-tile; Y = 16 x (16 NT + 4) floats of LDS of its own.
// src_read != nullptr: a source-path wave adds 1 there once its last memory rows have arrived (k_out_gru2).
template <int NT, int HG>
__device__ __forceinline__ void embed_out2_body(const EmbedOutArgs &E, float *Y, int lane, int bx, int gx, int path, int b, int *src_read)
{
    const float *__restrict__ memory = E.memory;
    const long long num_nodes = E.num_nodes, N = E.N;
    const int *__restrict__ nodes = E.nodes;
    const int D = E.D, M = E.M;
    const float *__restrict__ H = E.H, *__restrict__ S = E.S, *__restrict__ fc2_p = E.fc2_p, *__restrict__ fc2_b = E.fc2_b;
    const float *__restrict__ fc1s_p = E.fc1s_p, *__restrict__ fc1s_b = E.fc1s_b, *__restrict__ fc2s_p = E.fc2s_p, *__restrict__ fc2s_b = E.fc2s_b;
    float *__restrict__ out = E.out;
    int *status = E.status;
    constexpr int Dp = NT * 16, KC = NT, ldy = Dp + 4;
    const int r16 = lane & 15, g4 = lane >> 4;
    const int col = 16 * b + r16, OW = D * (M + 1);
    const long long tiles = (N + 15) / 16;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // columns this lane's float4 of chunk c covers: all four inside the row, or none (D % 4 == 0)
    bool cin[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) cin[c] = 16 * c + 4 * g4 < D;

    if (path == 0) {
        f32x4 w1[NT][KC], w2[KC];
#pragma unroll
        for (int bb = 0; bb < NT; ++bb)
#pragma unroll
            for (int c = 0; c < KC; ++c) w1[bb][c] = *reinterpret_cast<const f32x4 *>(fc1s_p + (size_t)(16 * bb + r16) * Dp + 16 * c + 4 * g4);
#pragma unroll
        for (int c = 0; c < KC; ++c) w2[c] = *reinterpret_cast<const f32x4 *>(fc2s_p + (size_t)col * Dp + 16 * c + 4 * g4);
        float b1v[NT];
#pragma unroll
        for (int bb = 0; bb < NT; ++bb) b1v[bb] = 16 * bb + r16 < D ? fc1s_b[16 * bb + r16] : 0.f;
        const float b2v = col < D ? fc2s_b[col] : 0.f;
        long long t = bx;
        int nd = (t < tiles && t * 16 + r16 < N) ? nodes[t * 16 + r16] : 0;
        for (; t < tiles; t += gx) {
            const long long r0 = t * 16;
            if (nd < 0 || nd >= num_nodes) { atomicExch(status, ZT_ERR_RANGE); nd = 0; }
            const bool rin = r0 + r16 < N;
            f32x4 a[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c)
                a[c] = (rin && cin[c]) ? *reinterpret_cast<const f32x4 *>(memory + (size_t)nd * D + 16 * c + 4 * g4) : zero4;
            const long long tn = t + gx;
            nd = (tn < tiles && tn * 16 + r16 < N) ? nodes[tn * 16 + r16] : 0;      // the next tile's ids, a tile ahead
            f32x4 acc1[NT];
#pragma unroll
            for (int bb = 0; bb < NT; ++bb) acc1[bb] = zero4;
#pragma unroll
            for (int c = 0; c < KC; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int bb = 0; bb < NT; ++bb)
                        acc1[bb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][j], w1[bb][c][j], acc1[bb], 0, 0, 0);
#pragma unroll
            for (int bb = 0; bb < NT; ++bb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = acc1[bb][j] + b1v[bb];
                    Y[(4 * g4 + j) * ldy + 16 * bb + r16] = (16 * bb + r16 < D && v > 0.f) ? v : 0.f;
                }
            wave_sync();
            f32x4 acc = zero4;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const f32x4 y = *reinterpret_cast<const f32x4 *>(Y + r16 * ldy + 16 * c + 4 * g4);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(y[j], w2[c][j], acc, 0, 0, 0);
            }
            if (col < D) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r0 + 4 * g4 + j < N) out[(size_t)(r0 + 4 * g4 + j) * OW + col] = acc[j] + b2v;
            }
            wave_sync();                                                   // Y is free for the next tile
        }
        // (every row this wave reads has been consumed by an MFMA: the loads have returned)
        if (src_read != nullptr && lane == 0) atomicAdd(src_read, 1);
        return;
    }
    // ---- neighbour path: fc2 on the reduced rows of model m ----
    const int m = path - 1;
    f32x4 w2[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) w2[c] = *reinterpret_cast<const f32x4 *>(fc2_p + (size_t)col * Dp + 16 * c + 4 * g4);
    const float b2v = col < D ? fc2_b[col] : 0.f;
    for (long long t = bx; t < tiles; t += gx) {
        const long long r0 = t * 16;
        const bool rin = r0 + r16 < N;
        const float *hp = H + (((size_t)m * N + (rin ? r0 + r16 : 0)) * HG) * D + 4 * g4;
        f32x4 g[HG][KC];
#pragma unroll
        for (int q = 0; q < HG; ++q)
#pragma unroll
            for (int c = 0; c < KC; ++c) g[q][c] = (rin && cin[c]) ? *reinterpret_cast<const f32x4 *>(hp + (size_t)q * D + 16 * c) : zero4;
        float sv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[j] = r0 + 4 * g4 + j < N ? S[(size_t)m * N + r0 + 4 * g4 + j] : 0.f;
        f32x4 acc = zero4;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            f32x4 a = g[0][c];
#pragma unroll
            for (int q = 1; q < HG; ++q) a += g[q][c];                     // a query row's groups, first to last
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w2[c][j], acc, 0, 0, 0);
        }
        if (col < D) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (r0 + 4 * g4 + j < N) out[(size_t)(r0 + 4 * g4 + j) * OW + (size_t)D * (m + 1) + col] = acc[j] + b2v * sv[j];
        }
    }
}

template <int NT, int HG>
__global__ __launch_bounds__(64) void k_embed_out2(EmbedOutArgs E)
{
    __shared__ __attribute__((aligned(16))) float Y[16 * (NT * 16 + 4)];
    embed_out2_body<NT, HG>(E, Y, threadIdx.x, blockIdx.x, gridDim.x, blockIdx.y, blockIdx.z, nullptr);
}

// ---------------------------------------------------------------------------
// k_embed_out3 (round 5): the same three layers, PERSISTENT, for batches beyond k_embed_out2's reach.  k_embed_out's time
// at 3 000-12 000 rows was rounds of dependent weight-fragment fetches from L2 per 32-row workgroup (35-40 us for 1 GFLOP
// at C5's batch).  Here the weights live in LDS for the launch, in the order the MFMAs consume them (fragment (N-tile b,
// k-chunk c) = 64 lanes x 4 floats, one conflict-free ds_read_b128 per four MFMAs), one workgroup per CU of the stream,
// and every WAVE strides over (16 rows x ALL seven N-tiles) units by itself: the A operand comes straight from memory
// into the MFMA lanes (float4 at columns 16 c + 4 g, as in k_embed_out2), the next unit's rows are requested before the
// current unit's MFMAs, a row is read once.  Same accumulation order as the other two kernels (k-chunks first to last),
// so the three agree to the bit.  D = 100 (Dp = 112).
// The two paths are device functions of their own (round 15): neither reads what the other writes, and only the source
// path reads the memory table.  aggregate.hip builds k_embed_out3 from both (workgroups [0, n_src) the source path), a
// source-only and a neighbour-only launch from one each; memory_update.hip runs the neighbour path behind the GRU tiles
// of k_nbr_gru, in that kernel's eight-wave workgroups.
// ---------------------------------------------------------------------------
constexpr int EO3_NT = 7, EO3_KC = 7, EO3_DP = 112, EO3_LDY = 116;
constexpr int EO3_FRAG = EO3_NT * EO3_KC * 256;      // floats of one weight matrix in fragment order
constexpr size_t EO3_SRC_LDS = (size_t)(2 * EO3_FRAG + AGG_WAVES * 16 * EO3_LDY) * 4;     // fc1s, fc2s, the waves' hidden rows
constexpr size_t EO3_NBR_LDS = (size_t)EO3_FRAG * 4;                                      // fc2

template <int THREADS>
__device__ __forceinline__ void eo3_fill(float *Wl, const float *__restrict__ Wp, int tid)
{
    constexpr int PER = (EO3_NT * EO3_KC * 64 + THREADS - 1) / THREADS;  // fragments-lanes per thread: all in flight, then stored
    f32x4 v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int idx = tid + q * THREADS, frag = idx >> 6, ln = idx & 63;
        const int b = frag / EO3_KC, c = frag - b * EO3_KC;
        v[q] = idx < EO3_NT * EO3_KC * 64
                   ? *reinterpret_cast<const f32x4 *>(Wp + (size_t)(16 * b + (ln & 15)) * EO3_DP + 16 * c + 4 * (ln >> 4))
                   : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int idx = tid + q * THREADS;
        if (idx < EO3_NT * EO3_KC * 64) reinterpret_cast<f32x4 *>(Wl)[idx] = v[q];
    }
}

// The source path: memory[nodes] -> fc1s -> relu -> fc2s.  Workgroup wg of n_wgs, four waves (AGG_THREADS); fc1s and fc2s
// resident (98 KB), the hidden rows through 7 KB of the wave's own LDS: EO3_SRC_LDS bytes at smem.
__device__ __forceinline__ void eo3_src_body(const EmbedOutArgs &E, char *smem, int wg, int n_wgs)
{
    const float *__restrict__ memory = E.memory;
    const long long num_nodes = E.num_nodes, N = E.N;
    const int *__restrict__ nodes = E.nodes;
    const int D = E.D, M = E.M;
    const float *__restrict__ fc1s_p = E.fc1s_p, *__restrict__ fc1s_b = E.fc1s_b, *__restrict__ fc2s_p = E.fc2s_p, *__restrict__ fc2s_b = E.fc2s_b;
    float *__restrict__ out = E.out;
    int *status = E.status;
    float *W0 = reinterpret_cast<float *>(smem);                         // fc1s
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int OW = D * (M + 1);
    const long long tiles = (N + 15) / 16;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    bool cin[EO3_KC];                                                    // this lane's float4 of chunk c lies inside the row
#pragma unroll
    for (int c = 0; c < EO3_KC; ++c) cin[c] = 16 * c + 4 * g4 < D;
    const f32x4 *Wf0 = reinterpret_cast<const f32x4 *>(W0) + lane;
    float *W1 = W0 + EO3_FRAG;                                           // fc2s
    float *Y = W1 + EO3_FRAG + wave * 16 * EO3_LDY;                      // this wave's hidden rows
    eo3_fill<AGG_THREADS>(W0, fc1s_p, tid);
    eo3_fill<AGG_THREADS>(W1, fc2s_p, tid);
    float b1v[EO3_NT], b2v[EO3_NT];
#pragma unroll
    for (int b = 0; b < EO3_NT; ++b) {
        b1v[b] = 16 * b + r16 < D ? fc1s_b[16 * b + r16] : 0.f;
        b2v[b] = 16 * b + r16 < D ? fc2s_b[16 * b + r16] : 0.f;
    }
    const f32x4 *Wf1 = reinterpret_cast<const f32x4 *>(W1) + lane;
    const long long stride = (long long)n_wgs * AGG_WAVES;
    long long t = (long long)wg * AGG_WAVES + wave;
    // ids two units ahead, rows one unit ahead
    auto node_of = [&](long long tt) -> int { return (tt < tiles && tt * 16 + r16 < N) ? nodes[tt * 16 + r16] : -1; };
    auto rows_of = [&](int nd, f32x4 (&a)[EO3_KC]) {
        const bool ok = nd >= 0 && nd < num_nodes;
#pragma unroll
        for (int c = 0; c < EO3_KC; ++c)
            a[c] = (ok && cin[c]) ? *reinterpret_cast<const f32x4 *>(memory + (size_t)nd * D + 16 * c + 4 * g4) : zero4;
    };
    int nd_cur = node_of(t), nd_nxt = node_of(t + stride);
    f32x4 a[EO3_KC], an[EO3_KC];
    if (t < tiles) rows_of(nd_cur, a);
    __syncthreads();                                                     // both weight images are in LDS
    for (; t < tiles; t += stride) {
        const long long r0 = t * 16;
        if (r0 + r16 < N && (nd_cur < 0 || nd_cur >= num_nodes)) atomicExch(status, ZT_ERR_RANGE);
        rows_of(nd_nxt, an);                                             // the next unit's rows, under this unit's MFMAs
        nd_cur = nd_nxt;
        nd_nxt = node_of(t + 2 * stride);
        f32x4 acc1[EO3_NT];
#pragma unroll
        for (int b = 0; b < EO3_NT; ++b) acc1[b] = zero4;
#pragma unroll
        for (int c = 0; c < EO3_KC; ++c) {
            f32x4 w[EO3_NT];
#pragma unroll
            for (int b = 0; b < EO3_NT; ++b) w[b] = Wf0[(b * EO3_KC + c) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)                                      // consecutive MFMAs on different accumulators
#pragma unroll
                for (int b = 0; b < EO3_NT; ++b) acc1[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][j], w[b][j], acc1[b], 0, 0, 0);
        }
#pragma unroll
        for (int b = 0; b < EO3_NT; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = acc1[b][j] + b1v[b];
                Y[(4 * g4 + j) * EO3_LDY + 16 * b + r16] = (16 * b + r16 < D && v > 0.f) ? v : 0.f;
            }
        wave_sync();
        f32x4 acc[EO3_NT];
#pragma unroll
        for (int b = 0; b < EO3_NT; ++b) acc[b] = zero4;
#pragma unroll
        for (int c = 0; c < EO3_KC; ++c) {
            const f32x4 y = *reinterpret_cast<const f32x4 *>(Y + r16 * EO3_LDY + 16 * c + 4 * g4);
            f32x4 w[EO3_NT];
#pragma unroll
            for (int b = 0; b < EO3_NT; ++b) w[b] = Wf1[(b * EO3_KC + c) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < EO3_NT; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(y[j], w[b][j], acc[b], 0, 0, 0);
        }
#pragma unroll
        for (int b = 0; b < EO3_NT; ++b) {
            const int col = 16 * b + r16;
            if (col < D) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r0 + 4 * g4 + j < N) out[(size_t)(r0 + 4 * g4 + j) * OW + col] = acc[b][j] + b2v[b];
            }
        }
        wave_sync();                                                     // Y is free for the next unit
#pragma unroll
        for (int c = 0; c < EO3_KC; ++c) a[c] = an[c];
    }
}

// The neighbour paths: fc2 on the reduced rows H, S of the M models; reads nothing of the memory table.  Workgroup wg of
// n_wgs, WAVES waves each (every thread of the workgroup comes here: one barrier); fc2 resident: EO3_NBR_LDS bytes at smem.
// FB: N-tile fragments of a k-chunk held at once -- all seven where the kernel has the register file to itself
// (k_embed_out3), fewer where the waves share it with another body's (k_nbr_gru: there the biases are fetched behind the
// MFMAs too; plain rows only, HG = 1).  Each accumulator sees its k-chunks first to last whatever FB is.
template <int HG, int WAVES, int FB>
__device__ __forceinline__ void eo3_nbr_body(const EmbedOutArgs &E, char *smem, int wg, int n_wgs)
{
    const long long N = E.N;
    const int D = E.D, M = E.M;
    const float *__restrict__ H = E.H, *__restrict__ S = E.S, *__restrict__ fc2_p = E.fc2_p, *__restrict__ fc2_b = E.fc2_b;
    float *__restrict__ out = E.out;
    constexpr bool LEAN = FB < EO3_NT;
    static_assert(HG == 1 || !LEAN, "partial-sum groups only with all seven fragments held (k_embed_out3)");
    float *W0 = reinterpret_cast<float *>(smem);                         // fc2
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int OW = D * (M + 1);
    const long long tiles = (N + 15) / 16;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    bool cin[EO3_KC];                                                    // this lane's float4 of chunk c lies inside the row
#pragma unroll
    for (int c = 0; c < EO3_KC; ++c) cin[c] = 16 * c + 4 * g4 < D;
    const f32x4 *Wf0 = reinterpret_cast<const f32x4 *>(W0) + lane;
    eo3_fill<64 * WAVES>(W0, fc2_p, tid);
    float b2v[LEAN ? 1 : EO3_NT];
    if constexpr (!LEAN) {
#pragma unroll
        for (int b = 0; b < EO3_NT; ++b) b2v[b] = 16 * b + r16 < D ? fc2_b[16 * b + r16] : 0.f;
    }
    const long long units = tiles * M;
    const long long stride = (long long)n_wgs * WAVES;
    long long u = (long long)wg * WAVES + wave;
    // a unit's A operand: a query row's HG partial-sum groups (k_fc1_agg_wide), added first to last.  HG = 1: the next
    // unit's rows are requested under this unit's MFMAs; HG > 1 (F = 172: at most a few units per wave at those batch
    // sizes): groups [q0, q0 + GQ) at a time, at the top of the unit
    constexpr int GQ = HG == 1 ? 1 : 5;
    auto rows_of = [&](long long uu, int q0, f32x4 (&g)[GQ][EO3_KC]) {
        const long long m = uu / tiles, r = (uu - m * tiles) * 16 + r16;
        const bool rin = uu < units && r < N;
        const float *hp = H + (((size_t)m * N + (rin ? r : 0)) * HG + q0) * D + 4 * g4;
#pragma unroll
        for (int q = 0; q < GQ; ++q)
#pragma unroll
            for (int c = 0; c < EO3_KC; ++c) g[q][c] = (rin && cin[c]) ? *reinterpret_cast<const f32x4 *>(hp + (size_t)q * D + 16 * c) : zero4;
    };
    f32x4 gn[GQ][EO3_KC];
    if (HG == 1) rows_of(u, 0, gn);
    __syncthreads();                                                     // the weight image is in LDS
    for (; u < units; u += stride) {
        const long long m = u / tiles, r0 = (u - m * tiles) * 16;
        f32x4 a[EO3_KC];
        if (HG == 1) {
#pragma unroll
            for (int c = 0; c < EO3_KC; ++c) a[c] = gn[0][c];
        } else {
#pragma nounroll
            for (int q0 = 0; q0 < HG; q0 += GQ) {
                rows_of(u, q0, gn);
#pragma unroll
                for (int c = 0; c < EO3_KC; ++c) {
                    if (q0 == 0) a[c] = gn[0][c]; else a[c] += gn[0][c];
#pragma unroll
                    for (int q = 1; q < GQ; ++q) a[c] += gn[q][c];
                }
            }
        }
        float sv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[j] = r0 + 4 * g4 + j < N ? S[(size_t)m * N + r0 + 4 * g4 + j] : 0.f;
        if (HG == 1) rows_of(u + stride, 0, gn);                         // the next unit's rows, under this unit's MFMAs
        // (LEAN: the fragments are read from LDS unit by unit -- left to itself the compiler lifts all 49 reads out of the unit
        //  loop, 196 registers that this kernel does not have)
        if constexpr (LEAN) asm volatile("" ::: "memory");
        f32x4 acc[EO3_NT];
#pragma unroll
        for (int b = 0; b < EO3_NT; ++b) acc[b] = zero4;
#pragma unroll
        for (int c = 0; c < EO3_KC; ++c) {
#pragma unroll
            for (int b0 = 0; b0 < EO3_NT; b0 += FB) {
                f32x4 w[FB];
#pragma unroll
                for (int b = 0; b < FB; ++b)
                    if (b0 + b < EO3_NT) w[b] = Wf0[((b0 + b) * EO3_KC + c) * 64];
#pragma unroll
                for (int j = 0; j < 4; ++j)                                  // consecutive MFMAs on different accumulators
#pragma unroll
                    for (int b = 0; b < FB; ++b)
                        if (b0 + b < EO3_NT) acc[b0 + b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][j], w[b][j], acc[b0 + b], 0, 0, 0);
            }
        }
#pragma unroll
        for (int b = 0; b < EO3_NT; ++b) {
            const int col = 16 * b + r16;
            if (col < D) {
                const float bias = LEAN ? fc2_b[col] : b2v[LEAN ? 0 : b];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r0 + 4 * g4 + j < N) out[(size_t)(r0 + 4 * g4 + j) * OW + (size_t)D * (m + 1) + col] = acc[b][j] + bias * sv[j];
            }
        }
    }
}

}  // namespace
