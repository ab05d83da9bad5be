// The node-classification decoder on the device, forward and backward: the reference's MLP (utils/util.py:28-42)
//   z = fc3( drop( relu( fc2( drop( relu( fc1(x) ) ) ) ) ) ),   x [N][H] -> 80 -> 10 -> z [N]
// as evaluation/evaluation.py:51-79 and a decoder's training loop apply it to the source embeddings of a batch.  The kernels
// read the parameters as they lie in the module (no packed copy); K runs over H at run time in chunks of DEC_KC columns staged
// in LDS, so LDS does not bound H: any H % 4 == 0 with 4 <= H <= 4352 (zt_affinity_rank's widths).
//
// Forward (one launch, k_decoder<NTW, TRAIN>).  Layer 1 runs on v_mfma_f32_16x16x4_f32: its 80 columns are five N-tiles
// exactly; a lane streams its row of fc1.weight as 16-byte vectors, the x tile comes from LDS.  Two arrangements of a 16-row
// tile (zt::decoder_plan picks):
//   DEC_ARR_FIVE  five waves own one N-tile each and share the 16 staged rows: the plan's pick at every N
//   DEC_ARR_ONE   a wave owns all five N-tiles of its 16 rows; four waves = 64 rows per workgroup (measured no faster
//                 anywhere: kept behind the test hook's pin as the form the pick is held against)
// Both add every element's products in the same order: they give the same bits.  The layer-1 tile (bias, ReLU, dropout applied
// in the accumulator lanes) goes through LDS into layer 2: one N-tile padded to 16, K = 80; columns 10..15 are fed zeros and
// read nothing.  Layer 3 is a ten-term sum per row in column order.  TRAIN keeps h1 [N][80] and h2 [N][10] after ReLU and
// dropout; the dropout mask is drop_scale (common.hpp) at element row * 80 + col of layer 1 and N * 80 + row * 10 + col of
// layer 2, so the backward regenerates it.
//
// Backward (three launches, nothing on the host in between, no atomics on any output):
//   k_dec_bwd_dx   per 16 rows: dh2 = dz w3 masked by h2 > 0 times the regenerated scale, dh1 = dh2 W2 masked likewise (both
//                  written to the workspace), and, where asked, d_x = dh1 W1 on the MFMA (K = 80)
//   k_dec_bwd_dw   d_fc1_w [80][H] = dh1^T x: a workgroup owns all 80 rows of 64 columns, K = N in steps of 64 through LDS,
//                  split over blockIdx.y into partial products
//   k_dec_bwd_fin  the 901 small sums (d_fc1_b, d_fc2_w, d_fc2_b, d_fc3_w, d_fc3_b) over the rows, and the partial products
//                  added first to last
// Every sum has a fixed association: two runs give the same bits.
#include "common.hpp"

using namespace zt;

namespace zt {
int g_decoder_arrangement = 0;        // test hook (zt_test_decoder_arrangement): 0 = the plan's pick
}

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int H1 = ZT_DECODER_H1, H2 = ZT_DECODER_H2;
constexpr int DEC_MIN_H = 4, DEC_MAX_H = 4352;
constexpr int DEC_KC = 256;              // columns of x a K-chunk stages
constexpr int DEC_LDX = DEC_KC + 4;      // row stride of the staged x tile (floats)
constexpr int DEC_LDH = H1 + 4;          // ... of the layer-1 tile
constexpr int DEC_LD2 = 12;              // ... of the layer-2 tile
constexpr int DEC_ARR_ONE = 1, DEC_ARR_FIVE = 5;
constexpr int DEC_MAX_SPLIT = 8;         // partial products of d_fc1_w
constexpr int GK = 64;                   // rows per K-step of k_dec_bwd_dw
constexpr int FIN_THREADS = 1024, FIN_WAVES = 16;
constexpr int FIN_OUTS = H1 + H2 * H1 + H2 + H2 + 1;      // 901
static_assert(H1 == 80 && H2 == 10, "five N-tiles and one padded N-tile");

__host__ __device__ inline int round_up16(int x) { return (x + 15) / 16 * 16; }

struct DecArgs {
    const float *x;
    long long N;
    int H;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float *logit, *prob, *h1, *h2;
    unsigned lo, hi, thr;
    float inv;
};

// U k-steps of 16 of a wave's NTW N-tiles: every weight load of the round is issued before the first MFMA
template <int NTW, int U>
__device__ __forceinline__ void l1_steps(int kc0, int c, int g4, int H, const float *(&wrow)[NTW], const float *as_p,
                                         f32x4 (&acc)[NTW])
{
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 w[U][NTW];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // H % 4 == 0: all four columns or none.  The load is unconditional, from a clamped address (no branch per load)
        const int k = kc0 + 16 * (c + u) + 4 * g4;
        const bool kok = k < H;
        const int kk = kok ? k : H - 4;
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(wrow[t] + kk);
            w[u][t] = kok ? v : zero4;
        }
    }
    __builtin_amdgcn_sched_barrier(0);                                   // (or the scheduler sinks every load to its first use)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(as_p + 16 * (c + u));
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w[u][t][j], acc[t], 0, 0, 0);
    }
}

template <int NTW, bool TRAIN>
__global__ __launch_bounds__(NTW == 5 ? 256 : 320) void k_decoder(const DecArgs a)
{
#pragma clang fp contract(off)
    constexpr int ROWS = NTW == 5 ? 64 : 16, THREADS = NTW == 5 ? 256 : 320;
    extern __shared__ __attribute__((aligned(16))) char dec_smem[];
    float *XS = reinterpret_cast<float *>(dec_smem);                     // [ROWS][DEC_LDX]: the x tile of a K-chunk
    float *HS = XS;                                                      // [ROWS][DEC_LDH]: the layer-1 tile, once x is done with
    float *H2S = XS + ROWS * DEC_LDH;                                    // [ROWS][DEC_LD2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int H = a.H;
    const long long N = a.N, r0 = (long long)blockIdx.x * ROWS;
    const int tile = NTW == 5 ? wave : 0, nt0 = NTW == 5 ? 0 : wave;     // this wave's 16 rows and its first N-tile
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float *wrow[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) wrow[t] = a.w1 + (size_t)(16 * (nt0 + t) + r16) * H;
    f32x4 acc[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) acc[t] = zero4;
    const float *as_p = XS + (16 * tile + r16) * DEC_LDX + 4 * g4;
    for (int kc0 = 0; kc0 < H; kc0 += DEC_KC) {
        const int kcw = H - kc0 < DEC_KC ? H - kc0 : DEC_KC, kcp4 = round_up16(kcw) / 4;
        if (kc0 > 0) __syncthreads();                                    // (the chunk before is read)
        // ---- stage the chunk: zero beyond the rows and beyond H ----
        for (int f = tid; f < ROWS * kcp4; f += THREADS) {
            const int row = f / kcp4, c4 = f - row * kcp4;
            const bool ok = 4 * c4 < kcw && r0 + row < N;
            const f32x4 v = ok ? *reinterpret_cast<const f32x4 *>(a.x + (size_t)(r0 + row) * H + kc0 + 4 * c4) : zero4;
            *reinterpret_cast<f32x4 *>(XS + row * DEC_LDX + 4 * c4) = v;
        }
        __syncthreads();
        const int nc = kcp4 / 4;
        int c = 0;
        constexpr int U = NTW == 5 ? 2 : 4;
        for (; c + U <= nc; c += U) l1_steps<NTW, U>(kc0, c, g4, H, wrow, as_p, acc);
        for (; c < nc; ++c) l1_steps<NTW, 1>(kc0, c, g4, H, wrow, as_p, acc);
    }
    __syncthreads();                                                     // (HS lies over XS)
    // ---- layer 1's epilogue in the accumulator lanes: lane (column col, rows 4 g4 + j) ----
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        const int col = 16 * (nt0 + t) + r16;
        const float bv = a.b1[col];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 16 * tile + 4 * g4 + j;
            float v = acc[t][j] + bv;
            v = v > 0.f ? v : 0.f;
            if constexpr (TRAIN) {
                const long long gr = r0 + row;
                v = v * drop_scale(a.lo, a.hi, a.thr, a.inv, (unsigned long long)gr * H1 + col);
                if (gr < N) a.h1[(size_t)gr * H1 + col] = v;
            }
            HS[row * DEC_LDH + col] = v;
        }
    }
    __syncthreads();
    // ---- layer 2: one N-tile padded to 16, K = 80; the wave that owns the rows (arrangement FIVE: wave 0) ----
    const bool owner = NTW == 5 || wave == 0;
    if (owner) {
        f32x4 acc2 = zero4;
        const float *hp = HS + (16 * tile + r16) * DEC_LDH + 4 * g4;
        const bool cok = r16 < H2;                                       // columns 10..15: zeros, nothing read
        const float *w2r = a.w2 + (cok ? r16 : 0) * H1 + 4 * g4;
#pragma unroll
        for (int c = 0; c < H1 / 16; ++c) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(hp + 16 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = cok ? w2r[16 * c + j] : 0.f;
                acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b, acc2, 0, 0, 0);
            }
        }
        if (cok) {
            const float bv = a.b2[r16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 16 * tile + 4 * g4 + j;
                float v = acc2[j] + bv;
                v = v > 0.f ? v : 0.f;
                if constexpr (TRAIN) {
                    const long long gr = r0 + row;
                    v = v * drop_scale(a.lo, a.hi, a.thr, a.inv,
                                       (unsigned long long)N * H1 + (unsigned long long)gr * H2 + r16);
                    if (gr < N) a.h2[(size_t)gr * H2 + r16] = v;
                }
                H2S[row * DEC_LD2 + r16] = v;
            }
        }
    }
    __syncthreads();
    // ---- layer 3: ten terms per row, in column order ----
    if (owner && lane < 16) {
        const int row = 16 * tile + lane;
        const long long gr = r0 + row;
        if (gr < N) {
            float z = 0.f;
#pragma unroll
            for (int c = 0; c < H2; ++c) z = z + H2S[row * DEC_LD2 + c] * a.w3[c];
            z = z + a.b3[0];
            if (a.logit != nullptr) a.logit[gr] = z;
            if (a.prob != nullptr) a.prob[gr] = 1.f / (1.f + expf(-z));
        }
    }
}

// U k-steps of 4 of one 64-column work item of k_dec_bwd_dx (scoring_train.hip's dx_steps with fc1.weight [80][H])
template <int U>
__device__ __forceinline__ void dx_steps(int k0, bool cok, int g4, int H, const float *__restrict__ wp, const float *arow,
                                         f32x4 (&acc)[4])
{
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int k = k0 + 4 * u + g4;                                   // (k < 80 always: 80 = 5 x 16)
        const f32x4 v = *reinterpret_cast<const f32x4 *>(wp + (size_t)k * H);
        w[u] = cok ? v : zero4;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float av = arow[k0 + 4 * u];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[u][i], acc[i], 0, 0, 0);
    }
}

struct DecBwdArgs {
    long long N;
    int H;
    const float *w1, *w2, *w3;
    const float *h1, *h2, *dz;
    float *dh1, *dh2, *dx;
    unsigned lo, hi, thr;
    float inv;
};

__global__ __launch_bounds__(256) void k_dec_bwd_dx(const DecBwdArgs a)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float D1[16 * DEC_LDH];      // dh1 of the 16 rows
    __shared__ float D2[16 * DEC_LD2];                                   // dh2
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int H = a.H;
    const long long N = a.N, r0 = (long long)blockIdx.x * 16;
    if (tid < 16 * H2) {
        const int row = tid / H2, c = tid - row * H2;
        const long long gr = r0 + row;
        float v = 0.f;
        if (gr < N) {
            const float h = a.h2[(size_t)gr * H2 + c];
            const float s = drop_scale(a.lo, a.hi, a.thr, a.inv, (unsigned long long)N * H1 + (unsigned long long)gr * H2 + c);
            v = h > 0.f ? a.dz[gr] * a.w3[c] * s : 0.f;
            a.dh2[(size_t)gr * H2 + c] = v;
        }
        D2[row * DEC_LD2 + c] = v;
    }
    __syncthreads();
    for (int f = tid; f < 16 * H1; f += 256) {
        const int row = f / H1, k = f - row * H1;
        const long long gr = r0 + row;
        float v = 0.f;
        if (gr < N) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < H2; ++c) s = s + D2[row * DEC_LD2 + c] * a.w2[c * H1 + k];      // ten terms in column order
            const float h = a.h1[(size_t)gr * H1 + k];
            v = h > 0.f ? s * drop_scale(a.lo, a.hi, a.thr, a.inv, (unsigned long long)gr * H1 + k) : 0.f;
            a.dh1[(size_t)gr * H1 + k] = v;
        }
        D1[row * DEC_LDH + k] = v;
    }
    if (a.dx == nullptr) return;
    __syncthreads();
    // work item q: columns [64 q, 64 q + 64) of d_x = dh1 W1.  Lane r16 holds columns 64 q + 4 r16 + i of MFMA tile i: one
    // 16-byte load of weight row k feeds the four tiles, and a lane's four results of a row are one 16-byte store.
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const int items = (H + 63) / 64;
    for (int q = wave; q < items; q += 4) {
        const int c0 = 64 * q + 4 * r16;
        const bool cok = c0 < H;                                         // H % 4 == 0: all four columns or none
        const float *arow = D1 + r16 * DEC_LDH + g4;
        const float *wp = a.w1 + (cok ? c0 : 0);
        f32x4 acc[4] = {zero4, zero4, zero4, zero4};
#pragma unroll
        for (int k0 = 0; k0 < H1; k0 += 16) dx_steps<4>(k0, cok, g4, H, wp, arow, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long gr = r0 + 4 * g4 + j;
            if (cok && gr < N) {
                const f32x4 o = {acc[0][j], acc[1][j], acc[2][j], acc[3][j]};
                *reinterpret_cast<f32x4 *>(a.dx + (size_t)gr * H + c0) = o;
            }
        }
    }
}

// C [80][H] (+ y 80 H: partial product y) = dh1^T x over rows [y kper, (y + 1) kper).  A workgroup of four waves owns all 80
// rows of C for 64 columns: wave w its 16-column N-tile with five accumulators.  K in steps of 64 rows through LDS, every
// load of a step in flight before the first LDS store (the tiling of train_ops.hip's k_gemm_f32<true, false>).
__global__ __launch_bounds__(256) void k_dec_bwd_dw(const float *__restrict__ dh1, const float *__restrict__ x, long long N, int H,
                                                    long long kper, float *__restrict__ C)
{
    __shared__ float As[H1][GK + 1];      // [m][k]
    __shared__ float Bs[GK][65];          // [k][n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const long long n0 = (long long)blockIdx.x * 64;
    const long long kbeg = (long long)blockIdx.y * kper, kend = kbeg + kper < N ? kbeg + kper : N;
    C += (size_t)blockIdx.y * H1 * H;
    f32x4 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int PA = H1 * GK / 256, PB = 64 * GK / 256;                // elements of each operand per thread and step
    for (long long k0 = kbeg; k0 < kend; k0 += GK) {
        float va[PA], vb[PB];
#pragma unroll
        for (int t = 0; t < PA; ++t) {
            const int idx = tid + t * 256, m = idx % H1;
            const long long gk = k0 + idx / H1;
            va[t] = gk < kend ? dh1[gk * H1 + m] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < PB; ++t) {
            const int idx = tid + t * 256;
            const long long gn = n0 + (idx & 63), gk = k0 + (idx >> 6);
            vb[t] = (gn < H && gk < kend) ? x[gk * H + gn] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < PA; ++t) {
            const int idx = tid + t * 256;
            As[idx % H1][idx / H1] = va[t];
        }
#pragma unroll
        for (int t = 0; t < PB; ++t) {
            const int idx = tid + t * 256;
            Bs[idx >> 6][idx & 63] = vb[t];
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < GK; kk += 4) {
            const float b = Bs[kk + g4][wave * 16 + r16];
#pragma unroll
            for (int i = 0; i < 5; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[i * 16 + r16][kk + g4], b, acc[i], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long row = i * 16 + g4 * 4 + r, col = n0 + wave * 16 + r16;
            if (col < H) C[row * H + col] = acc[i][r];
        }
}

// Workgroups [0, sb): 64 of the 901 small sums each, lane = sum: wave w adds rows w, w + 16, ... in ascending order with one
// accumulator, the waves meet in LDS and are added first to last.  Sum o: [0, 80) d_fc1_b, [80, 880) d_fc2_w [10][80],
// [880, 890) d_fc2_b, [890, 900) d_fc3_w, 900 d_fc3_b.  Workgroups [sb, ...): d_fc1_w = the `split` partial products of
// k_dec_bwd_dw, added first to last.  Any output may be NULL.
struct DecFinArgs {
    long long N;
    int H, split, sb;
    const float *dh1, *dh2, *h1, *h2, *dz, *partial;
    float *d_w1, *d_b1, *d_w2, *d_b2, *d_w3, *d_b3;
};

__global__ __launch_bounds__(FIN_THREADS) void k_dec_bwd_fin(const DecFinArgs a)
{
#pragma clang fp contract(off)
    __shared__ float part[FIN_WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= a.sb) {
        const size_t n4 = (size_t)H1 * a.H / 4, i = (size_t)(blockIdx.x - a.sb) * FIN_THREADS + tid;
        if (i < n4) {
            const f32x4 *p = reinterpret_cast<const f32x4 *>(a.partial) + i;
            f32x4 s = p[0];
            for (int z = 1; z < a.split; ++z) s += p[(size_t)z * n4];
            reinterpret_cast<f32x4 *>(a.d_w1)[i] = s;
        }
        return;
    }
    const int o = (int)blockIdx.x * 64 + lane;
    // sum o = sum_r A[r sa + ia] * (B ? B[r sb + ib] : 1)
    const float *A = nullptr, *B = nullptr;
    float *out = nullptr;
    int sa = 0, ia = 0, sb = 0, ib = 0;
    if (o < H1) { A = a.dh1; sa = H1; ia = o; out = a.d_b1 ? a.d_b1 + o : nullptr; }
    else if (o < H1 + H2 * H1) {
        const int e = o - H1, c = e / H1, k = e - c * H1;
        A = a.dh2; sa = H2; ia = c; B = a.h1; sb = H1; ib = k; out = a.d_w2 ? a.d_w2 + e : nullptr;
    }
    else if (o < H1 + H2 * H1 + H2) { const int c = o - H1 - H2 * H1; A = a.dh2; sa = H2; ia = c; out = a.d_b2 ? a.d_b2 + c : nullptr; }
    else if (o < FIN_OUTS - 1) { const int c = o - H1 - H2 * H1 - H2; A = a.dz; sa = 1; B = a.h2; sb = H2; ib = c; out = a.d_w3 ? a.d_w3 + c : nullptr; }
    else if (o == FIN_OUTS - 1) { A = a.dz; sa = 1; out = a.d_b3; }
    float s = 0.f;
    if (out != nullptr) {
        for (long long r0 = wave; r0 < a.N; r0 += (long long)FIN_WAVES * 4) {
            float va[4], vb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long r = r0 + (long long)u * FIN_WAVES;
                const bool ok = r < a.N;
                va[u] = ok ? A[r * sa + ia] : 0.f;
                vb[u] = ok && B != nullptr ? B[r * sb + ib] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s = s + va[u] * vb[u];
        }
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && out != nullptr) {
        float t = part[0][lane];
#pragma unroll
        for (int w = 1; w < FIN_WAVES; ++w) t = t + part[w][lane];
        out[0] = t;
    }
}

bool dec_width_ok(int H) { return H >= DEC_MIN_H && H <= DEC_MAX_H && H % 4 == 0; }

int dec_max_split(int H)
{
    const int tiles = (H + 63) / 64;
    const int s = 256 / tiles;
    return s < 1 ? 1 : (s > DEC_MAX_SPLIT ? DEC_MAX_SPLIT : s);
}

struct DecWs { size_t off_dh1, off_dh2, off_part, total; };
void dec_ws(int64_t max_N, int H, DecWs &p)
{
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t n = (size_t)(max_N > 0 ? max_N : 1);
    p.off_dh1 = take(n * H1 * 4);
    p.off_dh2 = take(n * H2 * 4);
    const int ms = dec_max_split(H);
    p.off_part = take(ms > 1 ? (size_t)ms * H1 * H * 4 : 0);
    p.total = o;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool weights_ok(const zt_decoder_weights *w)
{
    return w && w->fc1_w && w->fc1_b && w->fc2_w && w->fc2_b && w->fc3_w && w->fc3_b;
}

int dec_check_width(const char *who, int H)
{
    if (dec_width_ok(H)) return ZT_OK;
    set_error("%s: H=%d unsupported (H %% 4 == 0 and %d <= H <= %d)", who, H, DEC_MIN_H, DEC_MAX_H);
    return ZT_ERR_UNSUPPORTED;
}

template <int NTW, bool TRAIN>
int dec_launch(const DecArgs &a, const DecoderPlan &p, hipStream_t s)
{
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_decoder<NTW, TRAIN>), (size_t)p.lds_bytes));
    k_decoder<NTW, TRAIN><<<(unsigned)p.grid, p.threads, (size_t)p.lds_bytes, s>>>(a);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

int dec_forward(const char *who, const float *x, int64_t N, int32_t H, const zt_decoder_weights *w, float *logit, float *prob,
                float *h1, float *h2, bool training, float p, uint64_t seed, void *stream)
{
    if (N < 0 || H < 0 || !weights_ok(w) || (N > 0 && !x) || !aligned16(x) || !aligned16(w->fc1_w) || !(p >= 0.f) || !(p < 1.f) ||
        (training && N > 0 && (!logit || !h1 || !h2))) {
        set_error("%s: bad argument", who);
        return ZT_ERR_ARG;
    }
    const int rc = dec_check_width(who, H);
    if (rc != ZT_OK) return rc;
    if (N == 0) return ZT_OK;
    const DecoderPlan pl = decoder_plan(N, H, training, g_decoder_arrangement);
    if (pl.grid > 0x7fffffffll) {
        set_error("%s: N=%lld is beyond one launch", who, (long long)N);
        return ZT_ERR_ARG;
    }
    DecArgs a;
    a.x = x; a.N = N; a.H = H;
    a.w1 = w->fc1_w; a.b1 = w->fc1_b; a.w2 = w->fc2_w; a.b2 = w->fc2_b; a.w3 = w->fc3_w; a.b3 = w->fc3_b;
    a.logit = logit; a.prob = prob; a.h1 = h1; a.h2 = h2;
    a.lo = (unsigned)(seed & 0xffffffffull); a.hi = (unsigned)(seed >> 32);
    a.thr = drop_threshold(p);
    a.inv = a.thr ? 1.f / (1.f - p) : 1.f;
    hipStream_t s = (hipStream_t)stream;
    if (pl.arrangement == DEC_ARR_ONE) return training ? dec_launch<5, true>(a, pl, s) : dec_launch<5, false>(a, pl, s);
    return training ? dec_launch<1, true>(a, pl, s) : dec_launch<1, false>(a, pl, s);
}

}  // namespace

// The one place that picks the forward's arrangement, the rows per workgroup and the K-chunk, and the backward's split of
// d_fc1_w (host code only).  Arrangement: five waves per 16 rows at EVERY N.  Measured on an MI355X (tools/decoder_time.py, eval
// forward, microseconds per call, one wave / five waves per tile, both in one process round by round): 200x300 27.4 / 27.6,
// 600x300 26.9 / 26.3, 4096x300 27.3 / 26.9, 16384x300 27.1 / 27.3 -- ties inside the five-wave form's own spread of 2-6 %,
// the host's launch cost -- and 200x516 32.4 / 26.7, 65536x300 70.7 / 62.8, where the five-wave form wins by more than either
// spread.  There is no crossover in the measured range; the one-wave form stays reachable through the pin, for the tests that
// hold the two against each other (they give the same bits).
namespace zt {
DecoderPlan decoder_plan(int64_t N, int H, bool training, int pin)
{
    DecoderPlan p = {};
    if (N < 0 || !dec_width_ok(H)) return p;
    (void)training;                                                      // (both entries take the same arrangement)
    const int arr = pin == DEC_ARR_ONE ? DEC_ARR_ONE : DEC_ARR_FIVE;
    p.arrangement = arr;
    p.waves = arr == DEC_ARR_ONE ? 4 : 5;
    p.threads = 64 * p.waves;
    p.rows = arr == DEC_ARR_ONE ? 64 : 16;
    p.k_chunk = DEC_KC;
    p.grid = (N + p.rows - 1) / p.rows;
    p.lds_bytes = (long long)p.rows * DEC_LDX * 4;
    // d_fc1_w: K = N in partial products of whole 64-row steps, at least two steps each
    const long long steps = (N + GK - 1) / GK;
    const long long want = steps / 2 < 1 ? 1 : steps / 2;
    int split = (int)(want < dec_max_split(H) ? want : dec_max_split(H));
    const long long kper = (steps + split - 1) / split * GK;
    split = N > 0 ? (int)((N + kper - 1) / kper) : 1;
    p.split = split;
    p.k_per = kper;
    return p;
}
}  // namespace zt

extern "C" int zt_node_decoder_plan(int64_t N, int32_t H, int32_t training, int64_t *out)
{
    if (!out || N < 0) {
        set_error("zt_node_decoder_plan: bad argument");
        return ZT_ERR_ARG;
    }
    const int rc = dec_check_width("zt_node_decoder_plan", H);
    if (rc != ZT_OK) return rc;
    const DecoderPlan p = decoder_plan(N, H, training != 0, g_decoder_arrangement);
    out[0] = p.arrangement; out[1] = p.waves; out[2] = p.rows; out[3] = p.k_chunk; out[4] = p.grid; out[5] = p.lds_bytes;
    out[6] = p.split; out[7] = p.k_per;
    return ZT_OK;
}

extern "C" int zt_node_decoder(const float *x_dev, int64_t N, int32_t H, const zt_decoder_weights *weights, float *logit_dev,
                               float *prob_dev, void *stream)
{
    return dec_forward("zt_node_decoder", x_dev, N, H, weights, logit_dev, prob_dev, nullptr, nullptr, false, 0.f, 0, stream);
}

extern "C" int zt_node_decoder_train_forward(const float *x_dev, int64_t N, int32_t H, const zt_decoder_weights *weights, float p,
                                             uint64_t seed, float *logit_dev, float *h1_dev, float *h2_dev, void *stream)
{
    return dec_forward("zt_node_decoder_train_forward", x_dev, N, H, weights, logit_dev, nullptr, h1_dev, h2_dev, true, p, seed,
                       stream);
}

extern "C" int64_t zt_node_decoder_train_workspace_bytes(int64_t max_N, int32_t H)
{
    if (max_N < 0 || !dec_width_ok(H)) return -1;
    DecWs p;
    dec_ws(max_N, H, p);
    return (int64_t)p.total;
}

extern "C" int zt_node_decoder_train_backward(const float *x_dev, int64_t N, int32_t H, const zt_decoder_weights *weights,
                                              const float *h1_dev, const float *h2_dev, const float *dlogit_dev, float p,
                                              uint64_t seed, float *d_x_dev, float *d_fc1_w_dev, float *d_fc1_b_dev,
                                              float *d_fc2_w_dev, float *d_fc2_b_dev, float *d_fc3_w_dev, float *d_fc3_b_dev,
                                              void *workspace_dev, int64_t ws_max_N, void *stream)
{
    if (N < 0 || H < 0 || ws_max_N < N || !weights_ok(weights) || !(p >= 0.f) || !(p < 1.f) ||
        (N > 0 && (!x_dev || !h1_dev || !h2_dev || !dlogit_dev || !workspace_dev)) || !aligned16(x_dev) || !aligned16(weights->fc1_w) ||
        !aligned16(d_x_dev) || !aligned16(d_fc1_w_dev) || !aligned16(workspace_dev)) {
        set_error("zt_node_decoder_train_backward: bad argument");
        return ZT_ERR_ARG;
    }
    const int rc = dec_check_width("zt_node_decoder_train_backward", H);
    if (rc != ZT_OK) return rc;
    if (N == 0) return ZT_OK;
    if ((N + 15) / 16 > 0x7fffffffll) {
        set_error("zt_node_decoder_train_backward: N=%lld is beyond one launch", (long long)N);
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    DecWs ws;
    dec_ws(ws_max_N, H, ws);
    char *wp = reinterpret_cast<char *>(workspace_dev);
    float *dh1 = reinterpret_cast<float *>(wp + ws.off_dh1), *dh2 = reinterpret_cast<float *>(wp + ws.off_dh2);
    float *partial = reinterpret_cast<float *>(wp + ws.off_part);
    DecBwdArgs b;
    b.N = N; b.H = H; b.w1 = weights->fc1_w; b.w2 = weights->fc2_w; b.w3 = weights->fc3_w;
    b.h1 = h1_dev; b.h2 = h2_dev; b.dz = dlogit_dev; b.dh1 = dh1; b.dh2 = dh2; b.dx = d_x_dev;
    b.lo = (unsigned)(seed & 0xffffffffull); b.hi = (unsigned)(seed >> 32);
    b.thr = drop_threshold(p);
    b.inv = b.thr ? 1.f / (1.f - p) : 1.f;
    k_dec_bwd_dx<<<(unsigned)((N + 15) / 16), 256, 0, s>>>(b);
    int split = 1;
    if (d_fc1_w_dev != nullptr) {
        const DecoderPlan pl = decoder_plan(N, H, true, 0);
        split = pl.split;
        const dim3 grid((unsigned)((H + 63) / 64), (unsigned)split);
        k_dec_bwd_dw<<<grid, 256, 0, s>>>(dh1, x_dev, N, H, pl.k_per, split > 1 ? partial : d_fc1_w_dev);
    }
    if (split > 1 || d_fc1_b_dev || d_fc2_w_dev || d_fc2_b_dev || d_fc3_w_dev || d_fc3_b_dev) {
        DecFinArgs f;
        f.N = N; f.H = H; f.split = split; f.sb = (FIN_OUTS + 63) / 64;
        f.dh1 = dh1; f.dh2 = dh2; f.h1 = h1_dev; f.h2 = h2_dev; f.dz = dlogit_dev; f.partial = partial;
        f.d_w1 = d_fc1_w_dev; f.d_b1 = d_fc1_b_dev; f.d_w2 = d_fc2_w_dev; f.d_b2 = d_fc2_b_dev; f.d_w3 = d_fc3_w_dev; f.d_b3 = d_fc3_b_dev;
        const size_t n4 = (size_t)H1 * H / 4;
        const unsigned rb = split > 1 ? (unsigned)((n4 + FIN_THREADS - 1) / FIN_THREADS) : 0u;
        k_dec_bwd_fin<<<f.sb + rb, FIN_THREADS, 0, s>>>(f);
    }
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
