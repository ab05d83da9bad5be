// Link scoring and link-prediction metrics on the device.
//
// zt_affinity replaces TGN.compute_edge_probabilities' scorer (reference model/tgn_model.py:185-188 with
// MergeLayer, utils/util.py:14-26):
//   score = fc2(relu(fc1(cat[x1, x2]))),  x1 = [src | src], x2 = [dst | neg]  ->  sigmoid
// for the B positive pairs (src, dst) and the B negative pairs (src, neg) of a batch whose embeddings
// [3B][H] = [src | dst | neg] the aggregation has just written.  fc1 acts on a concatenation, so
// fc1([a | b]) = W_a a + W_b b + b1 and W_a src is SHARED by an edge's two pairs: three [16 x H] x [H x 16] products
// per 16 edges and N-tile instead of the reference's four.
//
// Organisation (the batch is small, the chain of dependent memory round trips is what costs): one WAVE per N-tile of
// the hidden layer keeps its 16 columns of W_a and W_b in registers and strides over tiles of 16 edges; the A operand
// comes straight from the embedding rows into the MFMA lanes (float4 at columns 16 c + 4 g: the k order the padded
// weights have); bias, ReLU and fc2's weight are applied in the accumulator lanes and summed over the wave's 16 columns
// with four DPP rotations.  The N-tiles' partial scores meet in memory: the LAST wave to arrive for a tile (one counter
// per tile, reset by that wave) adds them first to last -- a fixed order, so the probabilities do not depend on which
// wave finishes when -- and applies fc2's bias and the sigmoid.
//
// The two kernels of that organisation (k_affinity, k_affinity_tiled) are specialised for the reference's default width: hidden
// widths 200 and 300 (round_up16(H) = 16 KC, KC = 13 or 19 a template argument: weights and accumulators live in registers).
// Every other width the training scorer takes (H % 4 == 0, 4 <= H <= 768: D = 172 or 256 with one or two T-PPR models) runs
// two generic kernels in which K and N run over H at run time: k_affinity_gen (latency form: the weights are streamed, not
// kept) and k_affinity_gen_tiled (the training scorer's forward, scoring_fwd.hpp, without the hidden rows).  Which kernel a
// batch takes is decided in ONE place, affinity_kernel_plan (host code).
//
// zt_link_metrics replaces the per-batch scikit-learn calls of evaluation/evaluation.py:34-45 and train.py:218-227
// (average_precision_score, roc_auc_score, accuracy of argmax) with ONE single-workgroup kernel: bitonic sort of the 2B
// scores in LDS, two scans (true positives; start of every run of equal scores) and the two curve sums over the distinct
// thresholds in float64, ties handled as scikit-learn does (zebra_amd/evaluation.py states the definitions).  Beyond 8192
// pairs a second form sorts the positives' and the negatives' 32-bit keys as two runs (k_link_metrics_split); which form a
// batch takes is decided in ONE place, link_metrics_plan (host code).
#include "common.hpp"
#include "scoring_fwd.hpp"

using namespace zt;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int round_up16(int x) { return (x + 15) / 16 * 16; }

// fc1.weight [H][2H], fc1.bias [H], fc2.weight [1][H]  ->  Wa_p, Wb_p [Hp][Hp] (zero padded), b1_p [Hp], w2_p [Hp]
__global__ void k_pack_affinity(const float *__restrict__ fc1_w, const float *__restrict__ fc1_b, const float *__restrict__ fc2_w,
                                int H, int Hp, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int mat = Hp * Hp;
    if (i < 2 * mat) {
        const int which = i / mat, r = (i % mat) / Hp, c = i % Hp;
        out[i] = (r < H && c < H) ? fc1_w[(size_t)r * 2 * H + which * H + c] : 0.f;
    } else if (i < 2 * mat + Hp) {
        const int c = i - 2 * mat;
        out[i] = c < H ? fc1_b[c] : 0.f;
    } else if (i < 2 * mat + 2 * Hp) {
        const int c = i - 2 * mat - Hp;
        out[i] = c < H ? fc2_w[c] : 0.f;
    }
}

template <int KC>
__global__ __launch_bounds__(64) void k_affinity(const float *__restrict__ emb, long long B, int H, const float *__restrict__ packed,
                                                 const float *__restrict__ fc2_b, float *part, int *counters, float *__restrict__ prob)
{
    constexpr int Hp = KC * 16, NT = KC;
    const int lane = threadIdx.x, r16 = lane & 15, g4 = lane >> 4;
    const int nt = blockIdx.y, col = 16 * nt + r16;
    const float *Wa = packed, *Wb = packed + (size_t)Hp * Hp, *b1p = Wb + (size_t)Hp * Hp, *w2p = b1p + Hp;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 wa[KC], wb[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        wa[c] = *reinterpret_cast<const f32x4 *>(Wa + (size_t)col * Hp + 16 * c + 4 * g4);
        wb[c] = *reinterpret_cast<const f32x4 *>(Wb + (size_t)col * Hp + 16 * c + 4 * g4);
    }
    const float b1v = b1p[col], w2v = w2p[col], b2v = fc2_b[0];
    bool cin[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) cin[c] = 16 * c + 4 * g4 < H;           // H % 4 == 0: all four columns or none
    const long long tiles = (B + 15) / 16, Bp = tiles * 16;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long e0 = t * 16;
        const bool rin = e0 + r16 < B;
        const float *ps = emb + (size_t)(rin ? e0 + r16 : 0) * H + 4 * g4, *pd = ps + (size_t)B * H, *pn = pd + (size_t)B * H;
        f32x4 as[KC], ad[KC], an[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const bool ok = rin && cin[c];
            as[c] = ok ? *reinterpret_cast<const f32x4 *>(ps + 16 * c) : zero4;
            ad[c] = ok ? *reinterpret_cast<const f32x4 *>(pd + 16 * c) : zero4;
            an[c] = ok ? *reinterpret_cast<const f32x4 *>(pn + 16 * c) : zero4;
        }
        f32x4 au = zero4, ap = zero4, ang = zero4;
#pragma unroll
        for (int c = 0; c < KC; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                au = __builtin_amdgcn_mfma_f32_16x16x4f32(as[c][j], wa[c][j], au, 0, 0, 0);
                ap = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[c][j], wb[c][j], ap, 0, 0, 0);
                ang = __builtin_amdgcn_mfma_f32_16x16x4f32(an[c][j], wb[c][j], ang, 0, 0, 0);
            }
        // lane (column col, edges 4 g4 + j): relu(fc1) x fc2's weight, summed over the wave's 16 columns
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float hp = au[j] + ap[j] + b1v, hn = au[j] + ang[j] + b1v;
            hp = (hp > 0.f ? hp : 0.f) * w2v;
            hn = (hn > 0.f ? hn : 0.f) * w2v;
            hp += dpp_f<0x128>(hp); hp += dpp_f<0x124>(hp); hp += dpp_f<0x122>(hp); hp += dpp_f<0x121>(hp);
            hn += dpp_f<0x128>(hn); hn += dpp_f<0x124>(hn); hn += dpp_f<0x122>(hn); hn += dpp_f<0x121>(hn);
            if (r16 == 0) {                                              // (lane 0 of the row: ITS association of the 16 terms)
                part[((size_t)nt * 2 + 0) * Bp + e0 + 4 * g4 + j] = hp;
                part[((size_t)nt * 2 + 1) * Bp + e0 + 4 * g4 + j] = hn;
            }
        }
        __threadfence();
        int done = 0;
        if (lane == 0) done = atomicAdd(&counters[t], 1);
        done = __builtin_amdgcn_readfirstlane(done);
        if (done == NT - 1) {                                            // the last N-tile of this tile to arrive
            __threadfence();
            if (lane < 32) {
                const int e = lane & 15, which = lane >> 4;
                float pv[NT];                                            // all of them requested before the first is looked at
#pragma unroll
                for (int q = 0; q < NT; ++q)
                    pv[q] = __int_as_float(ld_agent(reinterpret_cast<const int *>(part + ((size_t)q * 2 + which) * Bp + e0 + e)));
                float sc = 0.f;
#pragma unroll
                for (int q = 0; q < NT; ++q) sc += pv[q];
                sc += b2v;
                if (e0 + e < B) prob[(size_t)which * B + e0 + e] = 1.f / (1.f + expf(-sc));
            }
            if (lane == 0) atomicExch(&counters[t], 0);                 // ready for the next launch
        }
    }
}

// Large batches (B > 2048: C5).  The wave-per-N-tile kernel above reads every embedding row once per N-tile (19 x) and
// runs one wave per SIMD: 190 us at B = 4096.  Here a workgroup of four waves owns 32 edges: their 96 embedding rows are
// staged in LDS once (118 KB, every load in flight before the first store), each wave takes every fourth N-tile with all
// six row tiles in accumulators (120 registers) and streams its own slice of W_a / W_b from L2 a k-chunk ahead -- each
// weight is read once per workgroup, each embedding row once per launch.  The waves' partial scores meet in LDS and
// are added in wave order.
template <int KC, int ET>           // ET: edges per workgroup, 16 (mid-size batches: more workgroups) or 32
__global__ __launch_bounds__(256, ET == 16 ? 2 : 1) void k_affinity_tiled(const float *__restrict__ emb, long long B, int H, const float *__restrict__ packed,
                                                           const float *__restrict__ fc2_b, float *__restrict__ prob)
{
    constexpr int Hp = KC * 16, NT = KC, NQ = (NT + 3) / 4, ldA = Hp + 4, ROWS = 3 * ET, H4MAX = Hp / 4, EM = ET / 16, MTS = 3 * EM;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *A = reinterpret_cast<float *>(smem);                          // [3 ET][ldA]: src rows, dst rows, neg rows of the tile
    float *part = A + ROWS * ldA;                                        // [4 waves][2][ET]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const float *Wa = packed, *Wb = packed + (size_t)Hp * Hp, *b1p = Wb + (size_t)Hp * Hp, *w2p = b1p + Hp;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const long long e0 = (long long)blockIdx.x * ET;
    const int h4 = H / 4;                                                // float4 per row (H % 4 == 0)
    // ---- stage the 96 rows: zero beyond the batch and beyond H ----
    constexpr int NST = (ROWS * H4MAX + 255) / 256;
    f32x4 st[NST];
#pragma unroll
    for (int q = 0; q < NST; ++q) {
        const int f = tid + q * 256, row = f / H4MAX, c4 = f - row * H4MAX;
        const long long e = e0 + (row & (ET - 1));
        const bool ok = row < ROWS && c4 < h4 && e < B;
        st[q] = ok ? *reinterpret_cast<const f32x4 *>(emb + ((size_t)(row / ET) * B + e) * H + 4 * c4) : zero4;
    }
    // this wave's first weight chunk rides with the staging loads
    bool live[NQ];
    int colq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { live[q] = wave + 4 * q < NT; colq[q] = 16 * (live[q] ? wave + 4 * q : 0) + r16; }
    f32x4 wa[2][NQ], wb[2][NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        wa[0][q] = *reinterpret_cast<const f32x4 *>(Wa + (size_t)colq[q] * Hp + 4 * g4);
        wb[0][q] = *reinterpret_cast<const f32x4 *>(Wb + (size_t)colq[q] * Hp + 4 * g4);
    }
#pragma unroll
    for (int q = 0; q < NST; ++q) {
        const int f = tid + q * 256, row = f / H4MAX, c4 = f - row * H4MAX;
        if (row < ROWS) *reinterpret_cast<f32x4 *>(A + row * ldA + 4 * c4) = st[q];
    }
    __syncthreads();
    f32x4 acc[MTS][NQ];
#pragma unroll
    for (int mt = 0; mt < MTS; ++mt)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[mt][q] = zero4;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        if (c + 1 < KC) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                wa[(c + 1) & 1][q] = *reinterpret_cast<const f32x4 *>(Wa + (size_t)colq[q] * Hp + 16 * (c + 1) + 4 * g4);
                wb[(c + 1) & 1][q] = *reinterpret_cast<const f32x4 *>(Wb + (size_t)colq[q] * Hp + 16 * (c + 1) + 4 * g4);
            }
        }
        f32x4 a[MTS];
#pragma unroll
        for (int mt = 0; mt < MTS; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(A + (16 * mt + r16) * ldA + 16 * c + 4 * g4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (!live[q]) continue;
#pragma unroll
                for (int mt = 0; mt < MTS; ++mt)
                    acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][j], mt < EM ? wa[c & 1][q][j] : wb[c & 1][q][j], acc[mt][q], 0, 0, 0);
            }
    }
    // ---- relu(fc1) x fc2's weight over this wave's columns: lane (column, edges 16 et + 4 g4 + j) ----
    float sp[EM][4], sn[EM][4];
#pragma unroll
    for (int et = 0; et < EM; ++et)
#pragma unroll
        for (int j = 0; j < 4; ++j) { sp[et][j] = 0.f; sn[et][j] = 0.f; }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (!live[q]) continue;
        const float b1v = b1p[colq[q]], w2v = w2p[colq[q]];
#pragma unroll
        for (int et = 0; et < EM; ++et)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float hp = acc[et][q][j] + acc[EM + et][q][j] + b1v, hn = acc[et][q][j] + acc[2 * EM + et][q][j] + b1v;
                sp[et][j] += (hp > 0.f ? hp : 0.f) * w2v;
                sn[et][j] += (hn > 0.f ? hn : 0.f) * w2v;
            }
    }
#pragma unroll
    for (int et = 0; et < EM; ++et)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = sp[et][j], y = sn[et][j];
            x += dpp_f<0x128>(x); x += dpp_f<0x124>(x); x += dpp_f<0x122>(x); x += dpp_f<0x121>(x);
            y += dpp_f<0x128>(y); y += dpp_f<0x124>(y); y += dpp_f<0x122>(y); y += dpp_f<0x121>(y);
            if (r16 == 0) { part[(wave * 2 + 0) * ET + 16 * et + 4 * g4 + j] = x; part[(wave * 2 + 1) * ET + 16 * et + 4 * g4 + j] = y; }
        }
    __syncthreads();
    if (tid < 2 * ET) {
        const int e = tid & (ET - 1), which = tid / ET;
        float sc = part[(0 * 2 + which) * ET + e];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) sc += part[(wv * 2 + which) * ET + e];
        sc += fc2_b[0];
        if (e0 + e < B) prob[(size_t)which * B + e0 + e] = 1.f / (1.f + expf(-sc));
    }
}

// ---------------------------------------------------------------------------------------------------------
// any hidden width: H % 4 == 0, 4 <= H <= 768
// ---------------------------------------------------------------------------------------------------------
// U k-chunks of 16 of k_affinity_gen, from chunk c (chunks beyond NT: clamped addresses, zero operands): the wave's 16 rows of
// the packed W_a / W_b and its three embedding rows, every load of the round issued before the round's first MFMA
constexpr int AG_U = 8;
template <int U>
__device__ __forceinline__ void gen_chunks(int c, int NT, int g4, int H, bool rin, const float *__restrict__ wa_row,
                                           const float *__restrict__ wb_row, const float *__restrict__ ps, const float *__restrict__ pd,
                                           const float *__restrict__ pn, f32x4 &au, f32x4 &ap, f32x4 &ang)
{
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 wa[U], wb[U], as[U], ad[U], an[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool live = c + u < NT;
        const int k = 16 * (live ? c + u : NT - 1) + 4 * g4;            // < Hp: inside the padded weight rows
        const bool kin = k < H;                                         // H % 4 == 0: all four columns or none
        const int ke = kin ? k : H - 4;                                 // (the loads: unconditional, from clamped addresses)
        const f32x4 va = *reinterpret_cast<const f32x4 *>(wa_row + k), vb = *reinterpret_cast<const f32x4 *>(wb_row + k);
        const f32x4 vs = *reinterpret_cast<const f32x4 *>(ps + ke), vd = *reinterpret_cast<const f32x4 *>(pd + ke);
        const f32x4 vn = *reinterpret_cast<const f32x4 *>(pn + ke);
        const bool ok = live && kin && rin;
        wa[u] = live ? va : zero4;
        wb[u] = live ? vb : zero4;
        as[u] = ok ? vs : zero4;
        ad[u] = ok ? vd : zero4;
        an[u] = ok ? vn : zero4;
    }
    __builtin_amdgcn_sched_barrier(0);                                   // (or the scheduler sinks every load to its first use)
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            au = __builtin_amdgcn_mfma_f32_16x16x4f32(as[u][j], wa[u][j], au, 0, 0, 0);
            ap = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[u][j], wb[u][j], ap, 0, 0, 0);
            ang = __builtin_amdgcn_mfma_f32_16x16x4f32(an[u][j], wb[u][j], ang, 0, 0, 0);
        }
}

// Generic latency form (small batches): one wave per (16-edge tile, N-tile), as k_affinity.  At the batch sizes it serves a wave
// sees ONE tile, so weights kept in registers would buy nothing (and NT = 48 chunks of two matrices would not fit): the wave
// streams its 16 rows of the packed, zero-padded W_a / W_b [Hp][Hp] in rounds of AG_U k-chunks beside the embedding rows.  The
// N-tiles' partial scores meet in the same part / counters workspace; the last wave to arrive adds the NT = Hp / 16 partials (up
// to 48) first to last and resets the counter.  No float atomics: two launches give the same bits.
__global__ __launch_bounds__(64) void k_affinity_gen(const float *__restrict__ emb, long long B, int H, const float *__restrict__ packed,
                                                     const float *__restrict__ fc2_b, float *part, int *counters, float *__restrict__ prob)
{
    const int Hp = round_up16(H), NT = Hp / 16;
    const int lane = threadIdx.x, r16 = lane & 15, g4 = lane >> 4;
    const int nt = blockIdx.y, col = 16 * nt + r16;                      // col < Hp: the padded rows are zero
    const float *Wa = packed, *Wb = packed + (size_t)Hp * Hp, *b1p = Wb + (size_t)Hp * Hp, *w2p = b1p + Hp;
    const float *wa_row = Wa + (size_t)col * Hp, *wb_row = Wb + (size_t)col * Hp;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float b1v = b1p[col], w2v = w2p[col], b2v = fc2_b[0];
    const long long tiles = (B + 15) / 16, Bp = tiles * 16;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long e0 = t * 16;
        const bool rin = e0 + r16 < B;
        const float *ps = emb + (size_t)(rin ? e0 + r16 : 0) * H, *pd = ps + (size_t)B * H, *pn = pd + (size_t)B * H;
        f32x4 au = zero4, ap = zero4, ang = zero4;
        for (int c = 0; c < NT; c += AG_U) gen_chunks<AG_U>(c, NT, g4, H, rin, wa_row, wb_row, ps, pd, pn, au, ap, ang);
        // lane (column col, edges 4 g4 + j): relu(fc1) x fc2's weight, summed over the wave's 16 columns
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float hp = au[j] + ap[j] + b1v, hn = au[j] + ang[j] + b1v;
            hp = (hp > 0.f ? hp : 0.f) * w2v;
            hn = (hn > 0.f ? hn : 0.f) * w2v;
            hp += dpp_f<0x128>(hp); hp += dpp_f<0x124>(hp); hp += dpp_f<0x122>(hp); hp += dpp_f<0x121>(hp);
            hn += dpp_f<0x128>(hn); hn += dpp_f<0x124>(hn); hn += dpp_f<0x122>(hn); hn += dpp_f<0x121>(hn);
            if (r16 == 0) {                                              // (lane 0 of the row: ITS association of the 16 terms)
                part[((size_t)nt * 2 + 0) * Bp + e0 + 4 * g4 + j] = hp;
                part[((size_t)nt * 2 + 1) * Bp + e0 + 4 * g4 + j] = hn;
            }
        }
        __threadfence();
        int done = 0;
        if (lane == 0) done = atomicAdd(&counters[t], 1);
        done = __builtin_amdgcn_readfirstlane(done);
        if (done == NT - 1) {                                            // the last N-tile of this tile to arrive
            __threadfence();
            if (lane < 32) {
                const int e = lane & 15, which = lane >> 4;
                float sc = 0.f;
                for (int q0 = 0; q0 < NT; q0 += 8) {                     // eight partials requested before the first is looked at
                    float pv[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int q = q0 + i < NT ? q0 + i : NT - 1;
                        pv[i] = __int_as_float(ld_agent(reinterpret_cast<const int *>(part + ((size_t)q * 2 + which) * Bp + e0 + e)));
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (q0 + i < NT) sc += pv[i];
                }
                sc += b2v;
                if (e0 + e < B) prob[(size_t)which * B + e0 + e] = 1.f / (1.f + expf(-sc));
            }
            if (lane == 0) atomicExch(&counters[t], 0);                 // ready for the next launch
        }
    }
}

// Generic tiled form (large batches).  k_affinity_tiled cannot be stretched: at NT = 48 its acc[3][NQ] beside the double-buffered
// weights exceed the 256 registers its launch bounds allow.  This is the training scorer's forward (scoring_fwd.hpp: sixteen
// waves own 16 edges, their 48 rows staged in LDS once, wave w takes N-tiles w, w + 16, ... with three accumulators, partials
// added in wave order) without the hidden rows.  It reads the MODULE'S OWN parameters (fc1.weight [H][2H] as it lies, 16-byte
// aligned), not the packed copy: the body is the training kernel's, instruction for instruction, and a weight is read once per
// workgroup either way.
__global__ __launch_bounds__(SCORE_THREADS) void k_affinity_gen_tiled(const float *__restrict__ emb, long long B, int H,
                                                                      const float *__restrict__ fc1_w, const float *__restrict__ fc1_b,
                                                                      const float *__restrict__ fc2_w, const float *__restrict__ fc2_b,
                                                                      float *__restrict__ prob)
{
    score_fwd_body<false>(emb, B, H, fc1_w, fc1_b, fc2_w, fc2_b, prob, nullptr);
}

// ---------------------------------------------------------------------------------------------------------
// metrics
// ---------------------------------------------------------------------------------------------------------
constexpr int MT_THREADS = 1024;
constexpr int MT_MAX = 16384;            // scores per call (2B) of the single form: 128 KB of LDS keys

// float -> unsigned whose ascending order is the DESCENDING order of the floats (NaN-free scores).  -0.0 takes +0.0's key:
// the two compare equal, so they are ONE threshold of the curves (by their bits they would be two)
__device__ __forceinline__ unsigned desc_key(float x)
{
    const unsigned bits = __float_as_uint(x);
    const unsigned u = bits == 0x80000000u ? 0u : bits;
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}

__global__ __launch_bounds__(MT_THREADS) void k_link_metrics(const float *__restrict__ pos, const float *__restrict__ neg, int B,
                                                             int n2, double *out, int accumulate, double *row)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64 *key = reinterpret_cast<u64 *>(smem);                             // [n2] (score key << 32) | label
    __shared__ double red[3][MT_THREADS / 64];
    __shared__ int part_t[MT_THREADS], part_s[MT_THREADS];
    const int tid = threadIdx.x, n = 2 * B;
    for (int i = tid; i < n2; i += MT_THREADS) {
        u64 kv = ~0ull;                                                   // padding sorts last
        if (i < n) kv = ((u64)desc_key(i < B ? pos[i] : neg[i - B]) << 32) | (i < B ? 1u : 0u);
        key[i] = kv;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += MT_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 a = key[i], b = key[l];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { key[i] = b; key[l] = a; }
                }
            }
            __syncthreads();
        }
    // every thread owns a contiguous chunk: true positives (sum scan) and run starts (max scan)
    const int per = n2 / MT_THREADS > 0 ? n2 / MT_THREADS : 1;
    const int lo = tid * per, hi = lo + per < n2 ? lo + per : n2;
    int tsum = 0, smax = -1;
    for (int i = lo; i < hi && i < n; ++i) {
        tsum += (int)(key[i] & 1u);
        if (i == 0 || (unsigned)(key[i] >> 32) != (unsigned)(key[i - 1] >> 32)) smax = i;
    }
    part_t[tid] = tsum; part_s[tid] = smax;
    __syncthreads();
    if (tid == 0) {                                                       // 1024 partials: a serial pass is microseconds
        int t = 0, sm = -1;
        for (int q = 0; q < MT_THREADS; ++q) {
            const int a = part_t[q], b = part_s[q];
            part_t[q] = t; part_s[q] = sm;                                // exclusive prefixes
            t += a; if (b > sm) sm = b;
        }
    }
    __syncthreads();
    // second pass: at the LAST element of every run (a distinct threshold) add the curve terms.  tps / fps "before the
    // run" are those at index (run start - 1); since tps is needed at arbitrary earlier indices, every thread re-walks
    // its chunk carrying (tps, tps at the start of the current run)
    double ap = 0.0, auc = 0.0, acc = 0.0;
    {
        int t = part_t[tid], start = part_s[tid];
        // true positives before the run that is open at the chunk's first element: walk back is not possible, so the
        // prefix pass below carries it: tps_before_run = tps at (start - 1)
        // (computed by a third, tiny scan: the value of the sum scan at each run start)
        int t_before = 0;
        if (start >= 0) {
            // tps at start - 1 = number of labels in [0, start): chunk prefixes + a walk inside the chunk that holds `start`
            const int owner = start / per;
            int c = part_t[owner];
            for (int i = owner * per; i < start; ++i) c += (int)(key[i] & 1u);
            t_before = c;
        }
        const double np_ = (double)B, nn_ = (double)(n - B);
        for (int i = lo; i < hi && i < n; ++i) {
            if (i == 0 || (unsigned)(key[i] >> 32) != (unsigned)(key[i - 1] >> 32)) { start = i; t_before = t; }
            t += (int)(key[i] & 1u);
            const bool last = (i == n - 1) || (unsigned)(key[i + 1] >> 32) != (unsigned)(key[i] >> 32);
            if (last) {
                const double tps = t, fps = (double)(i + 1) - tps;
                const double tb = t_before, fb = (double)start - tb;
                ap += (tps / np_ - tb / np_) * (tps / (tps + fps));
                auc += (fps / nn_ - fb / nn_) * (tps / np_ + tb / np_) * 0.5;
            }
        }
    }
    for (int i = tid; i < B; i += MT_THREADS) acc += pos[i] >= neg[i] ? 1.0 : 0.0;
    // fixed-order reduction: lanes by DPP-free shuffles, waves through LDS, thread 0 last
    for (int d = 32; d > 0; d >>= 1) { ap += __shfl_down(ap, d); auc += __shfl_down(auc, d); acc += __shfl_down(acc, d); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = ap; red[1][tid >> 6] = auc; red[2][tid >> 6] = acc; }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, u = 0.0, c = 0.0;
        for (int q = 0; q < MT_THREADS / 64; ++q) { a += red[0][q]; u += red[1][q]; c += red[2][q]; }
        c /= (double)B;
        if (accumulate) { out[0] += a; out[1] += u; out[2] += c; }
        else { out[0] = a; out[1] = u; out[2] = c; }
        if (row != nullptr) { row[0] = a; row[1] = u; row[2] = c; }
    }
}

// first index of an ascending run a[0 .. n) whose key is >= v (lower) / > v (upper)
__device__ __forceinline__ int run_lower(const unsigned *a, int n, unsigned v)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ int run_upper(const unsigned *a, int n, unsigned v)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] <= v) lo = m + 1; else hi = m; }
    return lo;
}

// The wide form (8192 < B <= 16384 pairs): 2B u64 words do not fit the 160 KB of LDS, 2B 32-bit keys do.  The label leaves the
// key: the B positive keys and the B negative keys are sorted as TWO runs (each padded to m2, one bitonic network over both:
// a compare-exchange partner i ^ j, j < m2, never leaves its half) and the curves are read off the pair.  Per distinct score
// the sums need only how many positives and how many negatives lie at or above it -- a position in the score's own run and a
// binary search in the other; the order inside a run of equal scores never matters.  The terms are k_link_metrics' own, in the
// same float64 expressions.  A threshold that no positive score takes adds (R_n - R_{n-1}) P_n = 0 to the average precision,
// one that no negative score takes adds a trapezoid of width 0 to the AUC: the positives' distinct keys carry the first sum,
// the negatives' the second.  Thread t takes elements t, t + 1024, ... of both runs; lanes, waves and thread 0 add in a fixed
// order as above.
__global__ __launch_bounds__(MT_THREADS) void k_link_metrics_split(const float *__restrict__ pos, const float *__restrict__ neg, int B,
                                                                   int m2, double *out, int accumulate, double *row)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned *key = reinterpret_cast<unsigned *>(smem);                   // [2 m2]: the positives' keys, then the negatives'
    __shared__ double red[3][MT_THREADS / 64];
    const int tid = threadIdx.x, n2 = 2 * m2;
    for (int i = tid; i < n2; i += MT_THREADS) {
        const int q = i & (m2 - 1);
        key[i] = q < B ? desc_key(i < m2 ? pos[q] : neg[q]) : 0xffffffffu; // padding sorts last (and is never looked at)
    }
    __syncthreads();
    for (int k = 2; k <= m2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += MT_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned a = key[i], b = key[l];
                    const bool up = ((i & (m2 - 1)) & k) == 0;            // (the last stage, k = m2: both halves ascending)
                    if ((a > b) == up) { key[i] = b; key[l] = a; }
                }
            }
            __syncthreads();
        }
    const unsigned *kp = key, *kn = key + m2;
    const double np_ = (double)B, nn_ = (double)B;
    double ap = 0.0, auc = 0.0, acc = 0.0;
    for (int i = tid; i < B; i += MT_THREADS) {
        const unsigned v = kp[i];
        if (i == B - 1 || kp[i + 1] != v) {                               // the last positive of a distinct score
            const double tps = (double)(i + 1), tb = (double)run_lower(kp, B, v), fps = (double)run_upper(kn, B, v);
            ap += (tps / np_ - tb / np_) * (tps / (tps + fps));
        }
        const unsigned u = kn[i];
        if (i == B - 1 || kn[i + 1] != u) {                               // the last negative of a distinct score
            const double fps = (double)(i + 1), fb = (double)run_lower(kn, B, u);
            const double tb = (double)run_lower(kp, B, u), tps = (double)run_upper(kp, B, u);
            auc += (fps / nn_ - fb / nn_) * (tps / np_ + tb / np_) * 0.5;
        }
        acc += pos[i] >= neg[i] ? 1.0 : 0.0;
    }
    for (int d = 32; d > 0; d >>= 1) { ap += __shfl_down(ap, d); auc += __shfl_down(auc, d); acc += __shfl_down(acc, d); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = ap; red[1][tid >> 6] = auc; red[2][tid >> 6] = acc; }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, u = 0.0, c = 0.0;
        for (int q = 0; q < MT_THREADS / 64; ++q) { a += red[0][q]; u += red[1][q]; c += red[2][q]; }
        c /= (double)B;
        if (accumulate) { out[0] += a; out[1] += u; out[2] += c; }
        else { out[0] = a; out[1] = u; out[2] = c; }
        if (row != nullptr) { row[0] = a; row[1] = u; row[2] = c; }
    }
}

struct AffPlan { int Hp; size_t off_part, off_cnt, total; };
void aff_plan(int64_t max_B, int H, AffPlan &p)
{
    p.Hp = round_up16(H);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    take(((size_t)2 * p.Hp * p.Hp + 2 * p.Hp) * 4);                       // packed weights first (offset 0)
    const size_t tiles = (size_t)((max_B + 15) / 16);
    p.off_cnt = take(tiles * 4);
    p.off_part = take((size_t)(p.Hp / 16) * 2 * tiles * 16 * 4);
    p.total = o;
}

// where the generic forms switch (tools/score_eval_time.py)
constexpr long long SPEC_TILED_MIN = 512, SPEC_ET32_MIN = 8192 + 1, GEN_TILED_MIN = 512;

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// The one place that says which kernel scores a batch, with which launch parameters (common.hpp)
AffinityPlan zt::affinity_kernel_plan(int64_t B, int H, int choice)
{
    AffinityPlan ap{AffForm::refused, 0, 0, 0u, 0u, 0u, 0};
    if (!score_width_ok(H) || B < 0) return ap;
    const int Hp = round_up16(H);
    const bool spec = Hp == 208 || Hp == 304;                             // H = D (n_tppr + 1), D = 100, n_tppr in {1, 2}
    // the library's pick: the specialised kernels where they exist.  Small batches: the latency-organised form; large ones: the
    // tiled one (all give the same probabilities to rounding; where the switches sit: tools/score_eval_time.py)
    AffForm form = spec ? (B >= SPEC_TILED_MIN ? AffForm::tiled : AffForm::latency)
                        : (B >= GEN_TILED_MIN ? AffForm::gen_tiled : AffForm::gen_latency);
    // a pinned form that cannot take the width falls back to the pick above
    if (choice == ZT_SCORE_GENERIC_LATENCY) form = AffForm::gen_latency;
    else if (choice == ZT_SCORE_GENERIC_TILED) form = AffForm::gen_tiled;
    else if (choice == ZT_SCORE_LATENCY && spec) form = AffForm::latency;
    else if (choice == ZT_SCORE_TILED && spec) form = AffForm::tiled;
    ap.form = form;
    const long long tiles = (B + 15) / 16;
    switch (form) {
    case AffForm::latency:
    case AffForm::gen_latency:
        // tiles x N-tiles waves; beyond ~3 waves per SIMD the waves stride over tiles (the specialised form: with their weights in registers)
        ap.KC = form == AffForm::latency ? Hp / 16 : 0;
        ap.gx = (unsigned)(tiles < 160 ? tiles : 160);
        ap.gy = (unsigned)(Hp / 16);
        ap.threads = 64;
        break;
    case AffForm::tiled:
        // 16 edges per workgroup while that fills the chip once (two workgroups fit a CU), 32 beyond
        ap.KC = Hp / 16;
        ap.ET = B < SPEC_ET32_MIN ? 16 : 32;
        ap.lds = ((size_t)3 * ap.ET * (Hp + 4) + 4 * 2 * ap.ET) * 4;
        ap.gx = (unsigned)((B + ap.ET - 1) / ap.ET);
        ap.gy = 1;
        ap.threads = 256;
        break;
    default:
        ap.lds = score_fwd_lds(H);
        ap.gx = (unsigned)tiles;
        ap.gy = 1;
        ap.threads = SCORE_THREADS;
        break;
    }
    return ap;
}

extern "C" int64_t zt_affinity_workspace_bytes(int64_t max_B, int32_t H)
{
    if (max_B <= 0 || H <= 0) return -1;
    if (affinity_kernel_plan(max_B, H, 0).form == AffForm::refused) return -1;
    AffPlan p;
    aff_plan(max_B, H, p);
    return (int64_t)p.total;
}

extern "C" int zt_affinity(const float *emb_dev, int64_t B, int32_t H, const zt_affinity_weights *wt, float *prob_dev,
                           void *workspace_dev, int64_t ws_max_B, int32_t weights_ready, void *stream)
{
    if (!emb_dev || !wt || !prob_dev || !workspace_dev || B < 0 || H <= 0 || ws_max_B < B) {
        set_error("zt_affinity: bad argument");
        return ZT_ERR_ARG;
    }
    const AffinityPlan kp = affinity_kernel_plan(B, H, kernel_choice(ZT_CHOICE_SCORE));
    if (kp.form == AffForm::refused) {
        set_error("zt_affinity: H=%d unsupported (H %% 4 == 0 and 4 <= H <= %d)", H, SCORE_MAX_H);
        return ZT_ERR_UNSUPPORTED;
    }
    if (B == 0) return ZT_OK;
    if (kp.form == AffForm::gen_tiled && (!aligned16(emb_dev) || !aligned16(wt->fc1_w))) {
        set_error("zt_affinity: the embeddings and fc1's weight are read as 16-byte vectors");
        return ZT_ERR_ARG;
    }
    AffPlan p;
    aff_plan(ws_max_B, H, p);
    hipStream_t s = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace_dev);
    float *packed = reinterpret_cast<float *>(ws);
    if (!weights_ready) {
        const int n = 2 * p.Hp * p.Hp + 2 * p.Hp;
        k_pack_affinity<<<(n + 255) / 256, 256, 0, s>>>(wt->fc1_w, wt->fc1_b, wt->fc2_w, H, p.Hp, packed);
        ZT_HIP(hipMemsetAsync(ws + p.off_cnt, 0, (size_t)((ws_max_B + 15) / 16) * 4, s));   // tile counters (self-resetting afterwards)
    }
    const dim3 grid(kp.gx, kp.gy);
    float *part = reinterpret_cast<float *>(ws + p.off_part);
    int *cnt = reinterpret_cast<int *>(ws + p.off_cnt);
    ZT_PROF_BEGIN(s, P_SCORE);
    int rc = ZT_OK;
    switch (kp.form) {
    case AffForm::latency:
        rc = dispatch<13, 19>(kp.KC, [&](auto kc) {
            k_affinity<kc.value><<<grid, kp.threads, 0, s>>>(emb_dev, B, H, packed, wt->fc2_b, part, cnt, prob_dev);
            return (int)ZT_OK;
        });
        break;
    case AffForm::tiled:
        rc = dispatch<13, 19>(kp.KC, [&](auto kc) {
            return dispatch<16, 32>(kp.ET, [&](auto et) {
                const void *fn = reinterpret_cast<const void *>(k_affinity_tiled<kc.value, et.value>);
                ZT_HIP(set_dynamic_lds(fn, kp.lds));
                k_affinity_tiled<kc.value, et.value><<<grid, kp.threads, kp.lds, s>>>(emb_dev, B, H, packed, wt->fc2_b, prob_dev);
                return (int)ZT_OK;
            });
        });
        break;
    case AffForm::gen_latency:
        k_affinity_gen<<<grid, kp.threads, 0, s>>>(emb_dev, B, H, packed, wt->fc2_b, part, cnt, prob_dev);
        break;
    default:
        ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_affinity_gen_tiled), kp.lds));
        k_affinity_gen_tiled<<<grid, kp.threads, kp.lds, s>>>(emb_dev, B, H, wt->fc1_w, wt->fc1_b, wt->fc2_w, wt->fc2_b, prob_dev);
        break;
    }
    ZT_PROF_END(s, P_SCORE);
    if (rc != ZT_OK) return rc;
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

// The one place that says which metrics kernel takes B pairs, with which launch parameters (common.hpp)
MetricsPlan zt::link_metrics_plan(int64_t B)
{
    static_assert(2 * METRICS_SINGLE_MAX_B == MT_MAX, "the single form's u64 keys: 128 KB of LDS");
    MetricsPlan mp{MetForm::refused, 0u, 0, 0u};
    if (B <= 0 || B > METRICS_MAX_B) return mp;
    mp.threads = MT_THREADS;
    if (B <= METRICS_SINGLE_MAX_B) {
        mp.form = MetForm::single;
        mp.n2 = MT_THREADS;                                               // >= one element per thread keeps the chunks simple
        while (mp.n2 < 2 * B) mp.n2 <<= 1;
        mp.lds = (size_t)mp.n2 * 8;
    } else {
        mp.form = MetForm::split;
        int m2 = MT_THREADS;
        while (m2 < B) m2 <<= 1;
        mp.n2 = 2 * m2;
        mp.lds = (size_t)mp.n2 * 4;
    }
    return mp;
}

extern "C" int zt_link_metrics_plan(int64_t B, int64_t *out)
{
    if (!out) { set_error("zt_link_metrics_plan: NULL out"); return ZT_ERR_ARG; }
    const MetricsPlan mp = link_metrics_plan(B);
    out[0] = (int64_t)mp.form; out[1] = mp.threads; out[2] = mp.n2; out[3] = (int64_t)mp.lds;
    return ZT_OK;
}

int zt::link_metrics_launch(const float *pos_dev, const float *neg_dev, int64_t B, double *out_dev, int accumulate, double *row_dev,
                            hipStream_t stream)
{
    if (!pos_dev || !neg_dev || !out_dev || B <= 0) { set_error("zt_link_metrics: bad argument"); return ZT_ERR_ARG; }
    const MetricsPlan mp = link_metrics_plan(B);
    if (mp.form == MetForm::refused) {
        set_error("zt_link_metrics: %lld pairs per call, at most %lld", (long long)B, (long long)METRICS_MAX_B);
        return ZT_ERR_UNSUPPORTED;
    }
    if (mp.form == MetForm::single) {
        ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_link_metrics), mp.lds));
        k_link_metrics<<<1, mp.threads, mp.lds, stream>>>(pos_dev, neg_dev, (int)B, mp.n2, out_dev, accumulate, row_dev);
    } else {
        ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_link_metrics_split), mp.lds));
        k_link_metrics_split<<<1, mp.threads, mp.lds, stream>>>(pos_dev, neg_dev, (int)B, mp.n2 / 2, out_dev, accumulate, row_dev);
    }
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_link_metrics(const float *pos_dev, const float *neg_dev, int64_t B, double *out_dev, int32_t accumulate,
                               void *stream)
{
    return link_metrics_launch(pos_dev, neg_dev, B, out_dev, accumulate, nullptr, (hipStream_t)stream);
}
