// The link scorer of a TRAINING step on the device, forward and backward:
// TGN.compute_edge_probabilities' tail (reference model/tgn_model.py:185-188 with MergeLayer, utils/util.py:14-26)
//   prob = sigmoid(fc2(relu(fc1(cat[x1, x2])))),  x1 = [src | src], x2 = [dst | neg]
// for the B positive and B negative pairs of a batch whose embeddings [3B][H] = [src | dst | neg] the aggregation produced,
// and what autograd derives from it.  scoring.hip's idea carries over: fc1 acts on a concatenation, so
// fc1([a | b]) = W_a a + W_b b + b1, the [2B][2H] concatenation is never built and W_a src is shared by an edge's two pairs.
// Unlike scoring.hip the kernels here read the UNPACKED parameters (they change every optimizer step: a pack pass per step
// would be a launch for nothing) -- W_a is columns [0, H) of a row of fc1.weight, W_b columns [H, 2H), 16-byte aligned
// because H % 4 == 0 -- and K runs over H at run time: one instantiation for every width 4 <= H <= 768.
//
// Forward (one launch, k_score_fwd): a workgroup of sixteen waves owns 16 edges.  Their 48 embedding rows are staged in LDS
// once (148 KB at H = 768); wave w takes the N-tiles w, w + 16, ... of the hidden layer with three accumulators (W_a src,
// W_b dst, W_b neg) on v_mfma_f32_16x16x4_f32, streams its 16 weight rows from L2 as 16-byte vectors, applies bias and ReLU
// in the accumulator lanes, writes the hidden rows (kept for the backward) and carries relu(.) x fc2.weight per lane.  The
// waves' partial scores meet in LDS and are added in wave order: the probabilities do not depend on timing.
//
// Backward (three launches, nothing on the host in between, no atomics on any output):
//   k_score_bwd_dx   per 16 edges: ds = dprob p (1 - p), dh = ds x w2 masked by hid > 0 (written out for the weight
//                    gradients and kept in LDS), then d_emb[src] = (dh_pos + dh_neg) W_a, d_emb[dst] = dh_pos W_b,
//                    d_emb[neg] = dh_neg W_b: a wave takes 64 output columns of one product -- a 16-byte load of a weight row
//                    feeds four MFMAs -- and K runs over the hidden index.
//   k_score_bwd_dw   d_fc1_w [H][2H] = dh^T [[src; src] | [dst; neg]]: ONE product with K = 2B (the tiling of train_ops.hip's
//                    k_gemm_f32<true, false>, the right operand addressed inside the embedding block); few tiles and a long
//                    K: K is split over blockIdx.z into partial products.
//   k_score_bwd_fin  d_fc1_b = colsum(dh), d_fc2_w = sum ds hid, d_fc2_b = sum ds, and the partial products added first to
//                    last.
// Every sum has a fixed association: two runs give the same bits.
#include "common.hpp"
#include "scoring_fwd.hpp"

using namespace zt;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ST_MAX_H = SCORE_MAX_H;    // 48 staged rows x (768 + 4) floats = 148 KB of the CU's 160 KB (scoring_fwd.hpp)
constexpr int ST_WAVES = SCORE_WAVES;
constexpr int ST_THREADS = SCORE_THREADS;
constexpr int ST_MAX_SPLIT = 8;          // partial products of the weight gradient

__host__ __device__ inline int round_up16(int x) { return (x + 15) / 16 * 16; }

// U k-steps of 4 of one work item of k_score_bwd_dx
template <int U>
__device__ __forceinline__ void dx_steps(int k0, bool cok, int g4, int H, const float *__restrict__ wp, const float *arow, f32x4 (&acc)[4])
{
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int k = k0 + 4 * u + g4;                                   // (the load: unconditional, from a clamped row)
        const f32x4 v = *reinterpret_cast<const f32x4 *>(wp + (size_t)(k < H ? k : H - 1) * 2 * H);
        w[u] = cok && k < H ? v : zero4;
    }
    __builtin_amdgcn_sched_barrier(0);                                   // (as in fwd_chunks)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float a = arow[k0 + 4 * u];                                // (zero beyond H: the rows are padded)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w[u][i], acc[i], 0, 0, 0);
    }
}

// (the body: scoring_fwd.hpp, shared with the eval scorer's generic tiled form; here the hidden rows are kept)
__global__ __launch_bounds__(ST_THREADS) void k_score_fwd(const float *__restrict__ emb, long long B, int H,
                                                          const float *__restrict__ fc1_w, const float *__restrict__ fc1_b,
                                                          const float *__restrict__ fc2_w, const float *__restrict__ fc2_b,
                                                          float *__restrict__ prob, float *__restrict__ hid)
{
    score_fwd_body<true>(emb, B, H, fc1_w, fc1_b, fc2_w, fc2_b, prob, hid);
}

// d_emb may be NULL (the embeddings need no gradient): dh and ds are still written for the other two kernels
__global__ __launch_bounds__(ST_THREADS) void k_score_bwd_dx(long long B, int H, const float *__restrict__ fc1_w,
                                                             const float *__restrict__ fc2_w, const float *__restrict__ prob,
                                                             const float *__restrict__ hid, const float *__restrict__ dprob,
                                                             float *__restrict__ dh, float *__restrict__ ds, float *__restrict__ d_emb)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Hp = round_up16(H), ld = Hp + 4, h4 = H / 4, hp4 = Hp / 4;
    float *D = reinterpret_cast<float *>(smem);                          // [48][ld]: dh_pos + dh_neg, dh_pos, dh_neg of the tile
    float *dsv = D + 48 * ld;                                            // [2][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const long long e0 = (long long)blockIdx.x * 16;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (tid < 32) {
        const long long e = e0 + (tid & 15), r = (long long)(tid >> 4) * B + e;
        float v = 0.f;
        if (e < B) {
            const float p = prob[r];
            v = dprob[r] * p * (1.f - p);
            ds[r] = v;
        }
        dsv[tid] = v;
    }
    __syncthreads();
    for (int f = tid; f < 16 * hp4; f += ST_THREADS) {
        const int row = f / hp4, c4 = f - row * hp4;
        const long long e = e0 + row;
        const bool ok = c4 < h4 && e < B;
        f32x4 dp = zero4, dn = zero4;
        if (ok) {
            const f32x4 hp = *reinterpret_cast<const f32x4 *>(hid + (size_t)e * H + 4 * c4);
            const f32x4 hn = *reinterpret_cast<const f32x4 *>(hid + (size_t)(B + e) * H + 4 * c4);
            const f32x4 w2 = *reinterpret_cast<const f32x4 *>(fc2_w + 4 * c4);
            const float sp = dsv[row], sn = dsv[16 + row];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dp[i] = hp[i] > 0.f ? sp * w2[i] : 0.f;
                dn[i] = hn[i] > 0.f ? sn * w2[i] : 0.f;
            }
            *reinterpret_cast<f32x4 *>(dh + (size_t)e * H + 4 * c4) = dp;
            *reinterpret_cast<f32x4 *>(dh + (size_t)(B + e) * H + 4 * c4) = dn;
        }
        *reinterpret_cast<f32x4 *>(D + row * ld + 4 * c4) = dp + dn;
        *reinterpret_cast<f32x4 *>(D + (16 + row) * ld + 4 * c4) = dp;
        *reinterpret_cast<f32x4 *>(D + (32 + row) * ld + 4 * c4) = dn;
    }
    if (d_emb == nullptr) return;
    __syncthreads();
    // work item (q, prod): columns [64 q, 64 q + 64) of product prod (0: (dh_pos + dh_neg) W_a -> src rows, 1: dh_pos W_b -> dst
    // rows, 2: dh_neg W_b -> neg rows).  Lane r16 holds columns 64 q + 4 r16 + i of MFMA tile i: one 16-byte load of weight row k
    // feeds the four tiles, and a lane's four results of an edge are one 16-byte store.
    const int items = 3 * ((H + 63) / 64);
    for (int it = wave; it < items; it += ST_WAVES) {
        const int q = it / 3, prod = it - 3 * q;
        const int c0 = 64 * q + 4 * r16;
        const bool cok = c0 < H;                                         // H % 4 == 0: all four columns or none
        const float *arow = D + (prod * 16 + r16) * ld + g4;
        const float *wp = fc1_w + (prod == 0 ? 0 : H) + (cok ? c0 : 0);
        f32x4 acc[4] = {zero4, zero4, zero4, zero4};
        for (int k0 = 0; k0 < Hp; k0 += 16) dx_steps<4>(k0, cok, g4, H, wp, arow, acc);       // (Hp % 16 == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long e = e0 + 4 * g4 + j;
            if (cok && e < B) {
                const f32x4 o = {acc[0][j], acc[1][j], acc[2][j], acc[3][j]};
                *reinterpret_cast<f32x4 *>(d_emb + ((size_t)prod * B + e) * H + c0) = o;
            }
        }
    }
}

// C [H][2H] (+ z H 2H: partial product z) = dh^T X over k in [z kper, (z + 1) kper), dh [2B][H],
// X [2B][2H] = [[src; src] | [dst; neg]] read inside emb [3B][H].  train_ops.hip's k_gemm_f32<true, false> tile: 64 x 64 per
// workgroup, K in steps of 64 through LDS, every load of a step in flight before the first LDS store.
constexpr int GK = 64;
__global__ __launch_bounds__(256) void k_score_bwd_dw(const float *__restrict__ dh, const float *__restrict__ emb, long long B, int H,
                                                      long long kper, float *__restrict__ C)
{
    __shared__ float As[64][GK + 1];      // [m][k]
    __shared__ float Bs[GK][65];          // [k][n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long M = H, N = 2 * (long long)H, K = 2 * B;
    const long long m0 = (long long)blockIdx.y * 64, n0 = (long long)blockIdx.x * 64;
    const long long kbeg = (long long)blockIdx.z * kper, kend = kbeg + kper < K ? kbeg + kper : K;
    C += (size_t)blockIdx.z * M * N;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int r16 = lane & 15, g4 = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int PT = 64 * GK / 256;     // elements of each operand per thread and step
    for (long long k0 = kbeg; k0 < kend; k0 += GK) {
        float va[PT], vb[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            const int idx = tid + t * 256;
            const long long gm = m0 + (idx & 63), gn = n0 + (idx & 63), gk = k0 + (idx >> 6);
            va[t] = (gm < M && gk < kend) ? dh[gk * H + gm] : 0.f;
            // column gn < H: src row of pair gk (the positive and the negative pair of an edge share it); else dst / neg row
            const long long xr = gn < H ? (gk < B ? gk : gk - B) : B + gk;
            vb[t] = (gn < N && gk < kend) ? emb[xr * H + (gn < H ? gn : gn - H)] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            const int idx = tid + t * 256;
            As[idx & 63][idx >> 6] = va[t];
            Bs[idx >> 6][idx & 63] = vb[t];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 4) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[wm + i * 16 + r16][kk + g4];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[kk + g4][wn + j * 16 + r16];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = m0 + wm + i * 16 + g4 * 4 + r, col = n0 + wn + j * 16 + r16;
                if (row < M && col < N) C[row * N + col] = acc[i][j][r];
            }
}

// Workgroups [0, cb): 64 columns each -- d_fc1_b[c] = sum_r dh[r][c], d_fc2_w[c] = sum_r ds[r] hid[r][c] over the 2B pair rows
// (sixteen waves stride over the rows, eight loads of a wave in flight, as train_ops.hip's k_colsum); workgroup 0 also
// d_fc2_b = sum_r ds[r].  Workgroups [cb, ...): d_fc1_w = the `split` partial products of k_score_bwd_dw, added first to last.
// Any of the outputs may be NULL.
__global__ __launch_bounds__(ST_THREADS) void k_score_bwd_fin(long long B, int H, const float *__restrict__ dh, const float *__restrict__ ds,
                                                              const float *__restrict__ hid, const float *__restrict__ partial, int split,
                                                              int cb, float *__restrict__ d_fc1_w, float *__restrict__ d_fc1_b,
                                                              float *__restrict__ d_fc2_w, float *__restrict__ d_fc2_b)
{
    __shared__ float part[2][ST_WAVES][64];
    __shared__ float red[ST_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long R = 2 * B;
    if ((int)blockIdx.x >= cb) {
        const size_t n4 = (size_t)H * 2 * H / 4, i = (size_t)(blockIdx.x - cb) * ST_THREADS + tid;
        if (i < n4) {
            const f32x4 *p = reinterpret_cast<const f32x4 *>(partial) + i;
            f32x4 s = p[0];
            for (int z = 1; z < split; ++z) s += p[(size_t)z * n4];
            reinterpret_cast<f32x4 *>(d_fc1_w)[i] = s;
        }
        return;
    }
    const int c = (int)blockIdx.x * 64 + lane;
    float s1 = 0.f, s2 = 0.f;
    if (c < H && (d_fc1_b != nullptr || d_fc2_w != nullptr)) {
        // (one accumulator each, rows in ascending order per wave: wave w adds rows w, w + 16, ...)
        for (long long r0 = wave; r0 < R; r0 += (long long)ST_WAVES * 8) {
            float v[8], h[8], d[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long long r = r0 + (long long)u * ST_WAVES;
                const bool ok = r < R;
                v[u] = ok ? dh[r * H + c] : 0.f;
                h[u] = ok ? hid[r * H + c] : 0.f;
                d[u] = ok ? ds[r] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { s1 += v[u]; s2 += d[u] * h[u]; }
        }
    }
    part[0][wave][lane] = s1;
    part[1][wave][lane] = s2;
    __syncthreads();
    if (wave < 2 && c < H) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < ST_WAVES; ++w) t += part[wave][w][lane];
        float *out = wave == 0 ? d_fc1_b : d_fc2_w;
        if (out != nullptr) out[c] = t;
    }
    if (blockIdx.x == 0 && d_fc2_b != nullptr) {
        float s = 0.f;
        for (long long r = tid; r < R; r += ST_THREADS) s += ds[r];
        for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);        // a fixed tree over the lanes, the waves in order
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
            for (int w = 0; w < ST_WAVES; ++w) t += red[w];
            d_fc2_b[0] = t;
        }
    }
}

bool st_width_ok(int H) { return H >= 4 && H <= ST_MAX_H && H % 4 == 0; }

// partial products of the weight gradient: the 64 x 64 tiles of [H][2H] alone leave most of the chip idle below H ~ 700
int st_max_split(int H)
{
    const int tiles = ((H + 63) / 64) * ((2 * H + 63) / 64);
    const int s = 256 / tiles;
    return s < 1 ? 1 : (s > ST_MAX_SPLIT ? ST_MAX_SPLIT : s);
}

struct ScoreTrainPlan { size_t off_dh, off_ds, off_part, total; };
void st_plan(int64_t max_B, int H, ScoreTrainPlan &p)
{
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t b = (size_t)(max_B > 0 ? max_B : 1);
    p.off_dh = take(2 * b * H * 4);
    p.off_ds = take(2 * b * 4);
    const int ms = st_max_split(H);
    p.off_part = take(ms > 1 ? (size_t)ms * H * 2 * H * 4 : 0);
    p.total = o;
}

// The one place that decides the backward's launches (host code only; zt_affinity_train_plan reports it and
// zt_affinity_train_backward launches from it).  d_fc1_w: K = 2B in partial products of whole 64-row steps, at least two steps
// each; the split is recomputed from the rounded part so that no part is empty (nine steps asked in four parts: three of 192
// rows).  Without d_fc1_w no product is launched and split = 1.
struct ScoreBwdPlan {
    int split, max_split;
    long long kper, steps;
    unsigned grid_dx, grid_dw[3], grid_fin;
    size_t lds_dx;
};
ScoreBwdPlan st_bwd_plan(int64_t B, int H, bool want_dw, bool want_sums)
{
    ScoreBwdPlan p = {};
    p.max_split = st_max_split(H);
    p.steps = (2 * B + GK - 1) / GK;
    const long long want = p.steps / 2 < 1 ? 1 : p.steps / 2;
    int split = (int)(want < p.max_split ? want : p.max_split);
    p.kper = (p.steps + split - 1) / split * GK;
    split = B > 0 ? (int)((2 * B + p.kper - 1) / p.kper) : 1;
    p.split = want_dw ? split : 1;
    p.grid_dx = (unsigned)((B + 15) / 16);
    p.lds_dx = ((size_t)48 * (round_up16(H) + 4) + 32) * 4;
    if (want_dw) {
        p.grid_dw[0] = (unsigned)((2 * H + 63) / 64);
        p.grid_dw[1] = (unsigned)((H + 63) / 64);
        p.grid_dw[2] = (unsigned)p.split;
    }
    if (p.split > 1 || want_sums) {
        const size_t n4 = (size_t)H * 2 * H / 4;
        p.grid_fin = (unsigned)((H + 63) / 64) + (p.split > 1 ? (unsigned)((n4 + ST_THREADS - 1) / ST_THREADS) : 0u);
    }
    return p;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int st_check_width(const char *who, int H)
{
    if (st_width_ok(H)) return ZT_OK;
    set_error("%s: H=%d unsupported (H %% 4 == 0 and 4 <= H <= %d)", who, H, ST_MAX_H);
    return ZT_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" int64_t zt_affinity_train_workspace_bytes(int64_t max_B, int32_t H)
{
    if (max_B < 0 || !st_width_ok(H)) return -1;
    ScoreTrainPlan p;
    st_plan(max_B, H, p);
    return (int64_t)p.total;
}

extern "C" int zt_affinity_train_plan(int64_t B, int32_t H, int64_t *out)
{
    if (!out || B < 0) {
        set_error("zt_affinity_train_plan: bad argument");
        return ZT_ERR_ARG;
    }
    const int rc = st_check_width("zt_affinity_train_plan", H);
    if (rc != ZT_OK) return rc;
    const ScoreBwdPlan p = st_bwd_plan(B, H, true, true);
    out[0] = p.split; out[1] = p.kper; out[2] = p.max_split; out[3] = p.steps; out[4] = p.grid_dx;
    out[5] = p.grid_dw[0]; out[6] = p.grid_dw[1]; out[7] = p.grid_dw[2]; out[8] = p.grid_fin; out[9] = (int64_t)p.lds_dx;
    return ZT_OK;
}

extern "C" int zt_affinity_train_forward(const float *emb_dev, int64_t B, int32_t H, const zt_affinity_weights *wt, float *prob_dev,
                                         float *hid_dev, void *stream)
{
    if (B < 0 || H < 0 || !wt || !wt->fc1_w || !wt->fc1_b || !wt->fc2_w || !wt->fc2_b || (B > 0 && (!emb_dev || !prob_dev || !hid_dev)) ||
        !aligned16(emb_dev) || !aligned16(wt->fc1_w)) {
        set_error("zt_affinity_train_forward: bad argument");
        return ZT_ERR_ARG;
    }
    const int rc = st_check_width("zt_affinity_train_forward", H);
    if (rc != ZT_OK) return rc;
    if (B == 0) return ZT_OK;
    const size_t lds = score_fwd_lds(H);
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_score_fwd), lds));
    k_score_fwd<<<(unsigned)((B + 15) / 16), ST_THREADS, lds, (hipStream_t)stream>>>(emb_dev, B, H, wt->fc1_w, wt->fc1_b, wt->fc2_w,
                                                                                     wt->fc2_b, prob_dev, hid_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_affinity_train_backward(const float *emb_dev, int64_t B, int32_t H, const zt_affinity_weights *wt,
                                          const float *prob_dev, const float *hid_dev, const float *dprob_dev, float *d_emb_dev,
                                          float *d_fc1_w_dev, float *d_fc1_b_dev, float *d_fc2_w_dev, float *d_fc2_b_dev,
                                          void *workspace_dev, int64_t ws_max_B, void *stream)
{
    if (B < 0 || H < 0 || ws_max_B < B || !wt || !wt->fc1_w || !wt->fc2_w ||
        (B > 0 && (!emb_dev || !prob_dev || !hid_dev || !dprob_dev || !workspace_dev)) || !aligned16(emb_dev) || !aligned16(wt->fc1_w) ||
        !aligned16(wt->fc2_w) || !aligned16(hid_dev) || !aligned16(d_emb_dev) || !aligned16(d_fc1_w_dev) || !aligned16(workspace_dev)) {
        set_error("zt_affinity_train_backward: bad argument");
        return ZT_ERR_ARG;
    }
    const int rc = st_check_width("zt_affinity_train_backward", H);
    if (rc != ZT_OK) return rc;
    if (B == 0) return ZT_OK;
    hipStream_t s = (hipStream_t)stream;
    ScoreTrainPlan p;
    st_plan(ws_max_B, H, p);
    char *ws = reinterpret_cast<char *>(workspace_dev);
    float *dh = reinterpret_cast<float *>(ws + p.off_dh), *ds = reinterpret_cast<float *>(ws + p.off_ds);
    float *partial = reinterpret_cast<float *>(ws + p.off_part);
    const ScoreBwdPlan pl = st_bwd_plan(B, H, d_fc1_w_dev != nullptr,
                                        d_fc1_b_dev != nullptr || d_fc2_w_dev != nullptr || d_fc2_b_dev != nullptr);
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_score_bwd_dx), pl.lds_dx));
    k_score_bwd_dx<<<pl.grid_dx, ST_THREADS, pl.lds_dx, s>>>(B, H, wt->fc1_w, wt->fc2_w, prob_dev, hid_dev, dprob_dev, dh, ds, d_emb_dev);
    const int split = pl.split;
    if (d_fc1_w_dev != nullptr) {
        const dim3 grid(pl.grid_dw[0], pl.grid_dw[1], pl.grid_dw[2]);
        k_score_bwd_dw<<<grid, 256, 0, s>>>(dh, emb_dev, B, H, pl.kper, split > 1 ? partial : d_fc1_w_dev);
    }
    if (pl.grid_fin > 0) {
        const int cb = (H + 63) / 64;
        k_score_bwd_fin<<<pl.grid_fin, ST_THREADS, 0, s>>>(B, H, dh, ds, hid_dev, partial, split, cb, d_fc1_w_dev, d_fc1_b_dev,
                                                          d_fc2_w_dev, d_fc2_b_dev);
    }
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
