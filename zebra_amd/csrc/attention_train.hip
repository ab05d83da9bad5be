// TemporalAttentionLayer in a training step: forward with the dropout of the attention weights inside, and the backward.
//
// Forward: attention_forward_tile<true> (attention_tile.hpp) -- the eval kernel's body plus the hashed keep-mask on the
// softmax weights and the stores of p, o, y and relu(fc1) for the backward.
//
// Backward, two stages, no float atomics, every sum in one fixed order (two calls give the same bits):
//   1. k_attention_bwd, one workgroup per tile of rq query rows in the forward's LDS carve-up: the merger and out_proj
//      backwards on transposed padded weights (d_hid, d_z, d_y, d_o), V recomputed on MFMA from the staged key rows,
//      d_p~ = d_o . V, the softmax backward, q and K recomputed, d_q and the elementwise d_K = d_s q, d_V = p~ d_o.  It writes
//      the row deltas d_hid, d_y, d_q / sqrt(hd), d_K, d_V to the workspace and the merger's part of d_src.
//   2. zt_gemm_f32 / zt_colsum_f32 (train_ops.hip, the same MFMA) turn the deltas into the weight and bias sums and into
//      d_a = d_K Wk + d_V Wv and d_x = d_q Wq.  The key rows' concatenation is never built: the three input arrays and the
//      column blocks of Wk, Wv and of their gradients are addressed in place through the leading dimensions.
// Saved against recomputed: p, o, y and relu(fc1) are kept ((k heads + 2 E + hidden) floats per row); q, K and V -- 2 k E
// floats per row -- are recomputed, which costs the forward's two key projections again and keeps the saved state ~15 x
// smaller at k = 20, E = 200.  The keep-mask is recomputed from (seed, element); `inv` from the padding mask.
#include "attention_tile.hpp"

#include <algorithm>

using namespace zt;

namespace {

__global__ void k_pad_wt(const float *__restrict__ W, int rows, int cols, float *__restrict__ Wp, int rows_p, int cols_p)
{
    // Wp [rows_p][cols_p] = W^T zero-padded, W [cols][rows]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_p * cols_p) return;
    const int r = i / cols_p, c = i % cols_p;
    Wp[i] = (r < rows && c < cols) ? W[(size_t)c * rows + r] : 0.f;
}

__global__ __launch_bounds__(ATT_THREADS) void k_attention_train_fwd(
    AttnDims d, long long N, const float *__restrict__ src, const float *__restrict__ src_t,
    const float *__restrict__ nf, const float *__restrict__ ef, const float *__restrict__ ntf,
    const unsigned char *__restrict__ mask, const float *__restrict__ Wq, const float *__restrict__ Wk,
    const float *__restrict__ Wv, const float *__restrict__ in_b, const float *__restrict__ Wo,
    const float *__restrict__ out_b, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, float *__restrict__ out, float *__restrict__ attn_w,
    AttnDrop dr, AttnSaved sv)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attention_forward_tile<true>(smem, d, N, src, src_t, nf, ef, ntf, mask, Wq, Wk, Wv, in_b, Wo, out_b, W1, b1, W2, b2, out,
                                 attn_w, dr, sv);
}

struct AttnDeltas {
    float *d_hid, *d_y, *d_qs, *d_K, *d_V;     // workspace rows (AttnTrainPlan)
    float *d_src;                              // [N][D] or NULL: receives the merger's part, d_z[E:]
};

// want_attn = 0: only the merger's and out_proj's deltas are asked for; want_kv = 0: nobody reads d_K and d_V
__global__ __launch_bounds__(ATT_THREADS) void k_attention_bwd(
    AttnDims d, long long N, const float *__restrict__ src, const float *__restrict__ src_t,
    const float *__restrict__ nf, const float *__restrict__ ef, const float *__restrict__ ntf,
    const unsigned char *__restrict__ mask, const float *__restrict__ Wq, const float *__restrict__ Wk,
    const float *__restrict__ Wv, const float *__restrict__ in_b, const float *__restrict__ W2T,
    const float *__restrict__ W1T, const float *__restrict__ WoT, const float *__restrict__ p_sv,
    const float *__restrict__ hid_sv, AttnDrop dr, const float *__restrict__ d_out, AttnDeltas o, int want_attn, int want_kv)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int rows_p = d.mt * 16;
    const AttnLds l = attn_carve(smem, d);
    float *A = l.A, *KV = l.KV, *Xq = l.Xq, *Qp = l.Qp, *Z = l.Z, *sc = l.sc;
    const int *inv = l.inv;
    const long long q0 = (long long)blockIdx.x * d.rq;
    const int nq = (int)((N - q0) < d.rq ? (N - q0) : d.rq);
    const int nrow = nq * d.k;
    const int k = d.k, E = d.E;

    attn_stage(d, l, q0, nq, src, src_t, nf, ef, ntf, mask);
    // ---- merger backward: d_hid = (d_out W2) [u > 0], d_z = d_hid W1 ----
    for (int f = tid; f < 16 * d.ldq; f += ATT_THREADS) {
        const int q = f / d.ldq, c = f - q * d.ldq;
        Z[f] = (q < nq && c < d.out_dim) ? d_out[(size_t)(q0 + q) * d.out_dim + c] : 0.f;
    }
    __syncthreads();
    lds_linear(Z, d.ldq, 1, W2T, d.Op, d.hidden, d.Hp / 16, nullptr, 1.f, false, Qp, d.ldq);
    __syncthreads();
    for (int f = tid; f < nq * d.hidden; f += ATT_THREADS) {
        const int q = f / d.hidden, c = f - q * d.hidden;
        const size_t gi = (size_t)(q0 + q) * d.hidden + c;
        const float v = hid_sv[gi] > 0.f ? Qp[(size_t)q * d.ldq + c] : 0.f;
        Qp[(size_t)q * d.ldq + c] = v;
        o.d_hid[gi] = v;
    }
    __syncthreads();
    lds_linear(Qp, d.ldq, 1, W1T, d.Hp, E + d.D, d.E2p / 16, nullptr, 1.f, false, Z, d.ldq);
    __syncthreads();
    // d_y = d_z[:E], zero for rows without neighbours; d_z[E:] is the merger's part of d_src.  Z keeps d_y alone.
    for (int f = tid; f < 16 * d.ldq; f += ATT_THREADS) {
        const int q = f / d.ldq, c = f - q * d.ldq;
        if (c >= d.E2p) continue;
        float v = 0.f;
        if (q < nq) {
            if (c < E) {
                v = inv[q] ? 0.f : Z[f];
                o.d_y[(size_t)(q0 + q) * E + c] = v;
            } else if (c < E + d.D && o.d_src) {
                o.d_src[(size_t)(q0 + q) * d.D + (c - E)] = Z[f];
            }
        }
        Z[f] = v;
    }
    if (!want_attn) return;
    __syncthreads();
    // ---- d_o = d_y Wo ----
    lds_linear(Z, d.ldq, 1, WoT, d.Ep, E, d.Ep / 16, nullptr, 1.f, false, Qp, d.ldq);
    __syncthreads();                                               // Z is KV: d_y is read before V lands on it
    // ---- V again; d_p~ = d_o . V per head; d_V = p~ d_o ----
    lds_linear(A, d.lda, d.mt, Wv, d.Ekp, E, d.Ep / 16, in_b + 2 * E, 1.f, false, KV, d.ldk);
    __syncthreads();
    for (int f = tid; f < rows_p * d.heads; f += ATT_THREADS) {
        const int g = f / d.heads, h = f - g * d.heads;
        float s = 0.f;
        if (g < nrow) {
            const int q = g / k;
            const float *dr_ = Qp + (size_t)q * d.ldq + h * d.hd, *vr = KV + (size_t)g * d.ldk + h * d.hd;
            for (int c = 0; c < d.hd; ++c) s += dr_[c] * vr[c];
        }
        sc[f] = s;
    }
    if (want_kv) {
        for (int f = tid; f < nrow * E; f += ATT_THREADS) {
            const int g = f / E, c = f - g * E;
            const int q = g / k, j = g - q * k, h = c / d.hd;
            const float pt = p_sv[((size_t)q0 * k + g) * d.heads + h] * attn_keep(dr, d, q0 + q, h, j);
            o.d_V[((size_t)q0 * k + g) * E + c] = pt * Qp[(size_t)q * d.ldq + c];
        }
    }
    __syncthreads();
    // ---- d_p = d_p~ m;  d_s = p (d_p - sum_i p_i d_p_i), in slot order ----
    for (int f = tid; f < nq * d.heads; f += ATT_THREADS) {
        const int q = f / d.heads, h = f - q * d.heads;
        const float *pr = p_sv + ((size_t)(q0 + q) * k) * d.heads + h;
        float dot = 0.f;
        for (int j = 0; j < k; ++j) {
            const float dp = sc[(q * k + j) * d.heads + h] * attn_keep(dr, d, q0 + q, h, j);
            sc[(q * k + j) * d.heads + h] = dp;
            dot += pr[(size_t)j * d.heads] * dp;
        }
        for (int j = 0; j < k; ++j) sc[(q * k + j) * d.heads + h] = pr[(size_t)j * d.heads] * (sc[(q * k + j) * d.heads + h] - dot);
    }
    // ---- q and K again (d_o in Qp and V in KV are dead: every read of them lies before the barrier above) ----
    lds_linear(Xq, d.ldq, 1, Wq, d.Ep, E, d.Ep / 16, in_b, rsqrtf((float)d.hd), false, Qp, d.ldq);
    lds_linear(A, d.lda, d.mt, Wk, d.Ekp, E, d.Ep / 16, in_b + E, 1.f, false, KV, d.ldk);
    __syncthreads();
    // ---- d_K = d_s q;  d_q = sum_j d_s_j K_j, stored with the forward's 1 / sqrt(hd) on it ----
    if (want_kv) {
        for (int f = tid; f < nrow * E; f += ATT_THREADS) {
            const int g = f / E, c = f - g * E;
            const int q = g / k, h = c / d.hd;
            o.d_K[((size_t)q0 * k + g) * E + c] = sc[g * d.heads + h] * Qp[(size_t)q * d.ldq + c];
        }
    }
    const float rs = rsqrtf((float)d.hd);
    for (int f = tid; f < nq * E; f += ATT_THREADS) {
        const int q = f / E, c = f - q * E, h = c / d.hd;
        float v = 0.f;
        for (int j = 0; j < k; ++j) v += sc[(q * k + j) * d.heads + h] * KV[(size_t)(q * k + j) * d.ldk + c];
        o.d_qs[(size_t)(q0 + q) * E + c] = v * rs;
    }
}

AttnDrop make_drop(float p, unsigned long long seed)
{
    AttnDrop dr;
    dr.lo = (unsigned)seed; dr.hi = (unsigned)(seed >> 32);
    dr.thr = drop_threshold(p);
    dr.inv_keep = dr.thr ? (float)(1.0 / (1.0 - (double)p)) : 1.f;
    return dr;
}

struct PaddedWeights {
    float *Wq, *Wk, *Wv, *Wo, *W1, *W2, *W2T, *W1T, *WoT;
};

PaddedWeights carve_weights(void *workspace, const AttnTrainPlan &p)
{
    char *b = reinterpret_cast<char *>(workspace);
    auto at = [&](size_t o) { return reinterpret_cast<float *>(b + o); };
    return PaddedWeights{at(p.off[0]), at(p.off[1]), at(p.off[2]), at(p.off[3]), at(p.off[4]), at(p.off[5]),
                         at(p.off_t[0]), at(p.off_t[1]), at(p.off_t[2])};
}

int pad(const float *W, int rows, int cols, float *Wp, int rp, int cp, hipStream_t s)
{
    k_pad_w<<<(rp * cp + 255) / 256, 256, 0, s>>>(W, rows, cols, cols, 0, Wp, rp, cp);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

// Wp [rp][cp] = W^T, W [cols][rows]
int pad_t(const float *W, int rows, int cols, float *Wp, int rp, int cp, hipStream_t s)
{
    k_pad_wt<<<(rp * cp + 255) / 256, 256, 0, s>>>(W, rows, cols, Wp, rp, cp);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

// the checks both entry points share; ZT_OK with *launch = false for N == 0
int check_call(const char *who, const void *const *required, int n_required, const zt_attn_weights *w, int64_t N, int32_t k,
               int32_t D, int32_t F, int32_t T, int32_t n_head, int32_t hidden, int32_t out_dim, float drop_p, AttnDims &d,
               AttnTrainPlan &p, bool &launch)
{
    launch = false;
    if (!w || N < 0 || k <= 0 || D <= 0 || F < 0 || T <= 0 || !(drop_p >= 0.f && drop_p < 1.f)) {
        set_error("%s: bad argument", who);
        return ZT_ERR_ARG;
    }
    if (N == 0) return ZT_OK;
    for (int i = 0; i < n_required; ++i)
        if (!required[i]) { set_error("%s: NULL buffer", who); return ZT_ERR_ARG; }
    if (!w->q_w || !w->k_w || !w->v_w || !w->in_b || !w->out_w || !w->out_b || !w->m1_w || !w->m1_b || !w->m2_w || !w->m2_b) {
        set_error("%s: NULL weight", who);
        return ZT_ERR_ARG;
    }
    if (!attention_train_plan(D, F, T, n_head, hidden, out_dim, k, d, p)) {
        set_error("%s: unsupported shape (heads<=4, E %% heads == 0, k <= 80 rows must fit the LDS tile)", who);
        return ZT_ERR_UNSUPPORTED;
    }
    launch = true;
    return ZT_OK;
}

}  // namespace

bool zt::attention_train_plan(int D, int F, int T, int heads, int hidden, int out_dim, int k, AttnDims &d, AttnTrainPlan &p)
{
    size_t lds = 0, ws = 0;
    if (!attention_plan(D, F, T, heads, hidden, out_dim, k, d, lds, p.off, ws)) return false;
    // the backward carves the same LDS: key rows, one projection at a time (V, then K), three 16-row blocks, the score column
    p.lds_fwd = lds;
    p.lds_bwd = lds;
    if (p.lds_bwd > ATT_LDS_BOUND) return false;
    p.fwd_ws = ws;
    size_t o = ws;
    auto take = [&](size_t b) { size_t r = o; o += (b + 255) & ~(size_t)255; return r; };
    p.off_t[0] = take((size_t)d.Hp * d.Op * 4);     // merger.fc2 transposed
    p.off_t[1] = take((size_t)d.E2p * d.Hp * 4);    // merger.fc1 transposed
    p.off_t[2] = take((size_t)d.Ep * d.Ep * 4);     // out_proj transposed
    p.fixed = o;
    p.ws_row = (size_t)4 * ((size_t)hidden + 2 * (size_t)d.E + 2 * (size_t)k * d.E);
    p.saved_row = (size_t)4 * ((size_t)k * heads + 2 * (size_t)d.E + (size_t)hidden);
    return true;
}

extern "C" int zt_attention_train_plan(int32_t D, int32_t F, int32_t T, int32_t n_head, int32_t hidden, int32_t out_dim,
                                       int32_t k, int64_t *out)
{
    if (!out) { set_error("zt_attention_train_plan: NULL out"); return ZT_ERR_ARG; }
    AttnDims d;
    AttnTrainPlan p;
    const bool ok = attention_train_plan(D, F, T, n_head, hidden, out_dim, k, d, p);
    const int64_t v[8] = {ok ? 1 : 0, ok ? d.rq : 0, ok ? d.mt : 0, ok ? (int64_t)p.lds_fwd : 0, ok ? (int64_t)p.lds_bwd : 0,
                          ok ? (int64_t)p.ws_row : 0, ok ? (int64_t)p.fixed : 0, ok ? (int64_t)p.saved_row : 0};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return ZT_OK;
}

extern "C" int64_t zt_attention_train_workspace_bytes(int64_t N, int32_t D, int32_t F, int32_t T, int32_t n_head,
                                                      int32_t hidden, int32_t out_dim, int32_t k)
{
    AttnDims d;
    AttnTrainPlan p;
    if (N < 0 || !attention_train_plan(D, F, T, n_head, hidden, out_dim, k, d, p)) return -1;
    return (int64_t)(p.fixed + (size_t)N * p.ws_row);
}

extern "C" int64_t zt_attention_train_saved_bytes(int64_t N, int32_t D, int32_t F, int32_t T, int32_t n_head, int32_t hidden,
                                                  int32_t out_dim, int32_t k)
{
    AttnDims d;
    AttnTrainPlan p;
    if (N < 0 || !attention_train_plan(D, F, T, n_head, hidden, out_dim, k, d, p)) return -1;
    return (int64_t)((size_t)N * p.saved_row);
}

namespace {

AttnSaved carve_saved(float *saved, const AttnDims &d, int64_t N)
{
    AttnSaved sv;
    sv.p = saved;
    sv.o = sv.p + (size_t)N * d.k * d.heads;
    sv.y = sv.o + (size_t)N * d.E;
    sv.hid = sv.y + (size_t)N * d.E;
    return sv;
}

}  // namespace

extern "C" int zt_attention_train_forward(const float *src_dev, const float *src_time_dev, const float *nbr_feat_dev,
                                          const float *edge_feat_dev, const float *nbr_time_dev, const uint8_t *mask_dev,
                                          int64_t N, int32_t k, int32_t D, int32_t F, int32_t T, int32_t n_head,
                                          int32_t hidden, int32_t out_dim, const zt_attn_weights *w, float drop_p,
                                          uint64_t drop_seed, float *out_dev, float *attn_w_dev, float *saved_dev,
                                          void *workspace_dev, void *stream)
{
    const void *req[] = {src_dev, src_time_dev, nbr_feat_dev, (F > 0 ? (const void *)edge_feat_dev : (const void *)src_dev),
                         nbr_time_dev, mask_dev, out_dev, attn_w_dev, saved_dev, workspace_dev};
    AttnDims d;
    AttnTrainPlan p;
    bool launch;
    const int rc = check_call("zt_attention_train_forward", req, 10, w, N, k, D, F, T, n_head, hidden, out_dim, drop_p, d, p, launch);
    if (rc != ZT_OK || !launch) return rc;
    hipStream_t s = (hipStream_t)stream;
    const PaddedWeights pw = carve_weights(workspace_dev, p);
    int e;
    if ((e = pad(w->q_w, d.E, d.E, pw.Wq, d.Ep, d.Ep, s)) != ZT_OK) return e;
    if ((e = pad(w->k_w, d.E, d.Ek, pw.Wk, d.Ep, d.Ekp, s)) != ZT_OK) return e;
    if ((e = pad(w->v_w, d.E, d.Ek, pw.Wv, d.Ep, d.Ekp, s)) != ZT_OK) return e;
    if ((e = pad(w->out_w, d.E, d.E, pw.Wo, d.Ep, d.Ep, s)) != ZT_OK) return e;
    if ((e = pad(w->m1_w, hidden, d.E + D, pw.W1, d.Hp, d.E2p, s)) != ZT_OK) return e;
    if ((e = pad(w->m2_w, out_dim, hidden, pw.W2, d.Op, d.Hp, s)) != ZT_OK) return e;
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_attention_train_fwd), p.lds_fwd));
    const unsigned grid = (unsigned)((N + d.rq - 1) / d.rq);
    k_attention_train_fwd<<<grid, ATT_THREADS, p.lds_fwd, s>>>(d, N, src_dev, src_time_dev, nbr_feat_dev, edge_feat_dev,
                                                               nbr_time_dev, mask_dev, pw.Wq, pw.Wk, pw.Wv, w->in_b, pw.Wo,
                                                               w->out_b, pw.W1, w->m1_b, pw.W2, w->m2_b, out_dev, attn_w_dev,
                                                               make_drop(drop_p, drop_seed), carve_saved(saved_dev, d, N));
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_attention_train_backward(const float *src_dev, const float *src_time_dev, const float *nbr_feat_dev,
                                           const float *edge_feat_dev, const float *nbr_time_dev, const uint8_t *mask_dev,
                                           int64_t N, int32_t k, int32_t D, int32_t F, int32_t T, int32_t n_head,
                                           int32_t hidden, int32_t out_dim, const zt_attn_weights *w, float drop_p,
                                           uint64_t drop_seed, const float *saved_dev, const float *d_out_dev,
                                           const zt_attn_grads *g, void *workspace_dev, void *stream)
{
    const void *req[] = {src_dev, src_time_dev, nbr_feat_dev, (F > 0 ? (const void *)edge_feat_dev : (const void *)src_dev),
                         nbr_time_dev, mask_dev, saved_dev, d_out_dev, g, workspace_dev};
    AttnDims d;
    AttnTrainPlan p;
    bool launch;
    const int rc = check_call("zt_attention_train_backward", req, 10, w, N, k, D, F, T, n_head, hidden, out_dim, drop_p, d, p, launch);
    if (rc != ZT_OK || !launch) return rc;
    const bool want_kv = g->d_nbr_feat || (F > 0 && g->d_edge_feat) || g->d_nbr_time || g->d_k_w || g->d_v_w || g->d_in_b;
    const bool want_attn = want_kv || g->d_src || g->d_src_time || g->d_q_w;
    const bool want_merger = g->d_out_w || g->d_out_b || g->d_m1_w || g->d_m1_b || g->d_m2_w || g->d_m2_b;
    if (!want_attn && !want_merger) return ZT_OK;
    hipStream_t s = (hipStream_t)stream;
    const PaddedWeights pw = carve_weights(workspace_dev, p);
    const int E = d.E, Ek = d.Ek;
    const int64_t NK = N * k;
    AttnDeltas o;
    o.d_hid = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace_dev) + p.fixed);
    o.d_y = o.d_hid + (size_t)N * hidden;
    o.d_qs = o.d_y + (size_t)N * E;
    o.d_K = o.d_qs + (size_t)N * E;
    o.d_V = o.d_K + (size_t)NK * E;
    o.d_src = g->d_src;
    const AttnSaved sv = carve_saved(const_cast<float *>(saved_dev), d, N);
    int e;
    if (want_attn) {
        if ((e = pad(w->q_w, E, E, pw.Wq, d.Ep, d.Ep, s)) != ZT_OK) return e;
        if ((e = pad(w->k_w, E, Ek, pw.Wk, d.Ep, d.Ekp, s)) != ZT_OK) return e;
        if ((e = pad(w->v_w, E, Ek, pw.Wv, d.Ep, d.Ekp, s)) != ZT_OK) return e;
        if ((e = pad_t(w->out_w, E, E, pw.WoT, d.Ep, d.Ep, s)) != ZT_OK) return e;
    }
    if ((e = pad_t(w->m2_w, hidden, out_dim, pw.W2T, d.Hp, d.Op, s)) != ZT_OK) return e;      // [hidden][out] = m2_w^T
    if ((e = pad_t(w->m1_w, E + D, hidden, pw.W1T, d.E2p, d.Hp, s)) != ZT_OK) return e;       // [E + D][hidden] = m1_w^T
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_attention_bwd), p.lds_bwd));
    const unsigned grid = (unsigned)((N + d.rq - 1) / d.rq);
    k_attention_bwd<<<grid, ATT_THREADS, p.lds_bwd, s>>>(d, N, src_dev, src_time_dev, nbr_feat_dev, edge_feat_dev, nbr_time_dev,
                                                         mask_dev, pw.Wq, pw.Wk, pw.Wv, w->in_b, pw.W2T, pw.W1T, pw.WoT, sv.p,
                                                         sv.hid, make_drop(drop_p, drop_seed), d_out_dev, o, want_attn ? 1 : 0,
                                                         want_kv ? 1 : 0);
    ZT_LAUNCH_CHECK();
    // ---- weight and bias sums over the rows: C = delta^T input (column blocks through ldb / ldc) ----
    auto gemm = [&](const float *A, const float *B, float *C, int64_t M, int64_t Nn, int64_t K, int64_t lda, int64_t ldb,
                    int64_t ldc, int ta, int acc) {
        if (M <= 0 || Nn <= 0) return (int)ZT_OK;
        return zt_gemm_f32(A, B, C, M, Nn, K, lda, ldb, ldc, ta, 0, acc, stream);
    };
    if (g->d_m2_w && (e = gemm(d_out_dev, sv.hid, g->d_m2_w, out_dim, hidden, N, out_dim, hidden, hidden, 1, 0)) != ZT_OK) return e;
    if (g->d_m2_b && (e = zt_colsum_f32(d_out_dev, N, out_dim, out_dim, g->d_m2_b, 0, stream)) != ZT_OK) return e;
    if (g->d_m1_w) {
        if ((e = gemm(o.d_hid, sv.y, g->d_m1_w, hidden, E, N, hidden, E, E + D, 1, 0)) != ZT_OK) return e;
        if ((e = gemm(o.d_hid, src_dev, g->d_m1_w + E, hidden, D, N, hidden, D, E + D, 1, 0)) != ZT_OK) return e;
    }
    if (g->d_m1_b && (e = zt_colsum_f32(o.d_hid, N, hidden, hidden, g->d_m1_b, 0, stream)) != ZT_OK) return e;
    if (g->d_out_w && (e = gemm(o.d_y, sv.o, g->d_out_w, E, E, N, E, E, E, 1, 0)) != ZT_OK) return e;
    if (g->d_out_b && (e = zt_colsum_f32(o.d_y, N, E, E, g->d_out_b, 0, stream)) != ZT_OK) return e;
    if (g->d_q_w) {
        if ((e = gemm(o.d_qs, src_dev, g->d_q_w, E, D, N, E, D, E, 1, 0)) != ZT_OK) return e;
        if ((e = gemm(o.d_qs, src_time_dev, g->d_q_w + D, E, T, N, E, T, E, 1, 0)) != ZT_OK) return e;
    }
    if (g->d_in_b) {
        if ((e = zt_colsum_f32(o.d_qs, N, E, E, g->d_in_b, 0, stream)) != ZT_OK) return e;
        if ((e = zt_colsum_f32(o.d_K, NK, E, E, g->d_in_b + E, 0, stream)) != ZT_OK) return e;
        if ((e = zt_colsum_f32(o.d_V, NK, E, E, g->d_in_b + 2 * E, 0, stream)) != ZT_OK) return e;
    }
    const float *dkv[2] = {o.d_K, o.d_V};
    float *dw[2] = {g->d_k_w, g->d_v_w};
    for (int i = 0; i < 2; ++i) {
        if (!dw[i]) continue;
        if ((e = gemm(dkv[i], nbr_feat_dev, dw[i], E, D, NK, E, D, Ek, 1, 0)) != ZT_OK) return e;
        if ((e = gemm(dkv[i], edge_feat_dev, dw[i] + D, E, F, NK, E, F, Ek, 1, 0)) != ZT_OK) return e;
        if ((e = gemm(dkv[i], nbr_time_dev, dw[i] + D + F, E, T, NK, E, T, Ek, 1, 0)) != ZT_OK) return e;
    }
    // ---- input gradients: d_x = (d_q / sqrt(hd)) Wq on top of the merger's d_src; d_a = d_K Wk + d_V Wv ----
    if (g->d_src && (e = gemm(o.d_qs, w->q_w, g->d_src, N, D, E, E, E, D, 0, 1)) != ZT_OK) return e;
    if (g->d_src_time && (e = gemm(o.d_qs, w->q_w + D, g->d_src_time, N, T, E, E, E, T, 0, 0)) != ZT_OK) return e;
    float *da[3] = {g->d_nbr_feat, F > 0 ? g->d_edge_feat : nullptr, g->d_nbr_time};
    const int col0[3] = {0, D, D + F}, wid[3] = {D, F, T};
    for (int i = 0; i < 3; ++i) {
        if (!da[i]) continue;
        if ((e = gemm(o.d_K, w->k_w + col0[i], da[i], NK, wid[i], E, E, Ek, wid[i], 0, 0)) != ZT_OK) return e;
        if ((e = gemm(o.d_V, w->v_w + col0[i], da[i], NK, wid[i], E, E, Ek, wid[i], 0, 1)) != ZT_OK) return e;
    }
    return ZT_OK;
}
