// TemporalAttentionLayer forward (reference model/temporal_attention.py:7-68).
//
// NOT on the reference's live path: the layer is only instantiated by
// GraphAttentionEmbedding, which train.py can never reach, so
// there are no reference call sites or outputs; parity is against a torch
// restatement (nn.MultiheadAttention + MergeLayer, zebra_amd/modules.py).
// Built because BASELINE.json's north_star names it.
//
//   q = [src | src_time]  (1 token, E = D+T);  k = v = [nbr | edge | nbr_time]  (n_nbr tokens, Ek = D+F+T)
//   nn.MultiheadAttention(E, heads, kdim = vdim = Ek) with key_padding_mask; rows whose neighbours are all
//   padding get slot 0 unmasked and their output zeroed; then MergeLayer([attn_out | src]).
//
// One workgroup per tile of RQ query rows.  The RQ*n_nbr key rows are staged in LDS once and go through the
// K and the V projection on exact-f32 MFMA (v_mfma_f32_16x16x4_f32) -- the batched QKV contraction is where
// the FLOPs are; scores, softmax, the weighted sum and the small output layers run on the same LDS-to-LDS
// building block.  This file: the eval forward (dropout = identity) and zt::attention_plan.  The tile's device code is
// attention_tile.hpp, shared with the training forward and backward (attention_train.hip).
#include "attention_tile.hpp"

#include <algorithm>

using namespace zt;

namespace {

__global__ __launch_bounds__(ATT_THREADS) void k_temporal_attention(
    AttnDims d, long long N, const float *__restrict__ src, const float *__restrict__ src_t,
    const float *__restrict__ nf, const float *__restrict__ ef, const float *__restrict__ ntf,
    const unsigned char *__restrict__ mask, const float *__restrict__ Wq, const float *__restrict__ Wk,
    const float *__restrict__ Wv, const float *__restrict__ in_b, const float *__restrict__ Wo,
    const float *__restrict__ out_b, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, float *__restrict__ out, float *__restrict__ attn_w)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attention_forward_tile<false>(smem, d, N, src, src_t, nf, ef, ntf, mask, Wq, Wk, Wv, in_b, Wo, out_b, W1, b1, W2, b2, out,
                                  attn_w, AttnDrop{}, AttnSaved{});
}

}  // namespace

// The one place that decides which shapes the layer takes and how a workgroup is tiled (common.hpp; pinned without a GPU
// through zt_test_attention_plan, tests/test_attention_cpu.py).
bool zt::attention_plan(int D, int F, int T, int heads, int hidden, int out_dim, int k, AttnDims &d, size_t &lds, size_t off[8],
                        size_t &ws)
{
    if (D <= 0 || F < 0 || T <= 0 || k <= 0 || hidden <= 0 || out_dim <= 0) return false;
    d.D = D; d.F = F; d.T = T; d.E = D + T; d.Ek = D + F + T; d.heads = heads; d.hidden = hidden; d.out_dim = out_dim;
    d.k = k;
    if (heads <= 0 || heads > 4 || d.E % heads) return false;
    d.hd = d.E / heads;
    d.Ep = round_up(d.E, 16); d.Ekp = round_up(d.Ek, 16); d.E2p = round_up(d.E + D, 16);
    d.Hp = round_up(hidden, 16); d.Op = round_up(out_dim, 16);
    d.lda = d.Ekp + 4; d.ldk = d.Ep + 4;
    d.ldq = std::max(std::max(d.E2p, d.Ep), std::max(d.Hp, d.Op)) + 4;
    int mt = ATT_MAX_MT;
    auto bytes = [&](int m) {
        const size_t kv = std::max((size_t)m * 16 * d.ldk, (size_t)16 * d.ldq);   // K/V tile, later the merger input
        return ((size_t)m * 16 * d.lda + kv) * 4 + (size_t)2 * 16 * d.ldq * 4 + (size_t)m * 16 * 4 * 4 + 64;
    };
    while (mt > 1 && bytes(mt) > ATT_LDS_BOUND) --mt;
    int rq = (mt * 16) / k;
    if (rq < 1) {
        mt = (k + 15) / 16; rq = 1;
        if (mt > ATT_MAX_MT) return false;
    }
    if (rq > 16) rq = 16;
    mt = (rq * k + 15) / 16;
    d.rq = rq; d.mt = mt;
    lds = bytes(mt);
    // the tile that is launched must fit: the loop above stops at one M-tile whether or not that one fits (D = T = 228, k = 10)
    if (lds > ATT_LDS_BOUND) return false;
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o += (b + 255) & ~(size_t)255; return r; };
    off[0] = take((size_t)d.Ep * d.Ep * 4);    // Wq
    off[1] = take((size_t)d.Ep * d.Ekp * 4);   // Wk
    off[2] = take((size_t)d.Ep * d.Ekp * 4);   // Wv
    off[3] = take((size_t)d.Ep * d.Ep * 4);    // Wo
    off[4] = take((size_t)d.Hp * d.E2p * 4);   // merger.fc1
    off[5] = take((size_t)d.Op * d.Hp * 4);    // merger.fc2
    ws = o;
    return true;
}

extern "C" int64_t zt_attention_workspace_bytes(int32_t D, int32_t F, int32_t T, int32_t n_head, int32_t hidden,
                                                int32_t out_dim, int32_t k)
{
    AttnDims d;
    size_t lds, off[8], ws;
    if (!attention_plan(D, F, T, n_head, hidden, out_dim, k, d, lds, off, ws)) return -1;
    return (int64_t)ws;
}

extern "C" int zt_temporal_attention(const float *src_dev, const float *src_time_dev, const float *nbr_feat_dev,
                                     const float *edge_feat_dev, const float *nbr_time_dev, const uint8_t *mask_dev,
                                     int64_t N, int32_t k, int32_t D, int32_t F, int32_t T, int32_t n_head,
                                     int32_t hidden, int32_t out_dim, const zt_attn_weights *w, float *out_dev,
                                     float *attn_w_dev, void *workspace_dev, void *stream)
{
    if (!w || N < 0 || k <= 0 || D <= 0 || F < 0 || T <= 0) { set_error("zt_temporal_attention: bad argument"); return ZT_ERR_ARG; }
    if (N == 0) return ZT_OK;
    if (!src_dev || !src_time_dev || !nbr_feat_dev || !nbr_time_dev || (F > 0 && !edge_feat_dev) || !mask_dev ||
        !out_dev || !attn_w_dev || !workspace_dev) {
        set_error("zt_temporal_attention: NULL buffer");
        return ZT_ERR_ARG;
    }
    AttnDims d;
    size_t lds, off[8], ws;
    if (!attention_plan(D, F, T, n_head, hidden, out_dim, k, d, lds, off, ws)) {
        set_error("zt_temporal_attention: unsupported shape (heads<=4, E %% heads == 0, k <= 80 rows must fit the LDS tile)");
        return ZT_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    char *wsb = reinterpret_cast<char *>(workspace_dev);
    float *Wq = reinterpret_cast<float *>(wsb + off[0]), *Wk = reinterpret_cast<float *>(wsb + off[1]);
    float *Wv = reinterpret_cast<float *>(wsb + off[2]), *Wo = reinterpret_cast<float *>(wsb + off[3]);
    float *W1 = reinterpret_cast<float *>(wsb + off[4]), *W2 = reinterpret_cast<float *>(wsb + off[5]);
    auto pad = [&](const float *W, int rows, int cols, float *Wp, int rp, int cp) {
        k_pad_w<<<(rp * cp + 255) / 256, 256, 0, s>>>(W, rows, cols, cols, 0, Wp, rp, cp);
    };
    pad(w->q_w, d.E, d.E, Wq, d.Ep, d.Ep);
    pad(w->k_w, d.E, d.Ek, Wk, d.Ep, d.Ekp);
    pad(w->v_w, d.E, d.Ek, Wv, d.Ep, d.Ekp);
    pad(w->out_w, d.E, d.E, Wo, d.Ep, d.Ep);
    pad(w->m1_w, hidden, d.E + D, W1, d.Hp, d.E2p);
    pad(w->m2_w, out_dim, hidden, W2, d.Op, d.Hp);
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_temporal_attention), lds));
    const unsigned grid = (unsigned)((N + d.rq - 1) / d.rq);
    k_temporal_attention<<<grid, ATT_THREADS, lds, s>>>(d, N, src_dev, src_time_dev, nbr_feat_dev, edge_feat_dev,
                                                        nbr_time_dev, mask_dev, Wq, Wk, Wv, w->in_b, Wo, w->out_b, W1,
                                                        w->m1_b, W2, w->m2_b, out_dev, attn_w_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
