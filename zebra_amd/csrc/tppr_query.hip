// zt_tppr_query: the rows extract_streaming_tppr (utils/util.py:447-469) gives for arbitrary (node, time) pairs, read from
// the streaming T-PPR state as it lies at rest.  Nothing of the handle is written: no control word, plan set, epoch, hub
// version or latch -- the handle travels to the kernel by value and only `rows` is dereferenced.  The caller orders the call
// behind every writer of the state (include/zebra_amd.h), so rows carry no tag that matters: load_row runs without its tag check.
//   k <= ZT_MAX_K:  one wavefront per (row, model): load_row(expect = 0) + emit_row, the code a negative role's row takes in
//                   k_stream -- the same bits by construction;
//   wider k:        the same wavefront strides over the row's entries, wide_emit's expressions (tppr_wide.hpp) straight from
//                   the granules instead of from that kernel's LDS copy of three rows.
#include "tppr_rows.hpp"

namespace {

constexpr int Q_WAVES = 4;      // (row, model) pairs per workgroup

__global__ __launch_bounds__(WAVE * Q_WAVES) void k_tppr_query(zt_tppr h, const int *__restrict__ nodes,
                                                               const double *__restrict__ ts, long long N, int m_lo, int nm,
                                                               int *__restrict__ on, int *__restrict__ oe, float *__restrict__ od,
                                                               float *__restrict__ ow, int *status)
{
    const int lane = lane_id(), k = h.k;
    const long long task = (long long)blockIdx.x * Q_WAVES + (threadIdx.x >> 6);       // wave-uniform
    if (task >= N * nm) return;
    const int mo = (int)(task / N);
    const long long i = task - (long long)mo * N;
    const long long x = nodes[i];
    const long long o = ((long long)mo * N + i) * k;
    if (x < 0 || x >= h.N) {                                   // the row of an empty dictionary; reported as zt_embed reports it
        for (int j = lane; j < k; j += WAVE) { on[o + j] = 0; oe[o + j] = 0; od[o + j] = 0.f; ow[o + j] = 0.f; }
        if (lane == 0 && status != nullptr) atomicExch(status, (int)ZT_ERR_RANGE);
        return;
    }
    const double tnow = ts[i];
    const int m = m_lo + mo;
    if (k <= ZT_MAX_K) {
        Row r;
        (void)load_row(h, m, x, lane, 0u, r);
        emit_row(r, k, lane, tnow, on + o, oe + o, od + o, ow + o);
        return;
    }
    const u64 *base = h.rows + ((long long)m * h.N + x) * h.rg;
    const int len = (int)(unsigned)base[0];
    for (int j = lane; j < k; j += WAVE) {
        const u64 *e = base + HDR + j;
        const bool a = j < len;
        u64 key = 0ull;
        double ets = 0.0, ew = 0.0;
        if (a) {
            const u64 lo32 = 0xffffffffull;
            key = ((e[k] & lo32) << 32) | (e[0] & lo32);
            ets = __longlong_as_double((long long)(((e[3 * k] & lo32) << 32) | (e[2 * k] & lo32)));
            ew = __longlong_as_double((long long)(((e[5 * k] & lo32) << 32) | (e[4 * k] & lo32)));
        }
        on[o + j] = (int)(unsigned)(key & 0xffffffffull);
        oe[o + j] = (int)(unsigned)(key >> 32);
        ow[o + j] = a ? (float)ew : 0.f;
        const float tsf = a ? (float)ets : 0.f;                 // tmp_timestamps is float32
        od[o + j] = len == 0 ? 0.f : (float)(tnow - (double)tsf);
    }
}

}  // namespace

extern "C" int zt_tppr_query(const zt_tppr *h, const int32_t *nodes_dev, const double *ts_dev, int64_t N, int32_t model,
                             int32_t *out_nodes_dev, int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev,
                             int32_t *status_dev, void *stream)
{
    if (!h || !nodes_dev || !ts_dev || !out_nodes_dev || !out_eidx_dev || !out_dt_dev || !out_w_dev || N < 0) {
        set_error("zt_tppr_query: bad argument");
        return ZT_ERR_ARG;
    }
    if (N == 0) return ZT_OK;                                  // (before the handle is looked at)
    if (model < -1 || model >= h->M) {
        set_error("zt_tppr_query: model %d of %d", model, h->M);
        return ZT_ERR_ARG;
    }
    const int nm = model < 0 ? h->M : 1;
    const long long blocks = (N * nm + Q_WAVES - 1) / Q_WAVES;
    if (blocks > 0x7fffffffll) {
        set_error("zt_tppr_query: N=%lld rows of %d models exceed one launch", (long long)N, nm);
        return ZT_ERR_UNSUPPORTED;
    }
    k_tppr_query<<<(unsigned)blocks, WAVE * Q_WAVES, 0, (hipStream_t)stream>>>(*h, nodes_dev, ts_dev, (long long)N,
                                                                               model < 0 ? 0 : model, nm, out_nodes_dev,
                                                                               out_eidx_dev, out_dt_dev, out_w_dev, status_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
