// Test hooks: direct access to device primitives whose rare paths need their
// own tests (exact top-k selection under ties).  Not part of the product API.
#include "numba_sort.hpp"
#include "tppr_state.hpp"
#include "test_hooks.h"

using namespace zt;

namespace {

struct HookLds {
    double a[1536];
    int sel[64];
    int perm[1536];
    int stk[96];
    SortLds sort;
};

// one wavefront per case; mode 0 = production dispatch (fast / wave / seq),
// 1 = force the wave-parallel exact sort (LDS), 2 = force the sequential replay,
// 3 = force the register-resident replay (n <= 64), 4 = the replay on ranks, 5 / 6 = topk_reg, candidates adjacent / split over the two wave halves (n <= 63, k <= 31)
__global__ __launch_bounds__(64) void k_test_topk(const double *__restrict__ vals, int n, int k, int cases, int mode,
                                                  int *sel_out, int *path_out)
{
    __shared__ HookLds L;
    const int c = blockIdx.x;
    if (c >= cases) return;
    const int lane = lane_id();
    for (int q = lane; q < n; q += WAVE) L.a[q] = vals[(size_t)c * n + q];
    wave_sync();
    int path;
    const long long t0 = (long long)wall_clock64();
    if (mode == 0) {
        path = topk_select_wave(L.a, n, k, L.sel, L.sort, L.perm, L.stk);
    } else if (mode == 4) {                       // the rank-domain replay on its own, ties or not
        const double v = lane < n ? L.a[lane] : 0.0;
        int lt;
        (void)topk_rank_reg(v, n, k, L.sel, &lt);
        topk_ties_reg(lt, n, k, L.sel);
        path = 4;
    } else if (mode == 5 || mode == 6) {          // the register-resident selection of merge_pair_reg:
        // 5 = candidates in lanes [0, n); 6 = split like the merge: the first half in lanes [0, n1), the rest from lane 32
        const int n1 = mode == 5 ? n : (n + 1) / 2;
        const int pos = lane < n1 ? lane : (mode == 6 && lane >= 32 && lane - 32 < n - n1 ? n1 + lane - 32 : -1);
        const u64 live = __ballot(pos >= 0);
        const double v = pos >= 0 ? L.a[pos] : 0.0;
        int slot;
        path = topk_reg(v, live, pos, n, k, &slot);
        if (slot >= 0) L.sel[slot] = pos;
        wave_sync();
    } else if (mode == 3) {
        numba_argsort_reg(L.a, n, L.sort);
        if (lane < k) L.sel[lane] = L.sort.r2[n - k + lane];
        wave_sync();
        path = 3;
    } else if (mode == 1) {
        numba_argsort_wave(L.a, n, L.sort);
        if (lane < k) L.sel[lane] = L.sort.r2[n - k + lane];
        wave_sync();
        path = 1;
    } else {
        if (lane == 0) {
            numba_argsort_seq(L.a, n, L.perm, L.stk);
            for (int q = 0; q < k; ++q) L.sel[q] = L.perm[n - k + q];
        }
        wave_sync();
        path = 2;
    }
    const long long t1 = (long long)wall_clock64();
    if (lane < k) sel_out[(size_t)c * k + lane] = L.sel[lane];
    if (lane == 0) path_out[c] = path | ((int)(t1 - t0) << 8);   // bits 8..: duration in 10 ns ticks
}

}  // namespace

extern "C" int zt_test_topk(const double *vals_dev, int32_t n, int32_t k, int32_t cases, int32_t mode,
                            int32_t *sel_out_dev, int32_t *path_out_dev, void *stream)
{
    if (!vals_dev || !sel_out_dev || !path_out_dev || n < 2 || k < 1 || k >= n || k > 64 || cases < 1 || n > 1536 ||
        (mode == 1 && n > 128) || ((mode == 3 || mode == 4) && n > 64) || ((mode == 5 || mode == 6) && (n > 63 || k > 31))) {
        set_error("zt_test_topk: bad argument");
        return ZT_ERR_ARG;
    }
    k_test_topk<<<cases, 64, 0, (hipStream_t)stream>>>(vals_dev, n, k, cases, mode, sel_out_dev, path_out_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

// move the launch epoch of a T-PPR handle (e.g. next to its wrap-around: all tags are cleared when it reaches 2^17 - 1)
extern "C" int zt_test_set_epoch(zt_tppr *h, uint32_t epoch)
{
    if (!h) return ZT_ERR_ARG;
    h->epoch = epoch > EPOCH_MAX ? EPOCH_MAX : epoch;
    return ZT_OK;
}

// the dependency plan zt_tppr_plan made last (tppr_prepass.hip), copied to host arrays: wo / pflag / hv [3 * B] (B = the
// planned launch's edges), owner_of [B], chain_node / chain_len [16], chain_edges [16][2048]; *n_chains = the chains picked
extern "C" int zt_test_tppr_plan_dump(zt_tppr *h, int32_t *wo, int32_t *pflag, int32_t *hv, int32_t *owner_of,
                                      int32_t *chain_node, int32_t *chain_len, int32_t *chain_edges, int32_t *n_chains)
{
    if (!h) return ZT_ERR_ARG;
    const zt_tppr::PlanSet &P = h->set[h->next_set ^ 1];
    if (!P.valid) return ZT_ERR_ARG;
    ZT_HIP(hipDeviceSynchronize());
    const size_t a = (size_t)P.B * P.n_roles * sizeof(int);
    ZT_HIP(hipMemcpy(wo, P.wo, a, hipMemcpyDeviceToHost));
    ZT_HIP(hipMemcpy(pflag, P.pflag, a, hipMemcpyDeviceToHost));
    ZT_HIP(hipMemcpy(hv, P.hv, a, hipMemcpyDeviceToHost));
    ZT_HIP(hipMemcpy(owner_of, P.owner_of, (size_t)P.B * sizeof(int), hipMemcpyDeviceToHost));
    ZT_HIP(hipMemcpy(chain_node, P.chain_node, MAX_CHAINS * sizeof(int), hipMemcpyDeviceToHost));
    ZT_HIP(hipMemcpy(chain_len, P.chain_len, MAX_CHAINS * sizeof(int), hipMemcpyDeviceToHost));
    ZT_HIP(hipMemcpy(chain_edges, P.chain_edges, (size_t)MAX_CHAINS * CH_MAX * sizeof(int), hipMemcpyDeviceToHost));
    ZT_HIP(hipMemcpy(n_chains, P.ctl + 4, sizeof(int), hipMemcpyDeviceToHost));
    return ZT_OK;
}

extern "C" int zt_test_embed_plan(int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k, int32_t have_table,
                                  int32_t training, int32_t agg_choice, int32_t out_choice, int32_t *agg_out, int32_t *out_out,
                                  int64_t *lds_out)
{
    if (!agg_out || !out_out || !lds_out) return ZT_ERR_ARG;
    const KernelPlan kp = embed_kernel_plan(N, D, F, T, M, k, have_table != 0, training != 0, agg_choice, out_choice);
    *agg_out = (int32_t)kp.agg;
    *out_out = (int32_t)kp.out;
    *lds_out = (int64_t)kp.lds;
    return ZT_OK;
}

extern "C" int zt_test_memory_plan(int64_t max_rows, int32_t D, int32_t msg_dim, int32_t F, int32_t T, int32_t gru_choice,
                                   int32_t msg_choice, int32_t held, int32_t out_form, int32_t hg, int32_t out_D, int32_t out_M,
                                   int32_t gx, int64_t out_N, int32_t same_memory, int64_t *out)
{
    if (!out || out_form < 0 || out_form > 3) return ZT_ERR_ARG;
    const HeldOut h{held != 0, (OutForm)out_form, hg, out_D, out_M, gx, (long long)out_N, same_memory != 0};
    const MemoryPlan mp = memory_kernel_plan(max_rows, D, msg_dim, F, T, gru_choice, msg_choice, h);
    const int64_t v[14] = {(int64_t)mp.refusal, (int64_t)mp.msg, (int64_t)mp.gru, (int64_t)mp.out, (int64_t)mp.lds, (int64_t)mp.lds2,
                           (int64_t)mp.lds_f, mp.gru_tiles, mp.NTg, mp.n_src_wgs, mp.n_nb_wgs, mp.out_tiles, mp.target,
                           mp.participants};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
    return ZT_OK;
}

extern "C" int zt_test_affinity_plan(int64_t B, int32_t H, int32_t choice, int64_t *out)
{
    if (!out) return ZT_ERR_ARG;
    const AffinityPlan ap = affinity_kernel_plan(B, H, choice);
    const int64_t v[7] = {(int64_t)ap.form, ap.KC, ap.ET, ap.gx, ap.gy, ap.threads, (int64_t)ap.lds};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return ZT_OK;
}

extern "C" int zt_test_attention_plan(int32_t D, int32_t F, int32_t T, int32_t n_head, int32_t hidden, int32_t out_dim, int32_t k,
                                      int64_t *out)
{
    if (!out) return ZT_ERR_ARG;
    AttnDims d;
    size_t lds = 0, off[8], ws = 0;
    const bool ok = attention_plan(D, F, T, n_head, hidden, out_dim, k, d, lds, off, ws);
    const int64_t v[4] = {ok ? 1 : 0, ok ? d.rq : 0, ok ? d.mt : 0, ok ? (int64_t)lds : 0};
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return ZT_OK;
}

extern "C" int zt_test_step_plan(int32_t streaming, int32_t masked, int32_t release, int64_t B, int64_t row_lo, int64_t row_hi,
                                 int32_t scoring, int32_t metrics, int32_t exchange, int32_t avg_topk, int32_t proj_table,
                                 int32_t wm_ready, int32_t by_member, int32_t tail_gated, int32_t waited, int32_t have_next,
                                 int64_t next_B, int32_t next_in_slot, int32_t next_by_member, int32_t next_launched,
                                 int32_t next_waited, int32_t next_tail_gated, int64_t *out)
{
    if (!out) return ZT_ERR_ARG;
    const StepFacts f{streaming != 0, masked != 0, release, (long long)B, (long long)row_lo, (long long)row_hi, scoring != 0,
                      metrics != 0, exchange != 0, avg_topk != 0, proj_table != 0, wm_ready != 0, by_member != 0, tail_gated != 0,
                      waited != 0, have_next != 0, (long long)next_B, next_in_slot != 0, next_by_member != 0, next_launched != 0,
                      next_waited != 0, next_tail_gated != 0};
    const StepPlan sp = pipeline_step_plan(f);
    const int64_t v[12] = {(int64_t)sp.gate, sp.wait_filled, sp.wait_launch, sp.gather, sp.avg_topk, sp.scored, sp.measured,
                           sp.gru_is_last, sp.tail_offer, sp.tail_wait_filled, sp.late_project, sp.exchange};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return ZT_OK;
}

extern "C" int zt_test_group_plan(int32_t streaming, int32_t release, int32_t want, int32_t n_more, int64_t *out)
{
    if (!out) return ZT_ERR_ARG;
    const GroupPlan gp = pipeline_group_plan(streaming != 0, release, want, n_more);
    out[0] = gp.by_member;
    out[1] = gp.limit;
    return ZT_OK;
}

extern "C" int zt_test_embed_divided(int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k, int32_t have_table,
                                     int32_t out_choice, int32_t *divided_out)
{
    if (!divided_out) return ZT_ERR_ARG;
    const KernelPlan kp = embed_kernel_plan(N, D, F, T, M, k, have_table != 0, false, 0, out_choice);
    *divided_out = kp.nbr_later ? 1 : 0;
    return ZT_OK;
}

// embed_ex with its output layers held back, then gru_update_ex with them: the two calls of a pipeline step, without the
// pipeline.  The GRU rows are the caller's: gru_ws holds the count (first word) and the row list (zt_gru_rows_offset).
extern "C" int zt_test_embed_gru(float *memory_dev, const float *efeat_dev, int64_t num_nodes, int64_t num_edges, int32_t D, int32_t F,
                                 int32_t T, const int32_t *nodes_dev, int64_t N, int32_t M, int32_t k, const int32_t *nbr_dev,
                                 const int32_t *eix_dev, const float *dt_dev, const float *w_dev, const zt_embed_weights *ew,
                                 float *out_dev, void *embed_ws, int32_t *status_dev, float *proj_table_dev, int32_t embed_ready,
                                 float *last_update_dev, const float *messages_dev, const float *msg_ts_dev, uint8_t *flags_dev,
                                 int32_t msg_dim, int64_t max_rows, const zt_gru_weights *gw, void *gru_ws, int32_t gru_ready,
                                 int32_t cell, int32_t max_wgs, int32_t *out_launch, void *stream)
{
    if (!out_launch || !nodes_dev || max_wgs < 0) return ZT_ERR_ARG;
    embed_out_deferred held{};
    held.max_wgs = max_wgs;
    int rc = embed_ex(memory_dev, efeat_dev, num_nodes, num_edges, D, F, T, nodes_dev, N, M, k, nbr_dev, eix_dev, dt_dev, w_dev, ew,
                      out_dev, embed_ws, status_dev, proj_table_dev, embed_ready, stream, nullptr, &held, nullptr);
    if (rc != ZT_OK) return rc;
    // what the GRU launch will make of them: 0 none (they ran in embed_ex), 1 in front, 2 / 3 fused, 4 behind the tiles (k_nbr_gru)
    HeldOut h{};
    if (held.valid) h = HeldOut{true, held.form, held.hg, held.args.D, held.args.M, held.gx, held.args.N, held.args.memory == memory_dev};
    *out_launch = (int32_t)memory_kernel_plan(max_rows, D, msg_dim, 0, 0, kernel_choice(ZT_CHOICE_GRU), 0, h).out;
    const float *wm_p = proj_table_dev ? embed_wm_ptr(embed_ws, N, D, F, T, M, k) : nullptr;
    return gru_update_ex(memory_dev, last_update_dev, messages_dev, msg_ts_dev, flags_dev, num_nodes, D, msg_dim, nodes_dev, max_rows,
                         nullptr, gw, gru_ws, gru_ready, wm_p, wm_p ? proj_table_dev : nullptr, stream, true, true, &held, cell);
}

extern "C" int zt_test_decoder_arrangement(int32_t value)
{
    if (value != 0 && value != 1 && value != 5) return ZT_ERR_ARG;
    g_decoder_arrangement = value;
    return ZT_OK;
}
