// Shared host/device helpers for libzebra_amd (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "../../include/zebra_amd.h"

namespace zt {

void set_error(const char *fmt, ...);

// Shared by the dense f32-MFMA kernels of the embedding path (aggregate.hip, aggregate_split.hip, aggregate_bwd.hip,
// embed_out_body.hpp, fc1_tile.hpp).  In a namespace of their own: other translation units keep helpers of these names.
namespace dense {
typedef float f32x4 __attribute__((ext_vector_type(4)));
__host__ __device__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
constexpr int AGG_LDS_BUDGET = 150 * 1024;     // dynamic LDS one workgroup of the aggregation kernels may ask for
constexpr int AGG_THREADS = 256;
constexpr int AGG_WAVES = 4;
constexpr int NTW = 2;             // N-tiles per wave -> D <= 128
constexpr int NTW_WIDE = 4;        // ... of the instantiations for 128 < D <= 256 (D % 4 == 0)
}  // namespace dense
// p -> threshold of drop_scale (0 = no dropout); host side
inline unsigned drop_threshold(float p)
{
    if (!(p > 0.f)) return 0u;
    const double t = (double)p * 4294967296.0;
    return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}

// The node decoder's launch (decoder.hip: zt::decoder_plan is the one place that picks it; zt_node_decoder_plan publishes it).
// pin: 0 = the plan's pick, 1 / 5 = that arrangement (the test hook zt_test_decoder_arrangement sets g_decoder_arrangement).
struct DecoderPlan {
    int arrangement;        // 0 refused; 1: one wave owns the five N-tiles of 16 rows; 5: five waves own one N-tile each
    int waves, threads, rows, k_chunk;
    long long grid, lds_bytes;
    int split;              // partial products of d_fc1_w in the backward
    long long k_per;        // rows per partial product
};
DecoderPlan decoder_plan(int64_t N, int H, bool training, int pin);
extern int g_decoder_arrangement;

// Optional HIP-event timing of individual kernels (zt_profile_* in the ABI):
// an event pair is recorded on the launch stream around the kernel; elapsed
// times are summed per kernel name when the profile is read.
enum ProfId { P_PREPASS = 0, P_STREAM, P_CLEANUP, P_PRUNE, P_EMBED_PREP, P_FC1_AGG, P_EMBED_OUT, P_STORE_MSG, P_GRU,
              P_SCORE, P_EXCHANGE, P_LINK_BCE, P_ADAM, P_COUNT };
extern bool g_prof_on;
void prof_begin(hipStream_t s, int id);
void prof_end(hipStream_t s, int id);
// zt_tppr_stream for callers inside the library (tppr_stream.hip)
int tppr_stream_ex(zt_tppr *h, const int32_t *nodes_dev, const double *ts_dev, const int64_t *eidx_dev, int64_t B,
                   int32_t n_roles, int32_t emit, int32_t model, int32_t *out_nodes_dev, int32_t *out_eidx_dev,
                   float *out_dt_dev, float *out_w_dev, uint64_t plan_token, void *stream, bool plan_ordered,
                   hipEvent_t *done_out, int32_t sub_B, int32_t *member_done_dev = nullptr);
// member_done_dev (launches over several batches: sub_B > 0): TPPR_MEMBER_WORDS ints, zero when the launch starts.  Word g counts
// the (edge, model) tasks of batch g whose output rows are written -- visible at agent scope when the count is -- so that a
// consumer of batch g's rows need not wait for the end of the launch: word g == B_g * models opens it (pipeline.hip:
// k_member_gate).  A launch that k_count rejected (ZT_ERR_RANGE) writes its empty rows and sets every word to INT_MAX.
constexpr int TPPR_MAX_MEMBERS = 8;         // batches per launch that can be released one by one
constexpr int TPPR_MEMBER_WORDS = TPPR_MAX_MEMBERS + 1;      // (the last word: workgroups of a rejected launch that are through)
// The output layers' arguments (k_embed_out, k_embed_out2, k_out_gru, k_out_gru2 take it by value: a kernel argument, keep
// the layout)
struct EmbedOutArgs {
    const float *memory;
    long long num_nodes;
    const int *nodes;
    long long N;
    int D, M;
    const float *H, *S, *fc2_p, *fc2_b, *fc1s_p, *fc1s_b, *fc2s_p, *fc2s_b;
    float *out;
    int *status;
};
// The embedding's kernels for one shape (aggregate.hip: embed_kernel_plan).  The aggregation: tiled_* = k_fc1_agg<TAB, MMT>
// over the [ef | time] tile of the projected table or the full [memory | ef | time] one, *_big its MAX_MT_BIG instantiation
// (80 < k); reg = k_fc1_agg_reg, wide = k_fc1_agg_wide (aggregate_wide.hip), d100 = k_fc1_agg_d100, split = k_fc1_agg_split
// (aggregate_split.hip).  Every kernel of a family gives the same bits; the choice is speed only (tests/test_launch_plan_cpu.py).
enum class AggKernel { unsupported, reg, wide, d100, tiled_table, tiled_full, tiled_table_big, tiled_full_big, split };
// the output layers: k_embed_out (tiled), k_embed_out2 (latency: small batches), k_embed_out3 (persist: large ones);
// persist_nbr: the neighbour paths of the persistent form alone -- what embed_ex holds back after it has launched the source
// path by itself (KernelPlan::nbr_later); never a plan's own answer
enum class OutForm { tiled, latency, persist, persist_nbr };
// why a shape is refused: no kernel or workspace for it / no tile holds a query row and no chunk of one fits (zt_embed: it needs
// the projected table) / partial-sum groups the output layers have no instantiation for
enum class Refusal { none, shape, no_split, groups };
struct KernelPlan {
    AggKernel agg;
    OutForm out;
    Refusal refusal;       // agg == unsupported: why
    size_t lds;            // dynamic LDS of the tiled and d100 launches (the other launchers size their own)
    int rq, mt, lda;       // their tile: query rows, 16-row M-tiles, leading dimension
    int hg;                // partial-sum groups per query row in H (k_fc1_agg_wide: k / 4; else 1)
    // out == persist, for a caller that can hold output layers back (embed_ex: `defer`): the source path is launched by itself
    // and the neighbour paths are handed on as OutForm::persist_nbr, for the GRU update's launch (k_nbr_gru).  A direct
    // zt_embed runs k_embed_out3 whole either way.  ZT_OUT_NBR_GRU asks for it at any batch size; ZT_OUT_WHOLE (the pick by
    // shape) and ZT_OUT_PERSIST forbid it.
    bool nbr_later;
};
// Pure host code (no HIP calls).  training: zt_agg_train_forward's choice (no table; tiled_full or split)
KernelPlan embed_kernel_plan(int64_t N, int D, int F, int T, int M, int k, bool have_table, bool training, int agg_choice,
                             int out_choice);
// The memory update's kernels for one shape (memory_update.hip: memory_kernel_plan): the message build (k_build_messages, or
// k_build_messages2: two batch positions per wave); the GRU / RNN update (none: no rows; tile = k_gru, split = k_gru_split);
// output layers held back by embed_ex (launched in front of the GRU kernel -- or on the way out of a refused or empty update
// --, fused with k_gru: k_out_gru, or with k_gru_split: k_out_gru2; fused_nbr: the neighbour paths of the persistent form behind
// k_gru's tiles in one grid, k_nbr_gru -- no gate: they read nothing the update writes).  The choice is speed only: wherever
// and in whichever form the output layers are launched they give the same bits, and so do the two message kernels; the two
// GRU forms agree to rounding, not to the bit (the split's four waves divide K among them and add their partial gate sums
// afterwards; tests/test_embed_gpu.py holds the two to 2e-6).  Held-back neighbour paths draw an update of <= 512 rows, the
// split's by the library's pick, to the tile: that happens under ZT_OUT_NBR_GRU only (the pipeline's update has two thirds
// as many rows as its output layers, which are divided from 8 192 rows on), and moves such an update's rows by that rounding.
enum class MsgKernel { one, two };
enum class GruForm { none, tile, split };
enum class OutLaunch { none, front, fused_tile, fused_split, fused_nbr };
enum class MemRefusal { none, arg, d_large, msg_wide };      // bad argument / D > 128 / message width too large
// the held-back output layers (embed_out_deferred) as far as the GRU launch needs them; same_memory: they read the table updated
struct HeldOut {
    bool present;
    OutForm form;
    int hg, D, M, gx;
    long long N;
    bool same_memory;
};
struct MemoryPlan {
    MsgKernel msg;
    GruForm gru;
    OutLaunch out;
    MemRefusal refusal;
    size_t lds, lds2, lds_f;           // dynamic LDS of k_gru, k_gru_split and the fused kernel
    int gru_tiles, NTg;                // 16-row tiles, hidden N-tiles
    int n_src_wgs, n_nb_wgs, out_tiles;     // k_out_gru2's source- and neighbour-path workgroups; k_out_gru's row tiles
                                            // (k_nbr_gru: n_nb_wgs = the neighbour workgroups asked for; the launch caps them at
                                            //  one per compute unit of the stream)
    unsigned grid;                     // workgroups of the launch (k_gru_split: x dimension)
    unsigned target, participants;     // the fused kernels' SrcGate
};
// Pure host code (no HIP calls).  F, T: the message's edge-feature and time widths; the choices: ZT_CHOICE_GRU, ZT_CHOICE_MESSAGES
MemoryPlan memory_kernel_plan(int64_t max_rows, int D, int msg_dim, int F, int T, int gru_choice, int msg_choice,
                              const HeldOut &held);
// The eval link scorer's kernel for one batch (scoring.hip: affinity_kernel_plan).  latency = k_affinity<KC> (one wave per
// 16-edge tile and N-tile, weights in registers), tiled = k_affinity_tiled<KC, ET> (ET edges per workgroup staged in LDS): the two
// specialised forms of round_up16(H) = 16 KC in {208, 304}; gen_latency = k_affinity_gen, gen_tiled = k_affinity_gen_tiled: any
// H % 4 == 0, 4 <= H <= 768 (K and N run over H at run time).  Every form computes the same function; they differ in how the
// float32 sums associate.  The values are the ZT_SCORE_* of ZT_CHOICE_SCORE.
enum class AffForm { refused = 0, latency = 1, tiled = 2, gen_latency = 3, gen_tiled = 4 };
struct AffinityPlan {
    AffForm form;
    int KC, ET;            // the specialised forms' template arguments (0 for the generic ones)
    unsigned gx, gy;       // grid
    unsigned threads;
    size_t lds;            // dynamic LDS
};
// Pure host code (no HIP calls).  A function of (B, H, choice) alone -- never of the workspace's max_B: the pipeline and a direct
// call pick the same kernel for the same batch.  choice: ZT_CHOICE_SCORE (a form the width cannot take: the library's pick)
AffinityPlan affinity_kernel_plan(int64_t B, int H, int choice);
// The link-metrics kernel for B positive and B negative scores (scoring.hip: link_metrics_plan).  single = k_link_metrics (the 2B
// scores as u64 (key | label) in one bitonic sort, n2 = the padded length, 8 bytes each); split = k_link_metrics_split (the B
// positive and the B negative 32-bit keys sorted as two runs of n2 / 2 each, 4 bytes per key, then walked together).  One
// workgroup either way.  The values are the ZT_METRICS_FORM_* of zt_link_metrics_plan.
enum class MetForm { refused = 0, single = 1, split = 2 };
constexpr int64_t METRICS_SINGLE_MAX_B = 8192, METRICS_MAX_B = 16384;
struct MetricsPlan {
    MetForm form;
    unsigned threads;
    int n2;                // keys in LDS (padding included)
    size_t lds;            // dynamic LDS
};
// Pure host code (no HIP calls): refused for B <= 0 and beyond METRICS_MAX_B pairs
MetricsPlan link_metrics_plan(int64_t B);
// One step of the pipeline (pipeline.hip: pipeline_step_plan): where the wait for this batch's T-PPR rows goes and what the
// step puts behind its GRU update.  The gate of a member: carried = the GRU kernel of the step before waited for its rows (no
// gate here); event = the main stream waits for the launch's event; front = k_member_gate in front of the aggregation;
// in_aggregation = the gate is offered to the aggregation kernel (embed_ex).  Every form releases the same rows: the choice is
// speed only, and the GPU suite cannot tell one from another (tests/test_launch_plan_cpu.py).
enum class GateForm { carried = 0, event = 1, front = 2, in_aggregation = 3 };
struct StepFacts {
    bool streaming, masked;            // the strategy; the T-PPR stream and the main stream own disjoint compute units
    int release;                       // ZT_CHOICE_GROUP_RELEASE
    long long B, row_lo, row_hi;       // the batch and the rows of it this step embeds
    bool scoring, metrics, exchange, avg_topk, proj_table;      // what is attached to the pipeline
    bool wm_ready;                     // the padded W_m is in the embed workspace (the GRU kernel refreshes the projected rows)
    bool by_member, tail_gated, waited;      // this member's slot; its bit of Slot::tail_gated
    bool have_next;                    // a valid batch follows; the rest describes it
    long long next_B;
    bool next_in_slot, next_by_member, next_launched, next_waited, next_tail_gated;
};
struct StepPlan {
    GateForm gate;
    bool wait_filled;                  // front / in_aggregation: the main stream waits for the slot's `filled` first (once per group)
    bool wait_launch;                  // event: ... for the launch's event (once per launch)
    bool gather;                       // a shard's rows of a streaming launch are brought together
    bool avg_topk;                     // k_avg_topk runs
    bool scored, measured;
    bool gru_is_last;                  // the GRU update is the last thing the step puts on the main stream
    bool tail_offer;                   // the next member's gate is offered to the GRU kernel's tail ...
    bool tail_wait_filled;             // ... behind the next slot's `filled`
    bool late_project;                 // zt_project_memory behind the GRU update (no padded W_m yet)
    bool exchange;
};
// Pure host code (no HIP calls, no pointer of the pipeline)
StepPlan pipeline_step_plan(const StepFacts &f);
// A launch group (pipeline.hip: make_group): released by member or by the launch's event, and how many batches it may take.
// want: zt_pipeline_set_group; n_more: the batches in sight behind the first
struct GroupPlan {
    bool by_member;
    int limit;
};
GroupPlan pipeline_group_plan(bool streaming, int release, int want, int n_more);
// The attention layer's tile for one shape (attention.hip: attention_plan).  One workgroup takes rq query rows (at most 16) and
// their rq * k key rows in mt 16-row M-tiles (at most 5); lda / ldk / ldq are the leading dimensions of its LDS regions.
struct AttnDims {
    int D, F, T, E, Ek, heads, hd, hidden, out_dim, k;
    int Ep, Ekp, E2p, Hp, Op;       // padded widths: E, Ek, E+D, hidden, out_dim
    int rq, mt, lda, ldk, ldq;
};
constexpr size_t ATT_LDS_BOUND = 158 * 1024;
// Pure host code (no HIP calls).  false: the shape is refused (a bad width, heads outside 1 ... 4 or not dividing E, a query
// row's k key rows beyond 5 M-tiles, or a tile whose dynamic LDS `lds` would exceed ATT_LDS_BOUND).  off[0 .. 5]: the padded
// weights' offsets in the workspace of `ws` bytes
bool attention_plan(int D, int F, int T, int heads, int hidden, int out_dim, int k, AttnDims &d, size_t &lds, size_t off[8],
                    size_t &ws);
// The layer's training pair (attention_train.hip; published by zt_attention_train_plan).  The tile (rq, mt) and the forward's
// LDS and padded weights are attention_plan's; the backward runs in the same LDS carve-up, so it refuses nothing more.
//   workspace = fixed + N * ws_row:  the forward's padded weights [0, fwd_ws), the transposed padded merger.fc2, merger.fc1
//     and out_proj at off_t[0 .. 2], then from `fixed` the row deltas d_hid [N][hidden], d_y [N][E], d_q / sqrt(hd) [N][E],
//     d_K [N k][E], d_V [N k][E], one after the other
//   saved = N * saved_row:  p [N][k][heads], o [N][E], y [N][E], relu(fc1) [N][hidden], one after the other
struct AttnTrainPlan {
    size_t lds_fwd, lds_bwd, fwd_ws, off[8], off_t[3], fixed, ws_row, saved_row;
};
bool attention_train_plan(int D, int F, int T, int heads, int hidden, int out_dim, int k, AttnDims &d, AttnTrainPlan &p);
// zt_link_metrics with a second destination: row (or NULL) receives the batch's three values whatever `accumulate` does to out
// (the metrics tail of the native step, pipeline.hip: the running sum and the per-batch table from one launch)
int link_metrics_launch(const float *pos_dev, const float *neg_dev, int64_t B, double *out_dev, int accumulate, double *row_dev,
                        hipStream_t stream);
// The output layers of an embed call, held back (embed_ex: `defer`) so that gru_update_ex can launch them in ONE kernel with the
// GRU update (k_out_gru, memory_update.hip): the two are independent apart from the memory rows the source path reads --
// the GRU half waits for those reads before it writes (a gate in the GRU workspace whose whole state is device memory: a
// count of source-path units that have their rows and a count of participants that have left; the last one out zeroes both, so
// every launch finds them at zero whatever the host did in between; the wait is bounded and reports to `status` / `latch`).
struct embed_out_deferred {
    bool valid;
    EmbedOutArgs args;
    int hg;
    OutForm form;          // (latency: gx tiles' worth of waves per path and N-tile; persist is never held back whole:
                           //  persist_nbr is its neighbour half, the source half launched already)
    int gx;
    int *latch;            // host-mapped word a gate wait that gives up writes ZT_ERR_TIMEOUT to (or NULL); kept across embed_ex calls
    int max_wgs = 0;       // the divided persistent form's launches (k_embed_src3, k_nbr_gru's neighbour half, k_embed_nbr3): at most
                           // so many persistent workgroups each; 0 = one per compute unit of the stream.  The caller's, like latch
};
struct member_gate;                                                         // (below: the wait for one batch's T-PPR rows)
int embed_out_launch(const embed_out_deferred &d, void *stream);           // aggregate.hip: the output layers as a kernel of their own
// zt_gru_update with the projected-table refresh folded into the GRU kernel (memory_update.hip); wm_p from embed_wm_ptr.
// counter_zeroed: the row counter (first word of the workspace) is zero already; select_done: the row list and the counter
// are filled (pipeline.hip: the message kernel hands its list of winners over), no compaction of flagged ids.
// cell: ZT_CELL_GRU (zt_gru_update) or ZT_CELL_RNN (zt_rnn_update: wt holds the RNNCell's weights), same workspace
int gru_update_ex(float *memory_dev, float *last_update_dev, const float *messages_dev, const float *msg_ts_dev,
                  uint8_t *flags_dev, int64_t num_nodes, int32_t D, int32_t msg_dim, const int32_t *ids_dev, int64_t n_ids,
                  const int32_t *n_ids_dev, const zt_gru_weights *wt, void *workspace_dev, int32_t weights_ready,
                  const float *wm_p, float *proj_table, void *stream, bool counter_zeroed = false, bool select_done = false,
                  embed_out_deferred *fuse = nullptr, int cell = ZT_CELL_GRU, const member_gate *tail_gate = nullptr,
                  bool *tail_carried = nullptr);
// tail_gate (pipeline.hip, "the gate at the tail of the GRU"): the wait for the NEXT batch's T-PPR rows, carried by the first
// workgroup of the plain k_gru once its rows are written; *tail_carried says whether the kernel that was launched took it along
// zt_store_messages_range that also zeroes one int (the GRU update's row counter: first word of its workspace)
int store_messages_ex(const float *memory_dev, const float *last_update_dev, const float *efeat_dev, const float *time_w_dev,
                      int64_t num_nodes, int64_t num_edges, int32_t D, int32_t F, int32_t T, const int32_t *src_dev,
                      const int32_t *dst_dev, const double *ts_dev, const int64_t *eidx_dev, int64_t B, int64_t pos_lo,
                      int64_t pos_hi, float *messages_dev, float *msg_ts_dev, uint8_t *flags_dev, int32_t *scratch_dev,
                      int32_t *uniq_ids_dev, int32_t *n_uniq_dev, int32_t *status_dev, int32_t *zero_word_dev, void *stream,
                      bool *zeroed_out = nullptr, bool set_flags = true);
// The wait for ONE batch's T-PPR rows inside a launch that covers several (pipeline.hip, "release by member"; the counter is
// tppr_stream_ex's member_done_dev): word == nullptr: none.  The persistent aggregation kernels take it as arguments and wait
// behind their weight prologue (no packet of its own on the stream); for the others member_gate_launch puts a one-wave kernel
// in front.
struct member_gate {
    const int32_t *word;
    int32_t target;
    int *latch;            // host-mapped word a wait that gives up writes ZT_ERR_TIMEOUT to (or NULL)
    int32_t *status;       // ... and the status word (gru_update_ex's tail gate: that call has no status argument of its own)
};
int member_gate_launch(const member_gate &g, int32_t *status_dev, void *stream);      // aggregate.hip
// zt_embed with an event the stream waits for between the aggregation kernel and the output layer (pipeline.hip: the
// message build; a wait packet right in front of the GRU costs the step ~6 us of command-processor time, here it is
// processed while the aggregation runs)
int embed_ex(const float *memory_dev, const float *efeat_dev, int64_t num_nodes, int64_t num_edges, int32_t D, int32_t F, int32_t T,
             const int32_t *nodes_dev, int64_t N, int32_t M, int32_t k, const int32_t *nbr_dev, const int32_t *eix_dev,
             const float *dt_dev, const float *w_dev, const zt_embed_weights *wt, float *out_dev, void *workspace_dev,
             int32_t *status_dev, const float *proj_table_dev, int32_t weights_ready, void *stream, hipEvent_t mid_wait,
             embed_out_deferred *defer = nullptr, const member_gate *gate = nullptr);
// W_m (the memory columns of fc1, padded to [Dp][Dp]) inside an embed workspace prepared for (N, D, F, T, M, k) (aggregate.hip)
const float *embed_wm_ptr(void *embed_ws, int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k);
// the persistent aggregate kernel for wide edge features (aggregate_wide.hip: F = 172, weights resident in LDS)
bool fc1_agg_wide_supported(int D, int F, int T, int k);
size_t fc1_agg_wide_weight_bytes();
void fc1_agg_wide_pack(const float *fc1_w_dev, const float *time_w_dev, const float *fc1_b_dev, float *packed_dev, hipStream_t s);
int fc1_agg_wide_launch(const float *P, const float *efeat, const float *time_w, long long num_nodes, long long num_edges,
                        long long N, int M, int k, const int *nbr, const int *eix, const float *dt, const float *w,
                        const float *packed, const float *b1, float *G, float *S, int *status, int cus, hipStream_t s,
                        const member_gate *gate = nullptr);
// the row-split aggregation (aggregate_split.hip): one workgroup per (model, query row), the k gathered rows in chunks --
// zt_agg_train_forward beyond one tile and zt_embed where no tile holds a query row.  rows: 0 = unsupported widths
int fc1_agg_split_rows(int D, int F, int T);
// zt_agg_train_backward takes (D, F, T, k) (aggregate_bwd.hip)
bool agg_backward_supported(int D, int F, int T, int k);
size_t fc1_agg_split_lds(int D, int F, int T);
// The arguments of the neighbour aggregation's general kernels (k_fc1_agg, k_fc1_agg_split take it by value beside their tile
// parameters; k_fc1_agg_bwd inside its BwdArgs): H[m][n][:] = sum_k w_k/sum(w) drop(relu(fc1([memory'[nbr] | ef | cos(dt w)])))
struct FcAggArgs {
    const float *memory;               // [num_nodes][ldm]: the memory table -- or (k_fc1_agg<true>) the projected table
    const float *efeat, *time_w;       // [num_edges][F], [T]
    long long num_nodes, num_edges, N;
    int D, F, T, M, k;
    int ldm;                           // row stride of `memory`: D (the projected table: Dp)
    const int *nbr, *eix;              // [M][N][k]
    const float *dt, *w;               // [M][N][k]
    const float *W1p;                  // [Dp][K1p] zero padded fc1 weight (the table path: its [ef | time] columns)
    int K1p;
    const float *b1;
    float *H, *S;                      // [M][N][D], [M][N]
    int *status;
    const float *overlay;              // training: [U][D] rows of the lazily updated memory, or NULL
    const int *row_map;                // [num_nodes]: overlay row or -1; NULL: no overlay
    unsigned drop_lo, drop_hi, drop_thr;   // training dropout of the hidden layer (drop_scale below); thr = 0: none
    float drop_inv;

    void set_dropout(float p, unsigned long long seed)
    {
        drop_lo = (unsigned)seed; drop_hi = (unsigned)(seed >> 32);
        drop_thr = drop_threshold(p);
        drop_inv = drop_thr ? 1.f / (1.f - p) : 1.f;
    }
};
int fc1_agg_split_launch(const FcAggArgs &a, hipStream_t s);
int pruned_topk_multi_fill(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t nq, int32_t width,
                           int32_t depth, int32_t n_models, const double *alpha_host, const double *beta_host, int32_t k,
                           int32_t *out_nodes_dev, int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev,
                           int32_t *status_dev, void *stream);     // tppr_prune.hip: empty rows written as zeros (no memset before)
void tppr_hint_cus(zt_tppr *h, hipStream_t s);      // tppr_prepass.hip: plan for the compute units of stream s
// exchange.hip: the row exchange of one step of a multi-GPU run on `stream` (pack -> all-gather -> scatter); the ids of
// the rows written (-1: padding) come back for the projected-row refresh
int exchange_step(zt_exchange *x, const int32_t *rows_dev, const int32_t *count_dev, void *stream, const int32_t **ids_out,
                  int64_t *n_ids_out);
void exchange_shape(const zt_exchange *x, int *rank, int *world);
constexpr int TPPR_MAX_LAUNCH = 16384;     // edges one T-PPR launch can cover (tppr_stream.hip: MAX_CHUNK)
// The memory / embedding widths the dense kernels take: D <= 128 (two N-tiles per wave of four, one per wave of eight), or
// 128 < D <= 256 with D % 4 == 0 (their wide instantiations move memory rows as 16-byte vectors)
constexpr int MAX_D = 256;
inline bool width_supported(int D) { return D > 0 && (D <= 128 || (D <= MAX_D && D % 4 == 0)); }

// hipFuncAttributeMaxDynamicSharedMemorySize of kernel fn raised to `bytes` where that is above 48 KB and above what was set
// for fn before (runtime.hip)
hipError_t set_dynamic_lds(const void *fn, size_t bytes);
// f(std::integral_constant<int, V>{}) for the V of Vs that equals v -- one instantiation of f per value -- and the ZT_* code
// it returns; ZT_ERR_UNSUPPORTED where v is none of Vs
template <int... Vs, class Fn>
int dispatch(int v, Fn &&f)
{
    int rc = ZT_ERR_UNSUPPORTED;
    (void)((v == Vs && (rc = f(std::integral_constant<int, Vs>{}), true)) || ...);
    return rc;
}

// flags of the events that only order streams of this device
inline unsigned sync_event_flags() { return 0u; }
// zt_set_kernel_choice: 0 = the library picks by shape (runtime.hip)
int kernel_choice(int which);
// CUs a stream may use (CU-masked streams: the size of the mask; queried per call -- runtime.hip)
int stream_cu_count(hipStream_t s);
#define ZT_PROF_BEGIN(s, id) do { if (zt::g_prof_on) zt::prof_begin((s), (id)); } while (0)
#define ZT_PROF_END(s, id) do { if (zt::g_prof_on) zt::prof_end((s), (id)); } while (0)

#define ZT_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            zt::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__,   \
                          __LINE__);                                                          \
            return ZT_ERR_HIP;                                                                \
        }                                                                                     \
    } while (0)

#define ZT_LAUNCH_CHECK()                                                                     \
    do {                                                                                      \
        hipError_t e__ = hipGetLastError();                                                   \
        if (e__ != hipSuccess) {                                                              \
            zt::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__),         \
                          __FILE__, __LINE__);                                                \
            return ZT_ERR_HIP;                                                                \
        }                                                                                     \
    } while (0)

typedef unsigned long long u64;

constexpr int WAVE = 64;

// ---- device helpers ---------------------------------------------------------
#if defined(__HIPCC__)

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }

// Make this wave's LDS writes visible to its own later cross-lane LDS reads
// (orders the compiler and drains lgkmcnt; no workgroup barrier involved).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// v from the lane a DPP control selects (0x120 | n: row_ror:n -- rotation inside each row of 16 lanes)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ u64 lanemask_lt() { return (1ull << lane_id()) - 1ull; }

// Agent-scope relaxed accesses: lower to global_load/store ... sc1 (L1 bypass /
// write-through), the form cross-CU hand-offs inside one launch need
// (cdna_hip_programming.md Guideline 16, recipe R1).
__device__ __forceinline__ u64 ld_agent(const u64 *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(u64 *p, u64 v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double *p)
{
    return __longlong_as_double((long long)ld_agent(reinterpret_cast<const u64 *>(p)));
}
__device__ __forceinline__ void st_agent(double *p, double v)
{
    st_agent(reinterpret_cast<u64 *>(p), (u64)__double_as_longlong(v));
}
__device__ __forceinline__ int ld_agent(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int *p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(float *p, float v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned ld_agent(const unsigned *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned *p, unsigned v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ONE lane's atomic add on behalf of its wave, without a branch in the program: the wave's queue claims (k_stream).
// What the obvious forms compile to (seen in the ISA, round 6): `if (lane == 0) old = atomicAdd(p, 1)` is jump-threaded with
// lane-0 code around it and the structurizer replays the loop body for the other lanes; `atomicAdd(p, lane == 0 ? 1 : 0)` --
// written to avoid that -- makes the compiler's atomic optimizer wrap the add in a scan over the 64 lanes ONE LANE AT A TIME
// (s_ff1 / v_readlane / v_writelane / s_andn2 ...: 9 instructions x 64 = ~580 per claim, on a chain workgroup whose instruction
// issue is what bounds a hub chain); `atomicAdd(p, 1)` by every lane with a pointer the compiler cannot prove uniform is 64
// atomics to one address (~10 ns each at the memory side).  Here: exec = lane 0 for the one instruction.
// PRECONDITION: called in wave-uniform control flow with every lane active (the top of k_stream's two queue loops) -- lane 0
// issues the add with ITS copy of the operands, and the result is read from lane 0.
// Returns the value before the add, wave-uniform.  p: LDS.
__device__ __forceinline__ int wave_claim_lds(int *p, int v)
{
    int old;
    unsigned long long save;
    const unsigned a = (unsigned)(unsigned long long)p;              // generic -> LDS: the low 32 bits are the LDS address
    asm volatile("s_mov_b64 %1, exec\n\t"
                 "s_mov_b64 exec, 1\n\t"
                 "ds_add_rtn_u32 %0, %2, %3\n\t"
                 "s_mov_b64 exec, %1\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(old), "=&s"(save) : "v"(a), "v"(v) : "memory");
    return __builtin_amdgcn_readlane(old, 0);
}
// p: global memory (agent scope, as atomicAdd)
__device__ __forceinline__ int wave_claim_global(int *p, int v)
{
    int old;
    unsigned long long save;
    asm volatile("s_mov_b64 %1, exec\n\t"
                 "s_mov_b64 exec, 1\n\t"
                 "global_atomic_add %0, %2, %3, off sc0\n\t"
                 "s_mov_b64 exec, %1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(old), "=&s"(save) : "v"(p), "v"(v) : "memory");
    return __builtin_amdgcn_readlane(old, 0);
}
// ... and without a result: fire and forget
__device__ __forceinline__ void wave_add_global(int *p, int v)
{
    unsigned long long save;
    asm volatile("s_mov_b64 %0, exec\n\t"
                 "s_mov_b64 exec, 1\n\t"
                 "global_atomic_add %1, %2, off\n\t"
                 "s_mov_b64 exec, %0"
                 : "=&s"(save) : "v"(p), "v"(v) : "memory");
}

// by ONE thread: poll `word` (agent scope) until it reaches `target`; bounded like every in-kernel wait of the library (4 s of
// the 100 MHz wall clock), then ZT_ERR_TIMEOUT to the status word and the latch.  false: gave up.
// SLEEP: 64-clock units between two polls.  Inside the persistent aggregation kernels EVERY workgroup polls the one word:
// at ~0.3 us a poll, 192 of them kept one memory channel busy with nothing else and k_stream -- whose counters live in that
// line -- lost 5 % (measured); there a poll every ~4 us (a gate that is open when the kernel arrives costs no sleep at all).
template <int SLEEP = 8>
__device__ __forceinline__ bool member_gate_wait(const int *word, int target, int *status, int *latch)
{
    unsigned spins = 0;
    long long t0 = 0;
    while (ld_agent(word) < target) {
        __builtin_amdgcn_s_sleep(SLEEP);
        if ((++spins & (SLEEP >= 64 ? 127u : 1023u)) == 0) {
            const long long now = (long long)wall_clock64();
            if (t0 == 0) t0 = now;
            else if (now - t0 > 400000000ll) {
                atomicExch(status, ZT_ERR_TIMEOUT);
                if (latch != nullptr) __hip_atomic_store(latch, (int)ZT_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return false;
            }
        }
    }
    return true;
}
// a whole workgroup: thread 0 waits, the others wait for it (word == nullptr: nothing, not even the barrier)
__device__ __forceinline__ void member_gate_enter(const int *word, int target, int *status, int *latch)
{
    if (word == nullptr) return;
    if (threadIdx.x == 0) (void)member_gate_wait<127>(word, target, status, latch);
    __syncthreads();
}

// cos(x) for the time encoding.  |x| < 4e6: float32 Cody-Waite reduction with three FMA steps
// (k = rint(x*2/pi), pi/2 split into floats, two FMA steps: each is exact up to one rounding of an O(1)
// value); larger arguments: the same reduction in float64.  Float32 polynomials on [-pi/4, pi/4].
// |err| <= 3e-7 over |x| <= 3e8 (ocml cosf: 7e-8), at a fraction of the instructions of the
// Payne-Hanek path large arguments take in ocml.
__device__ __forceinline__ float time_cos_poly(float rf, int q)
{
    const float s = rf * rf;
    const float c = fmaf(s, fmaf(s, fmaf(s, fmaf(s, 2.4801587e-5f, -1.3888889e-3f), 4.1666668e-2f), -0.5f), 1.0f);
    const float sn = rf * fmaf(s, fmaf(s, fmaf(s, fmaf(s, 2.7557319e-6f, -1.9841270e-4f), 8.3333338e-3f), -1.6666667e-1f), 1.0f);
    const float res = (q & 1) ? sn : c;
    return ((q + 1) & 2) ? -res : res;
}

__device__ __noinline__ float time_cosf_large(float x)
{
    // beyond 1e15 the quotient k no longer fits the float64 reduction below (k * pi/2 must stay exact to
    // ~1e-17 * k): take the library's Payne-Hanek path; such arguments (dt > 3e7 years) are not data
    if (!(fabsf(x) < 1.0e15f)) return cosf(x);
    const double xd = (double)x;
    const double kd = rint(xd * 0.63661977236758134308);
    double r = fma(-kd, 1.57079632679489655800e+00, xd);
    r = fma(-kd, 6.12323399573676603587e-17, r);
    return time_cos_poly((float)r, (int)((long long)kd & 3ll));   // |k| < 6.4e14: the quadrant from 64 bits
}

// the |x| < 4e6 formula of time_cosf alone (callers check the range themselves)
__device__ __forceinline__ float time_cosf_fast(float x)
{
    const float kf = rintf(x * 0.636619772f);
    float r = fmaf(kf, -1.57079637e+00f, x);
    r = fmaf(kf, 4.37113883e-08f, r);
    // quarter revolutions of the quadrant: fract(k / 4) = (k & 3) / 4, also for negative k
    return __builtin_amdgcn_cosf(fmaf(r, 0.159154943f, __builtin_amdgcn_fractf(kf * 0.25f)));
}

__device__ __forceinline__ float time_cosf(float x)
{
    if (fabsf(x) >= 4.0e6f) return time_cosf_large(x);
    const float kf = rintf(x * 0.636619772f);
    float r = fmaf(kf, -1.57079637e+00f, x);            // pi/2 = 1.57079637 - 4.37113883e-08 - 1.7e-15 (floats);
    r = fmaf(kf, 4.37113883e-08f, r);                   // the third term is < 5e-9 for |k| < 2.6e6
    // |r| <= pi/4 exactly reduced; the quadrant goes back in as quarter revolutions and v_cos_f32
    // (argument in revolutions) finishes: 9 instructions, max |err| 3e-7 over |x| < 4e6 (measured
    // against float64 cos on 4M arguments: a round-2 microbenchmark)
    const int q = (int)kf & 3;
    return __builtin_amdgcn_cosf(fmaf(r, 0.159154943f, 0.25f * (float)q));
}

// (aggregate.hip, aggregate_wide.hip: the time encoding computed in the MFMA operand lanes)
__device__ __forceinline__ float time_cosf_rev(float x)
{
    // cos(x) for |x| up to 3e8 (dt is seconds: 10 years) in SIX float32 instructions -- on this chip an f32 MFMA and
    // vector instructions of the same SIMD do not overlap, so every vector instruction beside the MFMAs costs its
    // full issue time (float64 ones twice that).  Revolutions x / 2pi with 1 / 2pi = c1 + c2 (two floats): the
    // product x c1 and its rounding error (one FMA) are carried separately, so the FRACTION of the large term is
    // exact; x c2 < 2 needs no such care.  rev = fract(x c1) + (err1 + x c2), then v_cos_f32 (argument in
    // revolutions).  max |error| 9e-7 over |x| <= 3e8 (mean 7e-8): tools/exp/cos_rev_check.py.
    const float c1 = 0x1.45f306p-3f, c2 = 0x1.b9391p-28f;
    const float p1 = x * c1, e1 = fmaf(x, c1, -p1);
    return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(p1) + fmaf(x, c2, e1));
}

// Training dropout of the hidden layer (nn.Dropout(0.1) between fc1's ReLU and fc2, modules/embedding_module.py:89,
// 323-326): the keep-mask of element idx = (gathered row) * D + column is a hash of (seed, idx), so the backward
// kernel regenerates it instead of reading it back.  thr = p * 2^32; returns 1 / (1 - p) for a kept element, else 0.
// (zebra_amd/modules.py: dropout_mask is the same arithmetic in numpy, for the tests.)
__device__ __forceinline__ float drop_scale(unsigned seed_lo, unsigned seed_hi, unsigned thr, float inv_keep,
                                            unsigned long long idx)
{
    unsigned h = ((unsigned)idx * 0x9E3779B1u) ^ seed_lo;
    h ^= ((unsigned)(idx >> 32) * 0x85EBCA77u) + seed_hi;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;      // murmur3 finaliser
    return h >= thr ? inv_keep : 0.f;
}

// floor(f / d) for small f via a precomputed multiplier m = fastdiv_magic(d); exact for f*d < 2^32.
__device__ __forceinline__ unsigned fastdiv_magic(unsigned d) { return d <= 1u ? 0u : 0xFFFFFFFFu / d + 1u; }   // 0 = divide by 1
__device__ __forceinline__ int fastdiv(int f, unsigned m) { return m == 0u ? f : (int)__umulhi((unsigned)f, m); }

#endif  // __HIPCC__

}  // namespace zt
