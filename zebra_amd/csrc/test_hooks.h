/* Test hooks: libzebra_amd_testhooks.so (zebra_amd/csrc/test_hooks.hip), built beside the product library and loaded
 * by the tests only.  Nothing here is part of the product ABI (include/zebra_amd.h). */
#ifndef ZEBRA_AMD_TEST_HOOKS_H
#define ZEBRA_AMD_TEST_HOOKS_H
#include "../../include/zebra_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Test hook (not product API): the exact top-k selection primitive on its    */
/* own.  vals [cases][n] float64; writes np.argsort(vals[c])[-k:] under       */
/* numba's quicksort semantics into sel_out [cases][k] and the path taken     */
/* (0 fast rank, 1 wave-parallel exact in LDS, 2 sequential exact, 3 exact in  */
/* registers on values, 4 exact in registers on ranks) into path_out.          */
/* mode: 0 = production dispatch, 1/2/3/4 = force that path, 5 / 6 = the        */
/* register-resident selection of the merge (one candidate per lane, adjacent  */
/* lanes / split over the two wave halves; n <= 63, k <= 31).                  */
/* ------------------------------------------------------------------------ */
int zt_test_topk(const double *vals_dev, int32_t n, int32_t k, int32_t cases,
                 int32_t mode, int32_t *sel_out_dev, int32_t *path_out_dev,
                 void *stream);
/* Test hook: set the T-PPR handle's launch epoch (the row tags' high bits), to
 * exercise the wrap-around (all tags are cleared when it reaches 2^18 - 1). */
int zt_test_set_epoch(zt_tppr *h, uint32_t epoch);
/* Test hook: the dependency plan zt_tppr_plan made last, copied to host arrays -- wo / pflag / hv [n_roles * B] (B = the
 * planned launch's edges), owner_of [B], chain_node / chain_len [16], chain_edges [16][2048], *n_chains. */
int zt_test_tppr_plan_dump(zt_tppr *h, int32_t *wo, int32_t *pflag, int32_t *hv, int32_t *owner_of, int32_t *chain_node,
                           int32_t *chain_len, int32_t *chain_edges, int32_t *n_chains);
/* Test hook: the embedding's kernel choice for one shape (zt::embed_kernel_plan, host code only): *agg_out = 0 unsupported,
 * 1 reg, 2 wide, 3 d100, 4 tiled table, 5 tiled full, 6 / 7 the same two with the big tile, 8 row split; *out_out = 0 tiled,
 * 1 latency, 2 persist (the output layers); *lds_out = the tiled / d100 launch's dynamic LDS.  training: zt_agg_train_forward's
 * choice; agg_choice / out_choice: the ZT_CHOICE_AGGREGATE / ZT_CHOICE_EMBED_OUT selections. */
int zt_test_embed_plan(int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k, int32_t have_table, int32_t training,
                       int32_t agg_choice, int32_t out_choice, int32_t *agg_out, int32_t *out_out, int64_t *lds_out);
/* Test hook: the memory update's kernel choice for one shape (zt::memory_kernel_plan, host code only).  The held-back output
 * layers: held (0 / 1), out_form (0 tiled, 1 latency, 2 persist, 3 the persistent form's neighbour half), hg, out_D, out_M, gx, out_N, same_memory.  out[14] =
 * refusal (0 none, 1 bad argument, 2 D > 128, 3 message width), message kernel (0 one, 1 two positions per wave), GRU form
 * (0 none, 1 tile, 2 split), output layers (0 none, 1 in front, 2 fused with the tile, 3 fused with the split, 4 the neighbour half behind the
 * tile's workgroups), lds, lds2,
 * lds_f, gru_tiles, NTg, n_src_wgs, n_nb_wgs, out_tiles, target, participants. */
int zt_test_memory_plan(int64_t max_rows, int32_t D, int32_t msg_dim, int32_t F, int32_t T, int32_t gru_choice,
                        int32_t msg_choice, int32_t held, int32_t out_form, int32_t hg, int32_t out_D, int32_t out_M,
                        int32_t gx, int64_t out_N, int32_t same_memory, int64_t *out);
/* Test hook: the eval link scorer's kernel for one batch (zt::affinity_kernel_plan, host code only).  choice: the
 * ZT_CHOICE_SCORE selection.  out[7] = form (0 refused, 1 latency, 2 tiled, 3 generic latency, 4 generic tiled: the ZT_SCORE_*
 * values), KC, ET (the specialised forms' template arguments, else 0), grid x, grid y, threads per workgroup, dynamic LDS. */
int zt_test_affinity_plan(int64_t B, int32_t H, int32_t choice, int64_t *out);
/* Test hook: the attention layer's tile for one shape (zt::attention_plan, host code only).  out[4] = supported (0 / 1), rq (query
 * rows per workgroup), mt (16-row M-tiles of key rows), dynamic LDS bytes; the last three are 0 where the shape is refused. */
int zt_test_attention_plan(int32_t D, int32_t F, int32_t T, int32_t n_head, int32_t hidden, int32_t out_dim, int32_t k,
                           int64_t *out);
/* Test hook: one pipeline step's choices (zt::pipeline_step_plan, host code only).  The facts, 0 / 1 unless said otherwise:
 * streaming (else pruning), masked, release (the ZT_CHOICE_GROUP_RELEASE value), B, row_lo, row_hi, scoring, metrics, exchange,
 * avg_topk, proj_table (each: attached), wm_ready (the padded W_m is in the embed workspace); the current member's slot:
 * by_member, its tail_gated bit, waited; the batch that follows: have_next, next_B, next_in_slot, and that slot's by_member,
 * launched, waited and the member's tail_gated bit.  out[12] = gate form (0 carried by the previous GRU kernel, 1 the launch's
 * event, 2 a kernel in front, 3 offered to the aggregation kernel), wait for `filled` first, wait for the launch's event,
 * shard gather, k_avg_topk, scored, measured, the GRU update is the main stream's last item, the tail gate is offered for the
 * next member, that needs the next slot's `filled`, late zt_project_memory, exchange. */
int zt_test_step_plan(int32_t streaming, int32_t masked, int32_t release, int64_t B, int64_t row_lo, int64_t row_hi,
                      int32_t scoring, int32_t metrics, int32_t exchange, int32_t avg_topk, int32_t proj_table, int32_t wm_ready,
                      int32_t by_member, int32_t tail_gated, int32_t waited, int32_t have_next, int64_t next_B,
                      int32_t next_in_slot, int32_t next_by_member, int32_t next_launched, int32_t next_waited,
                      int32_t next_tail_gated, int64_t *out);
/* Test hook: a launch group's release and size limit (zt::pipeline_group_plan).  want: zt_pipeline_set_group; n_more: batches
 * in sight behind the first.  out[2] = released by member (before "and more than one member"), batches it may take. */
int zt_test_group_plan(int32_t streaming, int32_t release, int32_t want, int32_t n_more, int64_t *out);
/* Test hook: pin the node decoder's arrangement process-wide (zt::decoder_plan: 0 = the plan's pick, 1 = one wave per 16 rows,
 * 5 = five waves per 16 rows); zt_node_decoder_plan answers under the pin.  ZT_ERR_ARG for any other value. */
int zt_test_decoder_arrangement(int32_t value);
/* Test hook: whether a caller that can hold output layers back (the pipeline) gets the persistent form divided for this shape
 * (zt::embed_kernel_plan's nbr_later, host code only): the source path launched by itself, the neighbour paths handed on to the
 * GRU update's launch (k_nbr_gru).  out_choice: the ZT_CHOICE_EMBED_OUT selection.  *divided_out = 0 / 1. */
int zt_test_embed_divided(int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k, int32_t have_table,
                          int32_t out_choice, int32_t *divided_out);
/* Test hook: the two calls of a pipeline step without the pipeline -- zt_embed with its output layers held back (zt::embed_ex),
 * then the memory update that takes them along (zt::gru_update_ex) -- under the process's ZT_CHOICE_EMBED_OUT / ZT_CHOICE_GRU.
 * The first arguments are zt_embed's, the rest zt_gru_update's (cell: ZT_CELL_GRU / ZT_CELL_RNN), except that the rows to
 * update are the caller's list: their count in gru_ws's first word, the ids at zt_gru_rows_offset, at most max_rows.
 * max_wgs: the divided persistent form's launches take at most so many persistent workgroups each (0 = one per compute unit
 * of the stream), so that a small grid's seams -- fewer units than striding waves, as many, one more -- sit at a test's sizes.
 * *out_launch = what became of the held-back layers (zt_test_memory_plan's values; 4 = behind the GRU tiles, k_nbr_gru). */
int zt_test_embed_gru(float *memory_dev, const float *efeat_dev, int64_t num_nodes, int64_t num_edges, int32_t D, int32_t F,
                      int32_t T, const int32_t *nodes_dev, int64_t N, int32_t M, int32_t k, const int32_t *nbr_dev,
                      const int32_t *eix_dev, const float *dt_dev, const float *w_dev, const zt_embed_weights *ew,
                      float *out_dev, void *embed_ws, int32_t *status_dev, float *proj_table_dev, int32_t embed_ready,
                      float *last_update_dev, const float *messages_dev, const float *msg_ts_dev, uint8_t *flags_dev,
                      int32_t msg_dim, int64_t max_rows, const zt_gru_weights *gw, void *gru_ws, int32_t gru_ready,
                      int32_t cell, int32_t max_wgs, int32_t *out_launch, void *stream);

#ifdef __cplusplus
}
#endif
#endif
