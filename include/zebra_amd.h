/*
 * zebra_amd.h -- C-ABI of libzebra_amd.so, the MI355X (gfx950) implementation
 * of Zebra's T-PPR + top-k aggregate + memory-update hot path.
 *
 * The reference has no FFI: its boundary is a set of Python attribute calls
 * (SURVEY.md section 8b).  Each entry point below names the reference method
 * it replaces (paths relative to the reference checkout).  The Python classes
 * in zebra_amd/ (tppr_finder, NeighborFinder, GraphDiffusionEmbedding, Memory,
 * GRUMemoryUpdater, TGN) bind these with ctypes; INTEGRATION.md shows the stub
 * a reference maintainer would add.
 *
 * Conventions
 *   - every function returns an int status (ZT_OK == 0) and never throws;
 *   - "dev" pointers are device (HBM) addresses, "host" pointers host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued on it and is stream-ordered; the library is not
 *     thread-safe per handle (the reference holds the GIL throughout);
 *   - node ids and edge ids are validated on the device: an out-of-range id
 *     rejects the whole call BEFORE any state is modified and latches
 *     ZT_ERR_RANGE in the handle's status word (zt_tppr_status / the status
 *     out-parameter), because the reference's Numba code would read out of
 *     bounds there (SURVEY.md 8b "Errors").
 */
#ifndef ZEBRA_AMD_H
#define ZEBRA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZT_OK 0
#define ZT_ERR_ARG (-1)         /* bad argument (NULL, non-positive size, k > ZT_MAX_K ...) */
#define ZT_ERR_RANGE (-2)       /* node / edge id out of range */
#define ZT_ERR_HIP (-3)         /* a HIP runtime call failed (see zt_last_error) */
#define ZT_ERR_UNSUPPORTED (-4) /* shape outside what the kernels were built for */
#define ZT_ERR_TIMEOUT (-5)     /* an in-kernel dependency wait hit its spin bound */

#define ZT_MAX_K 63             /* top-k width of the tuned paths: one dictionary entry per lane of a wavefront (streaming update with
                                 * hub chains, pruning query) */
#define ZT_MAX_K_WIDE 255       /* streaming T-PPR accepts k up to here (the reference's --topk is unbounded, train.py:46): beyond
                                 * ZT_MAX_K a correct-first path takes over -- one wavefront per model applies the edges in order
                                 * (csrc/tppr_wide.hpp), same state layout, same results as the oracle bit for bit, not tuned.  zt_embed
                                 * takes such rows through the generic kernel's 16-tile instantiation where a query row's tile fits LDS,
                                 * and through the row-split kernel (the row's neighbours in chunks of 80, csrc/aggregate_split.hip)
                                 * where none does; the training kernels any k up to here (the same row split beyond 80); the
                                 * pruning query any k up to here (its kept set strides over the lanes; the selection beyond
                                 * ZT_MAX_K is the generic replay of numba_sort.hpp) */

/* Human-readable description of the last failure on this thread. */
const char *zt_last_error(void);
/* Library / build information ("zebra_amd <version> gfx950"). */
const char *zt_version(void);

/* HIP streams restricted to the compute units [cu_lo, cu_hi) (CU masking):
 * the dependency-bound T-PPR kernel and the throughput-bound aggregation can
 * then run side by side without sharing CUs.  New work; the reference is
 * single-stream (train.py:145-146). */
int zt_stream_create_masked(void **stream_out, int32_t cu_lo, int32_t cu_hi);
int zt_stream_destroy(void *stream);

/* Kernel selection, for VALIDATION.  Several steps of the path have more than one kernel -- a latency-organised
 * one for small batches, a throughput-organised one for large ones, a generic one for shapes outside the reference's
 * default widths (train.py:33-36) -- and the library picks by shape.  zt_set_kernel_choice pins the pick process-wide
 * (value 0 = the library's choice again) so that tests can hold the kernels against each other, and against the
 * oracle, on the same inputs.  A pinned kernel that cannot take a shape falls back to the library's pick.  Not a
 * tuning interface: every kernel of a selector computes the same function. */
#define ZT_CHOICE_AGGREGATE 0   /* neighbour aggregation (zt_embed): ZT_AGG_GENERIC */
#define ZT_CHOICE_EMBED_OUT 1   /* output layers (zt_embed): ZT_OUT_TILED, ZT_OUT_LATENCY, ZT_OUT_PERSIST; zt_pipeline_*: also
                                 * ZT_OUT_NBR_GRU, ZT_OUT_WHOLE */
#define ZT_CHOICE_GRU 2         /* zt_gru_update: ZT_GRU_TILE, ZT_GRU_SPLIT */
#define ZT_CHOICE_MESSAGES 3    /* zt_store_messages: ZT_MSG_ONE, ZT_MSG_TWO (batch positions per wavefront) */
#define ZT_CHOICE_TPPR_CHAIN 4  /* hub chains of zt_tppr_stream: ZT_CHAIN_SINGLE (one position per critical section: the
                                 * library's one mode).  ZT_CHAIN_PAIRED / _SPINE / _DUO were built, bit-exact and measured
                                 * SLOWER, and were removed: the library answers ZT_ERR_UNSUPPORTED */
#define ZT_CHOICE_TPPR_PREPASS 5 /* dependency prepass of a launch of more than 4 096 accesses: ZT_PREPASS_LAUNCHES (one kernel per step,
                                 * eleven launches: the library's one form); ZT_PREPASS_COOP (one cooperative kernel with grid
                                 * barriers: not faster) was removed likewise */
#define ZT_CHOICE_GROUP_RELEASE 6 /* zt_pipeline_*: when the aggregation of a batch may start whose streaming T-PPR update shares a launch
                                 * with other batches.  ZT_RELEASE_MEMBER: as soon as that batch's rows are written (a counter per batch
                                 * inside the launch: the library's pick); ZT_RELEASE_LAUNCH: when the whole launch has ended (an event;
                                 * launch groups then taper towards the end of the batches in sight); ZT_RELEASE_LAUNCH_FULL: the
                                 * same without the taper (uniform launches for counter collection, which serialises kernels and so
                                 * cannot run a release by member: tools/profile_round.sh) */
#define ZT_CHOICE_SCORE 7       /* zt_affinity and the pipeline's scoring: ZT_SCORE_LATENCY, ZT_SCORE_TILED (the kernels specialised for
                                 * hidden widths 200 and 300; at any other width: the library's pick), ZT_SCORE_GENERIC_LATENCY,
                                 * ZT_SCORE_GENERIC_TILED (any width zt_affinity takes, 200 and 300 included) */
#define ZT_CHOICE_COUNT 8
#define ZT_AGG_GENERIC 1
#define ZT_OUT_TILED 1
#define ZT_OUT_LATENCY 2
#define ZT_OUT_PERSIST 3
#define ZT_OUT_NBR_GRU 4   /* the persistent form, and in the pipeline its neighbour paths run in the GRU update's grid (k_nbr_gru)
                            * behind a source-only launch, at any batch size: what the library picks by itself from 8 192 rows
                            * on.  (ZT_OUT_PERSIST: the persistent form whole, k_embed_out3, in the pipeline too) */
#define ZT_OUT_WHOLE 5     /* the library's pick by shape, but the output layers are never divided between two launches: the
                            * persistent form runs whole (k_embed_out3) in front of the GRU update */
#define ZT_GRU_TILE 1
#define ZT_GRU_SPLIT 2
#define ZT_CHAIN_SINGLE 1
#define ZT_CHAIN_PAIRED 2  /* removed; see DESIGN.md section 5 (two chain positions per critical section) */
#define ZT_CHAIN_SPINE 3   /* removed; see DESIGN.md section 5 (one wave per chain runs every critical section) */
#define ZT_CHAIN_DUO 4     /* removed; see DESIGN.md section 5 (spine mode with the weights on a wave of their own) */
#define ZT_PREPASS_LAUNCHES 1
#define ZT_PREPASS_COOP 2  /* removed; see DESIGN.md section 5 */
#define ZT_RELEASE_MEMBER 1
#define ZT_RELEASE_LAUNCH 2
#define ZT_RELEASE_LAUNCH_FULL 3
#define ZT_RELEASE_MEMBER_FRONT 4 /* by member, every batch's gate in front of its own step (the library's pick lets the GRU kernel of the
                                  * step before carry it where that kernel is the step's last: pipeline.hip) */
#define ZT_MSG_ONE 1
#define ZT_MSG_TWO 2
#define ZT_SCORE_LATENCY 1
#define ZT_SCORE_TILED 2
#define ZT_SCORE_GENERIC_LATENCY 3
#define ZT_SCORE_GENERIC_TILED 4
int zt_set_kernel_choice(int32_t which, int32_t value);

/* Per-kernel timing with HIP events recorded on the launch stream (replaces
 * the reference's unsynchronised wall-clock accumulators t_tppr etc.,
 * modules/embedding_module.py:73,220-225).  Names: tppr_prepass, tppr_stream,
 * tppr_cleanup, pruned_topk, embed_prep, fc1_agg, embed_out, store_messages,
 * gru_update.  zt_profile_enable(n): 0 off, 1 every launch, n > 1 every n-th
 * launch of each kernel (sampling).  zt_profile_read synchronises the device. */
int zt_profile_enable(int on);
int zt_profile_reset(void);
int zt_profile_read(const char *name, int64_t *count, double *total_ms);

/* ------------------------------------------------------------------------ */
/* Streaming T-PPR  --  utils/util.py:391-873 (class tppr_finder)            */
/* ------------------------------------------------------------------------ */

typedef struct zt_tppr zt_tppr;

/* tppr_finder.__init__ (utils/util.py:393-400): allocates the device-resident
 * state [n_tppr][num_nodes][k] (key, timestamp, weight) + length + normaliser,
 * all zero.  alpha/beta are host arrays of n_tppr doubles. */
int zt_tppr_create(zt_tppr **out, int64_t num_nodes, int32_t k, int32_t n_tppr,
                   const double *alpha_host, const double *beta_host);
int zt_tppr_destroy(zt_tppr *h);
/* Processes whose T-PPR update kernels share this device's compute units (default 1: the device is this
 * process's own -- one rank per GPU, the supported multi-GPU layout).  n > 1 (several ranks rehearsing on
 * ONE GPU): every launch takes 1/n of the CUs of its stream, so that the grids of all sharers are resident
 * together, and runs without hub chains, whose workgroups wait for one another.  New work; the reference
 * is one process on one device (train.py:145-146). */
int zt_tppr_set_device_share(zt_tppr *h, int32_t n_processes);
/* Statistics of the hub chains: synchronises `stream` and writes five zeros to out5.  The counters belonged to the
 * paired / spine / duo chain modes, which were removed; the one chain mode keeps no statistics on
 * its hot path.  Kept for its callers.  (The reference applies the edges one by one, utils/util.py:495-574.) */
int zt_tppr_chain_stats(zt_tppr *h, int64_t *out5, void *stream);

/* tppr_finder.reset_tppr (utils/util.py:419-434). */
int zt_tppr_reset(zt_tppr *h, void *stream);

/* Deep snapshot: dst <- src (same shape).  Replaces backup_tppr /
 * restore_tppr / restore_val_tppr (utils/util.py:436-444), which alias the
 * live state in the reference; the Python shim chooses
 * between deep and alias semantics. */
int zt_tppr_copy(zt_tppr *dst, const zt_tppr *src, void *stream);

/* tppr_finder.streaming_topk (utils/util.py:473-576), streaming_topk_no_fake
 * (:682-782), single_streaming_topk (:581-679) and the update loop of
 * compute_val_tppr (:787-870).
 *   nodes_dev : int32 [n_roles*B] = [src | dst | (neg)]
 *   ts_dev    : float64 [B]   (the reference reads only timestamps[:B], :499)
 *   eidx_dev  : int64 [B]
 *   n_roles   : 3 (with negatives) or 2
 *   emit      : 1 = fill the four output arrays, 0 = update only
 *   model     : -1 = all models, else only that one
 *   out_*_dev : [n_emitted_models][n_roles*B][k] int32/int32/float32/float32;
 *               every row is written (zeros when the dictionary is empty).
 *   plan_token: 0, or the token zt_tppr_plan returned for exactly this call.
 * Edges are applied in batch order, each seeing the state left by the edges
 * before it, exactly as the reference's sequential loop.
 * Errors: a batch with an out-of-range id is NOT applied, its output rows read
 * as empty dictionaries (zeros), and ZT_ERR_RANGE is latched in the handle:
 * every later zt_tppr_stream / zt_tppr_plan call returns it (as soon as the
 * device's write is visible to the host; no synchronisation is added) until
 * zt_tppr_status has reported and cleared it.  ZT_ERR_TIMEOUT likewise. */
int zt_tppr_stream(zt_tppr *h, const int32_t *nodes_dev, const double *ts_dev,
                   const int64_t *eidx_dev, int64_t B, int32_t n_roles,
                   int32_t emit, int32_t model, int32_t *out_nodes_dev,
                   int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev,
                   uint64_t plan_token, void *stream);

/* Optional, no reference counterpart: run the dependency prepass of a coming
 * zt_tppr_stream call ahead of time on another stream.  The prepass (which
 * edges of the batch touch the same node, in which order) reads only the ids,
 * never the T-PPR state, so it can overlap the previous call's update kernel.
 * *token_out identifies the plan: the zt_tppr_stream call it was made for
 * passes it back (same nodes_dev, B, n_roles, model; ordering between the two
 * streams is handled inside).  A call with token 0, or with a token whose plan
 * has been dropped (zt_tppr_reset / copy / import, or two newer plans), runs
 * its own prepass.  Two plans can be outstanding.  *token_out = 0 and a no-op
 * for B == 0 or B > 16384 (multi-launch calls plan inline).
 * The k_stream grid is sized for the compute units of the stream that RUNS it
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs of that stream's mask);
 * if that stream turns out to offer fewer CUs than the plan assumed, the grid
 * shrinks and hub chains are dropped for that launch (in-order queue only). */
int zt_tppr_plan(zt_tppr *h, const int32_t *nodes_dev, const int64_t *eidx_dev,
                 int64_t B, int32_t n_roles, int32_t model, uint64_t *token_out,
                 void *stream);

/* Rows of ARBITRARY nodes from the live state, read-only: out_* [n_emitted_models][N][k] -- model as in zt_tppr_stream:
 * -1 every model, else that one (ZT_ERR_ARG outside [-1, n_tppr)).  Row i is what extract_streaming_tppr
 * (utils/util.py:447-469) gives for the dictionary of nodes_dev[i] at current_timestamp = ts_dev[i] (N timestamps, one per
 * row): entries in dictionary order, dt = f32(f64(t) - f64(f32(entry ts))); entries j >= len of a non-empty row read
 * 0, 0, f32(t), 0; an empty row is all zeros -- the bits zt_tppr_stream emits for a negative sample's row.
 * An id outside [0, num_nodes) gives an all-zero row and ZT_ERR_RANGE in *status_dev (may be NULL), as in zt_embed.
 * N = 0: ZT_OK, nothing enqueued; a NULL pointer (status_dev apart) or N < 0: ZT_ERR_ARG before any device call.
 * The call reads the state's rows and NOTHING else of the handle -- no control word, plan, epoch, hub version or status
 * latch is read or written on the device, the handle is not modified on the host; a latched failure of an earlier launch
 * neither fails it nor is cleared by it.
 * CONTRACT: the call is enqueued on a stream ordered after every writer of the state (zt_tppr_stream, zt_tppr_import*,
 * zt_tppr_copy / reset, a pipeline's T-PPR stream), and where a pipeline owns the handle zt_pipeline_outstanding is 0 --
 * batches queried ahead have their updates applied already, the rows would be those of a later time. */
int zt_tppr_query(const zt_tppr *h, const int32_t *nodes_dev, const double *ts_dev, int64_t N, int32_t model,
                  int32_t *out_nodes_dev, int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev,
                  int32_t *status_dev, void *stream);
/* Synchronises `stream` and returns the latched status (ZT_OK, ZT_ERR_RANGE
 * or ZT_ERR_TIMEOUT) of the launches so far, clearing it. */
int zt_tppr_status(zt_tppr *h, void *stream);

/* State of model m to / from host arrays, dictionary items in iteration
 * order (attrs PPR_list / norm_list of the reference, utils/util.py:383-386):
 *   len int32[N], norm float64[N], eidx int64[N*k], node int64[N*k],
 *   ts float64[N*k], w float64[N*k]; slots >= len are zero.  Synchronous. */
int zt_tppr_export(zt_tppr *h, int32_t m, int32_t *len_host, double *norm_host,
                   int64_t *eidx_host, int64_t *node_host, double *ts_host,
                   double *w_host);
/* The same for the n nodes ids_host[0..n) only (outputs [n], [n][k]): what a
 * checkpoint of a 10^7-node graph wants -- only the nodes the stream has touched. */
int zt_tppr_export_rows(zt_tppr *h, int32_t m, const int64_t *ids_host, int64_t n,
                        int32_t *len_host, double *norm_host, int64_t *eidx_host,
                        int64_t *node_host, double *ts_host, double *w_host);
int zt_tppr_import(zt_tppr *h, int32_t m, const int32_t *len_host,
                   const double *norm_host, const int64_t *eidx_host,
                   const int64_t *node_host, const double *ts_host,
                   const double *w_host);
/* The same for the n nodes ids_host[0..n) only (inputs [n], [n][k]); rows of
 * other nodes are left as they are.  With zt_tppr_export_rows: a checkpoint
 * that only holds the nodes the stream has touched. */
int zt_tppr_import_rows(zt_tppr *h, int32_t m, const int64_t *ids_host, int64_t n,
                        const int32_t *len_host, const double *norm_host,
                        const int64_t *eidx_host, const int64_t *node_host,
                        const double *ts_host, const double *w_host);

/* ------------------------------------------------------------------------ */
/* Static adjacency + pruning T-PPR -- utils/util.py:90-276                  */
/* ------------------------------------------------------------------------ */

typedef struct zt_csr zt_csr;

/* get_neighbor_finder (utils/util.py:90-107): host edge arrays -> device CSR
 * (indptr int64[N+1], nbr int32[2E], eid int32[2E], ts float64[2E]); each
 * node's entries stably sorted by timestamp. */
int zt_csr_build(zt_csr **out, const int32_t *src_host, const int32_t *dst_host,
                 const int64_t *eidx_host, const double *ts_host, int64_t E,
                 int64_t num_nodes);
/* NeighborFinder(node_to_neighbors, node_to_edge_idxs, node_to_edge_timestamps)
 * (utils/util.py:146-149): adopt an adjacency that is already grouped by node
 * and time-sorted (host CSR arrays). */
int zt_csr_from_sorted(zt_csr **out, const int64_t *indptr_host, const int32_t *nbr_host,
                       const int32_t *eid_host, const double *ts_host, int64_t num_nodes);
int zt_csr_destroy(zt_csr *c);
/* Sizes and a host copy of the adjacency (attrs node_to_neighbors, ... of the
 * reference object). */
int zt_csr_size(const zt_csr *c, int64_t *num_nodes, int64_t *num_entries);
int zt_csr_export(const zt_csr *c, int64_t *indptr_host, int32_t *nbr_host, int32_t *eid_host,
                  double *ts_host);
/* NeighborFinder.find_before (utils/util.py:152-154) for one node: number of
 * entries strictly before t, and copies of that prefix (host, optional). */
int zt_csr_find_before(const zt_csr *c, int32_t v, double t, int64_t *count,
                       int32_t *nbr_host, int32_t *eid_host, double *ts_host,
                       int64_t cap);

/* The pruning query has two forms (the reference bounds neither --n_degree nor
 * --n_layer, train.py:25,28; a walk emits width + width^2 + ... + width^depth
 * states per query):
 *   lds        the candidate list and the frontier of a query live in LDS, one
 *              wavefront per query: up to 1280 states and a frontier
 *              (width^(depth-1)) of up to 512 entries.  Needs no preparation.
 *   workspace  the same arrays live in a slab of device memory that the CSR
 *              handle holds (zt_csr_reserve_pruning): up to
 *              ZT_PRUNE_WS_MAX_STATES states.  One workgroup per slab takes
 *              queries worker, worker + grid, ...
 * Both are bit-identical to the reference.  zt_prune_plan is where the form is
 * decided (host code only, no GPU call); the query entry points and the
 * reservation go through it. */
#define ZT_PRUNE_FORM_REFUSED 0
#define ZT_PRUNE_FORM_LDS 1
#define ZT_PRUNE_FORM_WORKSPACE 2
#define ZT_PRUNE_WS_MAX_STATES (1 << 18) /* sum_{d<=depth} width^d of the workspace form (50 x 3 = 127 550, 10 x 5 = 111 110) */
#define ZT_PRUNE_WS_MAX_SLABS 768        /* slabs of one reservation: what an MI355X keeps resident -- 256 compute units x 3
                                          * workgroups of 256 threads (the kernel's 140 vector registers: 3 waves per SIMD) */
#define ZT_PRUNE_PLAN_FIELDS 10
/* out[ZT_PRUNE_PLAN_FIELDS], all int64:
 *   [0] form               ZT_PRUNE_FORM_*
 *   [1] cap_c              states a query may emit: sum width^d (saturated at ZT_PRUNE_WS_MAX_STATES + 1 when refused for it)
 *   [2] cap_f              widest frontier: width^(depth-1)
 *   [3] models per launch  more models run as several launches
 *   [4] slab_bytes         workspace: bytes of one slab (0 for lds)
 *   [5] slabs              workspace: min(max_bytes / slab_bytes, ZT_PRUNE_WS_MAX_SLABS); 0 -> refused
 *   [6] grid               workspace: workgroups of a launch at most (= slabs; a launch takes min(queries, slabs));
 *                          lds: 0 (a launch takes ceil(queries / 4))
 *   [7] threads            per workgroup
 *   [8] lds_bytes          per workgroup (lds: dynamic; workspace: static)
 *   [9] states             = [1]
 * ZT_ERR_ARG for non-positive width / depth / n_models / k, a negative max_bytes or NULL out; else ZT_OK -- a refused form
 * is an answer, not a failure (zt_last_error says why). */
int zt_prune_plan(int32_t width, int32_t depth, int32_t n_models, int32_t k, int64_t max_bytes, int64_t *out);
/* Plans the workspace form for (width, depth, n_models, k) and allocates slabs x slab_bytes of device memory on the handle
 * (slabs: as many as fit max_bytes, at most ZT_PRUNE_WS_MAX_SLABS).  A later call replaces the reservation.  A shape the
 * lds form takes reserves nothing (an earlier reservation stays) and returns ZT_OK.  ZT_ERR_UNSUPPORTED: max_bytes below
 * one slab (the message names the bytes one slab needs), or a shape beyond ZT_PRUNE_WS_MAX_STATES.  A reservation covers
 * every query whose cap_c and cap_f are within the reserved ones, at any k and any number of models (more models than it
 * was planned for run as several launches).  The workspace serves one launch at a time: a launch records an event on its
 * stream and the next launch, if on another stream, waits for it on the device -- no host synchronisation and no
 * allocation inside a query call.  Calls on one handle are not thread-safe against each other. */
int zt_csr_reserve_pruning(zt_csr *c, int32_t width, int32_t depth, int32_t n_models, int32_t k, int64_t max_bytes);
/* Frees the reservation (after the launches that use it); zt_csr_destroy does so too. */
int zt_csr_release_pruning(zt_csr *c);

/* NeighborFinder.get_pruned_topk (utils/util.py:185-276): rows whose
 * dictionary is empty are left untouched, all others fully written (the
 * reference mutates caller-owned arrays in place).  A shape beyond the lds
 * form needs a reservation that covers it on the handle, else
 * ZT_ERR_UNSUPPORTED. */
int zt_pruned_topk(const zt_csr *c, const int32_t *q_nodes_dev,
                   const double *q_ts_dev, int64_t nq, int32_t width,
                   int32_t depth, double alpha, double beta, int32_t k,
                   int32_t *out_nodes_dev, int32_t *out_eidx_dev,
                   float *out_dt_dev, float *out_w_dev, int32_t *status_dev,
                   void *stream);
/* GraphDiffusionEmbedding.pruning_topk (modules/embedding_module.py:280-297):
 * the same query for every (alpha, beta) model of the ensemble in ONE walk of
 * the adjacency -- which states a query reaches depends on (node, time) only,
 * the models differ in the weights they carry along.  alpha_host / beta_host:
 * n_models host doubles; outputs are [n_models][nq][k], model-major, and follow
 * the same "empty rows stay untouched" rule. */
int zt_pruned_topk_multi(const zt_csr *c, const int32_t *q_nodes_dev,
                         const double *q_ts_dev, int64_t nq, int32_t width,
                         int32_t depth, int32_t n_models, const double *alpha_host,
                         const double *beta_host, int32_t k, int32_t *out_nodes_dev,
                         int32_t *out_eidx_dev, float *out_dt_dev, float *out_w_dev,
                         int32_t *status_dev, void *stream);

/* ------------------------------------------------------------------------ */
/* Gather + TimeEncode + transform + weighted sum                            */
/*   GraphDiffusionEmbedding.compute_embedding_tppr_ensemble, eval forward   */
/*   (modules/embedding_module.py:243-276, 320-328; model/time_encoding.py)  */
/* ------------------------------------------------------------------------ */

typedef struct {
    const float *fc1_w, *fc1_b;   /* [D][D+F+T], [D]   torch Linear layout */
    const float *fc2_w, *fc2_b;   /* [D][D], [D] */
    const float *fc1s_w, *fc1s_b; /* transform_source */
    const float *fc2s_w, *fc2s_b;
    const float *time_w;          /* TimeEncode frequencies [T] */
} zt_embed_weights;               /* all device pointers */

/*   memory_dev [num_nodes][D], efeat_dev [num_edges][F]
 *   nodes_dev int32[N]; nbr/eix int32 [M][N][k]; dt/w float32 [M][N][k]
 *   out_dev [N][D*(M+1)] = [transform_source(memory[nodes]) | model 0 | ...]
 *   workspace_dev: at least zt_embed_workspace_bytes(N, D, F, T, M, k) bytes
 *   (-1 = shape unsupported). */
int64_t zt_embed_workspace_bytes(int64_t N, int32_t D, int32_t F, int32_t T,
                                 int32_t M, int32_t k);
/*   weights_ready: 0 = pad the weight matrices into the workspace first (needed
 *   once per weight change); 1 = the workspace already holds them (same
 *   workspace, same shape, unchanged weights).
 *   proj_table_dev: NULL, or the projected memory table of zt_project_memory for
 *   memory_dev (see below): fc1's memory columns are then taken from it. */
int zt_embed(const float *memory_dev, const float *efeat_dev, int64_t num_nodes,
             int64_t num_edges, int32_t D, int32_t F, int32_t T,
             const int32_t *nodes_dev, int64_t N, int32_t M, int32_t k,
             const int32_t *nbr_dev, const int32_t *eix_dev, const float *dt_dev,
             const float *w_dev, const zt_embed_weights *weights, float *out_dev,
             void *workspace_dev, int32_t *status_dev, const float *proj_table_dev,
             int32_t weights_ready, void *stream);

/* Projected memory table (no reference counterpart; an algebraic rewrite of
 * modules/embedding_module.py:264-265).  fc1 is linear, so
 *   fc1([memory[nbr] | edge | time]) = W_m memory[nbr] + W_e edge + W_t time + b,
 * and W_m memory[v] depends on the NODE only: P[v] = W_m memory[v] is kept in a
 * table [num_nodes][round_up(D,16)] (zt_project_table_bytes) and refreshed for
 * the <= 2B rows a batch rewrites instead of being recomputed for the 3B*k*M
 * gathered neighbour rows.  rows_dev == NULL: every node (after the memory or
 * the weights changed wholesale); else the rows listed (ids < 0 and entries
 * beyond *count_dev, if given, are skipped).  workspace_dev / ws_N / ws_M / ws_k:
 * the zt_embed workspace (and the N, M, k it was sized for) that holds the
 * padded weights. */
int64_t zt_project_table_bytes(int64_t num_nodes, int32_t D);
int zt_project_memory(const float *memory_dev, int64_t num_nodes, int32_t D,
                      int32_t F, int32_t T, const zt_embed_weights *weights,
                      int32_t weights_ready, const int32_t *rows_dev,
                      const int32_t *count_dev, int64_t max_rows, float *table_dev,
                      void *workspace_dev, int64_t ws_N, int32_t ws_M, int32_t ws_k,
                      void *stream);

/* Training path of the same aggregation: modules/embedding_module.py:227-276 with
 * train=True.  The reference clones the whole memory table per batch (modules/memory_updater.py:79) and lets
 * autograd walk an [N,k,2D+F] tensor; here the lazily updated rows are a compact overlay
 * (row_map_dev[v] = overlay row of node v or -1; NULL = no overlay) and the backward is one fused kernel.
 *   forward : H_dev [M][N][D] = sum_k w_k/sum(w) relu(fc1([memory'[nbr] | ef | cos])), S_dev [M][N] = (sum w != 0)
 *   backward: from dH_dev [M][N][D] ACCUMULATES (+=) dW1_dev [D][D+F+T], db1_dev [D] and d_overlay_dev [U][D]
 *             (the gradient wrt the overlay rows; stored memory rows carry none)
 * fc2 and transform_source act on [N, D] matrices and stay plain GEMMs outside.
 * drop_p > 0: the reference's training dropout of the hidden layer (nn.Dropout(0.1) between fc1's ReLU and fc2,
 *   modules/embedding_module.py:89,323-326) inside the kernels: the keep-mask is a hash of (drop_seed, element),
 *   regenerated by the backward from the same seed -- pass the forward's values.
 * Shapes: D <= 128 or a multiple of 4 up to 256, k <= ZT_MAX_K_WIDE.  A query row of up to 80 neighbours is one tile of the fused kernels; a wider one
 *   is split into chunks of neighbours (forward: one workgroup per query row walks its chunks, H the same from run to run;
 *   backward: one tile per chunk), so F = 172 trains at any k up to ZT_MAX_K_WIDE as well.
 * workspaces: zt_embed_workspace_bytes(N, ...) / zt_agg_backward_workspace_bytes(D, F, T). */
int zt_agg_train_forward(const float *memory_dev, const float *overlay_dev, const int32_t *row_map_dev,
                         const float *efeat_dev, int64_t num_nodes, int64_t num_edges, int32_t D,
                         int32_t F, int32_t T, int64_t N, int32_t M, int32_t k, const int32_t *nbr_dev,
                         const int32_t *eix_dev, const float *dt_dev, const float *w_dev,
                         const zt_embed_weights *weights, float *H_dev, float *S_dev,
                         void *workspace_dev, int32_t *status_dev, float drop_p, uint64_t drop_seed,
                         void *stream);
int64_t zt_agg_backward_workspace_bytes(int32_t D, int32_t F, int32_t T);
/* 1 if zt_agg_train_forward and zt_agg_train_backward both take (N, D, F, T, M, k), else 0: the fused training path
 * where the library has kernels for the shape, the caller's own composition elsewhere. */
int32_t zt_agg_train_supported(int64_t N, int32_t D, int32_t F, int32_t T, int32_t M, int32_t k);
int zt_agg_train_backward(const float *memory_dev, const float *overlay_dev, const int32_t *row_map_dev,
                          const float *efeat_dev, const float *time_w_dev, int64_t num_nodes,
                          int64_t num_edges, int32_t D, int32_t F, int32_t T, int64_t N, int32_t M,
                          int32_t k, const int32_t *nbr_dev, const int32_t *eix_dev, const float *dt_dev,
                          const float *w_dev, const float *fc1_w_dev, const float *fc1_b_dev,
                          const float *dH_dev, float *dW1_dev, float *db1_dev, float *d_overlay_dev,
                          void *workspace_dev, float drop_p, uint64_t drop_seed, void *stream);

/* ------------------------------------------------------------------------ */
/* Memory: last-message store + GRU update                                   */
/* ------------------------------------------------------------------------ */

/* TGN.get_raw_messages + Memory.store_raw_messages (model/tgn_model.py:204-226,
 * modules/memory.py:27-30).  "Last message wins" over the 2B sequence
 * [src|dst]; overwrites messages[node], msg_ts[node], sets flags[node] = 1.
 *   scratch_dev: int32[num_nodes], all -1 on entry and restored to -1 on exit.
 *   uniq_ids_dev (optional): receives the unique endpoint ids, *n_uniq_dev
 *   their count (order unspecified). */
int zt_store_messages(const float *memory_dev, const float *last_update_dev,
                      const float *efeat_dev, const float *time_w_dev,
                      int64_t num_nodes, int64_t num_edges, int32_t D, int32_t F,
                      int32_t T, const int32_t *src_dev, const int32_t *dst_dev,
                      const double *ts_dev, const int64_t *eidx_dev, int64_t B,
                      float *messages_dev, float *msg_ts_dev, uint8_t *flags_dev,
                      int32_t *scratch_dev, int32_t *uniq_ids_dev,
                      int32_t *n_uniq_dev, int32_t *status_dev, void *stream);

/* Same, but only the winners whose batch position lies in [pos_lo, pos_hi)
 * (positions 0..2B over [src|dst]) are built and stored; "last occurrence" is
 * still resolved over the whole batch.  Used when the endpoints of a batch
 * are sharded across GPUs: every position has at most one winner, so a shard
 * touches at most pos_hi - pos_lo rows. */
int zt_store_messages_range(const float *memory_dev, const float *last_update_dev,
                            const float *efeat_dev, const float *time_w_dev,
                            int64_t num_nodes, int64_t num_edges, int32_t D, int32_t F,
                            int32_t T, const int32_t *src_dev, const int32_t *dst_dev,
                            const double *ts_dev, const int64_t *eidx_dev, int64_t B,
                            int64_t pos_lo, int64_t pos_hi, float *messages_dev,
                            float *msg_ts_dev, uint8_t *flags_dev, int32_t *scratch_dev,
                            int32_t *uniq_ids_dev, int32_t *n_uniq_dev,
                            int32_t *status_dev, void *stream);

typedef struct {
    const float *w_ih, *w_hh; /* [3D][msg], [3D][D]  (torch GRUCell, gates r,z,n) */
    const float *b_ih, *b_hh; /* [3D] */
} zt_gru_weights;             /* device pointers */

/* SequenceMemoryUpdater.update_memory / update_memory_in_test with
 * nn.GRUCell (modules/memory_updater.py:29-57,95-98), followed by
 * Memory.clear_messages (modules/memory.py:59-60) for the same ids.
 *   ids_dev == NULL : every node (update_memory_in_test);
 *   ids_dev != NULL : ids_dev[0 .. *n_ids_dev) if n_ids_dev != NULL, else
 *                     ids_dev[0 .. n_ids); duplicates are allowed.
 *   Flagged ids get last_update = msg_ts and memory = GRU(messages, memory);
 *   flags of all ids are cleared.
 *   flags_dev must be 4-byte aligned and padded to a multiple of 4 bytes (flag
 *   bytes are cleared with 32-bit atomics).
 *   workspace_dev: zt_gru_workspace_bytes(max_rows, D, msg_dim) bytes, where
 *   max_rows = n_ids (or num_nodes when ids_dev == NULL).  On return its first
 *   int32 holds the number of rows updated and the int32 array at byte
 *   zt_gru_rows_offset(D, msg_dim) their ids (duplicates in ids_dev are updated
 *   once).  The packed weights sit between the two, so their place does not
 *   depend on max_rows.
 *   weights_ready: 0 = pack the GRU weights into the workspace first; 1 = the
 *   workspace already holds them (same workspace, same weights; max_rows may
 *   differ from call to call). */
int64_t zt_gru_workspace_bytes(int64_t max_rows, int32_t D, int32_t msg_dim);
int64_t zt_gru_rows_offset(int32_t D, int32_t msg_dim);
int zt_gru_update(float *memory_dev, float *last_update_dev,
                  const float *messages_dev, const float *msg_ts_dev,
                  uint8_t *flags_dev, int64_t num_nodes, int32_t D,
                  int32_t msg_dim, const int32_t *ids_dev, int64_t n_ids,
                  const int32_t *n_ids_dev, const zt_gru_weights *weights,
                  void *workspace_dev, int32_t weights_ready, void *stream);

/* The memory cell of an update: nn.GRUCell (zt_gru_update, the default) or
 * nn.RNNCell (zt_rnn_update); zt_pipeline_set_cell picks it for a pipeline. */
#define ZT_CELL_GRU 0
#define ZT_CELL_RNN 1

/* zt_gru_update with nn.RNNCell in place of nn.GRUCell: RNNMemoryUpdater
 * (modules/memory_updater.py:100-103) with the cell's defaults (tanh, biases),
 *   memory = tanh(W_ih messages + b_ih + W_hh memory + b_hh).
 * The arguments are those of zt_gru_update; `weights` holds the RNN's shapes:
 * w_ih [D][msg], w_hh [D][D], b_ih and b_hh [D].  The workspace is the GRU's
 * (zt_gru_workspace_bytes, zt_gru_rows_offset: the row count and the row ids
 * sit where they sit for the GRU; the packed weights use the first third of
 * its weight region).  A workspace packed for the other cell must be called
 * with weights_ready = 0.  The bounds are the GRU's: ZT_ERR_UNSUPPORTED for
 * D outside (D <= 128, or a multiple of 4 up to 256) and for a message width whose staging tile needs more than 150 KB of
 * LDS (128 * (round16(msg_dim) + round16(D) + 4) + 128 bytes, the same limit
 * zt_gru_update applies).  zt_set_kernel_choice(ZT_CHOICE_GRU, ZT_GRU_TILE /
 * ZT_GRU_SPLIT) pins the kernel form for both cells. */
int zt_rnn_update(float *memory_dev, float *last_update_dev,
                  const float *messages_dev, const float *msg_ts_dev,
                  uint8_t *flags_dev, int64_t num_nodes, int32_t D,
                  int32_t msg_dim, const int32_t *ids_dev, int64_t n_ids,
                  const int32_t *n_ids_dev, const zt_gru_weights *weights,
                  void *workspace_dev, int32_t weights_ready, void *stream);

/* ------------------------------------------------------------------------ */
/* Training-side dense operators on exact-f32 MFMA (csrc/train_ops.hip).       */
/*   What the reference's autograd does with nn.GRUCell (get_updated_memory,   */
/*   modules/memory_updater.py:61-90,95-98) and nn.Linear (fc2,                */
/*   transform_source: modules/embedding_module.py:86-98,320-328) on the       */
/*   compact rows of a training step.                                          */
/* ------------------------------------------------------------------------ */
/* C[M][N] = op(A)[M][K] op(B)[K][N] (+ C if accumulate), row-major float32;
 * op(A)(m, k) = trans_a ? A[k * lda + m] : A[m * lda + k], likewise B.  All four
 * (trans_a, trans_b) forms exist.  A and B may be NULL when K == 0 (C = 0, or C kept
 * if accumulate); M == 0 or N == 0 writes nothing.  A leading dimension smaller than
 * the row it strides over -- lda < (trans_a ? M : K), ldb < (trans_b ? K : N),
 * ldc < N -- is refused with ZT_ERR_ARG before any launch (rows would overlap). */
int zt_gemm_f32(const float *A_dev, const float *B_dev, float *C_dev, int64_t M, int64_t N,
                int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t trans_a,
                int32_t trans_b, int32_t accumulate, void *stream);
/* out[c] (+)= sum over rows of X[r][c] (bias gradients); rows == 0: zeros, or out kept
 * if accumulate.  ldx < cols is refused with ZT_ERR_ARG before any launch. */
int zt_colsum_f32(const float *X_dev, int64_t rows, int64_t cols, int64_t ldx, float *out_dev,
                  int32_t accumulate, void *stream);
/* The batch's own rows of the lazily updated memory -- get_updated_memory(...)[nodes]
 * (modules/memory_updater.py:61-90, modules/embedding_module.py:320-322): out[i] =
 * overlay[row_map[nodes[i]]] where row_map (NULL: none) names an overlay row, else
 * memory[nodes[i]]; sel[i] = that overlay row or -1.  The backward adds d_out[i] to
 * d_overlay[sel[i]] (atomic: a node may appear several times; the caller zeroes d_overlay). */
int zt_overlay_rows(const float *memory_dev, const float *overlay_dev, const int32_t *row_map_dev,
                    const int32_t *nodes_dev, int64_t n, int32_t D, int64_t num_nodes,
                    float *out_dev, int32_t *sel_dev, void *stream);
int zt_overlay_rows_backward(const float *d_out_dev, const int32_t *sel_dev, int64_t n, int32_t D,
                             float *d_overlay_dev, void *stream);
/* h_out[u] = GRUCell(messages[ids[u]], memory[ids[u]]) for the U rows ids (the
 * lazily updated rows of get_updated_memory); saved [U][4 D] keeps r, z, n and
 * W_hn h + b_hn for the backward.  workspace: zt_gru_train_workspace_bytes. */
int64_t zt_gru_train_workspace_bytes(int64_t U, int32_t D, int32_t msg_dim);
int zt_gru_train_forward(const float *messages_dev, const float *memory_dev,
                         const int32_t *ids_dev, int64_t U, int32_t D, int32_t msg_dim,
                         const zt_gru_weights *weights, float *h_out_dev, float *saved_dev,
                         void *workspace_dev, void *stream);
/* Gradients of the four GRU parameters from d_h [U][D] (written, not
 * accumulated).  Messages and memory are buffers in the reference: they get
 * no gradient.  workspace_dev must be the FORWARD call's workspace, untouched:
 * it holds the gathered rows (the tables themselves change between forward
 * and backward, model/tgn_model.py:155-168). */
int zt_gru_train_backward(const float *d_h_dev, const float *messages_dev,
                          const float *memory_dev, const int32_t *ids_dev, int64_t U,
                          int32_t D, int32_t msg_dim, const float *saved_dev,
                          float *d_w_ih_dev, float *d_w_hh_dev, float *d_b_ih_dev,
                          float *d_b_hh_dev, void *workspace_dev, void *stream);
/* The same pair for nn.RNNCell (RNNMemoryUpdater): h_out[u] = tanh(W_ih x + b_ih
 * + W_hh h + b_hh) with x = messages[ids[u]], h = memory[ids[u]]; weights as for
 * zt_rnn_update.  saved is [U][D] and holds h_out.  The backward writes dW_ih
 * [D][msg], dW_hh [D][D], db_ih and db_hh [D].  The arguments, the workspace
 * (zt_gru_train_workspace_bytes) and the rule that the backward gets the
 * forward's workspace untouched are the GRU pair's. */
int zt_rnn_train_forward(const float *messages_dev, const float *memory_dev,
                         const int32_t *ids_dev, int64_t U, int32_t D, int32_t msg_dim,
                         const zt_gru_weights *weights, float *h_out_dev, float *saved_dev,
                         void *workspace_dev, void *stream);
int zt_rnn_train_backward(const float *d_h_dev, const float *messages_dev,
                          const float *memory_dev, const int32_t *ids_dev, int64_t U,
                          int32_t D, int32_t msg_dim, const float *saved_dev,
                          float *d_w_ih_dev, float *d_w_hh_dev, float *d_b_ih_dev,
                          float *d_b_hh_dev, void *workspace_dev, void *stream);

/* ------------------------------------------------------------------------ */
/* One batch as one call -- TGN.compute_temporal_embeddings, train=False      */
/*   (model/tgn_model.py:124-174) for device-resident batches.  The reference */
/*   issues these steps from Python on one stream (train.py:145-146); here     */
/*   they are enqueued from C++ on three streams: the T-PPR query of batch b+1 */
/*   (side stream, CU-masked to tppr_cus compute units when > 0) beside        */
/*   aggregate + messages + GRU of batch b (main stream, the remaining CUs),   */
/*   the dependency prepass of batch b+2 on a third.                           */
/* ------------------------------------------------------------------------ */
typedef struct {
    zt_tppr *tppr;                 /* streaming strategy: the T-PPR state; else NULL      */
    const zt_csr *csr;             /* pruning strategy: the adjacency; else NULL          */
    int32_t width, depth;          /* pruning: n_degree, n_layer (train.py:25,28)         */
    double alpha[16], beta[16];    /* pruning: per model                                  */
    float *memory, *last_update, *messages, *msg_ts;   /* Memory (modules/memory.py:19-25) */
    uint8_t *flags;                /* pending-message flags, padded to 4 bytes            */
    int32_t *scratch;              /* int32[num_nodes], all -1 (zt_store_messages)        */
    const float *efeat;
    int64_t num_nodes, num_edges;
    int32_t D, F, T, M, k;
    zt_embed_weights ew;
    zt_gru_weights gw;
    void *embed_ws;                /* zt_embed_workspace_bytes(3*max_B, ...)              */
    void *gru_ws;                  /* zt_gru_workspace_bytes(2*max_B, ...)                */
    float *proj_table;             /* zt_project_memory table kept current by the step, or NULL */
    int32_t *status;               /* latched ZT_ERR_RANGE of the aggregate / message kernels   */
    int64_t max_B;                 /* largest batch                                       */
} zt_pipeline_desc;                /* all pointers device memory */

typedef struct {
    const int32_t *src, *dst, *neg;   /* int32[B] each */
    const double *ts;                 /* float64[B]    */
    const int64_t *eidx;              /* int64[B]; also identifies the batch between calls */
    int64_t B;
} zt_batch;

typedef struct zt_pipeline zt_pipeline;
int zt_pipeline_create(zt_pipeline **out, const zt_pipeline_desc *desc, int32_t tppr_cus);
int zt_pipeline_destroy(zt_pipeline *p);
/* The stream the outputs are produced on (hipStream_t): consumers and any collective that follows a step
 * (the row exchange of a sharded run) are enqueued there. */
void *zt_pipeline_main_stream(zt_pipeline *p);
/* New table pointers / handles (Memory tensors replaced, neighbour finder swapped: desc != NULL) and / or
 * weights changed in place (weights_changed: the padded copies in the workspaces are remade). */
int zt_pipeline_update(zt_pipeline *p, const zt_pipeline_desc *desc, int32_t weights_changed);
/* One eval-mode batch.  next / plan (optional): the batches of the following two steps; `next` is QUERIED now
 * (streaming: its T-PPR update is applied), so it must be the batch of the next call.  Rows [row_lo, row_hi)
 * of [src|dst|neg] are embedded into out_emb_dev [row_hi-row_lo][D*(M+1)] and the last messages of the
 * endpoints at positions [pos_lo, pos_hi) of [src|dst] are stored and applied (a single GPU passes 0, 3B, 0,
 * 2B; shards of a multi-GPU run their slices and exchange the touched rows afterwards).  No host
 * synchronisation; errors of the device side are latched (zt_tppr_status, desc.status). */
int zt_pipeline_step(zt_pipeline *p, const zt_batch *cur, const zt_batch *next, const zt_batch *plan,
                     int64_t row_lo, int64_t row_hi, int64_t pos_lo, int64_t pos_hi, float *out_emb_dev);
/* The same step with a longer view of the stream: ahead[0 .. n_ahead) are the batches that follow `cur`, in order.
 * With zt_pipeline_set_group(p, g), g <= 4, the streaming T-PPR update of g consecutive batches runs as ONE launch
 * (edges applied in order across them, exactly as in separate calls; every batch's output rows form their own
 * block), which pays a launch's fixed costs once per group; the pipeline then queries the group after the current
 * one and plans the one after that, so 3 g + 1 batches in sight keep it full (a group takes at most n - 1 of the n followers in sight along -- the last three batches of a stream are queried one by one --; fewer: smaller groups).  Batches of
 * a group are equally long (the last may be shorter) and together at most 16384 edges.  zt_pipeline_step is this
 * call with ahead = {next, plan}.  The pruning strategy carries no state between batches: its group is 1. */
int zt_pipeline_set_group(zt_pipeline *p, int32_t group);
/* The memory cell of the pipeline's update: ZT_CELL_GRU (the default; desc.gw holds nn.GRUCell's weights) or
 * ZT_CELL_RNN (desc.gw holds nn.RNNCell's, shapes as for zt_rnn_update; desc.gru_ws is sized as for the GRU).
 * It takes effect at the next step, which packs the weights afresh.  ZT_ERR_ARG for a NULL pipeline or another value. */
int zt_pipeline_set_cell(zt_pipeline *p, int32_t cell);
/* embedding_module.average_topk (modules/embedding_module.py:232-233): with a non-NULL device float, every step
 * over a whole batch also writes the mean over the 2B rows of [src | dst] of the sum of model 0's T-PPR weights
 * there (main stream).  NULL switches it off. */
int zt_pipeline_set_stats(zt_pipeline *p, float *avg_topk_dev);
/* Batches whose T-PPR query was launched ahead of their step and that no step has consumed yet.  While it is
 * non-zero the streaming T-PPR state is AHEAD of the last step: a caller must not query or update the state
 * through zt_tppr_stream (or leave the announced order) before those batches have been stepped. */
int zt_pipeline_outstanding(const zt_pipeline *p);
/* Steps since zt_pipeline_create whose GRU kernel carried the NEXT batch's gate of the release by member at its tail, so that
 * the next step passed no gate of its own (pipeline.hip, "the gate at the tail of the GRU"); for tests and tools. */
int zt_pipeline_tail_gates(const zt_pipeline *p);
/* Returns ZT_ERR_TIMEOUT (once) when a kernel of an EARLIER step gave up a bounded in-kernel wait -- the gate between the
 * output layers and the GRU update in their shared launch waits at most 4 s for the source path's reads, then leaves the
 * memory rows of its tile untouched and reports to the status word of the descriptor and to a host-mapped latch that
 * this call looks at on entry: that step's memory update is incomplete. */
int zt_pipeline_step_ahead(zt_pipeline *p, const zt_batch *cur, const zt_batch *ahead, int32_t n_ahead,
                           int64_t row_lo, int64_t row_hi, int64_t pos_lo, int64_t pos_hi, float *out_emb_dev);
/* n consecutive whole-batch steps from one host call (the batch loop of evaluation/evaluation.py:19-45): step b sees
 * batches b + 1 .. b + look as `ahead`, never beyond the n given; its [3 B_b][D (M + 1)] embeddings go to
 * out_emb_dev + b * out_stride floats (out_stride 0: one buffer, overwritten every step). */
/* ---- the row exchange of a multi-GPU run inside the native step loop (no reference counterpart: the
 * reference is one process on one device, train.py:145-146).  One process per GPU; T-PPR state and tables replicated;
 * rank r embeds the rows shard_range(3B, r, world) of every batch, stores and applies the last messages of the winners at
 * positions shard_range(2B, r, world), and after the GRU update of the batch the rows every rank rewrote -- [id | memory
 * row | last_update], and [message row | message time] when with_messages -- are all-gathered with ONE fixed-size
 * collective (cap_rows >= ceil(2 max_B / world) rows per rank), scattered into the local tables, and the projected table
 * follows: all on the pipeline's main stream, enqueued by zt_pipeline_step_ahead / zt_pipeline_run themselves once
 * zt_pipeline_set_exchange has been called (row_lo .. pos_hi of the step call are then this rank's shard, as before).
 *   ZT_XCHG_RCCL: RCCL's ncclAllGather (xGMI), one rank per GPU; unique_id = the 128 bytes zt_exchange_unique_id wrote
 *                 on rank 0, distributed by the caller; zt_exchange_create is collective (ncclCommInitRank);
 *   ZT_XCHG_SHM : tests / rehearsals with several ranks on ONE GPU (RCCL refuses that layout): a POSIX shared-memory
 *                 segment named shm_name, two host synchronisations per step.
 * with_messages = 0 is enough for the eval protocol: a batch's messages are consumed by the GRU update of the step that
 * stored them (model/tgn_model.py:159-172); a caller that compares the messages table across ranks switches it on. */
#define ZT_XCHG_RCCL 1
#define ZT_XCHG_SHM 2
typedef struct {
    int32_t rank, world, transport, with_messages;
    const void *unique_id;         /* ZT_XCHG_RCCL: 128 bytes */
    const char *shm_name;          /* ZT_XCHG_SHM */
    int64_t cap_rows;
    float *memory, *last_update, *messages, *msg_ts;   /* the tables of zt_pipeline_desc */
    int32_t D, msg_dim;
} zt_exchange_desc;
typedef struct zt_exchange zt_exchange;
int zt_exchange_unique_id(void *id_out, int64_t bytes);
int zt_exchange_create(zt_exchange **out, const zt_exchange_desc *desc);
int zt_exchange_set_tables(zt_exchange *x, float *memory, float *last_update, float *messages, float *msg_ts);
int zt_exchange_destroy(zt_exchange *x);
/* x != NULL: every step of this pipeline ends with the exchange (and zt_pipeline_run shards every batch by x's rank and
 * world: out_emb_dev + b * out_stride then receives the rank's rows_hi - rows_lo embedding rows of step b); NULL: off.
 * The pipeline does not own x. */
int zt_pipeline_set_exchange(zt_pipeline *p, zt_exchange *x);
int zt_pipeline_run(zt_pipeline *p, const zt_batch *batches, int32_t n, int32_t look, float *out_emb_dev,
                    int64_t out_stride);

/* ------------------------------------------------------------------------ */
/* TemporalAttentionLayer.forward -- model/temporal_attention.py:7-68        */
/*   NOT on the reference's live path (never reachable from train.py); built */
/*   because the north star names it.  Eval forward (dropout = identity).    */
/* ------------------------------------------------------------------------ */
typedef struct {
    const float *q_w;            /* multi_head_target.q_proj_weight [E][E], E = D+T      */
    const float *k_w, *v_w;      /* k_proj_weight, v_proj_weight    [E][Ek], Ek = D+F+T   */
    const float *in_b;           /* in_proj_bias [3E] (q, k, v)                          */
    const float *out_w, *out_b;  /* out_proj [E][E], [E]                                 */
    const float *m1_w, *m1_b;    /* merger.fc1 [hidden][E+D], [hidden]                   */
    const float *m2_w, *m2_b;    /* merger.fc2 [out_dim][hidden], [out_dim]              */
} zt_attn_weights;               /* device pointers */

/*   src [N][D], src_time [N][T], nbr_feat [N][k][D], edge_feat [N][k][F],
 *   nbr_time [N][k][T], mask uint8 [N][k] (non-zero = padding)
 *   -> out [N][out_dim], attn_w [N][k] (head-averaged attention weights).
 *   Shapes taken: 1 <= n_head <= 4 dividing E; k <= 80; and one workgroup's tile -- a query row's k key rows, rounded
 *   up to 16, at width Ek, their projection at width E and three 16-row blocks as wide as the widest of E + D, hidden
 *   and out_dim -- within 158 KB of LDS (D = T = 100, F = 172: k <= 48; D = F = T = 172: k <= 16; D = T = 224, F = 1:
 *   k <= 16; D = T = 228 and wider: none).  Any other shape: zt_attention_workspace_bytes returns -1 and
 *   zt_temporal_attention ZT_ERR_UNSUPPORTED before anything is launched; there is no fall-back. */
int64_t zt_attention_workspace_bytes(int32_t D, int32_t F, int32_t T, int32_t n_head,
                                     int32_t hidden, int32_t out_dim, int32_t k);
int zt_temporal_attention(const float *src_dev, const float *src_time_dev,
                          const float *nbr_feat_dev, const float *edge_feat_dev,
                          const float *nbr_time_dev, const uint8_t *mask_dev, int64_t N,
                          int32_t k, int32_t D, int32_t F, int32_t T, int32_t n_head,
                          int32_t hidden, int32_t out_dim, const zt_attn_weights *weights,
                          float *out_dev, float *attn_w_dev, void *workspace_dev,
                          void *stream);

/* The layer in a training step (csrc/attention_train.hip): the same forward with the dropout of
 * nn.MultiheadAttention inside -- the softmax weights times a keep-mask that is a hash of drop_seed and the
 * element (n * n_head + h) * k + j, 1 / (1 - drop_p) or 0; attn_w is the head mean of the weights AFTER dropout,
 * as torch returns them -- and its backward.  With drop_p = 0 out and attn_w are zt_temporal_attention's bit for bit.
 * No float atomics: two calls on the same inputs give the same bits.  attn_w is not differentiated through.
 *
 * zt_attention_train_plan (host code only): out[8] = supported (0 / 1), rq (query rows per workgroup), mt (16-row
 *   M-tiles of key rows), dynamic LDS bytes of the forward and of the backward, workspace bytes per row, workspace
 *   bytes fixed, saved bytes per row; all 0 where the shape is refused.  The shapes are zt_temporal_attention's (the
 *   backward runs in the forward's LDS tile).
 * workspace: fixed + N * per row bytes, 16-byte aligned -- fixed holds the zero-padded weights of the forward (the
 *   only part the forward touches) and the transposed padded merger.fc2, merger.fc1 and out_proj; per row
 *   4 (hidden + 2 E + 2 k E) bytes: the row deltas d_hid, d_y, d_q / sqrt(hd), d_K, d_V.
 * saved: N * 4 (k n_head + 2 E + hidden) bytes -- the softmax weights before dropout, the concatenated heads, the
 *   out_proj output and relu(merger.fc1); q, K and V are recomputed by the backward.
 * The two size queries return -1 where the plan refuses (or N < 0).  Both calls: ZT_ERR_ARG for a NULL required
 * buffer, a negative size or drop_p outside [0, 1); ZT_ERR_UNSUPPORTED for a refused shape; N == 0 is ZT_OK and
 * launches nothing -- all before any device call. */
typedef struct {
    float *d_src, *d_src_time;                  /* [N][D], [N][T]                       */
    float *d_nbr_feat, *d_edge_feat, *d_nbr_time; /* [N][k][D], [N][k][F], [N][k][T]    */
    float *d_q_w, *d_k_w, *d_v_w, *d_in_b;      /* as zt_attn_weights                   */
    float *d_out_w, *d_out_b;
    float *d_m1_w, *d_m1_b, *d_m2_w, *d_m2_b;
} zt_attn_grads;                 /* device pointers; any may be NULL: that gradient is not computed */
int zt_attention_train_plan(int32_t D, int32_t F, int32_t T, int32_t n_head, int32_t hidden,
                            int32_t out_dim, int32_t k, int64_t *out);
int64_t zt_attention_train_workspace_bytes(int64_t N, int32_t D, int32_t F, int32_t T,
                                           int32_t n_head, int32_t hidden, int32_t out_dim,
                                           int32_t k);
int64_t zt_attention_train_saved_bytes(int64_t N, int32_t D, int32_t F, int32_t T, int32_t n_head,
                                       int32_t hidden, int32_t out_dim, int32_t k);
int zt_attention_train_forward(const float *src_dev, const float *src_time_dev,
                               const float *nbr_feat_dev, const float *edge_feat_dev,
                               const float *nbr_time_dev, const uint8_t *mask_dev, int64_t N,
                               int32_t k, int32_t D, int32_t F, int32_t T, int32_t n_head,
                               int32_t hidden, int32_t out_dim, const zt_attn_weights *weights,
                               float drop_p, uint64_t drop_seed, float *out_dev, float *attn_w_dev,
                               float *saved_dev, void *workspace_dev, void *stream);
/* d_out [N][out_dim]; saved as the forward of the same inputs, weights, drop_p and drop_seed left it. */
int zt_attention_train_backward(const float *src_dev, const float *src_time_dev,
                                const float *nbr_feat_dev, const float *edge_feat_dev,
                                const float *nbr_time_dev, const uint8_t *mask_dev, int64_t N,
                                int32_t k, int32_t D, int32_t F, int32_t T, int32_t n_head,
                                int32_t hidden, int32_t out_dim, const zt_attn_weights *weights,
                                float drop_p, uint64_t drop_seed, const float *saved_dev,
                                const float *d_out_dev, const zt_attn_grads *grads,
                                void *workspace_dev, void *stream);

/* ------------------------------------------------------------------------ */
/* Link scoring and link-prediction metrics      */
/* ------------------------------------------------------------------------ */
typedef struct {
    const float *fc1_w, *fc1_b;  /* affinity_score.fc1 [H][2H], [H]   (MergeLayer, utils/util.py:14-26) */
    const float *fc2_w, *fc2_b;  /* affinity_score.fc2 [1][H], [1]                                     */
} zt_affinity_weights;           /* device pointers */

/* TGN.compute_edge_probabilities' scorer (model/tgn_model.py:185-188):
 *   emb_dev [3B][H] = the batch's embeddings [src | dst | neg], H = D * (n_tppr + 1): any H with H % 4 == 0 and
 *                     4 <= H <= 768 -- the widths the training scorer below takes (ZT_ERR_UNSUPPORTED otherwise);
 *   prob_dev [2B]   = sigmoid(fc2(relu(fc1([src | dst])))) for the B positive pairs, then the same for (src, neg).
 * Hidden widths 200 and 300 (D = 100 with one or two T-PPR models) run kernels specialised for them, every other width
 * two generic ones (K and N run over H at run time); by batch size a latency-organised form or a tiled one
 * (ZT_CHOICE_SCORE pins the form).  No float atomics: two calls give the same bits.  emb_dev and fc1_w are 16-byte
 * aligned.
 * workspace_dev: zt_affinity_workspace_bytes(max_B, H) bytes (-1 = H unsupported), sized for ws_max_B >= B;
 * weights_ready as for zt_embed (0 also clears the workspace's tile counters: use it for a fresh workspace). */
int64_t zt_affinity_workspace_bytes(int64_t max_B, int32_t H);
int zt_affinity(const float *emb_dev, int64_t B, int32_t H, const zt_affinity_weights *weights,
                float *prob_dev, void *workspace_dev, int64_t ws_max_B, int32_t weights_ready,
                void *stream);
/* The same scorer for a TRAINING step, differentiable (csrc/scoring_train.hip): any H with H % 4 == 0 and
 * 4 <= H <= 768 (ZT_ERR_UNSUPPORTED otherwise), any B >= 0 (B = 0: ZT_OK, nothing touched).  The parameters are read
 * as they lie in the module (no packed copy, no weights_ready); emb_dev and the weight matrices are 16-byte aligned.
 *   forward:  emb_dev [3B][H] -> prob_dev [2B] (the layout zt_affinity writes) and hid_dev [2B][H], the hidden rows
 *             after the ReLU (pair rows: B positive, then B negative), kept for the backward.  One launch.
 *   backward: from dprob_dev [2B] and the forward's prob_dev / hid_dev: d_emb_dev [3B][H], d_fc1_w_dev [H][2H],
 *             d_fc1_b_dev [H], d_fc2_w_dev [H], d_fc2_b_dev [1], written, not accumulated.  An output that is not needed is
 *             NULL and its work is skipped.  At most three launches, no host synchronisation, no atomics: every sum
 *             has a fixed order, two runs give the same bits.
 * workspace_dev (backward only): zt_affinity_train_workspace_bytes(max_B, H) bytes (-1 = H unsupported), sized for
 * ws_max_B >= B; it holds d(hidden) [2B][H], d(score) [2B] and the partial products of the weight gradient. */
int64_t zt_affinity_train_workspace_bytes(int64_t max_B, int32_t H);
int zt_affinity_train_forward(const float *emb_dev, int64_t B, int32_t H,
                              const zt_affinity_weights *weights, float *prob_dev, float *hid_dev,
                              void *stream);
int zt_affinity_train_backward(const float *emb_dev, int64_t B, int32_t H,
                               const zt_affinity_weights *weights, const float *prob_dev,
                               const float *hid_dev, const float *dprob_dev, float *d_emb_dev,
                               float *d_fc1_w_dev, float *d_fc1_b_dev, float *d_fc2_w_dev,
                               float *d_fc2_b_dev, void *workspace_dev, int64_t ws_max_B,
                               void *stream);
/* zt_affinity_train_plan (host code only, the one place that decides; the backward launches from the same function): the
 * launches of zt_affinity_train_backward over B edges with every output asked for, out[ZT_AFFINITY_TRAIN_PLAN_FIELDS], all
 * int64:
 *   [0] split        partial products of d_fc1_w over K = 2B pair rows (1: written directly)
 *   [1] k_per        pair rows per partial product, whole 64-row steps
 *   [2] max_split    the most partial products this width takes
 *   [3] steps        64-row steps of K = 2B
 *   [4] grid_dx      workgroups of k_score_bwd_dx (16 edges each)
 *   [5..7] grid_dw   x, y, z of k_score_bwd_dw's grid (z = split)
 *   [8] grid_fin     workgroups of k_score_bwd_fin: the column sums, then the sum of the partial products
 *   [9] lds_dx       dynamic LDS of k_score_bwd_dx in bytes
 * With d_fc1_w_dev = NULL the backward runs no k_score_bwd_dw and takes split = 1.
 * ZT_ERR_ARG for NULL out or B < 0, ZT_ERR_UNSUPPORTED for the width. */
#define ZT_AFFINITY_TRAIN_PLAN_FIELDS 10
int zt_affinity_train_plan(int64_t B, int32_t H, int64_t *out);
/* evaluation/evaluation.py:34-45 and train.py:218-227 without the host: out_dev[0..3) (float64) =
 * (average_precision_score, roc_auc_score, mean(pos >= neg)) of B positive and B negative scores, scikit-learn's
 * definitions (distinct thresholds, ties included); accumulate != 0 adds to out_dev.  One single-workgroup kernel in one of
 * two forms: up to 8192 pairs the 2B scores are sorted together as 64-bit (key | label) words; from 8193 to 16384 pairs the
 * positive and the negative 32-bit keys are sorted as two runs and walked together (the 64-bit layout would not fit the
 * 160 KB of LDS).  Float64 sums in a fixed order, no float atomics: two calls give the same bits.  B > 16384:
 * ZT_ERR_UNSUPPORTED before any device call.  zt_link_metrics_plan is where the form is decided (host code only). */
int zt_link_metrics(const float *pos_dev, const float *neg_dev, int64_t B, double *out_dev,
                    int32_t accumulate, void *stream);
/* One source against many candidates (csrc/rank.hip): prob_dev [Q][C],
 *   prob[q][c] = sigmoid(fc2(relu(fc1([emb_q[q] | emb_c[cand_idx[q][c]]])))),
 * MergeLayer as compute_edge_probabilities applies it (model/tgn_model.py:185-188, utils/util.py:14-26).  emb_q_dev [Q][H],
 * emb_c_dev [Nc][H]; cand_idx_dev [Q][C] names rows of emb_c, -1 = absent (probability 0 is written); NULL: every query takes
 * all Nc candidates in order, and C must equal Nc (ZT_ERR_ARG otherwise).  The weights are read as they lie in the module
 * (UNPACKED, as zt_affinity_train_forward; fc1_b and fc2_w 16-byte aligned).  Two launches of the f32 MFMA GEMM project both
 * sides into the workspace (P_q = emb_q W_a^T, P_c = emb_c W_b^T), one pair kernel does the rest: H runs in chunks, so no
 * LDS-resident-row bound applies: any H % 4 == 0 with 4 <= H <= 4352 (ZT_ERR_UNSUPPORTED otherwise -- this bound is
 * zt_affinity_rank's own, zt_affinity and zt_affinity_train_* keep theirs).  Every pair's sum has one fixed association, no
 * float atomics: two calls give the same bits.  Q = 0 or C = 0: ZT_OK, nothing touched; argument checks come before any
 * device call.
 * workspace_dev: zt_affinity_rank_workspace_bytes(Q, Nc, H) bytes (-1: H unsupported, or a negative size), 16-byte aligned,
 * sized for THIS call's Q and Nc or more.  Its first int32 is the call's status word: the call sets it to 0, and to
 * ZT_ERR_RANGE when an index is >= Nc or below -1 (that pair reads probability 0); read it once the stream has passed the
 * call. */
int64_t zt_affinity_rank_workspace_bytes(int64_t Q, int64_t Nc, int32_t H);
int zt_affinity_rank(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                     const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w,
                     float *prob_dev, void *workspace_dev, void *stream);
/* The same scorer for a RANKING training step, differentiable (csrc/rank_train.hip).  Inputs, widths (H % 4 == 0,
 * 4 <= H <= 4352; ZT_ERR_UNSUPPORTED otherwise, before any launch), the C == Nc rule without an index and the status word
 * (first int32 of the workspace, set to 0 by each call) are zt_affinity_rank's; emb_q_dev, emb_c_dev and fc1_w are 16-byte
 * aligned.  Q = 0 or C = 0: ZT_OK, nothing touched; argument checks come before any device call; Q C must fit an int32.
 *   forward:  logit_dev [Q][C] = b2 + sum_h w2[h] relu((P_q[q][h] + b1[h]) + P_c[row][h]) -- zt_affinity_rank's pair sum:
 *             1 / (1 + expf(-logit)) has the bits zt_affinity_rank writes for the pair -- and -inf for an absent pair (index
 *             -1, or out of range: ZT_ERR_RANGE in the status word).  pq_dev [Q][H] and pc_dev [Nc][H] (16-byte aligned)
 *             receive the two projections; the caller keeps them for the backward.
 *   backward: from dl_dev [Q][C] = d(loss)/d(logit) (ignored at absent pairs) and the forward's pq_dev / pc_dev:
 *             d_emb_q_dev [Q][H], d_emb_c_dev [Nc][H] (a row no pair names: zeros), d_fc1_w_dev [H][2H], d_fc1_b_dev [H],
 *             d_fc2_w_dev [H], d_fc2_b_dev [1], written, not accumulated; an output that is not needed is NULL and its work
 *             is skipped.  The hidden layer is formed again from pq_dev and pc_dev: no array of Q C H elements exists.
 *             With an index the caller passes its transpose: row_ptr_dev int64 [Nc + 1] and pairs_dev int32 [n_pairs], the
 *             ids q C + c of the present pairs grouped by the row they name, ascending within a row.  A pair id outside
 *             [0, Q C), a pair listed under a row it does not name or a row range outside [0, n_pairs] is left out and sets
 *             ZT_ERR_RANGE in the status word; nothing is read or written out of bounds.  Two kernels, three zt_colsum_f32
 *             and four zt_gemm_f32; every sum has one fixed association, no float atomics: two runs give the same bits.
 * workspace_dev: zt_affinity_rank_train_workspace_bytes(Q, Nc, C, H) bytes (-1: H unsupported, or a negative size), 16-byte
 * aligned; the forward uses its status word only, the backward also d(P_q), d(P_c) and the partial sums of d_fc2_w. */
int64_t zt_affinity_rank_train_workspace_bytes(int64_t Q, int64_t Nc, int64_t C, int32_t H);
int zt_affinity_rank_train_forward(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                                   const int32_t *cand_idx_dev, int64_t C, int32_t H,
                                   const zt_affinity_weights *w, float *logit_dev, float *pq_dev,
                                   float *pc_dev, void *workspace_dev, void *stream);
int zt_affinity_rank_train_backward(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                                    const int32_t *cand_idx_dev, int64_t C, int32_t H,
                                    const zt_affinity_weights *w, const float *pq_dev,
                                    const float *pc_dev, const float *dl_dev, const int64_t *row_ptr_dev,
                                    const int32_t *pairs_dev, int64_t n_pairs, float *d_emb_q_dev,
                                    float *d_emb_c_dev, float *d_fc1_w_dev, float *d_fc1_b_dev,
                                    float *d_fc2_w_dev, float *d_fc2_b_dev, void *workspace_dev,
                                    void *stream);
/* The K likeliest candidates of every query (csrc/rank_topk.hip) without prob[Q][C]: emb_q_dev, emb_c_dev, cand_idx_dev (NULL:
 * every query takes all Nc rows in order, C == Nc), the weights, the width bound and the status word (first int32 of the
 * workspace; ZT_ERR_RANGE for an index >= Nc or < -1, that pair counts as absent) are zt_affinity_rank's, and every pair's
 * probability has the bits zt_affinity_rank writes for it (csrc/rank_pair.hpp: one pair sum for both).
 *   top_idx_dev [Q][K] (int32) = idx_base + c, c the column in [0, C); top_prob_dev [Q][K] = the probabilities: the K present
 *   candidates with the largest probability in descending order, equal probabilities in ascending index; slots beyond the
 *   number of present candidates read -1 and 0.  Present: the index is >= 0 and in range, the global column idx_base + c
 *   differs from skip_dev[q] (skip_dev NULL, or -1 for a query: nothing left out), and the probability is not NaN -- nor the
 *   candidate's projected row, which a NaN anywhere in its embedding makes NaN throughout (the pair sum's relu would drop it:
 *   zt_affinity_rank writes a finite number for such a row; here it is never selected).  The order
 *   on (probability, index) is strict: the result is a function of the inputs alone, whatever the workspace, slabs or grid.
 *   accumulate != 0: the K entries already in top_idx_dev / top_prob_dev (index -1: an empty slot) compete with this call's
 *   candidates; the caller keeps their indices outside [idx_base, idx_base + C).  A pool given in pieces, in any order, gives
 *   the bits of one call over the whole pool.
 * 1 <= K <= ZT_TOPK_MAX_K (K <= 0: ZT_ERR_ARG; above: ZT_ERR_UNSUPPORTED); idx_base < 0 or idx_base + C > INT32_MAX: ZT_ERR_ARG.
 * Q = 0: ZT_OK, nothing touched.  C = 0: ZT_OK, the output filled with -1 and 0, or left alone under accumulate.  Argument
 * checks come before any device call.
 * workspace_dev, 16-byte aligned, of workspace_bytes bytes as the caller states them: P_q, one list of K keys per query and span,
 * and P_c of ONE SLAB of candidate rows -- the pool is walked a slab at a time (per slab: the f32 MFMA GEMM, the pair kernel
 * over spans of candidate columns with a running top-K per wave, the merge kernel), so no "Q x C pairs exceed one launch" bound
 * applies and memory does not grow with the pool.  zt_affinity_topk_workspace_bytes(Q, Nc, H, K) is the recommended size
 * (-1: H or K unsupported, or a negative size); it stops growing once Nc exceeds the plan's slab cap (128 MiB of P_c, or 2^18 rows).  Its
 * value for Nc = 32 is the smallest size accepted (ZT_ERR_ARG below it).
 * zt_affinity_topk_plan is where the form, the slab rows, the spans and the grids are decided (host code only; indexed != 0:
 * cand_idx is given).  No float atomics, no workgroup waits for another: two calls give the same bits. */
#define ZT_TOPK_MAX_K 256
#define ZT_TOPK_FORM_LANE 1  /* K <= 64: a wave's list is one 64-bit key per lane */
#define ZT_TOPK_FORM_LANE4 2 /* 64 < K <= 256: four keys per lane */
#define ZT_TOPK_PLAN_FIELDS 12
/* plan_out[ZT_TOPK_PLAN_FIELDS], all int64:
 *   [0] form         ZT_TOPK_FORM_*
 *   [1] wave_queries queries a wave scores each candidate row against: 4 (shared pool: the row's registers are reused) or 1
 *   [2] q_tiles      tiles of 4 queries
 *   [3] slab_rows    rows of P_c the workspace holds (a multiple of 32)
 *   [4] n_slabs      slabs the pool is walked in: n_slabs * slab_rows >= Nc
 *   [5] span_cols    candidate columns per span (shared pool: of a slab's rows; indexed: of the C index columns)
 *   [6] n_spans      spans per slab
 *   [7] grid_pairs   workgroups of the pair kernel, per slab: q_tiles * n_spans
 *   [8] grid_merge   workgroups of the merge kernel, per slab
 *   [9] lists_offset byte offset of the per-span lists in the workspace
 *  [10] pc_offset    byte offset of the slab's P_c
 *  [11] min_bytes    the smallest workspace accepted
 * ZT_ERR_ARG for NULL plan_out, a negative size, C != Nc without indices or a workspace below min_bytes; K and H as above. */
int64_t zt_affinity_topk_workspace_bytes(int64_t Q, int64_t Nc, int32_t H, int32_t K);
int zt_affinity_topk(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                     const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w,
                     int32_t K, const int32_t *skip_dev, int64_t idx_base, int32_t accumulate,
                     int32_t *top_idx_dev, float *top_prob_dev,
                     void *workspace_dev, int64_t workspace_bytes, void *stream);
int zt_affinity_topk_plan(int64_t Q, int64_t Nc, int64_t C, int32_t H, int32_t K, int32_t indexed,
                          int64_t workspace_bytes, int64_t *plan_out);
/* zt_affinity_topk with a per-query set of absent columns.  ABSENT BITS: absent_dev [Q][absent_words] (uint32),
 * absent_words >= ceil(C / 32); bit c & 31 of word c >> 5 of row q, when set, means that the LOCAL column c in [0, C) of this
 * call (not idx_base + c) is not present for query q; bits at columns >= C are zero.  zt_exclude_mark writes this format.
 * Present: zt_affinity_topk's rule, and the column's bit is clear -- in the shared form every query tests its own row of bits,
 * whatever slab or span the column falls in.  A query whose columns are all absent gives -1 and 0 in every slot.  The plan,
 * the workspace (layout and size), the merge, accumulate, skip_dev, the NaN rule and the status word are zt_affinity_topk's;
 * under accumulate each piece of a pool comes with its own local bits.  absent_dev == NULL: zt_affinity_topk exactly.
 * A non-NULL absent_dev with absent_words < ceil(C / 32): ZT_ERR_ARG before any device call; every other error is
 * zt_affinity_topk's. */
int zt_affinity_topk_masked(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc,
                            const int32_t *cand_idx_dev, int64_t C, int32_t H, const zt_affinity_weights *w,
                            int32_t K, const int32_t *skip_dev, int64_t idx_base, int32_t accumulate,
                            int32_t *top_idx_dev, float *top_prob_dev,
                            void *workspace_dev, int64_t workspace_bytes,
                            const uint32_t *absent_dev, int64_t absent_words, void *stream);
/* Where a probability stands in a shared pool (csrc/rank_count.hip) without prob[Q][C]: for every query the number of present
 * candidates whose probability is ABOVE thr_dev[q] and the number EQUAL to it -- what a full-pool rank needs.  emb_q_dev,
 * emb_c_dev, the weights and the width bound (H % 4 == 0, 4 <= H <= 4352; ZT_ERR_UNSUPPORTED otherwise, before any launch) are
 * zt_affinity_rank's, and every pair's probability has the bits zt_affinity_rank writes for it (csrc/rank_pair.hpp).  The
 * shared pool only: every query takes all Nc rows in order, C == Nc (a per-query table goes through zt_affinity_rank and
 * zt_rank_metrics).
 *   Present: the shared form of zt_affinity_topk_masked's rule -- the candidate's projected row is not NaN, nor the
 *   probability; the global column idx_base + c differs from every one of skip_dev[q][0 .. n_skip) (int32 [Q][n_skip],
 *   0 <= n_skip <= ZT_COUNT_MAX_SKIP, -1: none; skip_dev may be NULL when n_skip == 0); and bit c & 31 of word c >> 5 of row q
 *   of absent_dev [Q][absent_words] is clear, c the LOCAL column (ABSENT BITS, above; absent_dev == NULL: no bits).
 *   above_dev[q] = #{present c : p > thr[q]}, equal_dev[q] = #{present c : p == thr[q]} (int32 [Q]): IEEE float compares, so a
 *   NaN threshold counts nothing and -0.0 equals +0.0.  accumulate != 0: the counts are ADDED to what the outputs hold; a pool
 *   given in pieces, in any order, each with its idx_base and its own local bits, gives the numbers of one call.  Integer
 *   sums: the result is a function of the inputs alone, whatever the workspace, slabs, spans or grid.
 * Q = 0: ZT_OK, nothing touched.  Nc = 0: ZT_OK, zeros written, or the outputs left alone under accumulate.  ZT_ERR_ARG before
 * any device call: a NULL emb_q_dev, emb_c_dev, w, thr_dev, above_dev, equal_dev or workspace_dev; a negative Q, Nc or
 * idx_base; n_skip outside 0 .. ZT_COUNT_MAX_SKIP, or n_skip > 0 with skip_dev NULL; a non-NULL absent_dev with
 * absent_words < ceil(Nc / 32); idx_base + Nc > INT32_MAX; a workspace below the minimum.
 * workspace_dev, 16-byte aligned, of workspace_bytes bytes as the caller states them: a head of 256 bytes, P_q, and P_c of ONE
 * SLAB of candidate rows -- per slab the f32 MFMA GEMM and one launch of the pair kernel over spans of candidate columns,
 * whose workgroups add their counts into the outputs with integer atomics (no partial counts in the workspace, no reduce
 * launch).  zt_affinity_count_workspace_bytes(Q, Nc, H) is the recommended size (-1: H unsupported, or a negative size); it
 * stops growing once Nc exceeds the slab cap (128 MiB of P_c, or 2^18 rows).  Its value for Nc = 32 is the smallest size
 * accepted.  zt_affinity_count_plan is where the slab rows, the spans and the grid are decided (host code only).  No float
 * atomics, no workgroup waits for another. */
#define ZT_COUNT_MAX_SKIP 4
#define ZT_COUNT_PLAN_FIELDS 9
/* plan_out[ZT_COUNT_PLAN_FIELDS], all int64:
 *   [0] q_tiles      tiles of 4 queries
 *   [1] slab_rows    rows of P_c the workspace holds (a multiple of 32)
 *   [2] n_slabs      slabs the pool is walked in: n_slabs * slab_rows >= Nc
 *   [3] span_cols    candidate columns of a slab per span (a multiple of 128, a workgroup's step)
 *   [4] n_spans      spans per slab
 *   [5] grid         workgroups of the pair kernel, per slab: q_tiles * n_spans
 *   [6] h_chunks     chunks of 1024 columns the hidden width runs in
 *   [7] pc_offset    byte offset of the slab's P_c in the workspace
 *   [8] min_bytes    the smallest workspace accepted
 * ZT_ERR_ARG for NULL plan_out, a negative size or a workspace below min_bytes; H as above. */
int64_t zt_affinity_count_workspace_bytes(int64_t Q, int64_t Nc, int32_t H);
int zt_affinity_count(const float *emb_q_dev, int64_t Q, const float *emb_c_dev, int64_t Nc, int32_t H,
                      const zt_affinity_weights *w, const float *thr_dev,
                      const int32_t *skip_dev, int32_t n_skip, int64_t idx_base, int32_t accumulate,
                      int32_t *above_dev, int32_t *equal_dev,
                      void *workspace_dev, int64_t workspace_bytes,
                      const uint32_t *absent_dev, int64_t absent_words, void *stream);
int zt_affinity_count_plan(int64_t Q, int64_t Nc, int32_t H, int64_t workspace_bytes, int64_t *plan_out);
/* Exclusion lists from the adjacency (csrc/seen.hip).  For query (v, t) = (q_nodes_dev[q], q_ts_dev[q]): begin_dev[q] =
 * indptr[v], len_dev[q] = the number of v's entries with a timestamp strictly below t -- the prefix zt_csr_find_before
 * returns, so an entry AT t is not seen.  The partners themselves are entries [begin, begin + len) of the handle's neighbour
 * array, duplicates included.  v < 0 or v >= num_nodes: len 0, and ZT_ERR_RANGE in *status_dev (the caller zeroes it; read it
 * once the stream has passed the call).  NULL pointers or Q < 0: ZT_ERR_ARG before any device call; Q = 0: ZT_OK, nothing
 * touched. */
int zt_csr_seen_ranges(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t Q,
                       int64_t *begin_dev, int64_t *len_dev, int32_t *status_dev, void *stream);
/* Absent bits (above) from per-query id lists: query q's list is ids[begin_dev[q] .. begin_dev[q] + len_dev[q]), ids being
 * ids_dev, or the handle's neighbour array when ids_dev is NULL (c may be NULL otherwise) -- a "seen" list is never copied;
 * ranges of the handle's array are clipped to it.  Lists may hold duplicates, any order, and ids that are not in the pool,
 * negative ones among them: those are ignored.  EVERY word of absent_dev [Q][absent_words] is written; the caller does not
 * zero it.  How an id becomes columns:
 *   range           cand_sorted_dev == NULL: column id - id_lo where that is in [0, C);
 *   shared list     cand_stride == 0: cand_sorted_dev [C] holds the pool's ids in ascending order (-1 entries first) and
 *                   cand_col_dev [C] the column each came from; every column whose id equals a list entry is set;
 *   per-query list  cand_stride == C: the same with row q of [Q][C] tables.
 * Integer ORs: the result is a function of the inputs alone.  NULL begin / len / absent, both c and ids_dev NULL, negative
 * Q, C or absent_words, absent_words < ceil(C / 32), a list without its columns or another stride: ZT_ERR_ARG before any
 * device call.  Q = 0 or absent_words = 0: ZT_OK, nothing touched. */
int zt_exclude_mark(const zt_csr *c, const int32_t *ids_dev, const int64_t *begin_dev, const int64_t *len_dev, int64_t Q,
                    int64_t id_lo, const int32_t *cand_sorted_dev, const int32_t *cand_col_dev, int64_t cand_stride,
                    int64_t C, uint32_t *absent_dev, int64_t absent_words, void *stream);
/* Negative sampling on the device (csrc/neg_sample.hip): up to K negatives for each of Q edges (src_dev[q], dst_dev[q]),
 * drawn reproducibly from the edge's own id list and from the destination pool pool_dev [n_pool], with the exclusions
 * applied while drawing.
 * THE ROW'S LIST.  For row q the list is ids[begin_dev[q] .. begin_dev[q] + len_dev[q]); ids is ids_dev, or the handle's
 * neighbour array when ids_dev is NULL: zt_exclude_mark's convention -- a negative begin or len gives an empty list, a range
 * of the handle's array is clipped to it (`len` below is the clipped length), duplicates and negative ids may occur.  c,
 * ids_dev, begin_dev and len_dev all NULL (or begin_dev and len_dev NULL) means every list is empty.
 * THE RULE.  Slots j < K_hist are HISTORICAL slots and the others are POOL slots.  All slots start empty.  In round
 * r = 0 .. rounds - 1, every slot that is still empty draws one id:
 *   - x is word 0 of Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter
 *     (row & 0xffffffff, row >> 32, j, r), row = row_base + q;
 *   - a historical slot with r < hist_rounds and len > 0 draws id = ids[begin + ((x * len) >> 32)]  (a LIST draw);
 *   - every other slot draws id = pool[(x * n_pool) >> 32]  (a POOL draw);
 *   - both products are 64-bit; len and n_pool are below 2^31.
 * The draw PASSES unless one of these holds:
 *   - id < 0;
 *   - id == dst[q];
 *   - ZT_NEG_EXCLUDE_SOURCE is set and id == src[q];
 *   - ZT_NEG_FILTER is set, it is a pool draw, and id occurs in the row's list;
 *   - ZT_NEG_DISTINCT is set and a slot filled in an earlier round holds id.
 * A passing draw is ACCEPTED unless ZT_NEG_DISTINCT is set and a lower-numbered slot's draw of the same round passed with
 * the same id.  Accepted draws fill their slots.  After the last round, empty slots read -1.
 * Every element of neg_dev [Q][K] is written; count_dev[q] (where not NULL) is (slots filled from the list, slots filled from
 * the pool).  The result is a function of the arguments alone -- not of the grid, not of the batch a row arrives in: a pass
 * over a split numbers its rows by row_base.  One workgroup per row, no global atomics, no row waits for another; under
 * ZT_NEG_FILTER a round that still has pool draws pending reads the row's list once.
 * zt_neg_sample_plan (host code only): out[0] = the form (0: K outside 1 .. ZT_NEG_MAX_K, refused -- still ZT_OK;
 * 1: one wave, K <= 128; 2: a workgroup of several waves), out[1] = threads of the workgroup, out[2] = the sort width (the
 * power of two >= max(K, 64)), out[3] = dynamic LDS bytes.  NULL out: ZT_ERR_ARG.
 * ZT_ERR_ARG before any device call: NULL d, src_dev, dst_dev, pool_dev or neg_dev; Q < 0; n_pool <= 0 with Q > 0; K outside
 * 1 .. ZT_NEG_MAX_K; K_hist outside 0 .. K; rounds outside 1 .. ZT_NEG_MAX_ROUNDS; hist_rounds outside 0 .. rounds; unknown
 * flag bits; begin_dev without len_dev or the reverse; lists with neither c nor ids_dev.  n_pool >= 2^31, a handle of 2^31
 * entries or more, or Q beyond one launch's workgroups: ZT_ERR_UNSUPPORTED (a list of the caller's ids_dev is read up to
 * 2^31 - 1 entries).  Q = 0: ZT_OK, nothing touched. */
#define ZT_NEG_MAX_K 4096
#define ZT_NEG_MAX_ROUNDS 8
#define ZT_NEG_FILTER 1         /* a pool draw that is in the row's list is rejected */
#define ZT_NEG_DISTINCT 2       /* no id twice in a row */
#define ZT_NEG_EXCLUDE_SOURCE 4 /* the row's source is rejected */
typedef struct zt_neg_desc {
    uint64_t seed;
    int64_t row_base;
    int32_t K, K_hist, rounds, hist_rounds, flags;
} zt_neg_desc;
int zt_neg_sample_plan(int32_t K, int64_t *out);
int zt_neg_sample(const zt_neg_desc *d, const int32_t *src_dev, const int32_t *dst_dev, int64_t Q,
                  const int32_t *pool_dev, int64_t n_pool,
                  const zt_csr *c, const int32_t *ids_dev, const int64_t *begin_dev, const int64_t *len_dev,
                  int32_t *neg_dev, int32_t *count_dev, void *stream);
/* Ranks, MRR and Hits@k of prob_dev [Q][C] (cand_idx_dev as above, may be NULL: every entry present).  Column 0 is the
 * positive:  rank = 1 + #{c >= 1 present : p_c > p_0} + 0.5 #{c >= 1 present : p_c == p_0}, the mean of the optimistic and
 * the pessimistic rank.  A query whose column 0 is absent is skipped and not counted.  rank_dev [Q] (or NULL) receives the
 * ranks, 0 for a skipped query.  acc_dev [5] (float64) is ADDED to: sum of 1 / rank, Hits@1, Hits@3, Hits@10 (rank <= n),
 * queries counted -- so a pass accumulates over its batches without a host read; the caller zeroes it.  One workgroup; the
 * per-query ranks are written, then one lane adds them to the sums first to last: a fixed order, the same bits on every
 * run.  Q = 0 or C = 0: ZT_OK, nothing touched; NULL prob_dev / acc_dev or a negative size: ZT_ERR_ARG before any device
 * call. */
int zt_rank_metrics(const float *prob_dev, const int32_t *cand_idx_dev, int64_t Q, int64_t C, float *rank_dev,
                    double *acc_dev, void *stream);
/* The same sums from counts (zt_affinity_count's above_dev / equal_dev, with the thresholds they were taken at):
 * rank = 1 + above + 0.5 equal in FLOAT64 -- a pool of ten million ids does not fit a float32 rank.  A query whose threshold
 * is NaN is skipped and not counted; its rank is 0.  rank_dev [Q] (float64, or NULL) receives the ranks.  acc_dev [5] is ADDED
 * to in zt_rank_metrics's layout and order (sum of 1 / rank, Hits@1, Hits@3, Hits@10, queries counted), one lane adding first
 * to last: where every rank is below 2^23 the sums have the bits zt_rank_metrics gives for the same ranks in the same order.
 * Q = 0: ZT_OK, nothing touched; NULL thr_dev / above_dev / equal_dev / acc_dev or Q < 0: ZT_ERR_ARG before any device
 * call. */
int zt_rank_metrics_counts(const float *thr_dev, const int32_t *above_dev, const int32_t *equal_dev, int64_t Q,
                           double *rank_dev, double *acc_dev, void *stream);
#define ZT_METRICS_FORM_REFUSED 0
#define ZT_METRICS_FORM_SINGLE 1 /* one bitonic sort of 2B 64-bit (key | label) words */
#define ZT_METRICS_FORM_SPLIT 2  /* positives and negatives sorted as two runs of 32-bit keys */
#define ZT_METRICS_MAX_B 16384
#define ZT_METRICS_PLAN_FIELDS 4
/* out[ZT_METRICS_PLAN_FIELDS], all int64:
 *   [0] form        ZT_METRICS_FORM_*  (refused: B <= 0 or B > ZT_METRICS_MAX_B; the other fields are 0 then)
 *   [1] threads     of the one workgroup
 *   [2] n2          keys in LDS, padding included (single: the next power of two >= max(1024, 2B); split: twice the next
 *                   power of two >= B)
 *   [3] lds_bytes   dynamic LDS (single: 8 n2; split: 4 n2)
 * ZT_ERR_ARG for NULL out; else ZT_OK -- a refused form is an answer, not a failure. */
int zt_link_metrics_plan(int64_t B, int64_t *out);
/* The scorer as the tail of the native step: with non-NULL weights every zt_pipeline_step_ahead over a WHOLE batch
 * (rows [0, 3B)) also scores that batch's 2B pairs behind its aggregation (main stream).  prob_dev: [2][2 * max_B]
 * floats, consecutive steps alternate between the halves.  workspace_dev as for
 * zt_affinity with ws_max_B = the pipeline's max_B.  NULL weights: off.
 * zt_pipeline_last_scores: makes `stream` wait for the last scoring and returns where its 2B probabilities are. */
int zt_pipeline_set_scoring(zt_pipeline *p, const zt_affinity_weights *weights, void *workspace_dev,
                            float *prob_dev);
int zt_pipeline_last_scores(zt_pipeline *p, void *stream, float **prob_out, int64_t *B_out);
/* The metrics as the tail of the scorer: with non-NULL sum_dev every SCORED step (scoring on, a whole batch) is followed by
 * the zt_link_metrics kernel over that step's probabilities -- the first B floats of its half of prob_dev against the next B.
 * The kernel ADDS the batch's (AP, AUC, accuracy) to sum_dev [3] (float64; the caller zeroes it) and, where per_batch_dev
 * [cap][3] is given, writes them to row i, i = the batches measured since this call.  It runs on the message stream behind the
 * scorer, never on the main stream; all of them on that one stream, in batch order: a run gives the same bits every time.
 * The main stream waits for a half's metrics kernel before the scorer rewrites that half two steps later.
 * NULL sum_dev: off (zt_pipeline_set_scoring with NULL weights turns it off as well).  Refused before anything is enqueued:
 * scoring off, cap < 0 (ZT_ERR_ARG); max_B > ZT_METRICS_MAX_B, an exchange attached -- a sharded step is never scored --
 * (ZT_ERR_UNSUPPORTED); and, by the step itself, a scored step that would write row cap (ZT_ERR_ARG).
 * zt_pipeline_metrics: makes `stream` wait for the last metrics kernel enqueued and returns in *n_out the batches measured
 * since the set call (the counterpart of zt_pipeline_last_scores). */
int zt_pipeline_set_metrics(zt_pipeline *p, double *sum_dev, double *per_batch_dev, int64_t cap);
int zt_pipeline_metrics(zt_pipeline *p, void *stream, int64_t *n_out);

/* ------------------------------------------------------------------------ */
/* Node classification: the decoder head (csrc/decoder.hip)                   */
/* ------------------------------------------------------------------------ */
#define ZT_DECODER_H1 80   /* the reference's hidden widths (MLP, utils/util.py:28-42): no others are taken */
#define ZT_DECODER_H2 10
typedef struct {
    const float *fc1_w, *fc1_b;  /* fc_1 [80][H], [80] */
    const float *fc2_w, *fc2_b;  /* fc_2 [10][80], [10] */
    const float *fc3_w, *fc3_b;  /* fc_3 [1][10], [1]  */
} zt_decoder_weights;            /* device pointers */
/* The reference's node-classification decoder (evaluation/evaluation.py:51-79 applies it to the source embeddings):
 *   z = fc3(drop(relu(fc2(drop(relu(fc1(x)))))))   x_dev [N][H] -> 80 -> 10 -> z [N]
 * for any H with H % 4 == 0 and 4 <= H <= 4352, the widths the one-vs-many scorer takes (ZT_ERR_UNSUPPORTED otherwise, before
 * any device call); K runs over H in chunks, LDS does not bound it.  N = 0: ZT_OK, nothing touched.  The parameters are read
 * as they lie in the module (no packed copy, no weights_ready); x_dev and fc1_w are 16-byte aligned, the other five need
 * no alignment, and nothing past row 10 of fc2_w, fc2_b or fc3_w is read.  Layer 1 runs on the f32 MFMA, layer 2 as one
 * N-tile padded to 16 fed through LDS, layer 3 as ten terms in column order.  No atomics: two calls give the same bits, and
 * the eval entry and the training entry at p = 0 give the same bits.
 *   eval:     writes logit_dev [N] and / or prob_dev [N] = sigmoid(z); either may be NULL.  One launch.
 *   training: dropout p in [0, 1) (0: none) from a 64-bit seed: element row * 80 + col of layer 1 and N * 80 + row * 10 + col of
 *             layer 2 is kept, and scaled by 1 / (1 - p), where its hash passes the threshold (the aggregation's dropout;
 *             zebra_amd/decoder.py decoder_dropout_mask is the same arithmetic in numpy).  Writes logit_dev [N] and keeps
 *             h1_dev [N][80] and h2_dev [N][10], both after ReLU and dropout, for the backward.  One launch.
 *   backward: from dlogit_dev [N], x_dev and the forward's h1_dev / h2_dev (p and seed as given there): d_x_dev [N][H],
 *             d_fc1_w_dev [80][H], d_fc1_b_dev [80], d_fc2_w_dev [10][80], d_fc2_b_dev [10], d_fc3_w_dev [10], d_fc3_b_dev [1],
 *             written, not accumulated.  An output that is not needed is NULL and its work is skipped (d_x_dev = NULL is the
 *             usual case: the embeddings come from a frozen model).  At most three launches, no host synchronisation, no
 *             atomics: every sum has a fixed order, two runs give the same bits.  d_x_dev and d_fc1_w_dev are 16-byte aligned.
 * workspace_dev (backward only): zt_node_decoder_train_workspace_bytes(max_N, H) bytes (-1 = H unsupported or max_N < 0),
 * 16-byte aligned, sized for ws_max_N >= N; it holds d(hidden 1) [N][80], d(hidden 2) [N][10] and the partial products of
 * d_fc1_w.
 * zt_node_decoder_plan (host code only, the one place that decides): out[ZT_DECODER_PLAN_FIELDS], all int64:
 *   [0] arrangement  5: five waves own one N-tile each and share 16 staged rows (the pick at every N: the other form, one
 *                    wave owning the five N-tiles of its 16 rows, value 1, measured no faster and is reached by the tests only)
 *   [1] waves        per workgroup
 *   [2] rows         per workgroup
 *   [3] k_chunk      columns of x staged in LDS at a time
 *   [4] grid         workgroups of the forward
 *   [5] lds_bytes    dynamic LDS of the forward
 *   [6] split        partial products of d_fc1_w in the backward (1: written directly)
 *   [7] k_per        rows per partial product
 * ZT_ERR_ARG for NULL out or N < 0, ZT_ERR_UNSUPPORTED for the width. */
#define ZT_DECODER_PLAN_FIELDS 8
int zt_node_decoder_plan(int64_t N, int32_t H, int32_t training, int64_t *out);
int zt_node_decoder(const float *x_dev, int64_t N, int32_t H, const zt_decoder_weights *weights,
                    float *logit_dev, float *prob_dev, void *stream);
int zt_node_decoder_train_forward(const float *x_dev, int64_t N, int32_t H,
                                  const zt_decoder_weights *weights, float p, uint64_t seed,
                                  float *logit_dev, float *h1_dev, float *h2_dev, void *stream);
int64_t zt_node_decoder_train_workspace_bytes(int64_t max_N, int32_t H);
int zt_node_decoder_train_backward(const float *x_dev, int64_t N, int32_t H,
                                   const zt_decoder_weights *weights, const float *h1_dev,
                                   const float *h2_dev, const float *dlogit_dev, float p, uint64_t seed,
                                   float *d_x_dev, float *d_fc1_w_dev, float *d_fc1_b_dev,
                                   float *d_fc2_w_dev, float *d_fc2_b_dev, float *d_fc3_w_dev,
                                   float *d_fc3_b_dev, void *workspace_dev, int64_t ws_max_N,
                                   void *stream);

/* The tail of a TRAINING step (csrc/train_tail.hip): the loss of train.py:212-213 and the optimizer step of train.py:215.
 *
 * Pair loss.  prob_dev [2B] holds B positive probabilities, then B negative ones (what zt_affinity_train_forward writes):
 *   loss_dev[0] = mean_i -max(log p_i, -100) + mean_j -max(log(1 - n_j), -100)
 * -- torch.nn.BCELoss with labels 1 and 0, added up -- and dprob_dev [2B] = (x - y) / max((1 - x) x, 1e-12) / B, the gradient
 * at grad_output = 1.  One launch for any B >= 1; logarithms, quotients and sums in float64 with a fixed association, rounded
 * to float32 once: two runs give the same bits, no atomics.  The backward is one launch, d_prob_dev = grad_loss_dev[0] *
 * dprob_dev: the scalar is read on the device, nothing synchronises.  B < 1 or a NULL pointer: ZT_ERR_ARG before any device
 * call. */
int zt_link_bce_forward(const float *prob_dev, int64_t B, float *loss_dev, float *dprob_dev, void *stream);
int zt_link_bce_backward(const float *dprob_dev, const float *grad_loss_dev, int64_t B, float *d_prob_dev, void *stream);
/* Label loss: torch.nn.BCELoss() (mean) of prob_dev [N] against a float label per row, label_dev [N]:
 *   loss_dev[0] = mean_i -(y_i max(log x_i, -100) + (1 - y_i) max(log(1 - x_i), -100))
 * and dprob_dev [N] = (x - y) / max((1 - x) x, 1e-12) / N, the gradient at grad_output = 1.  The pair loss's arithmetic and
 * launches: float64 logarithms, quotients and sums with a fixed association, rounded once; one launch each way, the backward
 * d_prob_dev = grad_loss_dev[0] * dprob_dev.  N < 1 or a NULL pointer: ZT_ERR_ARG before any device call. */
int zt_label_bce_forward(const float *prob_dev, const float *label_dev, int64_t N, float *loss_dev, float *dprob_dev,
                         void *stream);
int zt_label_bce_backward(const float *dprob_dev, const float *grad_loss_dev, int64_t N, float *d_prob_dev, void *stream);
/* Listwise loss of a ranking step over logit_dev [Q][C] (what zt_affinity_rank_train_forward writes: -inf where a pair is
 * absent).  target_dev [Q] (int32; NULL: column 0) names the positive's column; a query whose target is absent or outside
 * [0, C) is skipped, n_live queries remain; with none the loss is 0 and dl is all zeros.
 *   ZT_RANK_LOSS_SOFTMAX: loss = mean over live q of logsumexp over present c of logit[q][c] - logit[q][t_q],
 *                         dl = (softmax - onehot) / n_live;
 *   ZT_RANK_LOSS_BCE:     loss = mean over live q of -max(log sigma(logit[q][t_q]), -100) + mean over the n_neg present
 *                         non-target pairs of live queries of -max(log(1 - sigma(logit)), -100); dl = (sigma - 1) / n_live at a
 *                         target and sigma / n_neg elsewhere.  With C = 2 and nothing absent this is the pair loss of the same
 *                         probabilities -- formed from the logits in float64, so equal to it within float32 rounding, not in bits.
 * dl_dev [Q][C] is the gradient at grad_output = 1 (0 at absent pairs and skipped queries).  The pair loss's arithmetic:
 * float64 exponentials, logarithms and sums with a fixed association, rounded to float32 once, one launch, no atomics.  The
 * backward is one launch, d_logit_dev[i] = grad_loss_dev[0] * dl_dev[i] for n = Q C elements.  Q < 1, C < 1, an unknown mode
 * or a NULL pointer (target_dev apart): ZT_ERR_ARG before any device call. */
#define ZT_RANK_LOSS_SOFTMAX 0
#define ZT_RANK_LOSS_BCE 1
int zt_rank_loss_forward(const float *logit_dev, const int32_t *target_dev, int64_t Q, int64_t C, int32_t mode,
                         float *loss_dev, float *dl_dev, void *stream);
int zt_rank_loss_backward(const float *dl_dev, const float *grad_loss_dev, int64_t n, float *d_logit_dev, void *stream);
/* Adam for a whole list of float32 tensors in one launch per ZT_ADAM_MAX_TENSORS non-empty tensors: torch.optim.Adam's
 * single-tensor update without weight decay, amsgrad or maximize, in torch's order,
 *   m = m + (g - m) (1 - beta1);  v = v beta2 + (1 - beta2) g g;  p = p - step_size (m / (sqrt(v) / bias2_sqrt + eps))
 * with the multiply-add of each statement fused (one rounding), as torch's device kernels compile.
 * step_size = lr / (1 - beta1^t) and bias2_sqrt = sqrt(1 - beta2^t) are the caller's, computed in double, per tensor: the
 * tensors of a call may be at different steps.  1 - beta is formed in double from the shortest decimal that rounds to the
 * float given (0.999f stands for 0.999), which is the factor torch, holding the betas as Python floats, multiplies by.
 * The table is host memory and travels in the kernels' arguments: no copy, no synchronisation, nothing to keep alive after
 * the call returns.  The device pointers need no alignment (16-byte accesses where all four of a tensor have it).
 * n = 0: ZT_OK, no launch; an entry with numel = 0 is skipped.  ZT_ERR_ARG before any device call: n < 0, a NULL pointer in
 * an entry, numel < 0 or numel >= 2^31. */
typedef struct zt_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t numel;
    float step_size;
    float bias2_sqrt;
} zt_adam_tensor;
#define ZT_ADAM_CHUNK 4096      /* elements per workgroup */
#define ZT_ADAM_MAX_TENSORS 64  /* non-empty tensors per launch */
int zt_adam_step(const zt_adam_tensor *tensors_host, int32_t n, float beta1, float beta2, float eps, void *stream);
/* The launches a zt_adam_step over tensors of these sizes makes (host code only, no GPU call; the step goes through the same
 * walk): out[0] = launches, out[1 + i] = workgroups of launch i -- the sum of ceil(numel / ZT_ADAM_CHUNK) over its tensors,
 * which are the next ZT_ADAM_MAX_TENSORS non-empty ones in the order given.  out holds 1 + ceil(n / ZT_ADAM_MAX_TENSORS)
 * values at most.  ZT_ERR_ARG for n < 0, NULL out, or a size outside [0, 2^31). */
int zt_adam_plan(const int64_t *numel_host, int32_t n, int64_t *out);

/* ------------------------------------------------------------------------ */
/* One-node multi-GPU exchange of touched rows.  The reference  */
/* has no distributed code; this is the data-path step around the one RCCL     */
/* all-gather per batch.  A row travels as float32                             */
/*   [ id (int32 bits) | row of table 0 | row of table 1 | ... ],              */
/* tables being [num_rows][width] float32 arrays (memory, last_update,         */
/* messages, message timestamps).                                              */
/* ------------------------------------------------------------------------ */
typedef struct zt_row_tables {
    float *ptr[8];       /* device pointers */
    int32_t width[8];    /* floats per row */
    int32_t n;           /* tables in use, 1..8 */
} zt_row_tables;

/* out_dev [cap][1 + sum(width)]: slot r carries ids_dev[r] and its rows for
 * r < *n_valid_dev, id = -1 and zeros beyond (fixed-size payload). */
int zt_pack_rows(const zt_row_tables *tables, const int32_t *ids_dev,
                 const int32_t *n_valid_dev, int64_t cap, float *out_dev,
                 void *stream);
/* Every received row with id >= 0 overwrites that row of the local tables. */
int zt_scatter_rows(const zt_row_tables *tables, const float *recv_dev,
                    int64_t rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ZEBRA_AMD_H */
