// What the one-vs-many scorers do AROUND rank_pair.hpp's pair sum, each rule -- what a NaN candidate is, where the absent word
// is read, how a span is cut -- written once:
//   rk_load_chunk   the (P_q + b1) rows of a query tile and w2 into LDS, one chunk of RK_HC columns (all four kernels)
//   rk_tile_pairs   the TILE body of k_rank_pairs (rank.hip) and k_rank_train_fwd (rank_train.hip): the kernel supplies what a pair reads
//   rk_span_walk    the SPAN walk of k_topk_pairs (rank_topk.hip) and k_count_pairs (rank_count.hip): the kernel supplies what
//                   happens to a candidate's probability
// and the host plumbing of their calls: slab cap, span cutter, head of the workspace, checks and messages, fc1-half projection.
#pragma once

#include <algorithm>

#include "rank_pair.hpp"

namespace zt {

// ---- host ------------------------------------------------------------------------------------------------------------------
constexpr long long RK_SLAB_BYTES = 128ll << 20;     // P_c of one slab at most: half the Infinity Cache
constexpr long long RK_SLAB_ROWS = 1ll << 18;        // ... and its rows at most (narrow H): launches are long paid for by then

inline long long round_up_ll(long long x, long long m) { return (x + m - 1) / m * m; }
inline long long rank_cap_rows(int H) { return std::max(32ll, std::min(RK_SLAB_ROWS, RK_SLAB_BYTES / ((long long)H * 4) / 32 * 32)); }
// rows of a slab in `bytes` of workspace behind P_q and the lists (whole words of absent bits); what *_workspace_bytes recommends
inline long long rank_slab_rows(int H, long long bytes) { return std::min(rank_cap_rows(H), bytes / ((long long)H * 4) / 32 * 32); }
inline long long rank_pool_rows(long long Nc, int H) { return std::min(rank_cap_rows(H), round_up_ll(std::max(Nc, 32ll), 32)); }
// spans per query tile at most: target_wgs workgroups are worth cutting spans for
inline long long rank_max_spans(long long target_wgs, long long q_tiles) { return std::max(1ll, (target_wgs + q_tiles - 1) / std::max(1ll, q_tiles)); }
// cols columns cut into spans of whole steps, min_steps steps each at least: spans begin at multiples of the step, so a wave's
// 32 columns of a step lie in one word of absent bits
inline void rank_cut_spans(long long cols, long long step_cols, int min_steps, long long max_spans, long long &span_cols,
                           long long &n_spans)
{
    const long long n = std::min(max_spans, std::max(1ll, cols / (step_cols * min_steps)));
    span_cols = round_up_ll((std::max(cols, 1ll) + n - 1) / n, step_cols);
    n_spans = std::max(1ll, (cols + span_cols - 1) / span_cols);
}
// byte offset of what follows the status word and P_q in a workspace
inline long long rank_layout_head(long long Q, int H) { return (long long)RK_HEAD + round_up_ll(Q * (long long)H * 4, 256); }

inline int rank_width_refused(const char *who, int H)
{
    set_error("%s: H=%d unsupported (H %% 4 == 0 and %d <= H <= %d)", who, H, RANK_MIN_H, RANK_MAX_H);
    return ZT_ERR_UNSUPPORTED;
}
// false, with the message set: a NULL weight, or a pointer the kernels read as float4 that is not 16-byte aligned
inline bool rank_weights_ok(const char *who, const zt_affinity_weights *w, const void *workspace)
{
    if (w->fc1_w && w->fc1_b && w->fc2_w && w->fc2_b && !((uintptr_t)workspace & 15) && !((uintptr_t)w->fc1_b & 15) &&
        !((uintptr_t)w->fc2_w & 15))
        return true;
    set_error("%s: NULL weight, or workspace / fc1 bias / fc2 weight not 16-byte aligned", who);
    return false;
}
// out [rows][H] = emb W^T for one half of fc1.weight [H][2H]: W_a = columns [0, H), W_b = columns [H, 2H) (second_half) -- the
// same matrix, a pointer offset, ldb = 2H
inline int rank_project(const float *emb, const zt_affinity_weights *w, bool second_half, float *out, int64_t rows, int H, void *stream)
{
    return zt_gemm_f32(emb, w->fc1_w + (second_half ? H : 0), out, rows, H, H, H, 2 * (int64_t)H, H, 0, 1, 0, stream);
}

#if defined(__HIPCC__)

// ---- device ----------------------------------------------------------------------------------------------------------------
struct RkTileLds {
    float4 q[RK_TQ][RK_HC / 4];       // (P_q + b1) of the tile's query rows, one chunk of RK_HC columns
    float4 w[RK_HC / 4];              // w2 of the chunk
};

// columns [h0, h0 + hn) of query rows q0 .. q0 + RK_TQ - 1 (zeros beyond Q) and of w2 into LDS, by a workgroup of THREADS
template <int THREADS>
__device__ __forceinline__ void rk_load_chunk(RkTileLds &s, const float *__restrict__ Pq, const float *__restrict__ b1,
                                              const float *__restrict__ w2, long long Q, long long q0, int H, int h0, int hn)
{
    for (int v = threadIdx.x; v < (RK_TQ + 1) * (hn / 4); v += THREADS) {
        const int r = v / (hn / 4), c4 = v - r * (hn / 4);
        const float4 b = *reinterpret_cast<const float4 *>((r < RK_TQ ? b1 : w2) + h0 + 4 * c4);
        if (r == RK_TQ) { s.w[c4] = b; continue; }
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + r < Q) p = *reinterpret_cast<const float4 *>(Pq + (q0 + r) * H + h0 + 4 * c4);
        s.q[r][c4] = rk_query_bias(p, b);
    }
}

// One workgroup of RK_TQ waves: RK_TQ queries x RK_TC candidate slots.  Wave w owns query q0 + w; each of its four 16-lane groups
// owns RK_NC slots.  The (P_q + b1) rows of the tile and w2 lie in LDS one chunk of RK_HC columns at a time; a lane walks the
// chunk in steps of 64 columns, its float4 of the query row and of w2 from LDS (the four groups of a wave read the same address:
// a broadcast) against one 16-byte vector of each of its candidates' rows from memory.  A pair's sum: lane l of its group adds
// columns 4l .. 4l + 3 of every 64 in ascending order into one accumulator, then the sixteen lanes are folded by xor 8, 4, 2, 1
// -- one association whatever the tile, no atomics: the same bits on every run.  An index outside [-1, Nc) sets the status word
// and counts as absent.  out[q][c] = value(present, sum, b2): what a present and an absent pair read is the kernel's.
template <class Value>
__device__ __forceinline__ void rk_tile_pairs(RkTileLds &s_t, const float *__restrict__ Pq, const float *__restrict__ Pc,
                                              const int *__restrict__ cand_idx, long long Q, long long Nc, long long C, int H,
                                              long long ctiles, const float *__restrict__ b1, const float *__restrict__ w2,
                                              const float *__restrict__ b2, float *__restrict__ out, int *status, Value value)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, gl = lane & 15;
    const long long qt = blockIdx.x / ctiles, ct = blockIdx.x - qt * ctiles;
    const long long q0 = qt * RK_TQ, q = q0 + wave;
    const long long c0 = ct * RK_TC + grp * RK_NC;

    long long row[RK_NC];           // row of P_c, or -1: nothing to read (absent, out of range, beyond C or Q)
    bool bad = false;
#pragma unroll
    for (int j = 0; j < RK_NC; ++j) {
        const long long c = c0 + j;
        long long r = -1;
        if (q < Q && c < C) {
            r = cand_idx != nullptr ? (long long)cand_idx[q * C + c] : c;
            if (r < -1 || r >= Nc) { bad = true; r = -1; }
        }
        row[j] = r;
    }
    if (bad && gl == 0) atomicExch(status, (int)ZT_ERR_RANGE);

    float acc[RK_NC];
#pragma unroll
    for (int j = 0; j < RK_NC; ++j) acc[j] = 0.f;

    for (int h0 = 0; h0 < H; h0 += RK_HC) {
        const int hn = min(RK_HC, H - h0);                     // a multiple of 4
        if (h0 > 0) __syncthreads();                           // the chunk before has been read
        rk_load_chunk<WAVE * RK_TQ>(s_t, Pq, b1, w2, Q, q0, H, h0, hn);
        __syncthreads();
        for (int c4 = gl; c4 < hn / 4; c4 += RK_GROUP) {
            float4 pc[RK_NC];
#pragma unroll
            for (int j = 0; j < RK_NC; ++j) {
                pc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row[j] >= 0) pc[j] = *reinterpret_cast<const float4 *>(Pc + row[j] * H + h0 + 4 * c4);
            }
            const float4 pq = s_t.q[wave][c4], w = s_t.w[c4];
#pragma unroll
            for (int j = 0; j < RK_NC; ++j) acc[j] = rk_pair_step(acc[j], w, pq, pc[j]);
        }
    }
    const float bias2 = b2[0];
#pragma unroll
    for (int j = 0; j < RK_NC; ++j) {
        const float s = rk_fold16(acc[j]);
        const long long c = c0 + j;
        if (gl == 0 && q < Q && c < C) out[q * C + c] = value(row[j] >= 0, s, bias2);
    }
}

// what the span walk reads: the head of both kernels' arguments
struct RkWalkArgs {
    const float *Pq, *Pc;             // [Q][H]; the slab's rows [r0, r0 + rows) of P_c
    const int *cand_idx;              // [Q][C]: the indexed form (NQ == 1) alone
    long long Q, Nc, C, r0, rows, idx_base;
    long long n_spans, span_cols;
    int H;
    const float *b1, *w2, *b2;
    int *status;                      // the indexed form alone
    const unsigned *absent;           // [Q][absent_words] or NULL: read by the MASKED instantiations alone
    long long absent_words;
};

// One workgroup of WAVES waves: query tile q0 against span `span` of the candidate columns, in steps.
//   NQ = RK_TQ (shared pool): every wave scores all RK_TQ queries against ITS 32 candidates of the step -- a candidate row's
//        float4s are loaded into registers once and run against the four query rows from LDS.
//   NQ = 1 (indexed): wave w owns query q0 + w and walks the span's index columns 32 at a time, as rk_tile_pairs does; rows
//        outside the slab are passed over (another slab's launch takes them).
// MASKED: a candidate is present only if its bit of a.absent is clear -- bit c of row q, c the LOCAL column of the call
//        (a.r0 + mycol in the shared form: the slab's offset counts; mycol in the indexed form); every query of a wave tests
//        its own row.  The word is loaded ahead of the pair sum, once per wave.  false: none of this is compiled in.
// The (P_q + b1) rows and w2 lie in LDS a chunk of RK_HC columns at a time: H <= RK_HC loads them once (the barrier behind that
// load is one every workgroup passes before its first step), wider rows once per step and chunk.
// Per step and qi < NQ the walk calls consume(qi, p, present, gcol): p this lane's candidate's probability for query qi
// (q0 + qi, or q0 + wave where NQ == 1), gcol the index it is returned under, present what no kernel may count or select
// without.  The call stands under wave-uniform control flow with every lane active: the consumer may ballot.
template <int NQ, bool MASKED, int WAVES, class Consumer>
__device__ __forceinline__ void rk_span_walk(const RkWalkArgs &a, RkTileLds &s_t, long long q0, long long span, Consumer &&consume)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, gl = lane & 15;
    constexpr bool shared = NQ != 1;
    const int H = a.H;
    const long long cols = shared ? a.rows : a.C;                       // what the spans cut
    const long long lo = min(cols, span * a.span_cols), hi = min(cols, lo + a.span_cols);
    const long long step_cols = shared ? (long long)WAVES * RK_TC : RK_TC;
    const long long nsteps = (hi - lo + step_cols - 1) / step_cols;     // the same for all waves (barriers below)
    const int nchunks = (H + RK_HC - 1) / RK_HC;
    const float bias2 = a.b2[0];

    if (nchunks == 1) {
        rk_load_chunk<WAVE * WAVES>(s_t, a.Pq, a.b1, a.w2, a.Q, q0, H, 0, H);
        __syncthreads();
    }

    const int myj = rk_fold_pair(gl);                                   // the pair of its group whose sum this lane ends with
    for (long long t = 0; t < nsteps; ++t) {
        // this lane's own candidate: column, local row in the slab (-1: nothing to read)
        const long long mycol = lo + t * step_cols + (shared ? wave * RK_TC : 0) + grp * RK_NC + myj;
        int myrow = -1;
        if (mycol < hi) {
            if (shared) {
                myrow = (int)mycol;
            } else if (q0 + wave < a.Q) {
                const long long r = (long long)a.cand_idx[(q0 + wave) * a.C + mycol];
                if (r < -1 || r >= a.Nc) atomicExch(a.status, (int)ZT_ERR_RANGE);
                else if (r >= a.r0 && r < a.r0 + a.rows) myrow = (int)(r - a.r0);
            }
        }
        // a NaN anywhere in a candidate's embedding makes its whole projected row NaN; the pair sum's relu (fmaxf) would drop
        // it and zt_affinity_rank writes a finite number there -- here such a candidate is a NaN candidate: never present
        const bool nan_row = myrow >= 0 && a.Pc[(long long)myrow * H] != a.Pc[(long long)myrow * H];
        // MASKED: the wave's RK_TC = 32 columns of this step lie in ONE word of a query's bits -- spans begin at multiples of
        // the step (rank_cut_spans) and slabs at multiples of 32 rows (rank_slab_rows) --, so the word's address is the same
        // in every lane
        unsigned gone[NQ];
        if (MASKED) {
            static_assert(RK_TC == 32, "one word of absent bits per wave and step");
            const long long wcol = lo + t * step_cols + (shared ? __builtin_amdgcn_readfirstlane(wave) * RK_TC : 0);
            const long long word = ((shared ? a.r0 : 0) + wcol) >> 5;      // < ceil(C / 32) wherever wcol < hi
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                const long long q = q0 + (shared ? qi : __builtin_amdgcn_readfirstlane(wave));
                gone[qi] = (wcol < hi && q < a.Q) ? a.absent[q * a.absent_words + word] : 0u;
            }
        }
        int row[RK_NC];
#pragma unroll
        for (int j = 0; j < RK_NC; ++j)          // pair j's row from the lane of this group that owns it (bit 0 of gl clear)
            row[j] = __shfl(myrow, (lane & 48) | ((j & 4) << 1) | ((j & 2) << 1) | ((j & 1) << 1), WAVE);

        float acc[NQ][RK_NC];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
            for (int j = 0; j < RK_NC; ++j) acc[qi][j] = 0.f;

        for (int h0 = 0; h0 < H; h0 += RK_HC) {
            const int hn = min(RK_HC, H - h0);                 // a multiple of 4
            if (nchunks > 1) {
                __syncthreads();                               // the chunk before has been read
                rk_load_chunk<WAVE * WAVES>(s_t, a.Pq, a.b1, a.w2, a.Q, q0, H, h0, hn);
                __syncthreads();
            }
            for (int c4 = gl; c4 < hn / 4; c4 += RK_GROUP) {
                float4 pc[RK_NC];
#pragma unroll
                for (int j = 0; j < RK_NC; ++j) {
                    pc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (row[j] >= 0) pc[j] = *reinterpret_cast<const float4 *>(a.Pc + (long long)row[j] * H + h0 + 4 * c4);
                }
                const float4 w = s_t.w[c4];
#pragma unroll
                for (int qi = 0; qi < NQ; ++qi) {
                    const float4 pq = s_t.q[shared ? qi : wave][c4];
#pragma unroll
                    for (int j = 0; j < RK_NC; ++j) acc[qi][j] = rk_pair_step(acc[qi][j], w, pq, pc[j]);
                }
            }
        }
        // the index this lane's candidate goes under: <= INT32_MAX wherever myrow >= 0 (the host checks idx_base + C)
        const long long gcol = (shared ? a.r0 : 0) + mycol + a.idx_base;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            const float p = rk_prob(rk_fold16x8(acc[qi], gl), bias2);
            bool present = myrow >= 0 && !nan_row && (gl & 1) == 0 && p == p && q0 + (shared ? qi : wave) < a.Q;
            if (MASKED) present = present && ((gone[qi] >> (mycol & 31)) & 1u) == 0u;
            consume(qi, p, present, gcol);
        }
    }
}

#endif  // __HIPCC__

}  // namespace zt
