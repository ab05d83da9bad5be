// Per-query exclusion sets for the top-K scorer ("Read-only queries and ranking"):
//   zt_csr_seen_ranges  for a query (v, t) the slice of the adjacency that holds v's partners strictly before t -- the entries
//                       zt_csr_find_before returns: begin = indptr[v], len = lower_bound of t in v's time-sorted entries;
//   zt_exclude_mark     turns every query's list of ids into ABSENT BITS absent[Q][W]: bit c & 31 of word c >> 5 of row q set
//                       means local column c of the candidate pool is not present for query q (zt_affinity_topk_masked reads it).
// The mark kernel: one workgroup per (query, tile of MK_TILE_WORDS words).  The tile's bits sit in LDS; the workgroup strides
// over the list with consecutive lanes on consecutive entries, ORs bits into LDS and at the end writes the whole tile with
// plain vector stores -- every word of absent[Q][W] is written, no global atomics, no zero-fill by the caller, no workgroup
// waits for another.  Bits are ORed: the result does not depend on the order or the grid.  Every loop is bounded by len or C.
#include "csr_handle.hpp"

using namespace zt;

namespace {

constexpr int MK_THREADS = 256;
constexpr int MK_TILE_WORDS = 2048;                  // 65 536 columns, 8 KB of LDS: recommend's default pool_chunk is one tile

__global__ __launch_bounds__(MK_THREADS) void k_seen_ranges(const long long *__restrict__ indptr, const double *__restrict__ ats,
                                                            long long num_nodes, const int *__restrict__ q_nodes,
                                                            const double *__restrict__ q_ts, long long Q, long long *begin,
                                                            long long *len, int *status)
{
    const long long q = (long long)blockIdx.x * MK_THREADS + threadIdx.x;
    if (q >= Q) return;
    const long long v = q_nodes[q];
    if (v < 0 || v >= num_nodes) {
        atomicExch(status, (int)ZT_ERR_RANGE);
        begin[q] = 0;
        len[q] = 0;
        return;
    }
    const double t = q_ts[q];
    const long long b = indptr[v];
    long long lo = b, hi = indptr[v + 1];
    for (int it = 0; it < 64 && lo < hi; ++it) {     // lower_bound: the first entry whose timestamp is not below t
        const long long mid = lo + ((hi - lo) >> 1);
        if (ats[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    begin[q] = b;
    len[q] = lo - b;
}

struct MarkArgs {
    const int *ids;                   // the lists' array
    long long n_ids;                  // its length where known (the handle's array), else -1: begin / len are the caller's word
    const long long *begin, *len;     // [Q]
    long long Q, id_lo, C, words, n_tiles;
    const int *sorted, *col;          // NULL (range mode), or ascending ids and the columns they came from: [C], or [Q][C]
    long long stride;                 // 0 or C
    unsigned *absent;                 // [Q][words]
};

__global__ __launch_bounds__(MK_THREADS) void k_exclude_mark(const MarkArgs a)
{
    __shared__ unsigned s_bits[MK_TILE_WORDS];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x / a.n_tiles, tile = blockIdx.x - q * a.n_tiles;
    const long long w0 = tile * MK_TILE_WORDS, w1 = min(a.words, w0 + MK_TILE_WORDS);
    const long long c0 = w0 * 32, c1 = min(a.C, w1 * 32);             // the tile's columns: bits at columns >= C stay 0
    for (int w = tid; w < MK_TILE_WORDS; w += MK_THREADS) s_bits[w] = 0u;
    __syncthreads();
    long long b = a.begin[q], n = a.len[q];
    if (b < 0 || n < 0) n = 0;
    if (a.n_ids >= 0) n = b > a.n_ids ? 0 : min(n, a.n_ids - b);      // never past the handle's array
    if (c0 < c1) {
        const int *sorted = a.sorted ? a.sorted + q * a.stride : nullptr;
        const int *col = a.sorted ? a.col + q * a.stride : nullptr;
        for (long long i = tid; i < n; i += MK_THREADS) {
            const long long id = a.ids[b + i];
            if (id < 0) continue;                                      // (-1 is "absent" in a candidate list, never a member)
            if (sorted == nullptr) {
                const long long c = id - a.id_lo;
                if (c >= c0 && c < c1) atomicOr(&s_bits[(c - c0) >> 5], 1u << (c & 31));
                continue;
            }
            long long lo = 0, hi = a.C;                                // lower bound of id, then the run of equals
            for (int it = 0; it < 64 && lo < hi; ++it) {
                const long long mid = lo + ((hi - lo) >> 1);
                if (sorted[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            for (long long p = lo; p < a.C && sorted[p] == id; ++p) {
                const long long c = col[p];
                if (c >= c0 && c < c1) atomicOr(&s_bits[(c - c0) >> 5], 1u << (c & 31));
            }
        }
    }
    __syncthreads();
    unsigned *out = a.absent + q * a.words + w0;
    for (long long w = tid; w < w1 - w0; w += MK_THREADS) out[w] = s_bits[w];
}

}  // namespace

extern "C" int zt_csr_seen_ranges(const zt_csr *c, const int32_t *q_nodes_dev, const double *q_ts_dev, int64_t Q,
                                  int64_t *begin_dev, int64_t *len_dev, int32_t *status_dev, void *stream)
{
    if (!c || !q_nodes_dev || !q_ts_dev || !begin_dev || !len_dev || !status_dev || Q < 0) {
        set_error("zt_csr_seen_ranges: bad argument");
        return ZT_ERR_ARG;
    }
    const long long grid = (Q + MK_THREADS - 1) / MK_THREADS;
    if (grid > 0x7fffffffll) {
        set_error("zt_csr_seen_ranges: Q=%lld queries exceed one launch's workgroups", (long long)Q);
        return ZT_ERR_UNSUPPORTED;
    }
    if (Q == 0) return ZT_OK;
    k_seen_ranges<<<(unsigned)grid, MK_THREADS, 0, (hipStream_t)stream>>>(c->indptr, c->ts, c->N, q_nodes_dev, q_ts_dev, Q,
                                                                          reinterpret_cast<long long *>(begin_dev),
                                                                          reinterpret_cast<long long *>(len_dev), status_dev);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_exclude_mark(const zt_csr *c, const int32_t *ids_dev, const int64_t *begin_dev, const int64_t *len_dev, int64_t Q,
                               int64_t id_lo, const int32_t *cand_sorted_dev, const int32_t *cand_col_dev, int64_t cand_stride,
                               int64_t C, uint32_t *absent_dev, int64_t absent_words, void *stream)
{
    if ((!c && !ids_dev) || !begin_dev || !len_dev || !absent_dev || Q < 0 || C < 0 || absent_words < 0) {
        set_error("zt_exclude_mark: bad argument");
        return ZT_ERR_ARG;
    }
    if (absent_words < (C + 31) / 32) {
        set_error("zt_exclude_mark: absent_words=%lld, C=%lld columns need %lld", (long long)absent_words, (long long)C,
                  (long long)((C + 31) / 32));
        return ZT_ERR_ARG;
    }
    if (cand_sorted_dev != nullptr && (!cand_col_dev || (cand_stride != 0 && cand_stride != C))) {
        set_error("zt_exclude_mark: a candidate list needs its columns and a stride of 0 (shared) or C (per query)");
        return ZT_ERR_ARG;
    }
    const long long n_tiles = (absent_words + MK_TILE_WORDS - 1) / MK_TILE_WORDS;
    if (n_tiles > 0 && Q > 0x7fffffffll / n_tiles) {
        set_error("zt_exclude_mark: Q=%lld queries x %lld tiles exceed one launch's workgroups", (long long)Q, n_tiles);
        return ZT_ERR_UNSUPPORTED;
    }
    if (Q == 0 || absent_words == 0) return ZT_OK;
    MarkArgs a;
    a.ids = ids_dev ? ids_dev : c->nbr;
    a.n_ids = ids_dev ? -1 : (long long)c->E2;
    a.begin = reinterpret_cast<const long long *>(begin_dev);
    a.len = reinterpret_cast<const long long *>(len_dev);
    a.Q = Q; a.id_lo = id_lo; a.C = C; a.words = absent_words; a.n_tiles = n_tiles;
    a.sorted = cand_sorted_dev; a.col = cand_col_dev; a.stride = cand_sorted_dev ? cand_stride : 0;
    a.absent = absent_dev;
    k_exclude_mark<<<(unsigned)(Q * a.n_tiles), MK_THREADS, 0, (hipStream_t)stream>>>(a);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
