// Negative sampling for the ranking paths (include/zebra_amd.h, zt_neg_sample; DESIGN.md section 5, "Negative sampling"):
// per edge up to K ids, drawn with a counter-based generator from the edge's own id list (historical slots) and from the
// destination pool, the exclusions applied while drawing.  The header states the rule; tests/helpers_negsample.py restates
// it in numpy and the kernel is held to that bit for bit.
// The kernel: one workgroup per row, everything in (dynamic, 16-byte aligned) LDS.  A round is
//   draw     every empty slot computes its Philox word and reads its id; a draw that survives the per-draw tests (id >= 0,
//            not the destination, not the source) becomes a 64-bit word (id << 32 | 1 << 31 | slot); under DISTINCT the
//            slots filled in earlier rounds stand beside them as (id << 32 | slot), everything else is the all-ones word;
//   sort     one bitonic sort of the N2 words: equal ids are adjacent, an earlier round's slot first, then the round's
//            draws by slot number -- list draws before pool draws, because historical slots are the low-numbered ones;
//   scan     under FILTER, if a pool draw is pending: one coalesced pass over the row's list, each entry looked up in the
//            sorted words (lower bound, as k_exclude_mark does), marking the FIRST word of its id;
//   resolve  a draw fills its slot unless (DISTINCT) its predecessor holds the same id, or (FILTER, pool draw) the first
//            word of its id is marked.  Why the predecessor test is the rule: the first word of a run of equal ids is an
//            earlier round's slot (every draw of the run fails), or the lowest-numbered draw; that one passes unless it is
//            a marked pool draw, and then every later draw of the run is a marked pool draw too.
// Without DISTINCT and without a list to filter against nothing is sorted: a surviving draw fills its slot at once.
// Every loop is bounded by K, N2, len, rounds or 64 search steps; no global atomics; no row waits for another.
#include "csr_handle.hpp"

using namespace zt;

namespace {

constexpr u64 NS_NONE = ~0ull;                 // sorts behind every id (ids are below 2^31)
constexpr unsigned NS_DRAW = 0x80000000u;      // bit 31 of the low word: a draw of this round

struct NegPlan {
    int form;              // 0 refused; 1: one wave; 2: several
    int threads, n2;
    long long lds;
};

NegPlan neg_plan(int K)
{
    NegPlan p = {0, 0, 0, 0};
    if (K < 1 || K > ZT_NEG_MAX_K) return p;
    int n2 = 64;
    while (n2 < K) n2 <<= 1;
    p.n2 = n2;
    p.threads = n2 <= 128 ? 64 : (n2 <= 1024 ? 256 : 1024);
    p.form = p.threads == 64 ? 1 : 2;
    p.lds = (long long)n2 * 14 + 16;           // words 8, slots 4, kind 1, mark 1 per element; four control ints
    return p;
}

struct NegArgs {
    const int *src, *dst, *pool;
    long long n_pool;
    const int *ids;                   // the lists' array (NULL: no lists)
    long long n_ids;                  // its length where known (the handle's array), else -1
    const long long *begin, *len;     // [Q] (NULL: no lists)
    int *neg, *count;
    unsigned key_lo, key_hi;
    long long row_base;
    int K, K_hist, rounds, hist_rounds, flags, n2;
};

__device__ __forceinline__ unsigned philox_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// the first position whose word is not below `target`
__device__ __forceinline__ int lower_bound_words(const u64 *s_key, int n2, u64 target)
{
    int lo = 0, hi = n2;
    for (int it = 0; it < 64 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (s_key[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int T>
__global__ __launch_bounds__(T) void k_neg_sample(const NegArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ns_smem[];
    const int n2 = a.n2, K = a.K, tid = threadIdx.x;
    u64 *s_key = reinterpret_cast<u64 *>(ns_smem);                         // [n2]
    int *s_slot = reinterpret_cast<int *>(ns_smem + (size_t)n2 * 8);       // [n2]: the id a slot holds, -1: empty
    int *s_ctl = s_slot + n2;                                              // empty slots?, pool draws pending?, the two counts
    unsigned char *s_kind = reinterpret_cast<unsigned char *>(s_ctl + 4);  // [n2]: 1 filled from the list, 2 from the pool
    unsigned char *s_mark = s_kind + n2;                                   // [n2]: this position's id occurs in the list

    const long long q = blockIdx.x;
    const u64 row = (u64)(a.row_base + q);
    const unsigned c0 = (unsigned)row, c1 = (unsigned)(row >> 32);
    const int dst = a.dst[q], src = a.src[q];
    long long b = 0, n = 0;
    if (a.begin != nullptr && a.ids != nullptr) {
        b = a.begin[q]; n = a.len[q];
        if (b < 0 || n < 0) n = 0;
        if (a.n_ids >= 0) n = b > a.n_ids ? 0 : min(n, a.n_ids - b);      // never past the handle's array
        n = min(n, 0x7fffffffll);
    }
    const bool distinct = (a.flags & ZT_NEG_DISTINCT) != 0, excl = (a.flags & ZT_NEG_EXCLUDE_SOURCE) != 0;
    const bool filter = (a.flags & ZT_NEG_FILTER) != 0 && n > 0;
    const bool sorted = distinct || filter;

    for (int j = tid; j < n2; j += T) { s_slot[j] = -1; s_kind[j] = 0; }
    if (tid == 0) s_ctl[2] = s_ctl[3] = 0;
    for (int r = 0; r < a.rounds; ++r) {
        if (tid == 0) s_ctl[0] = s_ctl[1] = 0;
        __syncthreads();
        const bool hist_list = r < a.hist_rounds && n > 0;
        bool any_empty = false, pool_pending = false;
        for (int j = tid; j < n2; j += T) {
            u64 word = NS_NONE;
            if (j < K) {
                const int cur = s_slot[j];
                if (cur < 0) {
                    any_empty = true;
                    const u64 x = philox_word0(c0, c1, (unsigned)j, (unsigned)r, a.key_lo, a.key_hi);
                    const bool from_list = j < a.K_hist && hist_list;
                    const int id = from_list ? a.ids[b + (long long)((x * (u64)n) >> 32)]
                                             : a.pool[(long long)((x * (u64)a.n_pool) >> 32)];
                    if (id >= 0 && id != dst && !(excl && id == src)) {
                        if (sorted) {
                            word = ((u64)(unsigned)id << 32) | NS_DRAW | (unsigned)j;
                            pool_pending |= !from_list;
                        } else {
                            s_slot[j] = id;
                            s_kind[j] = from_list ? 1 : 2;
                        }
                    }
                } else if (distinct) {
                    word = ((u64)(unsigned)cur << 32) | (unsigned)j;
                }
            }
            if (sorted) { s_key[j] = word; s_mark[j] = 0; }
        }
        if (any_empty) s_ctl[0] = 1;                   // (every writer stores the same value)
        if (pool_pending) s_ctl[1] = 1;
        __syncthreads();
        const bool go_on = s_ctl[0] != 0, scan = filter && s_ctl[1] != 0;
        if (!go_on) break;                             // uniform: the row is full
        if (sorted) {
            for (int k = 2; k <= n2; k <<= 1) {
                for (int s = k >> 1; s > 0; s >>= 1) {
                    for (int i = tid; i < (n2 >> 1); i += T) {
                        const int lo = ((i & ~(s - 1)) << 1) | (i & (s - 1)), hi = lo | s;
                        const u64 x = s_key[lo], y = s_key[hi];
                        if ((x > y) == ((lo & k) == 0)) { s_key[lo] = y; s_key[hi] = x; }
                    }
                    __syncthreads();
                }
            }
            if (scan) {
                for (long long i0 = tid; i0 < n; i0 += 4 * T) {           // four loads in flight per lane, then their searches
                    int v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const long long i = i0 + (long long)u * T;
                        v[u] = i < n ? a.ids[b + i] : -1;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (v[u] < 0) continue;
                        const int p = lower_bound_words(s_key, n2, (u64)(unsigned)v[u] << 32);
                        if (p < n2 && (int)(s_key[p] >> 32) == v[u]) s_mark[p] = 1;
                    }
                }
                __syncthreads();
            }
            for (int p = tid; p < n2; p += T) {
                const u64 word = s_key[p];
                const unsigned low = (unsigned)word;
                if (word == NS_NONE || (low & NS_DRAW) == 0u) continue;
                const unsigned id = (unsigned)(word >> 32);
                const int j = (int)(low & ~NS_DRAW);
                const bool head = p == 0 || (unsigned)(s_key[p - 1] >> 32) != id;
                if (distinct && !head) continue;
                const bool from_list = j < a.K_hist && hist_list;
                if (scan && !from_list) {
                    const int h = head ? p : lower_bound_words(s_key, n2, (u64)id << 32);
                    if (s_mark[h] != 0) continue;
                }
                s_slot[j] = (int)id;
                s_kind[j] = from_list ? 1 : 2;
            }
        }
        __syncthreads();                               // the slots are final for this round; the control words are read
    }
    __syncthreads();
    int n_list = 0, n_pool = 0;
    int *out = a.neg + q * (long long)K;
    for (int j = tid; j < K; j += T) {
        out[j] = s_slot[j];
        n_list += s_kind[j] == 1;
        n_pool += s_kind[j] == 2;
    }
    if (a.count != nullptr) {
        if (n_list) atomicAdd(&s_ctl[2], n_list);
        if (n_pool) atomicAdd(&s_ctl[3], n_pool);
        __syncthreads();
        if (tid == 0) { a.count[2 * q] = s_ctl[2]; a.count[2 * q + 1] = s_ctl[3]; }
    }
}

template <int T>
int neg_launch(const NegArgs &a, long long Q, const NegPlan &p, hipStream_t stream)
{
    ZT_HIP(set_dynamic_lds(reinterpret_cast<const void *>(k_neg_sample<T>), (size_t)p.lds));
    k_neg_sample<T><<<(unsigned)Q, T, (size_t)p.lds, stream>>>(a);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

}  // namespace

extern "C" int zt_neg_sample_plan(int32_t K, int64_t *out)
{
    if (!out) {
        set_error("zt_neg_sample_plan: out is NULL");
        return ZT_ERR_ARG;
    }
    const NegPlan p = neg_plan(K);
    out[0] = p.form; out[1] = p.threads; out[2] = p.n2; out[3] = p.lds;
    return ZT_OK;
}

extern "C" int zt_neg_sample(const zt_neg_desc *d, const int32_t *src_dev, const int32_t *dst_dev, int64_t Q,
                             const int32_t *pool_dev, int64_t n_pool, const zt_csr *c, const int32_t *ids_dev,
                             const int64_t *begin_dev, const int64_t *len_dev, int32_t *neg_dev, int32_t *count_dev, void *stream)
{
    if (!d || !src_dev || !dst_dev || !pool_dev || !neg_dev || Q < 0 || (n_pool <= 0 && Q > 0)) {
        set_error("zt_neg_sample: bad argument");
        return ZT_ERR_ARG;
    }
    const NegPlan p = neg_plan(d->K);
    if (p.form == 0) {
        set_error("zt_neg_sample: K=%d is outside 1 .. %d", (int)d->K, ZT_NEG_MAX_K);
        return ZT_ERR_ARG;
    }
    if (d->K_hist < 0 || d->K_hist > d->K || d->rounds < 1 || d->rounds > ZT_NEG_MAX_ROUNDS || d->hist_rounds < 0 ||
        d->hist_rounds > d->rounds || (d->flags & ~(ZT_NEG_FILTER | ZT_NEG_DISTINCT | ZT_NEG_EXCLUDE_SOURCE)) != 0) {
        set_error("zt_neg_sample: K_hist=%d of K=%d, rounds=%d, hist_rounds=%d or flags=0x%x out of range", (int)d->K_hist,
                  (int)d->K, (int)d->rounds, (int)d->hist_rounds, (unsigned)d->flags);
        return ZT_ERR_ARG;
    }
    if ((begin_dev == nullptr) != (len_dev == nullptr) || (begin_dev != nullptr && !c && !ids_dev)) {
        set_error("zt_neg_sample: lists are begin_dev and len_dev together, over the handle's array or ids_dev");
        return ZT_ERR_ARG;
    }
    if (n_pool > 0x7fffffffll || (begin_dev != nullptr && !ids_dev && c->E2 > 0x7fffffffll) || Q > 0x7fffffffll) {
        set_error("zt_neg_sample: n_pool=%lld, the handle's entries or Q=%lld reach 2^31", (long long)n_pool, (long long)Q);
        return ZT_ERR_UNSUPPORTED;
    }
    if (Q == 0) return ZT_OK;
    NegArgs a;
    a.src = src_dev; a.dst = dst_dev; a.pool = pool_dev; a.n_pool = n_pool;
    a.ids = begin_dev == nullptr ? nullptr : (ids_dev ? ids_dev : c->nbr);
    a.n_ids = ids_dev ? -1 : (c ? (long long)c->E2 : -1);
    a.begin = reinterpret_cast<const long long *>(begin_dev);
    a.len = reinterpret_cast<const long long *>(len_dev);
    a.neg = neg_dev; a.count = count_dev;
    a.key_lo = (unsigned)d->seed; a.key_hi = (unsigned)(d->seed >> 32);
    a.row_base = d->row_base;
    a.K = d->K; a.K_hist = d->K_hist; a.rounds = d->rounds; a.hist_rounds = d->hist_rounds; a.flags = d->flags; a.n2 = p.n2;
    const hipStream_t s = (hipStream_t)stream;
    if (p.threads == 64) return neg_launch<64>(a, Q, p, s);
    if (p.threads == 256) return neg_launch<256>(a, Q, p, s);
    return neg_launch<1024>(a, Q, p, s);
}
