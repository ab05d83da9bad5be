// k_pruned_topk_ws (zebra_amd/csrc/tppr_prune.hip) run as HOST code, for checking the kernel's logic where no GPU is at hand:
// one workgroup at a time, 256 std::threads, std::barrier for __syncthreads and for the wave operations (__ballot, __shfl,
// __shfl_up rendezvous over the 64 threads of a wave), GCC atomics for the device atomics.  The walk and what else the two
// forms share is csrc/prune_walk.hpp, included as it is; kernel_body.inc (the kernel with its merge and selection, and the
// sequential sort it falls back to) is cut out of the sources by prune_ws_emu.py, which also writes the inputs (*.bin: CSR,
// queries, models, the oracle's outputs) and runs this program; it prints the number of output words that differ from the
// oracle's.  It says nothing about speed, and nothing about what only the device can get wrong (memory ordering between
// waves, launch plumbing): tests/test_prune_wide_gpu.py does.
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
typedef unsigned long long u64;
constexpr int WAVE = 64;
#define ZT_ERR_RANGE (-2)
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
struct Dim { int x; };
thread_local Dim threadIdx;
Dim blockIdx, gridDim;
static std::barrier<> blk(256);
static std::barrier<> *wb[4];
static std::atomic<u64> bal[4];
static int shv[4][64];
static std::atomic<int> orv{0};
inline int lane_id() { return threadIdx.x & 63; }
inline int wv() { return threadIdx.x / 64; }
inline void __syncthreads() { blk.arrive_and_wait(); }
inline void wave_sync() {}                    // (WaveGroup's barrier: the LDS form's group, not run here)
inline int __syncthreads_or(int v) { blk.arrive_and_wait(); if (v) orv.fetch_or(1); blk.arrive_and_wait(); int r = orv.load(); blk.arrive_and_wait(); if (threadIdx.x == 0) orv = 0; blk.arrive_and_wait(); return r; }
inline u64 __ballot(bool p) { auto &b = *wb[wv()]; b.arrive_and_wait(); if (p) bal[wv()].fetch_or(1ull << lane_id()); b.arrive_and_wait(); u64 r = bal[wv()].load(); b.arrive_and_wait(); if (lane_id() == 0) bal[wv()] = 0; b.arrive_and_wait(); return r; }
inline int __shfl(int v, int src) { auto &b = *wb[wv()]; shv[wv()][lane_id()] = v; b.arrive_and_wait(); int r = shv[wv()][src]; b.arrive_and_wait(); return r; }
inline int __shfl_up(int v, int d) { auto &b = *wb[wv()]; shv[wv()][lane_id()] = v; b.arrive_and_wait(); int r = lane_id() >= d ? shv[wv()][lane_id() - d] : v; b.arrive_and_wait(); return r; }
inline int __popcll(u64 x) { return __builtin_popcountll(x); }
inline int __ffsll(long long x) { return __builtin_ffsll(x); }
inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, 8); return r; }
inline u64 atomicCAS(u64 *p, u64 cmp, u64 v) { __atomic_compare_exchange_n(p, &cmp, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST); return cmp; }
inline int atomicMin(int *p, int v) { int o = __atomic_load_n(p, __ATOMIC_SEQ_CST); while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {} return o; }
inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline int atomicExch(int *p, int v) { return __atomic_exchange_n(p, v, __ATOMIC_SEQ_CST); }
inline void st_agent(u64 *p, u64 v) { __atomic_store_n(p, v, __ATOMIC_SEQ_CST); }
inline void st_agent(int *p, int v) { __atomic_store_n(p, v, __ATOMIC_SEQ_CST); }
inline int ld_agent(const int *p) { return __atomic_load_n(p, __ATOMIC_SEQ_CST); }
namespace {
#include "prune_walk.hpp"
#include "kernel_body.inc"
}
template <class T> std::vector<T> rd(const char *fn) { FILE *f = fopen(fn, "rb"); if (!f) { perror(fn); exit(2); } fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<T> v(n / sizeof(T)); if (fread(v.data(), 1, n, f) != (size_t)n) exit(2); fclose(f); return v; }
int main(int argc, char **argv)
{
    // args: width depth k M zero_empty fill nslabs
    int width = atoi(argv[1]), depth = atoi(argv[2]), k = atoi(argv[3]), M = atoi(argv[4]), zero_empty = atoi(argv[5]), fill = atoi(argv[6]), nsl = atoi(argv[7]);
    auto indptr = rd<long long>("indptr.bin"); auto nbr = rd<int>("nbr.bin"); auto eid = rd<int>("eid.bin"); auto ats = rd<double>("ts.bin");
    auto q = rd<int>("q.bin"); auto qt = rd<double>("qt.bin"); auto ab = rd<double>("ab.bin");
    auto en = rd<int>("exp_n.bin"); auto ee = rd<int>("exp_e.bin"); auto ed = rd<float>("exp_d.bin"); auto ew = rd<float>("exp_w.bin");
    long long nq = q.size(), N = indptr.size() - 1;
    long long cap = 0, lvl = 1, front = 1;
    for (int d = 0; d < depth; ++d) { front = lvl; lvl *= width; cap += lvl; }
    size_t sb = ws_slab_bytes((int)cap, (int)front, M);
    std::vector<char> slabs(sb * nsl, (char)0xAB);
    std::vector<int> on(M * nq * k, fill), oe(M * nq * k, fill); std::vector<float> od(M * nq * k, (float)fill), ow(M * nq * k, (float)fill);
    int status = 0;
    PruneModels pm; pm.M = M; for (int m = 0; m < M; ++m) { pm.alpha[m] = ab[2 * m]; pm.beta[m] = ab[2 * m + 1]; }
    for (int w = 0; w < 4; ++w) wb[w] = new std::barrier<>(64);
    gridDim.x = (int)(nq < nsl ? nq : nsl);
    for (int b = 0; b < gridDim.x; ++b) {
        blockIdx.x = b;
        std::vector<std::thread> th;
        for (int t = 0; t < 256; ++t) th.emplace_back([&, t] { threadIdx.x = t; k_pruned_topk_ws(indptr.data(), nbr.data(), eid.data(), ats.data(), N, q.data(), qt.data(), nq, width, depth, pm, k, on.data(), oe.data(), od.data(), ow.data(), nq * k, &status, (int)cap, (int)front, M, slabs.data(), (long long)sb, zero_empty); });
        for (auto &x : th) x.join();
    }
    long bad = 0;
    for (size_t i = 0; i < on.size(); ++i) bad += on[i] != en[i] || oe[i] != ee[i] || memcmp(&od[i], &ed[i], 4) || memcmp(&ow[i], &ew[i], 4);
    printf("width %d depth %d k %d M %d nq %lld slabs %d status %d mismatches %ld of %zu\n", width, depth, k, M, nq, nsl, status, bad, on.size());
    return bad != 0;
}
