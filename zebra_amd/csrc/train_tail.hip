// The tail of a TRAINING step on the device: the loss of train.py:212-213 with its gradient, and
// the optimizer step of train.py:215.
//
// Pair loss (k_link_bce_fwd, k_link_bce_bwd): prob [2B] is what the link scorer returns (scoring_train.hip: B positive pairs,
// then B negative ones);
//   loss = mean_i -max(log p_i, -100) + mean_j -max(log(1 - n_j), -100)
// is torch.nn.BCELoss with labels 1 and 0 added up, and dprob = (x - y) / max((1 - x) x, 1e-12) / B its gradient at
// grad_output = 1.  One workgroup of sixteen waves strides over the 2B probabilities.  The logarithms, the quotient and the sums
// are float64 and rounded to float32 ONCE: what comes out is the float64 composition's result to half a unit in the last place
// whatever B is -- 2B <= 8192 logarithms are microseconds, and a float32 logarithm alone would already cost the loss of B = 1
// its last bit.  A thread adds its elements in ascending order, the lanes of a wave meet in a fixed tree, the waves are added
// first to last: two runs give the same bits, there is no atomic.  The backward scales dprob by the incoming gradient, read
// from device memory: nothing of the loss ever goes through the host.
//
// Adam (k_adam): torch's single-tensor, non-capturable update without weight decay, amsgrad or maximize, for EVERY parameter
// of a group in one launch.  The table of tensors travels in the kernel's arguments by value (as apex's multi_tensor_apply
// does it): the gradients are fresh allocations every step, so a table in device memory would be a copy per step and a
// staging buffer to keep alive; this way there is no copy, no synchronisation and nothing to keep.  A tensor takes
// ceil(numel / ADAM_CHUNK) workgroups; a workgroup finds its tensor from the per-tensor block offsets in the arguments.
// 16-byte accesses where the tensor's four pointers allow them (a chunk starts a multiple of 16 bytes into its tensor), one
// element per lane otherwise: a parameter that is a view at an odd storage offset works.  The operations are torch's in
// torch's order, and the three multiply-adds are fused as in torch's own device kernels (lerp, addcmul and addcdiv compile to
// one fma each there): written out as fmaf, not left to the compiler, so that every build rounds alike.
#include "common.hpp"

#include <cmath>
#include <cstring>

using namespace zt;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BCE_THREADS = 1024, BCE_WAVES = BCE_THREADS / WAVE;
constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = ZT_ADAM_CHUNK;                 // elements per workgroup: four 16-byte accesses per lane and array
constexpr int ADAM_MAX_TENSORS = ZT_ADAM_MAX_TENSORS;     // per launch

__global__ __launch_bounds__(BCE_THREADS) void k_link_bce_fwd(const float *__restrict__ prob, long long B, float *__restrict__ loss,
                                                              float *__restrict__ dprob)
{
    __shared__ double part[2][BCE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double sp = 0.0, sn = 0.0;
    for (long long i = tid; i < 2 * B; i += BCE_THREADS) {
        const double x = (double)prob[i];
        const bool pos = i < B;
        double l = log(pos ? x : 1.0 - x), q = (1.0 - x) * x;
        l = l < -100.0 ? -100.0 : l;                                     // (a NaN stays one in both, as in torch)
        q = q < 1e-12 ? 1e-12 : q;
        if (pos) sp -= l; else sn -= l;
        dprob[i] = (float)((pos ? x - 1.0 : x) / q / (double)B);
    }
    for (int d = 32; d > 0; d >>= 1) {                                   // a fixed tree over the lanes
        sp += __shfl_down(sp, d);
        sn += __shfl_down(sn, d);
    }
    if (lane == 0) { part[0][wave] = sp; part[1][wave] = sn; }
    __syncthreads();
    if (tid == 0) {
        double tp = 0.0, tn = 0.0;
        for (int w = 0; w < BCE_WAVES; ++w) { tp += part[0][w]; tn += part[1][w]; }    // ... and the waves in order
        loss[0] = (float)(tp / (double)B + tn / (double)B);
    }
}

__global__ __launch_bounds__(256) void k_link_bce_bwd(const float *__restrict__ dprob, const float *__restrict__ grad_loss, long long n,
                                                      float *__restrict__ d_prob)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) d_prob[i] = grad_loss[0] * dprob[i];
}

// Label loss (k_label_bce_fwd): torch.nn.BCELoss() (mean) of prob [N] against a float label per row,
//   loss = mean_i -(y_i max(log x_i, -100) + (1 - y_i) max(log(1 - x_i), -100)),  dprob = (x - y) / max((1 - x) x, 1e-12) / N
// with k_link_bce_fwd's arithmetic: float64 logarithms, quotient and sums, one rounding, the same fixed order.
__global__ __launch_bounds__(BCE_THREADS) void k_label_bce_fwd(const float *__restrict__ prob, const float *__restrict__ label, long long N,
                                                               float *__restrict__ loss, float *__restrict__ dprob)
{
    __shared__ double part[BCE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (long long i = tid; i < N; i += BCE_THREADS) {
        const double x = (double)prob[i], y = (double)label[i];
        double l1 = log(x), l0 = log(1.0 - x), q = (1.0 - x) * x;
        l1 = l1 < -100.0 ? -100.0 : l1;                                  // (a NaN stays one, as in torch)
        l0 = l0 < -100.0 ? -100.0 : l0;
        q = q < 1e-12 ? 1e-12 : q;
        s -= y * l1 + (1.0 - y) * l0;
        dprob[i] = (float)((x - y) / q / (double)N);
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);             // a fixed tree over the lanes
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < BCE_WAVES; ++w) t += part[w];                // ... and the waves in order
        loss[0] = (float)(t / (double)N);
    }
}

// Listwise loss of a ranking step (k_rank_loss_fwd): logit [Q][C] from the one-vs-many scorer (rank_train.hip), -inf where a
// pair is absent; target[q] (NULL: column 0) is the positive's column.  A query whose target is absent (or outside [0, C)) is
// skipped; n_live queries remain.
//   softmax: loss = mean over live q of (logsumexp over present c of logit[q][c]) - logit[q][t_q],  dl = (softmax - onehot) / n_live
//   bce:     loss = mean over live q of -max(log sigma(logit[q][t_q]), -100)
//                 + mean over the n_neg present non-target pairs of live q of -max(log(1 - sigma(logit)), -100),
//            dl = (sigma - 1) / n_live at a target, sigma / n_neg elsewhere (as BCELoss's backward: not cut off where the log is)
// Absent pairs and skipped queries get dl = 0; with no live query the loss is 0.  The bce terms are formed from the LOGIT in
// float64 (log1p(exp(-|l|)) forms), not from a float32 probability: 1 - p of a rounded p would lose log(1 - sigma) its digits
// for l > 10.  The arithmetic rules are k_link_bce_fwd's: float64 exponentials, logarithms and sums, rounded to float32 once.
// A wave owns a query: its lanes add their columns in ascending order and meet in a fixed tree; lane 0 adds the wave's queries
// in ascending order and the waves are added first to last.  The counts n_live and n_neg are integers.
__device__ __forceinline__ double wave_sum(double v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return __shfl(v, 0);
}

__global__ __launch_bounds__(BCE_THREADS) void k_rank_loss_fwd(const float *__restrict__ logit, const int *__restrict__ target, long long Q,
                                                               long long C, int mode, float *__restrict__ loss, float *__restrict__ dl)
{
    __shared__ double part[2][BCE_WAVES];
    __shared__ long long cnt[2][BCE_WAVES];
    __shared__ long long total[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float NEG_INF = -INFINITY;
    // the counts
    long long nl = 0, nn = 0;
    for (long long q = wave; q < Q; q += BCE_WAVES) {
        const long long t = target != nullptr ? (long long)target[q] : 0;
        if (t < 0 || t >= C || logit[q * C + t] == NEG_INF) continue;       // (wave-uniform)
        ++nl;
        for (long long cb = 0; cb < C; cb += WAVE) {
            const long long c = cb + lane;
            nn += __popcll(__ballot(c < C && c != t && logit[q * C + c] != NEG_INF));
        }
    }
    if (lane == 0) { cnt[0][wave] = nl; cnt[1][wave] = nn; }
    __syncthreads();
    if (tid == 0) {
        long long a = 0, b = 0;
        for (int w = 0; w < BCE_WAVES; ++w) { a += cnt[0][w]; b += cnt[1][w]; }
        total[0] = a;
        total[1] = b;
    }
    __syncthreads();
    const double n_live = (double)total[0], n_neg = (double)total[1];
    double s0 = 0.0, s1 = 0.0;                                               // softmax: s0; bce: targets in s0, the others in s1
    for (long long q = wave; q < Q; q += BCE_WAVES) {
        const float *row = logit + q * C;
        float *drow = dl + q * C;
        const long long t = target != nullptr ? (long long)target[q] : 0;
        const bool live = t >= 0 && t < C && row[t] != NEG_INF;
        if (!live) {
            for (long long c = lane; c < C; c += WAVE) drow[c] = 0.f;
            continue;
        }
        if (mode == ZT_RANK_LOSS_SOFTMAX) {
            float m = NEG_INF;
            for (long long c = lane; c < C; c += WAVE) m = fmaxf(m, row[c]);
            for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
            const double md = (double)m;                                     // finite: the target is present
            double e = 0.0;
            for (long long c = lane; c < C; c += WAVE) {
                const float v = row[c];
                if (v != NEG_INF) e += exp((double)v - md);
            }
            e = wave_sum(e);
            const double lse = md + log(e);
            s0 += lse - (double)row[t];
            for (long long c = lane; c < C; c += WAVE) {
                const float v = row[c];
                double g = 0.0;
                if (v != NEG_INF) g = (exp((double)v - lse) - (c == t ? 1.0 : 0.0)) / n_live;
                drow[c] = (float)g;
            }
        } else {
            double a = 0.0;
            for (long long c = lane; c < C; c += WAVE) {
                const float v = row[c];
                if (v == NEG_INF) { drow[c] = 0.f; continue; }
                const double l = (double)v, ea = exp(-fabs(l)), lp = log1p(ea);
                const double sig = l >= 0.0 ? 1.0 / (1.0 + ea) : ea / (1.0 + ea);
                if (c == t) {                                                // (its term of the loss: below, by every lane)
                    drow[c] = (float)((sig - 1.0) / n_live);
                } else {
                    double lg = -(l >= 0.0 ? lp + l : lp);                   // log(1 - sigma(l))
                    lg = lg < -100.0 ? -100.0 : lg;
                    a -= lg;
                    drow[c] = (float)(sig / n_neg);
                }
            }
            s1 += wave_sum(a);
            const double l = (double)row[t], lp = log1p(exp(-fabs(l)));
            double lg = -(l >= 0.0 ? lp : lp - l);                           // log sigma(l)
            lg = lg < -100.0 ? -100.0 : lg;
            s0 -= lg;
        }
    }
    if (lane == 0) { part[0][wave] = s0; part[1][wave] = s1; }
    __syncthreads();
    if (tid == 0) {
        double t0 = 0.0, t1 = 0.0;
        for (int w = 0; w < BCE_WAVES; ++w) { t0 += part[0][w]; t1 += part[1][w]; }    // the waves in order
        double out = 0.0;
        if (total[0] > 0) out = t0 / n_live;
        if (mode != ZT_RANK_LOSS_SOFTMAX && total[1] > 0) out += t1 / n_neg;
        loss[0] = (float)out;
    }
}

// (a kernel argument: keep the layout.  3096 bytes of the 4 KB a launch may carry)
struct AdamArgs {
    float *param[ADAM_MAX_TENSORS];
    const float *grad[ADAM_MAX_TENSORS];
    float *exp_avg[ADAM_MAX_TENSORS];
    float *exp_avg_sq[ADAM_MAX_TENSORS];
    float step_size[ADAM_MAX_TENSORS];
    float bias2_sqrt[ADAM_MAX_TENSORS];
    int numel[ADAM_MAX_TENSORS];
    int block_off[ADAM_MAX_TENSORS + 1];      // first workgroup of tensor t; [n] = the grid
    int n;
    float beta1, one_minus_beta1, beta2, one_minus_beta2, eps;
};
static_assert(sizeof(AdamArgs) <= 4096, "the table must fit a launch's arguments");
static_assert(ADAM_MAX_TENSORS >= 32 && ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "");

struct AdamScalars { float beta1, omb1, beta2, omb2, eps, step_size, bias2_sqrt; };

// torch/optim/adam.py: lerp_, mul_ + addcmul_, sqrt / bias_correction2_sqrt + eps, addcdiv_
//   m = m + (g - m) (1 - beta1);  v = v beta2 + (1 - beta2) g g;  denom = sqrt(v) / bias2_sqrt + eps;  p = p - step_size (m / denom)
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamScalars &c)
{
#pragma clang fp contract(off)
    m = fmaf(c.omb1, g - m, m);
    v = fmaf(c.omb2, g * g, v * c.beta2);
    const float denom = sqrtf(v) / c.bias2_sqrt + c.eps;
    p = fmaf(-c.step_size, m / denom, p);
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adam(const AdamArgs a)
{
    // the tensor of this workgroup: the last t with block_off[t] <= blockIdx.x (empty tensors are not in the table)
    const int b = (int)blockIdx.x;
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block_off[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int t = lo;
    const int numel = a.numel[t];
    const int off = (b - a.block_off[t]) * ADAM_CHUNK;                   // (numel < 2^31: zt_adam_step)
    if (off >= numel) return;
    const int len = numel - off < ADAM_CHUNK ? numel - off : ADAM_CHUNK;
    float *__restrict__ p = a.param[t] + off;
    const float *__restrict__ g = a.grad[t] + off;
    float *__restrict__ m = a.exp_avg[t] + off;
    float *__restrict__ v = a.exp_avg_sq[t] + off;
    const AdamScalars c = {a.beta1, a.one_minus_beta1, a.beta2, a.one_minus_beta2, a.eps, a.step_size[t], a.bias2_sqrt[t]};
    const int tid = threadIdx.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    int done = 0;
    if (vec) {
        const int n4 = len >> 2;
        constexpr int U = ADAM_CHUNK / (4 * ADAM_THREADS);
        f32x4 pv[U], gv[U], mv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                                    // every load of the chunk in flight before the first use
            const int i = tid + u * ADAM_THREADS;
            if (i < n4) {
                pv[u] = reinterpret_cast<const f32x4 *>(p)[i];
                gv[u] = reinterpret_cast<const f32x4 *>(g)[i];
                mv[u] = reinterpret_cast<const f32x4 *>(m)[i];
                vv[u] = reinterpret_cast<const f32x4 *>(v)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = tid + u * ADAM_THREADS;
            if (i < n4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pe = pv[u][j], me = mv[u][j], ve = vv[u][j];
                    adam_element(pe, gv[u][j], me, ve, c);
                    pv[u][j] = pe;
                    mv[u][j] = me;
                    vv[u][j] = ve;
                }
                reinterpret_cast<f32x4 *>(p)[i] = pv[u];
                reinterpret_cast<f32x4 *>(m)[i] = mv[u];
                reinterpret_cast<f32x4 *>(v)[i] = vv[u];
            }
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < len; i += ADAM_THREADS) {               // the tail of an aligned tensor, or all of another
        float pe = p[i], me = m[i], ve = v[i];
        adam_element(pe, g[i], me, ve, c);
        p[i] = pe;
        m[i] = me;
        v[i] = ve;
    }
}

// 1 - beta as torch multiplies by it.  There the betas are Python floats: exp_avg_sq.mul_(beta2) rounds 0.999 to float32 and
// addcmul_(..., value=1 - beta2) rounds the float64 difference 0.001 -- which is NOT 1 - float32(0.999) = 0.00099998713 (1.3e-5
// off, a hundred times the rounding of the update).  The ABI carries float32: the decimal meant is taken to be the shortest
// one that rounds to the float given (0.999f -> 0.999), and the difference is formed in float64.  A beta that is exact in
// float32 (0.5, 0.875) comes back exactly.
float one_minus(float beta)
{
    static thread_local float last_beta = -1.f, last = 0.f;
    if (beta == last_beta) return last;
    double d = (double)beta;
    char buf[32];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof(buf), "%.*g", digits, (double)beta);
        const double back = strtod(buf, nullptr);
        if ((float)back == beta) { d = back; break; }
    }
    last_beta = beta;
    last = (float)(1.0 - d);
    return last;
}

// launches and their grids for a list of sizes (zt_adam_plan; zt_adam_step fills its tables from the same walk): tensors in the
// order given, empty ones left out, at most ADAM_MAX_TENSORS per launch.  fn(launch, slot, index, first block) per tensor
// kept, end(launch, tensors, blocks) per launch.  Returns the launches.
template <class Numel, class Fn, class End>
int adam_walk(int n, Numel numel, Fn &&fn, End &&end)
{
    int launches = 0, slot = 0;
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        const long long ne = numel(i);
        if (ne <= 0) continue;
        fn(launches, slot, i, blocks);
        blocks += (ne + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (++slot == ADAM_MAX_TENSORS) {
            end(launches, slot, blocks);
            ++launches;
            slot = 0;
            blocks = 0;
        }
    }
    if (slot > 0) {
        end(launches, slot, blocks);
        ++launches;
    }
    return launches;
}

}  // namespace

extern "C" int zt_link_bce_forward(const float *prob_dev, int64_t B, float *loss_dev, float *dprob_dev, void *stream)
{
    if (B < 1 || !prob_dev || !loss_dev || !dprob_dev) {
        set_error("zt_link_bce_forward: bad argument (B >= 1 and three device pointers expected)");
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    ZT_PROF_BEGIN(s, P_LINK_BCE);
    k_link_bce_fwd<<<1, BCE_THREADS, 0, s>>>(prob_dev, (long long)B, loss_dev, dprob_dev);
    ZT_PROF_END(s, P_LINK_BCE);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_link_bce_backward(const float *dprob_dev, const float *grad_loss_dev, int64_t B, float *d_prob_dev, void *stream)
{
    if (B < 1 || B > (INT64_MAX >> 2) || !dprob_dev || !grad_loss_dev || !d_prob_dev) {
        set_error("zt_link_bce_backward: bad argument (B >= 1 and three device pointers expected)");
        return ZT_ERR_ARG;
    }
    const long long n = 2 * (long long)B, grid = (n + 255) / 256;
    if (grid > 0x7fffffffll) {
        set_error("zt_link_bce_backward: B=%lld is beyond one launch", (long long)B);
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    ZT_PROF_BEGIN(s, P_LINK_BCE);
    k_link_bce_bwd<<<(unsigned)grid, 256, 0, s>>>(dprob_dev, grad_loss_dev, n, d_prob_dev);
    ZT_PROF_END(s, P_LINK_BCE);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_label_bce_forward(const float *prob_dev, const float *label_dev, int64_t N, float *loss_dev, float *dprob_dev,
                                    void *stream)
{
    if (N < 1 || !prob_dev || !label_dev || !loss_dev || !dprob_dev) {
        set_error("zt_label_bce_forward: bad argument (N >= 1 and four device pointers expected)");
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    ZT_PROF_BEGIN(s, P_LINK_BCE);
    k_label_bce_fwd<<<1, BCE_THREADS, 0, s>>>(prob_dev, label_dev, (long long)N, loss_dev, dprob_dev);
    ZT_PROF_END(s, P_LINK_BCE);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_label_bce_backward(const float *dprob_dev, const float *grad_loss_dev, int64_t N, float *d_prob_dev, void *stream)
{
    const long long grid = N < 1 ? 0 : (N - 1) / 256 + 1;
    if (N < 1 || grid > 0x7fffffffll || !dprob_dev || !grad_loss_dev || !d_prob_dev) {
        set_error("zt_label_bce_backward: bad argument (1 <= N within one launch and three device pointers expected)");
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    ZT_PROF_BEGIN(s, P_LINK_BCE);
    k_link_bce_bwd<<<(unsigned)grid, 256, 0, s>>>(dprob_dev, grad_loss_dev, (long long)N, d_prob_dev);
    ZT_PROF_END(s, P_LINK_BCE);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_rank_loss_forward(const float *logit_dev, const int32_t *target_dev, int64_t Q, int64_t C, int32_t mode, float *loss_dev,
                                    float *dl_dev, void *stream)
{
    if (Q < 1 || C < 1 || C > INT64_MAX / Q || !logit_dev || !loss_dev || !dl_dev) {
        set_error("zt_rank_loss_forward: bad argument (Q >= 1, C >= 1 and three device pointers expected)");
        return ZT_ERR_ARG;
    }
    if (mode != ZT_RANK_LOSS_SOFTMAX && mode != ZT_RANK_LOSS_BCE) {
        set_error("zt_rank_loss_forward: mode %d unknown (ZT_RANK_LOSS_SOFTMAX or ZT_RANK_LOSS_BCE)", mode);
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    ZT_PROF_BEGIN(s, P_LINK_BCE);
    k_rank_loss_fwd<<<1, BCE_THREADS, 0, s>>>(logit_dev, target_dev, (long long)Q, (long long)C, mode, loss_dev, dl_dev);
    ZT_PROF_END(s, P_LINK_BCE);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_rank_loss_backward(const float *dl_dev, const float *grad_loss_dev, int64_t n, float *d_logit_dev, void *stream)
{
    const long long grid = n < 1 ? 0 : (n - 1) / 256 + 1;
    if (n < 1 || grid > 0x7fffffffll || !dl_dev || !grad_loss_dev || !d_logit_dev) {
        set_error("zt_rank_loss_backward: bad argument (1 <= n within one launch and three device pointers expected)");
        return ZT_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    ZT_PROF_BEGIN(s, P_LINK_BCE);
    k_link_bce_bwd<<<(unsigned)grid, 256, 0, s>>>(dl_dev, grad_loss_dev, (long long)n, d_logit_dev);
    ZT_PROF_END(s, P_LINK_BCE);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}

extern "C" int zt_adam_plan(const int64_t *numel_host, int32_t n, int64_t *out)
{
    if (n < 0 || !out || (n > 0 && !numel_host)) {
        set_error("zt_adam_plan: bad argument");
        return ZT_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (numel_host[i] < 0 || numel_host[i] > 0x7fffffffll) {
            set_error("zt_adam_plan: tensor %d has %lld elements (0 <= numel < 2^31 expected)", i, (long long)numel_host[i]);
            return ZT_ERR_ARG;
        }
    out[0] = adam_walk(n, [&](int i) { return (long long)numel_host[i]; }, [](int, int, int, long long) {},
                       [&](int launch, int, long long blocks) { out[1 + launch] = blocks; });
    return ZT_OK;
}

extern "C" int zt_adam_step(const zt_adam_tensor *tensors_host, int32_t n, float beta1, float beta2, float eps, void *stream)
{
    if (n < 0 || (n > 0 && !tensors_host)) {
        set_error("zt_adam_step: bad argument");
        return ZT_ERR_ARG;
    }
    for (int i = 0; i < n; ++i) {
        const zt_adam_tensor &t = tensors_host[i];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || t.numel < 0 || t.numel > 0x7fffffffll) {
            set_error("zt_adam_step: tensor %d: four device pointers and 0 <= numel < 2^31 expected (numel %lld)", i, (long long)t.numel);
            return ZT_ERR_ARG;
        }
    }
    if (n == 0) return ZT_OK;
    hipStream_t s = (hipStream_t)stream;
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    a.beta1 = beta1;
    a.one_minus_beta1 = one_minus(beta1);
    a.beta2 = beta2;
    a.one_minus_beta2 = one_minus(beta2);
    a.eps = eps;
    bool failed = false;
    ZT_PROF_BEGIN(s, P_ADAM);
    adam_walk(n, [&](int i) { return (long long)tensors_host[i].numel; },
              [&](int, int slot, int i, long long first) {
                  const zt_adam_tensor &t = tensors_host[i];
                  a.param[slot] = t.param;
                  a.grad[slot] = t.grad;
                  a.exp_avg[slot] = t.exp_avg;
                  a.exp_avg_sq[slot] = t.exp_avg_sq;
                  a.step_size[slot] = t.step_size;
                  a.bias2_sqrt[slot] = t.bias2_sqrt;
                  a.numel[slot] = (int)t.numel;
                  a.block_off[slot] = (int)first;
              },
              [&](int, int slots, long long blocks) {
                  // (a launch's blocks: at most ADAM_MAX_TENSORS x 2^31 / ADAM_CHUNK = 2^25)
                  a.n = slots;
                  a.block_off[slots] = (int)blocks;
                  if (!failed) {
                      k_adam<<<(unsigned)blocks, ADAM_THREADS, 0, s>>>(a);
                      failed = hipPeekAtLastError() != hipSuccess;
                  }
              });
    ZT_PROF_END(s, P_ADAM);
    ZT_LAUNCH_CHECK();
    return ZT_OK;
}
