// Surrogate test of the transfer entropy (vaeteb/tenull.py): the KL per step of every
// (recording, variant) row, and the rank statistics of the observed row among its surrogates.
//
//   k_te_kl_steps    ts[r, s] = mean over L of the elementwise KL of step s of row r, te[r] = mean over
//                    (S, L): k_te_kl_rows's fp32 expression (te.hip) in its operation order, the prior
//                    read at row r / K.  The (R, S, L) elementwise tensor is never written.  One
//                    workgroup per row; a step belongs to a group of G = min(64, pow2 >= L) adjacent
//                    lanes (L = 32: a wave covers two steps, 256 contiguous bytes per operand).
//   k_tenull_stats   one workgroup per recording over ts (B, K1, S) and te (B, K1), variant 0 the
//                    observed row: the integer ranks of the row mean, of every step and of every step
//                    against the surrogates' maxima over steps, and the surrogates' mean / sd.
//   k_tenull_group   group_sums[k] = sum over recordings of te[b, k], one thread per variant.
//
// Summation orders (all in double, none through an atomic, so every result has the same bits on
// every run and a row's or a recording's result depends on that row or recording only):
//   step sum    lane i of the group adds l = i, i + G, ... in ascending l, then the group's lanes are
//               combined by xor shuffles with offsets G/2, ..., 1;
//   row sum     group g adds the step sums of s = g, g + 256/G, ... in ascending s; thread 0 adds the
//               groups' sums in group order;
//   surr_mean, surr_sd, step_surr_mean   one thread, k = 1 .. K1 - 1 in order;
//   group_sums  one thread per k, b = 0 .. B - 1 in order.
// The comparisons are float32 >= on the stored values, which a NaN on either side never satisfies;
// the maximum over steps skips NaN (-inf for a row of NaN only).
#include <math.h>

#include "common.h"

namespace vt {

static constexpr int TN_THREADS = 256;
static constexpr int TN_MAX_K1 = 4096;                    // variants per recording (LDS: mx, te)

__global__ __launch_bounds__(TN_THREADS) void k_te_kl_steps(const float* __restrict__ mu_c,
                                                            const float* __restrict__ lv_q,
                                                            const float* __restrict__ mu_y,
                                                            const float* __restrict__ lv_p, int K, int S_, int L,
                                                            int G, float* __restrict__ ts, float* __restrict__ te) {
    __shared__ double red[TN_THREADS];
    const int64_t r = blockIdx.x, n = (int64_t)S_ * L;
    const float* mc = mu_c + r * n;
    const float* lq_ = lv_q + r * n;
    const float* my = mu_y + (r / K) * n;
    const float* lp_ = lv_p + (r / K) * n;
    const int groups = TN_THREADS / G, g = threadIdx.x / G, i = threadIdx.x % G;
    double row = 0.0;
    for (int s0 = 0; s0 < S_; s0 += groups) {             // uniform trip count: every lane shuffles
        const int s = s0 + g;
        double acc = 0.0;
        if (s < S_) {
            const int64_t o = (int64_t)s * L;
            for (int l = i; l < L; l += G) {
                const float mq = mc[o + l] + my[o + l];
                const float lq = lq_[o + l], lp = lp_[o + l];
                const float dm = mq - my[o + l];
                const float v = 0.5f * (lp - lq - 1.f + (expf(lq) + dm * dm) / expf(lp));
                acc += (double)v;
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (s < S_) {
            if (i == 0) ts[r * S_ + s] = (float)(acc / (double)L);
            row += acc;
        }
    }
    if (i == 0) red[g] = row;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < groups; ++q) t += red[q];
        te[r] = (float)(t / (double)n);
    }
}

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(TN_THREADS) void k_tenull_stats(
    const float* __restrict__ ts, const float* __restrict__ te, int K1, int S_, int* __restrict__ count_ge,
    int* __restrict__ step_count_ge, int* __restrict__ max_count_ge, double* __restrict__ surr_mean,
    double* __restrict__ surr_sd, float* __restrict__ step_surr_mean) {
    __shared__ float s_mx[TN_MAX_K1];
    __shared__ float s_te[TN_MAX_K1];
    __shared__ int s_cnt[TN_THREADS / 64];
    const int64_t b = blockIdx.x;
    const float* tsb = ts + b * K1 * S_;
    const float* teb = te + b * K1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // phase 1: a wave per variant, its lanes over the steps
    for (int k = w; k < K1; k += TN_THREADS / 64) {
        const float* row = tsb + (int64_t)k * S_;
        float m = -INFINITY;
        for (int s = lane; s < S_; s += 64) {
            const float v = row[s];
            m = v > m ? v : m;                            // a NaN is never taken
        }
        m = wave_max_f(m);
        if (lane == 0) s_mx[k] = m;
    }
    for (int k = threadIdx.x; k < K1; k += TN_THREADS) s_te[k] = teb[k];
    __syncthreads();
    // the row mean's rank, and the surrogates' moments by one thread in k order
    {
        const float obs = s_te[0];
        int c = 0;
        for (int k = 1 + threadIdx.x; k < K1; k += TN_THREADS) c += s_te[k] >= obs ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[w] = c;
    }
    __syncthreads();
    if (threadIdx.x == TN_THREADS - 1) {                  // the last wave has the fewest steps below
        int c = 0;
        for (int q = 0; q < TN_THREADS / 64; ++q) c += s_cnt[q];
        count_ge[b] = c;
        const double K = (double)(K1 - 1);
        double sum = 0.0;
        for (int k = 1; k < K1; ++k) sum += (double)s_te[k];
        const double mean = sum / K;
        double ss = 0.0;
        for (int k = 1; k < K1; ++k) {
            const double d = (double)s_te[k] - mean;
            ss += d * d;
        }
        surr_mean[b] = mean;
        surr_sd[b] = sqrt(ss / (K - 1.0));                // K = 1: 0 / 0, a NaN
    }
    // phase 2: a thread per step, k in order; a wave reads 64 adjacent steps of one variant
    for (int s = threadIdx.x; s < S_; s += TN_THREADS) {
        const float obs = tsb[s];
        int c = 0, cm = 0;
        double sum = 0.0;
        for (int k = 1; k < K1; ++k) {
            const float v = tsb[(int64_t)k * S_ + s];
            c += v >= obs ? 1 : 0;
            cm += s_mx[k] >= obs ? 1 : 0;
            sum += (double)v;
        }
        step_count_ge[b * S_ + s] = c;
        max_count_ge[b * S_ + s] = cm;
        step_surr_mean[b * S_ + s] = (float)(sum / (double)(K1 - 1));
    }
}

__global__ __launch_bounds__(TN_THREADS) void k_tenull_group(const float* __restrict__ te, int64_t B, int K1,
                                                             double* __restrict__ group_sums) {
    const int k = blockIdx.x * TN_THREADS + threadIdx.x;
    if (k >= K1) return;
    double sum = 0.0;
    for (int64_t b = 0; b < B; ++b) sum += (double)te[b * K1 + k];
    group_sums[k] = sum;
}

}  // namespace vt

using namespace vt;

extern "C" {

int vt_te_kl_steps(const float* mu_c, const float* lv_q, const float* mu_y, const float* lv_p, int64_t B, int K,
                   int S_, int L, float* ts, float* te, void* stream) {
    VT_CHECK_ARG(B > 0 && K > 0 && S_ > 0 && L > 0, "vt_te_kl_steps: B/K/S/L");
    VT_CHECK_ARG(B * K < (1ll << 31) && (int64_t)S_ * L < (1ll << 31), "vt_te_kl_steps: grid / row size");
    VT_CHECK_ARG(mu_c != nullptr && lv_q != nullptr && mu_y != nullptr && lv_p != nullptr && ts != nullptr &&
                     te != nullptr,
                 "vt_te_kl_steps: null pointer");
    int G = 1;
    while (G < L && G < 64) G <<= 1;
    hipLaunchKernelGGL(k_te_kl_steps, dim3((unsigned)(B * K)), dim3(TN_THREADS), 0, S(stream), mu_c, lv_q, mu_y, lv_p,
                       K, S_, L, G, ts, te);
    VT_LAUNCH_CHECK("vt_te_kl_steps");
    return VT_OK;
}

int vt_tenull_stats(const float* ts, const float* te, int64_t B, int K1, int S_, int* count_ge, int* step_count_ge,
                    int* max_count_ge, double* surr_mean, double* surr_sd, float* step_surr_mean,
                    double* group_sums, void* stream) {
    VT_CHECK_ARG(B > 0 && B < (1ll << 31) && S_ > 0, "vt_tenull_stats: B/S");
    VT_CHECK_ARG(K1 >= 2 && K1 <= TN_MAX_K1, "vt_tenull_stats: K1=%d outside [2, %d]", K1, TN_MAX_K1);
    VT_CHECK_ARG(B * S_ < (1ll << 31), "vt_tenull_stats: B * S");
    VT_CHECK_ARG(ts != nullptr && te != nullptr && count_ge != nullptr && step_count_ge != nullptr &&
                     max_count_ge != nullptr && surr_mean != nullptr && surr_sd != nullptr &&
                     step_surr_mean != nullptr && group_sums != nullptr,
                 "vt_tenull_stats: null pointer");
    hipLaunchKernelGGL(k_tenull_stats, dim3((unsigned)B), dim3(TN_THREADS), 0, S(stream), ts, te, K1, S_, count_ge,
                       step_count_ge, max_count_ge, surr_mean, surr_sd, step_surr_mean);
    VT_LAUNCH_CHECK("vt_tenull_stats");
    hipLaunchKernelGGL(k_tenull_group, dim3((unsigned)((K1 + TN_THREADS - 1) / TN_THREADS)), dim3(TN_THREADS), 0,
                       S(stream), te, B, K1, group_sums);
    VT_LAUNCH_CHECK("vt_tenull_stats");
    return VT_OK;
}

}  // extern "C"
