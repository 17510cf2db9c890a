// Row kernels of the batched evaluation sweep (vaeteb/evaluate.py): UP gain sweep, UP ablation and
// the reconstruction-metrics histogram of the reference (ref/model/graph_model.py:1510-1870), one
// row per (recording, gain).
//
//   k_eval_scale_rows     x_ph_base * float(g)                                      (:1833)
//   k_te_latent_rows      k_te_kl_rows (te.hip) + the reparameterisation of k_latent_fwd (elbo.hip):
//                         the same elementwise expressions in the same operation order, so te / kl
//                         are vt_te_kl_rows's bits and z / mu_post are vt_elbo_latent_fwd's
//   k_recon_metrics_rows  VAF / MSE / SNR of mu_pr against the raw FHR               (:1619-1645)
//
// As te.hip: one workgroup per row, every fp32 element value widened to double before it is added,
// lane sums combined by wave shuffles, wave sums through LDS and added in index order; no atomics,
// the same order every run, and a row's result depends on that row and its recording's row only
// (so it does not move when the rows are split over several calls).
#include "common.h"

namespace vt {

static constexpr int EV_THREADS = 256;
static constexpr int EV_WAVES = EV_THREADS / 64;

__device__ __forceinline__ double ev_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum of v over the workgroup, the same value in every thread: wave sums in index order.  `red`
// holds EV_WAVES doubles and is free for reuse on return.
__device__ __forceinline__ double ev_block_sum_d(double v, double* red) {
    v = ev_wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < EV_WAVES; ++w) t += red[w];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_scale_rows(const float* __restrict__ x, int K, int64_t n,
                                                                const float* __restrict__ gains,
                                                                float* __restrict__ out) {
    const int64_t r = blockIdx.x;
    const float g = gains[r % K];
    const float* xr = x + (r / K) * n;
    float* o = out + r * n;
    int64_t done = 0;
    if (((reinterpret_cast<uintptr_t>(xr) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(xr);
        float4* o4 = reinterpret_cast<float4*>(o);
        for (int64_t i = threadIdx.x; i < n4; i += EV_THREADS) {
            float4 v = x4[i];
            v.x *= g, v.y *= g, v.z *= g, v.w *= g;
            o4[i] = v;
        }
        done = n4 << 2;
    }
    for (int64_t i = done + threadIdx.x; i < n; i += EV_THREADS) o[i] = xr[i] * g;   // tail / unaligned row
}

__global__ __launch_bounds__(EV_THREADS) void k_te_latent_rows(
    const float* __restrict__ mu_c, const float* __restrict__ lv_q, const float* __restrict__ mu_y,
    const float* __restrict__ lv_p, const float* __restrict__ eps, int K, int64_t n, float* __restrict__ z,
    float* __restrict__ mu_post, float* __restrict__ te, float* __restrict__ kl) {
    __shared__ double red[EV_WAVES];
    const int64_t r = blockIdx.x;
    const float* mc = mu_c + r * n;
    const float* lq_ = lv_q + r * n;
    const float* ep = eps + r * n;
    const float* my = mu_y + (r / K) * n;
    const float* lp_ = lv_p + (r / K) * n;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += EV_THREADS) {
        const float mq = mc[i] + my[i];
        const float lq = lq_[i], lp = lp_[i];
        if (mu_post != nullptr) mu_post[r * n + i] = mq;
        z[r * n + i] = mq + ep[i] * expf(0.5f * lq);
        const float dm = mq - my[i];
        const float v = 0.5f * (lp - lq - 1.f + (expf(lq) + dm * dm) / expf(lp));
        if (kl != nullptr) kl[r * n + i] = v;
        acc += (double)v;
    }
    acc = ev_wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < EV_WAVES; ++w) t += red[w];
        te[r] = (float)(t / (double)n);
    }
}

// Two passes over the row (the second comes from L2): means first, then the centred squares, so
// the variances keep their digits under a mean far larger than the spread.
__global__ __launch_bounds__(EV_THREADS) void k_recon_metrics_rows(const float* __restrict__ y,
                                                                   const float* __restrict__ pr, int K, int64_t n,
                                                                   float* __restrict__ out) {
    __shared__ double red[EV_WAVES];
    const int64_t r = blockIdx.x;
    const float* yr = y + (r / K) * n;
    const float* pp = pr + r * n;
    double sy = 0.0, sr = 0.0, syy = 0.0, srr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += EV_THREADS) {
        const float yf = yr[i];
        const float rf = yf - pp[i];           // the reference's float32 subtraction
        const double yd = (double)yf, rd = (double)rf;
        sy += yd, sr += rd, syy += yd * yd, srr += rd * rd;
    }
    const double inv_n = 1.0 / (double)n;
    const double mean_y = ev_block_sum_d(sy, red) * inv_n;
    const double mean_r = ev_block_sum_d(sr, red) * inv_n;
    const double sig = ev_block_sum_d(syy, red) * inv_n;
    const double mse = ev_block_sum_d(srr, red) * inv_n;
    double cy = 0.0, cr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += EV_THREADS) {
        const float yf = yr[i];
        const float rf = yf - pp[i];
        const double dy = (double)yf - mean_y, dr = (double)rf - mean_r;
        cy += dy * dy, cr += dr * dr;
    }
    const double var_y = ev_block_sum_d(cy, red) * inv_n;
    const double var_r = ev_block_sum_d(cr, red) * inv_n;
    if (threadIdx.x == 0) {
        const double vu = var_y > 1e-12 ? 1.0 - var_r / var_y : 0.0;
        const double vaf = vu < 0.0 ? 0.0 : (vu > 1.0 ? 1.0 : vu);
        const double snr = mse > 1e-12 ? 10.0 * log10(sig / mse) : 100.0;
        float* o = out + r * 4;
        o[0] = (float)vaf, o[1] = (float)mse, o[2] = (float)snr, o[3] = (float)vu;
    }
}

}  // namespace vt

using namespace vt;

extern "C" {

int vt_eval_scale_rows(const float* x, int64_t B, int K, int64_t row_elems, const float* gains, float* out,
                       void* stream) {
    VT_CHECK_ARG(B > 0 && K > 0 && row_elems > 0, "vt_eval_scale_rows: B/K/row_elems");
    VT_CHECK_ARG(B * K < (1ll << 31), "vt_eval_scale_rows: grid");
    VT_CHECK_ARG(x != nullptr && gains != nullptr && out != nullptr, "vt_eval_scale_rows: null pointer");
    hipLaunchKernelGGL(k_eval_scale_rows, dim3((unsigned)(B * K)), dim3(EV_THREADS), 0, S(stream), x, K, row_elems,
                       gains, out);
    VT_LAUNCH_CHECK("vt_eval_scale_rows");
    return VT_OK;
}

int vt_te_latent_rows(const float* mu_c, const float* lv_q, const float* mu_y, const float* lv_p, const float* eps,
                      int64_t B, int K, int64_t row_elems, float* z, float* mu_post, float* te, float* kl,
                      void* stream) {
    VT_CHECK_ARG(B > 0 && K > 0 && row_elems > 0, "vt_te_latent_rows: B/K/row_elems");
    VT_CHECK_ARG(B * K < (1ll << 31), "vt_te_latent_rows: grid");
    VT_CHECK_ARG(mu_c != nullptr && lv_q != nullptr && mu_y != nullptr && lv_p != nullptr && eps != nullptr &&
                     z != nullptr && te != nullptr,
                 "vt_te_latent_rows: null pointer");
    hipLaunchKernelGGL(k_te_latent_rows, dim3((unsigned)(B * K)), dim3(EV_THREADS), 0, S(stream), mu_c, lv_q, mu_y,
                       lv_p, eps, K, row_elems, z, mu_post, te, kl);
    VT_LAUNCH_CHECK("vt_te_latent_rows");
    return VT_OK;
}

int vt_recon_metrics_rows(const float* y, const float* pr, int64_t B, int K, int64_t n, float* out, void* stream) {
    VT_CHECK_ARG(B > 0 && K > 0 && n > 0, "vt_recon_metrics_rows: B/K/n");
    VT_CHECK_ARG(B * K < (1ll << 31), "vt_recon_metrics_rows: grid");
    VT_CHECK_ARG(y != nullptr && pr != nullptr && out != nullptr, "vt_recon_metrics_rows: null pointer");
    hipLaunchKernelGGL(k_recon_metrics_rows, dim3((unsigned)(B * K)), dim3(EV_THREADS), 0, S(stream), y, pr, K, n,
                       out);
    VT_LAUNCH_CHECK("vt_recon_metrics_rows");
    return VT_OK;
}

}  // extern "C"
