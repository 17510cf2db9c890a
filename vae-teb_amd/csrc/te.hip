// Transfer entropy per (recording, shift) row (vaeteb/te.py, the shift sweep).
//
// te[r] = mean over (S, L) of KL(q(z | x_r, y) || p(z | y)) elementwise, the reference's
// kld_tensor.mean() of one measure_transfer_entropy(reduce_mean=False) call
// (ref/model/graph_model.py:1371, ref/model/vae_teb_model.py:1071-1082, :1194-1226).  The posterior
// pieces mu_c / lv_q have one row per (recording, shift); the prior mu_y / lv_p has one row per
// recording and is read at row r / K (no broadcast copy).  The elementwise expression and its
// operation order are k_latent_fwd's (elbo.hip).
//
// One workgroup per row.  Every element's fp32 KL is widened to double before it is added, lane
// sums are combined by wave shuffles, wave sums through LDS, and thread 0 adds the wave sums in
// index order: no atomics, the same order every run, and a row's result depends on nothing but
// that row (so it does not move when the rows are split over several calls).
#include "common.h"

namespace vt {

static constexpr int TE_THREADS = 256;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(TE_THREADS) void k_te_kl_rows(const float* __restrict__ mu_c,
                                                           const float* __restrict__ lv_q,
                                                           const float* __restrict__ mu_y,
                                                           const float* __restrict__ lv_p, int K, int64_t n,
                                                           float* __restrict__ te, float* __restrict__ kl) {
    __shared__ double red[TE_THREADS / 64];
    const int64_t r = blockIdx.x;
    const float* mc = mu_c + r * n;
    const float* lq_ = lv_q + r * n;
    const float* my = mu_y + (r / K) * n;
    const float* lp_ = lv_p + (r / K) * n;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += TE_THREADS) {
        const float mq = mc[i] + my[i];
        const float lq = lq_[i], lp = lp_[i];
        const float dm = mq - my[i];
        const float v = 0.5f * (lp - lq - 1.f + (expf(lq) + dm * dm) / expf(lp));
        if (kl != nullptr) kl[r * n + i] = v;
        acc += (double)v;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < TE_THREADS / 64; ++w) t += red[w];
        te[r] = (float)(t / (double)n);
    }
}

}  // namespace vt

using namespace vt;

extern "C" {

int vt_te_kl_rows(const float* mu_c, const float* lv_q, const float* mu_y, const float* lv_p, int64_t B, int K,
                  int64_t row_elems, float* te, float* kl, void* stream) {
    VT_CHECK_ARG(B > 0 && K > 0 && row_elems > 0, "vt_te_kl_rows: B/K/row_elems");
    VT_CHECK_ARG(B * K < (1ll << 31), "vt_te_kl_rows: grid");
    VT_CHECK_ARG(mu_c != nullptr && lv_q != nullptr && mu_y != nullptr && lv_p != nullptr && te != nullptr,
                 "vt_te_kl_rows: null pointer");
    hipLaunchKernelGGL(k_te_kl_rows, dim3((unsigned)(B * K)), dim3(TE_THREADS), 0, S(stream), mu_c, lv_q, mu_y, lv_p,
                       K, row_elems, te, kl);
    VT_LAUNCH_CHECK("vt_te_kl_rows");
    return VT_OK;
}

}  // extern "C"
