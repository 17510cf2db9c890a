// Row kernels of the K-draw predictive distribution (vaeteb/predictive.py): K latent
// draws per recording, the decoder's Gaussian (mu_k, lv_k) for every draw, and the equal-weight
// mixture of the K Gaussians scored against the raw FHR y.  Rows r = b*K + k.
//
//   k_pred_draw_rows      z = mu + eps*exp(lv/2) (k_te_latent_rows's expression: the same bits) and
//                         logw = log p(z|y) - log q(z|x,y) of the row; one workgroup per row
//   k_pred_mixture_rows   per sample: mean, aleatoric / epistemic variance, mixture log density
//                         (online log-sum-exp over k) and PIT (mixture CDF at y); per sample tile:
//                         sum_i l_ki for every k, the sums of logdens / moment-matched NLL / sd and
//                         the PIT histogram and coverage counts, into the workspace.  Grid
//                         (sample tiles, B); mu and lv are read once.
//   k_pred_finish         one workgroup per recording: tile partials added in tile order, the
//                         importance weights added, the per-recording scalars written
//
// As evalm.hip: every fp32 element value is widened to double before it is added, lane sums go by
// wave shuffles, wave and tile sums are added in index order; no atomics (the counts are wave
// ballots), every workspace slot that is read was written by the same call, and a recording's
// results depend on that recording only.  The thread that owns a sample and the order of every sum
// do not depend on the alignment of the rows: the float4 path and the scalar path give equal bits.
#include "common.h"

namespace vt {

static constexpr int PD_THREADS = 256;
static constexpr int PD_WAVES = PD_THREADS / 64;
static constexpr int PD_PER = 4;                          // consecutive samples per thread
static constexpr int PD_TILE = PD_THREADS * PD_PER;       // samples per workgroup
static constexpr int PD_MAX_K = 64;
static constexpr int PD_MAX_BINS = 256;
static constexpr int PD_MAX_LEVELS = 8;
static constexpr int PD_SUMS = 3;                         // logdens, moment NLL, sd
static constexpr int PD_SCALARS = 5;                      // nll_mixture, nll_moment, sharpness, elbo, iwae
static constexpr float PD_LOG_2PI_F = 1.8378770664093453f;
static constexpr double PD_LOG_2PI = 1.8378770664093453;
static constexpr double PD_INF = __builtin_huge_val();

__device__ __forceinline__ double pd_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// v[c] = row[j0 + c] for c < nv, 0 beyond: one float4 when the four are in range and 16-byte aligned
// (j0 is a multiple of 4, so that is the row's own alignment), scalars otherwise.
__device__ __forceinline__ void pd_load4(const float* __restrict__ row, int64_t j0, int nv, float (&v)[PD_PER]) {
    const float* p = row + j0;
    if (nv == PD_PER && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < PD_PER; ++c) v[c] = c < nv ? p[c] : 0.f;
    }
}

__device__ __forceinline__ void pd_store4(float* __restrict__ row, int64_t j0, int nv, const float (&v)[PD_PER]) {
    float* p = row + j0;
    if (nv == PD_PER && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < PD_PER; ++c)
            if (c < nv) p[c] = v[c];
    }
}

__global__ __launch_bounds__(PD_THREADS) void k_pred_draw_rows(
    const float* __restrict__ mu, const float* __restrict__ lv, const float* __restrict__ eps,
    const float* __restrict__ mu_p, const float* __restrict__ lv_p, int K, int64_t m, float* __restrict__ z,
    float* __restrict__ logw) {
    __shared__ double red[PD_WAVES];
    const int64_t r = blockIdx.x;
    const float* mq_ = mu + (r / K) * m;
    const float* lq_ = lv + (r / K) * m;
    const float* ep = eps + r * m;
    double acc = 0.0;
    if (mu_p == nullptr) {
        for (int64_t i = threadIdx.x; i < m; i += PD_THREADS) z[r * m + i] = mq_[i] + ep[i] * expf(0.5f * lq_[i]);
    } else {
        const float* mp_ = mu_p + (r / K) * m;
        const float* lp_ = lv_p + (r / K) * m;
        for (int64_t i = threadIdx.x; i < m; i += PD_THREADS) {
            const float lq = lq_[i], lp = lp_[i], e = ep[i];
            const float zf = mq_[i] + e * expf(0.5f * lq);
            z[r * m + i] = zf;
            const float dz = zf - mp_[i];
            const float v = lq - lp + e * e - dz * dz * expf(-lp);
            acc += (double)v;
        }
    }
    acc = pd_wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < PD_WAVES; ++w) t += red[w];
        logw[r] = (float)(0.5 * t);
    }
}

// Workspace of one (recording, tile): [0, K) sum_i l_ki; [K, K+3) the sums of logdens, of the
// moment-matched NLL terms and of sqrt(v); then `bins` histogram counts and n_levels coverage counts
// (whole numbers held as doubles).
__global__ __launch_bounds__(PD_THREADS) void k_pred_mixture_rows(
    const float* __restrict__ y, const float* __restrict__ mu, const float* __restrict__ lv, int K, int64_t n,
    int bins, const double* __restrict__ levels, int n_levels, float* __restrict__ mean, float* __restrict__ var_a,
    float* __restrict__ var_e, float* __restrict__ pit, float* __restrict__ logdens, double* __restrict__ ws) {
    __shared__ double red_ll[PD_MAX_K][PD_WAVES];
    __shared__ double red_s[PD_SUMS][PD_WAVES];
    __shared__ int cnt[PD_WAVES][PD_MAX_BINS + PD_MAX_LEVELS];
    const int64_t b = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
    const int64_t j0 = tile * PD_TILE + (int64_t)PD_PER * threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t left = n - j0;
    const int nv = left >= PD_PER ? PD_PER : (left > 0 ? (int)left : 0);

    float yv[PD_PER], mk[PD_PER], lk[PD_PER];
    pd_load4(y + b * n, j0, nv, yv);
    double lm[PD_PER], ls[PD_PER], ps[PD_PER], va[PD_PER], sa[PD_PER], sb[PD_PER], mu0[PD_PER];
#pragma unroll
    for (int c = 0; c < PD_PER; ++c) lm[c] = -PD_INF, ls[c] = 0.0, ps[c] = 0.0, va[c] = 0.0, sa[c] = 0.0, sb[c] = 0.0, mu0[c] = 0.0;

    for (int k = 0; k < K; ++k) {
        const int64_t r = b * K + k;
        pd_load4(mu + r * n, j0, nv, mk);
        pd_load4(lv + r * n, j0, nv, lk);
        double llsum = 0.0;
#pragma unroll
        for (int c = 0; c < PD_PER; ++c) {
            const float d = yv[c] - mk[c];
            const float l = -0.5f * (PD_LOG_2PI_F + lk[c] + d * d * expf(-lk[c]));
            const double ld = (double)l;
            if (c < nv) llsum += ld;
            // online log-sum-exp: lm the running maximum, ls = sum exp(l - lm); a NaN stays in ls
            if (ld > lm[c]) {
                ls[c] = ls[c] * exp(lm[c] - ld) + 1.0;
                lm[c] = ld;
            } else if (ld != -PD_INF) {
                ls[c] += exp(ld - lm[c]);
            }
            const float t = d * expf(-0.5f * lk[c]);
            ps[c] += 0.5 * erfc(-(double)t * 0.70710678118654752440);
            va[c] += (double)expf(lk[c]);
            // spread about the first draw: exactly 0 when the draws coincide, no large-mean cancellation
            if (k == 0) mu0[c] = (double)mk[c];
            const double dm = (double)mk[c] - mu0[c];
            sa[c] += dm, sb[c] += dm * dm;
        }
        llsum = pd_wave_sum_d(llsum);
        if (lane == 0) red_ll[k][w] = llsum;
    }

    const double inv_k = 1.0 / (double)K, log_k = log((double)K);
    float o_mean[PD_PER], o_va[PD_PER], o_ve[PD_PER], o_pit[PD_PER], o_ld[PD_PER];
    int bin[PD_PER];
    unsigned cov[PD_PER];
    double s_ld = 0.0, s_mom = 0.0, s_sd = 0.0;
#pragma unroll
    for (int c = 0; c < PD_PER; ++c) {
        const double off = sa[c] * inv_k;
        const double mean_d = mu0[c] + off;
        const double va_d = va[c] * inv_k;
        double ve_d = sb[c] * inv_k - off * off;
        ve_d = ve_d < 0.0 ? 0.0 : ve_d;                  // keeps a NaN
        const double ld_d = lm[c] + log(ls[c]) - log_k;
        const double pit_d = ps[c] * inv_k;
        const double v = va_d + ve_d, res = (double)yv[c] - mean_d;
        o_mean[c] = (float)mean_d, o_va[c] = (float)va_d, o_ve[c] = (float)ve_d;
        o_pit[c] = (float)pit_d, o_ld[c] = (float)ld_d;
        bin[c] = -1, cov[c] = 0u;
        if (c < nv) {
            s_ld += ld_d;
            s_mom += 0.5 * (PD_LOG_2PI + log(v) + res * res / v);
            s_sd += sqrt(v);
            if (pit_d == pit_d) {                        // a NaN PIT is counted nowhere
                const int bi = (int)floor(pit_d * (double)bins);
                bin[c] = bi < bins - 1 ? bi : bins - 1;
                for (int l = 0; l < n_levels; ++l)
                    if (fabs(pit_d - 0.5) <= 0.5 * levels[l]) cov[c] |= 1u << l;
            }
        }
    }
    pd_store4(mean + b * n, j0, nv, o_mean);
    pd_store4(var_a + b * n, j0, nv, o_va);
    pd_store4(var_e + b * n, j0, nv, o_ve);
    if (pit != nullptr) pd_store4(pit + b * n, j0, nv, o_pit);
    if (logdens != nullptr) pd_store4(logdens + b * n, j0, nv, o_ld);

    // counts by wave ballot: whole numbers, no atomics
    for (int j = 0; j < bins; ++j) {
        int t = 0;
#pragma unroll
        for (int c = 0; c < PD_PER; ++c) t += __popcll(__ballot(bin[c] == j));
        if (lane == 0) cnt[w][j] = t;
    }
    for (int l = 0; l < n_levels; ++l) {
        int t = 0;
#pragma unroll
        for (int c = 0; c < PD_PER; ++c) t += __popcll(__ballot((cov[c] >> l) & 1u));
        if (lane == 0) cnt[w][bins + l] = t;
    }
    s_ld = pd_wave_sum_d(s_ld), s_mom = pd_wave_sum_d(s_mom), s_sd = pd_wave_sum_d(s_sd);
    if (lane == 0) red_s[0][w] = s_ld, red_s[1][w] = s_mom, red_s[2][w] = s_sd;
    __syncthreads();

    double* o = ws + (b * tiles + tile) * (int64_t)(K + PD_SUMS + bins + n_levels);
    const int t = threadIdx.x;
    if (t < K) {
        double s = 0.0;
        for (int q = 0; q < PD_WAVES; ++q) s += red_ll[t][q];
        o[t] = s;
    }
    if (t < PD_SUMS) {
        double s = 0.0;
        for (int q = 0; q < PD_WAVES; ++q) s += red_s[t][q];
        o[K + t] = s;
    }
    for (int j = t; j < bins + n_levels; j += PD_THREADS) {
        int s = 0;
        for (int q = 0; q < PD_WAVES; ++q) s += cnt[q][j];
        o[K + PD_SUMS + j] = (double)s;
    }
}

__global__ __launch_bounds__(PD_THREADS) void k_pred_finish(const double* __restrict__ ws,
                                                            const float* __restrict__ logw, int K, int64_t n,
                                                            int64_t tiles, int bins, int n_levels,
                                                            float* __restrict__ out, float* __restrict__ ll,
                                                            int* __restrict__ hist, float* __restrict__ coverage) {
    __shared__ double wk[PD_MAX_K];
    const int64_t b = blockIdx.x;
    const int64_t stride = K + PD_SUMS + bins + n_levels;
    const double* base = ws + b * tiles * stride;
    const double inv_n = 1.0 / (double)n;
    for (int j = threadIdx.x; j < stride; j += PD_THREADS) {
        double s = 0.0;
        for (int64_t q = 0; q < tiles; ++q) s += base[q * stride + j];
        if (j < K) {
            ll[b * K + j] = (float)s;
            wk[j] = s + (logw != nullptr ? (double)logw[b * K + j] : 0.0);
        } else if (j < K + PD_SUMS) {
            const int i = j - K;
            out[b * PD_SCALARS + i] = (float)((i == 0 ? -s : s) * inv_n);
        } else if (j < K + PD_SUMS + bins) {
            hist[b * bins + (j - K - PD_SUMS)] = (int)s;
        } else {
            coverage[b * n_levels + (j - K - PD_SUMS - bins)] = (float)(s * inv_n);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0, mx = -PD_INF;
        for (int k = 0; k < K; ++k) {
            sum += wk[k];
            if (wk[k] > mx) mx = wk[k];
        }
        double se = 0.0;
        for (int k = 0; k < K; ++k) se += wk[k] == mx ? 1.0 : exp(wk[k] - mx);   // a NaN weight stays
        out[b * PD_SCALARS + 3] = (float)(sum / (double)K);
        out[b * PD_SCALARS + 4] = (float)(mx + log(se) - log((double)K));
    }
}

}  // namespace vt

using namespace vt;

extern "C" {

int vt_pred_tile(void) { return PD_TILE; }

int vt_pred_draw_rows(const float* mu, const float* lv, const float* eps, const float* mu_p, const float* lv_p,
                      int64_t B, int K, int64_t row_elems, float* z, float* logw, void* stream) {
    VT_CHECK_ARG(B > 0 && K > 0 && row_elems > 0, "vt_pred_draw_rows: B/K/row_elems");
    VT_CHECK_ARG(B * K < (1ll << 31), "vt_pred_draw_rows: grid");
    VT_CHECK_ARG(mu != nullptr && lv != nullptr && eps != nullptr && z != nullptr && logw != nullptr,
                 "vt_pred_draw_rows: null pointer");
    VT_CHECK_ARG((mu_p == nullptr) == (lv_p == nullptr), "vt_pred_draw_rows: mu_p and lv_p go together");
    hipLaunchKernelGGL(k_pred_draw_rows, dim3((unsigned)(B * K)), dim3(PD_THREADS), 0, S(stream), mu, lv, eps, mu_p,
                       lv_p, K, row_elems, z, logw);
    VT_LAUNCH_CHECK("vt_pred_draw_rows");
    return VT_OK;
}

static int pred_check(const char* who, int64_t B, int K, int64_t n, int bins, int n_levels) {
    VT_CHECK_ARG(B > 0 && B <= 65535 && n > 0, "%s: B (1..65535) / n", who);
    VT_CHECK_ARG(K >= 1 && K <= PD_MAX_K, "%s: K must be in 1..%d, got %d", who, PD_MAX_K, K);
    VT_CHECK_ARG(bins >= 1 && bins <= PD_MAX_BINS, "%s: bins must be in 1..%d, got %d", who, PD_MAX_BINS, bins);
    VT_CHECK_ARG(n_levels >= 0 && n_levels <= PD_MAX_LEVELS, "%s: n_levels must be in 0..%d, got %d", who,
                 PD_MAX_LEVELS, n_levels);
    VT_CHECK_ARG((n + PD_TILE - 1) / PD_TILE < (1ll << 31), "%s: grid", who);
    return VT_OK;
}

int vt_pred_mixture_rows(const float* y, const float* mu, const float* lv, int64_t B, int K, int64_t n, int bins,
                         const double* levels, int n_levels, float* mean, float* var_aleatoric,
                         float* var_epistemic, float* pit, float* logdens, double* ws, void* stream) {
    const int rc = pred_check("vt_pred_mixture_rows", B, K, n, bins, n_levels);
    if (rc != VT_OK) return rc;
    VT_CHECK_ARG(y != nullptr && mu != nullptr && lv != nullptr && mean != nullptr && var_aleatoric != nullptr &&
                     var_epistemic != nullptr && ws != nullptr && (levels != nullptr || n_levels == 0),
                 "vt_pred_mixture_rows: null pointer");
    const int64_t tiles = (n + PD_TILE - 1) / PD_TILE;
    hipLaunchKernelGGL(k_pred_mixture_rows, dim3((unsigned)tiles, (unsigned)B), dim3(PD_THREADS), 0, S(stream), y, mu,
                       lv, K, n, bins, levels, n_levels, mean, var_aleatoric, var_epistemic, pit, logdens, ws);
    VT_LAUNCH_CHECK("vt_pred_mixture_rows");
    return VT_OK;
}

int vt_pred_finish(const double* ws, const float* logw, int64_t B, int K, int64_t n, int bins, int n_levels,
                   float* out, float* ll, int* pit_hist, float* coverage, void* stream) {
    const int rc = pred_check("vt_pred_finish", B, K, n, bins, n_levels);
    if (rc != VT_OK) return rc;
    VT_CHECK_ARG(B < (1ll << 31), "vt_pred_finish: grid");
    VT_CHECK_ARG(ws != nullptr && out != nullptr && ll != nullptr && pit_hist != nullptr &&
                     (coverage != nullptr || n_levels == 0),
                 "vt_pred_finish: null pointer");
    const int64_t tiles = (n + PD_TILE - 1) / PD_TILE;
    hipLaunchKernelGGL(k_pred_finish, dim3((unsigned)B), dim3(PD_THREADS), 0, S(stream), ws, logw, K, n, tiles, bins,
                       n_levels, out, ll, pit_hist, coverage);
    VT_LAUNCH_CHECK("vt_pred_finish");
    return VT_OK;
}

}  // extern "C"
