// Backward of the batched Scattering1D cascade (scatter.hip) and of the
// plugin's pad / subsample_fourier: the adjoints of the forward launches, with
// respect to the data operand only (filters are constants).  Gradients of
// complex buffers are stored as (d/d re, d/d im), as torch autograd does for
// the reference's trailing-dim-2 tensors (ref/kymatio/kymatio/backend/
// torch_backend.py:5-96 for the modulus convention).
//
//   k_scat_lowpass_bwd   forward  X[m] = (1/k) sum_c U[m + c Lp] phi[m + c Lp],
//                                 out[t] = Re ifft_Lp(X)[i0 + t]
//                        backward g (B, C, S) row ch[p] placed at [i0, i1) of a
//                                 zero complex row, gX = fft(.) / Lp in LDS,
//                                 gU[m + c Lp] = phi[m + c Lp] gX[m] / k
//   k_scat_mod_spec_bwd  forward  X = fold(A, psi_p), z = ifft_L(X), U^ = fft(|z|)
//                        backward gu = Re(unnormalised ifft(gU^)), gz = gu z / |z|
//                                 (0 where |z| = 0, the ModulusStable convention of
//                                 k_modulus_bwd), gX = fft(gz) / L; z is recomputed
//                                 from A as the forward does.  LDS: z + a ping-pong
//                                 pair + red = (3 L + 512) * 8 bytes: 100 KiB at
//                                 L = 4096, 196 KiB at 8192 (160 KiB per CU), so
//                                 L <= VT_SCAT_BWD_MAX_LDS = 4096; longer rows are
//                                 composed by the caller from vt_scat_filter_sub,
//                                 vt_fft / vt_fft_large and k_modulus_cplx_bwd
//   k_scat_fold_bwd      adjoint of cdgmm + subsample summed over the filters that
//                        share a parent: gA[b, a, i] = (1/k) sum_{p: a_idx[p] = a}
//                        psi_p[i] gX[b, p, i mod L]; one thread per output bin
//                        over a host-built CSR of a_idx in fixed order, no atomics
//                        (bitwise reproducible)
//   k_modulus_cplx_bwd   gz = Re(G) z / |z| for the composed route
//   k_pad_reflect_bwd    gx[i] = g[pl+i] + g[pl-i] (1 <= i <= pl)
//                                + g[pl+2N-2-i] (N-1-pr <= i <= N-2); pad < N, so a
//                        single reflection
//   k_subsample_fourier_bwd  gx[m + c L] = g[m] / k
#include "scatter.h"

namespace vt {

namespace {

constexpr int SCB_MAX_LDS = 4096;   // largest row of the fused k_scat_mod_spec_bwd

// row r = (b, p): g[b, ch[p], :] -> gU[r] (length n)
__global__ __launch_bounds__(SC_THREADS) void k_scat_lowpass_bwd(const float* __restrict__ g, int P, int n,
                                                                 const float* __restrict__ phi, int k, int i0,
                                                                 int i1, const int* __restrict__ ch, int out_C,
                                                                 const float2* __restrict__ tw,
                                                                 float2* __restrict__ gU) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int Lp = n / k;
    float2* X = sm;
    float2* Y = X + Lp;
    const int64_t r = blockIdx.x, b = r / P;
    const int p = (int)(r - b * P);
    const int S = i1 - i0;
    const float* src = g + (b * out_C + ch[p]) * S;
    for (int i = threadIdx.x; i < Lp; i += SC_THREADS)
        X[i] = make_float2(i >= i0 && i < i1 ? src[i - i0] : 0.f, 0.f);
    __syncthreads();
    const float2* R = fft_lds<false>(X, Y, Lp, tw, 1);
    const float sc = 1.0f / ((float)Lp * (float)k);
    float2* dst = gU + r * n;
    for (int m = threadIdx.x; m < n; m += SC_THREADS) dst[m] = cscale(R[m & (Lp - 1)], phi[m] * sc);
}

// row r = (b, p): A[b, a_idx[p]] (length n), gUh[r] (length L = n / k) -> gX[r] (length L)
__global__ __launch_bounds__(SC_THREADS) void k_scat_mod_spec_bwd(const float2* __restrict__ A, int64_t a_rows, int n,
                                                                  const int* __restrict__ a_idx,
                                                                  const float* __restrict__ pool,
                                                                  const int64_t* __restrict__ f_off, int P, int k,
                                                                  const float2* __restrict__ tw,
                                                                  const float2* __restrict__ gUh,
                                                                  float2* __restrict__ gX) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int L = n / k;
    float2* red = sm;
    float2* Z0 = sm + SC_THREADS;
    float2* Z1 = Z0 + L;
    float2* Z2 = Z1 + L;
    const int64_t r = blockIdx.x, b = r / P;
    const int p = (int)(r - b * P);
    const float2* gsrc = gUh + r * L;
    for (int i = threadIdx.x; i < L; i += SC_THREADS) Z2[i] = gsrc[i];
    fold_row<true>(A + (b * a_rows + a_idx[p]) * n, pool + f_off[p], L, k, Z0, red);
    const float2* Z = fft_lds<true>(Z0, Z1, L, tw, 1);    // L z, kept
    float2* T = Z == Z0 ? Z1 : Z0;
    float2* G = fft_lds<true>(Z2, T, L, tw, 1);           // unnormalised ifft(gU^)
    float2* F = G == Z2 ? T : Z2;
    for (int i = threadIdx.x; i < L; i += SC_THREADS) {
        const float2 z = Z[i];
        const float m = sqrtf(z.x * z.x + z.y * z.y);
        G[i] = m == 0.f ? make_float2(0.f, 0.f) : cscale(z, G[i].x / m);
    }
    __syncthreads();
    const float2* O = fft_lds<false>(G, F, L, tw, 1);
    const float sc = 1.0f / (float)L;
    float2* dst = gX + r * L;
    for (int i = threadIdx.x; i < L; i += SC_THREADS) dst[i] = cscale(O[i], sc);
}

// gA[b, a, i], i < n: children of parent a are cp[ptr[a]] .. cp[ptr[a + 1]) in fixed order
__global__ __launch_bounds__(256) void k_scat_fold_bwd(const float2* __restrict__ gX, int a_rows, int n,
                                                       const int* __restrict__ ptr, const int* __restrict__ cp,
                                                       const float* __restrict__ pool,
                                                       const int64_t* __restrict__ f_off, int P, int k,
                                                       float2* __restrict__ gA) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int a = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int L = n / k, m = i & (L - 1);
    float2 s = make_float2(0.f, 0.f);
    for (int q = ptr[a]; q < ptr[a + 1]; ++q) {
        const int p = cp[q];
        s = cadd(s, cscale(gX[(b * P + p) * L + m], pool[f_off[p] + i]));
    }
    gA[(b * a_rows + a) * n + i] = cscale(s, 1.0f / (float)k);
}

// out may be G (element-wise, in place)
__global__ void k_modulus_cplx_bwd(const float2* __restrict__ z, const float2* G, float2* out, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const float2 v = z[i];
        const float m = sqrtf(v.x * v.x + v.y * v.y);
        out[i] = m == 0.f ? make_float2(0.f, 0.f) : cscale(v, G[i].x / m);
    }
}

// g: rows of n_out = N + pl + pr elements, g_stride floats apart (2: the real part of a complex row)
__global__ void k_pad_reflect_bwd(const float* __restrict__ g, int g_stride, float scale, float* __restrict__ gx,
                                  int64_t rows, int N, int pl, int pr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * N) return;
    const int64_t r = t / N;
    const int i = (int)(t - r * N);
    const float* row = g + r * (int64_t)(N + pl + pr) * g_stride;
    float s = row[(int64_t)(pl + i) * g_stride];
    if (i >= 1 && i <= pl) s += row[(int64_t)(pl - i) * g_stride];
    if (i >= N - 1 - pr && i <= N - 2) s += row[(int64_t)(pl + 2 * N - 2 - i) * g_stride];
    gx[t] = s * scale;
}

// g: rows of L = n / k complex -> gx: rows of n complex
__global__ void k_subsample_fourier_bwd(const float2* __restrict__ g, float2* __restrict__ gx, int64_t rows, int n,
                                        int k) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * n) return;
    const int L = n / k;
    const int64_t r = t / n;
    const int i = (int)(t - r * n);
    gx[t] = cscale(g[r * L + i % L], 1.0f / (float)k);
}

}  // namespace
}  // namespace vt

using namespace vt;

extern "C" {

int vt_scat_lowpass_bwd(const float* g, int B, int P, int n, const float* phi, int k, int i0, int i1, const int* ch,
                        int out_C, const void* tw, void* gU, void* stream) {
    VT_CHECK_ARG(B > 0 && P > 0 && pow2i(n) && pow2i(k) && n / k >= 4 && n / k <= VT_FFT_MAX_LDS && 0 <= i0 &&
                     i0 < i1 && i1 <= n / k && out_C > 0,
                 "vt_scat_lowpass_bwd: n=%d k=%d [%d, %d)", n, k, i0, i1);
    const int Lp = n / k;
    hipLaunchKernelGGL(k_scat_lowpass_bwd, dim3((unsigned)((int64_t)B * P)), dim3(SC_THREADS),
                       (size_t)2 * Lp * sizeof(float2), S(stream), g, P, n, phi, k, i0, i1, ch, out_C,
                       (const float2*)tw, (float2*)gU);
    VT_LAUNCH_CHECK("vt_scat_lowpass_bwd");
    return VT_OK;
}

int vt_scat_mod_spec_bwd(const void* A, int B, int64_t a_rows, int n, const int* a_idx, const float* pool,
                         const int64_t* f_off, int P, int k, const void* tw, const void* gUh, void* gX,
                         void* stream) {
    VT_CHECK_ARG(B > 0 && a_rows > 0 && P > 0 && pow2i(n) && pow2i(k) && n / k >= 4 && n / k <= SCB_MAX_LDS,
                 "vt_scat_mod_spec_bwd: n=%d k=%d (n / k <= %d)", n, k, SCB_MAX_LDS);
    const int L = n / k;
    hipLaunchKernelGGL(k_scat_mod_spec_bwd, dim3((unsigned)((int64_t)B * P)), dim3(SC_THREADS),
                       (size_t)(SC_THREADS + 3 * L) * sizeof(float2), S(stream), (const float2*)A, a_rows, n, a_idx,
                       pool, f_off, P, k, (const float2*)tw, (const float2*)gUh, (float2*)gX);
    VT_LAUNCH_CHECK("vt_scat_mod_spec_bwd");
    return VT_OK;
}

int vt_scat_fold_bwd(const void* gX, int B, int a_rows, int n, const int* csr_ptr, const int* csr_p,
                     const float* pool, const int64_t* f_off, int P, int k, void* gA, void* stream) {
    VT_CHECK_ARG(B > 0 && B <= 65535 && a_rows > 0 && a_rows <= 65535 && P > 0 && pow2i(n) && pow2i(k) && k <= n,
                 "vt_scat_fold_bwd: B=%d a_rows=%d n=%d k=%d", B, a_rows, n, k);
    hipLaunchKernelGGL(k_scat_fold_bwd, dim3((unsigned)((n + 255) / 256), (unsigned)a_rows, (unsigned)B), dim3(256),
                       0, S(stream), (const float2*)gX, a_rows, n, csr_ptr, csr_p, pool, f_off, P, k, (float2*)gA);
    VT_LAUNCH_CHECK("vt_scat_fold_bwd");
    return VT_OK;
}

int vt_modulus_cplx_bwd(const void* z, const void* G, void* out, int64_t count, void* stream) {
    VT_CHECK_ARG(count > 0, "vt_modulus_cplx_bwd: empty");
    hipLaunchKernelGGL(k_modulus_cplx_bwd, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, S(stream),
                       (const float2*)z, (const float2*)G, (float2*)out, count);
    VT_LAUNCH_CHECK("vt_modulus_cplx_bwd");
    return VT_OK;
}

int vt_pad_reflect_bwd(const float* g, int g_stride, float scale, float* gx, int64_t rows, int N, int pad_left,
                       int pad_right, void* stream) {
    VT_CHECK_ARG(rows > 0 && N > 1 && g_stride >= 1 && pad_left >= 0 && pad_right >= 0 && pad_left < N &&
                     pad_right < N,
                 "vt_pad_reflect_bwd: N=%d pad=(%d, %d)", N, pad_left, pad_right);
    const int64_t total = rows * N;
    hipLaunchKernelGGL(k_pad_reflect_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(stream), g, g_stride,
                       scale, gx, rows, N, pad_left, pad_right);
    VT_LAUNCH_CHECK("vt_pad_reflect_bwd");
    return VT_OK;
}

int vt_subsample_fourier_bwd(const void* g, void* gx, int64_t rows, int n, int k, void* stream) {
    VT_CHECK_ARG(rows > 0 && k >= 1 && n % k == 0, "vt_subsample_fourier_bwd: n=%d k=%d", n, k);
    const int64_t total = rows * n;
    hipLaunchKernelGGL(k_subsample_fourier_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(stream),
                       (const float2*)g, (float2*)gx, rows, n, k);
    VT_LAUNCH_CHECK("vt_subsample_fourier_bwd");
    return VT_OK;
}

}  // extern "C"
