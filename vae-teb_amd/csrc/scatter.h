// Pieces shared by the batched Scattering1D cascade (scatter.hip) and its
// backward (scatter_bwd.hip): the workgroup size and the row fold.
#pragma once
#include "fft.h"

namespace vt {

namespace {

constexpr int SC_THREADS = 512;

// One workgroup folds one row: dst[m] = (1/k) sum_c src[m + c L] f[m + c L],
// m < L (cdgmm + subsample_fourier).  L >= SC_THREADS: a thread per bin, c
// serial; L < SC_THREADS: G = SC_THREADS / L threads per bin take every G-th c
// and their partials are summed in fixed order through `red` (LDS, SC_THREADS
// float2).  Reads are unit-stride across the workgroup either way.  Ends with
// a barrier when dst is LDS.
template <bool DST_LDS>
__device__ __forceinline__ void fold_row(const float2* __restrict__ src, const float* __restrict__ f, int L, int k,
                                         float2* dst, float2* red) {
    const int t = threadIdx.x;
    const float sc = 1.0f / (float)k;
    if (L >= SC_THREADS) {
        for (int m = t; m < L; m += SC_THREADS) {
            float2 s = make_float2(0.f, 0.f);
            for (int c = 0; c < k; ++c) s = cadd(s, cscale(src[(int64_t)c * L + m], f[(int64_t)c * L + m]));
            dst[m] = cscale(s, sc);
        }
        if (DST_LDS) __syncthreads();
        return;
    }
    const int G = SC_THREADS / L;   // L, SC_THREADS powers of two
    const int m = t % L, g = t / L;
    float2 s = make_float2(0.f, 0.f);
    for (int c = g; c < k; c += G) s = cadd(s, cscale(src[(int64_t)c * L + m], f[(int64_t)c * L + m]));
    red[t] = s;
    __syncthreads();
    if (t < L) {
        float2 a = red[t];
        for (int gg = 1; gg < G; ++gg) a = cadd(a, red[gg * L + t]);
        dst[t] = cscale(a, sc);
    }
    __syncthreads();
}

inline bool pow2i(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace
}  // namespace vt
