// Dataset normalisation statistics from the front-end's raw features (include/vaeteb.h,
// "dataset statistics"): per-channel {count, sum, sum of squares} in fp64, one pass over the
// fp32 features, no fp64 copy of them.
// replaces: _update_multi_channel_stats / _update_single_channel_stats
//           (ref/hdf5_dataset/calculate_dataset_stats.py:134-221)
//
// Two launches, both deterministic:
//   k_stats_partial  one workgroup per (chunk, channel); a chunk is VT_STATS_CHUNK_ROWS batch
//                    rows x VT_STATS_CHUNK_COLS steps.  Thread t takes elements t, t + 256, ...
//                    of the chunk (consecutive lanes read consecutive steps), a butterfly over
//                    the wave and a fixed sum over the 4 waves give the chunk's partial.
//   k_stats_combine  one thread per channel adds the channel's partials in chunk order and
//                    then adds the total to the persistent state.
// The kernel boundary orders the partials before the combine; there are no floating-point
// atomics (the library is built with -munsafe-fp-atomics), and the chunking is a function of
// the shapes alone, so the sums do not depend on the device or on what else is running.
// fp64 by design: the statistics are finalised as sum_sq / n - mean^2, which cancels; the pass
// runs once per dataset, not once per step.
#include "common.h"

namespace vt {
namespace {

constexpr int ST_T = 256;
constexpr int ST_ROWS = VT_STATS_CHUNK_ROWS;
constexpr int ST_COLS = VT_STATS_CHUNK_COLS;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// partial arrays are [chunk][channel]
__global__ __launch_bounds__(ST_T) void k_stats_partial(const float* __restrict__ in, int64_t B, int C, int in_C,
                                                        int64_t in_S, int s0, int S_len,
                                                        const int* __restrict__ kind, double log_eps, int n_cc,
                                                        double* __restrict__ psum, double* __restrict__ psq,
                                                        int64_t* __restrict__ pcnt) {
    __shared__ double sh_s[ST_T / 64], sh_q[ST_T / 64];
    __shared__ int sh_n[ST_T / 64];
    const int c = (int)(blockIdx.x % (unsigned)C);
    const int64_t p = blockIdx.x / (unsigned)C;
    const int64_t r0 = (p / n_cc) * ST_ROWS;
    const int c0 = (int)(p % n_cc) * ST_COLS;
    const int nr = (int)(B - r0 < ST_ROWS ? B - r0 : ST_ROWS);
    const int nc = S_len - c0 < ST_COLS ? S_len - c0 : ST_COLS;
    const int n = nr * nc;   // <= 32 * 1024
    const int k = kind != nullptr ? kind[c] : 0;
    const float* base = in + ((r0 * in_C + c) * in_S + s0 + c0);
    const int64_t row = (int64_t)in_C * in_S;
    double s = 0.0, q = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += ST_T) {
        const int r = i / nc, j = i - r * nc;
        const double x = (double)base[r * row + j];
        if (!__builtin_isfinite(x)) continue;
        double t = x;
        if (k == 1) t = log(fmax(x, 0.0) + log_eps);
        else if (k == 2) t = asinh(x);
        if (!__builtin_isfinite(t)) continue;
        s += t;
        q += t * t;
        ++cnt;
    }
    s = wave_sum_d(s);
    q = wave_sum_d(q);
    cnt = wave_sum_i(cnt);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        sh_s[w] = s;
        sh_q[w] = q;
        sh_n[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = sh_s[0], tq = sh_q[0];
        int tn = sh_n[0];
        for (int i = 1; i < ST_T / 64; ++i) {
            ts += sh_s[i];
            tq += sh_q[i];
            tn += sh_n[i];
        }
        const int64_t o = p * C + c;
        psum[o] = ts;
        psq[o] = tq;
        pcnt[o] = tn;
    }
}

__global__ __launch_bounds__(64) void k_stats_combine(int64_t P, int C, const double* __restrict__ psum,
                                                      const double* __restrict__ psq,
                                                      const int64_t* __restrict__ pcnt, int64_t* __restrict__ count,
                                                      double* __restrict__ sum, double* __restrict__ sum_sq) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    int64_t n = 0;
    for (int64_t p = 0; p < P; ++p) {   // chunk order, never arrival order
        s += psum[p * C + c];
        q += psq[p * C + c];
        n += pcnt[p * C + c];
    }
    count[c] += n;
    sum[c] += s;
    sum_sq[c] += q;
}

int64_t n_chunks(int64_t B, int S_len, int* n_cc) {
    *n_cc = (S_len + ST_COLS - 1) / ST_COLS;
    return ((B + ST_ROWS - 1) / ST_ROWS) * *n_cc;
}

int stats_launch(const char* name, const float* in, int64_t B, int C, int in_C, int64_t in_S, int s0, int S_len,
                 const int* kind, double log_eps, int64_t* count, double* sum, double* sum_sq, void* work,
                 int64_t work_bytes, void* stream) {
    VT_CHECK_ARG(B > 0 && C > 0 && S_len > 0 && in_C >= C && s0 >= 0 && (int64_t)s0 + S_len <= in_S,
                 "%s: shape (B %lld, C %d of %d, steps [%d, %d + %d) of %lld)", name, (long long)B, C, in_C, s0, s0,
                 S_len, (long long)in_S);
    VT_CHECK_ARG(in != nullptr && count != nullptr && sum != nullptr && sum_sq != nullptr && work != nullptr,
                 "%s: null buffer", name);
    VT_CHECK_ARG(log_eps >= 0.0, "%s: log_eps %g", name, log_eps);
    int n_cc = 0;
    const int64_t P = n_chunks(B, S_len, &n_cc);
    VT_CHECK_ARG(P <= 0x7fffffff / C, "%s: %lld chunks x %d channels exceed one grid", name, (long long)P, C);
    VT_CHECK_ARG(((uintptr_t)work & 7u) == 0 && work_bytes >= P * C * 24,
                 "%s: workspace of %lld bytes (8-byte aligned) needed, got %lld", name, (long long)(P * C * 24),
                 (long long)work_bytes);
    double* psum = (double*)work;
    double* psq = psum + P * C;
    int64_t* pcnt = (int64_t*)(psq + P * C);
    hipLaunchKernelGGL(k_stats_partial, dim3((unsigned)(P * C)), dim3(ST_T), 0, S(stream), in, B, C, in_C, in_S, s0,
                       S_len, kind, log_eps, n_cc, psum, psq, pcnt);
    VT_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(k_stats_combine, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, S(stream), P, C,
                       (const double*)psum, (const double*)psq, (const int64_t*)pcnt, count, sum, sum_sq);
    VT_LAUNCH_CHECK(name);
    return VT_OK;
}

}  // namespace
}  // namespace vt

using namespace vt;

extern "C" {

int vt_stats_chunking(int* rows, int* cols) {
    VT_CHECK_ARG(rows != nullptr && cols != nullptr, "vt_stats_chunking: null");
    *rows = ST_ROWS;
    *cols = ST_COLS;
    return VT_OK;
}

int vt_stats_workspace_bytes(int64_t B, int C, int S_len, int64_t* bytes) {
    VT_CHECK_ARG(B > 0 && C > 0 && S_len > 0 && bytes != nullptr, "vt_stats_workspace_bytes: shape");
    int n_cc = 0;
    const int64_t P = n_chunks(B, S_len, &n_cc);
    VT_CHECK_ARG(P <= 0x7fffffff / C, "vt_stats_workspace_bytes: %lld chunks x %d channels exceed one grid",
                 (long long)P, C);
    *bytes = P * C * 24;
    return VT_OK;
}

int vt_stats_accum(const float* in, int64_t B, int C, int in_C, int in_S, int s0, int S_len, const int* kind,
                   double log_eps, int64_t* count, double* sum, double* sum_sq, void* work, int64_t work_bytes,
                   void* stream) {
    return stats_launch("vt_stats_accum", in, B, C, in_C, in_S, s0, S_len, kind, log_eps, count, sum, sum_sq, work,
                        work_bytes, stream);
}

int vt_stats_accum_raw(const float* x, int64_t rows, int64_t row_stride, int N, int64_t* count, double* sum,
                       double* sum_sq, void* work, int64_t work_bytes, void* stream) {
    return stats_launch("vt_stats_accum_raw", x, rows, 1, 1, row_stride, 0, N, nullptr, 0.0, count, sum, sum_sq,
                        work, work_bytes, stream);
}

}  // extern "C"
