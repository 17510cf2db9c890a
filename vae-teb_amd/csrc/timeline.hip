// Windows -> recording timelines (C-ABI in include/vaeteb.h, Python side vaeteb/timeline.py):
//   vt_timeline_accumulate  overlapping windows added into packed per-position running sums
//                           (the canvas loop of SeqVaeTeb.get_predictions,
//                           ref/model/vae_teb_model.py:1228-1244, without the canvas)
//   vt_timeline_finish      weighted mean (torch.nanmean, :1246) and denormalize_signal_data
//                           (ref/model/graph_model.py:83-85) in one pass
//   vt_timeline_metrics     k_recon_metrics_rows (evalm.hip) over a recording's covered positions
//
// Gather, not scatter-add: a position is owned by one thread (inner == 1) or one half-wave
// (inner > 1).  The owner finds the windows that cover it in the ascending offset table and adds
// them in ascending window order into the fp32 sums it loaded, so the result has one order of
// additions whatever the grid is, and an ascending window list cut into consecutive calls repeats
// the single call's additions exactly.  No atomics, no LDS outside the metrics reduction.
#include "common.h"

// every product, sum and quotient below is rounded on its own (the finish pass is specified as
// quotient, product, sum; the accumulate pass must add the same way in every build)
#pragma clang fp contract(off)

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_WAVES = TL_THREADS / 64;
constexpr int TL_GROUP = 32;          // lanes that own one position when inner > 1
constexpr int TL_MAX_BLOCKS = 8192;   // the position loops are grid-stride past this

// first j in [0, W) with off[j] >= key (W when none)
__device__ __forceinline__ int64_t tl_lower_bound(const int64_t* __restrict__ off, int64_t W, int64_t key) {
    int64_t lo = 0, hi = W;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float tl_weight(int blend, int i, int n) {
    return blend ? (float)(i + 1 < n - i ? i + 1 : n - i) : 1.f;
}

// LANES == 1: thread t of the grid owns positions p0 + t, p0 + t + threads, ...
// LANES == TL_GROUP: half-wave g owns positions p0 + g, p0 + g + groups, ...; its lanes stride over
// the inner axis, keep double partial sums and combine them by xor shuffles inside the half-wave
// (every lane of a half-wave has the same p, so the whole half-wave takes the same branches).
template <int LANES>
__global__ __launch_bounds__(TL_THREADS) void k_timeline_accumulate(
    const float* __restrict__ vals, int64_t W, int n, int inner, const int64_t* __restrict__ dst_off,
    const int* __restrict__ len, int blend, float* __restrict__ acc, float* __restrict__ wacc, int* __restrict__ count,
    int64_t total) {
    int64_t p0 = dst_off[0], p1 = dst_off[W - 1] + n;
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > total ? total : p1;
    const int64_t owners = (int64_t)gridDim.x * (TL_THREADS / LANES);
    const int sub = LANES == 1 ? 0 : (int)(threadIdx.x & (LANES - 1));
    const double div = (double)inner;
    for (int64_t p = p0 + (int64_t)blockIdx.x * (TL_THREADS / LANES) + threadIdx.x / LANES; p < p1; p += owners) {
        int64_t j = tl_lower_bound(dst_off, W, p - n + 1);
        float a = 0.f, w = 0.f;
        int c = 0, seen = 0;
        for (; j < W; ++j) {
            const int64_t o = dst_off[j];
            if (o > p) break;
            int lj = len != nullptr ? len[j] : n;
            lj = lj > n ? n : lj;
            if (p - o >= lj) continue;
            const int i = (int)(p - o);                      // 0 <= i < len[j] <= n
            if (!seen) {
                a = acc[p], w = wacc[p], c = count[p];
                seen = 1;
            }
            const float* __restrict__ v = vals + (j * (int64_t)n + i) * inner;
            float vj;
            if (LANES == 1) {
                if (inner == 1) {
                    vj = v[0];
                } else {
                    double s = 0.0;
                    for (int l = 0; l < inner; ++l) s += (double)v[l];
                    vj = (float)(s / div);
                }
            } else {
                double s = 0.0;
                for (int l = sub; l < inner; l += LANES) s += (double)v[l];
#pragma unroll
                for (int m = LANES >> 1; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
                vj = (float)(s / div);
            }
            const float wj = tl_weight(blend, i, n);
            const float t = wj * vj;
            // the first window of a position starts its sums: m windows cost m - 1 additions
            a = c == 0 ? t : a + t;
            w = c == 0 ? wj : w + wj;
            c += 1;
        }
        if (seen && sub == 0) acc[p] = a, wacc[p] = w, count[p] = c;
    }
}

__device__ __forceinline__ float tl_finish_one(float a, float w, int c, float fill, float scale, float shift) {
    const float q = a / w;
    const float m = q * scale;
    return c ? m + shift : fill;
}

__global__ __launch_bounds__(TL_THREADS) void k_timeline_finish(const float* __restrict__ acc,
                                                                const float* __restrict__ wacc,
                                                                const int* __restrict__ count, int64_t total,
                                                                int vec, float fill, float scale, float shift,
                                                                float* __restrict__ out) {
    const int64_t threads = (int64_t)gridDim.x * TL_THREADS;
    const int64_t t0 = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x;
    int64_t done = 0;
    if (vec) {   // all four bases 16-byte aligned
        const int64_t n4 = total >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(acc);
        const float4* w4 = reinterpret_cast<const float4*>(wacc);
        const int4* c4 = reinterpret_cast<const int4*>(count);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int64_t i = t0; i < n4; i += threads) {
            const float4 a = a4[i], w = w4[i];
            const int4 c = c4[i];
            float4 o;
            o.x = tl_finish_one(a.x, w.x, c.x, fill, scale, shift);
            o.y = tl_finish_one(a.y, w.y, c.y, fill, scale, shift);
            o.z = tl_finish_one(a.z, w.z, c.z, fill, scale, shift);
            o.w = tl_finish_one(a.w, w.w, c.w, fill, scale, shift);
            o4[i] = o;
        }
        done = n4 << 2;
    }
    for (int64_t i = done + t0; i < total; i += threads)
        out[i] = tl_finish_one(acc[i], wacc[i], count[i], fill, scale, shift);
}

__device__ __forceinline__ double tl_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum of v over the workgroup, the same value in every thread: wave sums added in index order.
__device__ __forceinline__ double tl_block_sum_d(double v, double* red) {
    v = tl_wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < TL_WAVES; ++w) t += red[w];
    __syncthreads();
    return t;
}

// k_recon_metrics_rows (evalm.hip) over the covered positions of recording blockIdx.x
__global__ __launch_bounds__(TL_THREADS) void k_timeline_metrics(const float* __restrict__ y,
                                                                 const float* __restrict__ recon,
                                                                 const int* __restrict__ count,
                                                                 const int64_t* __restrict__ base,
                                                                 float* __restrict__ out) {
    __shared__ double red[TL_WAVES];
    const int64_t r = blockIdx.x;
    const int64_t b0 = base[r], b1 = base[r + 1];
    double sy = 0.0, sr = 0.0, syy = 0.0, srr = 0.0, sc = 0.0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += TL_THREADS) {
        if (count[i] > 0) {
            const float yf = y[i];
            const float rf = yf - recon[i];        // the reference's float32 subtraction
            const double yd = (double)yf, rd = (double)rf;
            sy += yd, sr += rd, syy += yd * yd, srr += rd * rd, sc += 1.0;
        }
    }
    const double covered = tl_block_sum_d(sc, red);   // an integer below 2^53: exact
    const double inv_n = 1.0 / covered;
    const double mean_y = tl_block_sum_d(sy, red) * inv_n;
    const double mean_r = tl_block_sum_d(sr, red) * inv_n;
    const double sig = tl_block_sum_d(syy, red) * inv_n;
    const double mse = tl_block_sum_d(srr, red) * inv_n;
    double cy = 0.0, cr = 0.0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += TL_THREADS) {
        if (count[i] > 0) {
            const float yf = y[i];
            const float rf = yf - recon[i];
            const double dy = (double)yf - mean_y, dr = (double)rf - mean_r;
            cy += dy * dy, cr += dr * dr;
        }
    }
    const double var_y = tl_block_sum_d(cy, red) * inv_n;
    const double var_r = tl_block_sum_d(cr, red) * inv_n;
    if (threadIdx.x == 0) {
        float* o = out + r * 5;
        if (covered > 0.0) {
            const double vu = var_y > 1e-12 ? 1.0 - var_r / var_y : 0.0;
            const double vaf = vu < 0.0 ? 0.0 : (vu > 1.0 ? 1.0 : vu);
            const double snr = mse > 1e-12 ? 10.0 * log10(sig / mse) : 100.0;
            o[0] = (float)vaf, o[1] = (float)mse, o[2] = (float)snr, o[3] = (float)vu;
            o[4] = (float)(covered / (double)(b1 - b0));
        } else {
            const float nan = __builtin_nanf("");
            o[0] = nan, o[1] = nan, o[2] = nan, o[3] = nan, o[4] = 0.f;
        }
    }
}

inline unsigned tl_blocks(int64_t owners, int per_block) {
    const int64_t b = (owners + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > TL_MAX_BLOCKS ? TL_MAX_BLOCKS : b));
}

}  // namespace

extern "C" {

int vt_timeline_accumulate(const float* vals, int64_t W, int n, int inner, const int64_t* dst_off, const int* len,
                           int blend, float* acc, float* wacc, int* count, int64_t total, void* stream) {
    VT_CHECK_ARG(n >= 1 && inner >= 1 && W >= 0 && total >= 0 && (blend == 0 || blend == 1),
                 "vt_timeline_accumulate: W=%lld n=%d inner=%d total=%lld blend=%d", (long long)W, n, inner,
                 (long long)total, blend);
    if (W == 0 || total == 0) return VT_OK;
    VT_CHECK_ARG(vals != nullptr && dst_off != nullptr && acc != nullptr && wacc != nullptr && count != nullptr,
                 "vt_timeline_accumulate: null pointer");
    // the positions of the call lie in a span of at most min(total, W * n + gaps); the grid is sized
    // by the covered part and strides over the rest
    const int64_t span = W * (int64_t)n < total ? W * (int64_t)n : total;
    if (inner == 1) {
        k_timeline_accumulate<1><<<dim3(tl_blocks(span, TL_THREADS)), dim3(TL_THREADS), 0, vt::S(stream)>>>(
            vals, W, n, inner, dst_off, len, blend, acc, wacc, count, total);
    } else {
        k_timeline_accumulate<TL_GROUP>
            <<<dim3(tl_blocks(span, TL_THREADS / TL_GROUP)), dim3(TL_THREADS), 0, vt::S(stream)>>>(
                vals, W, n, inner, dst_off, len, blend, acc, wacc, count, total);
    }
    VT_LAUNCH_CHECK("vt_timeline_accumulate");
    return VT_OK;
}

int vt_timeline_finish(const float* acc, const float* wacc, const int* count, int64_t total, float fill,
                       float scale, float shift, float* out, void* stream) {
    VT_CHECK_ARG(total >= 0, "vt_timeline_finish: total=%lld", (long long)total);
    if (total == 0) return VT_OK;
    VT_CHECK_ARG(acc != nullptr && wacc != nullptr && count != nullptr && out != nullptr,
                 "vt_timeline_finish: null pointer");
    const int vec = ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(wacc) |
                      reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int64_t items = vec ? (total + 3) / 4 : total;
    k_timeline_finish<<<dim3(tl_blocks(items, TL_THREADS)), dim3(TL_THREADS), 0, vt::S(stream)>>>(
        acc, wacc, count, total, vec, fill, scale, shift, out);
    VT_LAUNCH_CHECK("vt_timeline_finish");
    return VT_OK;
}

int vt_timeline_metrics(const float* y, const float* recon, const int* count, const int64_t* base, int64_t R,
                        float* out, void* stream) {
    VT_CHECK_ARG(R >= 0 && R < (1ll << 31), "vt_timeline_metrics: R=%lld", (long long)R);
    if (R == 0) return VT_OK;
    VT_CHECK_ARG(y != nullptr && recon != nullptr && count != nullptr && base != nullptr && out != nullptr,
                 "vt_timeline_metrics: null pointer");
    k_timeline_metrics<<<dim3((unsigned)R), dim3(TL_THREADS), 0, vt::S(stream)>>>(y, recon, count, base, out);
    VT_LAUNCH_CHECK("vt_timeline_metrics");
    return VT_OK;
}

}  // extern "C"
