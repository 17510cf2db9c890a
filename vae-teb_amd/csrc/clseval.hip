// Statistics of the classifier evaluation (vaeteb/clseval.py): given the class-1
// probability p of every kept window, one launch per statistic and integer results only.
//
//   k_cls_alarm_sweep   first[r, t]: the first kept window of recording r at which the strike rule
//                       raises the alarm under threshold t, -1 if none.  Grid (recordings, threshold
//                       tiles): the workgroup stages a chunk of the recording's p and ordinals in LDS
//                       once, every thread owns one threshold and walks the chunk (all lanes read the
//                       same LDS word: a broadcast); run / count / first are carried in registers from
//                       chunk to chunk.
//   k_cls_confusion     counts[g, t] = {tp, fp, tn, fn} of the windows of group g under threshold t.
//                       Grid (threshold tiles, groups, window slabs): the same staging, a thread counts
//                       its threshold's firing positives and negatives over the slab; integer atomics
//                       into the zeroed output when there is more than one slab.
//   k_cls_auc_ranks     {gt, eq, P, N} of a weighted window set from the ascending order of p: one
//                       workgroup per (replicate, group) scans the order once in spans of CE_SPAN.
//
// No floating-point accumulation anywhere: every sum is an integer sum, so the results are exact,
// identical run to run and independent of the launch geometry.  The comparisons are float32
// comparisons of the stored values (p > thr strict, ties by ==), which a NaN never satisfies.
// Every index read from a device table (rec_base, order, rec) is range-checked before it is used.
#include "common.h"

namespace vt {

static constexpr int CE_THREADS = 256;
static constexpr int CE_WAVES = CE_THREADS / 64;
static constexpr int CE_CHUNK = 1024;                     // windows staged per pass (alarm, confusion)
static constexpr int CE_SLAB = 8 * CE_CHUNK;              // windows per workgroup of the confusion kernel
static constexpr int CE_PER = 4;                          // consecutive sorted windows per thread
static constexpr int CE_SPAN = CE_THREADS * CE_PER;       // windows per block scan of the AUC kernel

__global__ __launch_bounds__(CE_THREADS) void k_cls_alarm_sweep(
    const float* __restrict__ p, int64_t W, const int64_t* __restrict__ rec_base, const int* __restrict__ ordinal,
    const float* __restrict__ thr, int T, int strike, int mode, int* __restrict__ first) {
    __shared__ float s_p[CE_CHUNK];
    __shared__ int s_brk[CE_CHUNK];                       // 1: the run restarts at this window
    const int64_t r = blockIdx.x;
    const int t = blockIdx.y * CE_THREADS + threadIdx.x;
    int64_t a = rec_base[r], b = rec_base[r + 1];
    a = a < 0 ? 0 : (a > W ? W : a);
    b = b < a ? a : (b > W ? W : b);
    const float th = t < T ? thr[t] : 0.f;
    int run = 0, found = -1;
    for (int64_t c0 = a; c0 < b; c0 += CE_CHUNK) {
        const int nc = (int)(b - c0 < CE_CHUNK ? b - c0 : CE_CHUNK);
        __syncthreads();                                  // the previous chunk has been walked
        for (int i = threadIdx.x; i < nc; i += CE_THREADS) {
            const int64_t j = c0 + i;
            s_p[i] = p[j];
            s_brk[i] = (ordinal != nullptr && j > a && ordinal[j] != ordinal[j - 1] + 1) ? 1 : 0;
        }
        __syncthreads();
        if (found < 0) {
            for (int i = 0; i < nc; ++i) {
                const bool fire = s_p[i] > th;
                if (mode == 0) {
                    if (s_brk[i]) run = 0;
                    run = fire ? run + 1 : 0;
                } else {
                    run += fire ? 1 : 0;
                }
                if (run >= strike) {
                    found = (int)(c0 - a) + i;
                    break;
                }
            }
        }
    }
    if (t < T) first[r * T + t] = found;
}

__global__ __launch_bounds__(CE_THREADS) void k_cls_confusion(
    const float* __restrict__ p, const uint8_t* __restrict__ label, const int* __restrict__ group, int64_t W,
    const float* __restrict__ thr, int T, int* __restrict__ counts, int use_atomics) {
    __shared__ float s_p[CE_CHUNK];
    __shared__ int s_l[CE_CHUNK];                         // 1 positive, 0 negative, -1 not in this group
    const int g = blockIdx.y;
    const int t = blockIdx.x * CE_THREADS + threadIdx.x;
    const int64_t a = (int64_t)blockIdx.z * CE_SLAB;
    const int64_t b = a + CE_SLAB < W ? a + CE_SLAB : W;
    const float th = t < T ? thr[t] : 0.f;
    int tp = 0, fp = 0, np_ = 0, nn = 0;
    for (int64_t c0 = a; c0 < b; c0 += CE_CHUNK) {
        const int nc = (int)(b - c0 < CE_CHUNK ? b - c0 : CE_CHUNK);
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += CE_THREADS) {
            const int64_t j = c0 + i;
            s_p[i] = p[j];
            const int gj = group != nullptr ? group[j] : 0;
            s_l[i] = gj == g ? (label[j] != 0 ? 1 : 0) : -1;
        }
        __syncthreads();
        for (int i = 0; i < nc; ++i) {
            const int l = s_l[i];
            if (l < 0) continue;                          // uniform: every lane reads the same word
            const int fire = s_p[i] > th ? 1 : 0;
            np_ += l, nn += 1 - l;
            tp += fire & l, fp += fire & (1 - l);
        }
    }
    if (t < T) {
        int* o = counts + ((int64_t)g * T + t) * 4;
        const int v[4] = {tp, fp, nn - fp, np_ - tp};
        if (use_atomics) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (v[c] != 0) atomicAdd(o + c, v[c]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = v[c];
        }
    }
}

struct ce_pair {
    long long a, b;
};
struct ce_sum {
    static __device__ __forceinline__ long long id() { return 0; }
    static __device__ __forceinline__ long long op(long long x, long long y) { return x + y; }
};
struct ce_max {
    static __device__ __forceinline__ long long id() { return -1; }
    static __device__ __forceinline__ long long op(long long x, long long y) { return x > y ? x : y; }
};

// Exclusive scan over the workgroup's threads of the pair v (both members under Op); *total: the
// reduction over all threads.  red holds CE_WAVES pairs; two barriers.
template <class Op>
__device__ __forceinline__ ce_pair ce_block_scan(ce_pair v, ce_pair* total, ce_pair* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    ce_pair inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long xa = __shfl_up(inc.a, o, 64), xb = __shfl_up(inc.b, o, 64);
        if (lane >= o) inc.a = Op::op(xa, inc.a), inc.b = Op::op(xb, inc.b);
    }
    __syncthreads();                                      // red is free again
    if (lane == 63) red[w] = inc;
    __syncthreads();
    ce_pair ex;
    ex.a = __shfl_up(inc.a, 1, 64), ex.b = __shfl_up(inc.b, 1, 64);
    if (lane == 0) ex.a = Op::id(), ex.b = Op::id();
    ce_pair pre = {Op::id(), Op::id()}, tot = {Op::id(), Op::id()};
#pragma unroll
    for (int q = 0; q < CE_WAVES; ++q) {
        if (q < w) pre.a = Op::op(pre.a, red[q].a), pre.b = Op::op(pre.b, red[q].b);
        tot.a = Op::op(tot.a, red[q].a), tot.b = Op::op(tot.b, red[q].b);
    }
    *total = tot;
    ex.a = Op::op(pre.a, ex.a), ex.b = Op::op(pre.b, ex.b);
    return ex;
}

// Sorted position k carries the window order[k] with weight w (0 outside the group, for a NaN p or
// a bad index), split into negative weight nw and positive weight pw by its label.  Nex_k / Pex_k:
// the negative / positive weight at positions < k.  A tie group starts at k (a head) when
// p_sorted[k] != p_sorted[k - 1]; Ns_k / Ps_k are Nex / Pex at the head of k's group — Nex and Pex
// never decrease, so they are the running maxima of the heads' values (a max-scan, carried across
// spans for a group that a span border cuts).  Then
//   gt = sum_k pw_k Ns_k                                   negatives strictly below a positive
//   eq = sum_k pw_k (Nex_k - Ns_k) + nw_k (Pex_k - Ps_k)   every (positive, negative) pair of a group once
__global__ __launch_bounds__(CE_THREADS) void k_cls_auc_ranks(
    const float* __restrict__ p_sorted, const int64_t* __restrict__ order, int64_t W,
    const uint8_t* __restrict__ label, const int* __restrict__ rec, const int* __restrict__ group,
    const int* __restrict__ mult, int64_t R, long long* __restrict__ out) {
    __shared__ ce_pair red[CE_WAVES];
    const int64_t rep = blockIdx.x;
    const int g = blockIdx.y, G = gridDim.y;
    const int* mrow = mult != nullptr ? mult + rep * R : nullptr;
    long long run_n = 0, run_p = 0;                       // negative / positive weight before the span
    long long open_n = 0, open_p = 0;                     // Ns / Ps of the tie group open at the span's start
    long long gt = 0, eq = 0;
    for (int64_t s0 = 0; s0 < W; s0 += CE_SPAN) {
        long long nw[CE_PER], pw[CE_PER];
        bool head[CE_PER];
        const int64_t k0 = s0 + (int64_t)CE_PER * threadIdx.x;
        ce_pair tsum = {0, 0};
#pragma unroll
        for (int c = 0; c < CE_PER; ++c) {
            const int64_t k = k0 + c;
            nw[c] = 0, pw[c] = 0, head[c] = false;
            if (k < W) {
                const float v = p_sorted[k];
                head[c] = k == 0 || v != p_sorted[k - 1];
                const int64_t i = order[k];
                if (v == v && i >= 0 && i < W && (group != nullptr ? group[i] : 0) == g) {
                    long long w = 1;
                    if (mrow != nullptr) {
                        const int rr = rec[i];
                        w = (rr >= 0 && rr < R) ? (long long)mrow[rr] : 0;
                    }
                    if (label[i] != 0) pw[c] = w; else nw[c] = w;
                }
            }
            tsum.a += nw[c], tsum.b += pw[c];
        }
        ce_pair tot_s, tot_m;
        const ce_pair off = ce_block_scan<ce_sum>(tsum, &tot_s, red);
        long long nex = run_n + off.a, pex = run_p + off.b;
        // the last head this thread holds, as (Nex, Pex) there; none: the identity
        ce_pair hm = {-1, -1};
        {
            long long n2 = nex, p2 = pex;
#pragma unroll
            for (int c = 0; c < CE_PER; ++c) {
                if (head[c]) hm.a = n2, hm.b = p2;
                n2 += nw[c], p2 += pw[c];
            }
        }
        const ce_pair before = ce_block_scan<ce_max>(hm, &tot_m, red);
        long long ns = before.a > open_n ? before.a : open_n;
        long long ps = before.b > open_p ? before.b : open_p;
#pragma unroll
        for (int c = 0; c < CE_PER; ++c) {
            if (head[c]) ns = nex, ps = pex;
            gt += pw[c] * ns;
            eq += pw[c] * (nex - ns) + nw[c] * (pex - ps);
            nex += nw[c], pex += pw[c];
        }
        run_n += tot_s.a, run_p += tot_s.b;
        open_n = tot_m.a > open_n ? tot_m.a : open_n;
        open_p = tot_m.b > open_p ? tot_m.b : open_p;
    }
    ce_pair tot;
    const ce_pair acc = {gt, eq};
    ce_block_scan<ce_sum>(acc, &tot, red);
    if (threadIdx.x == 0) {
        long long* o = out + (rep * G + g) * 4;
        o[0] = tot.a, o[1] = tot.b, o[2] = run_p, o[3] = run_n;
    }
}

}  // namespace vt

using namespace vt;

extern "C" {

int vt_cls_scan_span(void) { return CE_SPAN; }
int vt_cls_stage_chunk(void) { return CE_CHUNK; }

int vt_cls_alarm_sweep(const float* p, int64_t W, const int64_t* rec_base, int64_t R, const int* ordinal,
                       const float* thr, int T, int strike, int mode, int* first, void* stream) {
    VT_CHECK_ARG(W >= 0 && W < (1ll << 31) && R >= 0 && R < (1ll << 31) && T >= 0 && T <= (1 << 24),
                 "vt_cls_alarm_sweep: W / R (below 2^31) / T (at most 2^24)");
    VT_CHECK_ARG(strike >= 1, "vt_cls_alarm_sweep: strike must be at least 1, got %d", strike);
    VT_CHECK_ARG(mode == 0 || mode == 1, "vt_cls_alarm_sweep: mode must be 0 (consecutive) or 1 (cumulative), got %d",
                 mode);
    if (R == 0 || T == 0) return VT_OK;
    VT_CHECK_ARG(rec_base != nullptr && thr != nullptr && first != nullptr && (p != nullptr || W == 0),
                 "vt_cls_alarm_sweep: null pointer");
    const unsigned tiles = (unsigned)((T + CE_THREADS - 1) / CE_THREADS);
    hipLaunchKernelGGL(k_cls_alarm_sweep, dim3((unsigned)R, tiles), dim3(CE_THREADS), 0, S(stream), p, W, rec_base,
                       ordinal, thr, T, strike, mode, first);
    VT_LAUNCH_CHECK("vt_cls_alarm_sweep");
    return VT_OK;
}

int vt_cls_confusion(const float* p, const uint8_t* label, const int* group, int64_t W, int G, const float* thr, int T,
                     int* counts, void* stream) {
    VT_CHECK_ARG(W >= 0 && W < (1ll << 31) && G >= 0 && G <= 65535 && T >= 0 && T <= (1 << 24),
                 "vt_cls_confusion: W (below 2^31) / G (at most 65535) / T (at most 2^24)");
    if (G == 0 || T == 0) return VT_OK;
    VT_CHECK_ARG(thr != nullptr && counts != nullptr && ((p != nullptr && label != nullptr) || W == 0),
                 "vt_cls_confusion: null pointer");
    const int64_t slabs = W > 0 ? (W + CE_SLAB - 1) / CE_SLAB : 1;
    VT_CHECK_ARG(slabs <= 65535, "vt_cls_confusion: at most %lld windows", 65535ll * CE_SLAB);
    if (slabs > 1) {
        const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * 4 * (size_t)G * (size_t)T, S(stream));
        if (e != hipSuccess) {
            set_error("vt_cls_confusion: %s", hipGetErrorString(e));
            return VT_ERR_HIP;
        }
    }
    const unsigned tiles = (unsigned)((T + CE_THREADS - 1) / CE_THREADS);
    hipLaunchKernelGGL(k_cls_confusion, dim3(tiles, (unsigned)G, (unsigned)slabs), dim3(CE_THREADS), 0, S(stream), p,
                       label, group, W, thr, T, counts, slabs > 1 ? 1 : 0);
    VT_LAUNCH_CHECK("vt_cls_confusion");
    return VT_OK;
}

int vt_cls_auc_ranks(const float* p_sorted, const int64_t* order, int64_t W, const uint8_t* label, const int* rec,
                     const int* group, int G, const int* mult, int64_t Bt, int64_t R, int64_t* out, void* stream) {
    VT_CHECK_ARG(W >= 0 && W < (1ll << 31) && G >= 0 && G <= 65535 && Bt >= 0 && Bt < (1ll << 31) && R >= 0 &&
                     R < (1ll << 31),
                 "vt_cls_auc_ranks: W / Bt / R (below 2^31) / G (at most 65535)");
    if (G == 0 || Bt == 0) return VT_OK;
    VT_CHECK_ARG(out != nullptr && ((p_sorted != nullptr && order != nullptr && label != nullptr) || W == 0),
                 "vt_cls_auc_ranks: null pointer");
    VT_CHECK_ARG(mult == nullptr || (rec != nullptr || W == 0), "vt_cls_auc_ranks: mult needs rec");
    static_assert(sizeof(long long) == sizeof(int64_t), "int64_t");
    hipLaunchKernelGGL(k_cls_auc_ranks, dim3((unsigned)Bt, (unsigned)G), dim3(CE_THREADS), 0, S(stream), p_sorted,
                       order, W, label, rec, group, mult, R, reinterpret_cast<long long*>(out));
    VT_LAUNCH_CHECK("vt_cls_auc_ranks");
    return VT_OK;
}

}  // extern "C"
