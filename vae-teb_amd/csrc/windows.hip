// Recordings -> training windows (C-ABI in include/vaeteb.h, Python side vaeteb/windows.py):
//   vt_window_flat_stats  the signal-dropout gate's run-length statistics of every window row
//                         (find_flat_regions, ref/hdf5_dataset/create_hdf5_dataset.py:46-81, and
//                         the length arithmetic of :462-472), one wave per row
//   vt_window_gather      the kept rows copied out of the packed recordings into the (B, 2, N)
//                         batch the front-end takes
// A row is N consecutive floats at base + row_off[r]; rows overlap and start at any element.
// Neither kernel touches an element outside [row_off[r], row_off[r] + N).
#include "common.h"

namespace {

constexpr int WF_ROWS = 4;     // rows (waves) per 256-thread workgroup of the flat-stats kernel
constexpr int WF_TILES = 4;    // 64-sample tiles loaded ahead of the mask walk
constexpr int WG_CHUNK = 1024; // samples of one row a gather workgroup copies (256 threads x float4)

// Wave-uniform run-length state.  `open` counts the flat diffs of the run that reaches the
// current position (0: no run open); a run of m flat diffs is a region of m + 1 samples.
struct FlatState {
    int open, mx, total, count;
};

__device__ __forceinline__ void close_run(FlatState& s, int min_length) {
    const int len = s.open + 1;
    if (len >= min_length) {
        s.mx = len > s.mx ? len : s.mx;
        s.total += len;
        s.count += 1;
    }
    s.open = 0;
}

// Feed the 64 flat bits of one tile (bit l = diff ending at the tile's sample l) to the state.
__device__ __forceinline__ void walk_tile(FlatState& s, unsigned long long m, int min_length) {
    int rem = 64;   // bits of the tile not consumed yet; m is shifted so that bit 0 is the next one
    while (rem > 0) {
        if (!s.open) {
            if (m == 0ull) break;
            const int z = __builtin_ctzll(m);   // < 64 and < rem: a set bit lies inside the rest
            m >>= z;
            rem -= z;
        }
        const unsigned long long inv = ~m;
        const int ones = inv ? __builtin_ctzll(inv) : 64;   // <= rem: the shifts brought zeros in on top
        s.open += ones;
        if (ones == rem) break;   // the run reaches the tile's end and stays open
        close_run(s, min_length);
        m >>= ones;               // ones < rem <= 64
        rem -= ones;
    }
}

__global__ __launch_bounds__(64 * WF_ROWS) void k_window_flat_stats(const float* __restrict__ base,
                                                                    const int64_t* __restrict__ row_off, int64_t rows,
                                                                    int N, double tolerance, int min_length,
                                                                    int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * WF_ROWS + (threadIdx.x >> 6);
    if (r >= rows) return;   // whole waves leave: no barrier below
    const float* __restrict__ x = base + row_off[r];
    FlatState s = {0, 0, 0, 0};
    float carry = 0.f;   // the previous tile's last sample (unused for tile 0: its bit 0 is forced off)
    for (int t0 = 0; t0 < N; t0 += 64 * WF_TILES) {
        float v[WF_TILES];
#pragma unroll
        for (int k = 0; k < WF_TILES; ++k) {
            const int i = t0 + 64 * k + lane;
            v[k] = i < N ? x[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < WF_TILES; ++k) {
            const int i = t0 + 64 * k + lane;
            if (t0 + 64 * k < N) {   // wave-uniform
                float p = __shfl_up(v[k], 1, 64);
                if (lane == 0) p = carry;
                carry = __shfl(v[k], 63, 64);
                const bool flat = i > 0 && i < N && (double)fabsf(v[k] - p) <= tolerance;
                walk_tile(s, __ballot(flat), min_length);
            }
        }
    }
    if (s.open) close_run(s, min_length);   // a run still open at the last sample ends there
    if (lane == 0) {
        out[3 * r + 0] = s.mx;
        out[3 * r + 1] = s.total;
        out[3 * r + 2] = s.count;
    }
}

// block = (row r, chunk c): samples [c * WG_CHUNK, min(N, (c + 1) * WG_CHUNK)) of row r
__global__ __launch_bounds__(256) void k_window_gather(const float* __restrict__ base,
                                                       const int64_t* __restrict__ row_off, int chunks, int N,
                                                       float* __restrict__ out) {
    const int64_t r = blockIdx.x / chunks;
    const int c = blockIdx.x % chunks;
    const float* __restrict__ src = base + row_off[r];
    float* __restrict__ dst = out + r * (int64_t)N;
    const int j = c * WG_CHUNK + 4 * (int)threadIdx.x;
    if (j >= N) return;
    const bool vec = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;   // uniform over the row
    if (vec && j + 3 < N) {
        *reinterpret_cast<float4*>(dst + j) = *reinterpret_cast<const float4*>(src + j);
    } else {
        const int e = j + 4 < N ? j + 4 : N;
        for (int i = j; i < e; ++i) dst[i] = src[i];
    }
}

}  // namespace

extern "C" {

int vt_window_flat_stats(const float* base, const int64_t* row_off, int64_t rows, int N, double tolerance,
                         int min_length, int32_t* out, void* stream) {
    VT_CHECK_ARG(N >= 1 && min_length >= 1 && rows >= 0, "vt_window_flat_stats: rows=%lld N=%d min_length=%d",
                 (long long)rows, N, min_length);
    if (rows == 0) return VT_OK;
    VT_CHECK_ARG(base != nullptr && row_off != nullptr && out != nullptr, "vt_window_flat_stats: null pointer");
    const int64_t blocks = (rows + WF_ROWS - 1) / WF_ROWS;
    VT_CHECK_ARG(blocks < (1ll << 31), "vt_window_flat_stats: grid");
    k_window_flat_stats<<<dim3((unsigned)blocks), dim3(64 * WF_ROWS), 0, vt::S(stream)>>>(base, row_off, rows, N,
                                                                                         tolerance, min_length, out);
    VT_LAUNCH_CHECK("vt_window_flat_stats");
    return VT_OK;
}

int vt_window_gather(const float* base, const int64_t* row_off, int64_t rows, int N, float* out, void* stream) {
    VT_CHECK_ARG(N >= 1 && rows >= 0, "vt_window_gather: rows=%lld N=%d", (long long)rows, N);
    if (rows == 0) return VT_OK;
    VT_CHECK_ARG(base != nullptr && row_off != nullptr && out != nullptr, "vt_window_gather: null pointer");
    const int chunks = (N + WG_CHUNK - 1) / WG_CHUNK;
    VT_CHECK_ARG(rows < (1ll << 31) && rows * chunks < (1ll << 31), "vt_window_gather: grid");
    k_window_gather<<<dim3((unsigned)(rows * chunks)), dim3(256), 0, vt::S(stream)>>>(base, row_off, chunks, N, out);
    VT_LAUNCH_CHECK("vt_window_gather");
    return VT_OK;
}

}  // extern "C"
