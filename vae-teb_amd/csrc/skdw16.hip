// LSTM parameter gradients on bf16 MFMA for the 16-bit recurrences (SURVEY.md §8(a) a12;
// ref/model/vae_teb_model.py:474-480, :647-653: nn.LSTM's weight_ih / weight_hh / biases
// under the reference's 16-mixed autocast, where cuDNN forms them from 16-bit gate
// gradients and inputs with fp32 accumulation — graph_model.py:510, :709-711).
//
//   [dW_ih | dW_hh | db] = bf16(dG)^T bf16([x | h_{t-1} | 1])   (fp32 accumulation)
//
// over the B*S rows of a layer (x [rows][In], h [rows][H] read one row back within each
// sample, zero at t = 0).  dG comes in one of two formats per layer: fp32 [rows][4H] (gate
// rows n = g H + u: vt_lstm16_layer_bwd), rounded to bf16 here, or the bf16 image [rows][4H]
// the pair / quad recurrences write (columns k' = 4 u + g, the rounding already done: half the
// bytes, and no conversion).  The MFMA operands hold the same bits either way, and the image's
// column permutation is undone where the partial slab is written, so the two formats give the
// same gradients bit for bit.
//
// One launch (k_sk_dw16m) serves up to 4 layers: blockIdx.y is the layer, blockIdx.x its row
// block.  The exact-fp32 path (mlp.hip k_sk_dw, v_mfma_f32_16x16x4_f32) is MFMA-bound at
// fp32's 157 TF; here the rows are the MFMA reduction (v_mfma_f32_16x16x32_bf16, 32 rows per
// k-step) and the kernel is bound by how many loads it keeps in flight.  A workgroup of 4 waves
// streams its row range in 32-row chunks through double-buffered LDS images (dG [32][4H],
// [x | h_{t-1} | 1] [32][16 NTK], row-major bf16): the next chunk's rows are loaded into
// registers before the current chunk's MFMAs and stored to the other buffer after them — one
// barrier per chunk — and two workgroups are resident per CU (53 KB of LDS, <= 256 VGPRs at 4
// waves each), so one's loads fly during the other's MFMAs.  Operand fragments are read with the
// gfx950 transposed LDS read (ds_read_b64_tr_b16, rows contiguous per fragment).  Each wave owns
// four whole 16-row tiles of dW (each [x | h | 1] fragment read once per k-step for all four).
// Per-workgroup partial slabs, summed in the fixed order of mlp.hip's k_sk_sum by one launch for
// all layers (k_sk_sum16).  A layer's row partition depends on the row count alone — not on the
// format, nor on how many layers share the launch or where the layer stands among them.
#include <type_traits>

#include "common.h"
#include "skinny.h"

namespace vt {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef short v8i16 __attribute__((ext_vector_type(8)));

constexpr int G = 256;       // 4 H gate rows (H = 64)
constexpr int CR = 32;       // rows per chunk (one MFMA k-step)
constexpr int DS = G + 8;    // bf16 row stride of the dG image (16 B mod 128 B: conflict-free transposed reads)
constexpr int XSM = 16 * 9 + 8;   // largest row stride of the [x | h_{t-1} | 1] image (NTK = 9)
constexpr int NTH = 256;     // 4 waves

struct Batch {
    Dw16Layer l[SK_DW16_MAX_LAYERS];
};

__device__ __forceinline__ bf16x8 tr_frag(const __bf16* img, int col0, int stride) {
    // lane 4q+p of each 16-lane group: row (8 g + q), columns col0 + 4p .. +3; rows
    // +0..3 and +4..7 of the group's 8-row block (conv_bf16.hip tr_frag)
    const int lane = threadIdx.x & 63, g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const __bf16* a0 = img + (8 * g + q) * stride + col0 + 4 * p;
    const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)a0);
    const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) v4i16*)(a0 + 4 * stride));
    const v8i16 r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ bf16x4 cvt4(float4 v) {
    return bf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}

// part[blk][n][k'] (k' < K1 = In + H + 1) = sum over the workgroup's rows [rb, re) of
// bf16(dG[r][n]) bf16(X1[r][k']), X1 = [x | h_{t-1} | 1].  IMG: dG is the bf16 image (column
// c = 4 u + g holds gate row n = g H + u), else fp32 by gate row.
template <int NTK, bool IMG>
__device__ __forceinline__ void dw16_body(const Dw16Layer& L, int S, int R, int rpb, __bf16* gs, __bf16* xs) {
    constexpr int XS = 16 * NTK + 8;            // bf16 row stride of the [x | h_{t-1} | 1] image
    constexpr int UG = IMG ? 4 : 8;             // 16-byte dG loads per thread and chunk
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int In = L.In, K1 = In + 64 + 1;
    const int ix4 = In / 4, ipr = ix4 + 16;     // float4 of x, of [x | h_{t-1}] per row
    const int xitems = CR * ipr;                // <= 1024: at most 4 per thread
    const float* __restrict__ x = L.x;
    const float* __restrict__ h = L.h;
    const int rb = (int)blockIdx.x * rpb < R ? (int)blockIdx.x * rpb : R;
    const int re = (int64_t)rb + rpb < R ? rb + rpb : R;
    const int nch = (re - rb + CR - 1) / CR;
    // the ones column and the zero padding of both X1 images are the same for every chunk
    {
        const int padc = 16 * NTK - In - 64;
        for (int i = tid; i < CR * padc; i += NTH) {
            const int t = i / padc, c = In + 64 + (i - t * padc);
            const __bf16 v = (__bf16)(c == K1 - 1 ? 1.f : 0.f);
            xs[t * XS + c] = v;
            xs[CR * XSM + t * XS + c] = v;
        }
    }
    // this thread's items of a chunk's [x | h_{t-1}] rows: chunk row, LDS offset, source, and
    // the step (row mod S) of the h items' rows, carried from chunk to chunk
    int xt[4], xo[4], xr[4];
    int xg[4];          // float offset into x (x item) or h (h item, row - 1) at chunk row 0
    bool xv[4], xh[4];
    const int cs = CR % S;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = tid + NTH * u;
        xv[u] = i < xitems;
        const int t = xv[u] ? i / ipr : 0, j = xv[u] ? i - t * ipr : 0;
        xt[u] = t;
        xh[u] = j >= ix4;
        xo[u] = t * XS + (xh[u] ? In + 4 * (j - ix4) : 4 * j);
        xg[u] = xh[u] ? (t - 1) * 64 + 4 * (j - ix4) : t * In + 4 * j;
        xr[u] = (rb + t) % S;
    }
    typedef typename std::conditional<IMG, uint4, float4>::type gv_t;
    gv_t vg[UG];
    float4 vx[4];
    auto load = [&](int c0) {
        const int n = re - c0 < CR ? re - c0 : CR;
#pragma unroll
        for (int u = 0; u < UG; ++u) {
            const int i = tid + NTH * u;
            if constexpr (IMG) {
                const int t = i >> 5;   // 32 16-byte units per 256-column bf16 row
                vg[u] = t < n ? *reinterpret_cast<const uint4*>(static_cast<const __bf16*>(L.dG) +
                                                                (int64_t)(c0 + t) * G + 8 * (i & 31))
                              : make_uint4(0u, 0u, 0u, 0u);
            } else {
                const int t = i >> 6;   // 64 float4 per row
                vg[u] = t < n ? *reinterpret_cast<const float4*>(static_cast<const float*>(L.dG) +
                                                                 (int64_t)(c0 + t) * G + 4 * (i & 63))
                              : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (xv[u] && xt[u] < n) {
                if (!xh[u]) {
                    v = *reinterpret_cast<const float4*>(x + (int64_t)c0 * In + xg[u]);
                } else if (xr[u] != 0) {   // h_{t-1}: the previous row of the same sample
                    v = *reinterpret_cast<const float4*>(h + (int64_t)c0 * 64 + xg[u]);
                }
            }
            vx[u] = v;
            // the step of this item's row in the next chunk
            xr[u] += cs;
            if (xr[u] >= S) xr[u] -= S;
        }
    };
    // registers -> bf16 images (rows past the range are zero in dG: no contribution)
    auto store = [&](__bf16* g, __bf16* xi) {
#pragma unroll
        for (int u = 0; u < UG; ++u) {
            const int i = tid + NTH * u;
            if constexpr (IMG)
                *reinterpret_cast<uint4*>(g + (i >> 5) * DS + 8 * (i & 31)) = vg[u];
            else
                *reinterpret_cast<bf16x4*>(g + (i >> 6) * DS + 4 * (i & 63)) = cvt4(vg[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (xv[u]) *reinterpret_cast<bf16x4*>(xi + xo[u]) = cvt4(vx[u]);
    };
    // four whole 16-row dW tiles per wave: tn = 4 wv .. 4 wv + 3
    f32x4 acc[4][NTK];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < NTK; ++k) acc[a][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nch > 0) {
        load(rb);
        store(gs, xs);
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const int cur = c & 1;
        const __bf16* g = gs + cur * (CR * DS);
        const __bf16* xi = xs + cur * (CR * XSM);
        const bool more = c + 1 < nch;             // workgroup-uniform
        if (more) load(rb + CR * (c + 1));         // in flight during the MFMAs
        bf16x8 af[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) af[a] = tr_frag(g, 16 * (4 * wv + a), DS);
#pragma unroll
        for (int k = 0; k < NTK; ++k) {
            const bf16x8 b = tr_frag(xi, 16 * k, XS);
#pragma unroll
            for (int a = 0; a < 4; ++a)
                acc[a][k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], b, acc[a][k], 0, 0, 0);
        }
        // the other buffer was last read before the previous barrier
        if (more) store(gs + (cur ^ 1) * (CR * DS), xs + (cur ^ 1) * (CR * XSM));
        __syncthreads();
    }
    // D: col (k') = 16 k + (lane & 15), row (dG column) = 16 tn + 4 (lane >> 4) + r
    float* pb = L.part + (int64_t)blockIdx.x * G * K1;
    const int lr = lane & 15, lc = lane >> 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < NTK; ++k) {
            const int kk = 16 * k + lr;
            if (kk >= K1) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * (4 * wv + a) + 4 * lc + r;
                const int n = IMG ? (c & 3) * 64 + (c >> 2) : c;   // image column 4 u + g -> gate row g H + u
                pb[n * K1 + kk] = acc[a][k][r];
            }
        }
}

// layer blockIdx.y, row block blockIdx.x (the same count for every layer: they share R)
__global__ __launch_bounds__(NTH, 2) void k_sk_dw16m(Batch b, int S, int R, int rpb) {
    __shared__ __attribute__((aligned(16))) __bf16 gs[2 * CR * DS];
    __shared__ __attribute__((aligned(16))) __bf16 xs[2 * CR * XSM];
    const Dw16Layer& L = b.l[blockIdx.y];
    const int ntk = (L.In + 64 + 1 + 15) / 16;   // workgroup-uniform
#define VT_DW16(N_)                                          \
    case N_:                                                 \
        if (L.fmt) dw16_body<N_, true>(L, S, R, rpb, gs, xs); \
        else dw16_body<N_, false>(L, S, R, rpb, gs, xs);     \
        break;
    switch (ntk) {
        VT_DW16(5) VT_DW16(6) VT_DW16(7) VT_DW16(8) VT_DW16(9)
    }
#undef VT_DW16
}

// dW_ih[n][k] (+)= sum_b part[b][n][k] (k < In), dW_hh[n][k - In] (k < In + 64), db_ih[n] (and
// db_hh[n], when given) (+)= sum_b part[b][n][In + 64], for layer blockIdx.y.  Fixed order, that
// of mlp.hip's k_sk_sum: 64 outputs per workgroup, wave w sums blocks w, w + 4, w + 8, ... in
// sequence, then (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(256) void k_sk_sum16(Batch b, int blocks) {
    __shared__ float red[4][64];
    const Dw16Layer& L = b.l[blockIdx.y];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int K = L.In, K2 = 64, K1 = K + K2 + 1;
    const int total = G * K1;
    if ((int)blockIdx.x * 64 >= total) return;   // workgroup-uniform (the grid covers the widest layer)
    const int i = (int)blockIdx.x * 64 + lane;
    float a = 0.f;
    if (i < total) {
        const float* p = L.part + i;
        int bl = w;
        for (; bl + 60 < blocks; bl += 64) {
            float v[16];
#pragma unroll
            for (int m = 0; m < 16; ++m) v[m] = p[(int64_t)(bl + 4 * m) * total];
#pragma unroll
            for (int m = 0; m < 16; ++m) a += v[m];
        }
        for (; bl < blocks; bl += 4) a += p[(int64_t)bl * total];
    }
    red[w][lane] = a;
    __syncthreads();
    if (w != 0 || i >= total) return;
    const float t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    const int n = i / K1, k = i - n * K1;
    float* dst = k < K ? L.dW_ih + (int64_t)n * K + k : (k < K + K2 ? L.dW_hh + (int64_t)n * K2 + (k - K) : L.db_ih + n);
    *dst = L.accumulate ? *dst + t : t;
    if (k == K + K2 && L.db_hh) L.db_hh[n] = L.accumulate ? L.db_hh[n] + t : t;
}

}  // namespace

bool sk_lstm16_dw_ok(const void* dG, const float* x, int In, const float* h) {
    return In > 0 && In % 4 == 0 && In <= 64 && !(((uintptr_t)dG | (uintptr_t)x | (uintptr_t)h) & 15);
}

// row blocks of a layer: >= 256 rows each, at most L16DW_BLOCKS (256 instead of 128 workgroups:
// +0.05 ms per step) — a function of R alone
constexpr int L16DW_BLOCKS = 128;
static int64_t dw16_rows_per_block(int64_t R) {
    int64_t blocks = (R + 255) / 256;
    if (blocks > L16DW_BLOCKS) blocks = L16DW_BLOCKS;
    const int64_t rpb = (R + blocks - 1) / blocks;
    return (rpb + CR - 1) / CR * CR;   // whole chunks
}

int64_t sk_lstm16_dw_workspace(int64_t R, int In) {
    const int64_t rpb = dw16_rows_per_block(R);
    return (R + rpb - 1) / rpb * G * (In + 64 + 1);
}

// bf16 LSTM parameter gradients of nl <= 4 layers over the same R rows (see above); every layer
// In % 4 == 0, In <= 64, H = 64, 16-byte aligned operands.  ws: the layers' partial slabs,
// sum of sk_lstm16_dw_workspace(R, In) floats.
int sk_lstm16_dw_multi(int nl, const Dw16Layer* layers, int S, int64_t R, float* ws, int64_t ws_floats,
                       hipStream_t st) {
    if (nl < 1 || nl > SK_DW16_MAX_LAYERS || R < 1 || R >= ((int64_t)1 << 31) || S < 1) return VT_ERR_ARG;
    const int64_t rpb = dw16_rows_per_block(R), blocks = (R + rpb - 1) / rpb;
    Batch b;
    int64_t off = 0;
    int kmax = 0;
    for (int l = 0; l < nl; ++l) {
        b.l[l] = layers[l];
        if (!sk_lstm16_dw_ok(b.l[l].dG, b.l[l].x, b.l[l].In, b.l[l].h)) return VT_ERR_ARG;
        const int K1 = b.l[l].In + 64 + 1;
        b.l[l].part = ws + off;
        off += blocks * G * K1;
        if (K1 > kmax) kmax = K1;
    }
    if (off > ws_floats) return VT_ERR_ARG;
    for (int l = nl; l < SK_DW16_MAX_LAYERS; ++l) b.l[l] = b.l[0];   // never indexed (grid.y = nl)
    hipLaunchKernelGGL(k_sk_dw16m, dim3((unsigned)blocks, (unsigned)nl), dim3(NTH), 0, st, b, S, (int)R, (int)rpb);
    hipLaunchKernelGGL(k_sk_sum16, dim3((unsigned)((G * kmax + 63) / 64), (unsigned)nl), dim3(256), 0, st, b,
                       (int)blocks);
    return VT_OK;
}

int sk_lstm16_dw(const float* dG, const float* x, int In, const float* h, int S, int64_t R, float* dW_ih,
                 float* dW_hh, float* db_ih, float* db_hh, int accumulate, float* ws, int64_t ws_floats,
                 hipStream_t st) {
    Dw16Layer L{};
    L.dG = dG, L.x = x, L.h = h;
    L.dW_ih = dW_ih, L.dW_hh = dW_hh, L.db_ih = db_ih, L.db_hh = db_hh;
    L.In = In, L.fmt = 0, L.accumulate = accumulate;
    return sk_lstm16_dw_multi(1, &L, S, R, ws, ws_floats, st);
}

}  // namespace vt
