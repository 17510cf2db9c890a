// Skinny fp32-MFMA linear kernels (mlp.hip), dispatched from the vt_linear_*
// entry points of gemm.hip for widths <= 256.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vt {

constexpr int SK_MAX_N = 256;   // output columns of k_sk_gemm (16 tiles)
constexpr int SK_MAX_K1 = 144;  // K (+1 bias column) of k_sk_dw (9 tiles)

int sk_linear_fwd(const float* X, int64_t R, int K, const float* W, int N, const float* bias, float* Y,
                  hipStream_t st);
int sk_linear_ln_fwd(const float* X, int64_t R, int K, const float* W, int N, const float* bias, const float* g,
                     const float* beta, int act, float eps, float* Y, float* XH, float* RS, hipStream_t st);
int sk_linear_bwd_data(const float* dY, int64_t R, int N, const float* W, int K, float* dX, int accumulate,
                       hipStream_t st);
int64_t sk_dw_blocks(int64_t R);
int64_t sk_dw_workspace(int64_t R, int N, int K);
int sk_linear_bwd_weight(const float* dY, int64_t R, int N, const float* X, int K, float* dW, float* db,
                         int accumulate, float* ws, int64_t ws_floats, hipStream_t st);
// dW (+)= dY^T X, dW2 (+)= dY^T X2, db (and db2) (+)= column sums of dY, in one pass over dY
int sk_linear_bwd_weight2(const float* dY, int64_t R, int N, const float* X, int K, const float* X2, int K2,
                          float* dW, float* dW2, float* db, float* db2, int accumulate, float* ws, int64_t ws_floats,
                          hipStream_t st, int x2_shift = 0);
// skdw16.hip: the 16-bit LSTM's parameter gradients on bf16 MFMA (dG, x, h_{t-1} rounded to bf16,
// fp32 accumulation).  One layer of a batched call: dG is fp32 [R][4H] by gate row (fmt 0) or the
// recurrences' bf16 image [R][4H] with columns 4 u + g (fmt 1); x [R][In], h [R][64] (read one row
// back within each sample); outputs as sk_linear_bwd_weight2's.  part is set by the launcher.
constexpr int SK_DW16_MAX_LAYERS = 4;
struct Dw16Layer {
    const void* dG;
    const float* x;
    const float* h;
    float* dW_ih;
    float* dW_hh;
    float* db_ih;
    float* db_hh;   // may be null
    float* part;
    int In, fmt, accumulate;
};
// shape / alignment the bf16 kernel takes: In % 4 == 0, In <= 64, 16-byte aligned operands
bool sk_lstm16_dw_ok(const void* dG, const float* x, int In, const float* h);
// partial-slab floats of one layer of R rows
int64_t sk_lstm16_dw_workspace(int64_t R, int In);
// nl <= 4 layers over the same R rows of S-step samples in one launch (+ one for the fixed-order
// sum); VT_ERR_ARG when a layer is not sk_lstm16_dw_ok or ws is too small
int sk_lstm16_dw_multi(int nl, const Dw16Layer* layers, int S, int64_t R, float* ws, int64_t ws_floats,
                       hipStream_t st);
// one fp32-dG layer through the same kernel (the same row partition and summation order)
int sk_lstm16_dw(const float* dG, const float* x, int In, const float* h, int S, int64_t R, float* dW_ih,
                 float* dW_hh, float* db_ih, float* db_hh, int accumulate, float* ws, int64_t ws_floats,
                 hipStream_t st);

}  // namespace vt
