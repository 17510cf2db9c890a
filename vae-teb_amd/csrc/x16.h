// Host-side shape arithmetic of the staged 16-bit hand-off between conv blocks (conv.h x16_geo):
// row strides, item counts, LDS sizes and the shape gates of the kernels' X16 forms.  Plain
// integer functions without HIP types, so a stand-alone host program can check them under a
// sanitizer (tools/x16_host_check.cpp); the constexpr ones also size the kernels' registers.
#pragma once
#include <stdint.h>

namespace vt {

constexpr int X16_LDS_MAX = 160 * 1024;
constexpr int X16_RS = 40;          // conv_fwd16.hip RS: 16-bit row stride of window / tap rows
constexpr int X16_KMAX = 11;        // KMAXB

// channel stride of the staged rows
constexpr int x16_stride(int C) { return (C + 7) & ~7; }

// the producer (k_bn_apply_x16): a workgroup owns 64 output rows of one sample — 64 source rows,
// or 32 (+ one halo row) when the consumer upsamples; LDS: the per-channel parameters [C] float4,
// the 16-bit row image [65][stride] (upsampling, a sample's first tile also owns up-row 0) and,
// upsampling, y of the 33 source rows in fp32
constexpr int X16_CMAX = 128;
constexpr int X16_APPLY_OUT = 65;
constexpr int x16_apply_rows(int up) { return up ? 32 : 64; }
constexpr int64_t x16_apply_lds(int C, int up) {
    return 16 * (int64_t)C + X16_APPLY_OUT * (int64_t)x16_stride(C) * 2 + (up ? (int64_t)(x16_apply_rows(1) + 1) * C * 4 : 0);
}
// shapes it takes: samples along grid.y, up-domain row indices in int
constexpr bool x16_apply_ok(int B, int L, int C) {
    return B > 0 && B <= 65535 && L > 0 && L <= (1 << 29) && C > 0 && C <= X16_CMAX;
}

// forward (k_cfw16 X16): the 16-bit window of every 32-channel chunk, then the taps of one chunk;
// at least the BatchNorm statistics' two [4][TC] float reductions.  NT: 16-channel output tiles.
constexpr int64_t cfw16_x16_lds(int K, int NT, int nch) {
    const int PM = NT <= 2 ? 4 : 2, TC = 16 * NT, WIN = 64 * PM + K - 1;
    const int64_t lds = (int64_t)nch * WIN * X16_RS * 2 + (int64_t)K * TC * X16_RS * 2;
    return lds < 8 * TC * 4 ? 8 * TC * 4 : lds;
}

// weight gradient (k_cdw16 X16): window segments of 8 channels a thread prefetches per chunk of CR
// rows — sized for 128 input channels at 64-row chunks, 48 at 256-row chunks (nt threads)
constexpr int cdw16_x16_maxseg(int CR) { return CR == 64 ? 16 : 6; }
constexpr int cdw16_x16_ux(int CR, int K, int nt) { return ((CR + K - 1) * cdw16_x16_maxseg(CR) + nt - 1) / nt; }
// the chunk's window segments fit that prefetch
constexpr bool cdw16_x16_fits(int CR, int K, int Cin) { return (Cin + 15) / 16 * 2 <= cdw16_x16_maxseg(CR); }
// LDS: dY rows [CR][dstride] and the window [CR + KMAX + 8][xstride], 16-bit
constexpr int64_t cdw16_x16_lds(int CR, int dstride, int xstride) {
    return ((int64_t)CR * dstride + (int64_t)(CR + X16_KMAX + 8) * xstride) * 2;
}

}  // namespace vt
