// Stand-alone host check of the staged 16-bit hand-off's launch arithmetic (csrc/x16.h): row
// strides, the producer's item count, the forward's LDS size and the weight gradient's prefetch /
// LDS gates over every shape the entry points accept.  No HIP: build with any C++17 compiler,
// e.g.  c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//           -I vae-teb_amd/csrc tools/x16_host_check.cpp -o x16_host_check && ./x16_host_check
// (tests/test_x16_host_cpu.py does that).  Exit status 0 and "ok" when every invariant holds.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "x16.h"

using namespace vt;

#define REQUIRE(cond, ...)                    \
    do {                                      \
        if (!(cond)) {                        \
            fprintf(stderr, "FAILED %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
            exit(1);                          \
        }                                     \
    } while (0)

int main() {
    long checked = 0;
    // strides
    for (int C = 1; C <= 1024; ++C) {
        const int cs = x16_stride(C);
        REQUIRE(cs >= C && cs < C + 8 && cs % 8 == 0, "C %d stride %d", C, cs);
    }
    REQUIRE(!x16_apply_ok(0, 1, 1) && !x16_apply_ok(1, 0, 1) && !x16_apply_ok(1, 1, 0) &&
                !x16_apply_ok(1, 1, X16_CMAX + 1) && !x16_apply_ok(65536, 1, 1) && x16_apply_ok(65535, 1 << 29, X16_CMAX),
            "producer shape gate");
    // the producer's tiles, walked the way k_bn_apply_x16 indexes them (256 threads): the source run
    // stays inside the (L, C) sample rows it owns (+ the float4 alignment slack inside the tensor),
    // every LDS access inside its region, every output row of the sample written exactly once
    for (int up = 0; up <= 1; ++up)
        for (int C : {1, 2, 3, 5, 11, 22, 33, 55, 77, 87, 127, 128})
            for (int L : {1, 2, 8, 31, 32, 33, 37, 64, 65, 70, 300}) {
                const int B = 2, b = 1, NT = 256, cs = x16_stride(C), TR = x16_apply_rows(up), Lx = up ? 2 * L : L;
                const int64_t lds = x16_apply_lds(C, up), total = (int64_t)B * L * C;
                REQUIRE(lds <= 64 * 1024, "producer LDS C %d", C);
                const int64_t img0 = 16 * (int64_t)C, yf0 = img0 + X16_APPLY_OUT * (int64_t)cs * 2;
                std::vector<int> wrote((size_t)Lx, 0);
                for (int m0 = 0; m0 < L; m0 += TR) {
                    const int nrow = L - m0 < TR + up ? L - m0 : TR + up, n = nrow * C;
                    const int64_t f0 = ((int64_t)b * L + m0) * C, fa = f0 & ~(int64_t)3;
                    const int off = (int)(f0 - fa), nv = (off + n + 3) >> 2;
                    std::vector<char> have((size_t)(up ? n : X16_APPLY_OUT * cs), 0);
                    for (int tid = 0; tid < NT; ++tid) {
                        const int e0 = 4 * tid - off + 4 * C;
                        REQUIRE(e0 >= 0, "start index");
                        int r = e0 / C - 4, c = e0 % C;
                        const int rstep = (4 * NT) / C, cstep = (4 * NT) % C;
                        for (int i = tid; i < nv; i += NT) {
                            const int64_t g = fa + 4 * (int64_t)i;
                            REQUIRE(g >= 0 && g < total, "load start");   // the vector load itself is gated on g + 3 < total
                            int rr = r, cc = c;
                            for (int j = 0; j < 4; ++j) {
                                const int e = 4 * i + j - off;
                                if (e >= 0 && e < n) {
                                    REQUIRE(rr == e / C && cc == e % C, "row / channel tracking e %d", e);
                                    REQUIRE(g + j >= f0 && g + j < f0 + n && g + j < total, "element inside its rows");
                                    if (up) {
                                        REQUIRE(yf0 + 4 * (int64_t)(e + 1) <= lds, "y image");
                                        have[(size_t)e]++;
                                    } else {
                                        REQUIRE(rr < 64 && img0 + 2 * (int64_t)(rr * cs + cc + 1) <= yf0, "row image");
                                        have[(size_t)(rr * cs + cc)]++;
                                    }
                                }
                                if (++cc == C) { cc = 0; ++rr; }
                            }
                            r += rstep; c += cstep;
                            if (c >= C) { c -= C; ++r; }
                        }
                    }
                    const int t_lo = up ? (m0 == 0 ? 0 : 2 * m0 + 1) : m0;
                    const int t_end = up ? (2 * (m0 + TR) + 1 < Lx ? 2 * (m0 + TR) + 1 : Lx) : (m0 + TR < L ? m0 + TR : L);
                    const int nt = t_end - t_lo;
                    REQUIRE(nt > 0 && nt <= X16_APPLY_OUT, "output rows of a tile: %d", nt);
                    for (int r = 0; r < nt; ++r) {
                        const int t = t_lo + r;
                        if (up) {   // conv.h up_rows
                            float s = (t + 0.5f) * 0.5f - 0.5f;
                            s = s < 0.f ? 0.f : s;
                            const int i0 = (int)s, i1 = i0 + 1 < L ? i0 + 1 : L - 1;
                            REQUIRE(i0 >= m0 && i1 >= m0 && i0 - m0 < nrow && i1 - m0 < nrow, "source rows of t %d", t);
                            for (int c = 0; c < C; ++c)
                                REQUIRE(have[(size_t)((i0 - m0) * C + c)] == 1 && have[(size_t)((i1 - m0) * C + c)] == 1, "y read");
                        } else {
                            for (int c = 0; c < C; ++c) REQUIRE(have[(size_t)(r * cs + c)] == 1, "row image read");
                        }
                        REQUIRE(t >= 0 && t < Lx, "output row");
                        wrote[(size_t)t]++;
                    }
                }
                for (int t = 0; t < Lx; ++t) REQUIRE(wrote[(size_t)t] == 1, "up %d C %d L %d: row %d written %d times", up, C, L, t, wrote[(size_t)t]);
                ++checked;
            }
    // the LDS window image of the forward, written the way the kernel indexes it: every (row,
    // segment) item lands inside the window region, the taps inside what follows
    for (int K = 1; K <= X16_KMAX; ++K)
        for (int NT = 1; NT <= 6; ++NT)
            for (int nch = 1; nch <= 4; ++nch) {
                const int64_t lds = cfw16_x16_lds(K, NT, nch);
                REQUIRE(lds <= X16_LDS_MAX, "forward LDS K %d NT %d nch %d: %lld", K, NT, nch, (long long)lds);
                const int PM = NT <= 2 ? 4 : 2, TC = 16 * NT, WIN = 64 * PM + K - 1;
                std::vector<char> img((size_t)lds, 0);
                const int64_t xsz = (int64_t)nch * WIN * X16_RS * 2;
                for (int r = 0; r < WIN; ++r)
                    for (int s = 0; s < 4 * nch; ++s) {
                        const int64_t o = ((int64_t)((s >> 2) * WIN + r) * X16_RS + 8 * (s & 3)) * 2;
                        REQUIRE(o + 16 <= xsz, "window item r %d s %d", r, s);
                        for (int j = 0; j < 16; ++j) img[(size_t)(o + j)]++;
                    }
                for (int i = 0; i < K * TC * 4; ++i) {
                    const int oct = i & 3, rr = i >> 2, k = rr / TC, co = rr - k * TC;
                    const int64_t o = xsz + ((int64_t)(k * TC + co) * X16_RS + 8 * oct) * 2;
                    REQUIRE(o + 16 <= lds, "tap item %d", i);
                    for (int j = 0; j < 16; ++j) img[(size_t)(o + j)]++;
                }
                for (size_t i = 0; i < img.size(); ++i) REQUIRE(img[i] <= 1, "LDS byte %zu written twice", i);
                REQUIRE(lds >= 8 * TC * 4, "statistics scratch");
                ++checked;
            }
    // the weight gradient: the per-thread prefetch covers the chunk's window segments, and the
    // stores stay inside the window's LDS rows
    for (int CR : {64, 256})
        for (int K = 1; K <= X16_KMAX; ++K)
            for (int nt : {256, 512})
                for (int Cin = 1; Cin <= 128; ++Cin)
                    for (int Cout : {1, 16, 32, 33, 128}) {
                        const int cin16 = (Cin + 15) / 16 * 16, osegs = cin16 / 8;
                        const int dstride = 16 * ((Cout + 15) / 16) + 8, xstride = cin16 + 8;
                        const int ux = cdw16_x16_ux(CR, K, nt);
                        REQUIRE(cdw16_x16_fits(CR, K, Cin) == (osegs <= cdw16_x16_maxseg(CR)), "fits CR %d Cin %d", CR, Cin);
                        if (CR == 64) REQUIRE(cdw16_x16_fits(CR, K, Cin), "64-row chunks take every Cin <= 128 (%d)", Cin);
                        if (!cdw16_x16_fits(CR, K, Cin)) continue;
                        REQUIRE((int64_t)ux * nt >= (int64_t)(CR + K - 1) * osegs, "prefetch CR %d K %d nt %d Cin %d", CR, K,
                                nt, Cin);
                        const int64_t lds = cdw16_x16_lds(CR, dstride, xstride);
                        const int64_t x0 = (int64_t)CR * dstride * 2;
                        std::vector<char> img((size_t)lds, 0);
                        for (int i = 0; i < (CR + K - 1) * osegs; ++i) {
                            const int t = i / osegs, o = i - t * osegs;
                            const int64_t a = x0 + ((int64_t)t * xstride + 8 * o) * 2;
                            REQUIRE(a + 16 <= lds, "window store t %d o %d", t, o);
                            for (int j = 0; j < 16; ++j) img[(size_t)(a + j)]++;
                        }
                        // the MFMA phase's highest window row: 32 (CR / 32 - 1) + K - 1 + 31
                        REQUIRE(x0 + (int64_t)(CR + K - 1) * xstride * 2 <= lds, "MFMA rows");
                        if (CR == 64 || Cout <= 32) REQUIRE(lds <= X16_LDS_MAX, "LDS CR %d Cin %d Cout %d", CR, Cin, Cout);
                        ++checked;
                    }
    printf("ok (%ld shapes)\n", checked);
    return 0;
}
