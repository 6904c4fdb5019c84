// stft_core.hpp -- what the two STFT kernels share: the layout of a tile's span of samples in LDS and the float64 builder of the
// windowed DFT table that their forward GEMM multiplies it by.  analysis_kernel (analysis.hip) ends that product in
// magnitudes and a mel projection, denoise_kernel (denoise.hip, §6r) in a gain and the inverse transform.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

namespace wn {

typedef float floatx4 __attribute__((ext_vector_type(4)));

inline int stft_round16(int v) { return 16 * ((v + 15) / 16); }

// where local position l of a tile's span lies in LDS: four spare words per hop (analysis.hpp, "frames")
__device__ __forceinline__ unsigned span_at(const unsigned l, const unsigned hop) { return l + 4 * (l / hop); }

// words of LDS of a span of 15 hop + J' positions
inline size_t stft_span_words(int nFft, int hop) {
    const size_t span = 15 * (size_t)hop + stft_round16(nFft);
    return span + 4 * (span / hop + 1);
}

// a wave's tiles (of `tiles` over four waves) in the fewest passes of at most `most` at a time, and evenly over those
inline int stft_tiles_per_pass(int tiles, int most) {
    const int perWave = (tiles + 3) / 4, passes = (perWave + most - 1) / most;
    return (perWave + passes - 1) / passes;
}

// the periodic Hann window and one turn of cos / sin, in float64
struct StftBasis {
    std::vector<double> wnd, c, s;
    explicit StftBasis(int nFft) : wnd(nFft), c(nFft), s(nFft) {
        const double kPi = 3.14159265358979323846;
        for (int j = 0; j < nFft; j++) {
            c[j] = cos(2 * kPi * j / nFft);
            s[j] = sin(2 * kPi * j / nFft);
            wnd[j] = 0.5 - 0.5 * c[j];
        }
    }
};

// The windowed basis w[j] cos / -w[j] sin of bins k = 0 .. nFft / 2, float64 rounded to fp32 with the angle from k j mod nFft, so that
// its argument stays exact.  A fragments [K' / 16][re, im][J' / 16][64 lanes] x 4: lane (row lane & 15, k-step column lane >> 4),
// element e = k-step 4 q + e, i.e. sample 16 q + 4 e + (lane >> 4); zero rows and columns past the bins and the samples.
inline std::vector<float> stft_forward_table(int nFft, const StftBasis& b) {
    const int bins = nFft / 2 + 1, nk = stft_round16(bins) / 16, nq = stft_round16(nFft) / 16;
    std::vector<float> dft((size_t)nk * 2 * nq * 256, 0.f);
    for (int t = 0; t < nk; t++)
        for (int q = 0; q < nq; q++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 4; e++) {
                    const int k = t * 16 + (lane & 15), j = 16 * q + 4 * e + (lane >> 4);
                    if (k >= bins || j >= nFft) continue;
                    const int ph = (int)(((long long)k * j) % nFft);
                    dft[(((size_t)t * 2 * nq + q) * 64 + lane) * 4 + e] = (float)(b.wnd[j] * b.c[ph]);
                    dft[(((size_t)t * 2 * nq + nq + q) * 64 + lane) * 4 + e] = (float)(-b.wnd[j] * b.s[ph]);
                }
    return dft;
}

}  // namespace wn
