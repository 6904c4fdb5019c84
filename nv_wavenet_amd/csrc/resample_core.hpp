// resample_core.hpp -- the GEMM of the polyphase FIR (resample.hpp) behind its staging: shared by resample_kernel
// (resample.hip: requests in device memory) and slot_deliver_rate_kernel (slots_deliver_rate.hip: pieces of a slot step), which
// differ in where a tile's inputs come from and where its outputs go, not in the product.  One order of summation for an output
// whichever kernel computes it: that is what makes a slot session's rate pieces bit for bit nvw_resample of the whole utterance.
#pragma once

#include <hip/hip_runtime.h>

namespace wn {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kResampleWaves = 4, kResampleThreads = 64 * kResampleWaves;
constexpr int kResampleTilesMax = 5;      // row tiles a wave holds at a time (G = 1): five accumulators, five operand fragments in flight

// the table of one ratio as the kernels read it
struct ResampleTab {
    const floatx4* tab;      // [rowTiles][nq][64 lanes]: A fragments of v_mfma_f32_16x16x4_f32
    int Q, hop;
    int j0;
    int nq;                  // W' / 16: operand fragments of a row tile
    int rowTiles;
    int spare;               // s
};

// The product of one tile of `live` <= 16 G blocks whose span is staged in LDS (position l at word l + s (l / hop), the caller has
// synchronised).  G: 16-block groups of a workgroup (4: every wave its own group and all CH = rowTiles row tiles; 1: row tile t
// belongs to wave t & 3, CH of a wave's tiles per pass over the span).  store(col, p, v): output p < Q of block `col` < live of the
// tile has the sum v.
template <int G, int CH, class Store>
__device__ __forceinline__ void resample_tile_gemm(const float* span, const ResampleTab& a, int live, Store store) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, fl = lane & 15;
    const int hop = a.hop, spare = a.spare;
    const int grp = G == 4 ? w : 0;
    if (grp * 16 >= live) return;
    // (a block lane past the last live block reads the last one's inputs, and is not stored)
    const int col = grp * 16 + fl, src = col < live ? col : live - 1;
    const float* const bp = span + src * (hop + spare) + g;
    const floatx4* const tab = a.tab + lane;
    const int nq = a.nq, nrt = a.rowTiles;
    for (int first = G == 4 ? 0 : w; first < nrt; first += (G == 4 ? 1 : 4) * CH) {
        floatx4 acc[CH];
        size_t at[CH];                                  // (a tile past the last repeats the last, and is not stored)
#pragma unroll
        for (int i = 0; i < CH; i++) {
            acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
            const int t = first + (G == 4 ? 1 : 4) * i;
            at[i] = (size_t)(t < nrt ? t : nrt - 1) * nq * 64;
        }
        // input j = 16 qd + 4 e + g of the block lies pad = s (j / hop) words past bp[16 qd + 4 e]: rem = j mod hop, stepped by 4 <= hop
        int rem = g, pad = 0;
        for (int qd = 0; qd < nq; qd++) {
            floatx4 af[CH];
#pragma unroll
            for (int i = 0; i < CH; i++) af[i] = tab[at[i] + (size_t)qd * 64];
            float b[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                b[e] = bp[16 * qd + 4 * e + pad];
                rem += 4;
                const bool wrap = rem >= hop;
                rem -= wrap ? hop : 0;
                pad += wrap ? spare : 0;
            }
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int i = 0; i < CH; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], b[e], acc[i], 0, 0, 0);
        }
        // outputs 16 t + 4 g + r of block `col`
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const int t = first + (G == 4 ? 1 : 4) * i;
            if (t >= nrt || col >= live) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int p = t * 16 + 4 * g + r;
                if (p < a.Q) store(col, p, acc[i][r]);
            }
        }
    }
}

// The same product with the N dimension gathered (slots_deliver_denoise_rate.hpp): block lane fl of the wave is a block of any span
// staged in LDS, its input j at bp[j - g + s (j / hop)] -- bp = that span's block base + g; the caller has synchronised, and hands a
// dead lane a live lane's base.  The k-step order per accumulator is resample_tile_gemm's, so an output has its bits.  G = 4: the
// wave holds all CH = rowTiles row tiles (the caller gives every wave a group of 16 lanes of its own); G = 1: row tile t belongs to
// wave t & 3.  store(p, v): output p < Q of this lane's block has the sum v (live lanes only).
template <int G, int CH, class Store>
__device__ __forceinline__ void resample_gather_gemm(const float* bp, const ResampleTab& a, bool live, Store store) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int hop = a.hop, spare = a.spare;
    const floatx4* const tab = a.tab + lane;
    const int nq = a.nq, nrt = a.rowTiles;
    for (int first = G == 4 ? 0 : w; first < nrt; first += (G == 4 ? 1 : 4) * CH) {
        floatx4 acc[CH];
        size_t at[CH];                                  // (a tile past the last repeats the last, and is not stored)
#pragma unroll
        for (int i = 0; i < CH; i++) {
            acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
            const int t = first + (G == 4 ? 1 : 4) * i;
            at[i] = (size_t)(t < nrt ? t : nrt - 1) * nq * 64;
        }
        int rem = g, pad = 0;
        for (int qd = 0; qd < nq; qd++) {
            floatx4 af[CH];
#pragma unroll
            for (int i = 0; i < CH; i++) af[i] = tab[at[i] + (size_t)qd * 64];
            float b[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                b[e] = bp[16 * qd + 4 * e + pad];
                rem += 4;
                const bool wrap = rem >= hop;
                rem -= wrap ? hop : 0;
                pad += wrap ? spare : 0;
            }
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int i = 0; i < CH; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], b[e], acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const int t = first + (G == 4 ? 1 : 4) * i;
            if (t >= nrt || !live) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int p = t * 16 + 4 * g + r;
                if (p < a.Q) store(p, acc[i][r]);
            }
        }
    }
}

// int16 PCM of a sum: nearest-even, saturated
__device__ __forceinline__ short resample_pcm16(float v) { return (short)(int)fminf(fmaxf(rintf(v), -32768.f), 32767.f); }

// Calls f.template run<G, CH>() for the kernel variant of a ratio: groups = ResampleGeom::groups, ch = Resampler::tilesPerPass()
template <class F> bool resample_dispatch(int groups, int ch, F&& f) {
    if (groups == 4) switch (ch) {
            case 1: return f.template run<4, 1>();
            case 2: return f.template run<4, 2>();
            default: return f.template run<4, 3>();
        }
    switch (ch) {
        case 1: return f.template run<1, 1>();
        case 2: return f.template run<1, 2>();
        case 3: return f.template run<1, 3>();
        case 4: return f.template run<1, 4>();
        default: return f.template run<1, 5>();
    }
}

}  // namespace wn
