// slots_deliver_denoise.hip -- the kernel that delivers a step's PCM through the bias denoiser (slots_deliver_denoise.hpp).  Compiled
// once, both precisions: fp32 throughout, the window's samples become PCM through the table at the staging, the quotients int16 at
// the store.  The two GEMMs and the gain repeat denoise_kernel's (denoise.hip) expression for expression: the pieces of an
// utterance must be its bits.
#include "slots_deliver_denoise.hpp"

#include "resample_core.hpp"
#include "stft_core.hpp"

namespace wn {

namespace {

constexpr int kThreads = 256;                                   // four waves
constexpr int kBinTilesMax = 5, kSampleTilesMax = 8;            // as denoise_kernel holds them
constexpr int kLdsMax = 160 * 1024;

struct Args {
    DenoiseLaunch l;
    int nq, kp;              // J' / 16 and K'
};

// denoise_kernel's spectrum image: [2 K'][16], every block of four rows rotated by 16 (row / 4) words
__device__ __forceinline__ int spec_at(const int block, const int rot, const int fl) { return block * 64 + ((rot & 3) << 4) + fl; }

// PCM of sample i of the piece's stream (counted from its origin), i in [k0 - N, k0 + n): the window from the piece's first sample
// on, the history image below it; anything else, which no frame reads, is zero
__device__ __forceinline__ short stream_at(const DenoiseLaunch& a, const DenoisePiece& pc, const long long i) {
    const long long rel = i - pc.k0;
    if (i < 0 || rel >= pc.n || rel < -(long long)a.nFft) return 0;
    if (rel >= 0) {
        int t = a.T + (int)rel;      // (n <= W: one wrap at the most)
        if (t >= a.W) t -= a.W;
        return a.table[a.y[(size_t)pc.slot * a.W + t]];
    }
    return a.histIn[(size_t)pc.row * a.nFft + a.nFft + rel];
}
// ... of padded position u = i + N / 2, reflected at the origin and, where the stream ends with the piece, at its end
__device__ __forceinline__ short padded_at(const DenoiseLaunch& a, const DenoisePiece& pc, const long long u) {
    long long t = u - (a.nFft >> 1);
    const long long len = pc.k0 + pc.n;
    if (t < 0) t = -t;
    else if ((pc.flags & kDenoiseFin) && t >= len) t = 2 * (len - 1) - t;
    return stream_at(a, pc, t);
}

// the state of an unfinished piece into the other image: the last N samples, zero below the origin
__device__ __forceinline__ void history_out(const DenoiseLaunch& a, const DenoisePiece& pc, const int tid) {
    if (pc.flags & kDenoiseFin) return;
    short* const out = a.histOut + (size_t)pc.row * a.nFft;
    const long long k1 = pc.k0 + pc.n;
    for (int j = tid; j < a.nFft; j += kThreads) out[j] = stream_at(a, pc, k1 - a.nFft + j);
}

// CH: bin tiles a wave holds at a time in the forward GEMM; CI: sample tiles in the inverse one (as denoise_kernel)
template <int CH, int CI>
__global__ __launch_bounds__(kThreads) void slot_deliver_denoise_kernel(const Args args) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const DenoiseLaunch& a = args.l;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, fl = lane & 15;
    const int nFft = a.nFft, hop = a.hop, half = nFft >> 1, over = nFft / hop, accLen = nFft - hop;

    // ---- a piece without a new frame: its state moves on; a stream that ends at N / 2 samples or fewer is delivered as it is ----
    if ((int)blockIdx.x >= a.tiles) {
        const DenoisePiece pc = a.pieces[a.framed + ((int)blockIdx.x - a.tiles)];
        history_out(a, pc, tid);
        if (pc.flags & kDenoiseFin) {
            for (int o = tid; o < pc.count; o += kThreads) a.pcm[pc.offset + o] = stream_at(a, pc, o);
        } else {
            const float* const in = a.accIn + (size_t)pc.row * accLen;
            float* const out = a.accOut + (size_t)pc.row * accLen;
            for (int j = tid; j < accLen; j += kThreads) out[j] = pc.q0 > 0 ? in[j] : 0.f;
        }
        return;
    }

    float* const spec = (float*)lds;
    float* const img = spec + 2 * args.kp * 16;      // [16 pairs][J' + 4]: the staged frames; after the forward GEMM, the synthesised ones
    const int pitch = 16 * args.nq + 4;
    const DenoisePair* const pairs = a.pairs + (size_t)blockIdx.x * 16;

    // ---- the staging: pair c is wave c & 3's, a lane takes every 64th sample of its frame ----
    for (int c = w; c < 16; c += 4) {
        const DenoisePair pr = pairs[c];
        float* const dst = img + c * pitch;
        if (pr.piece < 0) {
            for (int j = lane; j < 16 * args.nq; j += 64) dst[j] = 0.f;
            continue;
        }
        const DenoisePiece pc = a.pieces[pr.piece];
        const long long u0 = (long long)pr.frame * hop;
        for (int j = lane; j < 16 * args.nq; j += 64) dst[j] = j < nFft ? (float)padded_at(a, pc, u0 + j) : 0.f;
    }
    const int myPiece = pairs[fl].piece;
    const float strength = myPiece >= 0 ? a.pieces[myPiece].strength : 0.f;
    __syncthreads();

    // ---- the DFT: bin tile t belongs to wave t & 3; CH of a wave's tiles per pass over the staged frames ----
    {
        const int nbt = args.kp >> 4, nq = args.nq;
        const floatx4* const tab = (const floatx4*)a.fwdTab + lane;
        const float* const bp = img + fl * pitch;
        const float invN = 1.f / (float)nFft;
        for (int first = w; first < nbt; first += 4 * CH) {
            floatx4 re[CH], im[CH];
            size_t at[CH];                                  // (a tile past the last repeats the last, and is not stored)
#pragma unroll
            for (int i = 0; i < CH; i++) {
                re[i] = floatx4{0.f, 0.f, 0.f, 0.f};
                im[i] = floatx4{0.f, 0.f, 0.f, 0.f};
                const int t = first + 4 * i < nbt ? first + 4 * i : nbt - 1;
                at[i] = (size_t)t * 2 * nq * 64;
            }
            for (int q = 0; q < nq; q++) {
                floatx4 ar[CH], ai[CH];
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    ar[i] = tab[at[i] + (size_t)q * 64];
                    ai[i] = tab[at[i] + (size_t)(nq + q) * 64];
                }
                float b[4];
#pragma unroll
                for (int e = 0; e < 4; e++) b[e] = bp[16 * q + 4 * e + g];
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < CH; i++) {
                        re[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[i][e], b[e], re[i], 0, 0, 0);
                        im[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai[i][e], b[e], im[i], 0, 0, 0);
                    }
            }
            // the gain on bins 16 t + 4 g + r, pair fl, and c_k / N; to the spectrum image (a bin past N / 2 has re = im = 0)
#pragma unroll
            for (int i = 0; i < CH; i++) {
                const int t = first + 4 * i;
                if (t >= nbt) continue;
                const floatx4 b4 = *(const floatx4*)(a.bias + 16 * t + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int k = 16 * t + 4 * g + r;
                    const float m = sqrtf(re[i][r] * re[i][r] + im[i][r] * im[i][r]);
                    const float gain = m > 0.f ? fmaxf(1.f - strength * b4[r] / m, 0.f) : 0.f;
                    const float sc = gain * (k == 0 || k == half ? invN : 2.f * invN);
                    spec[spec_at(4 * t + g, r + g, fl)] = re[i][r] * sc;
                    spec[spec_at((args.kp >> 2) + 4 * t + g, r + g, fl)] = im[i][r] * sc;
                }
            }
        }
    }
    __syncthreads();

    // ---- the inverse DFT: sample tile st belongs to wave st & 3; CI of a wave's tiles per pass over the spectrum image ----
    {
        const int nst = args.nq, nk2 = args.kp >> 3;      // 2 K' / 16
        const floatx4* const tab = (const floatx4*)a.invTab + lane;
        int off[4];
#pragma unroll
        for (int e = 0; e < 4; e++) off[e] = spec_at(e, g + e, fl);
        for (int first = w; first < nst; first += 4 * CI) {
            floatx4 acc[CI];
            size_t at[CI];                                  // (a tile past the last repeats the last, and is not stored)
#pragma unroll
            for (int i = 0; i < CI; i++) {
                acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};
                const int st = first + 4 * i < nst ? first + 4 * i : nst - 1;
                at[i] = (size_t)st * nk2 * 64;
            }
            for (int q = 0; q < nk2; q++) {
                floatx4 af[CI];
#pragma unroll
                for (int i = 0; i < CI; i++) af[i] = tab[at[i] + (size_t)q * 64];
                float b[4];
#pragma unroll
                for (int e = 0; e < 4; e++) b[e] = spec[q * 256 + off[e]];      // row 16 q + 4 e + g, pair fl
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < CI; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], b[e], acc[i], 0, 0, 0);
            }
            // samples 16 st + 4 g + (0 .. 3) of pair fl: one 16-byte store
#pragma unroll
            for (int i = 0; i < CI; i++) {
                const int st = first + 4 * i;
                if (st < nst) *(floatx4*)(img + fl * pitch + 16 * st + 4 * g) = acc[i];
            }
        }
    }
    __syncthreads();

    // ---- per piece of the tile: overlap-add onto the carried accumulator, four positions to a thread (hop is a multiple of 4: they
    //      share their covering frames); outputs below the last complete hop, the new accumulator behind it; the new history ----
    int last = 15;
    while (last > 0 && pairs[last].piece < 0) last--;      // (a tile has a pair, and its pairs lie in front)
    for (int p = pairs[0].piece; p <= pairs[last].piece; p++) {
        const DenoisePiece pc = a.pieces[p];
        const bool fin = (pc.flags & kDenoiseFin) != 0;
        const long long q0 = pc.q0, q1 = q0 + pc.nf;
        const long long outEnd = fin ? pc.k0 + pc.n + half : q1 * hop, hi = fin ? outEnd : outEnd + accLen;
        const long long t0 = q0 * hop > half ? q0 * hop - half : 0, carried = q0 > 0 ? q0 * hop + accLen : 0;
        const float* const accIn = a.accIn + (size_t)pc.row * accLen;
        float* const accOut = a.accOut + (size_t)pc.row * accLen;
        const float* const frames = img + pc.col0 * pitch;
        for (long long u = q0 * hop + 4 * tid; u < hi; u += 4 * kThreads) {
            const long long ub = u / hop;
            const long long fe = ub - over + 1 > 0 ? ub - over + 1 : 0;      // the first frame that covers u, and the first new one
            const long long fa = fe > q0 ? fe : q0;
            const long long fb = ub < q1 - 1 ? ub : q1 - 1;
            floatx4 y = floatx4{0.f, 0.f, 0.f, 0.f}, env = y;
            if (u < carried) y += *(const floatx4*)(accIn + (u - q0 * hop));
            for (long long f = fa; f <= fb; f++) y += *(const floatx4*)(frames + (int)(f - q0) * pitch + (int)(u - f * hop));
            if (u >= outEnd) {
                *(floatx4*)(accOut + (u - outEnd)) = y;
                continue;
            }
            for (long long f = fe; f <= fb; f++) env += *(const floatx4*)(a.wnd2 + (int)(u - f * hop));
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const long long o = u + r - half - t0;
                if (o >= 0 && o < pc.count) a.pcm[pc.offset + o] = resample_pcm16(y[r] / env[r]);
            }
        }
        history_out(a, pc, tid);
    }
}

int variant_of(int nFft) {
    const int ch = stft_tiles_per_pass(stft_round16(nFft / 2 + 1) / 16, kBinTilesMax), ci = stft_tiles_per_pass(stft_round16(nFft) / 16, kSampleTilesMax);
    return 3 * (ch <= 1 ? 0 : ch <= 3 ? 1 : 2) + (ci <= 1 ? 0 : ci <= 4 ? 1 : 2);
}

// Calls f.template run<CH, CI>() for the variant of a geometry: 1, 3 or 5 bin tiles, 1, 4 or 8 sample tiles (denoise.hip)
template <class F> bool dispatch(int variant, F&& f) {
    switch (variant) {
        case 0: return f.template run<1, 1>();
        case 1: return f.template run<1, 4>();
        case 2: return f.template run<1, 8>();
        case 3: return f.template run<3, 1>();
        case 4: return f.template run<3, 4>();
        case 5: return f.template run<3, 8>();
        case 6: return f.template run<5, 1>();
        case 7: return f.template run<5, 4>();
        default: return f.template run<5, 8>();
    }
}
struct Prepare {
    template <int CH, int CI> bool run() const {
        if (hipFuncSetAttribute((const void*)slot_deliver_denoise_kernel<CH, CI>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax) == hipSuccess)
            return true;
        (void)hipGetLastError();
        return false;
    }
};
struct Run {
    const Args& a;
    int blocks;
    size_t lds;
    hipStream_t stream;
    template <int CH, int CI> bool run() const {
        hipLaunchKernelGGL((slot_deliver_denoise_kernel<CH, CI>), dim3(blocks), dim3(kThreads), lds, stream, a);
        return hipGetLastError() == hipSuccess;
    }
};

}  // namespace

size_t slots_deliver_denoise_lds(int nFft, int hop) {
    (void)hop;
    return 4 * (32 * (size_t)stft_round16(nFft / 2 + 1) + 16 * ((size_t)stft_round16(nFft) + 4));
}

bool slots_deliver_denoise_prepare(int nFft, int hop) {
    return slots_deliver_denoise_lds(nFft, hop) <= (size_t)kLdsMax && dispatch(variant_of(nFft), Prepare{});
}

bool slots_deliver_denoise(hipStream_t stream, const DenoiseLaunch& l) {
    if (l.count <= 0) return true;
    if (l.framed < 0 || l.framed > l.count || l.tiles < 0 || l.tiles > l.framed || (l.tiles == 0) != (l.framed == 0) || l.pcm == NULL ||
        l.T < 0 || l.T >= l.W)
        return false;
    Args a;
    a.l = l;
    a.nq = stft_round16(l.nFft) / 16;
    a.kp = stft_round16(l.nFft / 2 + 1);
    return dispatch(variant_of(l.nFft), Run{a, l.tiles + (l.count - l.framed), slots_deliver_denoise_lds(l.nFft, l.hop), stream});
}

}  // namespace wn
