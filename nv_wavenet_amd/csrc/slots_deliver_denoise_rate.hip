// slots_deliver_denoise_rate.hip -- the kernel that delivers a step's PCM through the bias denoiser and at the caller's rate
// (slots_deliver_denoise_rate.hpp).  Compiled once, both precisions.  The front half repeats slot_deliver_denoise_kernel
// (slots_deliver_denoise.hip) expression for expression up to the quotient of the overlap-add; the back half is the GEMM of
// resample_core.hpp over blocks gathered across the tile's pieces.
#include "slots_deliver_denoise_rate.hpp"

#include "stft_core.hpp"

namespace wn {

namespace {

constexpr int kThreads = 256;                                   // four waves
constexpr int kBinTilesMax = 5, kSampleTilesMax = 8;            // as denoise_kernel holds them
constexpr int kLdsMax = 160 * 1024;
static_assert(kThreads == kResampleThreads, "resample_gather_gemm splits row tiles over this kernel's waves");

struct Args {
    DenoiseRateLaunch r;
    int nq, kp;              // J' / 16 and K'
    int specWords;           // max(32 K', S): the spectrum image and the spans that overlay it; the frames lie behind
};

// denoise_kernel's spectrum image: [2 K'][16], every block of four rows rotated by 16 (row / 4) words
__device__ __forceinline__ int spec_at(const int block, const int rot, const int fl) { return block * 64 + ((rot & 3) << 4) + fl; }

// PCM of sample i of the piece's stream (slots_deliver_denoise.hip)
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
__device__ __forceinline__ short padded_at(const DenoiseLaunch& a, const DenoisePiece& pc, const long long u) {
    long long t = u - (a.nFft >> 1);
    const long long len = pc.k0 + pc.n;
    if (t < 0) t = -t;
    else if ((pc.flags & kDenoiseFin) && t >= len) t = 2 * (len - 1) - t;
    return stream_at(a, pc, t);
}
__device__ __forceinline__ void history_out(const DenoiseLaunch& a, const DenoisePiece& pc, const int tid) {
    if (pc.flags & kDenoiseFin) return;
    short* const out = a.histOut + (size_t)pc.row * a.nFft;
    const long long k1 = pc.k0 + pc.n;
    for (int j = tid; j < a.nFft; j += kThreads) out[j] = stream_at(a, pc, k1 - a.nFft + j);
}

// Keeps a uniform value in vector registers.  The scalar file is full in the overlap-add: slot_deliver_denoise_kernel alone takes 96
// of its 102 registers there, so what this kernel adds to that loop lives in the vector file, which has room
template <class T> __device__ __forceinline__ T in_vgpr(T x) {
    asm volatile("" : "+v"(x));
    return x;
}

// z[t0 + rel] of the carried tail, rel in [-H, 0): zero below the origin and where the tail counts as zero
__device__ __forceinline__ short tail_at(const DenoiseRateLaunch& a, const DenoisePiece& pc, const long long t0, const long long rel) {
    if ((pc.flags & kDenoiseRateZeroTail) || t0 + rel < 0) return 0;
    return a.tailIn[(size_t)pc.row * a.H + a.H + rel];
}
// positions of a span of `blocks` blocks
__device__ __forceinline__ int span_len(const ResampleTab& t, const int blocks) { return blocks > 0 ? (blocks - 1) * t.hop + 16 * t.nq : 0; }

// The rate GEMM over pairs [begin, begin + n) of the launch, whose spans are staged (the caller has synchronised): groups of 16
// pairs, one per wave at a time with G = 4, one for all four waves with G = 1
template <int G, int RC>
__device__ __forceinline__ void rate_groups(const DenoiseRateLaunch& a, const float* span, const int begin, const int n) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, fl = lane & 15;
    for (int grp = G == 4 ? w : 0; grp * 16 < n; grp += G == 4 ? 4 : 1) {
        const int j = grp * 16 + fl;
        const bool live = j < n;
        const RatePair pr = a.ratePairs[begin + (live ? j : n - 1)];
        const DenoiseRatePiece* const pc = a.pieces + pr.piece;
        const float* const bp = span + pc->span + pr.block * (a.t.hop + a.t.spare) + g;
        const long long o0 = (pc->block0 + pr.block) * a.t.Q - pc->m0;
        const int count = pc->count;
        short* const out = a.l.pcm + pc->d.offset;
        resample_gather_gemm<G, RC>(bp, a.t, live, [&](int p, float v) {
            const long long o = o0 + p;
            if (o >= 0 && o < count) out[o] = resample_pcm16(v);
        });
    }
}

// CH: bin tiles a wave holds at a time in the forward GEMM; CI: sample tiles in the inverse one (as denoise_kernel); G, RC: as
// resample_tile_gemm's G and CH
template <int CH, int CI, int G, int RC>
__global__ __launch_bounds__(kThreads) void slot_deliver_denoise_rate_kernel(const Args args) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    // (the front half reads its arguments as slot_deliver_denoise_kernel does; the back half reads its own from the kernel-argument
    // segment where it uses them, so that they do not occupy scalar registers from the entry on)
    const DenoiseRateLaunch& ar = ((const Args*)__builtin_amdgcn_kernarg_segment_ptr())->r;
    const DenoiseLaunch& a = args.r.l;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, fl = lane & 15;
    const int nFft = a.nFft, hop = a.hop, half = nFft >> 1, over = nFft / hop, accLen = nFft - hop;
    float* const spec = (float*)lds;
    float* const span = spec;      // (from the barrier behind the inverse GEMM on)

    // ---- a piece without a new frame: its three states move on; a stream that ends at N / 2 samples or fewer is converted as it is ----
    if ((int)blockIdx.x >= a.tiles) {
        const DenoiseRatePiece rp = ar.pieces[a.framed + ((int)blockIdx.x - a.tiles)];
        const DenoisePiece& pc = rp.d;
        const int hopR = ar.t.hop, spare = ar.t.spare, H = ar.H;
        history_out(a, pc, tid);
        if (pc.flags & kDenoiseFin) {
            const long long i0 = rp.block0 * hopR + ar.t.j0;
            const int spanN = span_len(ar.t, rp.blocks);
            for (int l = tid; l < spanN; l += kThreads) {
                const long long i = i0 + l;
                span[rp.span + l + spare * (l / hopR)] = i >= 0 && i < pc.count ? (float)stream_at(a, pc, i) : 0.f;
            }
            __syncthreads();      // (the whole workgroup takes this branch)
            rate_groups<G, RC>(ar, span, rp.pair0, rp.blocks);
        } else {
            const float* const in = a.accIn + (size_t)pc.row * accLen;
            float* const out = a.accOut + (size_t)pc.row * accLen;
            for (int j = tid; j < accLen; j += kThreads) out[j] = pc.q0 > 0 ? in[j] : 0.f;
            const long long t0 = (long long)pc.q0 * hop > half ? (long long)pc.q0 * hop - half : 0;
            short* const tout = ar.tailOut + (size_t)pc.row * H;
            for (int j = tid; j < H; j += kThreads) tout[j] = tail_at(ar, pc, t0, j - H);
        }
        return;
    }

    float* const img = spec + args.specWords;        // [16 pairs][J' + 4]: the staged frames; after the forward GEMM, the synthesised ones
    const int pitch = 16 * args.nq + 4;
    const DenoisePair* const pairs = args.r.pairs + (size_t)blockIdx.x * 16;

    // ---- the staging: pair c is wave c & 3's, a lane takes every 64th sample of its frame ----
    for (int c = w; c < 16; c += 4) {
        const DenoisePair pr = pairs[c];
        float* const dst = img + c * pitch;
        if (pr.piece < 0) {
            for (int j = lane; j < 16 * args.nq; j += 64) dst[j] = 0.f;
            continue;
        }
        const DenoisePiece pc = args.r.pieces[pr.piece].d;
        const long long u0 = (long long)pr.frame * hop;
        for (int j = lane; j < 16 * args.nq; j += 64) dst[j] = j < nFft ? (float)padded_at(a, pc, u0 + j) : 0.f;
    }
    const int myPiece = pairs[fl].piece;
    const float strength = myPiece >= 0 ? args.r.pieces[myPiece].d.strength : 0.f;
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
                floatx4 ar4[CH], ai[CH];
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    ar4[i] = tab[at[i] + (size_t)q * 64];
                    ai[i] = tab[at[i] + (size_t)(nq + q) * 64];
                }
                float b[4];
#pragma unroll
                for (int e = 0; e < 4; e++) b[e] = bp[16 * q + 4 * e + g];
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < CH; i++) {
                        re[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar4[i][e], b[e], re[i], 0, 0, 0);
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
    __syncthreads();      // (the spectrum image is dead: the spans take its place)

    // ---- per piece of the tile: its span outside the new samples (carried tail, zeros); the overlap-add of §6s, its quotients
    //      rounded into the span and, the last H of an unfinished stream, into the new tail; the new accumulator and history ----
    int last = 15;
    while (last > 0 && pairs[last].piece < 0) last--;      // (a tile has a pair, and its pairs lie in front)
    const int pFirst = pairs[0].piece, pLast = pairs[last].piece;
    for (int p = pFirst; p <= pLast; p++) {
        const DenoisePiece pc = args.r.pieces[p].d;
        const bool fin = (pc.flags & kDenoiseFin) != 0;
        const long long q0 = pc.q0, q1 = q0 + pc.nf;
        const long long outEnd = fin ? pc.k0 + pc.n + half : q1 * hop, hi = fin ? outEnd : outEnd + accLen;
        const long long t0 = q0 * hop > half ? q0 * hop - half : 0, carried = q0 > 0 ? q0 * hop + accLen : 0;
        const float* const accIn = a.accIn + (size_t)pc.row * accLen;
        float* const accOut = a.accOut + (size_t)pc.row * accLen;
        const float* const frames = img + pc.col0 * pitch;
        // (what the back half adds, in vector registers: the span's first word and length, the span position of z[t0], the spare-word
        // layout, the tail index of z[t0] and the new tail)
        const DenoiseRatePiece& rp = ar.pieces[p];
        const int hopR = in_vgpr(ar.t.hop), spare = in_vgpr(ar.t.spare), H = ar.H;
        float* const sp = in_vgpr(span + rp.span);
        short* const tout = in_vgpr(ar.tailOut + (size_t)pc.row * H);
        const int spanN = in_vgpr(span_len(ar.t, rp.blocks));
        const int at0 = in_vgpr((int)(t0 - (rp.block0 * ar.t.hop + ar.t.j0))), keep = in_vgpr(H - pc.count);
        for (int l = tid; l < spanN; l += kThreads) {
            const int rel = l - at0;
            if (rel >= 0 && rel < pc.count) continue;      // (the overlap-add's)
            sp[l + spare * (l / hopR)] = rel < 0 && rel >= -H ? (float)tail_at(ar, pc, t0, rel) : 0.f;
        }
        if (!fin)      // (the part of the new tail that the old one still holds)
            for (int j = tid; j < keep; j += kThreads) tout[j] = tail_at(ar, pc, t0, j - keep);
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
                if (o < 0 || o >= pc.count) continue;
                const short z = resample_pcm16(y[r] / env[r]);
                const int l = at0 + (int)o;
                if (l >= 0 && l < spanN) sp[l + spare * (l / hopR)] = (float)z;
                if (!fin && keep + (int)o >= 0) tout[keep + (int)o] = z;
            }
        }
        history_out(a, pc, tid);
    }
    __syncthreads();

    // ---- the rate GEMM over the blocks of the tile's pieces, sixteen to a group whichever piece they belong to ----
    const int begin = ar.pieces[pFirst].pair0;
    rate_groups<G, RC>(ar, span, begin, ar.pieces[pLast].pair0 + ar.pieces[pLast].blocks - begin);
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
// ... and inside it f.template run<G, RC>() of resample_dispatch
template <int CH, int CI> struct PrepareRate {
    template <int G, int RC> bool run() const {
        if (hipFuncSetAttribute((const void*)slot_deliver_denoise_rate_kernel<CH, CI, G, RC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                kLdsMax) == hipSuccess)
            return true;
        (void)hipGetLastError();
        return false;
    }
};
struct Prepare {
    int groups, ch;
    template <int CH, int CI> bool run() const { return resample_dispatch(groups, ch, PrepareRate<CH, CI>{}); }
};
template <int CH, int CI> struct RunRate {
    const Args& a;
    int blocks;
    size_t lds;
    hipStream_t stream;
    template <int G, int RC> bool run() const {
        hipLaunchKernelGGL((slot_deliver_denoise_rate_kernel<CH, CI, G, RC>), dim3(blocks), dim3(kThreads), lds, stream, a);
        return hipGetLastError() == hipSuccess;
    }
};
struct Run {
    const Args& a;
    int blocks;
    size_t lds;
    hipStream_t stream;
    int groups, ch;
    template <int CH, int CI> bool run() const { return resample_dispatch(groups, ch, RunRate<CH, CI>{a, blocks, lds, stream}); }
};

long long spec_words(int nFft, long long spanWords) {
    const long long image = 32 * (long long)stft_round16(nFft / 2 + 1);
    return image > spanWords ? image : (spanWords + 3) / 4 * 4;      // (the frames behind stay 16-byte aligned)
}

}  // namespace

long long slots_deliver_denoise_rate_span_words(const DenoiseRateGeom& g) {
    const int half = g.nFft / 2;
    const long long Z = 16LL * g.hop + (16 / (half / g.hop)) * (long long)half;
    const long long B = Z / g.hopR + 1 + 16 * ((long long)(g.centre + g.down) / ((long long)g.down * g.Q) + 3);
    return B * (g.hopR + g.spare) + 16 * (g.wp + (long long)g.spare * ((g.wp - 1) / g.hopR));
}

size_t slots_deliver_denoise_rate_lds(int nFft, long long spanWords) {
    return 4 * ((size_t)spec_words(nFft, spanWords) + 16 * ((size_t)stft_round16(nFft) + 4));
}

bool slots_deliver_denoise_rate_prepare(int nFft, long long spanWords, int groups, int ch) {
    return slots_deliver_denoise_rate_lds(nFft, spanWords) <= (size_t)kLdsMax && dispatch(variant_of(nFft), Prepare{groups, ch});
}

bool slots_deliver_denoise_rate(hipStream_t stream, const DenoiseRateLaunch& r, long long spanWords, int groups, int ch) {
    const DenoiseLaunch& l = r.l;
    if (l.count <= 0) return true;
    if (l.framed < 0 || l.framed > l.count || l.tiles < 0 || l.tiles > l.framed || (l.tiles == 0) != (l.framed == 0) || l.pcm == NULL ||
        l.T < 0 || l.T >= l.W || r.H < 0 || slots_deliver_denoise_rate_lds(l.nFft, spanWords) > (size_t)kLdsMax)
        return false;
    Args a;
    a.r = r;
    a.nq = stft_round16(l.nFft) / 16;
    a.kp = stft_round16(l.nFft / 2 + 1);
    a.specWords = (int)spec_words(l.nFft, spanWords);
    return dispatch(variant_of(l.nFft), Run{a, l.tiles + (l.count - l.framed), slots_deliver_denoise_rate_lds(l.nFft, spanWords), stream, groups, ch});
}

}  // namespace wn
