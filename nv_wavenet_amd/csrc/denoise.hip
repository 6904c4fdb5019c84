// denoise.hip -- the kernel and the host side of wn::Denoiser (denoise.hpp).  Compiled once: fp32 throughout, the requests' sample
// types are a conversion at the staging and at the store.
#include "denoise.hpp"

#include "resample_core.hpp"
#include "stft_core.hpp"

#include <limits.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace wn {

namespace {

constexpr int kDenoiseWaves = 4, kDenoiseThreads = 64 * kDenoiseWaves;
constexpr int kDenoiseBinTilesMax = 5;        // bin tiles a wave holds at a time (forward): ten accumulators, ten operand fragments
constexpr int kDenoiseSampleTilesMax = 8;     // sample tiles a wave holds at a time (inverse): eight of each

struct DenoiseArgs {
    const DenoiseJob* jobs;
    int count;
    const floatx4* fwdTab;
    const floatx4* invTab;
    const float* bias;
    const float* wnd2;
    int nFft, hop;
    int nq;                  // J' / 16: operand fragments of a bin tile's real (or imaginary) part, and the sample tiles of a frame
    int kp;                  // K'
};

// where bin row `row` (real rows, then K' imaginary ones), frame fl, lies in the spectrum image: [2 K'][16] with every block of four
// rows rotated by 16 (row / 4) words, so that the accumulators' rows 4 g + r (g over lanes) and the B operand's rows 4 e + g both
// spread over the 64 banks
__device__ __forceinline__ int spec_at(const int block, const int rot, const int fl) { return block * 64 + ((rot & 3) << 4) + fl; }

// CH: bin tiles a wave holds at a time in the forward GEMM; CI: sample tiles in the inverse one.  The host picks them from the geometry.
template <int CH, int CI>
__global__ __launch_bounds__(kDenoiseThreads) void denoise_kernel(const DenoiseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* const spec = (float*)lds;
    float* const span = spec + 2 * a.kp * 16;      // the tile's samples; after the forward GEMM, its synthesised frames
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, fl = lane & 15;
    const int nFft = a.nFft, hop = a.hop, half = nFft >> 1, over = nFft / hop;

    // this workgroup's request by bisection of the first tiles, and its tile of the request's stream
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.jobs[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const DenoiseJob jb = a.jobs[lo];
    const long long ti = (long long)jb.tileBase + ((int)blockIdx.x - jb.tile0);
    const long long f0 = ti * (17 - over);

    // ---- the span: padded positions u0 + l; position u is sample u - N / 2, reflected at 0 and, where the stream ends, at its end ----
    {
        const int span_n = 15 * hop + 16 * a.nq;
        const long long u0 = f0 * hop, n = jb.frames == INT_MAX ? LLONG_MAX : jb.first + jb.nIn;
        for (int l = tid; l < span_n; l += kDenoiseThreads) {
            long long t = u0 + l - half;
            if (t < 0) t = -t;
            else if (t >= n) t = 2 * (n - 1) - t;
            const long long rel = t - jb.first;
            float v = 0.f;
            if (rel >= 0 && rel < jb.nIn) v = jb.inType == 16 ? (float)((const short*)jb.in)[rel] : ((const float*)jb.in)[rel];
            span[span_at(l, hop)] = v;
        }
    }
    __syncthreads();

    // ---- the DFT (as analysis_kernel): bin tile t belongs to wave t & 3; CH of a wave's tiles per pass over the span ----
    {
        const int nbt = a.kp >> 4, nq = a.nq;
        const floatx4* const tab = a.fwdTab + lane;
        const float* const bp = span + fl * (hop + 4);
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
                for (int e = 0; e < 4; e++) b[e] = bp[span_at(16 * q + 4 * e + g, hop)];
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < CH; i++) {
                        re[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[i][e], b[e], re[i], 0, 0, 0);
                        im[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai[i][e], b[e], im[i], 0, 0, 0);
                    }
            }
            // the gain on bins 16 t + 4 g + r, frame fl, and c_k / N; to the spectrum image (a bin past N / 2 has re = im = 0)
#pragma unroll
            for (int i = 0; i < CH; i++) {
                const int t = first + 4 * i;
                if (t >= nbt) continue;
                const floatx4 b4 = *(const floatx4*)(a.bias + 16 * t + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int k = 16 * t + 4 * g + r;
                    const float m = sqrtf(re[i][r] * re[i][r] + im[i][r] * im[i][r]);
                    const float gain = m > 0.f ? fmaxf(1.f - jb.strength * b4[r] / m, 0.f) : 0.f;
                    const float sc = gain * (k == 0 || k == half ? invN : 2.f * invN);
                    spec[spec_at(4 * t + g, r + g, fl)] = re[i][r] * sc;
                    spec[spec_at((a.kp >> 2) + 4 * t + g, r + g, fl)] = im[i][r] * sc;
                }
            }
        }
    }
    __syncthreads();

    // ---- the inverse DFT: sample tile st belongs to wave st & 3; CI of a wave's tiles per pass over the spectrum image ----
    float* const img = span;                    // [16 frames][J' + 4]
    const int pitch = 16 * a.nq + 4;
    {
        const int nst = a.nq, nk2 = a.kp >> 3;      // 2 K' / 16
        const floatx4* const tab = a.invTab + lane;
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
                for (int e = 0; e < 4; e++) b[e] = spec[q * 256 + off[e]];      // row 16 q + 4 e + g, frame fl
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < CI; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], b[e], acc[i], 0, 0, 0);
            }
            // samples 16 st + 4 g + (0 .. 3) of frame f0 + fl: one 16-byte store
#pragma unroll
            for (int i = 0; i < CI; i++) {
                const int st = first + 4 * i;
                if (st < nst) *(floatx4*)(img + fl * pitch + 16 * st + 4 * g) = acc[i];
            }
        }
    }
    __syncthreads();

    // ---- overlap-add of the owned positions, four to a thread (hop is a multiple of 4: they share their covering frames) ----
    const long long uLo = ti == 0 ? half : (f0 + over - 1) * hop, uHi = (f0 + 16) * hop;
    for (long long u = (uLo & ~3LL) + 4 * tid; u < uHi; u += 4 * kDenoiseThreads) {
        const long long ub = u / hop;
        const long long fa = ub - over + 1 > f0 ? ub - over + 1 : f0;      // (below f0 only in tile 0: no frame before the first)
        const long long fb = ub < jb.frames - 1 ? ub : jb.frames - 1;
        floatx4 y = floatx4{0.f, 0.f, 0.f, 0.f}, env = y;
        for (long long f = fa; f <= fb; f++) {
            const int j = (int)(u - f * hop);
            y += *(const floatx4*)(img + (int)(f - f0) * pitch + j);
            env += *(const floatx4*)(a.wnd2 + j);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const long long o = u + r - half - jb.t0;
            if (o < 0 || o >= jb.count) continue;
            const float v = y[r] / env[r];
            if (jb.outType == 16) ((short*)jb.out)[o] = resample_pcm16(v);
            else ((float*)jb.out)[o] = v;
        }
    }
}

template <int CH, int CI>
bool launchDenoise(const DenoiseArgs& a, int tiles, size_t lds, hipStream_t stream, bool optIn) {
    if (optIn && hipFuncSetAttribute((const void*)denoise_kernel<CH, CI>, hipFuncAttributeMaxDynamicSharedMemorySize, kDenoiseLdsMax) != hipSuccess)
        return false;
    hipLaunchKernelGGL((denoise_kernel<CH, CI>), dim3(tiles), dim3(kDenoiseThreads), lds, stream, a);
    return hipGetLastError() == hipSuccess;
}

template <int CH>
bool launchDenoise(int ci, const DenoiseArgs& a, int tiles, size_t lds, hipStream_t stream, bool optIn) {
    switch (ci) {
        case 0: return launchDenoise<CH, 1>(a, tiles, lds, stream, optIn);
        case 1: return launchDenoise<CH, 4>(a, tiles, lds, stream, optIn);
        default: return launchDenoise<CH, 8>(a, tiles, lds, stream, optIn);
    }
}

template <typename T>
bool upload(T*& dst, const std::vector<T>& src) {
    dst = NULL;
    if (hipMalloc((void**)&dst, src.size() * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    gpuErrChk(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return true;
}

}  // namespace

size_t Denoiser::ldsBytes(int nFft, int hop) {
    const size_t jp = stft_round16(nFft), kp = stft_round16(nFft / 2 + 1), span = stft_span_words(nFft, hop), img = 16 * (jp + 4);
    return 4 * (32 * kp + (span > img ? span : img));
}

void Denoiser::clear() {
    for (float* p : {m_fwdTab, m_invTab, m_bias, m_wnd2})
        if (p) gpuErrChk(hipFree(p));
    if (m_jobs) gpuErrChk(hipFree(m_jobs));
    m_fwdTab = m_invTab = m_bias = m_wnd2 = NULL;
    m_jobs = NULL;
    m_jobCap = 0;
    m_nFft = 0;
}

bool Denoiser::set(int nFft, int hop, const float* bias) {
    if (nFft < kDenoiseFftMin || nFft > kDenoiseFftMax || (nFft & 3) != 0 || hop < 4 || (hop & 3) != 0 || nFft % hop != 0 ||
        nFft / hop < kDenoiseOverlapMin || nFft / hop > kDenoiseOverlapMax || bias == NULL || is_device_ptr(bias) ||
        ldsBytes(nFft, hop) > (size_t)kDenoiseLdsMax)
        return false;
    const int bins = nFft / 2 + 1, kp = stft_round16(bins), jp = stft_round16(nFft), nst = jp / 16, nk2 = 2 * kp / 16;
    std::vector<float> b(kp, 0.f), w2(jp, 0.f);
    for (int k = 0; k < bins; k++) {
        if (!(bias[k] >= 0.f) || !std::isfinite(bias[k])) return false;
        b[k] = bias[k];
    }
    const StftBasis basis(nFft);
    for (int j = 0; j < nFft; j++) w2[j] = (float)(basis.wnd[j] * basis.wnd[j]);
    // the synthesis basis as A fragments: lane (row lane & 15 = sample, k-step column lane >> 4), element e = k-step 4 q + e, i.e. row
    // 16 q + 4 e + (lane >> 4) of the spectrum image: bin kk for kk < K' (cos), bin kk - K' otherwise (-sin)
    std::vector<float> inv((size_t)nst * nk2 * 256, 0.f);
    for (int st = 0; st < nst; st++)
        for (int q = 0; q < nk2; q++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 4; e++) {
                    const int j = st * 16 + (lane & 15), kk = 16 * q + 4 * e + (lane >> 4), k = kk < kp ? kk : kk - kp;
                    if (j >= nFft || k >= bins) continue;
                    const int ph = (int)(((long long)k * j) % nFft);
                    inv[(((size_t)st * nk2 + q) * 64 + lane) * 4 + e] = (float)(kk < kp ? basis.wnd[j] * basis.c[ph] : -basis.wnd[j] * basis.s[ph]);
                }
    float* d[4] = {NULL, NULL, NULL, NULL};
    if (!upload(d[0], stft_forward_table(nFft, basis)) || !upload(d[1], inv) || !upload(d[2], b) || !upload(d[3], w2)) {
        for (float* p : d)
            if (p) gpuErrChk(hipFree(p));
        return false;
    }
    gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be reading what is replaced)
    for (float* p : {m_fwdTab, m_invTab, m_bias, m_wnd2})
        if (p) gpuErrChk(hipFree(p));
    m_fwdTab = d[0];
    m_invTab = d[1];
    m_bias = d[2];
    m_wnd2 = d[3];
    m_nFft = nFft;
    m_hop = hop;
    return true;
}

long long Denoiser::ready(long long k, int last) const {
    if (!isSet() || k <= m_nFft / 2) return 0;
    if (last) return k;
    const long long r = ((k - m_nFft / 2) / m_hop + 1) * m_hop - m_nFft / 2;
    return r > 0 ? r : 0;
}

bool Denoiser::acceptable(const DenoiseReq* reqs, int count) const {
    if (!isSet() || reqs == NULL || count < 1 || count > 65535) return false;
    const int half = m_nFft / 2, over = m_nFft / m_hop;
    long long tiles = 0;
    for (int i = 0; i < count; i++) {
        const DenoiseReq& r = reqs[i];
        if (r.in == NULL || r.out == NULL || (r.inType != 16 && r.inType != 32) || (r.outType != 16 && r.outType != 32) || r.nIn < 1 ||
            r.count < 1 || r.first < 0 || r.t0 < 0 || r.first > 0x7ffffff0LL - r.nIn || !(r.strength >= 0.f) || !std::isfinite(r.strength))
            return false;
        // the outputs that the samples below first + nIn give, and the lowest sample that the range needs: its first output's first
        // covering frame starts at ((t0 + N/2) / hop - O + 1) hop - N/2 (below 0: the reflection, which reads from sample 0 on)
        if (r.t0 + r.count > ready(r.first + r.nIn, r.last)) return false;
        const long long ub0 = (r.t0 + half) / m_hop, ub1 = (r.t0 + r.count - 1 + half) / m_hop, need0 = (ub0 - over + 1) * m_hop - half;
        if ((need0 > 0 ? need0 : 0) < r.first) return false;
        if (!is_device_ptr(r.in) || !is_device_ptr((const char*)r.in + (size_t)(r.nIn - 1) * (r.inType / 8)) || !is_device_ptr(r.out) ||
            !is_device_ptr((const char*)r.out + (size_t)(r.count - 1) * (r.outType / 8)))
            return false;
        tiles += tileOf(ub1) - tileOf(ub0) + 1;
        if (tiles > 0x7ffffff0) return false;
    }
    return true;
}

bool Denoiser::run(const DenoiseReq* reqs, int count, hipStream_t stream) {
    if (!acceptable(reqs, count)) return false;
    const int half = m_nFft / 2;
    std::vector<DenoiseJob> jobs(count);
    int tiles = 0;
    for (int i = 0; i < count; i++) {
        const DenoiseReq& r = reqs[i];
        DenoiseJob& jb = jobs[i];
        memset(&jb, 0, sizeof(jb));
        jb.in = r.in;
        jb.out = r.out;
        jb.first = r.first;
        jb.t0 = r.t0;
        jb.nIn = r.nIn;
        jb.count = r.count;
        jb.frames = r.last ? (int)((r.first + r.nIn) / m_hop + 1) : INT_MAX;
        jb.tile0 = tiles;
        jb.tileBase = (int)tileOf((r.t0 + half) / m_hop);
        jb.inType = r.inType;
        jb.outType = r.outType;
        jb.strength = r.strength;
        tiles += (int)(tileOf((r.t0 + r.count - 1 + half) / m_hop) - jb.tileBase + 1);
    }
    if (count > m_jobCap) {
        gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be using what is replaced)
        if (m_jobs) gpuErrChk(hipFree(m_jobs));
        gpuErrChk(hipMalloc((void**)&m_jobs, 2 * (size_t)count * sizeof(DenoiseJob)));
        m_stage.make(2, (size_t)count * sizeof(DenoiseJob));
        m_jobCap = count;
    }
    // the requests through pinned staging, two halves used by alternate calls (as the resampler stages its requests)
    DenoiseJob* const dev = m_jobs + (size_t)m_stage.at() * m_jobCap;
    void* const host = m_stage.acquire();
    memcpy(host, jobs.data(), (size_t)count * sizeof(DenoiseJob));
    gpuErrChk(hipMemcpyAsync(dev, host, (size_t)count * sizeof(DenoiseJob), hipMemcpyHostToDevice, stream));
    m_stage.release(stream);

    DenoiseArgs a;
    a.jobs = dev;
    a.count = count;
    a.fwdTab = (const floatx4*)m_fwdTab;
    a.invTab = (const floatx4*)m_invTab;
    a.bias = m_bias;
    a.wnd2 = m_wnd2;
    a.nFft = m_nFft;
    a.hop = m_hop;
    a.nq = stft_round16(m_nFft) / 16;
    a.kp = stft_round16(m_nFft / 2 + 1);
    // the smallest built variant that holds a wave's tiles in the fewest passes: 1, 3 or 5 bin tiles, 1, 4 or 8 sample tiles
    const int ch = stft_tiles_per_pass(a.kp / 16, kDenoiseBinTilesMax), ci = stft_tiles_per_pass(a.nq, kDenoiseSampleTilesMax);
    const int vh = ch <= 1 ? 0 : ch <= 3 ? 1 : 2, vi = ci <= 1 ? 0 : ci <= 4 ? 1 : 2;
    const size_t lds = ldsBytes(m_nFft, m_hop);
    const bool optIn = !(m_ldsReady >> (3 * vh + vi) & 1);      // (per engine, hence per device: the attribute belongs to the device's copy of the kernel)
    bool ok = false;
    switch (vh) {
        case 0: ok = launchDenoise<1>(vi, a, tiles, lds, stream, optIn); break;
        case 1: ok = launchDenoise<3>(vi, a, tiles, lds, stream, optIn); break;
        default: ok = launchDenoise<5>(vi, a, tiles, lds, stream, optIn); break;
    }
    if (ok) m_ldsReady |= (unsigned short)(1 << (3 * vh + vi));
    return ok;
}

}  // namespace wn
