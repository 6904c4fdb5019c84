// analysis.hip -- the kernel and the host side of wn::Analysis (analysis.hpp).  Compiled once: fp32 throughout, the request's
// precision is a conversion at the store.
#include "analysis.hpp"

#include "stft_core.hpp"

#include <math.h>
#include <string.h>

#include <vector>

namespace wn {

namespace {

constexpr int kAnalysisWaves = 4, kAnalysisThreads = 64 * kAnalysisWaves;
constexpr int kAnalysisTilesMax = 5;      // bin tiles a wave holds at a time: ten accumulators, ten operand fragments in flight

inline int round16(int v) { return stft_round16(v); }

struct AnalysisArgs {
    const AnalysisJob* jobs;
    int count;
    const floatx4* dftTab;
    const floatx4* melTab;
    const short* mulawTab;
    int nFft, hop, nMel;
    int nq;                  // J' / 16: operand fragments of a bin tile's real (or imaginary) part
    int kp;                  // K'
    int spanWords;           // words of LDS before the magnitude image
    int thresholds;          // of the mu-law table: the largest y
    float logFloor;          // the fp32 of log 1e-5
};

// The samples [16 hop ti, 16 hop (ti + 1)) of a request, clipped to n: y = how many thresholds are <= p.
__device__ __forceinline__ void mulaw_tile(const AnalysisJob& jb, const int ti, const short* thr, const int nthr, const int hop, const int tid) {
    int top = 1;
    while (2 * top <= nthr) top *= 2;
    const long long t0 = (long long)ti * 16 * hop;
    const long long t1 = t0 + 16 * hop < jb.n ? t0 + 16 * hop : jb.n;
    for (long long t = t0 + tid; t < t1; t += kAnalysisThreads) {
        const int p = jb.pcm[t];
        int pos = 0;
        for (int step = top; step >= 1; step >>= 1) {
            const int at = pos + step;                  // (thr[at - 1] is read only where it exists)
            const int v = thr[(at <= nthr ? at : nthr) - 1];
            pos += (at <= nthr && v <= p) ? step : 0;
        }
        jb.y[t] = pos;
    }
}

// CH: bin tiles a wave holds at a time; the host picks the smallest that does the bins in the fewest passes.
template <int CH>
__global__ __launch_bounds__(kAnalysisThreads) void analysis_kernel(const AnalysisArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* const span = (float*)lds;
    float* const mag = span + a.spanWords;
    short* const thr = (short*)(mag + a.kp * 16);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, fl = lane & 15;
    const int nFft = a.nFft, hop = a.hop;

    // this workgroup's request by bisection of the first tiles, and its tile of it
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.jobs[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const AnalysisJob jb = a.jobs[lo];
    const int ti = blockIdx.x - jb.tile0;

    if (jb.y != NULL)
        for (int i = tid; i < a.thresholds; i += kAnalysisThreads) thr[i] = a.mulawTab[i];
    if (jb.mel != NULL) {
        // the span: padded positions u0 + l; position u is sample u - nFft / 2, reflected at both ends; zero from the end of the last frame
        const int span_n = 15 * hop + 16 * a.nq;
        const long long u0 = (long long)ti * 16 * hop, uEnd = (long long)(jb.frames - 1) * hop + nFft;
        for (int l = tid; l < span_n; l += kAnalysisThreads) {
            const long long u = u0 + l;
            float v = 0.f;
            if (u < uEnd) {
                long long t = u - nFft / 2;
                if (t < 0) t = -t;
                else if (t >= jb.n) t = 2 * ((long long)jb.n - 1) - t;
                v = (float)jb.pcm[t] * (1.f / 32768.f);
            }
            span[span_at(l, hop)] = v;
        }
    }
    __syncthreads();
    if (jb.y != NULL) mulaw_tile(jb, ti, thr, a.thresholds, hop, tid);
    if (jb.mel == NULL) return;

    // ---- the DFT: bin tile t belongs to wave t & 3; CH of a wave's tiles per pass over the span ----
    const int nbt = a.kp >> 4, nq = a.nq;
    const floatx4* const tab = a.dftTab + lane;
    const float* const bp = span + fl * (hop + 4);
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
        // |X| of bins 16 t + 4 g + r, frame fl, to the image [K'][16]
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const int t = first + 4 * i;
            if (t < nbt)
#pragma unroll
                for (int r = 0; r < 4; r++) mag[(t * 16 + 4 * g + r) * 16 + fl] = sqrtf(re[i][r] * re[i][r] + im[i][r] * im[i][r]);
        }
    }
    __syncthreads();

    // ---- the mel projection: channel tile ct belongs to wave ct & 3, at most two a wave ----
    const int nct = (a.nMel + 15) >> 4, nk = a.kp >> 4;
    if (w >= nct) return;
    const floatx4* const mt = a.melTab + lane;
    const size_t at0 = (size_t)w * nk * 64, at1 = (size_t)(w + 4 < nct ? w + 4 : w) * nk * 64;
    floatx4 acc0 = floatx4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    for (int q = 0; q < nk; q++) {
        const floatx4 a0 = mt[at0 + (size_t)q * 64], a1 = mt[at1 + (size_t)q * 64];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float b = mag[(16 * q + 4 * e + g) * 16 + fl];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b, acc1, 0, 0, 0);
        }
    }
    const long long f = (long long)ti * 16 + fl;
    if (f >= jb.frames) return;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int ct = w + 4 * s;
        if (ct >= nct) break;
        const floatx4 acc = s ? acc1 : acc0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int c = ct * 16 + 4 * g + r;
            if (c >= a.nMel) continue;
            // log(max(m, 1e-5)) = max(log m, log 1e-5): a zero (or, with a basis of mixed signs, a negative) sum takes the floor
            const float v = fmaxf(logf(acc[r]), a.logFloor);
            const long long o = c * jb.cStride + f * jb.fStride;
            if (jb.precision == 16) ((_Float16*)jb.mel)[o] = (_Float16)v;
            else ((float*)jb.mel)[o] = v;
        }
    }
}

template <int CH>
bool launchAnalysis(const AnalysisArgs& a, int tiles, size_t lds, hipStream_t stream, bool optIn) {
    if (optIn && hipFuncSetAttribute((const void*)analysis_kernel<CH>, hipFuncAttributeMaxDynamicSharedMemorySize, kAnalysisLdsMax) != hipSuccess)
        return false;
    hipLaunchKernelGGL((analysis_kernel<CH>), dim3(tiles), dim3(kAnalysisThreads), lds, stream, a);
    return hipGetLastError() == hipSuccess;
}

// the reference's mu_law_encode in float64
int mulaw_of(int p, int levels) {
    const double mu = levels - 1, x = p / 32768.0;
    const double m = log1p(mu * fabs(x)) / log1p(mu);
    return (int)(((x < 0 ? -m : m) + 1) / 2 * mu + 0.5);
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

size_t Analysis::ldsBytes(int nFft, int hop, int levels) {
    const size_t span = 15 * (size_t)hop + round16(nFft);
    return 4 * (span + 4 * (span / hop + 1)) + 64 * (size_t)round16(nFft / 2 + 1) + 16 * (size_t)((2 * levels + 15) / 16);
}

void Analysis::clear() {
    if (m_dftTab) gpuErrChk(hipFree(m_dftTab));
    if (m_melTab) gpuErrChk(hipFree(m_melTab));
    if (m_mulawTab) gpuErrChk(hipFree(m_mulawTab));
    if (m_jobs) gpuErrChk(hipFree(m_jobs));
    m_dftTab = m_melTab = NULL;
    m_mulawTab = NULL;
    m_jobs = NULL;
    m_jobCap = 0;
    m_nFft = 0;
}

bool Analysis::set(int nFft, int hop, int nMel, const float* basis, int levels) {
    if (nFft < kAnalysisFftMin || nFft > kAnalysisFftMax || (nFft & 3) != 0 || hop < 1 || hop > nFft || nMel < 1 || nMel > kAnalysisMelMax ||
        basis == NULL || is_device_ptr(basis) || levels < 2 || levels > 65536 || ldsBytes(nFft, hop, levels) > (size_t)kAnalysisLdsMax)
        return false;
    const int bins = nFft / 2 + 1, nk = round16(bins) / 16, nct = (nMel + 15) / 16;
    const std::vector<float> dft = stft_forward_table(nFft, StftBasis(nFft));
    // the mel basis as A fragments: lane (row lane & 15, k-step column lane >> 4), element e = k-step 4 q + e, i.e. bin 16 q + 4 e + (lane >> 4)
    std::vector<float> mel((size_t)nct * nk * 256, 0.f);
    for (int ct = 0; ct < nct; ct++)
        for (int q = 0; q < nk; q++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 4; e++) {
                    const int ch = ct * 16 + (lane & 15), k = 16 * q + 4 * e + (lane >> 4);
                    if (ch < nMel && k < bins) mel[(((size_t)ct * nk + q) * 64 + lane) * 4 + e] = basis[(size_t)ch * bins + k];
                }
    // thresholds: the smallest p with y(p) >= k, k = 1 .. y(32767) (y never decreases)
    std::vector<short> thr;
    for (int p = -32768; p < 32768; p++)
        for (const int y = mulaw_of(p, levels); (int)thr.size() < y;) thr.push_back((short)p);
    if (thr.empty() || (int)thr.size() > levels - 1) return false;

    float *dDft, *dMel;
    short* dThr;
    if (!upload(dDft, dft)) return false;
    if (!upload(dMel, mel)) {
        gpuErrChk(hipFree(dDft));
        return false;
    }
    if (!upload(dThr, thr)) {
        gpuErrChk(hipFree(dDft));
        gpuErrChk(hipFree(dMel));
        return false;
    }
    gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be reading what is replaced)
    if (m_dftTab) gpuErrChk(hipFree(m_dftTab));
    if (m_melTab) gpuErrChk(hipFree(m_melTab));
    if (m_mulawTab) gpuErrChk(hipFree(m_mulawTab));
    m_dftTab = dDft;
    m_melTab = dMel;
    m_mulawTab = dThr;
    m_nFft = nFft;
    m_hop = hop;
    m_nMel = nMel;
    m_levels = levels;
    return true;
}

bool Analysis::acceptable(const AnalysisReq* reqs, int count) const {
    if (!ready() || reqs == NULL || count < 1 || count > 65535) return false;
    long long tiles = 0;
    for (int i = 0; i < count; i++) {
        const AnalysisReq& q = reqs[i];
        if (q.pcm == NULL || q.n <= m_nFft / 2 || q.n > 0x7ffffff0 || (q.mel == NULL && q.y == NULL)) return false;
        if (!is_device_ptr(q.pcm) || !is_device_ptr(q.pcm + (q.n - 1))) return false;
        const int fr = q.n / m_hop + 1;
        if (q.mel != NULL) {
            if ((q.precision != 32 && q.precision != 16) || q.cStride <= 0 || q.fStride <= 0) return false;
            const size_t eb = q.precision == 16 ? 2 : 4;
            if (!is_device_ptr(q.mel) || !is_device_ptr((const char*)q.mel + ((size_t)(m_nMel - 1) * q.cStride + (size_t)(fr - 1) * q.fStride) * eb))
                return false;
        }
        if (q.y != NULL && (!is_device_ptr(q.y) || !is_device_ptr(q.y + (q.n - 1)))) return false;
        tiles += (fr + 15) / 16;
        if (tiles > 0x7ffffff0) return false;
    }
    return true;
}

bool Analysis::run(const AnalysisReq* reqs, int count, hipStream_t stream) {
    if (!acceptable(reqs, count)) return false;
    std::vector<AnalysisJob> jobs(count);
    int tiles = 0;
    for (int i = 0; i < count; i++) {
        const AnalysisReq& q = reqs[i];
        AnalysisJob& jb = jobs[i];
        memset(&jb, 0, sizeof(jb));
        jb.pcm = q.pcm;
        jb.mel = q.mel;
        jb.y = q.y;
        jb.cStride = q.cStride;
        jb.fStride = q.fStride;
        jb.n = q.n;
        jb.frames = q.n / m_hop + 1;
        jb.tile0 = tiles;
        jb.precision = q.precision;
        tiles += (jb.frames + 15) / 16;
    }
    if (count > m_jobCap) {
        gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be using what is replaced)
        if (m_jobs) gpuErrChk(hipFree(m_jobs));
        gpuErrChk(hipMalloc((void**)&m_jobs, 2 * (size_t)count * sizeof(AnalysisJob)));
        m_stage.make(2, (size_t)count * sizeof(AnalysisJob));
        m_jobCap = count;
    }
    // the requests through pinned staging, two halves used by alternate calls (as the upsampling pass stages its requests)
    AnalysisJob* const dev = m_jobs + (size_t)m_stage.at() * m_jobCap;
    void* const host = m_stage.acquire();
    memcpy(host, jobs.data(), (size_t)count * sizeof(AnalysisJob));
    gpuErrChk(hipMemcpyAsync(dev, host, (size_t)count * sizeof(AnalysisJob), hipMemcpyHostToDevice, stream));
    m_stage.release(stream);

    AnalysisArgs a;
    a.jobs = dev;
    a.count = count;
    a.dftTab = (const floatx4*)m_dftTab;
    a.melTab = (const floatx4*)m_melTab;
    a.mulawTab = m_mulawTab;
    a.nFft = m_nFft;
    a.hop = m_hop;
    a.nMel = m_nMel;
    a.nq = round16(m_nFft) / 16;
    a.kp = round16(m_nFft / 2 + 1);
    const size_t span = 15 * (size_t)m_hop + round16(m_nFft);
    a.spanWords = (int)(span + 4 * (span / m_hop + 1));
    a.thresholds = mulaw_of(32767, m_levels);      // (as set() counted them)
    a.logFloor = (float)log(1e-5);
    const size_t lds = ldsBytes(m_nFft, m_hop, m_levels);
    // a wave's bin tiles in the fewest passes of at most kAnalysisTilesMax, and evenly over those
    const int perWave = (a.kp / 16 + kAnalysisWaves - 1) / kAnalysisWaves, passes = (perWave + kAnalysisTilesMax - 1) / kAnalysisTilesMax;
    const int ch = (perWave + passes - 1) / passes;
    const bool optIn = !(m_ldsReady >> ch & 1);      // (per engine, hence per device: the attribute belongs to the device's copy of the kernel)
    bool ok = false;
    switch (ch) {
        case 1: ok = launchAnalysis<1>(a, tiles, lds, stream, optIn); break;
        case 2: ok = launchAnalysis<2>(a, tiles, lds, stream, optIn); break;
        case 3: ok = launchAnalysis<3>(a, tiles, lds, stream, optIn); break;
        case 4: ok = launchAnalysis<4>(a, tiles, lds, stream, optIn); break;
        default: ok = launchAnalysis<5>(a, tiles, lds, stream, optIn); break;
    }
    if (ok) m_ldsReady |= (unsigned char)(1 << ch);
    return ok;
}

}  // namespace wn
