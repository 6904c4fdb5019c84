// resample.hip -- the kernel and the host side of wn::Resampler (resample.hpp).  Compiled once: fp32 throughout, the requests' sample
// types are a conversion at the staging and at the store.
#include "resample.hpp"

#include <string.h>

#include <vector>

namespace wn {

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kResampleWaves = 4, kResampleThreads = 64 * kResampleWaves;
constexpr int kResampleTilesMax = 5;      // row tiles a wave holds at a time (G = 1): five accumulators, five operand fragments in flight

inline int round16(long long v) { return (int)(16 * ((v + 15) / 16)); }

struct ResampleArgs {
    const ResampleJob* jobs;
    int count;
    const floatx4* tab;
    int Q, hop;
    int j0;
    int nq;                  // W' / 16: operand fragments of a row tile
    int rowTiles;
    int spare;               // s
};

// G: 16-block groups of a workgroup (4: every wave its own group and all CH = rowTiles row tiles; 1: row tile t belongs to wave t & 3,
// CH of a wave's tiles per pass over the span).
template <int G, int CH>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float span[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, fl = lane & 15;
    const int hop = a.hop, spare = a.spare;

    // this workgroup's request by bisection of the first tiles, and its tile of it
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.jobs[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const ResampleJob jb = a.jobs[lo];
    const int ti = blockIdx.x - jb.tile0;
    // its blocks of the range: ti * 16 G + (0 .. live), and the span that they read: inputs i0 + (0 .. span_n)
    const int left = jb.blocks - ti * 16 * G, live = left < 16 * G ? left : 16 * G;
    const long long blk0 = jb.block0 + (long long)ti * 16 * G;
    const long long i0 = blk0 * hop + a.j0;
    const int span_n = (live - 1) * hop + 16 * a.nq;
    for (int l = tid; l < span_n; l += kResampleThreads) {
        const long long rel = i0 + l - jb.first;      // (first >= 0: an index below zero is below first)
        float v = 0.f;
        if (rel >= 0 && rel < jb.nIn) v = jb.inType == 16 ? (float)((const short*)jb.in)[rel] : ((const float*)jb.in)[rel];
        span[l + spare * (l / hop)] = v;
    }
    __syncthreads();

    const int grp = G == 4 ? w : 0;
    if (grp * 16 >= live) return;
    // (a block lane past the last live block reads the last one's inputs, and is not stored)
    const int col = grp * 16 + fl, src = col < live ? col : live - 1;
    const float* const bp = span + src * (hop + spare) + g;
    const floatx4* const tab = a.tab + lane;
    const int nq = a.nq, nrt = a.rowTiles;
    const long long mBlock = (blk0 + col) * a.Q - jb.m0;      // the block's first output, relative to the range
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
        // outputs 16 t + 4 g + r of block `col`, those of the range only
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const int t = first + (G == 4 ? 1 : 4) * i;
            if (t >= nrt || col >= live) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int p = t * 16 + 4 * g + r;
                const long long o = mBlock + p;
                if (p >= a.Q || o < 0 || o >= jb.count) continue;
                if (jb.outType == 16) ((short*)jb.out)[o] = (short)(int)fminf(fmaxf(rintf(acc[i][r]), -32768.f), 32767.f);
                else ((float*)jb.out)[o] = acc[i][r];
            }
        }
    }
}

template <int G, int CH>
bool launchResample(const ResampleArgs& a, int tiles, size_t lds, hipStream_t stream, bool optIn) {
    if (optIn && hipFuncSetAttribute((const void*)resample_kernel<G, CH>, hipFuncAttributeMaxDynamicSharedMemorySize, kResampleLdsMax) != hipSuccess)
        return false;
    hipLaunchKernelGGL((resample_kernel<G, CH>), dim3(tiles), dim3(kResampleThreads), lds, stream, a);
    return hipGetLastError() == hipSuccess;
}

int gcd(int a, int b) { return b == 0 ? a : gcd(b, a % b); }
// floor and ceiling of a / b, b > 0, for a of either sign
long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

}  // namespace

ResampleGeom resampleGeom(int up, int down, int nTaps) {
    ResampleGeom g;
    g.q = 1;
    while (up * g.q < 16 || g.q * down < 4) g.q++;
    g.Q = up * g.q;
    g.hop = g.q * down;
    const long long c = (nTaps - 1) / 2;
    g.j0 = (int)-(c / up);
    g.wp = round16(((long long)(g.Q - 1) * down + c) / up - g.j0 + 1);
    g.rowTiles = (g.Q + 15) / 16;
    g.groups = g.rowTiles < 4 ? 4 : 1;
    g.spare = ((4 - g.hop) % 8 + 8) % 8;
    const long long span = (long long)(16 * g.groups - 1) * g.hop + g.wp;
    g.spanWords = span + g.spare * (span / g.hop + 1);
    return g;
}

void Resampler::clear() {
    if (m_tab) gpuErrChk(hipFree(m_tab));
    if (m_jobs) gpuErrChk(hipFree(m_jobs));
    m_tab = NULL;
    m_jobs = NULL;
    m_jobCap = 0;
}

bool Resampler::set(int up, int down, const double* taps, int nTaps) {
    if (up < 1 || up > kResampleFactorMax || down < 1 || down > kResampleFactorMax || gcd(up, down) != 1 || nTaps < 1 || (nTaps & 1) == 0 ||
        taps == NULL || is_device_ptr(taps))
        return false;
    const ResampleGeom g = resampleGeom(up, down, nTaps);
    if (4 * g.spanWords > kResampleLdsMax) return false;
    // A fragments: lane (row lane & 15, k-step column lane >> 4), element e = k-step 4 qd + e, i.e. input 16 qd + 4 e + (lane >> 4)
    const int nq = g.wp / 16;
    const long long c = (nTaps - 1) / 2;
    std::vector<float> tab((size_t)g.rowTiles * nq * 256, 0.f);
    for (int t = 0; t < g.rowTiles; t++)
        for (int qd = 0; qd < nq; qd++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 4; e++) {
                    const int p = t * 16 + (lane & 15), j = 16 * qd + 4 * e + (lane >> 4);
                    const long long k = c + (long long)p * down - (long long)(j + g.j0) * up;
                    if (p < g.Q && k >= 0 && k < nTaps) tab[(((size_t)t * nq + qd) * 64 + lane) * 4 + e] = (float)taps[k];
                }
    float* dTab = NULL;
    if (hipMalloc((void**)&dTab, tab.size() * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    gpuErrChk(hipMemcpy(dTab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be reading what is replaced)
    if (m_tab) gpuErrChk(hipFree(m_tab));
    m_tab = dTab;
    m_up = up;
    m_down = down;
    m_centre = (int)c;
    m_g = g;
    m_ldsReady = false;      // (another ratio may take another kernel)
    return true;
}

bool Resampler::acceptable(const ResampleReq* reqs, int count) const {
    if (!ready() || reqs == NULL || count < 1 || count > 65535) return false;
    const long long kIndexMax = 1LL << 50;      // (index x factor stays far from overflow)
    long long tiles = 0;
    for (int i = 0; i < count; i++) {
        const ResampleReq& r = reqs[i];
        if (r.in == NULL || r.out == NULL || (r.inType != 16 && r.inType != 32) || (r.outType != 16 && r.outType != 32) || r.nIn < 1 ||
            r.count < 1 || r.first < 0 || r.m0 < 0 || r.first > kIndexMax || r.m0 > kIndexMax)
            return false;
        // the inputs that the range needs: [ceil((m0 M - c) / L), floor(((m0 + count - 1) M + c) / L)], those of index >= 0
        const long long need0 = ceil_div(r.m0 * m_down - m_centre, m_up), need1 = floor_div((r.m0 + r.count - 1) * m_down + m_centre, m_up);
        if ((need0 > 0 ? need0 : 0) < r.first || (!r.last && need1 >= r.first + r.nIn)) return false;
        if (!is_device_ptr(r.in) || !is_device_ptr((const char*)r.in + (size_t)(r.nIn - 1) * (r.inType / 8)) || !is_device_ptr(r.out) ||
            !is_device_ptr((const char*)r.out + (size_t)(r.count - 1) * (r.outType / 8)))
            return false;
        const long long blocks = (r.m0 + r.count - 1) / m_g.Q - r.m0 / m_g.Q + 1;
        tiles += (blocks + 16 * m_g.groups - 1) / (16 * m_g.groups);
        if (tiles > 0x7ffffff0) return false;
    }
    return true;
}

bool Resampler::run(const ResampleReq* reqs, int count, hipStream_t stream) {
    if (!acceptable(reqs, count)) return false;
    std::vector<ResampleJob> jobs(count);
    int tiles = 0;
    for (int i = 0; i < count; i++) {
        const ResampleReq& r = reqs[i];
        ResampleJob& jb = jobs[i];
        memset(&jb, 0, sizeof(jb));
        jb.in = r.in;
        jb.out = r.out;
        jb.first = r.first;
        jb.m0 = r.m0;
        jb.block0 = r.m0 / m_g.Q;
        jb.nIn = r.nIn;
        jb.count = r.count;
        jb.blocks = (int)((r.m0 + r.count - 1) / m_g.Q - jb.block0 + 1);
        jb.tile0 = tiles;
        jb.inType = r.inType;
        jb.outType = r.outType;
        tiles += (jb.blocks + 16 * m_g.groups - 1) / (16 * m_g.groups);
    }
    if (count > m_jobCap) {
        gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be using what is replaced)
        if (m_jobs) gpuErrChk(hipFree(m_jobs));
        gpuErrChk(hipMalloc((void**)&m_jobs, 2 * (size_t)count * sizeof(ResampleJob)));
        m_stage.make(2, (size_t)count * sizeof(ResampleJob));
        m_jobCap = count;
    }
    // the requests through pinned staging, two halves used by alternate calls (as the analysis front end stages its requests)
    ResampleJob* const dev = m_jobs + (size_t)m_stage.at() * m_jobCap;
    void* const host = m_stage.acquire();
    memcpy(host, jobs.data(), (size_t)count * sizeof(ResampleJob));
    gpuErrChk(hipMemcpyAsync(dev, host, (size_t)count * sizeof(ResampleJob), hipMemcpyHostToDevice, stream));
    m_stage.release(stream);

    ResampleArgs a;
    a.jobs = dev;
    a.count = count;
    a.tab = (const floatx4*)m_tab;
    a.Q = m_g.Q;
    a.hop = m_g.hop;
    a.j0 = m_g.j0;
    a.nq = m_g.wp / 16;
    a.rowTiles = m_g.rowTiles;
    a.spare = m_g.spare;
    const size_t lds = 4 * (size_t)m_g.spanWords;
    // G = 1: a wave's row tiles in the fewest passes of at most kResampleTilesMax, and evenly over those
    const int perWave = (m_g.rowTiles + kResampleWaves - 1) / kResampleWaves, passes = (perWave + kResampleTilesMax - 1) / kResampleTilesMax;
    const int ch = m_g.groups == 4 ? m_g.rowTiles : (perWave + passes - 1) / passes;
    const bool optIn = !m_ldsReady;      // (per engine, hence per device: the attribute belongs to the device's copy of the kernel)
    bool ok = false;
    if (m_g.groups == 4) switch (ch) {
            case 1: ok = launchResample<4, 1>(a, tiles, lds, stream, optIn); break;
            case 2: ok = launchResample<4, 2>(a, tiles, lds, stream, optIn); break;
            default: ok = launchResample<4, 3>(a, tiles, lds, stream, optIn); break;
        }
    else switch (ch) {
            case 1: ok = launchResample<1, 1>(a, tiles, lds, stream, optIn); break;
            case 2: ok = launchResample<1, 2>(a, tiles, lds, stream, optIn); break;
            case 3: ok = launchResample<1, 3>(a, tiles, lds, stream, optIn); break;
            case 4: ok = launchResample<1, 4>(a, tiles, lds, stream, optIn); break;
            default: ok = launchResample<1, 5>(a, tiles, lds, stream, optIn); break;
        }
    if (ok) m_ldsReady = true;
    return ok;
}

}  // namespace wn
