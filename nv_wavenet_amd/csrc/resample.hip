// resample.hip -- the kernel and the host side of wn::Resampler (resample.hpp).  Compiled once: fp32 throughout, the requests' sample
// types are a conversion at the staging and at the store.
#include "resample.hpp"

#include "resample_core.hpp"

#include <string.h>

#include <vector>

namespace wn {

namespace {

inline int round16(long long v) { return (int)(16 * ((v + 15) / 16)); }

struct ResampleArgs {
    const ResampleJob* jobs;
    int count;
    ResampleTab t;
};

// G, CH: as resample_tile_gemm (resample_core.hpp)
template <int G, int CH>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float span[];
    const int tid = threadIdx.x;
    const int hop = a.t.hop, spare = a.t.spare;

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
    const long long i0 = blk0 * hop + a.t.j0;
    const int span_n = (live - 1) * hop + 16 * a.t.nq;
    for (int l = tid; l < span_n; l += kResampleThreads) {
        const long long rel = i0 + l - jb.first;      // (first >= 0: an index below zero is below first)
        float v = 0.f;
        if (rel >= 0 && rel < jb.nIn) v = jb.inType == 16 ? (float)((const short*)jb.in)[rel] : ((const float*)jb.in)[rel];
        span[l + spare * (l / hop)] = v;
    }
    __syncthreads();

    // outputs of the range only
    resample_tile_gemm<G, CH>(span, a.t, live, [&](int col, int p, float v) {
        const long long o = (blk0 + col) * a.t.Q - jb.m0 + p;
        if (o < 0 || o >= jb.count) return;
        if (jb.outType == 16) ((short*)jb.out)[o] = resample_pcm16(v);
        else ((float*)jb.out)[o] = v;
    });
}

template <int G, int CH>
bool launchResample(const ResampleArgs& a, int tiles, size_t lds, hipStream_t stream, bool optIn) {
    if (optIn && hipFuncSetAttribute((const void*)resample_kernel<G, CH>, hipFuncAttributeMaxDynamicSharedMemorySize, kResampleLdsMax) != hipSuccess)
        return false;
    hipLaunchKernelGGL((resample_kernel<G, CH>), dim3(tiles), dim3(kResampleThreads), lds, stream, a);
    return hipGetLastError() == hipSuccess;
}

struct ResampleLaunch {
    const ResampleArgs& a;
    int tiles;
    size_t lds;
    hipStream_t stream;
    bool optIn;
    template <int G, int CH> bool run() const { return launchResample<G, CH>(a, tiles, lds, stream, optIn); }
};

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

ResampleTab Resampler::tab() const {
    ResampleTab t;
    t.tab = (const floatx4*)m_tab;
    t.Q = m_g.Q;
    t.hop = m_g.hop;
    t.j0 = m_g.j0;
    t.nq = m_g.wp / 16;
    t.rowTiles = m_g.rowTiles;
    t.spare = m_g.spare;
    return t;
}

// G = 1: a wave's row tiles in the fewest passes of at most kResampleTilesMax, and evenly over those
int Resampler::tilesPerPass() const {
    const int perWave = (m_g.rowTiles + kResampleWaves - 1) / kResampleWaves, passes = (perWave + kResampleTilesMax - 1) / kResampleTilesMax;
    return m_g.groups == 4 ? m_g.rowTiles : (perWave + passes - 1) / passes;
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
    a.t = tab();
    const size_t lds = 4 * (size_t)m_g.spanWords;
    const bool optIn = !m_ldsReady;      // (per engine, hence per device: the attribute belongs to the device's copy of the kernel)
    const bool ok = resample_dispatch(m_g.groups, tilesPerPass(), ResampleLaunch{a, tiles, lds, stream, optIn});
    if (ok) m_ldsReady = true;
    return ok;
}

}  // namespace wn
