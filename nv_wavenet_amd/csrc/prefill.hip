// prefill.hip -- the kernels and the host side of wn::Prefill (prefill.hpp).  Compiled once: R in {32, 64, 128, 256}, both precisions.
#include "prefill.hpp"

#include <string.h>

#include <vector>

#include "time_tiles.hpp"

namespace wn {

namespace {

// x_0[k] = embPrev[y[k-2]] + embCur[y[k-1]] (history 128 before the start), tanh when the model says so: the embedding of wavenet_wg.
// blockIdx.y: request, x: time tile.  Rows at and past n (the padding of the last tile) are zero.
template <bool F16>
__global__ __launch_bounds__(256) void prefill_embed_kernel(const PrefillJob* __restrict__ jobs, int R, int A, const void* __restrict__ embPrevV,
                                                            const void* __restrict__ embCurV, int tanhEmbed, float* __restrict__ xf,
                                                            char* __restrict__ xd, int rows) {
    using elem = typename Prec<F16>::elem;
    using quad = typename Prec<F16>::quad;
    const PrefillJob jb = jobs[blockIdx.y];
    const int tile0 = blockIdx.x;
    if (tile0 >= jb.tiles) return;
    const elem* const embPrev = (const elem*)embPrevV;
    const elem* const embCur = (const elem*)embCurV;
    const int rowB = R * (int)sizeof(elem), quads = R / 4;
    for (int it = threadIdx.x; it < 16 * quads; it += blockDim.x) {
        const int q = it % quads, r = tile0 * 16 + it / quads, k = jb.t0 + r;
        const int tile = q >> 2, g = q & 3;
        floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
        if (k < jb.n) {
            const int yc = k >= 1 ? clamp_sample(jb.y[k - 1], A) : 128, yp = k >= 2 ? clamp_sample(jb.y[k - 2], A) : 128;
            const floatx4 ep = quad_to_f32(*(const quad*)(embPrev + (size_t)yp * R + q * 4));
            const floatx4 ec = quad_to_f32(*(const quad*)(embCur + (size_t)yc * R + q * 4));
            v = ep + ec;
            if (tanhEmbed) {
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = tanh_t<F16>(v[e]);
            }
        }
        const size_t row = (size_t)blockIdx.y * rows + r;
        *(floatx4*)(xf + row * R + q * 4) = v;
        put_quad<F16>(xd + row * rowB + quad_off<F16>(tile, g), v);
        if (k == jb.n - 1) put_quad<F16>(jb.dst + sizeof(SlotStateHeader) + quad_off<F16>(tile, g), v);      // layer 0: d = 1, one slot
    }
}

// One layer over one time tile of one request: gate pre-activation (bias, conditioning, dilated tap, current tap), gate, residual.
// The four waves split the output rows as in wavenet_wg and exchange h through LDS.  blockIdx.y: request, x: time tile.
template <bool F16, int R>
__global__ __launch_bounds__((PCfg<F16, R>::THREADS)) void prefill_layer_kernel(const PrefillJob* __restrict__ jobs, const PrefillLayer ly,
                                                                                const char* __restrict__ wblob, size_t waveBytes,
                                                                                const float* __restrict__ bl, int nCond, float* __restrict__ xf,
                                                                                const char* __restrict__ xdIn, char* __restrict__ xdOut, int rows) {
    using C = PCfg<F16, R>;
    using P = Prec<F16>;
    using frag = typename P::frag;
    using elem = typename P::elem;
    constexpr int NW = C::NW, HTW = C::HTW, KF_R = C::KF_R, KFC = C::KFC, RT = C::RT, ROWB = C::ROWB;
    __shared__ __attribute__((aligned(16))) char hbuf[KF_R * 1024];

    const PrefillJob jb = jobs[blockIdx.y];
    if ((int)blockIdx.x >= jb.tiles) return;      // (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const int r = blockIdx.x * 16 + j, k = jb.t0 + r;      // this lane's column: window row, local sample
    const unsigned laneOff = (unsigned)lane * 16u;
    const char* const wbase = wblob + (size_t)w * waveBytes;
    const size_t jobRow = (size_t)blockIdx.y * rows;

    // gate bias
    floatx4 acc[1][2 * HTW];
#pragma unroll
    for (int i = 0; i < HTW; i++) {
        acc[0][2 * i] = *(const floatx4*)(bl + (w + NW * i) * 16 + g * 4);
        acc[0][2 * i + 1] = *(const floatx4*)(bl + (w + NW * i + RT) * 16 + g * 4);
    }
    // + Wcond c: the features of 16 consecutive samples as B fragments, straight from the caller's tensor, converted as the window
    // feed converts them (slot_feed_kernel); columns past n - 1 (the padding of the last tile) repeat the last sample
    {
        frag cf[1][KFC];
        const long long kk = k < jb.n ? k : jb.n - 1;
#pragma unroll
        for (int kf = 0; kf < KFC; kf++)
#pragma unroll
            for (int e = 0; e < P::EPL; e++) {
                const int c = (kf * P::TPF + (e >> 2)) * 16 + 4 * g + (e & 3);
                float v = 0.f;
                if (c < nCond) {
                    const long long at = c * jb.cStride + kk * jb.tStride;
                    v = jb.precision == 16 ? (float)((const _Float16*)jb.x)[at] : ((const float*)jb.x)[at];
                }
                cf[0][kf][e] = (elem)v;
            }
        gemm_direct<F16, 1, 2 * HTW, KFC>(wbase + (size_t)ly.cond * 1024, laneOff, acc, cf);
    }
    // + Wprev x_l[t - d]: zero before the start, as at a start from silence (and before the window: those columns reach no blob)
    const char* const inJob = xdIn + jobRow * ROWB;
    {
        frag xp[1][KF_R];
        const int rp = r - ly.d;
#pragma unroll
        for (int kf = 0; kf < KF_R; kf++) {
            frag v = {};
            if (rp >= 0) v = *(const frag*)(inJob + (size_t)rp * ROWB + (kf * 4 + g) * 16);
            xp[0][kf] = v;
        }
        gemm_direct<F16, 1, 2 * HTW, KF_R>(wbase + (size_t)ly.prev * 1024, laneOff, acc, xp);
    }
    // + Wcur x_l[t]
    {
        frag xb[1][KF_R];
#pragma unroll
        for (int kf = 0; kf < KF_R; kf++) xb[0][kf] = *(const frag*)(inJob + (size_t)r * ROWB + (kf * 4 + g) * 16);
        gemm_direct<F16, 1, 2 * HTW, KF_R>(wbase + (size_t)ly.cur * 1024, laneOff, acc, xb);
    }
    // gate -> h as B fragments
#pragma unroll
    for (int i = 0; i < HTW; i++) lds_put_tile<F16>(hbuf, w + NW * i, lane, gate4<F16>(acc[0][2 * i], acc[0][2 * i + 1]));
    __syncthreads();
    frag hb[1][KF_R];
    lds_get_frags<F16, KF_R>(hbuf, lane, hb[0]);
    // residual: (Bres + x) + Wres h
    float* const xrow = xf + (jobRow + r) * R;
    floatx4 xa[1][HTW];
#pragma unroll
    for (int i = 0; i < HTW; i++)
        xa[0][i] = *(const floatx4*)(bl + 2 * R + (w + NW * i) * 16 + g * 4) + *(const floatx4*)(xrow + (w + NW * i) * 16 + g * 4);
    gemm_direct<F16, 1, HTW, KF_R>(wbase + (size_t)ly.res * 1024, laneOff, xa, hb);
    // x_{l+1}[k]: the running residual in fp32 (read again by this lane only), the operand in T_data, and -- the last dOut samples --
    // the ring slot of layer l + 1 in the blob
    char* const orow = xdOut + (jobRow + r) * ROWB;
    const bool ring = k < jb.n && k >= jb.n - ly.dOut;
    char* const slot = jb.dst + sizeof(SlotStateHeader) + (size_t)(ly.offOut + (k & (ly.dOut - 1))) * ROWB;
#pragma unroll
    for (int i = 0; i < HTW; i++) {
        const int tile = w + NW * i;
        *(floatx4*)(xrow + tile * 16 + g * 4) = xa[0][i];
        put_quad<F16>(orow + quad_off<F16>(tile, g), xa[0][i]);
        if (ring) put_quad<F16>(slot + quad_off<F16>(tile, g), xa[0][i]);
    }
}

// The blob step: the ring slots no sample of the prime has written (layer l, residues n .. d_l - 1) are zero, and the header.
// blockIdx.y: request.
__global__ __launch_bounds__(256) void prefill_finish_kernel(const PrefillJob* __restrict__ jobs, SlotStateHeader hdr, int rowB, int A) {
    const PrefillJob jb = jobs[blockIdx.y];
    uintx4* const out = (uintx4*)(jb.dst + sizeof(SlotStateHeader));
    const int pps = rowB / 16;
    Dil dl = dil_first();
    for (int l = 0; l < hdr.numLayers; l++) {
        if (dl.d > jb.n) {
            const int first = (dl.off + jb.n) * pps, cnt = (dl.d - jb.n) * pps;
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) out[first + i] = uintx4{0u, 0u, 0u, 0u};
        }
        dl = dil_next(dl, hdr.maxDilation, false);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr.done = jb.n;
        hdr.uid = jb.uid;
        hdr.pad[0] = jb.temp;
        hdr.yInPrev = jb.n >= 2 ? clamp_sample(jb.y[jb.n - 2], A) : 128;
        hdr.yInCur = clamp_sample(jb.y[jb.n - 1], A);
        *(SlotStateHeader*)jb.dst = hdr;
    }
}

template <bool F16, int R>
bool launchLayers(const PrefillModel& m, const PrefillJob* jobs, int count, int maxTiles, float* xf, char* xd0, char* xd1, int rows,
                  hipStream_t stream) {
    using C = PCfg<F16, R>;
    hipLaunchKernelGGL((prefill_embed_kernel<F16>), dim3(maxTiles, count), dim3(256), 0, stream, jobs, R, m.A, m.embPrev, m.embCur, m.tanhEmbed, xf,
                       xd0, rows);
    if (hipGetLastError() != hipSuccess) return false;
    char* in = xd0;
    char* out = xd1;
    for (int l = 0; l + 1 < m.numLayers; l++) {
        hipLaunchKernelGGL((prefill_layer_kernel<F16, R>), dim3(maxTiles, count), dim3(C::THREADS), 0, stream, jobs, m.layers[l], (const char*)m.wblob,
                           m.waveStreamFrags * 1024, m.bias + (size_t)l * m.biasL, m.nCond, xf, (const char*)in, out, rows);
        if (hipGetLastError() != hipSuccess) return false;
        char* const t = in;
        in = out;
        out = t;
    }
    return true;
}

}  // namespace

Prefill::~Prefill() {
    if (m_scratch) gpuErrChk(hipFree(m_scratch));
    if (m_jobs) gpuErrChk(hipFree(m_jobs));
}

bool Prefill::acceptable(const PrefillModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, bool ownX) {
    if (m.nCond <= 0 || reqs == NULL || count < 1 || count > 65535) return false;
    if (m.R != 32 && m.R != 64 && m.R != 128 && m.R != 256) return false;
    const int rowB = m.R * (m.f16 ? 2 : 4);
    const size_t blobBytes = sizeof(SlotStateHeader) + (size_t)m.ringSlots * rowB;
    if (dst == NULL || ((size_t)dst & 15) != 0 || (stride & 15) != 0 || stride < (long long)blobBytes) return false;
    char* const first = (char*)store_target(dst);
    const size_t span = (size_t)(count - 1) * (size_t)stride + blobBytes - 16;
    if (first == NULL || (char*)store_target((char*)dst + span) != first + span) return false;
    for (int i = 0; i < count; i++) {
        const PrefillReq& q = reqs[i];
        if (q.n < 1 || q.y == NULL || (q.precision != 32 && q.precision != 16) || q.cStride <= 0 || q.tStride <= 0 ||
            !temperature_ok(q.temperature) || !is_device_ptr(q.y))
            return false;
        if (!ownX && (q.x == NULL || !is_device_ptr(q.x))) return false;
    }
    return true;
}

bool Prefill::run(const PrefillModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, hipStream_t stream, bool ownX) {
    if (!acceptable(m, reqs, count, dst, stride, ownX)) return false;
    const int rowB = m.R * (m.f16 ? 2 : 4);
    char* const first = (char*)store_target(dst);
    const int W = prefill_window(m.ringSlots);
    std::vector<PrefillJob> jobs(count);
    int maxTiles = 0;
    for (int i = 0; i < count; i++) {
        const PrefillReq& q = reqs[i];
        PrefillJob& jb = jobs[i];
        memset(&jb, 0, sizeof(jb));
        jb.y = q.y;
        jb.x = q.x;
        jb.cStride = q.cStride;
        jb.tStride = q.tStride;
        jb.dst = first + (size_t)i * (size_t)stride;
        jb.n = q.n;
        jb.t0 = prefill_first(q.n, W);
        jb.tiles = (q.n - jb.t0 + 15) / 16;
        jb.precision = q.precision;
        jb.uid = q.uid;
        jb.temp = temperature_word(q.temperature);
        if (jb.tiles > maxTiles) maxTiles = jb.tiles;
    }
    // scratch: the fp32 running residual and two T_data images of x, [count][rows] each
    const int rows = maxTiles * 16;
    const size_t cells = (size_t)count * rows, need = cells * m.R * 4 + 2 * cells * rowB;
    if (need > m_scratchBytes || count > m_jobCap) {
        gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be using what is replaced)
        if (need > m_scratchBytes) {
            if (m_scratch) gpuErrChk(hipFree(m_scratch));
            gpuErrChk(hipMalloc((void**)&m_scratch, need));
            m_scratchBytes = need;
        }
        if (count > m_jobCap) {
            if (m_jobs) gpuErrChk(hipFree(m_jobs));
            gpuErrChk(hipMalloc((void**)&m_jobs, 2 * (size_t)count * sizeof(PrefillJob)));
            m_stage.make(2, (size_t)count * sizeof(PrefillJob));
            m_jobCap = count;
        }
    }
    float* const xf = (float*)m_scratch;
    char* const xd0 = m_scratch + cells * m.R * 4;
    char* const xd1 = xd0 + cells * rowB;
    // the requests through pinned staging, two halves used by alternate calls (as a list save stages its entries)
    PrefillJob* const dev = m_jobs + (size_t)m_stage.at() * m_jobCap;
    void* const host = m_stage.acquire();
    memcpy(host, jobs.data(), (size_t)count * sizeof(PrefillJob));
    gpuErrChk(hipMemcpyAsync(dev, host, (size_t)count * sizeof(PrefillJob), hipMemcpyHostToDevice, stream));
    m_stage.release(stream);

    bool ok = false;
#define WN_PREFILL_CASE(RR)                                                                                                    \
    case RR:                                                                                                                   \
        ok = m.f16 ? launchLayers<true, RR>(m, dev, count, maxTiles, xf, xd0, xd1, rows, stream)                               \
                   : launchLayers<false, RR>(m, dev, count, maxTiles, xf, xd0, xd1, rows, stream);                             \
        break;
    switch (m.R) {
        WN_PREFILL_CASE(32)
        WN_PREFILL_CASE(64)
        WN_PREFILL_CASE(128)
        WN_PREFILL_CASE(256)
    }
#undef WN_PREFILL_CASE
    SlotStateHeader hdr = {};
    hdr.magic = kSlotStateMagic;
    hdr.version = kSlotStateVersion;
    hdr.precision = m.f16 ? 16 : 32;
    hdr.R = m.R;
    hdr.numLayers = m.numLayers;
    hdr.maxDilation = m.maxDilation;
    hipLaunchKernelGGL(prefill_finish_kernel, dim3(8, count), dim3(256), 0, stream, (const PrefillJob*)dev, hdr, rowB, m.A);
    return hipGetLastError() == hipSuccess && ok;
}

}  // namespace wn
