// mel_time.hip -- the kernel and the host side of wn::MelTime (mel_time.hpp).  Compiled once, both precisions.
#include "mel_time.hpp"

#include <string.h>

#include <vector>

#include "time_tiles.hpp"

namespace wn {

namespace {

constexpr int kMelTimeWaves = 4;
// Up to this many column groups per phase the operand is read straight from the table (L2), above it from LDS (LABNOTES.md,
// "Prefill and scoring from mel"; -DWN_MELTIME_DIRECT_GROUPS=0 / =1000000000 build the two extremes for a measurement).
#ifndef WN_MELTIME_DIRECT_GROUPS
#define WN_MELTIME_DIRECT_GROUPS kMelTimeWaves
#endif

// B fragments of one frame of this lane's column (channels 4g .. of every 16), converted as pack_features_kernel and
// slot_mel_stage_kernel convert frames: through fp32 to T_data, zero for channels >= nCond and for a frame that does not count
// (counts: all ones or zero).
// The loads are unconditional (a channel past the last reads the last) so that a frame is one batch of loads.
template <bool F16, typename T>
WN_DEV void mel_frags(const T* __restrict__ frame, const long long cStride, const unsigned counts, const int nCond, const int g,
                      typename Prec<F16>::frag (&b)[feat_kfc<F16>()]) {
    using P = Prec<F16>;
#pragma unroll
    for (int kf = 0; kf < feat_kfc<F16>(); kf++)
#pragma unroll
        for (int e = 0; e < P::EPL; e++) {
            const int c = (kf * P::TPF + (e >> 2)) * 16 + 4 * g + (e & 3);
            const float v = (float)frame[(c < nCond ? c : nCond - 1) * cStride];
            // (the zero as a bit mask in a vector register: 24 compare masks held over the tap loop cost scalar registers)
            const unsigned keep = (unsigned)((c - nCond) >> 31) & counts;
            b[kf][e] = (typename P::elem)__uint_as_float(__float_as_uint(v) & keep);
        }
}

// One group of 16 columns at phase r: lane column j is column grp * 16 + j of the call, i.e. frame f of one request; its sample
// f * stride + r is stored when it lies in the request's range.  The operand A_r is read from LDS (LDSA) or from the table itself.
template <bool F16, bool LDSA>
WN_DEV void mel_time_group(const MelTimeJob* __restrict__ jobs, const int count, const int ncol, const int grp, const int r,
                           const char* __restrict__ aR, const float* __restrict__ bias, const int m, const int stride, const int nCond,
                           const int lane) {
    using P = Prec<F16>;
    using frag = typename P::frag;
    using elem = typename P::elem;
    constexpr int KFC = feat_kfc<F16>(), RTU = kUpRowTiles;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int g = lane >> 4;
    const int rt = (nCond + 15) >> 4, row = rt * 16;
    // this lane's column (a partial group repeats the last column), its request by bisection of the first columns
    const bool live = grp * 16 + (lane & 15) < ncol;
    const int col = live ? grp * 16 + (lane & 15) : ncol - 1;
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].col0 <= col) lo = mid;
        else hi = mid - 1;
    }
    const MelTimeJob jb = jobs[lo];
    const int f = jb.f0 + (col - jb.col0);

    floatx4 acc[RTU];
#pragma unroll
    for (int tr = 0; tr < RTU; tr++) acc[tr] = *(const floatx4*)(bias + tr * 16 + g * 4);
    auto load_b = [&](frag (&b)[KFC], const int j) {
        const int fj = f - j;                           // (frames before the first contribute nothing)
        const long long at = (long long)(fj < 0 ? 0 : fj) * jb.fStride;
        if (jb.precision == 16) mel_frags<F16, _Float16>((const _Float16*)jb.mel + at, jb.cStride, ~(unsigned)(fj >> 31), nCond, g, b);
        else mel_frags<F16, float>((const float*)jb.mel + at, jb.cStride, ~(unsigned)(fj >> 31), nCond, g, b);
    };
    auto taps = [&](const frag (&b)[KFC], const int j) {
#pragma unroll
        for (int kf = 0; kf < KFC; kf++)
#pragma unroll
            for (int tr = 0; tr < RTU; tr++) {
                const size_t at = (size_t)((tr * m + j) * KFC + kf) * 1024 + (size_t)lane * 16;
                frag a;
                if constexpr (LDSA) a = *(const frag*)(lds + at);
                else a = *(const frag*)(aR + at);
                acc[tr] = mma(a, b[kf], acc[tr]);
            }
    };
    for (int j = 0; j < m; j++) {
        frag b[KFC];
        load_b(b, j);
        taps(b, j);
    }
    const int t = f * stride + r;
    if (!live || t < jb.a || t >= jb.b) return;
    char* const out = jb.dst + ((size_t)(t - jb.a) * row + 4 * g) * sizeof(elem);
#pragma unroll
    for (int tr = 0; tr < RTU; tr++)
        if (tr < rt) put_quad<F16>(out + tr * 16 * sizeof(elem), acc[tr]);
}

// LDSA: a workgroup takes a phase (blockIdx.x, looping), its operand in LDS as in the lockstep kernel, its waves share the phase's
// column groups with the other workgroups of the phase (blockIdx.y).  !LDSA: a wave takes a phase (looping) of the group blockIdx.y, the operand's
// fragments straight from the table (L2): where a phase has no more groups than a workgroup has waves, no fragment is read twice.
template <bool F16, bool LDSA>
__global__ __launch_bounds__(64 * kMelTimeWaves) void mel_time_upsample_kernel(const MelTimeJob* __restrict__ jobs, int count, int ncol,
                                                                              const typename Prec<F16>::elem* __restrict__ tab,
                                                                              const float* __restrict__ bias, int m, int stride, int nCond) {
    constexpr int KFC = feat_kfc<F16>(), EPL = Prec<F16>::EPL, NWU = kMelTimeWaves, NTH = 64 * NWU;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nA = kUpRowTiles * m * KFC;                             // fragments of one phase's operand
    const int ngrp = (ncol + 15) / 16;
    if constexpr (LDSA) {
        extern __shared__ __attribute__((aligned(16))) char lds[];
        for (int r = blockIdx.x; r < stride; r += gridDim.x) {
            __syncthreads();                                          // (the previous phase's readers are done)
            const uintx4* src = (const uintx4*)(tab + (size_t)r * nA * 64 * EPL);
            for (int i = tid; i < nA * 64; i += NTH) ((uintx4*)lds)[i] = src[i];
            __syncthreads();
            for (int grp = blockIdx.y * NWU + w; grp < ngrp; grp += gridDim.y * NWU)
                mel_time_group<F16, true>(jobs, count, ncol, grp, r, NULL, bias, m, stride, nCond, lane);
        }
    } else {
        for (int r = blockIdx.x * NWU + w; r < stride; r += gridDim.x * NWU)
            mel_time_group<F16, false>(jobs, count, ncol, blockIdx.y, r, (const char*)(tab + (size_t)r * nA * 64 * EPL), bias, m, stride, nCond, lane);
    }
}

template <bool F16>
bool launchMelTime(const MelTimeModel& md, const MelTimeJob* jobs, int count, int ncol, hipStream_t stream, bool& ldsReady) {
    using elem = typename Prec<F16>::elem;
    constexpr int NWU = kMelTimeWaves;
    const int m = md.window / md.stride, ngrp = (ncol + 15) / 16;
    if (ngrp <= WN_MELTIME_DIRECT_GROUPS && ngrp <= 65535) {
        // a group per blockIdx.y, a phase per wave; about 1024 workgroups (the grid loops over the phases beyond)
        const int gxAll = (md.stride + NWU - 1) / NWU, gxMax = (1024 + ngrp - 1) / ngrp;
        hipLaunchKernelGGL((mel_time_upsample_kernel<F16, false>), dim3(gxAll < gxMax ? gxAll : gxMax, ngrp), dim3(64 * NWU), 0, stream, jobs, count,
                           ncol, (const elem*)md.tab, md.bias, m, md.stride, md.nCond);
        return hipGetLastError() == hipSuccess;
    }
    // (the operand of one phase: RTU x m x KFC KiB, up to 125 KiB in fp32 at five taps)
    // (per engine, hence per device: the attribute belongs to the device's copy of the kernel)
    if (!ldsReady) {
        if (hipFuncSetAttribute((const void*)mel_time_upsample_kernel<F16, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess)
            return false;
        ldsReady = true;
    }
    // a phase per workgroup (up to 1024; the grid loops), more workgroups per phase where there are few phases
    const int gx = md.stride < 1024 ? md.stride : 1024;
    int gy = (ngrp + NWU - 1) / NWU;
    const int gyMax = (1024 + gx - 1) / gx;
    if (gy > gyMax) gy = gyMax;
    const size_t lds = (size_t)kUpRowTiles * m * feat_kfc<F16>() * 1024;
    hipLaunchKernelGGL((mel_time_upsample_kernel<F16, true>), dim3(gx, gy), dim3(64 * NWU), lds, stream, jobs, count, ncol, (const elem*)md.tab,
                       md.bias, m, md.stride, md.nCond);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

MelTime::~MelTime() {
    if (m_rows) gpuErrChk(hipFree(m_rows));
    if (m_jobs) gpuErrChk(hipFree(m_jobs));
}

char* MelTime::rows(size_t bytes) {
    if (bytes > m_rowsBytes) {
        gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be using what is replaced)
        if (m_rows) gpuErrChk(hipFree(m_rows));
        m_rows = NULL;
        m_rowsBytes = 0;
        gpuErrChk(hipMalloc((void**)&m_rows, bytes));
        m_rowsBytes = bytes;
    }
    return m_rows;
}

bool MelTime::acceptable(const MelTimeModel& m, const MelTimeReq* reqs, int count, bool ownDst) {
    if (m.nCond <= 0 || m.nCond > kCondChannelsMax || m.stride <= 0 || m.window < m.stride || reqs == NULL || count < 1 || count > 65535)
        return false;
    const size_t rowB = (size_t)mel_time_row(m.nCond) * (m.f16 ? 2 : 4);
    const int taps = m.window / m.stride;
    long long cols = 0;
    for (int i = 0; i < count; i++) {
        const MelTimeReq& q = reqs[i];
        if (q.mel == NULL || (q.precision != 32 && q.precision != 16) || q.cStride <= 0 || q.fStride <= 0 || q.frames < 1 || q.first < 0 ||
            q.count < 1)
            return false;
        const long long end = (long long)q.first + q.count;
        if (end > 0x7fffffff || (long long)q.frames * m.stride < end) return false;
        // the first and the last element the kernel reads
        const int fLo = q.first / m.stride - (taps - 1) > 0 ? q.first / m.stride - (taps - 1) : 0, fHi = (int)((end - 1) / m.stride);
        const size_t eb = q.precision == 16 ? 2 : 4;
        if (!is_device_ptr((const char*)q.mel + (size_t)fLo * q.fStride * eb) ||
            !is_device_ptr((const char*)q.mel + ((size_t)(m.nCond - 1) * q.cStride + (size_t)fHi * q.fStride) * eb))
            return false;
        if (!ownDst && (q.dst == NULL || ((size_t)q.dst & 15) != 0 || !is_device_ptr(q.dst) ||
                        !is_device_ptr((const char*)q.dst + (size_t)q.count * rowB - 1)))
            return false;
        cols += fHi - q.first / m.stride + 1;
        if (cols > 0x7ffffff0) return false;
    }
    return true;
}

bool MelTime::run(const MelTimeModel& m, const MelTimeReq* reqs, int count, hipStream_t stream, bool ownDst) {
    if (!acceptable(m, reqs, count, ownDst)) return false;
    std::vector<MelTimeJob> jobs(count);
    int ncol = 0;
    for (int i = 0; i < count; i++) {
        const MelTimeReq& q = reqs[i];
        MelTimeJob& jb = jobs[i];
        memset(&jb, 0, sizeof(jb));
        jb.mel = q.mel;
        jb.cStride = q.cStride;
        jb.fStride = q.fStride;
        jb.dst = (char*)q.dst;
        jb.a = q.first;
        jb.b = q.first + q.count;
        jb.f0 = q.first / m.stride;
        jb.col0 = ncol;
        jb.precision = q.precision;
        ncol += (jb.b - 1) / m.stride - jb.f0 + 1;
    }
    if (count > m_jobCap) {
        gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be using what is replaced)
        if (m_jobs) gpuErrChk(hipFree(m_jobs));
        gpuErrChk(hipMalloc((void**)&m_jobs, 2 * (size_t)count * sizeof(MelTimeJob)));
        m_stage.make(2, (size_t)count * sizeof(MelTimeJob));
        m_jobCap = count;
    }
    // the requests through pinned staging, two halves used by alternate calls (as prefill stages its requests)
    MelTimeJob* const dev = m_jobs + (size_t)m_stage.at() * m_jobCap;
    void* const host = m_stage.acquire();
    memcpy(host, jobs.data(), (size_t)count * sizeof(MelTimeJob));
    gpuErrChk(hipMemcpyAsync(dev, host, (size_t)count * sizeof(MelTimeJob), hipMemcpyHostToDevice, stream));
    m_stage.release(stream);
    return m.f16 ? launchMelTime<true>(m, dev, count, ncol, stream, m_ldsReady) : launchMelTime<false>(m, dev, count, ncol, stream, m_ldsReady);
}

}  // namespace wn
