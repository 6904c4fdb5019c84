// slots_mel.hip -- the per-step kernels of mel columns in slot mode (slots_mel.hpp): descriptor updates, the frame gather, the
// upsampling, the placement into window rows.  Compiled once, both precisions.
#include "slots_mel.hpp"
#include "wn_kernels.hpp"

namespace wn {

__global__ __launch_bounds__(256) void slot_mel_apply_kernel(MelDesc* __restrict__ desc, const MelUpdate* __restrict__ upd, int nUpd) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nUpd; i += gridDim.x * blockDim.x) desc[upd[i].column] = upd[i].d;
}

// Frame gather.  One workgroup per (listed tile, TB stage frames) or (listed tile, SB samples), the 16 columns' descriptors in LDS.
// Stage frame q of column b is its frame (counter - start_b) / stride + q - (m - 1): the frames its first upsampled frame and the
// m - 1 before it read.  The first kind converts them as pack_features_kernel converts a mel tensor (through fp32 to T_data, zero for
// channels >= nCond, frames < 0 and frames not available) into an LDS image of the fragments, written as 16-byte pieces; its task 0
// also writes each column's placement (colInfo: phase of its first sample, samples of the step it may store -- 0 for other columns).
// The second kind writes the selectors of the mel columns' lanes, philox_selector(seed, {k, uid}) for local samples k below
// frames x stride, 0.5 past them (as slot_feed_kernel past an utterance's length).
template <bool F16>
__global__ __launch_bounds__(256) void slot_mel_stage_kernel(typename Prec<F16>::elem* __restrict__ stage, float* __restrict__ sel,
                                                             int2* __restrict__ colInfo, const MelDesc* __restrict__ desc,
                                                             const int* __restrict__ tileList, int nTiles, int maxBatch, int nCond, int stride,
                                                             int m, int nq, long long counter, int T, int W, int count, unsigned key0,
                                                             unsigned key1) {
    using elem = typename Prec<F16>::elem;
    constexpr int KFC = feat_kfc<F16>(), TPF = Prec<F16>::TPF, EPL = Prec<F16>::EPL, KC = KFC * 16 * TPF, TB = 8, SB = 64;
    __shared__ __attribute__((aligned(16))) elem img[TB * KFC * 64 * EPL];
    __shared__ MelDesc dl[16];
    const int tid = threadIdx.x;
    const int qblocks = (nq + TB - 1) / TB, sblocks = (count + SB - 1) / SB;
    const size_t nblk = (size_t)nTiles * (qblocks + sblocks);
    for (size_t bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
        const int ti = (int)(bi % nTiles), task = (int)(bi / nTiles), tile = tileList[ti];
        if (tid < 16) {
            const int b = tile * 16 + tid;
            if (b < maxBatch) dl[tid] = desc[b];
            else dl[tid].state = 0;
        }
        __syncthreads();
        if (task < qblocks) {
            const int q0 = task * TB;
            for (int i = tid; i < 16 * KC * TB; i += 256) {
                const int tt = i % TB, c = (i / TB) % KC, j = i / (TB * KC);
                const MelDesc& d = dl[j];
                float v = 0.f;
                if (d.state && c < nCond && q0 + tt < nq) {
                    const long long f = (counter - d.start) / stride + q0 + tt - (m - 1);
                    if (f >= 0 && f < d.frames) {
                        const long long at = c * d.cStride + f * d.fStride;
                        v = d.precision == 16 ? (float)((const _Float16*)d.mel)[at] : ((const float*)d.mel)[at];
                    }
                }
                const int kf = c / (16 * TPF), tk = (c / 16) % TPF, g = (c % 16) / 4, r = c % 4;
                img[((tt * KFC + kf) * 64 + g * 16 + j) * EPL + tk * 4 + r] = (elem)v;
            }
            if (task == 0 && tid < 16) {
                const MelDesc& d = dl[tid];
                int2 ci = make_int2(0, 0);
                if (d.state) {
                    const long long kLo = counter - d.start, lim = (long long)d.frames * stride - kLo;
                    ci.x = (int)(kLo % stride);
                    ci.y = (int)(lim < count ? lim : count);
                }
                colInfo[ti * 16 + tid] = ci;
            }
            __syncthreads();
            for (int pi = tid; pi < TB * KFC * 64; pi += 256) {
                const int tt = pi / (KFC * 64), rem = pi % (KFC * 64);
                if (q0 + tt < nq)
                    *(uintx4*)(stage + (((size_t)(q0 + tt) * nTiles + ti) * KFC * 64 + rem) * EPL) = *(const uintx4*)(img + (size_t)pi * EPL);
            }
        } else {
            const int s0 = (task - qblocks) * SB;
            for (int i = tid; i < 16 * SB; i += 256) {
                const int j = i % 16, t = s0 + i / 16, b = tile * 16 + j;
                const MelDesc& d = dl[j];
                if (!d.state || t >= count || b >= maxBatch) continue;
                const long long k = counter + t - d.start;
                const float s = (k >= 0 && k < (long long)d.frames * stride) ? philox_selector(key0, key1, (unsigned)k, d.uid) : 0.5f;
                sel[(size_t)((T + t) % W) * maxBatch + b] = s;
            }
        }
        __syncthreads();      // (img and dl are rewritten by the next task)
    }
}

// Upsampling: upsample_features_kernel with columns of one tile at different phases.  A workgroup takes a phase r (its operand A_r,
// RTU x m*KFC fragments, in LDS), a wave CB columns (stage frame q, listed tile) at a time; MFMA lane column j is column tile*16 + j
// at ITS frame (counter - start_j) / stride + q, whose B operand is stage frame q + m - 1 - tap -- a whole 1-KiB fragment read, as
// the lockstep kernel reads its mel fragments.  The accumulation is the lockstep kernel's: the bias, then taps ascending, within a
// tap kf ascending, per row tile, with the same mma.  Lane column j's result is its sample t = q*stride + r - phase_j of the step:
// every phase of a frame that straddles the step's edges is computed, and only samples t in [0, colInfo.y) are stored -- into
// `out`, the column's own record of the sample ([nTiles*16][count] records of KFC x 4 x 16 B, [kf][g] in the record), not into the
// window: the 16 columns of a tile are at 16 phases, i.e. in 16 different workgroups, and 16-byte stores of them straight into the
// window's fragments (each 128-byte line shared by 8 columns) ran at 0.46 TB/s (LABNOTES).  slot_mel_place_kernel moves the records.
template <bool F16>
__global__ __launch_bounds__(64 * up_waves<F16>()) WN_UP_ATTR void slot_mel_upsample_kernel(
    typename Prec<F16>::elem* __restrict__ feat, const typename Prec<F16>::elem* __restrict__ stage, const int2* __restrict__ colInfo,
    const int* __restrict__ tileList, int nTiles, const typename Prec<F16>::elem* __restrict__ tab, const float* __restrict__ bias, int m,
    int stride, int nf, int count) {
    using P = Prec<F16>;
    using frag = typename P::frag;
    constexpr int KFC = feat_kfc<F16>(), EPL = P::EPL, RTU = kUpRowTiles;
    constexpr int CB = up_cols<F16>(), NWU = up_waves<F16>(), NTH = 64 * NWU;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
    const int nA = RTU * m * KFC;                                     // fragments of one phase's operand
    const int ncol = nf * nTiles;
    const int ngrp = (ncol + CB - 1) / CB;
    for (int r = blockIdx.x; r < stride; r += gridDim.x) {
        __syncthreads();                                              // (the previous phase's readers are done)
        const uintx4* src = (const uintx4*)(tab + (size_t)r * nA * 64 * EPL);
        for (int i = tid; i < nA * 64; i += NTH) ((uintx4*)lds)[i] = src[i];
        __syncthreads();
        for (int grp = blockIdx.y * NWU + w; grp < ngrp; grp += gridDim.y * NWU) {
            int qcol[CB], tcol[CB];
            int2 info[CB];
#pragma unroll
            for (int c = 0; c < CB; c++) {
                const int col = grp * CB + c < ncol ? grp * CB + c : ncol - 1;      // (a partial group repeats its last column)
                qcol[c] = col / nTiles;
                tcol[c] = col % nTiles;
                info[c] = colInfo[tcol[c] * 16 + (lane & 15)];
            }
            floatx4 acc[CB][RTU];
#pragma unroll
            for (int c = 0; c < CB; c++)
#pragma unroll
                for (int tr = 0; tr < RTU; tr++) acc[c][tr] = *(const floatx4*)(bias + tr * 16 + g * 4);
            auto load_b = [&](frag (&b)[CB][KFC], const int j) {
#pragma unroll
                for (int c = 0; c < CB; c++) {
                    const char* mf = (const char*)(stage + ((size_t)(qcol[c] + m - 1 - j) * nTiles + tcol[c]) * KFC * 64 * EPL);
#pragma unroll
                    for (int kf = 0; kf < KFC; kf++) b[c][kf] = *(const frag*)(mf + ((size_t)kf * 64 + lane) * 16);
                }
            };
            auto taps = [&](const frag (&b)[CB][KFC], const int j) {
#pragma unroll
                for (int kf = 0; kf < KFC; kf++)
#pragma unroll
                    for (int tr = 0; tr < RTU; tr++) {
                        const frag a = *(const frag*)(lds + (size_t)((tr * m + j) * KFC + kf) * 1024 + (size_t)lane * 16);
#pragma unroll
                        for (int c = 0; c < CB; c++) acc[c][tr] = mma(a, b[c][kf], acc[c][tr]);
                    }
            };
            frag b0[CB][KFC], b1[CB][KFC];
            load_b(b0, 0);
            for (int j = 0; j < m; j += 2) {
                if (j + 1 < m) load_b(b1, j + 1);
                taps(b0, j);
                if (j + 1 < m) {
                    if (j + 2 < m) load_b(b0, j + 2);
                    taps(b1, j + 1);
                }
            }
#pragma unroll
            for (int c = 0; c < CB; c++) {
                const int t = qcol[c] * stride + r - info[c].x;      // sample of the step of lane column j
                if (grp * CB + c >= ncol || t < 0 || t >= info[c].y) continue;
                char* out = (char*)feat + ((size_t)(tcol[c] * 16 + (lane & 15)) * count + t) * KFC * 64 * EPL * sizeof(typename P::elem) / 16;
#pragma unroll
                for (int kf = 0; kf < KFC; kf++) {
                    frag o;
                    if constexpr (F16) {
                        const floatx4 lo = acc[c][2 * kf], hi = (2 * kf + 1 < RTU) ? acc[c][2 * kf + 1 < RTU ? 2 * kf + 1 : 0] : floatx4{0.f, 0.f, 0.f, 0.f};
                        o = half8{(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3], (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2],
                                  (_Float16)hi[3]};
                    } else {
                        o = acc[c][kf < RTU ? kf : 0];
                    }
                    *(frag*)(out + (size_t)(kf * 4 + g) * 16) = o;
                }
            }
        }
    }
}

// The records -> window rows (T + t) mod W.  One workgroup per (listed tile, TB samples): the 16 columns' records read in runs of
// TB x KFC x 64 contiguous bytes into an LDS image of the fragments, written as 16-byte pieces -- whole 1-KiB fragments where all 16
// columns of the tile are mel columns; only the lanes of mel columns and their samples below colInfo.y are written.
template <bool F16>
__global__ __launch_bounds__(256) void slot_mel_place_kernel(typename Prec<F16>::elem* __restrict__ feat, const uintx4* __restrict__ rec,
                                                             const int2* __restrict__ colInfo, const int* __restrict__ tileList, int nTiles,
                                                             int tiles, int T, int W, int count) {
    constexpr int KFC = feat_kfc<F16>(), EPL = Prec<F16>::EPL, TB = 8, NP = KFC * 4;      // 16-byte pieces of a record
    __shared__ uintx4 img[TB * KFC * 64];
    __shared__ int lim[16];
    const int tid = threadIdx.x;
    const size_t nblk = (size_t)nTiles * ((count + TB - 1) / TB);
    for (size_t bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
        const int ti = (int)(bi % nTiles), t0 = (int)(bi / nTiles) * TB;
        if (tid < 16) lim[tid] = colInfo[ti * 16 + tid].y;
        __syncthreads();
        for (int i = tid; i < 16 * TB * NP; i += 256) {
            const int p = i % NP, tt = (i / NP) % TB, j = i / (NP * TB), t = t0 + tt;
            if (t < lim[j]) img[(tt * KFC + p / 4) * 64 + (p % 4) * 16 + j] = rec[((size_t)(ti * 16 + j) * count + t) * NP + p];
        }
        __syncthreads();
        const int tile = tileList[ti];
        for (int pi = tid; pi < TB * KFC * 64; pi += 256) {
            const int tt = pi / (KFC * 64), lane = pi % 64, t = t0 + tt;
            if (t < lim[lane & 15])
                *(uintx4*)(feat + (((size_t)((T + t) % W) * tiles + tile) * KFC * 64 + pi % (KFC * 64)) * EPL) = img[pi];
        }
        __syncthreads();      // (img and lim are rewritten by the next task)
    }
}

bool slots_mel_apply(hipStream_t stream, MelDesc* desc, const MelUpdate* upd, int nUpd) {
    const int g = (nUpd + 255) / 256;
    hipLaunchKernelGGL(slot_mel_apply_kernel, dim3(g < 1 ? 1 : g > 64 ? 64 : g), dim3(256), 0, stream, desc, upd, nUpd);
    return hipGetLastError() == hipSuccess;
}

template <bool F16>
bool slots_mel_prepare() {
    // (the operand of one phase: RTU x m x KFC KiB, up to 125 KiB in fp32 at five taps)
    return hipFuncSetAttribute((const void*)slot_mel_upsample_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) ==
           hipSuccess;
}

template <bool F16>
bool slots_mel_feed(hipStream_t stream, void* feat, float* sel, void* stage, void* records, int* colInfo, const MelDesc* desc, const int* tileList,
                    int nTiles, int maxBatch, int tiles, int nCond, const void* upTab, const float* upBias, int m, int stride,
                    long long counter, int T, int W, int count, unsigned long long seed) {
    using elem = typename Prec<F16>::elem;
    constexpr int KFC = feat_kfc<F16>();
    const int nf = slots_mel_frames(count, stride), nq = nf + m - 1;
    const size_t nblk = (size_t)nTiles * ((nq + 7) / 8 + (count + 63) / 64);
    hipLaunchKernelGGL((slot_mel_stage_kernel<F16>), dim3((unsigned)(nblk > 65536 ? 65536 : nblk)), dim3(256), 0, stream, (elem*)stage, sel,
                       (int2*)colInfo, desc, tileList, nTiles, maxBatch, nCond, stride, m, nq, counter, T, W, count, (unsigned)seed,
                       (unsigned)(seed >> 32));
    if (hipGetLastError() != hipSuccess) return false;
    // grid as upsampleFeatures: a phase per workgroup (up to 1024), more workgroups per phase where phases have few columns
    const int gx = stride < 1024 ? stride : 1024;
    const long long cols = (long long)nf * nTiles;
    int gy = (int)((cols + 255) / 256);
    const int gyMax = (1024 + gx - 1) / gx;
    if (gy > gyMax) gy = gyMax;
    if (gy < 1) gy = 1;
    const size_t lds = (size_t)kUpRowTiles * m * KFC * 1024;
    hipLaunchKernelGGL((slot_mel_upsample_kernel<F16>), dim3(gx, gy), dim3(64 * up_waves<F16>()), lds, stream, (elem*)records,
                       (const elem*)stage, (const int2*)colInfo, tileList, nTiles, (const elem*)upTab, upBias, m, stride, nf, count);
    if (hipGetLastError() != hipSuccess) return false;
    const size_t nplace = (size_t)nTiles * ((count + 7) / 8);
    hipLaunchKernelGGL((slot_mel_place_kernel<F16>), dim3((unsigned)(nplace > 65536 ? 65536 : nplace)), dim3(256), 0, stream, (elem*)feat,
                       (const uintx4*)records, (const int2*)colInfo, tileList, nTiles, tiles, T, W, count);
    return hipGetLastError() == hipSuccess;
}

template bool slots_mel_prepare<true>();
template bool slots_mel_prepare<false>();
template bool slots_mel_feed<true>(hipStream_t, void*, float*, void*, void*, int*, const MelDesc*, const int*, int, int, int, int, const void*,
                                   const float*, int, int, long long, int, int, int, unsigned long long);
template bool slots_mel_feed<false>(hipStream_t, void*, float*, void*, void*, int*, const MelDesc*, const int*, int, int, int, int, const void*,
                                    const float*, int, int, long long, int, int, int, unsigned long long);

}  // namespace wn
