// slots.hip -- the per-step kernels of slot mode (slots.hpp): resetting columns, feeding the window.  Compiled once, both precisions.
#include "slots.hpp"
#include "wn_kernels.hpp"

namespace wn {

// Column reset.  blockIdx.y walks the restarted columns, x the column's share of its tile's ring: lanes 16g + j (j = column mod 16) of
// every 1-KiB fragment of every ring slot, 16-byte vector stores, 32-bit index arithmetic.  Per restarted column ringSlots x R x 16 x
// sizeof(T_data) / 16 bytes are stored (C3 fp16: 2046 slots x 2 fragments x 4 pieces x 16 B = 256 KiB) -- nothing of the other
// columns' lanes is touched.  Blocks of row 0 then write the descriptors and set the history of the restarted columns.
__global__ __launch_bounds__(256) void slot_reset_kernel(SlotDesc* __restrict__ desc, const SlotUpdate* __restrict__ upd, int nUpd,
                                                         const int* __restrict__ cols, int nCols, uintx4* __restrict__ ring,
                                                         int ringSlots, int fragsPerSlot, int* __restrict__ yInPrev,
                                                         int* __restrict__ yInCur) {
    const int per = ringSlots * fragsPerSlot * 4;                       // pieces of one column: (slot, fragment) x 4 lanes
    const size_t perTile = (size_t)ringSlots * fragsPerSlot * 64;       // 16-byte pieces of one tile's ring
    for (int c = blockIdx.y; c < nCols; c += gridDim.y) {
        const int b = cols[c];
        uintx4* const base = ring + (size_t)(b >> 4) * perTile + (b & 15);
        for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < per; r += gridDim.x * blockDim.x)
            base[(r >> 2) * 64 + (r & 3) * 16] = uintx4{0u, 0u, 0u, 0u};
    }
    if (blockIdx.y != 0) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nUpd; i += gridDim.x * blockDim.x) {
        const SlotUpdate u = upd[i];
        desc[u.column] = u.d;
        if (u.reset) {
            yInPrev[u.column] = 128;      // mu-law silence, as silence_kernel
            yInCur[u.column] = 128;
        }
    }
}

// Window feed.  One workgroup per (tile, TB samples), like pack_features_kernel: the 16 columns' descriptors in LDS, the features
// gathered into an LDS image of the fragments with the time axis innermost (a [n_cond][T] utterance is read in runs of TB
// consecutive samples), written as 16-byte pieces at window rows (T + i) mod W; the selector row beside them.  Bytes per column and
// sample: n_cond x 4 (fp32 source) or x 2 (fp16) read, KFC x 64 B written (fp16 engine, KFC = 3: 192 B; fp32, KFC = 5: 320 B), 4 B of
// selector written -- at 12 288 columns and a chunk of 256 samples, fp16 source, 0.50 GB read and 0.62 GB written.
template <bool F16>
__global__ __launch_bounds__(256) void slot_feed_kernel(typename Prec<F16>::elem* __restrict__ feat, float* __restrict__ sel,
                                                        const SlotDesc* __restrict__ desc, int cols, int maxBatch, int tiles, int tilesUsed,
                                                        int nCond, long long counter, int T, int W, int count, unsigned key0,
                                                        unsigned key1) {
    using elem = typename Prec<F16>::elem;
    constexpr int KFC = feat_kfc<F16>(), TPF = Prec<F16>::TPF, EPL = Prec<F16>::EPL, KC = KFC * 16 * TPF, TB = 8;
    __shared__ __attribute__((aligned(16))) elem img[TB * KFC * 64 * EPL];
    __shared__ SlotDesc dl[16];
    const int tid = threadIdx.x;
    const int tblocks = (count + TB - 1) / TB;
    const size_t nblk = (size_t)tilesUsed * tblocks;
    for (size_t bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
        const int tile = (int)(bi % tilesUsed), t0 = (int)(bi / tilesUsed) * TB;
        if (tid < 16) {
            const int b = tile * 16 + tid;
            if (b < cols) dl[tid] = desc[b];
            else dl[tid].active = 0;
        }
        __syncthreads();
        for (int i = tid; i < 16 * KC * TB; i += 256) {
            const int tt = i % TB, c = (i / TB) % KC, j = i / (TB * KC);
            const SlotDesc& d = dl[j];
            const long long k = counter + t0 + tt - d.start;
            float v = 0.f;
            if (d.active && c < nCond && t0 + tt < count && k >= 0 && k < d.length) {
                const long long at = c * d.cStride + k * d.tStride;
                v = d.precision == 16 ? (float)((const _Float16*)d.x)[at] : ((const float*)d.x)[at];
            }
            const int kf = c / (16 * TPF), tk = (c / 16) % TPF, g = (c % 16) / 4, r = c % 4;
            img[((tt * KFC + kf) * 64 + g * 16 + j) * EPL + tk * 4 + r] = (elem)v;
        }
        if (tid < TB * 16) {
            const int tt = tid / 16, j = tid % 16, b = tile * 16 + j;
            if (t0 + tt < count && b < maxBatch) {
                const SlotDesc& d = dl[j];
                const long long k = counter + t0 + tt - d.start;
                const float s = (d.active && k >= 0 && k < d.length) ? philox_selector(key0, key1, (unsigned)k, d.uid) : 0.5f;
                sel[(size_t)((T + t0 + tt) % W) * maxBatch + b] = s;
            }
        }
        __syncthreads();
        for (int pi = tid; pi < TB * KFC * 64; pi += 256) {
            const int tt = pi / (KFC * 64), rem = pi % (KFC * 64);
            if (t0 + tt < count) {
                const size_t row = (size_t)((T + t0 + tt) % W);
                *(uintx4*)(feat + ((row * tiles + tile) * KFC * 64 + rem) * EPL) = *(const uintx4*)(img + (size_t)pi * EPL);
            }
        }
        __syncthreads();      // (img and dl are rewritten by the next task)
    }
}

static int gridOf(size_t n, size_t cap) {
    size_t g = (n + 255) / 256;
    return (int)(g > cap ? cap : (g ? g : 1));
}

bool slots_reset(hipStream_t stream, SlotDesc* desc, const SlotUpdate* upd, int nUpd, const int* cols, int nCols, void* ring,
                 int ringSlots, int fragsPerSlot, int* yInPrev, int* yInCur) {
    const int per = ringSlots * fragsPerSlot * 4;
    const int gx = gridOf((size_t)(per > nUpd ? per : nUpd), 64), gy = nCols < 1 ? 1 : nCols > 1024 ? 1024 : nCols;
    hipLaunchKernelGGL(slot_reset_kernel, dim3(gx, gy), dim3(256), 0, stream, desc, upd, nUpd, cols, nCols, (uintx4*)ring, ringSlots,
                       fragsPerSlot, yInPrev, yInCur);
    return hipGetLastError() == hipSuccess;
}

bool slots_pcm(hipStream_t stream, const int* y, short* pcm, const short* table, int cols, int W, int t0, int count) {
    hipLaunchKernelGGL(mulaw_pcm_kernel, dim3(gridOf((size_t)cols * count, 4096)), dim3(256), 0, stream, y, pcm, table, cols, W, t0, count);
    return hipGetLastError() == hipSuccess;
}

template <bool F16>
bool slots_feed(hipStream_t stream, void* feat, float* sel, const SlotDesc* desc, int cols, int maxBatch, int tiles, int nCond,
                long long counter, int T, int W, int count, unsigned long long seed) {
    const int tilesUsed = (cols + 15) / 16;
    const size_t nblk = (size_t)tilesUsed * ((count + 7) / 8);
    hipLaunchKernelGGL((slot_feed_kernel<F16>), dim3((unsigned)(nblk > 65536 ? 65536 : nblk)), dim3(256), 0, stream,
                       (typename Prec<F16>::elem*)feat, sel, desc, cols, maxBatch, tiles, tilesUsed, nCond, counter, T, W, count,
                       (unsigned)seed, (unsigned)(seed >> 32));
    return hipGetLastError() == hipSuccess;
}

template bool slots_feed<true>(hipStream_t, void*, float*, const SlotDesc*, int, int, int, int, long long, int, int, int, unsigned long long);
template bool slots_feed<false>(hipStream_t, void*, float*, const SlotDesc*, int, int, int, int, long long, int, int, int, unsigned long long);

}  // namespace wn
