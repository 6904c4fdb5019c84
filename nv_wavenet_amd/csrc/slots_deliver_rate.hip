// slots_deliver_rate.hip -- the kernel that delivers a step's PCM at the caller's rate (slots_deliver_rate.hpp).  Compiled once,
// both precisions: fp32 throughout, the window's samples become PCM through the table at the staging, the sums int16 at the store.
#include "slots_deliver_rate.hpp"

#include "resample.hpp"

namespace wn {

namespace {

// PCM of local sample first + rel of the piece's utterance, rel in [-H, n): the window from the piece's first sample on, the old
// tail below it; zero below the utterance's sample 0
__device__ __forceinline__ short rate_input(const RateLaunch& a, const RatePiece& pc, const int* row, const short* tin, long long rel) {
    if (pc.first + rel < 0) return 0;
    if (rel >= 0) {
        int t = a.T + (int)rel;      // (n <= W: one wrap at the most)
        if (t >= a.W) t -= a.W;
        return a.table[row[t]];
    }
    return (pc.flags & kRateZeroTail) ? (short)0 : tin[a.H + rel];
}

// G, CH: as resample_tile_gemm (resample_core.hpp)
template <int G, int CH>
__global__ __launch_bounds__(kResampleThreads) void slot_deliver_rate_kernel(const RateLaunch a) {
    extern __shared__ __attribute__((aligned(16))) float span[];
    const int tid = threadIdx.x;
    const int hop = a.t.hop, spare = a.t.spare, H = a.H;

    // this workgroup's piece by bisection of the first tiles, and its tile of it
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.pieces[mid].tile0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const RatePiece pc = a.pieces[lo];
    const int ti = blockIdx.x - pc.tile0;
    const int* const row = a.y + (size_t)pc.slot * a.W;
    const short* const tin = a.tailIn + (size_t)pc.tailRow * H;

    // the new tail: local samples first + n - H .. first + n - 1, into the other image
    if (ti == 0) {
        short* const tout = a.tailOut + (size_t)pc.tailRow * H;
        for (int j = tid; j < H; j += kResampleThreads) tout[j] = rate_input(a, pc, row, tin, (long long)pc.n - H + j);
    }
    if (pc.blocks == 0) return;      // (the whole workgroup: a piece without outputs)

    // its blocks of the range: ti * 16 G + (0 .. live), and the span that they read: inputs i0 + (0 .. span_n)
    const int left = pc.blocks - ti * 16 * G, live = left < 16 * G ? left : 16 * G;
    const long long blk0 = pc.block0 + (long long)ti * 16 * G;
    const long long i0 = blk0 * hop + a.t.j0;
    const int span_n = (live - 1) * hop + 16 * a.t.nq;
    for (int l = tid; l < span_n; l += kResampleThreads) {
        // (below first - H: read only by outputs below m0, which are not stored; from first + n on: zero when finished, else read
        // only by outputs from m0 + count on)
        const long long rel = i0 + l - pc.first;
        span[l + spare * (l / hop)] = rel >= -H && rel < pc.n ? (float)rate_input(a, pc, row, tin, rel) : 0.f;
    }
    __syncthreads();

    short* const out = a.pcm + pc.offset;
    resample_tile_gemm<G, CH>(span, a.t, live, [&](int col, int p, float v) {
        const long long o = (blk0 + col) * a.t.Q - pc.m0 + p;
        if (o >= 0 && o < pc.count) out[o] = resample_pcm16(v);
    });
}

struct RatePrepare {
    template <int G, int CH> bool run() const {
        if (hipFuncSetAttribute((const void*)slot_deliver_rate_kernel<G, CH>, hipFuncAttributeMaxDynamicSharedMemorySize, kResampleLdsMax) ==
            hipSuccess)
            return true;
        (void)hipGetLastError();
        return false;
    }
};
struct RateRun {
    const RateLaunch& a;
    size_t lds;
    hipStream_t stream;
    template <int G, int CH> bool run() const {
        hipLaunchKernelGGL((slot_deliver_rate_kernel<G, CH>), dim3(a.tiles), dim3(kResampleThreads), lds, stream, a);
        return hipGetLastError() == hipSuccess;
    }
};

}  // namespace

bool slots_deliver_rate_prepare(int groups, int ch) { return resample_dispatch(groups, ch, RatePrepare{}); }

bool slots_deliver_rate(hipStream_t stream, const RateLaunch& a, int groups, int ch, size_t ldsBytes) {
    if (a.count <= 0) return true;
    if (a.tiles < a.count || a.pcm == NULL || a.T < 0 || a.T >= a.W || ldsBytes > (size_t)kResampleLdsMax) return false;
    return resample_dispatch(groups, ch, RateRun{a, ldsBytes, stream});
}

}  // namespace wn
