// time_kernels.hpp -- the kernels of the time-parallel pass (time_pass.hpp) and their launches: the embedding, one layer, the blob
// step.  The kernels read the engine's own weight streams (with Wcond in every layer's part, the gate rows pre-scaled) and bias
// table (with bcond added) at positions from Cfg (TimeModel): there is no second copy of the model.  Sums go in the engine's order
// with the engine's own device functions (mma, gemm_direct, gate4, tanh_t, lds_put_tile's rounding), and one column of an MFMA's
// result does not depend on what the other fifteen hold.  Included by the objects that instantiate them (prefill.hip,
// score_carry.hip); every object gets its own copies, hence the unnamed namespace.
#pragma once

#include "time_pass.hpp"
#include "time_tiles.hpp"

namespace wn {

namespace {

// x_0[k] = embPrev[y(k-2)] + embCur[y(k-1)] over the chunk, k = k0 + r, tanh when the model says so: the embedding of wavenet_wg.
// y(k0 - 1) and y(k0 - 2) are read from in front of y where the job says they lie there, else they are the job's history words.
// With an out-state, x_0[k0 + n - 1] also goes to layer 0's one slot (d = 1) of the out blob.  blockIdx.y: request, x: time tile.
// Rows at and past n (the padding of the last tile) are zero.
template <bool F16>
__global__ __launch_bounds__(256) void time_embed_kernel(const TimeJob* __restrict__ jobs, int R, int A, const void* __restrict__ embPrevV,
                                                         const void* __restrict__ embCurV, int tanhEmbed, float* __restrict__ xf,
                                                         char* __restrict__ xd) {
    using elem = typename Prec<F16>::elem;
    using quad = typename Prec<F16>::quad;
    const TimeJob jb = jobs[blockIdx.y];
    const int tile0 = blockIdx.x;
    if (tile0 >= jb.tiles) return;
    const elem* const embPrev = (const elem*)embPrevV;
    const elem* const embCur = (const elem*)embCurV;
    const int rowB = R * (int)sizeof(elem), quads = R / 4;
    const int hCur = clamp_sample(jb.yInCur, A), hPrev = clamp_sample(jb.yInPrev, A);
    for (int it = threadIdx.x; it < 16 * quads; it += blockDim.x) {
        const int q = it % quads, r = tile0 * 16 + it / quads;
        const int tile = q >> 2, g = q & 3;
        floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
        if (r < jb.n) {
            const int yc = r + jb.yBefore >= 1 ? clamp_sample(jb.y[r - 1], A) : hCur;
            const int yp = r + jb.yBefore >= 2 ? clamp_sample(jb.y[r - 2], A) : r == 1 ? hCur : hPrev;
            const floatx4 ep = quad_to_f32(*(const quad*)(embPrev + (size_t)yp * R + q * 4));
            const floatx4 ec = quad_to_f32(*(const quad*)(embCur + (size_t)yc * R + q * 4));
            v = ep + ec;
            if (tanhEmbed) {
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = tanh_t<F16>(v[e]);
            }
        }
        const size_t row = (size_t)jb.row0 + r;
        *(floatx4*)(xf + row * R + q * 4) = v;
        put_quad<F16>(xd + row * rowB + quad_off<F16>(tile, g), v);
        if (jb.out != nullptr && r == jb.n - 1) put_quad<F16>(jb.out + sizeof(SlotStateHeader) + quad_off<F16>(tile, g), v);
    }
}

// One layer over one time tile of one request: gate pre-activation (bias, conditioning, dilated tap, current tap, k ascending), gate,
// residual as (Bres + x) then Wres h, skip.  The waves split the output rows as in wavenet_wg and exchange h through LDS.  Scratch
// rows are laid out as blob slots are, so a B operand is one 16-byte load per lane and fragment at any per-lane sample offset: taps
// with d < 16 straddle two time tiles for free.
//   S > 0: the skip GEMM on the h fragments, skip[k] (+)= Wskip_l h, into an fp32 sum in the scratch that the same lane reads and
//          writes; first: the sum starts here (from zero).  S = 0: no skip path.
//   IN:    the dilated tap of a column before the chunk (r - d < 0) comes from the job's in-state, where it has one.  Without the
//          switch that tap is zero -- a prefill window's edge -- and the job's in-state is not looked at.
// With an out-state, x_{l+1} of the chunk's last dOut samples also goes to it.
//   last: no residual (the last layer's is part of no ring and feeds nothing; without the skip path that layer is not launched).
// blockIdx.y: request, x: time tile.
template <bool F16, int R, int S, bool IN>
__global__ __launch_bounds__((PCfg<F16, R>::THREADS)) void time_layer_kernel(const TimeJob* __restrict__ jobs, const TimeLayer ly, int first, int last,
                                                                             const char* __restrict__ wblob, size_t waveBytes,
                                                                             const float* __restrict__ bl, int nCond, float* __restrict__ xf,
                                                                             const char* __restrict__ xdIn, char* __restrict__ xdOut,
                                                                             float* __restrict__ skf) {
    using C = PCfg<F16, R>;
    using P = Prec<F16>;
    using frag = typename P::frag;
    constexpr int NW = C::NW, HTW = C::HTW, KF_R = C::KF_R, KFC = C::KFC, RT = C::RT, ROWB = C::ROWB;
    constexpr int STW = S / 16 / NW;
    static_assert((S / 16) % NW == 0, "skip tiles must split evenly over the waves");
    __shared__ __attribute__((aligned(16))) char hbuf[KF_R * 1024];

    const TimeJob jb = jobs[blockIdx.y];
    if ((int)blockIdx.x >= jb.tiles) return;      // (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const int r = blockIdx.x * 16 + j;            // this lane's column: sample k0 + r
    const unsigned laneOff = (unsigned)lane * 16u;
    const char* const wbase = wblob + (size_t)w * waveBytes;
    const size_t jobRow = (size_t)jb.row0;

    // gate bias
    floatx4 acc[1][2 * HTW];
#pragma unroll
    for (int i = 0; i < HTW; i++) {
        acc[0][2 * i] = *(const floatx4*)(bl + (w + NW * i) * 16 + g * 4);
        acc[0][2 * i + 1] = *(const floatx4*)(bl + (w + NW * i + RT) * 16 + g * 4);
    }
    // + Wcond c: column r of the chunk's features as B fragments, straight from the caller's tensor; columns past n - 1 (the padding
    // of the last tile) repeat the last sample
    {
        frag cf[1][KFC];
        feature_frags<F16, KFC>(jb.x, jb.precision, jb.cStride, jb.tStride, r < jb.n ? r : jb.n - 1, nCond, g, cf[0]);
        gemm_direct<F16, 1, 2 * HTW, KFC>(wbase + (size_t)ly.cond * 1024, laneOff, acc, cf);
    }
    // + Wprev x_l[k - d]: a scratch row inside the chunk; before it the in-state's slot of sample k0 + r - d; zero before the
    // utterance's start and without an in-state
    const char* const inJob = xdIn + jobRow * ROWB;
    {
        frag xp[1][KF_R];
        const int rp = r - ly.d;
        if constexpr (IN) {
            // one unconditional load from an address that is valid either way, then the mask
            const int kp = jb.k0 + rp;
            const bool inChunk = rp >= 0, inState = !inChunk && jb.in != nullptr && kp >= 0;
            const char* src = inJob + (size_t)(inChunk ? rp : r) * ROWB;
            if (inState) src = jb.in + sizeof(SlotStateHeader) + (size_t)(ly.off + (kp & (ly.d - 1))) * ROWB;
            const bool live = inChunk || inState;
#pragma unroll
            for (int kf = 0; kf < KF_R; kf++) {
                frag v = *(const frag*)(src + (kf * 4 + g) * 16);
                if (!live) v = frag{};
                xp[0][kf] = v;
            }
        } else {
#pragma unroll
            for (int kf = 0; kf < KF_R; kf++) {
                frag v = {};
                if (rp >= 0) v = *(const frag*)(inJob + (size_t)rp * ROWB + (kf * 4 + g) * 16);
                xp[0][kf] = v;
            }
        }
        gemm_direct<F16, 1, 2 * HTW, KF_R>(wbase + (size_t)ly.prev * 1024, laneOff, acc, xp);
    }
    // + Wcur x_l[k]
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
    // residual: (Bres + x) + Wres h -> x_{l+1}[k]: the running residual in fp32 (read again by this lane only), the operand in T_data,
    // and -- the chunk's last dOut samples, with an out-state -- the slot of layer l + 1 that the absolute sample k owns
    if (S == 0 || !last) {
        float* const xrow = xf + (jobRow + r) * R;
        floatx4 xa[1][HTW];
#pragma unroll
        for (int i = 0; i < HTW; i++)
            xa[0][i] = *(const floatx4*)(bl + 2 * R + (w + NW * i) * 16 + g * 4) + *(const floatx4*)(xrow + (w + NW * i) * 16 + g * 4);
        gemm_direct<F16, 1, HTW, KF_R>(wbase + (size_t)ly.res * 1024, laneOff, xa, hb);
        char* const orow = xdOut + (jobRow + r) * ROWB;
        const bool ring = jb.out != nullptr && r < jb.n && r >= jb.n - ly.dOut;
        char* const slot = jb.out + sizeof(SlotStateHeader) + (size_t)(ly.offOut + ((jb.k0 + r) & (ly.dOut - 1))) * ROWB;
#pragma unroll
        for (int i = 0; i < HTW; i++) {
            const int tile = w + NW * i;
            *(floatx4*)(xrow + tile * 16 + g * 4) = xa[0][i];
            put_quad<F16>(orow + quad_off<F16>(tile, g), xa[0][i]);
            if (ring) put_quad<F16>(slot + quad_off<F16>(tile, g), xa[0][i]);
        }
    }
    // skip[k] (+)= Wskip_l h: the engine's accumulator, kept in memory between the layers (fp32: nothing is rounded on the way)
    if constexpr (S > 0) {
        float* const srow = skf + (jobRow + r) * S;
        floatx4 sk[1][STW];
#pragma unroll
        for (int i = 0; i < STW; i++) {
            floatx4 v = floatx4{0.f, 0.f, 0.f, 0.f};
            if (!first) v = *(const floatx4*)(srow + (w + NW * i) * 16 + g * 4);
            sk[0][i] = v;
        }
        gemm_direct<F16, 1, STW, KF_R>(wbase + (size_t)ly.skip * 1024, laneOff, sk, hb);
#pragma unroll
        for (int i = 0; i < STW; i++) *(floatx4*)(srow + (w + NW * i) * 16 + g * 4) = sk[0][i];
    }
}

// The out-state's rest: in every layer with d > n the slots whose residue no sample of [k0, k0 + n) has keep the in-state's bytes
// (zero without one), and the header.  blockIdx.y: request (nothing for one without an out-state).
template <bool F16>
__global__ __launch_bounds__(256) void time_finish_kernel(const TimeJob* __restrict__ jobs, SlotStateHeader hdr, int A) {
    const TimeJob jb = jobs[blockIdx.y];
    if (jb.out == nullptr) return;
    uintx4* const out = (uintx4*)(jb.out + sizeof(SlotStateHeader));
    const uintx4* const in = (const uintx4*)(jb.in != nullptr ? jb.in + sizeof(SlotStateHeader) : nullptr);
    const int pps = hdr.R * (int)sizeof(typename Prec<F16>::elem) / 16;      // 16-byte pieces of a slot
    Dil dl = dil_first();
    for (int l = 0; l < hdr.numLayers; l++) {
        if (dl.d > jb.n) {
            const int cnt = dl.d * pps;
            for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
                const int q = i / pps;                                      // the slot's residue
                if (((q - jb.k0) & (dl.d - 1)) >= jb.n) {                   // no k in [k0, k0 + n) with k mod d = q
                    const int at = dl.off * pps + i;
                    uintx4 v = uintx4{0u, 0u, 0u, 0u};
                    if (in != nullptr) v = in[at];
                    out[at] = v;
                }
            }
        }
        dl = dil_next(dl, hdr.maxDilation, false);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr.done = jb.k0 + jb.n;
        hdr.uid = jb.uid;
        hdr.pad[0] = jb.temp;
        hdr.yInPrev = clamp_sample(jb.n >= 2 ? jb.y[jb.n - 2] : jb.yInCur, A);      // (a prefill window with t0 > 0 has n >= W > 2)
        hdr.yInCur = clamp_sample(jb.y[jb.n - 1], A);
        *(SlotStateHeader*)jb.out = hdr;
    }
}

// The embedding, the layers and -- when some job has an out-state -- the blob step of `count` jobs (at most maxTiles time
// tiles each): every layer with the skip path, all but the last without.  false: a rejected launch.
template <bool F16, int R, int S, bool IN>
bool time_launch(const TimeModel& m, const TimeJob* jobs, int count, int maxTiles, bool anyOut, const TimeScratch& sc, hipStream_t stream) {
    using C = PCfg<F16, R>;
    hipLaunchKernelGGL((time_embed_kernel<F16>), dim3(maxTiles, count), dim3(256), 0, stream, jobs, R, m.A, m.embPrev, m.embCur, m.tanhEmbed, sc.xf,
                       sc.xd0);
    if (hipGetLastError() != hipSuccess) return false;
    char* in = sc.xd0;
    char* out = sc.xd1;
    const int L = m.numLayers, launched = S > 0 ? L : L - 1;
    for (int l = 0; l < launched; l++) {
        hipLaunchKernelGGL((time_layer_kernel<F16, R, S, IN>), dim3(maxTiles, count), dim3(C::THREADS), 0, stream, jobs, m.layers[l],
                           l == 0 ? 1 : 0, l == L - 1 ? 1 : 0, (const char*)m.wblob, m.waveStreamFrags * 1024, m.bias + (size_t)l * m.biasL, m.nCond,
                           sc.xf, (const char*)in, out, sc.skf);
        if (hipGetLastError() != hipSuccess) return false;
        char* const t = in;
        in = out;
        out = t;
    }
    if (anyOut) hipLaunchKernelGGL(time_finish_kernel<F16>, dim3(8, count), dim3(256), 0, stream, jobs, time_blob_header(m), m.A);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

}  // namespace wn
