// score_carry.hip -- the kernels and the host side of scoring with carried state (score_carry.hpp): Score::chunksCheck and
// Score::runChunks.  Compiled once: the (R, S) of the built shapes, both precisions.  The head is score.hip's.
#include "score_carry.hpp"

#include <limits.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "slots_state.hpp"
#include "time_tiles.hpp"

namespace wn {

namespace {

// x_0[k] = embPrev[y(k-2)] + embCur[y(k-1)] over the chunk, k = k0 + r: score_embed_kernel's arithmetic, with y(k0 - 1) and
// y(k0 - 2) from the job (the in-state's history words; 128 from silence).  With an out-state, x_0[k0 + n - 1] goes to layer 0's one
// slot of the out blob, as prefill_embed_kernel does.  blockIdx.y: request, x: time tile.  Rows at and past n are zero.
template <bool F16>
__global__ __launch_bounds__(256) void score_carry_embed_kernel(const CarryJob* __restrict__ jobs, int R, int A, const void* __restrict__ embPrevV,
                                                                const void* __restrict__ embCurV, int tanhEmbed, float* __restrict__ xf,
                                                                char* __restrict__ xd) {
    using elem = typename Prec<F16>::elem;
    using quad = typename Prec<F16>::quad;
    const CarryJob jb = jobs[blockIdx.y];
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
            const int yc = r >= 1 ? clamp_sample(jb.y[r - 1], A) : hCur;
            const int yp = r >= 2 ? clamp_sample(jb.y[r - 2], A) : r == 1 ? hCur : hPrev;
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
        if (jb.out != nullptr && r == jb.n - 1) put_quad<F16>(jb.out + sizeof(SlotStateHeader) + quad_off<F16>(tile, g), v);      // layer 0: d = 1, one slot
    }
}

// One layer over one time tile of one chunk: score_layer_kernel's body, operand for operand.  Two differences: the dilated tap of a
// column before the chunk (r - d < 0) comes from the in-state, and x_{l+1} of the chunk's last dOut samples also goes to the out-state.
// blockIdx.y: request, x: time tile.
template <bool F16, int R, int S>
__global__ __launch_bounds__((PCfg<F16, R>::THREADS)) void score_carry_layer_kernel(const CarryJob* __restrict__ jobs, const CarryLayer ly, int first,
                                                                                    int last, const char* __restrict__ wblob, size_t waveBytes,
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

    const CarryJob jb = jobs[blockIdx.y];
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
    // + Wcond c: column r of the chunk's own features; columns past n - 1 (the padding of the last tile) repeat the last sample
    {
        frag cf[1][KFC];
        feature_frags<F16, KFC>(jb.x, jb.precision, jb.cStride, jb.tStride, r < jb.n ? r : jb.n - 1, nCond, g, cf[0]);
        gemm_direct<F16, 1, 2 * HTW, KFC>(wbase + (size_t)ly.cond * 1024, laneOff, acc, cf);
    }
    // + Wprev x_l[k - d]: a scratch row inside the chunk; before it the in-state's slot of sample k0 + r - d; zero before the
    // utterance's start and without an in-state.  One unconditional load from an address that is valid either way, then the mask.
    const char* const inJob = xdIn + jobRow * ROWB;
    {
        frag xp[1][KF_R];
        const int rp = r - ly.d, kp = jb.k0 + rp;
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
    // residual: (Bres + x) + Wres h -> x_{l+1}[k]: the running residual in fp32, the operand in T_data, and -- the chunk's last dOut
    // samples, with an out-state -- the slot of layer l + 1 that the absolute sample k owns
    if (!last) {
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
    // skip[k] (+)= Wskip_l h
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

// The out-state's rest: in every layer with d > n the slots whose residue no sample of [k0, k0 + n) has keep the in-state's bytes
// (zero from silence), and the header.  blockIdx.y: request (nothing for one without an out-state).
__global__ __launch_bounds__(256) void score_carry_finish_kernel(const CarryJob* __restrict__ jobs, SlotStateHeader hdr, int rowB, int A) {
    const CarryJob jb = jobs[blockIdx.y];
    if (jb.out == nullptr) return;
    uintx4* const out = (uintx4*)(jb.out + sizeof(SlotStateHeader));
    const uintx4* const in = (const uintx4*)(jb.in != nullptr ? jb.in + sizeof(SlotStateHeader) : nullptr);
    const int pps = rowB / 16;
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
        hdr.yInPrev = clamp_sample(jb.n >= 2 ? jb.y[jb.n - 2] : jb.yInCur, A);
        hdr.yInCur = clamp_sample(jb.y[jb.n - 1], A);
        *(SlotStateHeader*)jb.out = hdr;
    }
}

template <bool F16, int R, int S>
bool launchCarry(const ScoreModel& m, const CarryLayer* layers, const CarryJob* jobs, int count, int maxTiles, float* xf, char* xd0, char* xd1,
                 float* skf, hipStream_t stream) {
    using C = PCfg<F16, R>;
    hipLaunchKernelGGL((score_carry_embed_kernel<F16>), dim3(maxTiles, count), dim3(256), 0, stream, jobs, R, m.A, m.embPrev, m.embCur, m.tanhEmbed,
                       xf, xd0);
    if (hipGetLastError() != hipSuccess) return false;
    char* in = xd0;
    char* out = xd1;
    const int L = m.numLayers;
    for (int l = 0; l < L; l++) {
        hipLaunchKernelGGL((score_carry_layer_kernel<F16, R, S>), dim3(maxTiles, count), dim3(C::THREADS), 0, stream, jobs, layers[l], l == 0 ? 1 : 0,
                           l == L - 1 ? 1 : 0, (const char*)m.wblob, m.waveStreamFrags * 1024, m.bias + (size_t)l * m.biasL, m.nCond, xf,
                           (const char*)in, out, skf);
        if (hipGetLastError() != hipSuccess) return false;
        char* const t = in;
        in = out;
        out = t;
    }
    return true;
}

long long paddedSamples(int n) { return ((long long)n + 15) & ~15LL; }

size_t blobBytes(const ScoreModel& m) { return sizeof(SlotStateHeader) + (size_t)m.ringSlots * m.R * (m.f16 ? 2 : 4); }

// the device-side address of `bytes` of device or mapped pinned memory at p, 16-byte aligned; NULL for anything else
char* blobTarget(const void* p, size_t bytes, bool* pinned) {
    if (p == NULL || ((size_t)p & 15) != 0) return NULL;
    const int type = pointer_type(p);
    if (type != hipMemoryTypeDevice && type != hipMemoryTypeManaged && type != hipMemoryTypeHost) return NULL;
    *pinned = type == hipMemoryTypeHost;
    char* const first = (char*)store_target((void*)p);
    if (first == NULL || (char*)store_target((char*)p + bytes - 16) != first + bytes - 16) return NULL;
    return first;
}

bool headerFits(const ScoreModel& m, const SlotStateHeader& h) {
    float T, P;      // (word 10: zero, or the bits of a valid temperature; word 11: zero, or the bits of a valid probability floor)
    return h.magic == kSlotStateMagic && h.version == kSlotStateVersion && h.precision == (m.f16 ? 16 : 32) && h.R == m.R &&
           h.numLayers == m.numLayers && h.maxDilation == m.maxDilation && h.done >= 0 && temperature_of_word(h.pad[0], T) &&
           min_p_of_word(h.pad[1], P);
}

}  // namespace

bool Score::chunksCheck(const ScoreModel& m, const ScoreChunkReq* reqs, int count, bool ownX, std::vector<ScoreChunkIn>& in) {
    if (m.nCond <= 0 || reqs == NULL || count < 1 || count > 65535) return false;
    // everything the whole pass refuses
    {
        std::vector<ScoreReq> plain(count);
        for (int i = 0; i < count; i++) {
            const ScoreChunkReq& q = reqs[i];
            plain[i] = ScoreReq{q.y, q.n, q.x, q.precision, q.cStride, q.tStride, q.temperature, q.logp, q.rows};
        }
        if (!acceptable(m, plain.data(), count, ownX)) return false;
    }
    const size_t bytes = blobBytes(m);
    in.assign(count, ScoreChunkIn{NULL, NULL, 0, 0u, 128, 128});
    // the blobs' ranges: every out-state clear of every in-state and of every other out-state (equal lengths: neighbours by address)
    std::vector<std::pair<size_t, int>> spans;      // (device-side address, 1: out-state)
    std::vector<const void*> devStates;             // distinct in-states in device memory, in order of appearance
    std::vector<std::pair<const void*, SlotStateHeader>> seen;      // every distinct in-state once
    std::unordered_map<const void*, size_t> index;
    for (int i = 0; i < count; i++) {
        const ScoreChunkReq& q = reqs[i];
        if (q.state != NULL) {
            bool pinned = false;
            in[i].in = blobTarget(q.state, bytes, &pinned);
            if (in[i].in == NULL) return false;
            if (index.find(q.state) == index.end()) {
                index[q.state] = seen.size();
                SlotStateHeader h = {};
                if (pinned) memcpy(&h, q.state, sizeof(h));
                else devStates.push_back(q.state);
                seen.push_back(std::make_pair(q.state, h));
                spans.push_back(std::make_pair((size_t)in[i].in, 0));
            }
        }
        if (q.stateOut != NULL) {
            bool pinned = false;
            in[i].out = blobTarget(q.stateOut, bytes, &pinned);
            if (in[i].out == NULL) return false;
            spans.push_back(std::make_pair((size_t)in[i].out, 1));
        }
    }
    std::sort(spans.begin(), spans.end());
    for (size_t s = 1; s < spans.size(); s++)
        if (spans[s].first - spans[s - 1].first < bytes && (spans[s].second || spans[s - 1].second)) return false;
    // the headers of the device blobs: blocking copies on the null stream (a save on a non-blocking stream must have been ordered
    // before this call, as for nvw_slot_resume); an arithmetic progression inside one allocation -- the rows of one earlier call --
    // takes one 2-D copy
    if (!devStates.empty()) {
        const size_t nd = devStates.size();
        std::vector<SlotStateHeader> hdr(nd);
        bool rows = nd >= 2 && (const char*)devStates[1] > (const char*)devStates[0];
        const size_t step = rows ? (size_t)((const char*)devStates[1] - (const char*)devStates[0]) : 0;
        for (size_t s = 2; s < nd && rows; s++) rows = (const char*)devStates[s] == (const char*)devStates[0] + s * step;
        if (rows) {
            void* base = NULL;
            size_t size = 0;
            if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)devStates[0]) != hipSuccess) {
                (void)hipGetLastError();
                rows = false;
            } else {
                rows = (const char*)devStates[nd - 1] + bytes <= (const char*)base + size;
            }
        }
        if (rows) {
            gpuErrChk(hipMemcpy2D(hdr.data(), sizeof(SlotStateHeader), devStates[0], step, sizeof(SlotStateHeader), nd, hipMemcpyDeviceToHost));
        } else {
            for (size_t s = 0; s < nd; s++) gpuErrChk(hipMemcpy(&hdr[s], devStates[s], sizeof(SlotStateHeader), hipMemcpyDeviceToHost));
        }
        size_t at = 0;
        for (size_t s = 0; s < seen.size() && at < nd; s++)
            if (seen[s].first == devStates[at]) seen[s].second = hdr[at++];
    }
    for (size_t s = 0; s < seen.size(); s++)
        if (!headerFits(m, seen[s].second)) return false;
    for (int i = 0; i < count; i++) {
        const ScoreChunkReq& q = reqs[i];
        in[i].uid = q.uid;
        if (q.state == NULL) continue;
        const SlotStateHeader& h = seen[index[q.state]].second;
        if ((long long)h.done + q.n > (long long)INT_MAX - 16) return false;
        in[i].k0 = h.done;
        in[i].uid = h.uid;
        in[i].yInPrev = h.yInPrev;
        in[i].yInCur = h.yInCur;
    }
    return true;
}

bool Score::runChunks(const ScoreModel& m, const ScoreChunkReq* reqs, int count, const std::vector<ScoreChunkIn>& in, hipStream_t stream) {
    if (reqs == NULL || count < 1 || (int)in.size() != count) return false;
    CarryLayer layers[128];
    for (int l = 0, off = 0; l < m.numLayers; l++) {
        const ScoreLayer& s = m.layers[l];
        const int dN = l + 1 < m.numLayers ? m.layers[l + 1].d : 1;
        layers[l] = CarryLayer{s.cond, s.prev, s.cur, s.res, s.skip, s.d, off, dN, off + s.d};
        off += s.d;
    }
    // scratch: score.hpp's rows, [total padded samples] each
    long long total = 0;
    for (int i = 0; i < count; i++) total += paddedSamples(reqs[i].n);
    const int rowB = m.R * (m.f16 ? 2 : 4);
    const size_t cells = (size_t)total;
    char* const base = scratch(cells * score_row_bytes(m.f16, m.R, m.S));
    float* const xf = (float*)base;
    char* const xd0 = base + cells * m.R * 4;
    char* const xd1 = xd0 + cells * rowB;
    float* const skf = (float*)(xd1 + cells * rowB);
    // the requests through pinned staging, two halves used by alternate calls: [cap] CarryJob, then [cap] ScoreJob for the head
    const size_t each = sizeof(CarryJob) + sizeof(ScoreJob);
    if (count > m_chunkCap) {
        gpuErrChk(hipDeviceSynchronize());      // (an earlier call may still be using what is replaced)
        if (m_chunkJobs) gpuErrChk(hipFree(m_chunkJobs));
        m_chunkJobs = NULL;
        m_chunkCap = 0;
        gpuErrChk(hipMalloc((void**)&m_chunkJobs, 2 * (size_t)count * each));
        m_chunkStage.make(2, (size_t)count * each);
        m_chunkCap = count;
    }
    char* const dev = m_chunkJobs + (size_t)m_chunkStage.at() * m_chunkCap * each;
    char* const host = (char*)m_chunkStage.acquire();
    CarryJob* const cj = (CarryJob*)host;
    ScoreJob* const hj = (ScoreJob*)(host + (size_t)count * sizeof(CarryJob));
    int maxTiles = 0;
    bool anyOut = false;
    long long row = 0;
    for (int i = 0; i < count; i++) {
        const ScoreChunkReq& q = reqs[i];
        CarryJob& c = cj[i];
        memset(&c, 0, sizeof(c));
        c.y = q.y;
        c.x = q.x;
        c.cStride = q.cStride;
        c.tStride = q.tStride;
        c.in = in[i].in;
        c.out = in[i].out;
        c.row0 = row;
        c.n = q.n;
        c.tiles = (int)(paddedSamples(q.n) / 16);
        c.precision = q.precision;
        c.k0 = in[i].k0;
        c.uid = in[i].uid;
        c.temp = temperature_word(q.temperature);
        c.yInPrev = in[i].yInPrev;
        c.yInCur = in[i].yInCur;
        ScoreJob& h = hj[i];
        memset(&h, 0, sizeof(h));
        h.y = q.y;
        h.logp = (float*)store_target(q.logp);
        h.rows = q.rows;
        h.row0 = row;
        h.n = q.n;
        h.tiles = c.tiles;
        h.precision = q.precision;
        h.scale = temperature_scale(q.temperature);
        row += paddedSamples(q.n);
        if (c.tiles > maxTiles) maxTiles = c.tiles;
        anyOut = anyOut || c.out != NULL;
    }
    gpuErrChk(hipMemcpyAsync(dev, host, (size_t)count * each, hipMemcpyHostToDevice, stream));
    m_chunkStage.release(stream);
    const CarryJob* const devCarry = (const CarryJob*)dev;
    const ScoreJob* const devHead = (const ScoreJob*)(dev + (size_t)count * sizeof(CarryJob));

    bool ok = false;
#define WN_CARRY_CASE(RR, SS, AA)                                                                                              \
    if (m.R == RR && m.S == SS && m.A == AA)                                                                                   \
        ok = m.f16 ? launchCarry<true, RR, SS>(m, layers, devCarry, count, maxTiles, xf, xd0, xd1, skf, stream)                \
                   : launchCarry<false, RR, SS>(m, layers, devCarry, count, maxTiles, xf, xd0, xd1, skf, stream);
    WN_SCORE_SHAPES(WN_CARRY_CASE)
#undef WN_CARRY_CASE
    if (!ok) return false;
    if (anyOut) {
        SlotStateHeader hdr = {};
        hdr.magic = kSlotStateMagic;
        hdr.version = kSlotStateVersion;
        hdr.precision = m.f16 ? 16 : 32;
        hdr.R = m.R;
        hdr.numLayers = m.numLayers;
        hdr.maxDilation = m.maxDilation;
        hipLaunchKernelGGL(score_carry_finish_kernel, dim3(8, count), dim3(256), 0, stream, devCarry, hdr, rowB, m.A);
        if (hipGetLastError() != hipSuccess) return false;
    }
    return score_launch_head(m, devHead, count, maxTiles, skf, stream);
}

}  // namespace wn
