// score.hip -- the head kernel and the host side of wn::Score (score.hpp): the (S, A) of the built shapes, both precisions.  The
// layer kernels are score_carry.hip's.
#include "score.hpp"

#include "time_tiles.hpp"

namespace wn {

namespace {

// ---- head ------------------------------------------------------------------------------------------------------------------
constexpr int kScoreLdsMax = 80 * 1024;      // two head workgroups share a CU's 160 KiB
template <bool F16, int NW, int S, int A, int TT> struct HCfg {
    static constexpr int TPF = Prec<F16>::TPF;
    static constexpr int ST = S / 16, AT = A / 16, STW = ST / NW, ATW = AT / NW, KF_S = ST / TPF, KF_A = AT / TPF;
    static constexpr int THREADS = NW * 64;
    static constexpr int LPU = 4 * NW, RPL = A / LPU;       // softmax lanes per sample, logits per lane (as Cfg)
    static constexpr int LROW = A + 4;                      // padded logits row (floats)
    static constexpr int SKBUF = TT * KF_S * 1024, ZSBUF = TT * KF_A * 1024, LGBUF = TT * 16 * LROW * 4;
    // the logits take the place of the two exchange images (a barrier between the last zs read and the first logit write)
    static constexpr int LDS = SKBUF + ZSBUF > LGBUF ? SKBUF + ZSBUF : LGBUF;
    static constexpr bool FITS = LDS <= kScoreLdsMax && TT * ATW * 4 <= 128;      // ... and the logits' accumulators leave room for operands
};
// Time tiles of 16 samples per head workgroup: Wzs and Wza are read from L2 once per workgroup, so once per TT tiles.  Two where
// they fit (LDS, accumulators), else one; WN_SCORE_HEAD_TILES asks for 1, 2 or 4.  Measured at C3 fp16, 256 requests x 2 048
// samples, the whole pass: 10.90 / 10.46 / 10.75 ms with 1 / 2 / 4 (LABNOTES.md, "Scoring").
template <bool F16, int NW, int S, int A> constexpr int score_head_tiles() {
    constexpr int want = WN_SCORE_HEAD_TILES > 0 ? WN_SCORE_HEAD_TILES : 2;
    if constexpr (want >= 4 && HCfg<F16, NW, S, A, 4>::FITS) return 4;
    else if constexpr (want >= 2 && HCfg<F16, NW, S, A, 2>::FITS) return 2;
    else return 1;
}

// acc[bt][mt] += W(tile mt) * b[bt] with the weight fragments loaded on the spot (fragment order of gemm()) and the B fragments read
// from their LDS image as they are needed
template <bool F16, int BT, int MT, int KF>
WN_DEV void gemm_direct_ldsb(const char* src, unsigned laneOff, floatx4 (&acc)[BT][MT], const char* bimg, int lane) {
    using frag = typename Prec<F16>::frag;
    constexpr int G = MT >= 4 ? 4 : MT, UK = KF <= 16 ? KF : 8;      // (the long K loops of A = 1024 stay loops)
#pragma unroll
    for (int mg = 0; mg < MT / G; mg++)
#pragma unroll UK
        for (int kf = 0; kf < KF; kf++) {
            frag b[BT];
#pragma unroll
            for (int bt = 0; bt < BT; bt++) b[bt] = *(const frag*)(bimg + (((bt * KF + kf) * 64 + lane) << 4));
#pragma unroll
            for (int mi = 0; mi < G; mi++) {
                const frag a = *(const frag*)(src + (size_t)((mg * KF + kf) * G + mi) * 1024 + laneOff);
#pragma unroll
                for (int bt = 0; bt < BT; bt++) acc[bt][mg * G + mi] = mma(a, b[bt], acc[bt][mg * G + mi]);
            }
        }
}

constexpr float kLn2 = 0.693147180559945309417f;
// log softmax of one logit: z' - m' - log2(sum) in the exponent's units (mneg = -m * scale, as softmax_pick forms it), then * ln 2
WN_DEV float log_softmax1(float z, float scale, float mneg, float l2sum) { return (__builtin_fmaf(z, scale, mneg) - l2sum) * kLn2; }

// The head over TT time tiles of one request: relu(skip + sum of the skip biases) -> Zs = relu(Bzs + Wzs .) -> Za = Bza + Wza . ->
// log softmax(Za / T), the picked row's to logp and (when asked for) all of them to rows.  blockIdx.y: request, x: group of TT tiles.
template <bool F16, int NW, int S, int A, int TT>
__global__ __launch_bounds__((HCfg<F16, NW, S, A, TT>::THREADS)) void score_head_kernel(const TimeJob* __restrict__ jobs, const char* __restrict__ wblob,
                                                                                        size_t waveBytes, unsigned headZs, unsigned headZa,
                                                                                        const float* __restrict__ bias, int biasL, int skipBiasAt,
                                                                                        int L, const float* __restrict__ skf) {
    using H = HCfg<F16, NW, S, A, TT>;
    constexpr int STW = H::STW, ATW = H::ATW, KF_S = H::KF_S, KF_A = H::KF_A, LPU = H::LPU, RPL = H::RPL, LROW = H::LROW;
    static_assert(H::ST % NW == 0 && H::AT % NW == 0 && RPL % 4 == 0, "tiles must split evenly over the waves");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* const skbuf = lds;
    char* const zsbuf = lds + H::SKBUF;
    float* const lgbuf = (float*)lds;

    const TimeJob jb = jobs[blockIdx.y];
    const int tile0 = blockIdx.x * TT;
    if (tile0 >= jb.tiles) return;      // (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, j = lane & 15;
    const unsigned laneOff = (unsigned)lane * 16u;
    const char* const wbase = wblob + (size_t)w * waveBytes;
    const float* const headBias = bias + (size_t)L * biasL;      // Bzs[A], Bza[A]

    // relu(skip + (Bskip_0 + ... + Bskip_{L-1})): the biases summed in layer order, as wavenet_wg folds them
    floatx4 sbs[STW];
#pragma unroll
    for (int i = 0; i < STW; i++) {
        const float* const at = bias + skipBiasAt + (w + NW * i) * 16 + g * 4;
        floatx4 run = *(const floatx4*)at;
        for (int l = 1; l < L; l++) run += *(const floatx4*)(at + (size_t)l * biasL);
        sbs[i] = run;
    }
#pragma unroll
    for (int bt = 0; bt < TT; bt++) {
        // (a group's tiles past the request's last repeat it: computed, never written)
        const int tile = tile0 + bt < jb.tiles ? tile0 + bt : jb.tiles - 1;
        const float* const srow = skf + ((size_t)jb.row0 + tile * 16 + j) * S;
#pragma unroll
        for (int i = 0; i < STW; i++) {
            floatx4 v = *(const floatx4*)(srow + (w + NW * i) * 16 + g * 4) + sbs[i];
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = __builtin_fmaxf(v[r], 0.f);
            lds_put_tile<F16>(skbuf + bt * KF_S * 1024, w + NW * i, lane, v);
        }
    }
    __syncthreads();
    {
        floatx4 zs[TT][ATW];
#pragma unroll
        for (int bt = 0; bt < TT; bt++)
#pragma unroll
            for (int i = 0; i < ATW; i++) zs[bt][i] = *(const floatx4*)(headBias + (w + NW * i) * 16 + g * 4);
        gemm_direct_ldsb<F16, TT, ATW, KF_S>(wbase + (size_t)headZs * 1024, laneOff, zs, skbuf, lane);
#pragma unroll
        for (int bt = 0; bt < TT; bt++)
#pragma unroll
            for (int i = 0; i < ATW; i++) {
#pragma unroll
                for (int r = 0; r < 4; r++) zs[bt][i][r] = __builtin_fmaxf(zs[bt][i][r], 0.f);
                lds_put_tile<F16>(zsbuf + bt * KF_A * 1024, w + NW * i, lane, zs[bt][i]);
            }
    }
    __syncthreads();
    floatx4 za[TT][ATW];
#pragma unroll
    for (int bt = 0; bt < TT; bt++)
#pragma unroll
        for (int i = 0; i < ATW; i++) za[bt][i] = *(const floatx4*)(headBias + A + (w + NW * i) * 16 + g * 4);
    gemm_direct_ldsb<F16, TT, ATW, KF_A>(wbase + (size_t)headZa * 1024, laneOff, za, zsbuf, lane);
    __syncthreads();      // every wave is done with the exchange images: the logits take their place
    // logits -> LDS [sample][row] (row stride padded by 4 floats: conflict-free b128 writes)
#pragma unroll
    for (int bt = 0; bt < TT; bt++)
#pragma unroll
        for (int i = 0; i < ATW; i++) *(floatx4*)(lgbuf + (bt * 16 + j) * LROW + (w + NW * i) * 16 + g * 4) = za[bt][i];
    __syncthreads();

    // ---- log softmax: LPU lanes per sample, RPL consecutive rows per lane; maximum, exp2 and sum as softmax_pick does them ----
    const int su = tid / LPU, sq = tid % LPU;
#pragma unroll
    for (int bt = 0; bt < TT; bt++) {
        const float* const lrow = lgbuf + (bt * 16 + su) * LROW + sq * RPL;
        float m = lrow[0];
        for (int i = 0; i < RPL / 4; i++) {
            const floatx4 v = *(const floatx4*)(lrow + i * 4);
#pragma unroll
            for (int r = 0; r < 4; r++) m = __builtin_fmaxf(m, v[r]);
        }
        m = group_reduce_f<LPU>(m, [](float a, float b) { return __builtin_fmaxf(a, b); });
        const float scale = jb.scale, mneg = -m * scale;
        float lsum = 0.f;
        for (int i = 0; i < RPL / 4; i++) {
            const floatx4 v = *(const floatx4*)(lrow + i * 4);
#pragma unroll
            for (int r = 0; r < 4; r++) lsum += __builtin_amdgcn_exp2f(__builtin_fmaf(v[r], scale, mneg));
        }
        // the group's total as softmax_pick forms it: inclusive scan of the lane sums, the largest prefix sum
        float incl = lsum;
        {
            float up = dpp_f<0x111>(incl);
            if (sq >= 1) incl += up;
            up = dpp_f<0x112>(incl);
            if (sq >= 2) incl += up;
            if (LPU >= 8) {
                up = dpp_f<0x114>(incl);
                if (sq >= 4) incl += up;
            }
            if (LPU >= 16) {
                up = dpp_f<0x118>(incl);
                if (sq >= 8) incl += up;
            }
        }
        const float total = group_reduce_f<LPU>(incl, [](float a, float b) { return __builtin_fmaxf(a, b); });
        const float l2sum = __builtin_log2f(total);
        const int k = (tile0 + bt) * 16 + su;
        if (tile0 + bt < jb.tiles && k < jb.n) {      // nothing for the padding columns
            if (sq == 0) {
                const int y = clamp_sample(jb.y[k], A);
                jb.logp[k] = log_softmax1(lgbuf[(bt * 16 + su) * LROW + y], scale, mneg, l2sum);
            }
            if (jb.rows != nullptr) {
                float* const out = jb.rows + (size_t)k * A + sq * RPL;
                for (int i = 0; i < RPL / 4; i++) {
                    const floatx4 v = *(const floatx4*)(lrow + i * 4);
                    *(floatx4*)(out + i * 4) = floatx4{log_softmax1(v[0], scale, mneg, l2sum), log_softmax1(v[1], scale, mneg, l2sum),
                                                       log_softmax1(v[2], scale, mneg, l2sum), log_softmax1(v[3], scale, mneg, l2sum)};
                }
            }
        }
    }
}

constexpr int score_nw(int R) { return R / 16 >= 4 ? 4 : R / 16; }

template <bool F16, int R, int S, int A>
bool launchHead(const TimeModel& m, const TimeJob* jobs, int count, int maxTiles, const float* skf, hipStream_t stream) {
    constexpr int NW = score_nw(R), TT = score_head_tiles<F16, NW, S, A>();
    using H = HCfg<F16, NW, S, A, TT>;
    static_assert(H::FITS, "the head does not fit a CU");
    const auto head = score_head_kernel<F16, NW, S, A, TT>;
    static const bool ldsOk = hipFuncSetAttribute((const void*)head, hipFuncAttributeMaxDynamicSharedMemorySize, H::LDS) == hipSuccess;
    if (!ldsOk) return false;
    hipLaunchKernelGGL(head, dim3((maxTiles + TT - 1) / TT, count), dim3(H::THREADS), H::LDS, stream, jobs, (const char*)m.wblob,
                       m.waveStreamFrags * 1024, m.headZs, m.headZa, m.bias, m.biasL, 3 * R, m.numLayers, skf);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

bool score_launch_head(const TimeModel& m, const TimeJob* jobs, int count, int maxTiles, const float* skf, hipStream_t stream) {
    bool ok = false;
#define WN_SCORE_HEAD(RR, SS, AA)                                                                                              \
    if (m.R == RR && m.S == SS && m.A == AA)                                                                                   \
        ok = m.f16 ? launchHead<true, RR, SS, AA>(m, jobs, count, maxTiles, skf, stream)                                       \
                   : launchHead<false, RR, SS, AA>(m, jobs, count, maxTiles, skf, stream);
    WN_SCORE_SHAPES(WN_SCORE_HEAD)
#undef WN_SCORE_HEAD
    return ok;
}

bool Score::acceptable(const TimeModel& m, const ScoreReq* reqs, int count, bool ownX) {
    if (!time_call_ok(m, reqs, count)) return false;
    bool shape = false;
#define WN_SCORE_IS(RR, SS, AA) shape = shape || (m.R == RR && m.S == SS && m.A == AA);
    WN_SCORE_SHAPES(WN_SCORE_IS)
#undef WN_SCORE_IS
    if (!shape) return false;
    long long total = 0;
    for (int i = 0; i < count; i++) {
        const ScoreReq& q = reqs[i];
        if (!time_inputs_ok(q.y, q.n, q.x, q.precision, q.cStride, q.tStride, q.temperature, ownX)) return false;
        if (q.logp == NULL || ((size_t)q.logp & 3) != 0) return false;
        char* const lp = (char*)store_target(q.logp);
        const size_t span = (size_t)(q.n - 1) * sizeof(float);
        if (lp == NULL || (char*)store_target((char*)q.logp + span) != lp + span) return false;
        if (q.rows != NULL && (((size_t)q.rows & 15) != 0 || !is_device_ptr(q.rows) || !is_device_ptr(q.rows + (size_t)q.n * m.A - 1))) return false;
        total += padded_samples(q.n);
        if (total > score_max_samples(m.f16, m.R, m.S)) return false;
    }
    return true;
}

bool Score::run(const TimeModel& m, const ScoreReq* reqs, int count, hipStream_t stream, bool ownX) {
    if (!acceptable(m, reqs, count, ownX)) return false;
    TimeJob* const jobs = m_jobs.begin(count);
    int maxTiles = 0;
    long long total = 0;
    for (int i = 0; i < count; i++) {
        const ScoreReq& q = reqs[i];
        TimeJob& jb = jobs[i];
        jb.y = q.y;
        jb.x = q.x;
        jb.cStride = q.cStride;
        jb.tStride = q.tStride;
        jb.logp = (float*)store_target(q.logp);
        jb.rows = q.rows;
        jb.row0 = total;
        jb.n = q.n;
        jb.tiles = (int)(padded_samples(q.n) / 16);
        jb.precision = q.precision;
        jb.yInPrev = jb.yInCur = 128;
        jb.scale = temperature_scale(q.temperature);
        total += padded_samples(q.n);
        if (jb.tiles > maxTiles) maxTiles = jb.tiles;
    }
    const TimeScratch sc = time_carve(m_scratch.atLeast((size_t)total * time_scratch_bytes(m.f16, m.R, m.S)), (size_t)total, m);
    const TimeJob* const dev = m_jobs.send(jobs, count, stream);

    return launchLayers(m, dev, count, maxTiles, false, sc, stream) && score_launch_head(m, dev, count, maxTiles, sc.skf, stream);
}

}  // namespace wn
