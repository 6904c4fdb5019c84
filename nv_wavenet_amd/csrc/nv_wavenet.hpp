// nv_wavenet.hpp -- host engine: nvWavenetInfer<T_weight, T_data, R, S, A> for MI355X (gfx950).
//
// Drop-in for the class of the same name in /root/reference/nv_wavenet.cuh:220-640: same template
// parameters, Implementation enum values, constructor, setEmbeddings / setLayerWeights /
// setOutWeights / setInputs, run / run_partial / run_chunks and debug getters, with the same
// argument meaning, layouts (col-major fp32 weights in, host OR device pointers, data copied),
// defaults and error convention (HIP errors print "GPUassert: ..." and exit, precondition
// violations assert, unsupported shapes make run() return false, nv_wavenet_util.cuh:34-40,
// nv_wavenet_singleblock.cuh:273-286).  Streams are hipStream_t.
//
// What is different underneath.  `Implementation` selects between device-code ORGANISATIONS of the
// same MFMA engine (all parity-tested against each other and the oracle):
//   SINGLE_BLOCK            one workgroup runs the whole network for its utterance tile(s), weights
//                           streamed from L2 every sample: wn::wavenet_wg with 1 to 4 tiles of 16
//                           utterances per workgroup by batch size
//   DUAL_BLOCK, PERSISTENT  wn::wavenet_chain: the layer stack split over a chain of CUs, each holding
//                           its layers' weights resident in registers + LDS, plus a head CU; hand-offs
//                           through L2-visible tagged granules (wn_chain.hpp); fewest CUs that hold the model
//   MANYBLOCK_NONPERSISTENT the same chain with one layer per CU
//   AUTO                    chosen from (R, S, A, L, batch, CUs): see pickOrganisation()
// An explicit Organisation (last constructor argument, beyond the reference's signature) overrides.
// batch_size_per_block is validated like the reference (nv_wavenet.cuh:559-561) but the batch tile is
// fixed by the MFMA shape (16 utterances), so it is a no-op hint.  Device buffers are laid out for this
// engine, not for the reference's kernels; the getters return the reference's layouts.
#pragma once

#include <assert.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <memory>
#include <type_traits>
#include <vector>

#include "gpu_check.hpp"
#include "mel_time.hpp"
#include "prefill.hpp"
#include "score.hpp"
#include "score_carry.hpp"
#include "slots_session.hpp"
#include "wn_chain.hpp"
#include "wn_kernels.hpp"

// kernel organisations (beyond the reference: its Implementation enum maps onto these, see above)
enum nvwOrganisation {
    NVW_ORG_AUTO = 0,     // from Implementation and the batch size
    NVW_ORG_WG = 1,       // wn::wavenet_wg, 1 to 4 tiles per workgroup by batch size
    NVW_ORG_WG1 = 2,      // wn::wavenet_wg, one tile per workgroup
    NVW_ORG_WG2 = 3,      // wn::wavenet_wg, two tiles per workgroup
    NVW_ORG_WG3 = 4,      // wn::wavenet_wg, three tiles per workgroup (fp16, R <= 64; else two)
    NVW_ORG_CHAIN = 5,    // wn::wavenet_chain, as many layers per CU as stay resident
    NVW_ORG_CHAIN1 = 6,   // wn::wavenet_chain, one layer per CU
    NVW_ORG_RETIRED7 = 7, // were: wn::wavenet_bcast (every wave its own tile, weights broadcast through an LDS ring; rounds 3-4) and its
    NVW_ORG_RETIRED8 = 8, // variants: measured, never real time anywhere, removed in round 5 (LABNOTES.md) -- refused
    NVW_ORG_RETIRED9 = 9,
    NVW_ORG_WG4 = 10,     // wn::wavenet_wg, four tiles per workgroup (round 6: fp16, R <= 64, dump-free launches with packed conditioning; else three)
    NVW_ORG_LAST = NVW_ORG_WG4
};

template <typename T_weight, typename T_data, int R = 64, int S = 128, int A = 256>
class nvWavenetInfer : protected wn::SlotHost {
public:
    enum Implementation { AUTO = 0, SINGLE_BLOCK, DUAL_BLOCK, PERSISTENT, MANYBLOCK_NONPERSISTENT };

    static constexpr bool F16 = !std::is_same<T_data, float>::value;
    static_assert(std::is_same<T_data, float>::value || std::is_same<T_data, half>::value,
                  "T_data must be float or half");
    static_assert(std::is_same<T_weight, float>::value == std::is_same<T_data, float>::value,
                  "T_weight/T_data must be <float,float> or <half2,half>");

protected:
    using C = wn::Cfg<F16, R, S, A, 1>;   // stream / layout constants do not depend on BT
    using CC = wn::CCfg<F16, R, S, A>;     // multi-CU chain
    using elem = typename wn::Prec<F16>::elem;
    // in-kernel conditioning (setConditioningWeights + features): the stream that also carries Wcond
    static constexpr int KFC = wn::feat_kfc<F16>();                    // feature fragments per tile and sample
    static constexpr int KC = KFC * 16 * wn::Prec<F16>::TPF;           // channels the features are padded to
    using CF = wn::Cfg<F16, R, S, A, 1, KFC>;
    static_assert(wn::kSoftScaleUnit == wn::kLog2e, "T = 1 is the kernel's default scale");

    Implementation m_implementation;
    int m_numLayers, m_maxBatch, m_maxSamples, m_maxDilation, m_tiles, m_numCUs;
    int m_org;           // resolved organisation: NVW_ORG_WG1 / WG2 / WG3 / WG (by batch at run time) / CHAIN / CHAIN1
    bool m_supported;    // false: this shape does not fit the CU (run() returns false, like the reference's unsupported variants)
    int m_chainLpc, m_chainStages;   // layers per chain stage, stages (layer stages + head)
    bool m_tanhEmbed;
    int m_num_samples_per_chunk;
    int m_ringSlots;
    int m_ringDirtyTiles;         // leading tiles whose rings launches have written since they were last zero
    int m_schedMode;              // compiled dilation schedule (wavenet_wg_cs) where a launch is eligible: 0 yes (default), -1 never
    int m_ringLdsMode;            // ring slots of the short dilations in LDS during wavenet_wg launches: 0 as many as fit (default), -1 never
    int m_lastStride;    // row stride of m_yOut in the latest launch (= its num_samples)

    elem* m_wblob;      // packed weight fragments: L layers then the head
    float* m_bias;      // fp32 biases
    elem* m_embedPrev;  // [A][R]
    elem* m_embedCur;
    elem* m_cond;       // packed conditioning (allocated by the first setInputs / setConditioning / packConditioning)
    int m_condRawSamples;
    const void* m_condRaw;    // or: the caller's [N][L][maxBatch][2R] device tensor, consumed in place (setConditioningDirect)
    int m_condRawKind;        // 1: fp32, 2: fp16 (T_data of the fp16 engine)
    const void* m_condUser;   // or: the caller's device buffer ALREADY in the engine's fragment order (setConditioningPacked)
    int m_condUserSamples;    // samples that buffer holds (+ one padding sample)
    // in-kernel conditioning (round 5): Lh = Wcond c + bcond computed by wavenet_wg from the upsampled features
    elem* m_wblobF;           // the weight streams with the conditioning weights in every layer's part (Cfg<.., KFC>)
    float* m_biasF;           // bias table with bcond added to the gate biases
    float* m_condW;           // [L][KC][2R] fp32: the conditioning weight, col-major per layer, channels zero-padded
    float* m_condB;           // [L][2R]
    int2* m_restream;         // fragment map plain stream -> that stream (restream_kernel)
    int m_restreamN;
    int m_nCond;              // channels of the model's features (0: no conditioning weights handed over)
    bool m_featDirty;         // m_wblobF / m_biasF are behind m_wblob / m_bias / m_condW
    elem* m_upTab;            // upsampling (setUpsampling): the ConvTranspose1d weight as MFMA A operands, [stride][5][m * KFC] fragments
    float* m_upBias;          // its bias, [80] fp32
    int m_upWindow, m_upStride;
    elem* m_melFrag;          // the utterances' mel frames in fragment order (setMel), [m_melFrames][m_tiles][KFC] fragments
    int m_melFrames, m_melCap;
    elem* m_feat;             // features packed by the engine (packFeatures), [maxSamples][m_tiles][KFC] fragments
    const void* m_featPtr;    // the features the runs read: m_feat or the caller's buffer in that order (setConditioningFeatures)
    int m_featSamples;
    float* m_outputSelectors;
    elem* m_ring;
    int *m_yInPrev, *m_yInCur, *m_yOut;
    float *m_XtOut, *m_skipOut, *m_Zs, *m_Za, *m_p;
    unsigned long long* m_mail;   // chain mailboxes
    unsigned* m_chainStatus;      // [0] time-out code of the chain launch in flight (0 = fine), [1] code of the latest launch that
                                  // gave up, [2] launches that gave up and were re-run by wavenet_wg (wn::chain_settle_kernel)
    size_t m_mailBytes;
    elem* m_ringShadow;           // the dilation rings as they were before the chain launch in flight ...
    int* m_histShadow;            // ... and the sample history: what the fallback launch starts from
    long long m_chainTimeoutTicks;

    float* m_stage;     // device staging for fp32 uploads from host pointers
    size_t m_stageElems;

    // extensions beyond the reference: in-kernel selectors, int16 PCM output
    bool m_useRng;
    unsigned long long m_rngSeed;
    short* m_pcm;       // [maxBatch][maxSamples] int16, allocated on first setAudioOut
    short* m_mulaw;     // [A] PCM value of every sample index
    short* m_pcmUser;   // caller's buffer (host or device), filled wherever yOut is
    size_t m_pcmUserElems;   // its size in int16 values when the caller said so (0: unknown)
    unsigned long long* m_clk;   // clock probe of the latest wavenet_wg launch (wn::Params::clk), when switched on
    bool m_clkOn;

    // sampling temperature per column (slots_sampler.hpp), lockstep and slot mode
    wn::SamplingTable m_temps;
    wn::PrimeTable m_prime;           // the lockstep primes (slots_prime.hpp)
    wn::Score m_score;                // scratch and staging of scoreSamples (score.hpp), nothing until the first call
    wn::MelTime m_melTime;            // staging and feature rows of upsampleRequests / prefillStatesMel / scoreSamplesMel (mel_time.hpp), nothing until the first call
    wn::Prefill m_prefill;            // scratch and staging of prefillStates (prefill.hpp), nothing until the first call
    // slot mode (slots_session.hpp): made at the end of the constructor, when the facts it is given are known
    std::unique_ptr<wn::SlotSession> m_slots;

    // events of run_chunks / run_stream, made on first use and kept
    std::vector<hipEvent_t> m_poolEvents;
    hipEvent_t pooledEvent(size_t i) {
        while (m_poolEvents.size() <= i) {
            hipEvent_t ev;
            gpuErrChk(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            m_poolEvents.push_back(ev);
        }
        return m_poolEvents[i];
    }
    static bool isDevicePtr(const void* ptr) { return wn::is_device_ptr(ptr); }
    // ---- staging of fp32 host sources: every array of ONE upload call gets its own place in the
    //      staging buffer, so the pack kernels of that call can all be in flight; the public set* calls
    //      end with one stream synchronisation (the caller may free or reuse its buffers afterwards)
    size_t m_stageUsed;
    void stageBegin(size_t totalElems) {
        if (totalElems > m_stageElems) {
            gpuErrChk(hipStreamSynchronize(0));
            if (m_stage) gpuErrChk(hipFree(m_stage));
            gpuErrChk(hipMalloc(&m_stage, totalElems * sizeof(float)));
            m_stageElems = totalElems;
        }
        m_stageUsed = 0;
    }
    const float* onDevice(const float* src, size_t n) {
        if (isDevicePtr(src)) return src;
        assert(m_stageUsed + n <= m_stageElems);
        float* d = m_stage + m_stageUsed;
        m_stageUsed += (n + 3) & ~(size_t)3;
        gpuErrChk(hipMemcpyAsync(d, src, n * sizeof(float), hipMemcpyHostToDevice, 0));
        return d;
    }
    static int gridFor(size_t n) {
        size_t g = (n + 255) / 256;
        return (int)(g > 4096 ? 4096 : (g ? g : 1));
    }
    // col-major fp32 M x K -> the NW per-wave fragment streams; blockFrag = fragment offset of this
    // matrix inside each wave's stream
    void packWeight(size_t blockFrag, const float* src, int M, int K, int gateRT) {
        const float* d = onDevice(src, (size_t)M * K);
        hipLaunchKernelGGL((wn::pack_weight_kernel<F16>), dim3(gridFor((size_t)M * K)), dim3(256), 0, 0,
                           m_wblob + blockFrag * C::FRAG_ELEMS, d, M, K, C::NW,
                           C::waveStreamFrags(m_numLayers) * C::FRAG_ELEMS, gateRT);
        gpuErrChk(hipGetLastError());
    }
    void convertTo(elem* dst, const float* src, size_t n) {
        const float* d = onDevice(src, n);
        hipLaunchKernelGGL((wn::convert_kernel<F16>), dim3(gridFor(n)), dim3(256), 0, 0, dst, d, n);
        gpuErrChk(hipGetLastError());
    }
    // (dump: the kernel variant that can dump holds every layer's running skip-bias sum in LDS, the dump-free one a single row)
    template <int BT> static size_t ldsNeed(int L, int embTables, bool dump = true) { return wn::Cfg<F16, R, S, A, BT>::ldsBytes(L, embTables, dump); }
    static constexpr size_t kLdsMax = 160 * 1024;
    template <int BT> bool ldsFits(bool dump = true) const { return ldsNeed<BT>(m_numLayers, 0, dump) <= kLdsMax; }
    // how many embedding tables fit in LDS beside everything else: 2, 1 (current tap) or 0
    template <int BT> int embTables(bool dump = true) const {
        return ldsNeed<BT>(m_numLayers, 2, dump) <= kLdsMax ? 2 : ldsNeed<BT>(m_numLayers, 1, dump) <= kLdsMax ? 1 : 0;
    }
    // DUMP = false (no activation dump code at all): every conditioning path of the fp16 engine (the production path); for the fp32
    // engine -- the parity mode, and what the reference's PyTorch entry wavenet_infer() runs -- the packed-conditioning kernels and
    // the chain (round 6: that entry has no getter that could read a dump, pytorch/wavenet_infer.h:33-58); fp32 launches that read
    // the conditioning in place or compute it from features carry the dump code whether asked or not
    // dilation schedule (nv_wavenet.cuh:99,110-111) as a table in the kernel arguments: dilation and first ring slot
    void fillSchedule(wn::Params& p) const {
        int d = 1, off = 0;
        for (int l = 0; l < m_numLayers; l++) {
            p.dil[l].d = d;
            p.dil[l].off = off;
            p.dil[l].lds = 0;
            off += d;
            d <<= 1;
            if (d > m_maxDilation) d = 1;
        }
        p.dil[m_numLayers] = p.dil[0];
        p.dil[m_numLayers + 1] = p.dil[1];
    }
    // The ring slots of the short dilations in LDS (round 6): the largest dilation D (a power of two) whose layers' slots -- sum of d
    // over the layers with d <= D, BT x R/32 KiB each -- fit beside everything else; 0: none.  The first Cfg::RING_INPLACE slots take the space
    // the exchange images left when they moved onto the head's image (Cfg::OVERLAY): `need` counts it already; the others follow them
    // (Cfg::ringSlotOffset).  Sets p.ldsRingD and the LDS slot numbers of the schedule table; returns the bytes to add to the launch's
    // dynamic LDS (0 when the in-place slots are enough: p.ldsRingD says whether there are any).
    template <int BT> size_t placeLdsRing(wn::Params& p, size_t need) const {
        using CB = wn::Cfg<F16, R, S, A, BT>;
        int D = 0;
        for (int d = 1; d <= m_maxDilation && d <= WN_LDS_RING_MAXD; d <<= 1)
            if (need + (size_t)CB::ringTailSlots(CB::ldsRingSlots(m_numLayers, m_maxDilation, d)) * CB::RING_SLOT <= kLdsMax) D = d;
        p.ldsRingD = D;
        int slot = 0;
        for (int l = 0; l < m_numLayers; l++) {
            p.dil[l].lds = slot;
            if (p.dil[l].d <= D) slot += p.dil[l].d;
        }
        p.dil[m_numLayers] = p.dil[0];
        p.dil[m_numLayers + 1] = p.dil[1];
        return (size_t)CB::ringTailSlots(slot) * CB::RING_SLOT;
    }
    // ... and whether a launch uses them (the LR instantiations of wavenet_wg: the dump-free kernels).
    // m_ringLdsMode >= 0 (default): as many of the short dilations as fit; -1: never.  Measured at C3 (us per sample with / without):
    // one tile per workgroup, d <= 4 on chip, 21.1 / 21.7; two tiles, d <= 2 in the place of the older tap's embedding table,
    // 28.4 / 29.2; four tiles, d <= 1, 43.6 / 44.2 (LABNOTES round 6, separate calls); three tiles, one call with the arms alternating
    // (LABNOTES, "Exchange images on the head's image"): d <= 2 with the in-place slots 36.7 / 37.6, d <= 1 as before them 37.2.
    static constexpr bool lrBuilt(bool dump, int raw) { return !dump && (raw == 0 || F16); }      // (fp32 engines: dump-free code exists for the packed conditioning only)
    template <int BT> size_t ringPlan(wn::Params& p, size_t need, bool dump, int raw) const {
        p.ldsRingD = 0;
#ifdef WN_EXP_TWO_WG
        if (BT == 1) return 0;
#endif
        if (!lrBuilt(dump, raw) || m_ringLdsMode < 0) return 0;
        wn::Params q = p;
        const size_t bytes = placeLdsRing<BT>(q, need);
        if (q.ldsRingD <= 0) return 0;
        p = q;
        return bytes;
    }
    // The kernels with a compiled dilation schedule (wavenet_wg<.., LR, CYC = 10, LD>): the three-tile fp16 dump-free launch with packed
    // conditioning of a model whose dilations run 1 .. 512 in whole cycles, with the slots of d <= 1 (LD = 1) or d <= 2 (LD = 2) in LDS.
    // Returns LD for a launch whose ring plan keeps d <= ringD on chip, 0 for a launch that reads its schedule at run time.  (More may
    // fit than LD = 2 holds: placing fewer layers than fit is always legal; the caller caps the plan to 2^(LD-1).)
    static constexpr int kCycle = 10;
    // ... and, for a model of exactly kStraight cycles, the layer count compiled in as well (wavenet_wg_sl: the sample's layers as
    // straight-line code, no join with loads in flight); other whole numbers of cycles keep the cycle loop
    static constexpr int kStraight = 2;
    bool straightLine() const { return m_numLayers == kStraight * kCycle; }
    static constexpr bool schedBuilt(int bt, bool dump, int raw) { return F16 && WG3 && bt == 3 && !dump && raw == 0; }
    int compiledSchedule(int bt, bool dump, int raw, int ringD) const {
        if (!schedBuilt(bt, dump, raw) || m_schedMode < 0) return 0;
        if (m_maxDilation != (1 << (kCycle - 1)) || m_numLayers % kCycle != 0 || ringD < 1) return 0;
        return ringD >= 2 ? 2 : 1;
    }
    // caps a ring plan to the layers with d <= D: the LDS slot numbers of the schedule table as placeLdsRing counts them
    void capLdsRing(wn::Params& p, int D) const {
        p.ldsRingD = D;
        int slot = 0;
        for (int l = 0; l < m_numLayers; l++) {
            p.dil[l].lds = slot;
            if (p.dil[l].d <= D) slot += p.dil[l].d;
        }
        p.dil[m_numLayers] = p.dil[0];
        p.dil[m_numLayers + 1] = p.dil[1];
    }
    template <int BT, bool EMB, bool DUMP, int RAW> bool launchK(wn::Params& p, int tiles, int nEmb, hipStream_t stream) {
        using CB = wn::Cfg<F16, R, S, A, BT>;
        const int grid = (tiles + BT - 1) / BT;
        p.embLds = nEmb;
        const size_t need = ldsNeed<BT>(m_numLayers, nEmb, DUMP);
        if constexpr (lrBuilt(DUMP, RAW)) {
            const size_t ringBytes = ringPlan<BT>(p, need, DUMP, RAW);
            if constexpr (schedBuilt(BT, DUMP, RAW)) {
                const int ld = compiledSchedule(BT, DUMP, RAW, p.ldsRingD);
                if (ld > 0) {
                    capLdsRing(p, 1 << (ld - 1));      // (the LDS of the plan stays: no smaller than what the capped one needs)
                    if (straightLine()) {
                        if (ld == 2) hipLaunchKernelGGL((wn::wavenet_wg_sl<F16, R, S, A, BT, EMB, kCycle, kStraight, 2>), dim3(grid), dim3(CB::THREADS), need + ringBytes, stream, p);
                        else hipLaunchKernelGGL((wn::wavenet_wg_sl<F16, R, S, A, BT, EMB, kCycle, kStraight, 1>), dim3(grid), dim3(CB::THREADS), need + ringBytes, stream, p);
                    } else if (ld == 2) hipLaunchKernelGGL((wn::wavenet_wg_cs<F16, R, S, A, BT, EMB, kCycle, 2>), dim3(grid), dim3(CB::THREADS), need + ringBytes, stream, p);
                    else hipLaunchKernelGGL((wn::wavenet_wg_cs<F16, R, S, A, BT, EMB, kCycle, 1>), dim3(grid), dim3(CB::THREADS), need + ringBytes, stream, p);
                    return hipGetLastError() == hipSuccess;
                }
            }
            if (p.ldsRingD > 0) {
                hipLaunchKernelGGL((wn::wavenet_wg<F16, R, S, A, BT, EMB, DUMP, RAW, true>), dim3(grid), dim3(CB::THREADS), need + ringBytes, stream, p);
                return hipGetLastError() == hipSuccess;
            }
        }
        p.ldsRingD = 0;
        hipLaunchKernelGGL((wn::wavenet_wg<F16, R, S, A, BT, EMB, DUMP, RAW>), dim3(grid), dim3(CB::THREADS), need, stream, p);
        return hipGetLastError() == hipSuccess;
    }
    // embedding tables of a launch in LDS: as many as fit; a launch whose two tables leave no room for a single ring slot gives up the
    // OLDER tap's table for ring slots (its gather is one sample early, off the dependent chain; C3 at two tiles: 28.4 against 29.2 us).
    // With the in-place slots (Cfg::RING_INPLACE) the two layers of dilation 1 always fit: the older table likewise goes where it stands
    // between them and a longer dilation (d <= 1 alone is two layers of twenty at C3: 37.3 against 37.4 us at three tiles), and stays
    // where the same dilations fit beside it.
    template <int BT> int planEmb(bool dump, int raw) const {
        int nEmb = embTables<BT>(dump);
#ifdef WN_EXP_TWO_WG
        if (BT == 1) return 0;      // (experiment: two workgroups per CU: 80 KiB of LDS each)
#endif
        if (nEmb == 2 && m_ringLdsMode >= 0 && lrBuilt(dump, raw)) {
            wn::Params q;
            fillSchedule(q);
            placeLdsRing<BT>(q, ldsNeed<BT>(m_numLayers, 2, dump));
            const int D2 = q.ldsRingD;
            placeLdsRing<BT>(q, ldsNeed<BT>(m_numLayers, 1, dump));
            if (D2 == 0 || (D2 < 2 && q.ldsRingD > D2)) nEmb = 1;
        }
        return nEmb;
    }
    template <int BT, bool DUMP, int RAW> bool launchE(wn::Params& p, int tiles, hipStream_t stream) {
        const int nEmb = planEmb<BT>(DUMP, RAW);
        return nEmb ? launchK<BT, true, DUMP, RAW>(p, tiles, nEmb, stream) : launchK<BT, false, DUMP, RAW>(p, tiles, 0, stream);
    }
    template <int BT, bool DUMP> bool launchD(wn::Params& p, int tiles, hipStream_t stream) {
        if (p.condRawKind == 3) return launchE<BT, DUMP, 3>(p, tiles, stream);
        if constexpr (F16) {
            if (p.condRawKind == 2) return launchE<BT, DUMP, 2>(p, tiles, stream);
        }
        return p.condRawKind == 1 ? launchE<BT, DUMP, 1>(p, tiles, stream) : launchE<BT, DUMP, 0>(p, tiles, stream);
    }
    template <int BT> bool launch(wn::Params& p, int tiles, hipStream_t stream) {
        if (!p.dump) {
            if constexpr (F16) return launchD<BT, false>(p, tiles, stream);
            else if (p.condRawKind == 0) return launchE<BT, false, 0>(p, tiles, stream);
        }
        return launchD<BT, true>(p, tiles, stream);
    }
    template <int BT, bool EMB, bool DUMP, int RAW> void allowLdsK() {
        const size_t need = ldsNeed<BT>(m_numLayers, EMB ? embTables<BT>(DUMP) : 0, DUMP);
        if (need <= kLdsMax) {
            gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_wg<F16, R, S, A, BT, EMB, DUMP, RAW>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
            if constexpr (lrBuilt(DUMP, RAW))      // (the whole LDS: what the tables leave free holds ring slots, placeLdsRing)
                gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_wg<F16, R, S, A, BT, EMB, DUMP, RAW, true>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            if constexpr (schedBuilt(BT, DUMP, RAW)) {
                gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_wg_cs<F16, R, S, A, BT, EMB, kCycle, 1>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
                gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_wg_cs<F16, R, S, A, BT, EMB, kCycle, 2>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
                gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_wg_sl<F16, R, S, A, BT, EMB, kCycle, kStraight, 1>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
                gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_wg_sl<F16, R, S, A, BT, EMB, kCycle, kStraight, 2>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            }
        }
    }
    template <int BT, bool DUMP> void allowLdsD() {
        allowLdsK<BT, false, DUMP, 0>();
        allowLdsK<BT, true, DUMP, 0>();
        allowLdsK<BT, false, DUMP, 1>();
        allowLdsK<BT, true, DUMP, 1>();
        allowLdsK<BT, false, DUMP, 3>();
        allowLdsK<BT, true, DUMP, 3>();
        if constexpr (F16) {
            allowLdsK<BT, false, DUMP, 2>();
            allowLdsK<BT, true, DUMP, 2>();
        }
    }
    template <int BT> void allowLds() {
        allowLdsD<BT, true>();
        if constexpr (F16) allowLdsD<BT, false>();
        else {
            allowLdsK<BT, false, false, 0>();
            allowLdsK<BT, true, false, 0>();
        }
    }
    float* headBias() { return m_bias + (size_t)m_numLayers * C::BIAS_L; }

    // ---- organisation ----------------------------------------------------------------------------
    static int chainStagesFor(int L, int lpc) { return (L + lpc - 1) / lpc + 1; }
    // layers per stage: the fewest stages that keep every layer resident, balanced
    static int chainLpcMax(int L) {
        if (!CC::SUPPORTED) return 0;
        const int ns = (L + CC::LPC - 1) / CC::LPC;
        return (L + ns - 1) / ns;
    }
    // a chain of `stages` CUs serves up to TPC_MAX tiles in turn (round 5): all tiles of the batch ride resident chains
    bool chainFits(int lpc, int tiles) const {
        return lpc > 0 && chainStagesFor(m_numLayers, lpc) * ((tiles + CC::TPC_MAX - 1) / CC::TPC_MAX) <= m_numCUs;
    }
    // The single-workgroup organisation: one, two or -- fp16, R <= 64 -- three or four tiles per workgroup (split over the 4 SIMDs
    // of a CU) by batch size, see wgTiles(); beyond four tiles per CU the launch has more workgroups than CUs.
    int singleOrg(int) const { return NVW_ORG_WG; }
    // Per-sample time models (microseconds) of the organisations that can run `tiles` tiles, from the shape: weight bytes per
    // sample W, layers L, CUs.  Every constant is a measurement on MI355X, kept with its source:
    struct OrgTimes {
        // the multi-CU chain only competes at batches of a few tiles, where the GPU holds its full shader clock
        // (profiles/r04_clock_wg_sweep.json: 2.39 GHz up to 192 busy CUs, 2.0 with all 256)
        static constexpr double kClockMHz = 2390.0;
        static constexpr double kStreamBytesPerClk = 58.0;   // weight stream L2 -> registers of one CU (scripts/ubench/stream.hip)
        static constexpr double kStreamLayerUs = 0.25;       // dependent chain per layer beside the stream (one tile)
        static constexpr double kHeadUs = 4.0;               // head GEMMs + softmax + embedding, either organisation
        static constexpr double kChainHopUs = 1.1;           // one stage hand-off (hop 0.55 + entry / exit)
        static constexpr double kChainLayerUs(int r) { return r >= 128 ? 0.55 : 0.4; }   // resident-weight layer of a stage
        // several tiles per chain: a sample of a tile occupies the busiest stage (the head) this long, so a chain's sample period is
        // max(trip round the chain, tiles per chain x this)  (round 5, C4: profiles/r05_chain_c4_tiles_per_chain.json)
        static constexpr double kChainUnitUs = 5.0;
    };
    int pickOrganisation(int tiles) const {
        const int single = singleOrg(tiles);
        const int lpc = chainLpcMax(m_numLayers);
        if (!chainFits(lpc, tiles)) return single;
        const double wBytes = sizeof(elem) * ((double)m_numLayers * (5.0 * R * R + (double)S * R) + (double)A * S + (double)A * A);
        // one workgroup per (1 .. wgMax) tiles, whole rounds of them beyond one per CU
        const int wgMax = WG3 ? 3 : WG2 ? 2 : 1;
        const int rounds = (tiles + wgMax * m_numCUs - 1) / (wgMax * m_numCUs);
        const double tStream = (wBytes / (OrgTimes::kStreamBytesPerClk * OrgTimes::kClockMHz) + OrgTimes::kStreamLayerUs * m_numLayers + OrgTimes::kHeadUs) * rounds;
        const int stages = chainStagesFor(m_numLayers, lpc), perLaunch = m_numCUs / stages;
        const int tpc = (tiles + perLaunch - 1) / perLaunch;
        // several tiles per chain: measured where wavenet_wg cannot be real time (C4, R = 128); the shapes with a three-tile
        // wavenet_wg have their throughput organisation in that (C3: 1.3 utterances per CU and us against the chain's 0.7)
        if (tpc > 1 && WG3) return single;
        double tChain = OrgTimes::kChainHopUs * stages + OrgTimes::kChainLayerUs(R) * m_numLayers + OrgTimes::kHeadUs;
        if (tpc * OrgTimes::kChainUnitUs > tChain) tChain = tpc * OrgTimes::kChainUnitUs;
        // (the time model of wavenet_wg is its one-tile latency: with two or three tiles per workgroup, i.e. beyond one tile per CU, a
        //  sample takes up to twice as long -- the chain is only preferred there when even that is slower)
        const double tWg = tiles > m_numCUs ? tStream * (tiles > 2 * m_numCUs && WG3 ? 1.9 : WG2 ? 1.4 : 1.0) : tStream;
        return tChain < tWg ? NVW_ORG_CHAIN : single;
    }
    void resolveOrganisation(int requested) {
        const int tiles = (m_maxBatch + 15) / 16;
        int org = requested;
        if (org == NVW_ORG_AUTO) {
            switch (m_implementation) {
                case SINGLE_BLOCK: org = singleOrg(tiles); break;
                case DUAL_BLOCK:
                case PERSISTENT: org = chainFits(chainLpcMax(m_numLayers), tiles) ? NVW_ORG_CHAIN : singleOrg(tiles); break;
                case MANYBLOCK_NONPERSISTENT:
                    org = (CC::SUPPORTED && chainFits(1, tiles)) ? NVW_ORG_CHAIN1
                          : chainFits(chainLpcMax(m_numLayers), tiles) ? NVW_ORG_CHAIN : singleOrg(tiles);
                    break;
                default: org = pickOrganisation(tiles); break;
            }
        }
        if (org == NVW_ORG_CHAIN && !chainFits(chainLpcMax(m_numLayers), tiles)) org = singleOrg(tiles);
        if (org == NVW_ORG_CHAIN1 && !(CC::SUPPORTED && chainFits(1, tiles))) org = singleOrg(tiles);
        m_org = org;
        m_chainLpc = org == NVW_ORG_CHAIN ? chainLpcMax(m_numLayers) : org == NVW_ORG_CHAIN1 ? 1 : 0;
        m_chainStages = m_chainLpc ? chainStagesFor(m_numLayers, m_chainLpc) : 0;
    }
    bool isChain() const { return m_chainLpc > 0; }
    // launches whose chains serve several tiles use the instantiation that requests a unit's packed conditioning up front (wn_chain.hpp: HOIST)
    // (built for the shapes whose stages hold at most two layers -- R = 128: C4 --, where it costs no scratch; C2 / C3 stages hold five and spill with it)
    static constexpr bool kChainHoistBuilt = F16 && CC::SUPPORTED && CC::LP <= 2 && A <= 512;      // (the A = 1024 head spills as it is)
    static bool chainHoists(int tpc) { return kChainHoistBuilt && tpc > WN_CHAIN_HOIST_FROM; }
    // tiles per chain for a batch of `tiles` tiles: as few as put every tile on a resident chain, at most TPC_MAX
    int chainTpc(int tiles) const {
        const int perLaunch = m_numCUs / (m_chainStages > 0 ? m_chainStages : 1);
        int tpc = perLaunch > 0 ? (tiles + perLaunch - 1) / perLaunch : 1;
#ifdef WN_CHAIN_TPC_MIN      // (experiment: the mailbox layout of several tiles per chain for launches that have one)
        if (tpc < WN_CHAIN_TPC_MIN) tpc = WN_CHAIN_TPC_MIN;
#endif
        return tpc < 1 ? 1 : tpc > CC::TPC_MAX ? CC::TPC_MAX : tpc;
    }
    // tiles per workgroup of wn::wavenet_wg for a batch of `tiles` tiles
    static constexpr bool WG3 = F16 && R <= 64;   // shapes with a three-tile instantiation
    static constexpr bool WG2 = R < 128;          // ... with a two-tile one (two tiles of R >= 128 need the registers of three: 300-560 spilled,
                                                  // slower than one tile; they fit the LDS only for shallow models anyway)
    bool wg3Fits() const {
        if constexpr (WG3) return ldsFits<3>();
        return false;
    }
    // ... with a four-tile one (round 6): dump-free kernels only -- the folded skip-bias table is what makes room for the fourth tile's
    // exchange images -- and for the packed conditioning; other launches of such an engine take three tiles per workgroup
    static constexpr bool WG4 = WG3;
    bool wg4Fits() const {
        if constexpr (WG4) return ldsFits<4>(false);
        return false;
    }
    int wgTiles(int tiles) const {
#ifdef WN_EXP_TWO_WG
        if (m_org == NVW_ORG_WG && tiles <= 2 * m_numCUs) return 1;      // (experiment: up to two one-tile workgroups per CU)
#endif
        // AUTO beyond three tiles per CU: the launch runs in whole rounds of workgroups, ceil(tiles / (BT x CUs)) of them; a round of
        // four-tile workgroups takes 1.3 times a round of three-tile ones at the socket's power limit (47 against 36 us per sample,
        // LABNOTES round 6), so four tiles win where they save a round: (3, 4] and (6, 8] tiles per CU ...
        bool four = m_org == NVW_ORG_WG4;
        if (m_org == NVW_ORG_WG && tiles > WN_WG4_FROM * m_numCUs) {
            const int r4 = (tiles + 4 * m_numCUs - 1) / (4 * m_numCUs), r3 = (tiles + 3 * m_numCUs - 1) / (3 * m_numCUs);
            four = r4 * 47 <= r3 * 36;
        }
        if (four && wg4Fits() && wg3Fits()) return 4;
        const bool three = four || m_org == NVW_ORG_WG3 || (m_org == NVW_ORG_WG && tiles > 2 * m_numCUs);
        if (three && wg3Fits()) return 3;
        const bool two = three || m_org == NVW_ORG_WG2 || (m_org == NVW_ORG_WG && tiles > m_numCUs);
        if constexpr (WG2) return (two && ldsFits<2>()) ? 2 : 1;
        return 1;
    }

public:
    nvWavenetInfer(int numLayers, int maxDilation, int batchSize, int numSamples, int impl = 0,
                   bool tanhEmbed = true, int organisation = NVW_ORG_AUTO)
        : m_implementation((Implementation)impl), m_numLayers(numLayers), m_maxBatch(batchSize),
          m_maxSamples(numSamples), m_maxDilation(maxDilation), m_tanhEmbed(tanhEmbed),
          m_num_samples_per_chunk(0), m_lastStride(numSamples), m_cond(NULL), m_condRawSamples(0), m_condRaw(NULL), m_condRawKind(0), m_condUser(NULL), m_condUserSamples(0),
          m_wblobF(NULL), m_biasF(NULL), m_condW(NULL), m_condB(NULL), m_restream(NULL), m_restreamN(0), m_nCond(0), m_featDirty(true),
          m_upTab(NULL), m_upBias(NULL), m_upWindow(0), m_upStride(0), m_melFrag(NULL), m_melFrames(0), m_melCap(0),
          m_feat(NULL), m_featPtr(NULL), m_featSamples(0),
          m_mail(NULL), m_chainStatus(NULL), m_mailBytes(0), m_ringShadow(NULL), m_histShadow(NULL),
          m_chainTimeoutTicks(wn::kChainTimeoutTicks), m_stage(NULL), m_stageElems(0), m_useRng(false), m_rngSeed(0), m_pcm(NULL),
          m_mulaw(NULL), m_pcmUser(NULL), m_pcmUserElems(0), m_clk(NULL), m_clkOn(false), m_temps(batchSize), m_prime(batchSize), m_stageUsed(0) {
        assert(numLayers >= 2 && batchSize > 0 && numSamples > 0 && maxDilation > 0);
        m_ringDirtyTiles = 0;
        m_ringLdsMode = 0;
        m_schedMode = 0;
        assert(numLayers <= wn::kMaxLayers);
        {
            int dev = 0;
            hipDeviceProp_t prop;
            gpuErrChk(hipGetDevice(&dev));
            gpuErrChk(hipGetDeviceProperties(&prop, dev));
            m_numCUs = prop.multiProcessorCount;
        }
        resolveOrganisation(organisation);
        // The bias table of the whole model lives in the LDS of a wavenet_wg workgroup: a model whose
        // table does not fit cannot run there (the reference prints and returns false for shapes a
        // variant does not support, nv_wavenet_singleblock.cuh:273-286)
        m_supported = isChain() || ldsFits<1>();
        if (!m_supported)
            fprintf(stderr, "nvWavenetInfer: R=%d S=%d A=%d with %d layers needs %zu bytes of LDS (> 160 KiB): unsupported\n", R,
                    S, A, numLayers, ldsNeed<1>(numLayers, 0));

        // conditioning / ring are allocated for whole workgroups (two to four tiles per workgroup may be chosen), else
        // exactly the tiles of the batch
        {
            const int tiles = (batchSize + 15) / 16;
            int group = isChain() ? 1 : wgTiles(tiles);
            // (an engine that launches four tiles per workgroup also launches three: smaller batches, launches that dump or read the
            //  conditioning in place)
            if (group >= 3 && wg4Fits()) group = 12;
            m_tiles = (tiles + group - 1) / group * group;
        }

        // dilation schedule (nv_wavenet.cuh:99,110-111): d doubles per layer, back to 1 past maxDilation
        {
            int d = 1, slots = 0;
            for (int l = 0; l < numLayers; l++) {
                slots += d;
                d <<= 1;
                if (d > maxDilation) d = 1;
            }
            m_ringSlots = slots;
        }

        const size_t wElems = (size_t)C::NW * C::waveStreamFrags(numLayers) * C::FRAG_ELEMS;
        gpuErrChk(hipMalloc(&m_wblob, wElems * sizeof(elem)));
        gpuErrChk(hipMemset(m_wblob, 0, wElems * sizeof(elem)));
        const size_t bElems = (size_t)numLayers * C::BIAS_L + 2 * A;
        gpuErrChk(hipMalloc(&m_bias, bElems * sizeof(float)));
        gpuErrChk(hipMemset(m_bias, 0, bElems * sizeof(float)));
        gpuErrChk(hipMalloc(&m_embedPrev, (size_t)A * R * sizeof(elem)));
        gpuErrChk(hipMalloc(&m_embedCur, (size_t)A * R * sizeof(elem)));
        gpuErrChk(hipMemset(m_embedPrev, 0, (size_t)A * R * sizeof(elem)));
        gpuErrChk(hipMemset(m_embedCur, 0, (size_t)A * R * sizeof(elem)));

        // (the packed conditioning -- the largest buffer by far -- is allocated when a caller first packs some: engines
        //  that only ever read the conditioning in place never pay for it)
        gpuErrChk(hipMalloc(&m_outputSelectors, (size_t)numSamples * batchSize * sizeof(float)));
        gpuErrChk(hipMemset(m_outputSelectors, 0, (size_t)numSamples * batchSize * sizeof(float)));

        const size_t ringBytes = ringElems() * sizeof(elem);
        gpuErrChk(hipMalloc(&m_ring, ringBytes));
        gpuErrChk(hipMemset(m_ring, 0, ringBytes));

        gpuErrChk(hipMalloc(&m_yInPrev, batchSize * sizeof(int)));
        gpuErrChk(hipMalloc(&m_yInCur, batchSize * sizeof(int)));
        gpuErrChk(hipMalloc(&m_yOut, (size_t)numSamples * batchSize * sizeof(int)));
        gpuErrChk(hipMemset(m_yOut, 0, (size_t)numSamples * batchSize * sizeof(int)));

        gpuErrChk(hipMalloc(&m_XtOut, (size_t)numLayers * R * batchSize * sizeof(float)));
        gpuErrChk(hipMalloc(&m_skipOut, (size_t)numLayers * S * batchSize * sizeof(float)));
        gpuErrChk(hipMalloc(&m_Zs, (size_t)A * batchSize * sizeof(float)));
        gpuErrChk(hipMalloc(&m_Za, (size_t)A * batchSize * sizeof(float)));
        gpuErrChk(hipMalloc(&m_p, (size_t)A * batchSize * sizeof(float)));
        gpuErrChk(hipMemset(m_XtOut, 0, (size_t)numLayers * R * batchSize * sizeof(float)));
        gpuErrChk(hipMemset(m_skipOut, 0, (size_t)numLayers * S * batchSize * sizeof(float)));
        gpuErrChk(hipMemset(m_Zs, 0, (size_t)A * batchSize * sizeof(float)));
        gpuErrChk(hipMemset(m_Za, 0, (size_t)A * batchSize * sizeof(float)));
        gpuErrChk(hipMemset(m_p, 0, (size_t)A * batchSize * sizeof(float)));

        gpuErrChk(hipMalloc(&m_chainStatus, 4 * sizeof(unsigned)));
        gpuErrChk(hipMemset(m_chainStatus, 0, 4 * sizeof(unsigned)));
        if (isChain()) {
            {
                const int tiles = (batchSize + 15) / 16, perLaunch = m_numCUs / m_chainStages;
                m_mailBytes = CC::mailGranules(tiles < perLaunch ? tiles : perLaunch, m_chainStages, chainTpc(tiles)) * sizeof(unsigned long long);
            }
            gpuErrChk(hipMalloc(&m_mail, m_mailBytes));
            gpuErrChk(hipMemset(m_mail, 0, m_mailBytes));
            gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_chain<F16, R, S, A, true>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)CC::ldsBytes()));
            gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_chain<F16, R, S, A, false>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)CC::ldsBytes()));
            if constexpr (kChainHoistBuilt)      // (several tiles per chain: the instantiation that requests a unit's conditioning up front)
                gpuErrChk(hipFuncSetAttribute((const void*)wn::wavenet_chain<F16, R, S, A, false, true>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)CC::ldsBytes()));
            if (chainHasFallback()) {
                gpuErrChk(hipMalloc(&m_ringShadow, ringBytes));
                gpuErrChk(hipMalloc(&m_histShadow, 2 * (size_t)batchSize * sizeof(int)));
            }
        }

        hipLaunchKernelGGL(wn::silence_kernel, dim3(1), dim3(256), 0, 0, m_yInPrev, m_yInCur, m_maxBatch);
        gpuErrChk(hipGetLastError());

        if (ldsFits<1>()) {            // (a chain engine launches wavenet_wg as its fallback)
            allowLds<1>();
            if (!isChain()) {
                if constexpr (WG2) allowLds<2>();
                if constexpr (WG3) allowLds<3>();
                if constexpr (WG4) {
                    if (wg4Fits()) {
                        allowLdsK<4, false, false, 0>();
                        allowLdsK<4, true, false, 0>();
                    }
                }
            }
        }
        gpuErrChk(hipDeviceSynchronize());
        m_slots.reset(new wn::SlotSession(wn::SlotFacts{m_maxBatch, m_tiles, m_numLayers, m_maxDilation, m_ringSlots, (int)(R * 16 * sizeof(elem) / 1024), R,
                                                        F16, featureElems(1), m_supported, m_ring, m_yInPrev, m_yInCur, A},
                                          *this, m_temps));
    }

    virtual ~nvWavenetInfer() {
        gpuErrChk(hipDeviceSynchronize());
        m_slots.reset();
        for (hipEvent_t ev : m_poolEvents) gpuErrChk(hipEventDestroy(ev));
        gpuErrChk(hipFree(m_wblob));
        gpuErrChk(hipFree(m_bias));
        gpuErrChk(hipFree(m_embedPrev));
        gpuErrChk(hipFree(m_embedCur));
        if (m_cond) gpuErrChk(hipFree(m_cond));
        if (m_wblobF) gpuErrChk(hipFree(m_wblobF));
        if (m_biasF) gpuErrChk(hipFree(m_biasF));
        if (m_condW) gpuErrChk(hipFree(m_condW));
        if (m_condB) gpuErrChk(hipFree(m_condB));
        if (m_restream) gpuErrChk(hipFree(m_restream));
        if (m_feat) gpuErrChk(hipFree(m_feat));
        if (m_upTab) gpuErrChk(hipFree(m_upTab));
        if (m_upBias) gpuErrChk(hipFree(m_upBias));
        if (m_melFrag) gpuErrChk(hipFree(m_melFrag));
        gpuErrChk(hipFree(m_outputSelectors));
        gpuErrChk(hipFree(m_ring));
        gpuErrChk(hipFree(m_yInPrev));
        gpuErrChk(hipFree(m_yInCur));
        gpuErrChk(hipFree(m_yOut));
        gpuErrChk(hipFree(m_XtOut));
        gpuErrChk(hipFree(m_skipOut));
        gpuErrChk(hipFree(m_Zs));
        gpuErrChk(hipFree(m_Za));
        gpuErrChk(hipFree(m_p));
        gpuErrChk(hipFree(m_chainStatus));
        if (m_mail) gpuErrChk(hipFree(m_mail));
        if (m_ringShadow) gpuErrChk(hipFree(m_ringShadow));
        if (m_histShadow) gpuErrChk(hipFree(m_histShadow));
        if (m_stage) gpuErrChk(hipFree(m_stage));
        if (m_pcm) gpuErrChk(hipFree(m_pcm));
        if (m_mulaw) gpuErrChk(hipFree(m_mulaw));
        if (m_clk) gpuErrChk(hipFree(m_clk));
    }

    // false: the shape does not fit this GPU's CUs in the chosen organisation; run() returns false
    bool supported() const { return m_supported; }
    // Multi-CU launches.  A wavenet_chain launch whose workgroups are not all resident in time (other work holds CUs:
    // another stream, engine or process) gives up -- every spin is bounded -- and the SAME stream then re-runs the
    // launch's samples on wavenet_wg from the state the launch started with (launchChain), so the samples delivered are
    // the right ones either way.  chainStatus(): 0, or the code of a give-up that could NOT be repaired (0x100+stage: x,
    // 0x200+stage: skip sums, 0x300: head, 0x400+: placement exchange); chainFallbacks(): launches that were re-run;
    // chainLastTimeout(): the code of the latest of them.  All three synchronise the device.
    unsigned chainStatus() { return statusWord(0); }
    unsigned chainFallbacks() { return statusWord(2); }
    unsigned chainLastTimeout() { return statusWord(1); }
    // Clock probe (measurement aid; wavenet_wg launches): workgroup 0 of every launch that follows records the shader-clock
    // counter and the constant-rate wall-clock counter at its start and end.  lastLaunchClockGHz(): shader ticks per wall
    // second of the latest launch = the clock the chip granted it under its power budget (0 when no launch was probed);
    // synchronises the device.
    void setClockProbe(bool on) {
        if (on && !m_clk) {
            gpuErrChk(hipMalloc(&m_clk, 4 * sizeof(unsigned long long)));
            gpuErrChk(hipMemset(m_clk, 0, 4 * sizeof(unsigned long long)));
        }
        m_clkOn = on;
    }
    double lastLaunchClockGHz() {
        if (!m_clk) return 0.0;
        unsigned long long c[4];
        gpuErrChk(hipDeviceSynchronize());
        gpuErrChk(hipMemcpy(c, m_clk, sizeof(c), hipMemcpyDeviceToHost));
        int dev = 0, wallKHz = 0;
        gpuErrChk(hipGetDevice(&dev));
        gpuErrChk(hipDeviceGetAttribute(&wallKHz, hipDeviceAttributeWallClockRate, dev));
        if (c[3] <= c[1] || wallKHz <= 0) return 0.0;
        return (double)(c[2] - c[0]) / (double)(c[3] - c[1]) * (double)wallKHz * 1e-6;
    }
    // The dilation ring on chip (north_star: "ring buffer staged in LDS with coalesced HBM spill"): wavenet_wg launches keep the slots
    // of the layers with the shortest dilations in the LDS their tables leave free, loaded from / spilled to the HBM ring at the
    // launch's ends.  mode >= 0 (default 0): as many layers as fit -- a model with a short maxDilation keeps its WHOLE ring on chip and
    // touches the HBM ring at the ends of a launch only; C3 (maxDilation 512) keeps d <= 4 / 2 / 1 / 1 at one / two / three / four tiles
    // per workgroup --; -1: never.  Samples are identical either way (tests/test_parity_gpu.py).
    void setRingInLds(int mode) { m_ringLdsMode = mode < 0 ? -1 : 0; }
    // The dilation schedule compiled into the kernel (see compiledSchedule): mode >= 0 (default 0): where a launch is eligible; -1: never
    // (every launch reads its schedule at run time).  Samples and ring are identical either way, so launches of both kinds mix.
    void setCompiledSchedule(int mode) { m_schedMode = mode < 0 ? -1 : 0; }
    // bound of every hand-off spin of the chain (default 1.5 s)
    void setChainTimeoutMs(double ms) { m_chainTimeoutTicks = (long long)(ms * 1e5); }

    // ---- model upload: fp32 in, host or device pointers, data is copied ---------------------
    // embedPrev / embedCur: [A][R]   (nv_wavenet.cuh:396-399)
    virtual void setEmbeddings(float* embedPrev, float* embedCur) {
        stageBegin((size_t)2 * A * R);
        convertTo(m_embedPrev, embedPrev, (size_t)A * R);
        convertTo(m_embedCur, embedCur, (size_t)A * R);
        gpuErrChk(hipStreamSynchronize(0));
    }
    // ---- in-kernel conditioning (beyond the reference class; SURVEY.md 8f rank 1 "feeding Lh directly") -------------------------
    // The model's conditioning convolution (cond_layers of pytorch/wavenet.py:73-74,197): Wcond [L][2R][nCond] (its weight
    // [2R*L][nCond][1] as it is), bcond [L][2R], fp32, host or device, copied.  With them and the upsampled features
    // (setConditioningFeatures / packFeatures) wavenet_wg computes Lh[t][l] = Wcond[l] c[t] + bcond[l] itself: the [N][L][B][2R]
    // tensor of setInputs is never built.  false: more channels than the kernels are built for (kCondChannelsMax).
    bool setConditioningWeights(const float* Wcond, const float* bcond, int nCond) {
        if (nCond <= 0 || nCond > wn::kCondChannelsMax) return false;
        const size_t nW = (size_t)m_numLayers * 2 * R * nCond, nB = (size_t)m_numLayers * 2 * R;
        stageBegin(nW + nB + 8);
        if (!m_condW) {
            gpuErrChk(hipMalloc(&m_condW, (size_t)m_numLayers * KC * 2 * R * sizeof(float)));
            gpuErrChk(hipMalloc(&m_condB, nB * sizeof(float)));
        }
        gpuErrChk(hipMemsetAsync(m_condW, 0, (size_t)m_numLayers * KC * 2 * R * sizeof(float), 0));
        const float* dW = onDevice(Wcond, nW);
        hipLaunchKernelGGL(wn::cond_weight_arrange_kernel, dim3(gridFor(nW)), dim3(256), 0, 0, m_condW, dW, m_numLayers, 2 * R, nCond, KC);
        gpuErrChk(hipGetLastError());
        gpuErrChk(hipMemcpyAsync(m_condB, bcond, nB * sizeof(float), hipMemcpyDefault, 0));
        gpuErrChk(hipStreamSynchronize(0));
        if (nCond != m_nCond) {
            // the upsampling table, its bias and the mel frames were packed for the old channel count: hand them over again
            m_upStride = 0;
            m_upWindow = 0;
            m_melFrames = 0;
        }
        m_nCond = nCond;
        m_featDirty = true;
        return true;
    }
    int conditioningChannels() const { return m_nCond; }
    int featureFragments() const { return KFC; }
    // elements (T_data) of numSamples samples of features in fragment order: numSamples x condTiles() x KFC x 64 x EPL
    size_t featureElems(int numSamples) const { return (size_t)numSamples * m_tiles * KFC * C::FRAG_ELEMS; }
    // Features the caller has produced in fragment order (device memory, T_data; pack_features_kernel documents the order):
    // used in place, kept alive and unchanged until the runs that follow have completed.  Resets the history like setInputs.
    void setConditioningFeatures(const void* frags, int numSamples) {
        assert(numSamples > 0 && numSamples <= m_maxSamples && m_nCond > 0);
        assert(isDevicePtr(frags));
        resetHistory(0);
        gpuErrChk(hipStreamSynchronize(0));
        dropLhConditioning();
        m_featPtr = frags;
        m_featSamples = numSamples;
    }
    // Samples [firstSample, firstSample + count) of the features from a device tensor of `precision`-bit floats addressed as
    // x[b * bStride + c * cStride + (t - firstSample) * tStride] (the model's upsample output [B][nCond][T] has strides (nCond*T, T, 1);
    // channels-last [B][T][nCond] works as well), into the engine's own buffer, asynchronously on `stream`.  History untouched.
    void packFeatures(const void* x, int precision, long long bStride, long long cStride, long long tStride, int firstSample, int count,
                      hipStream_t stream = 0) {
        assert(firstSample >= 0 && count > 0 && firstSample + count <= m_maxSamples && m_nCond > 0);
        assert(precision == 32 || precision == 16);
        assert(isDevicePtr(x));
        if (!m_feat) {
            gpuErrChk(hipMalloc(&m_feat, featureElems(m_maxSamples) * sizeof(elem)));
            gpuErrChk(hipMemsetAsync(m_feat, 0, featureElems(m_maxSamples) * sizeof(elem), stream));
            gpuErrChk(hipStreamSynchronize(stream));
        }
        dropLhConditioning();
        m_featPtr = m_feat;
        m_featSamples = m_maxSamples;      // (run_partial of a chunk only reads what has been packed: the caller's ordering, as with packConditioning)
        const int tilesUsed = (m_maxBatch + 15) / 16;
        const size_t nblk = (size_t)tilesUsed * ((count + 7) / 8);
        hipLaunchKernelGGL((wn::pack_features_kernel<F16>), dim3((unsigned)(nblk > 65536 ? 65536 : nblk)), dim3(256), 0, stream,
                           m_feat + featureElems(firstSample), x, precision, bStride, cStride, tStride, m_nCond, m_maxBatch, count, m_tiles,
                           tilesUsed);
        gpuErrChk(hipGetLastError());
    }
    // the whole utterance at once (resets the history like setInputs; synchronises)
    void setFeatures(const void* x, int precision, long long bStride, long long cStride, long long tStride, int numSamples) {
        resetHistory(0);
        packFeatures(x, precision, bStride, cStride, tStride, 0, numSamples, 0);
        gpuErrChk(hipStreamSynchronize(0));
    }
    bool conditioningFromFeatures() const { return m_featPtr != NULL; }
    // ---- ... and the upsampling in front of it (the other half of WaveNet.get_cond_input, pytorch/wavenet.py:195-197) -----------
    // The model's `upsample` ConvTranspose1d: upW [nCond][nCond][window], upB [nCond], fp32, host or device, copied; window must be a
    // multiple of stride (the reference's 800 / 200), at most 5 strides.  Needs setConditioningWeights first (the channel count).
    static constexpr int kUpMaxTaps = 5;      // (the operands of a workgroup's phases sit in LDS: phases x 5 x taps x KFC KiB <= 160 KiB)
    bool setUpsampling(const float* upW, const float* upB, int window, int stride) {
        if (m_nCond <= 0 || stride <= 0 || window < stride || window % stride != 0 || window / stride > kUpMaxTaps) return false;
        const size_t nW = (size_t)m_nCond * m_nCond * window;
        stageBegin(nW + 128);
        if (m_upTab) gpuErrChk(hipFree(m_upTab));
        const size_t tabElems = (size_t)stride * wn::kUpRowTiles * (window / stride) * KFC * C::FRAG_ELEMS;
        gpuErrChk(hipMalloc(&m_upTab, tabElems * sizeof(elem)));
        if (!m_upBias) gpuErrChk(hipMalloc(&m_upBias, wn::kUpRowTiles * 16 * sizeof(float)));
        gpuErrChk(hipMemsetAsync(m_upBias, 0, wn::kUpRowTiles * 16 * sizeof(float), 0));
        const float* dW = onDevice(upW, nW);
        hipLaunchKernelGGL((wn::pack_upsample_kernel<F16>), dim3(gridFor(tabElems)), dim3(256), 0, 0, m_upTab, dW, m_nCond, window, stride);
        gpuErrChk(hipGetLastError());
        gpuErrChk(hipMemcpyAsync(m_upBias, upB, m_nCond * sizeof(float), hipMemcpyDefault, 0));
        // (per engine, hence per device: the attribute belongs to the device's copy of the kernel)
        gpuErrChk(hipFuncSetAttribute((const void*)wn::upsample_features_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        gpuErrChk(hipStreamSynchronize(0));
        if (stride != m_upStride) m_melFrames = 0;      // frames handed over for another stride were checked against that stride
        m_upWindow = window;
        m_upStride = stride;
        return true;
    }
    int upsamplingStride() const { return m_upStride; }
    int melSamples() const { return m_melFrames * m_upStride; }      // samples the frames handed over with setMel upsample to (0: none)
    bool hasFeatureBuffer() const { return m_feat != NULL; }         // the engine's own feature buffer exists (packFeatures / upsampleFeatures)
    int maxBatch() const { return m_maxBatch; }
    // debug getter: samples [firstSample, firstSample + count) of the engine's own feature buffer (fragment order, T_data) -> dst
    void getFeatures(void* dst, int firstSample, int count) {
        assert(m_feat != NULL && firstSample >= 0 && count > 0 && firstSample + count <= m_maxSamples);
        gpuErrChk(hipDeviceSynchronize());
        gpuErrChk(hipMemcpy(dst, m_feat + featureElems(firstSample), featureElems(count) * sizeof(elem), hipMemcpyDefault));
    }
    // The utterances' features before upsampling ("mel frames"): device tensor of `precision`-bit floats addressed
    // x[b * bStride + c * cStride + f * fStride], frames <= maxSamples / stride; copied (into fragment order).  Resets the history like
    // setInputs: the start of an utterance batch.
    void setMel(const void* mel, int precision, long long bStride, long long cStride, long long fStride, int frames) {
        assert(m_upStride > 0 && frames > 0 && (long long)frames * m_upStride <= m_maxSamples);
        assert(isDevicePtr(mel) && (precision == 32 || precision == 16));
        if (frames > m_melCap) {
            if (m_melFrag) gpuErrChk(hipFree(m_melFrag));
            m_melCap = m_maxSamples / m_upStride;
            gpuErrChk(hipMalloc(&m_melFrag, featureElems(m_melCap) * sizeof(elem)));
        }
        resetHistory(0);
        const int tilesUsed = (m_maxBatch + 15) / 16;
        gpuErrChk(hipMemsetAsync(m_melFrag, 0, featureElems(frames) * sizeof(elem), 0));      // (tiles beyond the batch: zero frames)
        const size_t nblk = (size_t)tilesUsed * ((frames + 7) / 8);
        hipLaunchKernelGGL((wn::pack_features_kernel<F16>), dim3((unsigned)(nblk > 65536 ? 65536 : nblk)), dim3(256), 0, 0, m_melFrag, mel, precision,
                           bStride, cStride, fStride, m_nCond, m_maxBatch, frames, m_tiles, tilesUsed);
        gpuErrChk(hipGetLastError());
        gpuErrChk(hipStreamSynchronize(0));
        m_melFrames = frames;
    }
    // Samples [firstSample, firstSample + count) of the upsampled features from the frames handed over with setMel, into the engine's
    // feature buffer, asynchronously on `stream` (one MFMA kernel: upsample_features_kernel); the runs that follow read them.
    void upsampleFeatures(int firstSample, int count, hipStream_t stream = 0) {
        assert(m_upStride > 0 && m_melFrames > 0);
        assert(firstSample >= 0 && count > 0 && firstSample + count <= m_melFrames * m_upStride);
        if (!m_feat) {
            gpuErrChk(hipMalloc(&m_feat, featureElems(m_maxSamples) * sizeof(elem)));
            gpuErrChk(hipMemsetAsync(m_feat, 0, featureElems(m_maxSamples) * sizeof(elem), stream));
            gpuErrChk(hipStreamSynchronize(stream));
        }
        dropLhConditioning();
        m_featPtr = m_feat;
        m_featSamples = m_melFrames * m_upStride;
        const int m = m_upWindow / m_upStride, tilesUsed = (m_maxBatch + 15) / 16;
        const size_t lds = (size_t)wn::up_phases<F16>() * wn::kUpRowTiles * m * KFC * 1024;      // (a pair of phases in fp16)
        // a phase per workgroup; phases with few columns (long strides, short chunks) get more workgroups per phase
        const int pairs = (m_upStride + wn::up_phases<F16>() - 1) / wn::up_phases<F16>();
        const int gx = pairs < 1024 ? pairs : 1024;
        const long long cols = (long long)((count + m_upStride - 1) / m_upStride + 1) * tilesUsed;
        int gy = (int)((cols + 255) / 256);         // (a wave takes groups of two or four columns)
        const int gyMax = (1024 + gx - 1) / gx;
        if (gy > gyMax) gy = gyMax;
        if (gy < 1) gy = 1;
        hipLaunchKernelGGL((wn::upsample_features_kernel<F16>), dim3(gx, gy), dim3(64 * wn::up_waves<F16>()), lds, stream, m_feat, m_melFrag, m_upTab, m_upBias, m, m_upStride,
                           m_tiles, tilesUsed, firstSample, count);
        gpuErrChk(hipGetLastError());
    }
    // Features in, samples out (role of pytorch/inference.py:40-62 around run_chunks, nv_wavenet.cuh:445-497): the whole utterance
    // batch chunk by chunk -- upsampling of a chunk's features, its generation launch, the copy of its samples (and PCM) on a second
    // stream, consume(yOut, first, count) on the calling thread -- from the frames handed over with setMel.  Selectors: the seed or
    // table in force.  num_samples <= frames * stride.
    template <class Callback>
    bool run_stream(int num_samples_per_chunk, Callback consume, int num_samples, int batch_size, int* yOut = NULL, hipStream_t stream = 0) {
        assert(num_samples_per_chunk > 0 && m_melFrames > 0 && num_samples <= m_melFrames * m_upStride);
        struct Piece {
            int first, count;
            hipEvent_t generated, delivered;
        };
        std::vector<Piece> pieces;
        for (int first = 0; first < num_samples; first += num_samples_per_chunk) {
            Piece pc;
            pc.first = first;
            pc.count = num_samples - first < num_samples_per_chunk ? num_samples - first : num_samples_per_chunk;
            pc.generated = pooledEvent(2 * pieces.size());
            pc.delivered = pooledEvent(2 * pieces.size() + 1);
            pieces.push_back(pc);
        }
        // (the events are the engine's, made once.  A second stream exists only where it buys something: when the samples or the PCM
        //  go to HOST memory, so that the copy of a chunk overlaps the generation of the next; device-resident outputs are copied in
        //  stream order, 20 us per chunk.  Made per call and destroyed at its end -- 1.4 ms -- because streams kept alive in the engine
        //  take hardware queues away from the caller's own streams: with them pooled, a launch on a caller's side stream queued up
        //  behind a kernel of another of its streams, tests/..::test_chain_launch_that_cannot_become_resident..)
        const bool hostOut = (yOut != NULL && !isDevicePtr(yOut)) || (m_pcmUser != NULL && !isDevicePtr(m_pcmUser));
        hipStream_t genStream = stream, outStream = stream;
        const bool ownGen = hostOut && !stream;
        if (ownGen) gpuErrChk(hipStreamCreate(&genStream));
        if (hostOut) gpuErrChk(hipStreamCreate(&outStream));
        bool ok = true;
        for (size_t k = 0; k < pieces.size(); k++) {
            const Piece& pc = pieces[k];
            // (the generation kernel holds every CU for the length of its launch: the upsampling of a chunk runs in front of it on the
            //  same stream -- 1 to 2 % of the chunk's time -- instead of beside it)
            upsampleFeatures(pc.first, pc.count, genStream);
            m_num_samples_per_chunk = pc.count;
            ok = run_partial(pc.first, num_samples, batch_size, NULL, 1, false, genStream) && ok;
            gpuErrChk(hipEventRecord(pc.generated, genStream));
            if (hostOut) gpuErrChk(hipStreamWaitEvent(outStream, pc.generated, 0));
            if (yOut) getYOut(yOut, pc.first, pc.count, outStream);
            if (m_pcmUser) getAudioOut(m_pcmUser, pc.first, pc.count, outStream);
            gpuErrChk(hipEventRecord(pc.delivered, outStream));
        }
        m_num_samples_per_chunk = 0;
        for (size_t k = 0; k < pieces.size(); k++) {
            gpuErrChk(hipEventSynchronize(pieces[k].delivered));
            consume(yOut, pieces[k].first, pieces[k].count);
        }
        if (ownGen) gpuErrChk(hipStreamDestroy(genStream));
        if (hostOut) gpuErrChk(hipStreamDestroy(outStream));
        return ok;
    }
    // col-major Wprev,Wcur 2RxR; Bh 2R; Wres RxR; Bres R; Wskip SxR; Bskip S (nv_wavenet.cuh:400-409)
    virtual void setLayerWeights(int layer, float* Wprev, float* Wcur, float* Bh, float* Wres, float* Bres,
                                 float* Wskip, float* Bskip) {
        assert(layer >= 0 && layer < m_numLayers);
        stageBegin((size_t)5 * R * R + (size_t)S * R + 3 * R + S + 32);
        float* b = m_bias + (size_t)layer * C::BIAS_L;
        // one launch packs the four matrices and the three bias vectors of the layer
        wn::LayerSrc src;
        src.Wprev = onDevice(Wprev, (size_t)2 * R * R);
        src.Wcur = onDevice(Wcur, (size_t)2 * R * R);
        src.Bh = onDevice(Bh, 2 * R);
        src.Wres = onDevice(Wres, (size_t)R * R);
        src.Bres = onDevice(Bres, R);
        src.Wskip = onDevice(Wskip, (size_t)S * R);
        src.Bskip = onDevice(Bskip, S);
        hipLaunchKernelGGL((wn::pack_layer_kernel<F16>), dim3(gridFor((size_t)5 * R * R + (size_t)S * R)), dim3(256), 0, 0,
                           m_wblob, b, src, R, S, C::NW, C::waveStreamFrags(m_numLayers) * C::FRAG_ELEMS,
                           (int)C::streamPos(layer, C::O_PREV, m_numLayers), (int)C::streamPos(layer, C::O_CUR, m_numLayers),
                           (int)C::streamPos(layer, C::O_RES, m_numLayers), (int)C::streamPos(layer, C::O_SKIP, m_numLayers));
        gpuErrChk(hipGetLastError());
        gpuErrChk(hipStreamSynchronize(0));
        m_featDirty = true;
    }
    // col-major Wzs AxS, Bzs A, Wza AxA, Bza A (nv_wavenet.cuh:410-415)
    virtual void setOutWeights(float* Wzs, float* Bzs, float* Wza, float* Bza) {
        stageBegin((size_t)A * S + (size_t)A * A + 16);
        const size_t hf = C::headOffsetFrags(m_numLayers);
        packWeight(hf + C::O_ZS, Wzs, A, S, 0);
        packWeight(hf + C::O_ZA, Wza, A, A, 0);
        gpuErrChk(hipMemcpyAsync(headBias(), Bzs, A * sizeof(float), hipMemcpyDefault, 0));
        gpuErrChk(hipMemcpyAsync(headBias() + A, Bza, A * sizeof(float), hipMemcpyDefault, 0));
        gpuErrChk(hipStreamSynchronize(0));
        m_featDirty = true;
    }

    // Lh: [maxSamples][L][maxBatch][2R] conditioning, outputSelectors: [maxSamples][maxBatch]
    // uniform draws; resets the sample history to 128 (nv_wavenet.cuh:417-422).
    void setInputs(float* Lh, float* outputSelectors) { setInputs(Lh, outputSelectors, m_maxSamples); }
    // Same with numSamples <= maxSamples rows of Lh / outputSelectors (an utterance shorter than the
    // engine's capacity: both layouts are sample-major, so a prefix is a valid input)
    void setInputs(float* Lh, float* outputSelectors, int numSamples) {
        setConditioning(Lh, numSamples);
        m_useRng = false;
        gpuErrChk(hipMemcpy(m_outputSelectors, outputSelectors, (size_t)numSamples * m_maxBatch * sizeof(float),
                            hipMemcpyDefault));
    }

    // ---- extensions beyond the reference --------------------------------
    // The conditioning half of setInputs (also resets the history to 128); pair it with
    // setSelectorSeed() and no [N][B] selector matrix is ever built or uploaded.
    void setConditioning(float* Lh) { setConditioning(Lh, m_maxSamples); }
    void setConditioning(float* Lh, int numSamples, hipStream_t stream = 0) {
        assert(numSamples > 0 && numSamples <= m_maxSamples);
        resetHistory(stream);
        packConditioning(Lh, 0, numSamples, stream);
        gpuErrChk(hipStreamSynchronize(stream));
    }
    // Packs samples [firstSample, firstSample + count) of the conditioning (Lh points at sample firstSample)
    // into the engine's fragment order, asynchronously on `stream` when Lh is device memory: lets a caller
    // stream the conditioning chunk by chunk behind run_partial() of the previous chunk.  From here on the engine
    // reads the packed copy (a tensor handed over with setConditioningDirect is let go).
    void packConditioning(float* Lh, int firstSample, int count, hipStream_t stream = 0) {
        assert(firstSample >= 0 && count > 0 && firstSample + count <= m_maxSamples);
        m_condRaw = NULL;
        m_condRawKind = 0;
        m_condUser = NULL;
        m_featPtr = NULL;
        const size_t rows = (size_t)count * m_numLayers;
        const size_t srcPerRow = (size_t)m_maxBatch * 2 * R;
        const size_t dstPerRow = (size_t)m_tiles * 16 * 2 * R;
        if (!m_cond) {
            const size_t condElems = (size_t)(m_maxSamples + 1) * m_numLayers * dstPerRow;   // + one padding sample
            gpuErrChk(hipMalloc(&m_cond, condElems * sizeof(elem)));
            // zeroed before ANY stream may pack into it (a later chunk packed on another stream must not be overtaken by this)
            gpuErrChk(hipMemsetAsync(m_cond, 0, condElems * sizeof(elem), stream));
            gpuErrChk(hipStreamSynchronize(stream));
        }
        elem* const dst0 = m_cond + (size_t)firstSample * m_numLayers * dstPerRow;
        const bool dev = isDevicePtr(Lh);
        // host sources go through the staging buffer in chunks of <= 64 Mi floats
        size_t chunkRows = dev ? rows : ((size_t)64 << 20) / srcPerRow;
        if (chunkRows < 1) chunkRows = 1;
        if (!dev) stageBegin((chunkRows < rows ? chunkRows : rows) * srcPerRow);
        for (size_t r0 = 0; r0 < rows; r0 += chunkRows) {
            const size_t nr = (rows - r0 < chunkRows) ? rows - r0 : chunkRows;
            const float* src = Lh + r0 * srcPerRow;
            if (!dev) {
                gpuErrChk(hipStreamSynchronize(stream));   // the previous chunk's kernel has read the staging buffer
                gpuErrChk(hipMemcpy(m_stage, src, nr * srcPerRow * sizeof(float), hipMemcpyHostToDevice));
                src = m_stage;
            }
            // one workgroup per (row, tile): 16 utterances x 2R channels, read and written coalesced
            const size_t nblk = nr * (size_t)m_tiles;
            const int grid = (int)(nblk > 65536 ? 65536 : nblk);
            hipLaunchKernelGGL((wn::pack_cond_tiled_kernel<F16, R>), dim3(grid), dim3(256), 0, stream, dst0 + r0 * dstPerRow, src, nr,
                               m_maxBatch, m_tiles);
            gpuErrChk(hipGetLastError());
        }
    }
    // Device-resident conditioning WITHOUT the copy (the reference's own recommendation, README.md:44; SURVEY.md 8f
    // rank 1): Lh is the caller's [numSamples][L][maxBatch][2R] tensor in device memory, fp32 (precision = 32) or -- fp16
    // engine -- T_data = fp16 (precision = 16: half the bytes; the reference keeps m_Lh in T_data, nv_wavenet.cuh:326); the
    // kernels read it in place (16 / 8 bytes per lane and gate tile) and nothing is packed.  The caller keeps it alive and
    // unchanged until the run calls that follow have completed.  Resets the sample history like setInputs.  Host pointers
    // (fp32 only) fall back to setConditioning.
    void setConditioningDirect(const void* Lh, int numSamples, int precision = 32) {
        assert(numSamples > 0 && numSamples <= m_maxSamples);
        assert(precision == 32 || (precision == 16 && F16));
        if (!isDevicePtr(Lh)) {
            assert(precision == 32);
            setConditioning((float*)Lh, numSamples);
            return;
        }
        resetHistory(0);
        gpuErrChk(hipStreamSynchronize(0));
        m_condRaw = Lh;
        m_condRawKind = precision == 16 ? 2 : 1;
        m_condRawSamples = numSamples;
        m_condUser = NULL;
        m_featPtr = NULL;
    }
    // Conditioning that the caller has PRODUCED in the engine's own fragment order (round 3): T_data
    // [numSamples + 1][L][condTiles()][wave][fragment][lane][EPL], gate rows pre-scaled -- exactly what packConditioning writes
    // (pack_cond_tiled_kernel documents the order; nv_wavenet_amd/nv_wavenet.py: cond_fragment_order / get_cond_input(layout=
    // "packed") produce it from the model's conditioning convolution by permuting and scaling that convolution's output
    // channels, i.e. for free).  The generation kernels then run their packed path on the caller's buffer: no copy, no second
    // pass, no in-place conversions -- the headline kernel as it is.  The buffer holds one padding sample past the last (the
    // prefetch reads ahead), stays alive and unchanged until the runs that follow have completed.  Resets the history.
    void setConditioningPacked(const void* frags, int numSamples) {
        assert(numSamples > 0 && numSamples <= m_maxSamples);
        assert(isDevicePtr(frags));
        resetHistory(0);
        gpuErrChk(hipStreamSynchronize(0));
        m_condRaw = NULL;
        m_condRawKind = 0;
        m_featPtr = NULL;
        m_condUser = frags;
        m_condUserSamples = numSamples;      // (run_partial refuses to generate past what the caller handed over)
    }
    // elements (T_data) a packed buffer of numSamples samples must hold: (numSamples + 1) x L x condTiles() x 16 x 2R
    size_t condPackedElems(int numSamples) const { return (size_t)(numSamples + 1) * m_numLayers * m_tiles * 16 * 2 * R; }
    // tiles of 16 utterances per (sample, layer) row of the packed conditioning (the batch rounded up to whole workgroups)
    int condTiles() const { return m_tiles; }
    bool conditioningInPlace() const { return m_condRaw != NULL; }
    // the selector half of setInputs: [numSamples][maxBatch] uniform draws (host or device), conditioning and history untouched
    void setSelectors(float* outputSelectors, int numSamples) {
        assert(numSamples > 0 && numSamples <= m_maxSamples);
        m_useRng = false;
        gpuErrChk(hipMemcpy(m_outputSelectors, outputSelectors, (size_t)numSamples * m_maxBatch * sizeof(float), hipMemcpyDefault));
    }
    // Selectors are drawn inside the kernel: Philox4x32-10, counter {sample, utterance, 0, 0}, key =
    // seed (replaces the rand() table of pytorch/wavenet_infer.cu:92-94).  A later setInputs()
    // returns to the uploaded table.
    void setSelectorSeed(unsigned long long seed) {
        m_useRng = true;
        m_rngSeed = seed;
    }
    // int16 PCM beside the indices: pcm[b][t] = int16(32768 * mu_law_decode(y[b][t], A))
    // (pytorch/utils.py:62-70, inference.py:58-60).  pcmOut: caller-owned [batch][num_samples] int16 of the run calls
    // that follow, host or device; filled by run / run_partial / run_chunks wherever yOut is; NULL disables.
    // pcmElems: the buffer's size in int16 values (0 = not stated); a stated size is checked by every run call.
    void setAudioOut(short* pcmOut, size_t pcmElems = 0) {
        m_pcmUser = pcmOut;
        m_pcmUserElems = pcmOut ? pcmElems : 0;
        if (pcmOut && !m_pcm) {
            gpuErrChk(hipMalloc(&m_pcm, (size_t)m_maxSamples * m_maxBatch * sizeof(short)));
            gpuErrChk(hipMemset(m_pcm, 0, (size_t)m_maxSamples * m_maxBatch * sizeof(short)));
            ensureMulaw();
        }
    }
    // the PCM value of every sample index, on the device (made once)
    void ensureMulaw() {
        if (!m_mulaw) {
            std::vector<short> table(A);
            const double mu = (double)A - 1.0;
            for (int y = 0; y < A; y++) {
                const double signal = 2.0 * ((double)y / mu) - 1.0;
                const double magnitude = (1.0 / mu) * (std::pow(1.0 + mu, std::fabs(signal)) - 1.0);
                const double v = 32768.0 * (signal > 0 ? magnitude : (signal < 0 ? -magnitude : 0.0));
                // Truncation like numpy's astype('int16') in the reference's inference.py:58-60, INCLUDING its
                // wrap of the top bin (y = A-1 -> +32768 -> -32768): kept on purpose, this output is pinned
                // bit for bit to the reference's own utils.py / inference.py (tests/golden/mulaw_pcm.npz)
                table[y] = (short)(int)v;
            }
            gpuErrChk(hipMalloc(&m_mulaw, A * sizeof(short)));
            gpuErrChk(hipMemcpy(m_mulaw, table.data(), A * sizeof(short), hipMemcpyHostToDevice));
        }
    }
    void getAudioOut(short* pcm, int offset, int size, hipStream_t stream = 0) {
        gpuErrChk(hipMemcpy2DAsync(pcm + offset, m_lastStride * sizeof(short), m_pcm + offset,
                                   m_lastStride * sizeof(short), size * sizeof(short), m_maxBatch, hipMemcpyDefault,
                                   stream));
    }

    // Which device code run(num_samples, batch_size, ..., dumpActivations) launches: kernel name with its
    // template arguments, tiles per workgroup, workgroups, dynamic LDS bytes (for benchmarks / logs).
    void kernelInfo(int batch_size, bool dumpActivations, char* buf, int n) const {
        const int tiles = (batch_size + 15) / 16;
        const bool feat = m_featPtr != NULL || m_slots->active();      // (a slot-mode step launches wavenet_wg<.., RAW=3> as the features path)
        const bool chainLaunch = isChain() && !feat;
        const bool dump = dumpActivations || (!F16 && !chainLaunch && (feat || m_condRaw));      // (see launch())
        if (chainLaunch) {
            const int perLaunch = m_numCUs / m_chainStages, chains = tiles < perLaunch ? tiles : perLaunch;
            const int tpcNow = chainTpc((m_maxBatch + 15) / 16);
            snprintf(buf, n, "wn::wavenet_chain<%s,%d,%d,%d,DUMP=%d%s> stages=%d layers/stage=%d chains=%d tiles/chain=%d wgs=%d lds=%zu",
                     F16 ? "fp16" : "fp32", R, S, A, dump ? 1 : 0, (!dump && chainHoists(tpcNow)) ? ",HOIST=1" : "", m_chainStages, m_chainLpc, chains, tpcNow,
                     m_chainStages * chains, CC::ldsBytes());
            return;
        }
        const int raw = feat ? 3 : m_condRaw ? m_condRawKind : 0;
        const int bt = launchTiles(tiles, dump, raw);
        int nEmb = planEmb<1>(dump, raw);
        size_t lds = ldsNeed<1>(m_numLayers, nEmb, dump);
        if constexpr (WG2) {
            if (bt == 2) {
                nEmb = planEmb<2>(dump, raw);
                lds = ldsNeed<2>(m_numLayers, nEmb, dump);
            }
        }
        if constexpr (WG3) {
            if (bt == 3) {
                nEmb = planEmb<3>(dump, raw);
                lds = ldsNeed<3>(m_numLayers, nEmb, dump);
            }
            if (bt == 4) {
                nEmb = planEmb<4>(dump, raw);
                lds = ldsNeed<4>(m_numLayers, nEmb, dump);
            }
        }
        // ring slots in LDS (ringPlan): the largest dilation held there, 0 = the launch keeps the whole ring in HBM
        int ringD = 0;
        {
            wn::Params q;
            fillSchedule(q);
            size_t rb = 0;
            if (bt == 1) rb = ringPlan<1>(q, lds, dump, raw);
            if constexpr (WG2) {
                if (bt == 2) rb = ringPlan<2>(q, lds, dump, raw);
            }
            if constexpr (WG3) {
                if (bt == 3) rb = ringPlan<3>(q, lds, dump, raw);
                if (bt == 4) rb = ringPlan<4>(q, lds, dump, raw);
            }
            lds += rb;
            ringD = q.ldsRingD;
        }
        // compiled dilation schedule (compiledSchedule): its kernels hold d <= 2 at the most
        const int ld = compiledSchedule(bt, dump, raw, ringD);
        if (ld > 0) ringD = 1 << (ld - 1);
        char ring[64] = "";
        if (ringD > 0) snprintf(ring, sizeof(ring), " ring_in_lds=d<=%d%s", ringD, ld > 0 ? (straightLine() ? " cycles=2 sched=cycle10" : " sched=cycle10") : "");
        snprintf(buf, n, "wn::wavenet_wg<%s,%d,%d,%d,BT=%d,EMBLDS=%d,DUMP=%d,RAW=%d%s> tiles/wg=%d wgs=%d lds=%zu%s",
                 F16 ? "fp16" : "fp32", R, S, A, bt, nEmb, dump ? 1 : 0, raw, ringD > 0 ? ",LR=1" : "", bt, (tiles + bt - 1) / bt, lds, ring);
    }

    // ---- debug getters: last generated sample's activations, reference layouts --------------
    void getXtOut(int layer, float* hXt) {
        gpuErrChk(hipMemcpy(hXt, m_XtOut + (size_t)layer * m_maxBatch * R, (size_t)m_maxBatch * R * sizeof(float),
                            hipMemcpyDefault));
    }
    void getSkipOut(int layer, float* hSkipOut) {
        gpuErrChk(hipMemcpy(hSkipOut, m_skipOut + (size_t)layer * m_maxBatch * S,
                            (size_t)m_maxBatch * S * sizeof(float), hipMemcpyDefault));
    }
    void getZs(float* hZs) { gpuErrChk(hipMemcpy(hZs, m_Zs, (size_t)m_maxBatch * A * sizeof(float), hipMemcpyDefault)); }
    void getZa(float* hZa) { gpuErrChk(hipMemcpy(hZa, m_Za, (size_t)m_maxBatch * A * sizeof(float), hipMemcpyDefault)); }
    void getP(float* hP) { gpuErrChk(hipMemcpy(hP, m_p, (size_t)m_maxBatch * A * sizeof(float), hipMemcpyDefault)); }
    // Columns [offset, offset + size) of every utterance's row, device -> caller (host or device),
    // asynchronously on `stream` (role of nv_wavenet.cuh:439-444): the sample buffer is [batch][stride]
    // on both sides, so this is one strided 2-D copy of `size` ints per row.
    void getYOut(int* yOut, int offset, int size, hipStream_t stream = 0) {
        const size_t rowBytes = (size_t)m_lastStride * sizeof(int);
        gpuErrChk(hipMemcpy2DAsync(yOut + offset, rowBytes, m_yOut + offset, rowBytes, (size_t)size * sizeof(int),
                                   (size_t)m_maxBatch, hipMemcpyDefault, stream));
    }

    // ---- sampling temperature (beyond the reference; slots_sampler.hpp) ------------------------------------------
    // Column b of the runs that follow samples from softmax(logits / T[b]), b < n; the columns past n, and all of them with
    // T == NULL, from softmax(logits) as before.  T: a host array, 1 <= n <= maxBatch, every value finite and in [2^-10, 2^10].
    // The values stay in force across setFeatures / setMel / resetHistory and between run_partial chunks until the next call; a
    // call between two chunks takes effect at the next chunk and leaves the history alone.  They reach every launch of the
    // features path (the conditioning computed in the kernel); while any column's T is not 1 a run on packed or in-place
    // conditioning, or on a multi-CU engine, prints one line and returns false.  T = 1 is bit-identical to never having called
    // this; for T a power of two the samples are those of the model with Wza / T and Bza / T.  Greedy (argmax) decoding is not
    // offered: T = 2^-10 approaches it, but still draws between logits that tie at the maximum.  Synchronises.
    // false (nothing changes): in slot mode (slotSetTemperature is the call there), n outside the batch with a non-NULL T, or a
    // bad value.
    bool setTemperatures(const float* T, int n) { return setSampling(&wn::Sampling::temperature, T, n, wn::temperature_ok); }
    // the temperature in force for column b (1 when none was ever set)
    float temperature(int b) const { return m_temps.get(b).temperature; }
    // Params::floorOn of a features-path launch: bit 0, a floor other than 0 is in force; bit 1, a tail cut (either has made the table)
    int floorMask() const { return (m_temps.on[wn::kMinP] > 0 ? 1 : 0) | (m_temps.cutting() > 0 ? 2 : 0); }

    // ---- probability floor, min-p (beyond the reference; slots_sampler.hpp) ----------------------------------------
    // Column b of the runs that follow draws from its tempered distribution WITHOUT the bins whose probability is below minP[b] times
    // that of the most probable bin, renormalised; b < n; the columns past n, and all of them with minP == NULL, from the whole
    // distribution as before.  minP: a host array, 1 <= n <= maxBatch, every value finite and in [0, 0.5].  Everything else as
    // setTemperatures: in force until the next call, a call between two chunks takes effect at the next chunk, only the features
    // path honours it and the other paths refuse while any floor is not 0; floor 0 is bit-identical to never having called this.
    // Synchronises.  false (nothing changes): in slot mode (slotSetMinP is the call there), n outside the batch, or a bad value.
    bool setMinP(const float* minP, int n) { return setSampling(&wn::Sampling::minP, minP, n, wn::min_p_ok); }
    // the floor in force for column b (0 when none was ever set)
    float minP(int b) const { return m_temps.get(b).minP; }

    // ---- tail cuts, top-k and top-p (beyond the reference; slots_sampler.hpp) ---------------------------------------
    // Column b of the runs that follow draws from the topK[b] most probable bins of its tempered distribution (0: off), and from the
    // smallest set of most probable bins whose mass reaches topP[b] (1: off), ties at either boundary included; the cuts and the
    // floor intersect, each defined on the full tempered distribution.  b < n; the columns past n, and all of them with a NULL
    // array, are off.  Host arrays, 1 <= n <= maxBatch; topK in [0, A]; topP finite and in (0, 1].  Everything else as setMinP, and
    // none of the three calls resets another's values; with every column off the runs are bit-identical to never having called
    // these.  Synchronises.  false (nothing changes): in slot mode (slotSetTopK / slotSetTopP are the calls there), n outside the
    // batch, or a bad value.
    bool setTopK(const int* topK, int n) {
        return setSampling(&wn::Sampling::topK, topK, n, [](int k) { return wn::top_k_ok(k, A); });
    }
    bool setTopP(const float* topP, int n) { return setSampling(&wn::Sampling::topP, topP, n, wn::top_p_ok); }
    // the cuts in force for column b (0 and 1 when none was ever set)
    int topK(int b) const { return m_temps.get(b).topK; }
    float topP(int b) const { return m_temps.get(b).topP; }
private:
    // The four lockstep setters: every value is checked before anything changes, the other three kinds stay as they are.
    template <class V, class Ok>
    bool setSampling(V wn::Sampling::*field, const V* v, int n, Ok ok) {
        if (m_slots->active()) return false;
        if (v != NULL) {
            if (n < 1 || n > m_maxBatch) return false;
            for (int b = 0; b < n; b++)
                if (!ok(v[b])) return false;
        }
        gpuErrChk(hipDeviceSynchronize());
        m_temps.resetKind(field);
        for (int b = 0; v != NULL && b < n; b++) {
            wn::Sampling s = m_temps.get(b);
            s.*field = v[b];
            m_temps.set(b, s);
        }
        m_temps.upload();
        return true;
    }
public:

    // ---- primed generation (beyond the reference; slots_prime.hpp) -------------------------------------------------
    // Column b < batch of the runs that follow starts with the forced samples y[b * stride + k], k < n[b] (0 <= n[b] <= maxN <=
    // maxSamples; 0: not primed): they are delivered and fed back like drawn samples, and from sample n[b] on the column draws as
    // always -- selector {t, b} of the seed, or row t of the uploaded table.  y: int32, host or device, maxN values per column, stride
    // >= maxN; copied.  y == NULL clears.  In force across setFeatures / setMel / resetHistory and between run_partial chunks until the
    // next call.  A launch whose range holds a forced sample reads an engine-owned second selector table, filled for its rows by one
    // small launch ahead of it (prime_selectors); the caller's table is never written, and a launch past every prime is what it was.
    // Only the features path honours a prime: while one is in force a run on packed or in-place conditioning, or a chain launch,
    // prints one line and returns false.  Synchronises.  false (nothing changes): in slot mode (slotPrime is the call there), batch
    // outside 1 .. maxBatch, maxN outside 0 .. maxSamples, stride < maxN, an n[b] outside 0 .. maxN, or a value outside 0 .. A-1 in host
    // memory (device values are clamped into that range by the kernel).
    bool setPrime(const int* y, const int* n, int batch, int maxN, long long stride) {
        if (m_slots->active()) return false;
        if (y == NULL) {
            gpuErrChk(hipDeviceSynchronize());
            m_prime.clear();
            return true;
        }
        if (n == NULL || batch < 1 || batch > m_maxBatch || maxN < 0 || maxN > m_maxSamples || stride < maxN) return false;
        for (int b = 0; b < batch; b++)
            if (n[b] < 0 || n[b] > maxN) return false;
        if (!isDevicePtr(y))
            for (int b = 0; b < batch; b++)
                for (int k = 0; k < n[b]; k++)
                    if (y[b * stride + k] < 0 || y[b * stride + k] >= A) return false;
        m_prime.set(y, n, batch, maxN, stride, m_maxSamples);
        return true;
    }
    // ---- prefill: a prime's state blob from a time-parallel pass (beyond the reference; prefill.hpp) ------------------
    // W: the trailing samples of a prime that determine the state behind it (sum of the dilations + the two history words); 0 without
    // conditioning weights
    int prefillWindow() const { return m_nCond > 0 ? wn::prefill_window(m_ringSlots) : 0; }
    // For request i < count the blob that slotStart(x, uid), slotSetTemperature, slotPrime(y, n), steps up to local sample n and slotSave
    // would have produced -- byte for byte -- at dst + i * stride (16-byte aligned device or mapped pinned memory, stride a multiple of
    // 16 and at least slotStateBytes()), from ONE set of layer launches over the last W samples of every prime, asynchronously on
    // `stream`; y and x stay alive until it has run.  Works in and outside slot mode and touches no ring, column or session.  Calls
    // of one engine share its scratch: one stream, or ordered by the caller.  Returns count; 0 with nothing written: no conditioning
    // weights, a shape that does not fit a CU, count outside 1 .. 65535, an n < 1, a temperature outside [2^-10, 2^10], a bad
    // precision, pointer, alignment or stride.
    int prefillStates(const wn::PrefillReq* reqs, int count, void* dst, long long stride, hipStream_t stream = 0) {
        if (m_nCond <= 0 || !m_supported) return 0;
        wn::TimeModel m = timeModel();
        if (m_featDirty) buildFeatStream(stream);
        m.wblob = m_wblobF;
        m.bias = m_biasF;
        return m_prefill.run(m, reqs, count, dst, stride, stream) ? count : 0;
    }
    // ---- scoring: per-sample log-likelihoods from a time-parallel pass (beyond the reference; score.hpp) ---------------
    // the largest sum of n, each rounded up to 16, that one scoreSamples call accepts (its scratch stays under wn::kScoreScratchCap);
    // 0 without conditioning weights
    int scoreMaxSamples() const { return m_nCond > 0 && m_supported ? wn::score_max_samples(F16, R, S) : 0; }
    // For request i < count: logp[t] = log softmax(Za_t / T)[y[t]] for t < n (natural logarithm, fp32; and, where rows is not NULL,
    // rows[t][a] = log softmax(Za_t / T)[a]), with Za_t the logits of sample t of a column started from silence, fed y[0 .. t) and
    // reading feature column t.  ONE set of layer launches over all of [0, n) of every request, asynchronously on `stream`; y, x and
    // the outputs stay alive until it has run.  Works in and outside slot mode and touches no ring, column or session.  Calls of one
    // engine share its scratch: one stream, or ordered by the caller.  Returns count; 0 with nothing written or launched: no
    // conditioning weights, count outside 1 .. 65535, an n < 1, a temperature outside [2^-10, 2^10], a bad precision, stride or
    // pointer, a misaligned or unreachable output, a total over scoreMaxSamples().
    int scoreSamples(const wn::ScoreReq* reqs, int count, hipStream_t stream = 0) {
        if (m_nCond <= 0 || !m_supported) return 0;
        wn::TimeModel m = timeModel();
        // (checked before anything is queued: a refused call launches nothing, the stream rebuild included)
        if (!wn::Score::acceptable(m, reqs, count)) return 0;
        if (m_featDirty) buildFeatStream(stream);
        m.wblob = m_wblobF;
        m.bias = m_biasF;
        return m_score.run(m, reqs, count, stream) ? count : 0;
    }
    // the model as prefill, scoring and scoring with carried state see it (time_pass.hpp), without the weight stream and the bias
    // table: buildFeatStream may still replace them
    wn::TimeModel timeModel() const {
        const int L = m_numLayers;
        wn::TimeModel m;
        m.f16 = F16;
        m.R = R;
        m.S = S;
        m.A = A;
        m.numLayers = L;
        m.maxDilation = m_maxDilation;
        m.ringSlots = m_ringSlots;
        m.nCond = m_nCond;
        m.tanhEmbed = m_tanhEmbed ? 1 : 0;
        m.wblob = NULL;
        m.waveStreamFrags = CF::waveStreamFrags(L);
        m.headZs = (unsigned)(CF::headOffsetFrags(L) + CF::O_ZS);
        m.headZa = (unsigned)(CF::headOffsetFrags(L) + CF::O_ZA);
        m.bias = NULL;
        m.biasL = C::BIAS_L;
        m.embPrev = m_embedPrev;
        m.embCur = m_embedCur;
        for (int l = 0, d = 1, off = 0; l < L; l++) {
            int dN = d << 1;
            if (dN > m_maxDilation) dN = 1;
            m.layers[l] = wn::TimeLayer{(unsigned)CF::streamPos(l, CF::O_COND, L), (unsigned)CF::streamPos(l, CF::O_PREV, L),
                                        (unsigned)CF::streamPos(l, CF::O_CUR, L), (unsigned)CF::streamPos(l, CF::O_RES, L),
                                        (unsigned)CF::streamPos(l, CF::O_SKIP, L), d, off, dN, off + d};
            off += d;
            d = dN;
        }
        return m;
    }
    // ---- prefill and scoring from mel frames: a time-parallel upsampling pass (beyond the reference; mel_time.hpp) ----
    // elements of a row of upsampled features: 16 * ceil(nCond / 16); 0 without setUpsampling
    int upsampleRowElems() const { return m_upStride > 0 ? wn::mel_time_row(m_nCond) : 0; }
    wn::MelTimeModel melTimeModel() const { return wn::MelTimeModel{F16, m_nCond, m_upWindow, m_upStride, m_upTab, m_upBias}; }
    // For request i < count the upsampled features of samples [first, first + count) of its frames, as rows of upsampleRowElems()
    // T_data elements (channels >= nCond zero) -- bit for bit what upsampleFeatures stores for that utterance and sample --, from ONE
    // launch, asynchronously on `stream`.  Frames max(0, first / stride - (m - 1)) .. (first + count - 1) / stride are read, in
    // place.  Returns count; 0 with nothing written or launched: no setUpsampling, count outside 1 .. 65535, mel not in device
    // memory, a bad precision or stride, frames * stride short of the range, first < 0, count < 1, dst not 16-byte aligned device
    // memory.
    int upsampleRequests(const wn::MelTimeReq* reqs, int count, hipStream_t stream = 0) {
        if (m_upStride <= 0) return 0;
        return m_melTime.run(melTimeModel(), reqs, count, stream) ? count : 0;
    }
    // prefillStates from frames: samples [t0, n) of every request are upsampled into the engine's own rows, and the prefill launches
    // read those.  The blob is byte for byte the one slotStartMel, slotPrime(y, n), steps to n and slotSave produce.
    int prefillStatesMel(const wn::PrefillMelReq* reqs, int count, void* dst, long long stride, hipStream_t stream = 0) {
        if (m_nCond <= 0 || !m_supported || m_upStride <= 0 || reqs == NULL || count < 1 || count > 65535) return 0;
        wn::TimeModel pm = timeModel();
        const wn::MelTimeModel mm = melTimeModel();
        const int W = wn::prefill_window(m_ringSlots);
        const size_t rowB = (size_t)wn::mel_time_row(m_nCond) * sizeof(elem);
        std::vector<wn::MelTimeReq> ur(count);
        std::vector<wn::PrefillReq> pr(count);
        std::vector<size_t> at(count);
        size_t bytes = 0;
        for (int i = 0; i < count; i++) {
            const wn::PrefillMelReq& q = reqs[i];
            if (q.n < 1) return 0;
            const int t0 = wn::prefill_first(q.n, W);
            ur[i] = wn::MelTimeReq{q.mel, q.precision, q.cStride, q.fStride, q.frames, t0, q.n - t0, NULL};
            pr[i] = wn::PrefillReq{q.y, q.n, NULL, F16 ? 16 : 32, 1, (long long)wn::mel_time_row(m_nCond), q.uid, q.temperature};
            at[i] = bytes;
            bytes += (size_t)(q.n - t0) * rowB;
        }
        // (checked before anything is queued: a refused call launches nothing)
        if (!wn::MelTime::acceptable(mm, ur.data(), count, true) || !wn::Prefill::acceptable(pm, pr.data(), count, dst, stride, true)) return 0;
        char* const rows = m_melTime.rows(bytes);
        for (int i = 0; i < count; i++) {
            ur[i].dst = rows + at[i];
            pr[i].x = rows + at[i];
        }
        if (m_featDirty) buildFeatStream(stream);
        pm.wblob = m_wblobF;
        pm.bias = m_biasF;
        if (!m_melTime.run(mm, ur.data(), count, stream, true)) return 0;
        return m_prefill.run(pm, pr.data(), count, dst, stride, stream, true) ? count : 0;
    }
    // scoreSamples from frames: samples [0, n) of every request are upsampled into the engine's own rows (an allocation beside the
    // scoring scratch: upsampleRowElems() * sizeof(T_data) bytes per sample, at most scoreMaxSamples() of them), and the scoring
    // launches read those.  Accepts what scoreMaxSamples() accepts.
    int scoreSamplesMel(const wn::ScoreMelReq* reqs, int count, hipStream_t stream = 0) {
        if (m_nCond <= 0 || !m_supported || m_upStride <= 0 || reqs == NULL || count < 1 || count > 65535) return 0;
        wn::TimeModel sm = timeModel();
        const wn::MelTimeModel mm = melTimeModel();
        const size_t rowB = (size_t)wn::mel_time_row(m_nCond) * sizeof(elem);
        std::vector<wn::MelTimeReq> ur(count);
        std::vector<wn::ScoreReq> sr(count);
        std::vector<size_t> at(count);
        size_t bytes = 0;
        for (int i = 0; i < count; i++) {
            const wn::ScoreMelReq& q = reqs[i];
            if (q.n < 1) return 0;
            ur[i] = wn::MelTimeReq{q.mel, q.precision, q.cStride, q.fStride, q.frames, 0, q.n, NULL};
            sr[i] = wn::ScoreReq{q.y, q.n, NULL, F16 ? 16 : 32, 1, (long long)wn::mel_time_row(m_nCond), q.temperature, q.logp, q.rows};
            at[i] = bytes;
            bytes += (size_t)q.n * rowB;
        }
        if (!wn::MelTime::acceptable(mm, ur.data(), count, true) || !wn::Score::acceptable(sm, sr.data(), count, true)) return 0;
        char* const rows = m_melTime.rows(bytes);
        for (int i = 0; i < count; i++) {
            ur[i].dst = rows + at[i];
            sr[i].x = rows + at[i];
        }
        if (m_featDirty) buildFeatStream(stream);
        sm.wblob = m_wblobF;
        sm.bias = m_biasF;
        if (!m_melTime.run(mm, ur.data(), count, stream, true)) return 0;
        return m_score.run(sm, sr.data(), count, stream, true) ? count : 0;
    }
    // ---- scoring with carried state: time chunks, from and to a state blob (beyond the reference; score_carry.hpp) ----
    // For request i < count the chunk y[0 .. n) is scored as local samples done .. done + n - 1 of an utterance, done = that of the
    // in-state (a blob of slotSave / slotsSaveList / prefillStates* / this call; NULL: from silence at 0), x the CHUNK's feature
    // columns: logp (and rows) are BIT FOR BIT those scoreSamples gives for these samples in a pass over [0, done + n), and
    // stateOut, where not NULL, is BYTE FOR BYTE the blob prefillStates gives for the first done + n samples.  In-states are read
    // only and may be shared; their headers are read with blocking copies on the null stream (pinned ones in place) before anything
    // is queued.  Uses the scoring scratch: scoreMaxSamples() bounds the sum of padded n.  Returns count; 0 with nothing written or
    // launched: what scoreSamples refuses, a state of another engine shape, precision or layout version, a misaligned or
    // unreachable state, done + n beyond INT_MAX - 16, a stateOut that overlaps a state or another stateOut of the call.
    int scoreChunks(const wn::ScoreChunkReq* reqs, int count, hipStream_t stream = 0) {
        if (m_nCond <= 0 || !m_supported) return 0;
        wn::TimeModel m = timeModel();
        std::vector<wn::ScoreChunkIn> in;
        if (!wn::Score::chunksCheck(m, reqs, count, false, in)) return 0;
        if (m_featDirty) buildFeatStream(stream);
        m.wblob = m_wblobF;
        m.bias = m_biasF;
        return m_score.runChunks(m, reqs, count, in, stream) ? count : 0;
    }
    // scoreChunks from frames: mel holds the utterance's frames from frame 0; samples [done, done + n) of every request are upsampled
    // into the engine's own rows (which start at the chunk), and the chunk pass reads those.
    int scoreChunksMel(const wn::ScoreChunkMelReq* reqs, int count, hipStream_t stream = 0) {
        if (m_nCond <= 0 || !m_supported || m_upStride <= 0 || reqs == NULL || count < 1 || count > 65535) return 0;
        wn::TimeModel sm = timeModel();
        const wn::MelTimeModel mm = melTimeModel();
        const size_t rowB = (size_t)wn::mel_time_row(m_nCond) * sizeof(elem);
        std::vector<wn::MelTimeReq> ur(count);
        std::vector<wn::ScoreChunkReq> sr(count);
        std::vector<size_t> at(count);
        size_t bytes = 0;
        for (int i = 0; i < count; i++) {
            const wn::ScoreChunkMelReq& q = reqs[i];
            if (q.n < 1) return 0;
            sr[i] = wn::ScoreChunkReq{q.state, q.y, q.n, NULL, F16 ? 16 : 32, 1, (long long)wn::mel_time_row(m_nCond), q.uid, q.temperature,
                                      q.logp, q.rows, q.stateOut};
            at[i] = bytes;
            bytes += (size_t)q.n * rowB;
        }
        std::vector<wn::ScoreChunkIn> in;
        if (!wn::Score::chunksCheck(sm, sr.data(), count, true, in)) return 0;
        for (int i = 0; i < count; i++) {
            const wn::ScoreChunkMelReq& q = reqs[i];
            ur[i] = wn::MelTimeReq{q.mel, q.precision, q.cStride, q.fStride, q.frames, in[i].k0, q.n, NULL};
        }
        if (!wn::MelTime::acceptable(mm, ur.data(), count, true)) return 0;
        char* const rows = m_melTime.rows(bytes);
        for (int i = 0; i < count; i++) {
            ur[i].dst = rows + at[i];
            sr[i].x = rows + at[i];
        }
        if (m_featDirty) buildFeatStream(stream);
        sm.wblob = m_wblobF;
        sm.bias = m_biasF;
        if (!m_melTime.run(mm, ur.data(), count, stream, true)) return 0;
        return m_score.runChunks(sm, sr.data(), count, in, stream) ? count : 0;
    }
    // ---- generation --------------------------------------------------------------------------
    // Generates num_samples in pieces of num_samples_per_chunk and hands every finished piece to
    // consume(yOut, firstSample, count) on the calling thread (role of nv_wavenet.cuh:445-497).  Two
    // streams: generation of piece k+1 is enqueued right behind piece k and never waits for the host;
    // the device-to-caller copy of piece k runs on a second stream as soon as an event says piece k is
    // complete, so copies and consumers overlap the generation of later pieces.  Returns after the
    // last piece has been consumed.
    template <class Callback>
    bool run_chunks(int num_samples_per_chunk, Callback consume, int num_samples, int batch_size, int* yOut = NULL,
                    int batch_size_per_block = 1, bool dumpActivations = false, hipStream_t stream = 0) {
        (void)dumpActivations;
        assert(num_samples_per_chunk > 0);
        struct Piece {
            int first, count;
            hipEvent_t generated, delivered;
        };
        std::vector<Piece> pieces;
        for (int first = 0; first < num_samples; first += num_samples_per_chunk) {
            Piece pc;
            pc.first = first;
            pc.count = num_samples - first < num_samples_per_chunk ? num_samples - first : num_samples_per_chunk;
            pc.generated = pooledEvent(2 * pieces.size());
            pc.delivered = pooledEvent(2 * pieces.size() + 1);
            pieces.push_back(pc);
        }
        // (the events are the engine's, made once.  A second stream exists only where it buys something: when the samples or the PCM
        //  go to HOST memory, so that the copy of a chunk overlaps the generation of the next; device-resident outputs are copied in
        //  stream order, 20 us per chunk.  Made per call and destroyed at its end -- 1.4 ms -- because streams kept alive in the engine
        //  take hardware queues away from the caller's own streams: with them pooled, a launch on a caller's side stream queued up
        //  behind a kernel of another of its streams, tests/..::test_chain_launch_that_cannot_become_resident..)
        const bool hostOut = (yOut != NULL && !isDevicePtr(yOut)) || (m_pcmUser != NULL && !isDevicePtr(m_pcmUser));
        hipStream_t genStream = stream, outStream = stream;
        const bool ownGen = hostOut && !stream;
        if (ownGen) gpuErrChk(hipStreamCreate(&genStream));
        if (hostOut) gpuErrChk(hipStreamCreate(&outStream));

        bool ok = true;
        for (size_t k = 0; k < pieces.size(); k++) {
            const Piece& pc = pieces[k];
            m_num_samples_per_chunk = pc.count;
            // The reference dumps activations in every chunk (nv_wavenet.cuh:471, hard-coded true) and
            // its test reads them back afterwards; only the last chunk's dump can be observed, so only
            // the last chunk runs the dump-capable kernel variant.
            ok = run_partial(pc.first, num_samples, batch_size, NULL, batch_size_per_block, k + 1 == pieces.size(), genStream) && ok;
            gpuErrChk(hipEventRecord(pc.generated, genStream));
            if (hostOut) gpuErrChk(hipStreamWaitEvent(outStream, pc.generated, 0));
            if (yOut) getYOut(yOut, pc.first, pc.count, outStream);
            if (m_pcmUser) getAudioOut(m_pcmUser, pc.first, pc.count, outStream);
            gpuErrChk(hipEventRecord(pc.delivered, outStream));
        }
        m_num_samples_per_chunk = 0;
        for (size_t k = 0; k < pieces.size(); k++) {
            gpuErrChk(hipEventSynchronize(pieces[k].delivered));
            consume(yOut, pieces[k].first, pieces[k].count);
        }
        if (ownGen) gpuErrChk(hipStreamDestroy(genStream));
        if (hostOut) gpuErrChk(hipStreamDestroy(outStream));
        if (isChain() && chainStatus() != 0) ok = false;   // (everything has completed: the check costs nothing)
        return ok;
    }

    // Generates samples [init_sample, init_sample + chunk) continuing from device-resident state
    // (history, dilation ring); chunk = the run_chunks chunk, or num_samples (nv_wavenet.cuh:499-635).
    // Asynchronous on `stream`.  yOut (host or device, [batch][num_samples] ints) receives the
    // sample buffer when non-NULL.
    bool run_partial(int init_sample, int num_samples, int batch_size, int* yOut = NULL, int batch_size_per_block = 1,
                     bool dumpActivations = false, hipStream_t stream = 0) {
        assert(batch_size_per_block > 0 && batch_size_per_block < 5);
        assert(batch_size % batch_size_per_block == 0);
        assert(batch_size > 0 && batch_size <= m_maxBatch);
        assert(num_samples <= m_maxSamples);
        assert(m_condRaw != NULL || m_cond != NULL || m_condUser != NULL || m_featPtr != NULL);  // some conditioning has been handed over
        assert(m_featPtr == NULL || num_samples <= m_featSamples);
        assert(m_condRaw == NULL || num_samples <= m_condRawSamples);      // ... and the in-place tensor covers the run
        assert(m_condUser == NULL || num_samples <= m_condUserSamples);    // ... and so does a caller's packed buffer
        assert(m_pcmUser == NULL || m_pcmUserElems == 0 || m_pcmUserElems >= (size_t)batch_size * num_samples);
        if (m_implementation == SINGLE_BLOCK) assert(S <= 4 * R);
        if (!m_supported) return false;
        const int* const on = m_temps.on;
        if (!m_featPtr && (on[wn::kTemperature] > 0 || on[wn::kMinP] > 0 || m_temps.cutting() > 0)) {
            // only the kernels that compute the conditioning from the features read the table: nothing is generated rather than
            // generated with the values off
            if (on[wn::kTemperature] > 0)
                fprintf(stderr, "nvWavenetInfer: %d columns have a sampling temperature other than 1, which packed or in-place conditioning "
                        "and multi-CU launches cannot honour: use the features path, or setTemperatures(NULL, 0)\n", on[wn::kTemperature]);
            else if (on[wn::kMinP] > 0)
                fprintf(stderr, "nvWavenetInfer: %d columns have a probability floor (min-p) other than 0, which packed or in-place "
                        "conditioning and multi-CU launches cannot honour: use the features path, or setMinP(NULL, 0)\n", on[wn::kMinP]);
            else
                fprintf(stderr, "nvWavenetInfer: some columns have a tail cut (%d top-k, %d top-p), which packed or in-place conditioning "
                        "and multi-CU launches cannot honour: use the features path, or setTopK(NULL, 0) and setTopP(NULL, 0)\n",
                        on[wn::kTopK], on[wn::kTopP]);
            return false;
        }

        if (m_prime.any() && !m_featPtr) {
            fprintf(stderr, "nvWavenetInfer: %d columns carry a prime, which packed or in-place conditioning and multi-CU launches cannot "
                    "honour: use the features path, or setPrime(NULL, ..)\n", m_prime.primed);
            return false;
        }

        // a new utterance: the dilation rings read as zero until written (wavenet_wg takes x[t-d] = 0 for t < d from the ring
        // itself).  resetHistory() -- every way of handing over a new utterance's conditioning calls it -- has normally done this
        // already, outside the generation's critical path; this covers run() after run() on the same inputs.
        if (init_sample == 0) clearRings(stream);
        const int tiles = (batch_size + 15) / 16;
        if (isChain() && !m_featPtr) slotRingsDirty(tiles);      // (a chain launch writes the rings of the batch's tiles only)
        else wgRingsDirty(tiles);
        wn::Params p = baseParams();
        p.cond = m_condUser ? m_condUser : m_cond;
        p.condRaw = m_condRaw;
        p.condRawKind = m_condRaw ? m_condRawKind : 0;
        p.feat = NULL;
        if (m_featPtr) {
            // the conditioning is computed by wavenet_wg from the features: its own stream (with Wcond) and bias table (with bcond)
            if (m_featDirty) buildFeatStream(stream);
            p.wblob = m_wblobF;
            p.bias = m_biasF;
            p.feat = m_featPtr;
            p.condRawKind = 3;
        }
        p.sel = m_outputSelectors;
        p.yOut = m_yOut;
        p.batch = batch_size;
        p.numSamples = num_samples;
        p.condSamples = m_featPtr ? m_featSamples : m_condRaw ? m_condRawSamples : m_maxSamples;
        p.initSample = init_sample;
        p.count = m_num_samples_per_chunk ? m_num_samples_per_chunk : num_samples;
        if (p.initSample + p.count > num_samples) p.count = num_samples - p.initSample;
        p.dump = dumpActivations ? 1 : 0;
        p.useRng = m_useRng ? 1 : 0;
        p.softScale = m_featPtr ? m_temps.softScale : NULL;
        p.floorOn = m_featPtr ? floorMask() : 0;
        m_lastStride = num_samples;
        if (p.count <= 0) return true;
        bool primeOk = true;
        if (m_prime.any() && p.initSample < m_prime.maxN) {
            // the launch's range holds a forced sample: its rows of the second table -- the primes, and beyond them what the launch
            // would have used
            primeOk = wn::prime_selectors(stream, m_prime.sel, p.initSample, p.count, batch_size, m_maxBatch, m_prime.yDev, m_prime.yStride,
                                          m_prime.nDev, p.useRng, m_rngSeed, m_outputSelectors, A);
            p.sel = m_prime.sel;
            p.useRng = 0;
            p.forced = 1;
        }

        // (computing the conditioning from the features is wavenet_wg's: a chain engine runs it for such a launch)
        bool result = (isChain() && !m_featPtr) ? launchChain(p, tiles, stream) : launchWg(p, tiles, stream);
        result = result && primeOk;
        if (m_pcmUser != NULL) {
            // the indices of a finished sample are final: the expansion is a per-element map of yOut
            hipLaunchKernelGGL(wn::mulaw_pcm_kernel, dim3(gridFor((size_t)batch_size * p.count)), dim3(256), 0, stream,
                               m_yOut, m_pcm, m_mulaw, batch_size, num_samples, p.initSample, p.count);
            result = result && hipGetLastError() == hipSuccess;
        }
        if (yOut != NULL) {
            gpuErrChk(hipMemcpyAsync(yOut, m_yOut, (size_t)num_samples * batch_size * sizeof(int), hipMemcpyDefault, stream));
            if (m_pcmUser != NULL)
                gpuErrChk(hipMemcpyAsync(m_pcmUser, m_pcm, (size_t)num_samples * batch_size * sizeof(short),
                                         hipMemcpyDefault, stream));
        }
        return result;
    }

    // Samples [init_sample, init_sample + count) only, asynchronously on `stream` (what run_chunks does per
    // chunk, for callers that drive the chunks themselves, e.g. with the conditioning streamed in between)
    bool run_range(int init_sample, int count, int num_samples, int batch_size, hipStream_t stream = 0) {
        m_num_samples_per_chunk = count;
        const bool ok = run_partial(init_sample, num_samples, batch_size, NULL, 1, false, stream);
        m_num_samples_per_chunk = 0;
        return ok;
    }
    // the sample history back to 128 (what setInputs does) and a clean hand-off status, asynchronously on `stream`
    void resetHistory(hipStream_t stream = 0) {
        hipLaunchKernelGGL(wn::silence_kernel, dim3(1), dim3(256), 0, stream, m_yInPrev, m_yInCur, m_maxBatch);
        gpuErrChk(hipGetLastError());
        gpuErrChk(hipMemsetAsync(m_chainStatus, 0, sizeof(unsigned), stream));
        clearRings(stream);
    }
    // zeroes the dilation rings of the tiles that launches have written since the last clear (4 MiB per tile at C3: 1 ms at 12 288
    // utterances, once per utterance)
    void clearRings(hipStream_t stream) {
        if (m_ringDirtyTiles > 0)
            gpuErrChk(hipMemsetAsync(m_ring, 0, (size_t)m_ringDirtyTiles * m_ringSlots * R * 16 * sizeof(elem), stream));
        m_ringDirtyTiles = 0;
    }

    // ---- slot mode: continuous batching (slots_session.hpp; DESIGN.md "Slot mode") ----
    wn::SlotSession& slots() { return *m_slots; }


    bool run(int num_samples, int batch_size, int* yOut = NULL, int batch_size_per_block = 1,
             bool dumpActivations = false, hipStream_t stream = 0) {
        m_num_samples_per_chunk = 0;
        return run_partial(0, num_samples, batch_size, yOut, batch_size_per_block, dumpActivations, stream);
    }

protected:
    void dropLhConditioning() {
        m_condRaw = NULL;
        m_condRawKind = 0;
        m_condUser = NULL;
    }
    // m_wblobF / m_biasF from m_wblob / m_bias / m_condW / m_condB, asynchronously on `stream`
    void buildFeatStream(hipStream_t stream) {
        assert(m_nCond > 0);
        const int L = m_numLayers;
        const size_t wElems = (size_t)C::NW * CF::waveStreamFrags(L) * C::FRAG_ELEMS;
        const int bTotal = L * C::BIAS_L + 2 * A;
        if (!m_wblobF) {
            gpuErrChk(hipMalloc(&m_wblobF, wElems * sizeof(elem)));
            gpuErrChk(hipMalloc(&m_biasF, (size_t)bTotal * sizeof(float)));
            std::vector<int2> map;
            for (int l = 0; l < L; l++)
                for (int i = 0; i < C::FLW; i++) map.push_back(make_int2((int)C::streamPos(l, i, L), (int)CF::streamPos(l, i, L)));
            for (int q = 0; q < C::FHW; q++)
                map.push_back(make_int2((int)C::headOffsetFrags(L) + C::headFrag(q), (int)CF::headOffsetFrags(L) + CF::headFrag(q)));
            m_restreamN = (int)map.size();
            gpuErrChk(hipMalloc(&m_restream, map.size() * sizeof(int2)));
            gpuErrChk(hipMemcpy(m_restream, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice));
        }
        gpuErrChk(hipMemsetAsync(m_wblobF, 0, wElems * sizeof(elem), stream));
        hipLaunchKernelGGL(wn::restream_kernel, dim3(gridFor((size_t)C::NW * m_restreamN * 64)), dim3(256), 0, stream, (wn::uintx4*)m_wblobF,
                           (const wn::uintx4*)m_wblob, (const int2*)m_restream, m_restreamN, C::waveStreamFrags(L), CF::waveStreamFrags(L), C::NW);
        gpuErrChk(hipGetLastError());
        for (int l = 0; l < L; l++) {
            hipLaunchKernelGGL((wn::pack_weight_kernel<F16>), dim3(gridFor((size_t)2 * R * KC)), dim3(256), 0, stream,
                               m_wblobF + CF::streamPos(l, CF::O_COND, L) * C::FRAG_ELEMS, m_condW + (size_t)l * KC * 2 * R, 2 * R, KC, C::NW,
                               CF::waveStreamFrags(L) * C::FRAG_ELEMS, R / 16);
            gpuErrChk(hipGetLastError());
        }
        hipLaunchKernelGGL((wn::feat_bias_kernel<F16>), dim3(gridFor(bTotal)), dim3(256), 0, stream, m_biasF, m_bias, m_condB, L, R, C::BIAS_L,
                           bTotal);
        gpuErrChk(hipGetLastError());
        m_featDirty = false;
    }
    size_t ringElems() const { return (size_t)m_tiles * m_ringSlots * R * 16; }
    unsigned statusWord(int i) {
        unsigned s = 0;
        gpuErrChk(hipDeviceSynchronize());
        gpuErrChk(hipMemcpy(&s, m_chainStatus + i, sizeof(unsigned), hipMemcpyDeviceToHost));
        return s;
    }
    // tiles per workgroup of THIS launch: the four-tile kernels exist dump-free and for the packed conditioning only (with the conditioning
    // computed in the kernel a fourth tile does not fit the register file: 2-31 spilled registers by shape, and no faster -- LABNOTES round 6)
    int launchTiles(int tiles, bool dump, int raw) const {
        const int bt = wgTiles(tiles);
        return (bt == 4 && (dump || raw != 0)) ? 3 : bt;
    }
    // ---- what a slot-mode session needs of its engine (wn::SlotHost) ----
    wn::SlotLive slotLive() const override { return wn::SlotLive{m_nCond, m_upTab, m_upBias, m_upWindow, m_upStride, m_rngSeed}; }
    const short* slotMulaw() override {
        ensureMulaw();
        return m_mulaw;
    }
    void slotFeatStreamReady(hipStream_t stream) override {
        if (m_featDirty) buildFeatStream(stream);
    }
    void slotRingsDirty(int tiles) override {
        if (tiles > m_ringDirtyTiles) m_ringDirtyTiles = tiles;
    }
    // (the launch of run_partial for features, with the window's buffers and the selector table)
    bool slotGenerate(const void* feat, const float* sel, int* y, int W, int t0, int count, int cols, bool forced,
                      hipStream_t stream) override {
        const int tiles = (cols + 15) / 16;
        wgRingsDirty(tiles);
        wn::Params p = baseParams();
        p.wblob = m_wblobF;
        p.bias = m_biasF;
        p.cond = NULL;
        p.condRaw = NULL;
        p.condRawKind = 3;
        p.feat = feat;
        p.sel = sel;
        p.yOut = y;
        p.batch = cols;
        p.numSamples = W;
        p.condSamples = W;
        p.initSample = t0;
        p.count = count;
        p.dump = 0;
        p.useRng = 0;
        p.softScale = m_temps.softScale;
        p.floorOn = floorMask();
        p.forced = forced ? 1 : 0;
        return launchWg(p, tiles, stream);
    }
    // what every launch's Params share: the model, the ring and history, the debug outputs, the shape and schedule, the seed
    wn::Params baseParams() const {
        wn::Params p;
        p.wblob = m_wblob;
        p.bias = m_bias;
        p.embPrev = m_embedPrev;
        p.embCur = m_embedCur;
        p.gate = NULL;
        p.ring = m_ring;
        p.maxDilation = m_maxDilation;
        p.yInPrev = m_yInPrev;
        p.yInCur = m_yInCur;
        p.xtOut = m_XtOut;
        p.skipOut = m_skipOut;
        p.zs = m_Zs;
        p.za = m_Za;
        p.p = m_p;
        p.numLayers = m_numLayers;
        p.maxBatch = m_maxBatch;
        p.ringSlots = m_ringSlots;
        p.ldsRingD = 0;                 // (the wavenet_wg launchers place ring slots in the LDS their tables leave free: placeLdsRing)
        p.tiles = m_tiles;
        p.tileBase = 0;
        p.tanhEmbed = m_tanhEmbed ? 1 : 0;
        p.embLds = 0;
        p.forced = 0;
        p.floorOn = 0;
        p.rngKey0 = (unsigned)m_rngSeed;
        p.rngKey1 = (unsigned)(m_rngSeed >> 32);
        p.clk = m_clkOn ? m_clk : NULL;
        fillSchedule(p);
        return p;
    }
    // the tiles whose rings a wavenet_wg launch on `tiles` tiles writes: a workgroup of BT tiles stores into the rings of ALL its
    // tiles, the padding tiles beyond the batch included (a later, larger batch must find those slots zero as well)
    void wgRingsDirty(int tiles) {
        int bt = wgTiles(tiles);
        if (bt >= 3 && wg4Fits()) bt = 12;      // (three or four tiles per workgroup by launch: both roundings)
        const int touched = (tiles + bt - 1) / bt * bt;
        slotRingsDirty(touched > m_tiles ? m_tiles : touched);
    }
    // wavenet_wg by batch size: one to four tiles per workgroup
    bool launchWg(wn::Params& p, int tiles, hipStream_t stream) {
        const int bt = launchTiles(tiles, p.dump != 0, p.condRawKind);
        if (bt == 4) {
            if constexpr (WG4) return launchE<4, false, 0>(p, tiles, stream);
            return false;
        }
        if (bt == 3) {
            if constexpr (WG3) return launch<3>(p, tiles, stream);
            return false;
        }
        if (bt == 2) {
            if constexpr (WG2) return launch<2>(p, tiles, stream);
            return false;
        }
        return launch<1>(p, tiles, stream);
    }
    // a chain launch that gives up can be re-run by wavenet_wg when the model's bias table fits one workgroup's LDS
    bool chainHasFallback() const { return ldsFits<1>(); }

    // The multi-CU chain: every (tile, stage) workgroup must be resident at the same time, so tiles are launched in
    // groups of at most CUs / stages chains; mailboxes are re-zeroed before every launch.  Residency cannot be
    // guaranteed when other work shares the GPU, so every chain launch is bracketed, in stream order and without any
    // host round trip: (1) rings and history of the launch's tiles are copied aside; (2) the chain runs; (3) if it
    // gave up (status word set by the first spin that timed out), chain_restore_kernel puts rings and history back
    // and a wavenet_wg launch gated on the status word generates the launch's samples instead (arithmetic and state
    // layouts are the same in both organisations, bit for bit); (4) chain_settle_kernel counts the event and clears
    // the word.  When the chain completes, (3) is two empty launches.
    bool launchChain(wn::Params& p, int tiles, hipStream_t stream) {
        wn::ChainParams cp;
        cp.mail = m_mail;
        cp.status = m_chainStatus;
        cp.stages = m_chainStages;
        cp.lpc = m_chainLpc;
        cp.timeoutTicks = m_chainTimeoutTicks;
        const int perLaunch = m_numCUs / m_chainStages;
        if (perLaunch < 1) return false;
        const bool dump = p.dump != 0;
        const bool fallback = m_ringShadow != NULL;
        const size_t ringTileElems = (size_t)m_ringSlots * R * 16;
        // tiles beyond the chains that are resident at once ride the same chains, up to TPC_MAX per chain (round 5); more than
        // that takes further launches
        const int tpc = chainTpc((m_maxBatch + 15) / 16);        // (what the mailboxes were sized for)
        cp.tpc = tpc;
        const int tilesPerLaunch = perLaunch * tpc;
        for (int t0 = 0; t0 < tiles; t0 += tilesPerLaunch) {
            const int nT = tiles - t0 < tilesPerLaunch ? tiles - t0 : tilesPerLaunch;
            cp.tile0 = t0;
            cp.ntiles = nT;
            cp.chains = nT < perLaunch ? nT : perLaunch;
            const int b0 = t0 * 16, nb = (p.batch - b0 < nT * 16 ? p.batch - b0 : nT * 16);
            if (fallback) {
                gpuErrChk(hipMemcpyAsync(m_ringShadow + t0 * ringTileElems, m_ring + t0 * ringTileElems,
                                         nT * ringTileElems * sizeof(elem), hipMemcpyDeviceToDevice, stream));
                gpuErrChk(hipMemcpyAsync(m_histShadow + b0, m_yInPrev + b0, nb * sizeof(int), hipMemcpyDeviceToDevice, stream));
                gpuErrChk(hipMemcpyAsync(m_histShadow + m_maxBatch + b0, m_yInCur + b0, nb * sizeof(int), hipMemcpyDeviceToDevice, stream));
            }
            gpuErrChk(hipMemsetAsync(m_mail, 0, CC::mailGranules(cp.chains, m_chainStages, tpc) * sizeof(unsigned long long), stream));
            const int grid = 8 * m_chainStages * ((cp.chains + 7) / 8);
            p.embLds = CC::embTables();
            p.gate = NULL;
            if (dump) {
                hipLaunchKernelGGL((wn::wavenet_chain<F16, R, S, A, true>), dim3(grid), dim3(C::THREADS), CC::ldsBytes(), stream, p, cp);
            } else {
                bool hoisted = false;
                if constexpr (kChainHoistBuilt) {
                    if (chainHoists(tpc)) {
                        hipLaunchKernelGGL((wn::wavenet_chain<F16, R, S, A, false, true>), dim3(grid), dim3(C::THREADS), CC::ldsBytes(), stream, p, cp);
                        hoisted = true;
                    }
                }
                if (!hoisted) hipLaunchKernelGGL((wn::wavenet_chain<F16, R, S, A, false>), dim3(grid), dim3(C::THREADS), CC::ldsBytes(), stream, p, cp);
            }
            if (hipGetLastError() != hipSuccess) return false;
            if (fallback) {
                const size_t n16 = nT * ringTileElems * sizeof(elem) / 16;
                hipLaunchKernelGGL(wn::chain_restore_kernel, dim3(gridFor(n16)), dim3(256), 0, stream, (const unsigned*)m_chainStatus,
                                   (wn::uintx4*)(m_ring + t0 * ringTileElems), (const wn::uintx4*)(m_ringShadow + t0 * ringTileElems), n16,
                                   m_yInPrev + b0, m_yInCur + b0, (const int*)(m_histShadow + b0), (const int*)(m_histShadow + m_maxBatch + b0), nb);
                if (hipGetLastError() != hipSuccess) return false;
                // the same samples for the same tiles on wavenet_wg, one tile per workgroup, only if the chain gave up
                wn::Params q = p;
                q.gate = m_chainStatus;
                q.batch = b0 + nb;
                const int nEmb = embTables<1>();
                q.embLds = nEmb;
                bool ok;
                if (nEmb) ok = launchGated<true>(q, t0, nT, nEmb, stream);
                else ok = launchGated<false>(q, t0, nT, 0, stream);
                if (!ok) return false;
                hipLaunchKernelGGL(wn::chain_settle_kernel, dim3(1), dim3(1), 0, stream, m_chainStatus);
                if (hipGetLastError() != hipSuccess) return false;
            }
        }
        return true;
    }
    // wavenet_wg<BT = 1> for tiles [tile0, tile0 + ntiles), gated on Params::gate
    template <bool EMB> bool launchGated(wn::Params& q, int tile0, int ntiles, int nEmb, hipStream_t stream) {
        q.tileBase = tile0;
        const int kind = q.condRawKind;
        const bool dump = q.dump != 0 || (!F16 && kind != 0);      // (see launch(): the fp32 dump-free kernel is the packed one)
        const size_t lds = ldsNeed<1>(m_numLayers, nEmb, dump);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(ntiles), dim3(C::THREADS), lds, stream, q);
            return hipGetLastError() == hipSuccess;
        };
        if (!dump) {
            if constexpr (F16) {
                if (kind == 2) return go(wn::wavenet_wg<F16, R, S, A, 1, EMB, false, 2>);
                if (kind == 1) return go(wn::wavenet_wg<F16, R, S, A, 1, EMB, false, 1>);
            }
            return go(wn::wavenet_wg<F16, R, S, A, 1, EMB, false, 0>);
        }
        if constexpr (F16) {
            if (kind == 2) return go(wn::wavenet_wg<F16, R, S, A, 1, EMB, true, 2>);
        }
        if (kind == 1) return go(wn::wavenet_wg<F16, R, S, A, 1, EMB, true, 1>);
        return go(wn::wavenet_wg<F16, R, S, A, 1, EMB, true, 0>);
    }
};
