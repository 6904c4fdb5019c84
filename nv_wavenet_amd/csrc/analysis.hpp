// analysis.hpp -- the analysis front end: int16 PCM to mu-law sample indices and log-mel frames, batched.
//
// The inverse of where the engine ends (mulaw_pcm_kernel): what scoring and priming take of a recording.  For PCM p[0 .. n),
// x = p / 32768 reflect-padded by nFft / 2 on both sides, frame f = padded samples [f * hop, f * hop + nFft), f = 0 .. n / hop:
//   X[k]      = sum_j w[j] x_f[j] e^{-2 pi i k j / nFft},  k = 0 .. nFft / 2,  w the periodic Hann window of length nFft
//   mel[c][f] = log(max(sum_k M[c][k] |X[k]|, 1e-5))                           (Tacotron-2's TacotronSTFT.mel_spectrogram)
//   y[t]      = int((sign(x) log1p(mu |x|) / log1p(mu) + 1) / 2 * mu + 0.5),   mu = A - 1
// in fp32 throughout: a second of audio is 0.18 GFLOP here against about 41 to generate it.
//
// One launch per call over (request, tile of 16 consecutive frames), a workgroup of four waves per tile; the 16 frames are the N
// dimension of v_mfma_f32_16x16x4_f32.
//   DFT      a GEMM against a table of w[j] cos / -w[j] sin (float64 rounded to fp32, bins padded to K' = 16 ceil((nFft / 2 + 1) / 16)
//            with zero rows, samples to J' = 16 ceil(nFft / 16) with zero columns), in A-fragment order: one 16-byte load per lane
//            is four k-steps of a bin tile.  Any nFft that is a multiple of 4 is served, 800 as well as 1024.
//   frames   the tile's span of 15 hop + J' samples is staged in LDS once, reflected at the utterance's ends, zero past the last
//            frame; the B operand of sample j of frame f is read at f * hop + j (a Toeplitz read: every sample stored once, read
//            nFft / hop times).  Position l lies at word l + 4 (l / hop): frame lanes are hop + 4 words apart, which is 4 times an
//            odd number modulo 64 when hop is a multiple of 32, so the 64 lanes (16 frames x 4 samples) of a read hit 64 banks.
//   bins     bin tile t belongs to wave t mod 4; a wave holds a real and an imaginary accumulator for up to five of its tiles at
//            a time and makes as many passes over the span as that takes.
//   mel      |X| goes from the accumulators to an LDS image [K'][16]; after a barrier a second GEMM multiplies the mel basis (A-
//            fragment order, rows padded to 16s) by it, then log, the floor (in the log domain: exactly the fp32 of log 1e-5) and
//            the store to mel[c * cStride + f * fStride] in the request's precision, f < frames only.
//   mu-law   the workgroup of tile i encodes samples [16 hop i, 16 hop (i + 1)) by a branch-free binary search of A - 1 int16
//            thresholds in LDS, built on the host from the float64 formula: exact by construction, no transcendental here.
// Touches no ring, column or session; works inside and outside slot mode.
#pragma once

#include <hip/hip_runtime.h>

#include "slots_session.hpp"

namespace wn {

// one request (nvw_analysis_req)
struct AnalysisReq {
    const short* pcm;        // device memory, n samples
    int n;
    void* mel;               // NULL, or device memory: mel[c * cStride + f * fStride], frames(n) frames of nMel channels
    int precision;
    long long cStride, fStride;
    int* y;                  // NULL, or device memory, n values
};
// ... as the kernel sees it
struct AnalysisJob {
    const short* pcm;
    void* mel;
    int* y;
    long long cStride, fStride;
    int n, frames;
    int tile0;               // its first tile among those of the call
    int precision;
};
static_assert(sizeof(AnalysisJob) == 56, "AnalysisJob layout");

constexpr int kAnalysisLdsMax = 160 * 1024;      // of a workgroup (gfx950)
constexpr int kAnalysisFftMin = 64, kAnalysisFftMax = 2048, kAnalysisMelMax = 128;

// The engine-owned side: the tables of one geometry and the requests' staging.  Calls of one engine are issued on one stream, or
// ordered by the caller.
class Analysis {
public:
    Analysis() {}
    Analysis(const Analysis&) = delete;
    ~Analysis() { clear(); }
    // the geometry, the caller's mel basis M [nMel][nFft / 2 + 1] (host memory) and the engine's A.  Builds and uploads the three
    // tables; synchronises.  false, with the previous geometry kept: nFft not a multiple of 4 in 64 .. 2048, hop outside 1 .. nFft,
    // nMel outside 1 .. 128, no basis, or span + magnitude image + thresholds beyond the LDS of a workgroup.
    bool set(int nFft, int hop, int nMel, const float* basis, int levels);
    bool ready() const { return m_nFft > 0; }
    // bytes of LDS a workgroup of this geometry takes
    static size_t ldsBytes(int nFft, int hop, int levels);
    // n / hop + 1; 0 when not set, or for an n that run() refuses (n <= nFft / 2: the reflection needs that many samples)
    int frames(int n) const { return ready() && n > m_nFft / 2 ? n / m_hop + 1 : 0; }
    // what run() refuses, without touching the GPU's queues
    bool acceptable(const AnalysisReq* reqs, int count) const;
    // count requests, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    bool run(const AnalysisReq* reqs, int count, hipStream_t stream);

private:
    void clear();
    int m_nFft = 0, m_hop = 0, m_nMel = 0, m_levels = 0;
    float* m_dftTab = NULL;      // [K' / 16][re, im][J' / 16][64 lanes] x 4
    float* m_melTab = NULL;      // [ceil(nMel / 16)][K' / 16][64 lanes] x 4
    short* m_mulawTab = NULL;    // [levels - 1]: the smallest p with y(p) >= k, k = 1 .. levels - 1
    AnalysisJob* m_jobs = NULL;
    int m_jobCap = 0;
    unsigned char m_ldsReady = 0;      // bit CH: the dynamic-LDS opt-in of analysis_kernel<CH> has been made on this engine's device
    StageRing m_stage;
};

}  // namespace wn
