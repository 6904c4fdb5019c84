// denoise.hpp -- the bias denoiser at the PCM boundary: STFT, spectral subtraction and inverse STFT in one kernel, batched, ragged
// and by output range.
//
// What callers of this family of vocoders run on every delivered utterance (the Denoiser beside Tacotron-2 / WaveGlow): the model's
// stationary noise floor, measured once as a magnitude spectrum b[k], is subtracted from the STFT magnitude, the phase kept.  With
// N = nFft (= the window length), hop a divisor of N with O = N / hop in 4 .. 16, w the periodic Hann window, a stream x[0 .. n) in
// PCM units (nothing is divided by 32768), n > N / 2:
//   xp     = x reflect-padded by N / 2 on both sides
//   X_f[k] = sum_j w[j] xp[f hop + j] e^{-2 pi i k j / N},           f = 0 .. n / hop, k = 0 .. N / 2
//   Y_f[k] = X_f[k] max(1 - strength b[k] / |X_f[k]|, 0)             (0 where |X_f[k]| = 0)
//   y_f[j] = w[j] / N sum_k c_k Re(Y_f[k] e^{+2 pi i k j / N}),      c_0 = c_{N/2} = 1, otherwise 2
//   out[t] = sum_f y_f[t + N/2 - f hop] / sum_f w^2[t + N/2 - f hop], t = 0 .. n - 1, both sums over the existing frames that cover
//            t, in ascending f
// i.e. torch.istft(gain * torch.stft(x, center=True, pad_mode="reflect")), in fp32 throughout; an int16 output is the quotient rounded
// to nearest-even and saturated.  O >= 4 keeps the envelope >= 0.25 at the utterance's ends.
//
// One launch per call over (request, tile), a workgroup of four waves per tile; the N dimension of v_mfma_f32_16x16x4_f32 is 16
// consecutive frames f0 .. f0 + 15.
//   tiles    overlap, outputs do not: tile i (counted from frame 0 of the STREAM, not of the range) starts at frame f0 = i (17 - O)
//            and owns the padded positions [(f0 + O - 1) hop, (f0 + 16) hop), tile 0 from N / 2: every owned position has all its O
//            covering frames inside the tile, nothing is accumulated across workgroups, no atomics.  A tile recomputes O - 1 frames
//            of its neighbour (16 / 13 of the work at O = 4).  Which tile computes an output, and in which order, depends on its
//            absolute position only: a range, or any chunking of a stream, is bit for bit the whole call.
//   forward  as §6o: the span of 15 hop + J' samples staged once in LDS (reflected at the stream's ends, zero where the request holds
//            none, the same skew), the windowed cos / -sin table of stft_core.hpp as A operand, a real and an imaginary accumulator per
//            bin tile, bin tiles over waves.
//   gain     in registers: m = sqrt(re^2 + im^2), g = m > 0 ? max(1 - s b[k] / m, 0) : 0, re, im *= g c_k / N, to the spectrum
//            image [2 K'][16] in LDS (real rows, then imaginary), each block of four rows rotated by 16 (row / 4) words.
//   inverse  a second GEMM, M = the J' samples of a frame, K = 2 K', N = the 16 frames.  A: w[j] cos(2 pi k j / N) and
//            -w[j] sin(2 pi k j / N), float64 (angle from k j mod N) rounded to fp32, A fragments [J' / 16][2 K' / 16][64 lanes] x 4;
//            B: the spectrum image, lane l reads row 4 q' + (l >> 4), frame l & 15; sample tiles over waves.
//   add      the synthesis tiles go to an LDS image [16 frames][J' + 4] that overlays the span (dead after the forward GEMM); after
//            a barrier each thread sums, for four consecutive owned positions, the covering frames in ascending f and, in the same
//            order, w^2 from a table, divides, converts and stores the outputs of [t0, t0 + count) only.
// LDS: 4 (32 K' + max(15 hop + J' + 4 ((15 hop + J') / hop + 1), 16 (J' + 4))) bytes, J' = N rounded up to 16, K' = N / 2 + 1 rounded
// up to 16: 130 KiB at 1024 / 256.  Touches no ring, column or session; works inside and outside slot mode.
#pragma once

#include <hip/hip_runtime.h>

#include "slots_session.hpp"

namespace wn {

// one request (nvw_denoise_req)
struct DenoiseReq {
    const void* in;          // device memory, nIn samples of inType bits (16: int16, 32: fp32): absolute samples first .. first + nIn - 1
    int inType;
    long long first;
    int nIn;
    int last;                // 1: the stream ends at first + nIn
    void* out;               // device memory, count samples of outType bits: outputs t0 .. t0 + count - 1
    int outType;
    long long t0;
    int count;
    float strength;
};
// ... as the kernel sees it
struct DenoiseJob {
    const void* in;
    void* out;
    long long first, t0;
    int nIn, count;
    int frames;              // n / hop + 1 of a stream that ends here; INT_MAX otherwise (every frame that the range needs exists)
    int tile0;               // its first tile among those of the call
    int tileBase;            // ... and which tile of the stream that is
    int inType, outType;
    float strength;
};
static_assert(sizeof(DenoiseJob) == 64, "DenoiseJob layout");

constexpr int kDenoiseLdsMax = 160 * 1024;      // of a workgroup (gfx950)
constexpr int kDenoiseFftMin = 64, kDenoiseFftMax = 1024, kDenoiseOverlapMin = 4, kDenoiseOverlapMax = 16;

// The engine-owned side: the tables of one geometry and the requests' staging.  Calls of one engine are issued on one stream, or
// ordered by the caller.
class Denoiser {
public:
    Denoiser() {}
    Denoiser(const Denoiser&) = delete;
    ~Denoiser() { clear(); }
    // the geometry and the caller's bias spectrum b[0 .. nFft / 2] (host memory, >= 0).  Builds and uploads the tables; synchronises.
    // false, with the previous geometry kept: nFft not a multiple of 4 in 64 .. 1024, hop not a multiple of 4 that divides nFft with
    // nFft / hop in 4 .. 16, no bias or one in device memory, a negative or non-finite bias, or more LDS than a workgroup has.
    bool set(int nFft, int hop, const float* bias);
    bool isSet() const { return m_nFft > 0; }
    // the geometry and the tables on the device, for the kernel that shares them (slots_deliver_denoise.hpp)
    int nFft() const { return m_nFft; }
    int hop() const { return m_hop; }
    const float* forwardTable() const { return m_fwdTab; }
    const float* inverseTable() const { return m_invTab; }
    const float* biasTable() const { return m_bias; }
    const float* envelopeTable() const { return m_wnd2; }
    // bytes of LDS a workgroup of this geometry takes
    static size_t ldsBytes(int nFft, int hop);
    // the leading outputs computable from the first k samples: k itself for a stream that ends there (0 for one that run() refuses,
    // k <= nFft / 2), otherwise those whose every covering frame lies below k, max(0, ((k - N/2) / hop + 1) hop - N/2).  0 when not set.
    long long ready(long long k, int last) const;
    // what run() refuses, without touching the GPU's queues
    bool acceptable(const DenoiseReq* reqs, int count) const;
    // count requests in one launch, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    bool run(const DenoiseReq* reqs, int count, hipStream_t stream);

private:
    void clear();
    // the tile of the stream that owns padded block ub = (t + N/2) / hop
    long long tileOf(long long ub) const { const int o = m_nFft / m_hop; return ub >= o - 1 ? (ub - o + 1) / (17 - o) : 0; }
    int m_nFft = 0, m_hop = 0;
    float* m_fwdTab = NULL;      // [K' / 16][re, im][J' / 16][64 lanes] x 4
    float* m_invTab = NULL;      // [J' / 16][2 K' / 16][64 lanes] x 4
    float* m_bias = NULL;        // [K'], zero past the bins
    float* m_wnd2 = NULL;        // [J']: the fp32 of w^2, zero past the window
    DenoiseJob* m_jobs = NULL;
    int m_jobCap = 0;
    unsigned short m_ldsReady = 0;      // bit 3 i + j: the dynamic-LDS opt-in of that kernel variant has been made on this engine's device
    StageRing m_stage;
};

}  // namespace wn
