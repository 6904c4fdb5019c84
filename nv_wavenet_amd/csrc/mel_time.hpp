// mel_time.hpp -- upsampled features of a request's sample range from its mel frames, as rows.
//
// The lockstep upsampling (upsample_features_kernel) is organised by batch tile and engine counter, the slot one
// (slot_mel_upsample_kernel) by column and step.  This pass is organised by REQUEST and TIME RANGE: request i is frames
// mel[c * cStride + f * fStride] (fp16 or fp32, nCond channels, `frames` written), a sample range [a, b) and a destination, and gets
//   dst[(t - a) * row + c] = b[c] + sum_{j < m} sum_ci mel[ci][f - j] W[ci][c][j * stride + r],   t = f * stride + r in [a, b),
// in the engine's T_data, row = 16 * ceil(nCond / 16) elements, channels >= nCond exactly zero -- bit for bit what the lockstep kernel
// stores for that utterance and sample: the A operands are the engine's own table (pack_upsample_kernel's layout) and bias, the
// accumulator starts from the bias, taps ascend, kf ascends within a tap, per row tile, with the same mma; frames f - j < 0 are zero
// operands; frames and results are converted as pack_features_kernel and upsample_features_kernel convert them; and one column of an
// MFMA's result does not depend on the other fifteen.  There is no second copy of the upsampling weights.
//
// All 16 columns of an MFMA share a phase r, so the N dimension is (request, frame) pairs at one phase: the columns of a call are
// the frames a / stride .. (b - 1) / stride of every request, flattened over the requests and taken 16 at a time, the same for
// every phase.  A lane finds its column's request by bisection of the jobs' first columns and gathers its frames in place from the
// caller's strided tensor: frames max(0, a / stride - (m - 1)) .. (b - 1) / stride are read and no others.  Samples outside [a, b)
// of the frames that straddle its edges, and the columns that pad the last group, are computed and not stored.  One launch per
// call, ordered by the stream; nothing waits for another workgroup.
//
// The feature passes fed from such rows (prefillStatesMel, scoreSamplesMel) read them with precision = the engine's own (their
// conversion is the identity), cStride = 1, tStride = row.
#pragma once

#include <hip/hip_runtime.h>

#include "slots_session.hpp"

namespace wn {

// one request (nvw_upsample_req)
struct MelTimeReq {
    const void* mel;         // device memory: mel[c * cStride + f * fStride]
    int precision;
    long long cStride, fStride;
    int frames;              // frames written; frames * stride >= first + count
    int first, count;        // the range [first, first + count)
    void* dst;               // count rows of `row` T_data elements, 16-byte aligned device memory
};
// one request of the passes fed from frames (nvw_prefill_mel_req, nvw_score_mel_req): PrefillReq / ScoreReq with frames for features
struct PrefillMelReq {
    const int* y;
    int n;
    const void* mel;
    int precision;
    long long cStride, fStride;
    int frames;
    unsigned uid;
    float temperature;
};
struct ScoreMelReq {
    const int* y;
    int n;
    const void* mel;
    int precision;
    long long cStride, fStride;
    int frames;
    float temperature;
    float* logp;
    float* rows;
};
// ... as the kernel sees it
struct MelTimeJob {
    const void* mel;
    long long cStride, fStride;
    char* dst;
    int a, b;                // the range
    int f0;                  // a / stride: the frame of its first column
    int col0;                // its first column among those of the call
    int precision, pad;
};
static_assert(sizeof(MelTimeJob) == 56, "MelTimeJob layout");
// the upsampling as the engine holds it
struct MelTimeModel {
    bool f16;
    int nCond, window, stride;
    const void* tab;         // m_upTab: [stride][kUpRowTiles][m * KFC] fragments
    const float* bias;       // m_upBias
};

// elements of a row
inline int mel_time_row(int nCond) { return 16 * ((nCond + 15) / 16); }

// The engine-owned side: the requests' staging, and the feature-row scratch of the mel entries (grown on demand).  Calls of one
// engine are issued on one stream, or ordered by the caller: they share the scratch.  Touches no ring, column or session.
class MelTime {
public:
    MelTime() {}
    MelTime(const MelTime&) = delete;
    ~MelTime();
    // what run() refuses, without touching the GPU's queues (tab and bias of m are not looked at).  ownDst: the destinations lie in
    // rows() and are not looked at either.
    static bool acceptable(const MelTimeModel& m, const MelTimeReq* reqs, int count, bool ownDst = false);
    // the rows of count requests, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    bool run(const MelTimeModel& m, const MelTimeReq* reqs, int count, hipStream_t stream, bool ownDst = false);
    // the feature-row scratch, at least `bytes` (synchronises when it has to grow)
    char* rows(size_t bytes);

private:
    char* m_rows = NULL;
    size_t m_rowsBytes = 0;
    MelTimeJob* m_jobs = NULL;
    int m_jobCap = 0;
    bool m_ldsReady = false;     // the LDS variant's dynamic-LDS opt-in has been made on this engine's device
    StageRing m_stage;
};

}  // namespace wn
