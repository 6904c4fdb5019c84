// score.hpp -- per-sample log-likelihoods from a time-parallel pass.
//
// logp[t] = log softmax(Za_t / T)[y[t]], where Za_t are the logits wavenet_wg<.., RAW = 3> hands to softmax_pick at sample t of a
// column that started from silence, was fed y[0 .. t) and reads feature column t.  Every sample is known, so this is the
// time-parallel pass (time_pass.hpp) over the whole of [0, n) with no states, every layer, the skip path, and the head:
//   * head, several time tiles per workgroup: relu(skip + Bskip_0 + .. + Bskip_{L-1}) rounded to T_data, Zs = relu(Bzs + Wzs .)
//     rounded to T_data, Za = Bza + Wza ., then z' = Za * (log2(e) / T), the maximum, exp2 and the sum as softmax_pick does them,
//     logp = (z'_y - m' - log2(sum)) * ln 2 in fp32 -- and, when asked for, the same for every row a.
// logp is written for t < n only, rows likewise; nothing for the padding columns of the last tile.
//
// With carried state (score_carry.hpp) the pass runs over a time chunk [k0, k0 + n) of an utterance: from a state
// blob at done = k0 instead of silence, and, when asked, to the blob at done = k0 + n.  The layer kernels of both are
// score_carry.hip's instantiations -- a request without states takes the same code, which measured faster than an instantiation
// without the state taps (LABNOTES.md) --; the head is score.hip's, launched through score_launch_head, and the scratch is this
// class's: one allocation, one cap.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "time_pass.hpp"

// the (R, S, A) the Makefile builds engines for
#define WN_SCORE_SHAPES(X) X(32, 128, 256) X(64, 128, 256) X(64, 256, 256) X(128, 256, 256) X(64, 128, 512) X(256, 256, 256) X(32, 256, 256) X(128, 256, 1024)

namespace wn {

// the scratch of one call never exceeds this; nvw_score_max_samples follows from it
constexpr size_t kScoreScratchCap = (size_t)1 << 30;

// one request (nvw_score_req)
struct ScoreReq {
    const int* y;            // the samples, device memory, n values (clamped into 0 .. A-1 as slot_prime_kernel clamps them)
    int n;
    const void* x;           // the utterance's features as for slotStart: x[c * cStride + t * tStride]; columns [0, n) are read
    int precision;
    long long cStride, tStride;
    float temperature;
    float* logp;             // n floats, device memory or mapped pinned host memory
    float* rows;             // NULL, or n * A floats, device memory, 16-byte aligned
};
// the largest sum of padded n (each n rounded up to 16) of one call
inline int score_max_samples(bool f16, int R, int S) {
    const size_t rows = (kScoreScratchCap / time_scratch_bytes(f16, R, S)) & ~(size_t)15;
    return rows > 0x7ffffff0u ? 0x7ffffff0 : (int)rows;
}

// the head over the skip sums of `count` jobs (at most maxTiles time tiles each): score_head_kernel for the model's shape, as the
// whole pass launches it.  false: a shape that is not built, or a rejected launch.
bool score_launch_head(const TimeModel& m, const TimeJob* jobs, int count, int maxTiles, const float* skf, hipStream_t stream);

struct ScoreChunkReq;      // (score_carry.hpp)
struct ScoreChunkIn;

// The engine-owned side: scratch (grown on demand, at most kScoreScratchCap), the requests' staging.  Calls of one engine are issued
// on one stream, or ordered by the caller: they share the scratch.  Touches no ring, column or session.
class Score {
public:
    // logp (and rows) of count requests, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    // what run() refuses, without touching the GPU's queues (wblob and bias of m are not looked at)
    // ownX: x lies in the engine's own feature rows (mel_time.hpp) and is not looked at
    static bool acceptable(const TimeModel& m, const ScoreReq* reqs, int count, bool ownX = false);
    bool run(const TimeModel& m, const ScoreReq* reqs, int count, hipStream_t stream, bool ownX = false);

    // ---- with carried state (score_carry.hip) ----
    // Every check of a chunk call, the blocking reads of the in-states' headers included; queues nothing.  in[i]: where request i
    // starts and what its embedding and out-state take from its in-state.
    static bool chunksCheck(const TimeModel& m, const ScoreChunkReq* reqs, int count, bool ownX, std::vector<ScoreChunkIn>& in);
    // logp (rows, out-states) of count checked requests, asynchronously on `stream`
    bool runChunks(const TimeModel& m, const ScoreChunkReq* reqs, int count, const std::vector<ScoreChunkIn>& in, hipStream_t stream);

private:
    // the embedding, the layers and the blob step for the model's shape (score_carry.hip: one set of instantiations serves the whole
    // pass and the chunks).  false: a shape that is not built, or a rejected launch.
    static bool launchLayers(const TimeModel& m, const TimeJob* jobs, int count, int maxTiles, bool anyOut, const TimeScratch& sc,
                             hipStream_t stream);
    GrowBuffer m_scratch;
    TimeJobs m_jobs;
};

}  // namespace wn
