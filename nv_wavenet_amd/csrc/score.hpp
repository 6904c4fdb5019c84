// score.hpp -- per-sample log-likelihoods from a time-parallel pass.
//
// logp[t] = log softmax(Za_t / T)[y[t]], where Za_t are the logits wavenet_wg<.., RAW = 3> hands to softmax_pick at sample t of a
// column that started from silence, was fed y[0 .. t) and reads feature column t.  Every sample is known, so the pass is the
// prefill pass (prefill.hpp) with the parts prefill leaves out: 16 consecutive samples of one utterance in the MFMA N dimension, one
// launch per layer ordered by the stream -- no grid-wide barrier, no flag, nothing that waits for another workgroup -- but over the
// whole of [0, n), every layer, and with the skip path, the head and the softmax:
//   * embedding: x_0 as prefill_embed_kernel computes it;
//   * layer l = 0 .. L-1: gate and residual as prefill_layer_kernel (same operands, same order, same device functions), then the
//     skip GEMM on the h fragments already in registers, skip[t] += Wskip_l h, into an fp32 sum in the scratch that the same lane
//     reads and writes; the sum starts from zero and goes in layer order, k ascending: the engine's order.  The last layer's
//     residual is not computed;
//   * head, several time tiles per workgroup: relu(skip + Bskip_0 + .. + Bskip_{L-1}) rounded to T_data, Zs = relu(Bzs + Wzs .)
//     rounded to T_data, Za = Bza + Wza ., then z' = Za * (log2(e) / T), the maximum, exp2 and the sum as softmax_pick does them,
//     logp = (z'_y - m' - log2(sum)) * ln 2 in fp32 -- and, when asked for, the same for every row a.
// The kernels read the engine's own weight streams and bias table at positions from Cfg (ScoreModel): no second copy of the model.
// logp is written for t < n only, rows likewise; nothing for the padding columns of the last tile.
//
// With carried state (score_carry.hpp) the same pass runs over a time chunk [k0, k0 + n) of an utterance: from a state
// blob at done = k0 instead of silence, and, when asked, to the blob at done = k0 + n.  Its layer kernels are score_carry.hip's;
// the head is this file's, launched through score_launch_head, and the scratch is this class's: one allocation, one cap.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "slots_session.hpp"

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
// ... as the kernels see it
struct ScoreJob {
    const int* y;
    const void* x;
    long long cStride, tStride;
    float* logp;
    float* rows;
    long long row0;          // first scratch row of the request
    int n, tiles, precision;
    float scale;             // log2(e) / T
};
static_assert(sizeof(ScoreJob) == 72, "ScoreJob layout");
// one layer's launch: where its matrices start in a wave's stream (1-KiB fragments), its dilation
struct ScoreLayer {
    unsigned cond, prev, cur, res, skip;
    int d;
};
// the model as the engine holds it
struct ScoreModel {
    bool f16;
    int R, S, A, numLayers, nCond, tanhEmbed;
    const void* wblob;       // NW per-wave streams with the conditioning weights (m_wblobF)
    size_t waveStreamFrags;
    unsigned headZs, headZa; // where Wzs and Wza start in a wave's stream
    const float* bias;       // [L][biasL]: Bh + bcond | Bres | Bskip, then Bzs[A], Bza[A] (m_biasF)
    int biasL;
    const void *embPrev, *embCur;
    ScoreLayer layers[128];
    int maxDilation, ringSlots;      // the ring of a state blob (slots_state.hpp): read by the pass with carried state only
};

// bytes of scratch per padded sample: the fp32 residual, two T_data images of x, the fp32 skip sum
inline size_t score_row_bytes(bool f16, int R, int S) { return (size_t)R * 4 + 2 * (size_t)R * (f16 ? 2 : 4) + (size_t)S * 4; }
// the largest sum of padded n (each n rounded up to 16) of one call
inline int score_max_samples(bool f16, int R, int S) {
    const size_t rows = (kScoreScratchCap / score_row_bytes(f16, R, S)) & ~(size_t)15;
    return rows > 0x7ffffff0u ? 0x7ffffff0 : (int)rows;
}

// the head over the skip sums of `count` jobs (at most maxTiles time tiles each): score_head_kernel for the model's shape, as the
// whole pass launches it.  false: a shape that is not built, or a rejected launch.
bool score_launch_head(const ScoreModel& m, const ScoreJob* jobs, int count, int maxTiles, const float* skf, hipStream_t stream);

struct ScoreChunkReq;      // (score_carry.hpp)
struct ScoreChunkIn;

// The engine-owned side: scratch (grown on demand, at most kScoreScratchCap), the requests' staging.  Calls of one engine are issued
// on one stream, or ordered by the caller: they share the scratch.  Touches no ring, column or session.
class Score {
public:
    Score() {}
    Score(const Score&) = delete;
    ~Score();
    // logp (and rows) of count requests, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    // what run() refuses, without touching the GPU's queues (wblob and bias of m are not looked at)
    // ownX: x lies in the engine's own feature rows (mel_time.hpp) and is not looked at
    static bool acceptable(const ScoreModel& m, const ScoreReq* reqs, int count, bool ownX = false);
    bool run(const ScoreModel& m, const ScoreReq* reqs, int count, hipStream_t stream, bool ownX = false);

    // ---- with carried state (score_carry.hip) ----
    // Every check of a chunk call, the blocking reads of the in-states' headers included; queues nothing.  in[i]: where request i
    // starts and what its embedding and out-state take from its in-state.
    static bool chunksCheck(const ScoreModel& m, const ScoreChunkReq* reqs, int count, bool ownX, std::vector<ScoreChunkIn>& in);
    // logp (rows, out-states) of count checked requests, asynchronously on `stream`
    bool runChunks(const ScoreModel& m, const ScoreChunkReq* reqs, int count, const std::vector<ScoreChunkIn>& in, hipStream_t stream);

private:
    // the scratch, at least `need` bytes (synchronises when it has to grow)
    char* scratch(size_t need);
    char* m_scratch = NULL;
    size_t m_scratchBytes = 0;
    ScoreJob* m_jobs = NULL;
    int m_jobCap = 0;
    StageRing m_stage;
    char* m_chunkJobs = NULL;      // two halves of [cap] CarryJob + [cap] ScoreJob, nothing until the first chunk call
    int m_chunkCap = 0;
    StageRing m_chunkStage;
};

}  // namespace wn
