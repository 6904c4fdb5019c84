// score_carry.hpp -- scoring with carried state: a time chunk of an utterance, from and to a state blob.
//
// The scoring pass (score.hpp) starts from silence at local sample 0 and leaves nothing behind.  Here a request is a CHUNK: the
// samples y[0 .. n) are local samples k0 .. k0 + n - 1 of an utterance, k0 = the `done` of its in-state (slots_state.hpp), or 0 from
// silence; x holds the chunk's own feature columns.  What a layer needs from before the chunk is exactly what a blob holds: x_l[k]
// for the last d_l samples, laid out like a scratch row, and the two history words of the embedding.  The fp32 running residual and
// the fp32 skip sum are per sample and carry nothing across time.  So every sample is computed with the operands of the whole pass in
// the order of the whole pass, and one column of an MFMA's result does not depend on the other fifteen: logp and rows are bit for bit
// those of score.hpp's pass over [0, k0 + n), and the out-state is byte for byte the blob of prefill.hpp at n' = k0 + n.
//
// This is the time-parallel pass (time_pass.hpp) with everything on: tiles are relative to the chunk, lane column r = 16 * tile + j is
// local sample k = k0 + r, and k0 need not be a multiple of 16.
//   * embedding: y(k0 - 1), y(k0 - 2) from the in-state's header (128 from silence);
//   * layer l: the dilated tap of a column with r - d_l < 0 is read from the in-state's slot off_l + ((k0 + r - d_l) mod d_l) -- a
//     zero operand where k0 + r - d_l < 0 or there is no in-state --, and, with an out-state, x_{l+1} of the chunk's last
//     min(n, d_{l+1}) samples also goes to the out blob's slots by ABSOLUTE k;
//   * finish (only when some request has an out-state): the slots of every layer with d_l > n that no sample of the chunk maps to
//     keep the in-state's bytes (zero from silence), and the header;
//   * head: score.hip's score_head_kernel, launched through score_launch_head on the same jobs.
// One launch per layer, ordered by the stream: no grid-wide barrier, no flag, nothing that waits for another workgroup.  In-states
// are read only, and several requests may share one; an out-state overlaps no in-state and no other out-state of the call (a layer's
// launch overwrites slots the next layer's launch still reads from the in-state).  The scratch is wn::Score's: one allocation, one cap.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "score.hpp"

namespace wn {

// one request (nvw_score_chunk_req)
struct ScoreChunkReq {
    const void* state;       // NULL: from silence at local sample 0; else a blob, device or pinned memory, 16-byte aligned: read only
    const int* y;            // the chunk's n samples = local samples done .. done + n - 1, device memory
    int n;
    const void* x;           // the CHUNK's features: x[c * cStride + i * tStride] is feature column done + i
    int precision;
    long long cStride, tStride;
    unsigned uid;            // header of stateOut when state is NULL; otherwise the in-state's uid is kept
    float temperature;
    float* logp;             // n floats, device or pinned
    float* rows;             // NULL, or n * A floats, device, 16-byte aligned
    void* stateOut;          // NULL, or a blob's bytes, device or pinned, 16-byte aligned
};
// ... from frames (nvw_score_chunk_mel_req): the utterance's frames from frame 0
struct ScoreChunkMelReq {
    const void* state;
    const int* y;
    int n;
    const void* mel;
    int precision;
    long long cStride, fStride;
    int frames;
    unsigned uid;
    float temperature;
    float* logp;
    float* rows;
    void* stateOut;
};
// what the host took from a request's in-state (Score::chunksCheck)
struct ScoreChunkIn {
    const char* in;          // device-side address of the in-state, NULL from silence
    char* out;               // device-side address of the out-state, NULL without
    int k0;                  // done of the in-state, 0 from silence
    unsigned uid;
    int yInPrev, yInCur;     // 128, 128 from silence
};

}  // namespace wn
