// prefill.hpp -- a prime's state blob from a time-parallel pass.
//
// Every sample of a prime y[0 .. n) is known, so nothing inside it is autoregressive: layer l at sample t needs x_l[t], x_l[t - d_l]
// and the features of t.  Prefill is the time-parallel pass (time_pass.hpp) over the chunk [t0, n) of the prime, with no in-state, an
// out-state and no skip path: skip, head, softmax and pick feed no state and are not computed.  What comes out is the slot-state blob
// (slots_state.hpp) that a column started from silence, primed with y and stepped to local sample n would have saved -- byte for
// byte, header and payload, in both precisions.
// The state after n samples depends on the last W = sum(d_l) + 2 of them only (the two more are the history words the embedding
// reads), so the pass covers [t0, n), t0 = max(0, n - W) rounded down to a tile of 16, whatever n is.  Positions of layer l before
// n - sum_{k >= l} d_k are computed from taps outside the window (read as zero); none of them is a ring value, and none reaches a blob.
//
// Launches of one call (count requests): the embedding (x_0, and layer 0's ring slot), layers 0 .. L-2 (layer l writes x_{l+1}: to
// the scratch as fp32 running residual and as T_data operand, ping-ponged, and its last d_{l+1} samples to the blobs), and the blob
// step that comes last: the ring slots no sample has written (zero) and the headers.  The last layer's residual is part of no ring
// and is not computed.
#pragma once

#include <hip/hip_runtime.h>

#include "time_pass.hpp"

namespace wn {

// one request (nvw_prefill_req)
struct PrefillReq {
    const int* y;            // the prime, device memory, n values (clamped into 0 .. A-1 as slot_prime_kernel clamps them)
    int n;
    const void* x;           // the utterance's features as for slotStart: x[c * cStride + k * tStride]; columns [t0, n) are read
    int precision;
    long long cStride, tStride;
    unsigned uid;
    float temperature;
};

// samples that determine a state: sum of the dilations + the two history words
inline int prefill_window(int ringSlots) { return ringSlots + 2; }
// first sample of the pass over a prime of n: max(0, n - W) rounded down to a tile of 16
inline int prefill_first(int n, int W) { return (n > W ? n - W : 0) & ~15; }

// The engine-owned side: scratch sized by W (grown on demand), the requests' staging.  Calls of one engine are issued on one
// stream, or ordered by the caller: they share the scratch.
class Prefill {
public:
    // what run() refuses, without touching the GPU's queues (wblob and bias of m are not looked at).  ownX: x is the engine's own
    // feature rows (mel_time.hpp), which start at column t0, and is not looked at.
    static bool acceptable(const TimeModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, bool ownX = false);
    // count blobs to dst + i * stride, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    bool run(const TimeModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, hipStream_t stream, bool ownX = false);

private:
    GrowBuffer m_scratch;
    TimeJobs m_jobs;
};

}  // namespace wn
