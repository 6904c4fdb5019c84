// prefill.hpp -- a prime's state blob from a time-parallel pass.
//
// Every sample of a prime y[0 .. n) is known, so nothing inside it is autoregressive: layer l at sample t needs x_l[t], x_l[t - d_l]
// and the features of t.  Where the generation kernels put 16 utterances in the MFMA N dimension, the prefill kernels put 16
// CONSECUTIVE SAMPLES of one utterance there, and run the model layer by layer over a window of samples: one launch per layer,
// ordered by the stream -- no grid-wide barrier, no flag, nothing that can wait for another workgroup.  Skip, head, softmax and pick
// feed no state and are not computed.  What comes out is the slot-state blob (slots_state.hpp) that a column started from silence,
// primed with y and stepped to local sample n would have saved -- byte for byte, header and payload, in both precisions:
//   * the kernels read the engine's own weight streams (with Wcond in every layer's part, the gate rows pre-scaled) and bias table
//     (with bcond added), fragment positions from Cfg::streamPos: there is no second copy of the model;
//   * the gate pre-activation is summed in the engine's order -- bias, conditioning, dilated tap, current tap, k ascending --, the
//     residual as (Bres + x) then Wres h, with the engine's own device functions (mma, gemm_direct, gate1, tanh_t, lds_put_tile's
//     rounding), and one column of an MFMA's result does not depend on what the other fifteen hold.
// The state after n samples depends on the last W = sum(d_l) + 2 of them only (the two more are the history words the embedding
// reads), so the pass covers [t0, n), t0 = max(0, n - W) rounded down to a tile of 16, whatever n is.  Positions of layer l before
// n - sum_{k >= l} d_k are computed from taps outside the window (read as zero); none of them is a ring value, and none reaches a blob.
//
// Launches of one call (count requests): the embedding (x_0, and layer 0's ring slot), layers 0 .. L-2 (layer l writes x_{l+1}: to
// the scratch as fp32 running residual and as T_data operand, ping-ponged, and its last d_{l+1} samples to the blobs), and the blob
// step that comes last: the ring slots no sample has written (zero) and the headers.  The last layer's residual is part of no ring
// and is not computed.  Scratch rows are laid out as blob slots are ([fragment][g] pieces of 16 bytes), so a B operand is one
// 16-byte load per lane and fragment at any per-lane sample offset: taps with d < 16 straddle two time tiles for free.
#pragma once

#include <hip/hip_runtime.h>

#include "slots_session.hpp"

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
// ... as the kernels see it
struct PrefillJob {
    const int* y;
    const void* x;
    long long cStride, tStride;
    char* dst;               // the blob
    int n, t0, tiles, precision;
    unsigned uid;
    int temp;                // header word 10
};
static_assert(sizeof(PrefillJob) == 64, "PrefillJob layout");
// one layer's launch: where its matrices start in a wave's stream (1-KiB fragments), its dilation, and the ring of the layer it
// produces the input of
struct PrefillLayer {
    unsigned cond, prev, cur, res;
    int layer, d;
    int dOut, offOut;
};
// the model as the engine holds it
struct PrefillModel {
    bool f16;
    int R, A, numLayers, maxDilation, ringSlots, nCond, tanhEmbed;
    const void* wblob;       // NW per-wave streams with the conditioning weights (m_wblobF)
    size_t waveStreamFrags;
    const float* bias;       // [L][biasL]: Bh + bcond | Bres | Bskip (m_biasF)
    int biasL;
    const void *embPrev, *embCur;
    PrefillLayer layers[128];
};

// samples that determine a state: sum of the dilations + the two history words
inline int prefill_window(int ringSlots) { return ringSlots + 2; }
// first sample of the pass over a prime of n: max(0, n - W) rounded down to a tile of 16
inline int prefill_first(int n, int W) { return (n > W ? n - W : 0) & ~15; }

// The engine-owned side: scratch sized by W (grown on demand), the requests' staging.  Calls of one engine are issued on one
// stream, or ordered by the caller: they share the scratch.
class Prefill {
public:
    Prefill() {}
    Prefill(const Prefill&) = delete;
    ~Prefill();
    // what run() refuses, without touching the GPU's queues (wblob and bias of m are not looked at).  ownX: x is a base derived
    // from the engine's own feature rows (mel_time.hpp) -- possibly in front of the allocation, since the kernels index it by the
    // absolute sample -- and is not looked at.
    static bool acceptable(const PrefillModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, bool ownX = false);
    // count blobs to dst + i * stride, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    bool run(const PrefillModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, hipStream_t stream, bool ownX = false);

private:
    char* m_scratch = NULL;
    size_t m_scratchBytes = 0;
    PrefillJob* m_jobs = NULL;
    int m_jobCap = 0;
    StageRing m_stage;
};

}  // namespace wn
