// slots.hpp -- slot mode (continuous batching): the per-column state around the unchanged generation kernels.
//
// In slot mode every column of the batch holds one utterance that starts and ends on its own.  What a column's samples depend on
// is its descriptor (features, length, uid) and the engine seed: local sample k of an utterance takes the features x[:, k] and
// the selector philox_selector(seed, {k, uid}) -- the counter of the lockstep in-kernel draw with the utterance's uid for the
// column -- and its dilation rings and sample history start as resetHistory() leaves them.  The window of W samples (a multiple
// of the largest dilation) wraps: window row t mod W holds the features and selectors of the sample generated at t, and
// wavenet_wg<.., RAW=3> is launched on window rows with useRng = 0, so its ring index t & (d-1) stays that of t.
// The kernels (slots.hip) are compiled once for both precisions; the engine calls the launchers below.
#pragma once

#include <hip/hip_runtime.h>

namespace wn {

// one column's utterance (48 bytes, device array [maxBatch])
struct SlotDesc {
    const void* x;           // upsampled features, device memory: x[c * cStride + k * tStride], channel c, local sample k
    long long cStride, tStride;
    long long start;         // value of the engine's sample counter at the utterance's local sample 0 (k = counter - start: nothing
                             // to advance per step, so the feed's workgroups only ever read the descriptor)
    int length;              // samples of the utterance: features past it read as zero
    unsigned uid;            // word 1 of the Philox counter of its selectors
    int precision;           // 32 | 16: element type of x
    int active;              // 0: idle column (zero features)
};
static_assert(sizeof(SlotDesc) == 48, "SlotDesc layout");

// a descriptor handed over by the host for column `column`; reset != 0: the utterance starts (history and rings of the column too)
struct SlotUpdate {
    int column;
    int reset;
    int pad0, pad1;
    SlotDesc d;
};

// Zeroes the dilation rings of the nCols columns listed in cols (ring [tiles][ringSlots][fragsPerSlot KiB], utterance j of a tile
// owning lanes 16g + j of every fragment), writes the nUpd descriptors and sets the history of the restarted columns to 128.
// Asynchronous on `stream`.
bool slots_reset(hipStream_t stream, SlotDesc* desc, const SlotUpdate* upd, int nUpd, const int* cols, int nCols, void* ring,
                 int ringSlots, int fragsPerSlot, int* yInPrev, int* yInCur);
// The window rows (T + i) mod W, i < count, of the first `cols` columns: feature fragments ([W][tiles][KFC] of the engine's
// T_data, the order of pack_features_kernel) and selectors ([W][maxBatch] fp32), from the descriptors and the sample counter
// `counter` of row T.  Asynchronous on `stream`.
template <bool F16>
bool slots_feed(hipStream_t stream, void* feat, float* sel, const SlotDesc* desc, int cols, int maxBatch, int tiles, int nCond,
                long long counter, int T, int W, int count, unsigned long long seed);
// pcm[b][t] = table[y[b][t]] for window rows [t0, t0 + count) of the first `cols` columns of the [.][W] windows (mulaw_pcm_kernel)
bool slots_pcm(hipStream_t stream, const int* y, short* pcm, const short* table, int cols, int W, int t0, int count);

}  // namespace wn
