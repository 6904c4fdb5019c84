// slots_mel.hpp -- slot mode from mel frames: columns whose utterance is handed over as frames before upsampling.
//
// A mel column's window rows are upsampled in the step that generates them, from its frames, with the table of setUpsampling --
// the sums of upsample_features_kernel, so that its samples are those of the column uid of a lockstep setMel + generate_stream run.
// Its SlotDesc stays inactive: slot_feed_kernel writes zeros into its lanes, and the mel feed then overwrites them.  Frames may be
// handed over piecewise (the upsampling is causal: sample k reads frames k / stride - j, j < window / stride); a step never goes
// past the frames available (slotsHeadroom).  The kernels (slots_mel.hip) are compiled once for both precisions.
#pragma once

#include <hip/hip_runtime.h>

namespace wn {

// one mel column's utterance (48 bytes, device array [maxBatch])
struct MelDesc {
    const void* mel;          // frames, device memory: mel[c * cStride + f * fStride], channel c, frame f
    long long cStride, fStride;
    long long start;          // value of the engine's sample counter at the utterance's local sample 0
    int frames;               // frames available: local samples below frames x stride can be generated
    unsigned uid;             // word 1 of the Philox counter of its selectors
    int precision;            // 32 | 16: element type of mel
    int state;                // 0: not a mel column, 1: running (more frames may come), 2: running, final (length frames x stride)
};
static_assert(sizeof(MelDesc) == 48, "MelDesc layout");

struct MelUpdate {
    int column;
    int pad;
    MelDesc d;
};

// Writes the nUpd descriptors.  Asynchronous on `stream`.
bool slots_mel_apply(hipStream_t stream, MelDesc* desc, const MelUpdate* upd, int nUpd);
// frames of each column a step of `count` samples upsamples (whole frames, those straddling its edges included), and the frames
// of each column it reads (m = window / stride taps back)
inline int slots_mel_frames(int count, int stride) { return (count + stride - 2) / stride + 1; }
inline int slots_mel_stage_frames(int count, int stride, int m) { return slots_mel_frames(count, stride) + m - 1; }
// Sets the dynamic-LDS limit of the upsampling kernel of this precision on the current device (once per engine).
template <bool F16>
bool slots_mel_prepare();
// The window rows (T + i) mod W, i < count, of the mel columns of the nTiles tiles listed in tileList (ascending tile numbers):
// their frames gathered into `stage` ([slots_mel_stage_frames][nTiles][KFC] fragments, T_data, the order of pack_features_kernel;
// frames before the first or not yet available are zero), the per-column placement into `colInfo` ([nTiles * 16]), the selectors
// ([W][maxBatch] fp32) and the feature fragments ([W][tiles][KFC]) of the mel columns' lanes -- nothing of other columns' lanes --
// through `records` ([nTiles * 16][count] samples of KFC KiB / 16 each: the columns' upsampled samples in their own order).
// upTab / upBias: the table and bias of setUpsampling (m taps); counter: the engine's sample counter of row T.  Asynchronous.
template <bool F16>
bool slots_mel_feed(hipStream_t stream, void* feat, float* sel, void* stage, void* records, int* colInfo, const MelDesc* desc, const int* tileList,
                    int nTiles, int maxBatch, int tiles, int nCond, const void* upTab, const float* upBias, int m, int stride,
                    long long counter, int T, int W, int count, unsigned long long seed);

}  // namespace wn
