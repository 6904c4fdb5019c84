// slots_deliver.hpp -- slot mode: ragged delivery of a step's samples.
//
// A plain step copies [maxBatch][count] rows out of the window, idle columns and the samples past an utterance's end included.  A
// ragged step delivers pieces: piece p is the n valid samples of column `slot` in this step, contiguous at element `offset` of a
// ragged int32 sample buffer and / or a ragged int16 PCM buffer (one offset for both).  Every offset is a multiple of 8 elements,
// so every store but a piece's tail is one (PCM) or two (samples) 16-byte vector stores; the 0 to 7 elements between the end of a
// piece and the start of the next are not written.  The PCM is looked up from the int32 window through the table of
// mulaw_pcm_kernel: a ragged step needs neither the PCM window nor the PCM launch.  The outputs may be device memory or pinned
// host memory mapped into the device's address space.  The kernel (slots_deliver.hip) is compiled once for both precisions.
#pragma once

#include <hip/hip_runtime.h>

namespace wn {

// one piece as the kernel reads it
struct DeliverPiece {
    int slot;                // column
    int n;                   // samples, 1 .. count
    long long offset;        // first element in both outputs, a multiple of 8
};
static_assert(sizeof(DeliverPiece) == 16, "DeliverPiece layout");

constexpr int kDeliverAlign = 8;      // elements

// one piece as the caller sees it (nvw_slot_piece of include/nv_wavenet_c.h, field for field)
struct SlotPiece {
    int slot;                // column
    unsigned uid;            // of the utterance
    long long first;         // local index of the piece's first sample
    int n;                   // samples
    int finished;            // this piece ends the utterance
    long long offset;        // as DeliverPiece
};
static_assert(sizeof(SlotPiece) == 32, "SlotPiece layout");

// Window rows (T + k) mod W, k < n, of column `slot` of y [columns][W] -> samples[offset + k], pcm[offset + k] = table[sample], for
// each of the nPieces pieces (device memory); samples or pcm may be NULL, not both.  One launch, whether or not the rows wrap.
// Asynchronous.
bool slots_deliver(hipStream_t stream, const int* y, const short* table, int T, int W, int count, const DeliverPiece* pieces, int nPieces,
                   int* samples, short* pcm);

}  // namespace wn
