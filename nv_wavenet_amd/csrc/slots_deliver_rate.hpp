// slots_deliver_rate.hpp -- slot mode: ragged delivery at the caller's sample rate.
//
// slot_deliver_kernel (slots_deliver.hpp) delivers a step's PCM at the model's rate.  This kernel converts while it delivers: the
// PCM of piece p is outputs m0 .. m0 + count - 1 of its utterance's stream at rate L / M (the definition of resample.hpp, x[i] =
// table[sample i] by local index i, zero below 0 and, once the utterance is finished, from its end on), int16, contiguous at element
// `offset` of the PCM buffer.  All of that is host knowledge (rate_delivered below), so the pieces are filled before anything is
// launched, as the sample pieces are.
//
// One four-wave workgroup per (piece, tile of 16 G output blocks); the block grid counts from the utterance's output 0, so an
// output's row tile and the order of its sum do not depend on how the utterance was cut into steps: the pieces of an utterance,
// concatenated, are bit for bit nvw_resample of its whole PCM.  The tile's span is staged in LDS once as fp32 in the spare-word
// layout of §6p: a position of local index in [first - H, first) comes from the column's tail, one in [first, first + n) from window
// row (T + i - first) mod W of the int32 window through the mu-law PCM table (the wrap is a matter of the staging: one launch), the
// rest is zero.  Then the GEMM of resample_core.hpp against the resampler slot's table, rint, saturate, and plain vector stores of
// the outputs in [m0, m0 + count).
//
// Tails: the last H = ceil(2 c / L) PCM values of an utterance, int16, zero where it has none.  The workgroups of a piece read the
// tail while one of them replaces it, so there are two images: a step reads one and writes the other (the first tile's workgroup
// of every piece, from old tail plus piece; a piece without outputs has one workgroup that does only this), and the session flips
// after every rate step.  Tails are indexed by a host-side map from column to tail row carried in the piece record: a move swaps
// two host integers.  Compiled once for both precisions.
#pragma once

#include <hip/hip_runtime.h>

#include "resample_core.hpp"

namespace wn {

// one piece as the kernel reads it
struct RatePiece {
    int slot;                // column
    int tailRow;             // its row of the tail images
    int n;                   // samples of the step, 1 .. count
    int flags;               // kRateZeroTail: the old tail counts as zero (a resume without one)
    long long first;         // local index of the piece's first sample
    long long m0;            // first output
    long long offset;        // first element of the PCM output, a multiple of 8
    long long block0;        // m0 / Q
    int count;               // outputs, may be 0
    int blocks;              // of the range: (m0 + count - 1) / Q - block0 + 1; 0 when count is 0
    int tile0;               // its first tile among those of the launch (a piece has at least one)
    int pad;
};
static_assert(sizeof(RatePiece) == 64, "RatePiece layout");
constexpr int kRateZeroTail = 1;

// one piece's PCM as the caller sees it (nvw_slot_rate_piece of include/nv_wavenet_c.h, field for field), parallel to SlotPiece
struct SlotRatePiece {
    long long m0;            // first output of the utterance in this piece
    int count;               // outputs, may be 0
    int pad;
    long long offset;        // first element of the PCM output, a multiple of 8
};
static_assert(sizeof(SlotRatePiece) == 24, "SlotRatePiece layout");

// floor and ceiling of a / b, b > 0, for a of either sign
inline long long rate_floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline long long rate_ceil_div(long long a, long long b) { return -rate_floor_div(-a, b); }
// D(k): the outputs of an unfinished stream whose every input is below k, max(0, ceil((k L - c) / M)) ...
inline long long rate_delivered(long long k, int up, int down, int centre) {
    const long long d = rate_ceil_div(k * up - centre, down);
    return d > 0 ? d : 0;
}
// ... and the history that the first of the next ones may reach back over: H = ceil(2 c / L)
inline int rate_tail_len(int up, int centre) { return (int)((2LL * centre + up - 1) / up); }

struct RateLaunch {
    const RatePiece* pieces;      // device memory
    int count;
    int tiles;                    // of all pieces
    const int* y;                 // the window [columns][W] ...
    const short* table;           // ... and the PCM value of every sample index
    int T, W;                     // the step's first window row
    const short* tailIn;          // [columns][H]: the image this step reads ...
    short* tailOut;               // ... and the one it writes
    int H;
    short* pcm;
    ResampleTab t;
};

// the dynamic-LDS opt-in of the kernel variant (groups, ch) on the current device; false when the runtime refuses
bool slots_deliver_rate_prepare(int groups, int ch);
// One launch over the tiles of a.count pieces with `ldsBytes` of LDS; asynchronous.  The variant is prepared.
bool slots_deliver_rate(hipStream_t stream, const RateLaunch& a, int groups, int ch, size_t ldsBytes);

}  // namespace wn
