// slots_deliver_denoise.hpp -- slot mode: ragged delivery through the bias denoiser, the STFT state carried across steps
// (DESIGN.md §6s).
//
// denoise_kernel (denoise.hpp, §6r) is stateless: a tile is 16 consecutive frames of ONE stream, and a streaming caller who asks
// for the one frame a step completes pays for sixteen.  This kernel delivers while it denoises: the PCM of piece p is outputs
// t0 .. t0 + count - 1 of §6r's definition on its column's stream x[i] = table[sample i], i counted from the stream origin s0 (the
// local index of the column's first piece after a start, or after a resume without denoise state), int16, at element `offset` of
// the PCM buffer.  With N = nFft, O = N / hop, after k samples of an unfinished stream
//   q(k) = k > N/2 ? (k - N/2) / hop + 1 : 0        frames are complete (frame f covers samples [f hop - N/2, f hop + N/2)), and
//   D(k) = max(0, q(k) hop - N/2)                   outputs have all their covering frames: nvw_denoise_ready(k, 0).
// A finished stream of length n > N/2 has n / hop + 1 frames and n outputs; one of n <= N/2, for which the reflection is undefined,
// is delivered unchanged.  All of that is host knowledge, so pieces and (piece, frame) pairs are laid out before the launch.
//
// Work split: the N dimension of v_mfma_f32_16x16x4_f32 is 16 (piece, frame) pairs gathered ACROSS columns -- a column result of
// the matrix instruction depends on its own B column only.  A step's new frames q(k0) .. q(k1) - 1 of every piece (up to n / hop
// for a piece that finishes) are laid into tiles of 16 in piece order, a piece's frames never straddling two tiles; one four-wave
// workgroup per tile, and one per piece without a new frame (it moves its state on, and delivers a short stream unchanged).  A step
// that gives some piece more than 16 frames is issued by the session as several launches over sub-ranges of its samples.
//   staging  B operand [16 pairs][J' + 4] fp32 in LDS: pair c holds the N samples of its frame, each from the column's history
//            image (below the piece) or from window row (T + i - k0) mod W through the mu-law PCM table, reflected at the origin
//            and, for a finishing piece, at the stream's end; zero past N.  Lane (g, fl) reads word fl (J' + 4) + 16 q + 4 e + g:
//            J' + 4 is 4 mod 8, so fl (J' + 4) runs over sixteen distinct multiples of 4 mod 64 and the 64 lanes hit 64 banks.
//   forward, gain, inverse   as denoise_kernel, expression for expression: the same tables, the same k-step order per
//            accumulator, the same rotated spectrum image, the same CH / CI choice -- so a frame's synthesis is bit for bit §6r's.
//   add      the synthesis tiles overlay the staged frames ([16][J' + 4]).  Per piece of the tile, four positions to a thread: the
//            carried accumulator (+0 where there is none), then the new frames in ascending f -- denoise_kernel's order of
//            summation, hence its bits --; positions below q(k1) hop (all, when the piece finishes) are divided by the envelope
//            summed from the w^2 table, rounded, saturated and stored in [t0, t0 + count); the N - hop behind them are the new
//            accumulator.  No atomics; no workgroup waits for another.
// State per column, two images each (a launch reads one and writes the other, the session flips): the last N PCM values (int16)
// and the N - hop partial sums (fp32) behind the last complete frame's hop.  Rows are indexed through the session's column-to-row
// map, so a move costs no launch.  LDS: 4 (32 K' + 16 (J' + 4)) bytes, never more than denoise_kernel's.  Compiled once.
#pragma once

#include <hip/hip_runtime.h>

namespace wn {

// one piece of one launch as the kernel reads it; indices count from the stream origin
struct DenoisePiece {
    int slot;                // column
    int row;                 // its row of the state images
    int n;                   // samples of the launch's range, 1 .. W: window rows T .. T + n - 1
    int flags;               // kDenoiseFin: the stream ends with this range
    long long k0;            // samples of the stream before it
    long long offset;        // element of the PCM output that takes output t0 = max(0, q0 hop - N/2)
    int q0;                  // frames complete before
    int nf;                  // new frames q0 .. q0 + nf - 1, at most 16
    int count;               // outputs, may be 0
    int col0;                // the N-column of frame q0 in its tile
    float strength;
    int pad[3];
};
static_assert(sizeof(DenoisePiece) == 64, "DenoisePiece layout");
constexpr int kDenoiseFin = 1;
// one N-column of a tile: frame `frame` of piece `piece` of the launch (piece < 0: none)
struct DenoisePair {
    int piece, frame;
};

inline long long denoise_frames(long long k, int nFft, int hop) { return k > nFft / 2 ? (k - nFft / 2) / hop + 1 : 0; }
inline long long denoise_delivered(long long k, int nFft, int hop) {
    const long long d = denoise_frames(k, nFft, hop) * hop - nFft / 2;
    return d > 0 ? d : 0;
}
inline int denoise_hist_len(int nFft) { return nFft; }
inline int denoise_acc_len(int nFft, int hop) { return nFft - hop; }

struct DenoiseLaunch {
    const DenoisePiece* pieces;   // device memory: the pieces with new frames in tile order, then those without
    const DenoisePair* pairs;     // device memory: [tiles][16]
    int count, framed, tiles;     // pieces in all, those with new frames, their tiles
    const int* y;                 // the window [columns][W] ...
    const short* table;           // ... and the PCM value of every sample index
    int T, W;                     // the range's first window row
    const short* histIn;          // [rows][N]: the image this launch reads ...
    short* histOut;               // ... and the one it writes
    const float* accIn;           // [rows][N - hop], likewise
    float* accOut;
    short* pcm;
    const float *fwdTab, *invTab, *bias, *wnd2;      // wn::Denoiser's tables
    int nFft, hop;
};

// bytes of LDS a workgroup of this geometry takes
size_t slots_deliver_denoise_lds(int nFft, int hop);
// the dynamic-LDS opt-in of the geometry's kernel variant on the current device; false when the runtime refuses
bool slots_deliver_denoise_prepare(int nFft, int hop);
// One launch over a.tiles + (a.count - a.framed) workgroups; asynchronous.  The variant is prepared.
bool slots_deliver_denoise(hipStream_t stream, const DenoiseLaunch& a);

}  // namespace wn
