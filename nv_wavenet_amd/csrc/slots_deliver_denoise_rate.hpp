// slots_deliver_denoise_rate.hpp -- slot mode: ragged delivery through the bias denoiser AND at the caller's sample rate, in one
// launch.
//
// slot_deliver_denoise_kernel (§6s) delivers cleaned PCM at the model's rate, slot_deliver_rate_kernel (§6q) converts what the model
// generated; a caller who wants cleaned PCM at its own rate had to take the first across the host boundary and convert it on a
// second engine, in a launch whose tiles hold one or two live blocks.  This kernel chains the two inside one workgroup: the cleaned
// samples never leave the chip.  A column's stream x[i] = table[sample i], i from the stream origin s0 (§6s), is cleaned by §6r's
// definition into the int16 stream z (rint, saturated; z = x for a stream that finishes at N / 2 samples or fewer), z is converted
// by §6p's definition at L / M, and the outputs are numbered from 0 at s0.  After k samples of an unfinished stream
//   R(D(k)) = rate_delivered(denoise_delivered(k))   outputs are out; the finishing piece carries the rest up to ceil(n L / M).
// All of that is host knowledge.  An utterance's pieces, concatenated, are bit for bit nvw_resample of nvw_denoise of its whole PCM.
//
// Front half: §6s's tile, expression for expression -- (piece, frame) pairs from the host, staging, forward GEMM, gain, inverse
// GEMM, overlap-add order -- so a cleaned sample has §6r's bits.  The overlap-add does not store to the PCM buffer: it stores
// resample_pcm16(y / env) as fp32 into the piece's SPAN in LDS, and the last H of them as int16 into the column's new tail.
//   spans    the span area overlays the spectrum image, dead behind the barrier that follows the inverse GEMM.  Each piece of the
//            tile has a span of its own in §6p's spare-word layout (position l at word l + s (l / hop_r), hop_r = q M), laid out
//            against the block grid counted from the utterance's output 0: position 0 is input block0 hop_r + j0 of z.  Positions
//            in [t0, t1) = [D(k0), D(k0 + n)) (up to the stream's end where it finishes) are the overlap-add's; [t0 - H, t0) come
//            from the column's carried tail of z (zero below the origin or under kRateZeroTail); everything else is zero -- past
//            the end of a finished stream that is the definition, elsewhere it is read only by outputs that are not stored.
//   rate     the N dimension of v_mfma_f32_16x16x4_f32 is 16 (piece, block) pairs gathered ACROSS the pieces of the tile, every
//            lane with its own span base: one frame per step yields 1 to 2 blocks of a piece, sixteen consecutive blocks of one
//            piece would be dead lanes.  The pairs come from the host next to the frame pairs (DESIGN.md §6t says why).  The
//            k-step order per accumulator, the table and the G / CH choice are resample_tile_gemm's (resample_gather_gemm of
//            resample_core.hpp), so an output has nvw_resample's bits.  The workgroup loops over its groups of 16 pairs; outputs in
//            [m0, m0 + count) go to the PCM buffer with plain vector stores.  No atomics; no workgroup waits for another.
// A piece without a new frame keeps its one workgroup: it moves the three states on, and for a short finishing stream stages z = x
// and converts it.
// State per column, two images each, flipped together per launch: §6s's history (N int16) and accumulator (N - hop fp32), §6q's
// tail of z (H int16); all indexed through the session's column-to-row map.
//
// LDS: 4 (max(32 K', S) + 16 (J' + 4)) bytes, S the span words of a tile.  With Z the cleaned samples of a tile, B its blocks:
//   Z <= 16 hop + F N/2     16 new frames; a finishing piece adds N / 2 and has at least (N/2) / hop frames, so F = 16 / ((N/2) / hop)
//   B <= Z / hop_r + 1 + 16 ((c + M) / (M Q) + 3)     a piece of z cleaned samples has at most (z L + c) / M + 2 outputs, which
//                           touch at most (outputs - 1) / Q + 2 blocks; at most 16 pieces
//   S <= B (hop_r + s) + 16 (W' + s ((W' - 1) / hop_r))     a span of b blocks is (b - 1)(hop_r + s) + W' + s ((W' - 1) / hop_r) words
// (slots_deliver_denoise_rate_span_words).  The session checks every tile it lays out against S.
#pragma once

#include <hip/hip_runtime.h>

#include "resample_core.hpp"
#include "slots_deliver_denoise.hpp"
#include "slots_deliver_rate.hpp"

namespace wn {

// one piece of one launch as the kernel reads it
struct DenoiseRatePiece {
    DenoisePiece d;          // §6s's record; count = cleaned samples t1 - t0 of the range, offset = element of the PCM output that
                             // takes output m0; flags may carry kRateZeroTail << 1
    long long m0;            // first output of the range: R(t0)
    long long block0;        // m0 / Q
    int count;               // outputs, may be 0
    int blocks;              // of the range: (m0 + count - 1) / Q - block0 + 1; 0 when count is 0
    int span;                // word of the tile's span area where its span begins
    int pair0;               // its first (piece, block) pair among the launch's; its blocks follow each other
};
static_assert(sizeof(DenoiseRatePiece) == 96, "DenoiseRatePiece layout");
constexpr int kDenoiseRateZeroTail = kRateZeroTail << 1;
// one N-column of the rate GEMM: block block0 + `block` of piece `piece` of the launch
struct RatePair {
    int piece, block;
};

// what the two stages' geometries give this one (wn::Denoiser, wn::ResampleGeom)
struct DenoiseRateGeom {
    int nFft, hop;           // N and the frame hop
    int up, down, centre;    // L, M, c
    int Q, hopR, spare, wp;  // outputs of a block, its input hop q M, s, W'
};
// the composed count: outputs delivered after k samples of an unfinished stream
inline long long denoise_rate_delivered(long long k, const DenoiseRateGeom& g) {
    return rate_delivered(denoise_delivered(k, g.nFft, g.hop), g.up, g.down, g.centre);
}
// words of a span of b >= 1 blocks
inline long long denoise_rate_span_of(const DenoiseRateGeom& g, long long b) {
    return (b - 1) * (g.hopR + g.spare) + g.wp + (long long)g.spare * ((g.wp - 1) / g.hopR);
}
// the most blocks that z cleaned samples of one piece touch
inline long long denoise_rate_blocks_most(const DenoiseRateGeom& g, long long z) {
    return ((z * g.up + g.centre) / g.down + 1) / g.Q + 2;
}
// S: the span words that a tile can need (the bound above)
long long slots_deliver_denoise_rate_span_words(const DenoiseRateGeom& g);

struct DenoiseRateLaunch {
    const DenoiseRatePiece* pieces;   // device memory: the pieces with new frames in tile order, then those without
    const DenoisePair* pairs;         // device memory: [tiles][16]
    const RatePair* ratePairs;        // device memory: the pieces' blocks in piece order
    DenoiseLaunch l;                  // §6s's launch (its pieces NULL; pcm takes the rate outputs)
    const short* tailIn;              // [rows][H]: the image this launch reads ...
    short* tailOut;                   // ... and the one it writes
    int H;
    ResampleTab t;
};

// bytes of LDS a workgroup takes
size_t slots_deliver_denoise_rate_lds(int nFft, long long spanWords);
// the dynamic-LDS opt-in of the kernel variant on the current device; false when the budget exceeds a workgroup's LDS or the
// runtime refuses
bool slots_deliver_denoise_rate_prepare(int nFft, long long spanWords, int groups, int ch);
// One launch over l.tiles + (l.count - l.framed) workgroups; asynchronous.  The variant is prepared.
bool slots_deliver_denoise_rate(hipStream_t stream, const DenoiseRateLaunch& a, long long spanWords, int groups, int ch);

}  // namespace wn
