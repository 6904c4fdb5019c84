// resample.hpp -- sample-rate conversion by a rational factor L / M: a polyphase FIR as an fp32 matrix-instruction GEMM, batched,
// ragged and by output range.
//
// The PCM <-> engine boundary at rates other than the model's: recordings arrive at 44.1 / 48 / 16 kHz, a serving stack delivers at
// 8 / 16 / 44.1 / 48 kHz.  L the up factor, M the down factor, coprime; prototype taps h[0 .. T), T odd, centre c = (T - 1) / 2,
// defined at rate L * rate_in with the gain of L folded in.  A stream x[i] by absolute index i >= 0, zero for i < 0 and, when the
// request says `last`, from its end on:
//   out[m] = sum_i x[i] h[c + m M - i L]   over the i with 0 <= c + m M - i L < T,   i in [ceil((m M - c) / L), floor((m M + c) / L)]
// in PCM units (nothing is divided by 32768), accumulated in fp32; an int16 output is the sum rounded to nearest-even and saturated
// to [-32768, 32767].  A complete stream of n samples has ceil(n L / M) outputs.
//
// One launch per call over (request, tile of 16 G consecutive blocks), a workgroup of four waves per tile.
//   GEMM     a block is Q = L q consecutive outputs b Q + p, q the smallest with L q >= 16 and q M >= 4: outputs m and m + L share a
//            phase, so every block multiplies the same table H[p][j] = h[c + p M - (j + j0) L] (zero outside [0, T); float64 rounded
//            to fp32; rows padded to 16s with zero rows, columns to W' = 16 ceil(W / 16) with zero columns) by the W inputs
//            b q M + j0 + j, j0 = -floor(c / L), W = floor(((Q - 1) M + c) / L) - j0 + 1.  H is stored in A-fragment order of
//            v_mfma_f32_16x16x4_f32: one 16-byte load per lane is four k-steps of a row tile.  Blocks are counted from output 0,
//            not from the request's first output: an output's row and the order of its sum do not depend on the range asked for,
//            which is what makes a range, or any chunking of a stream, bit for bit the whole call.
//   inputs   16 consecutive blocks are the N dimension; the B operand of input j of block lane f is read at f * hop + j, hop = q M
//            (a Toeplitz read: every input stored once, read about W / hop times).  The tile's span of (16 G - 1) hop + W' inputs
//            is staged in LDS once as fp32 -- int16 is converted there --, zero where the stream has none.  Position l lies at
//            word l + s (l / hop) with s = (4 - hop) mod 8 spare words per hop: block lanes are hop + s = 4 (mod 8) words apart,
//            which is 4 times an odd number modulo 64, so the 64 lanes of a read (16 blocks x 4 inputs) hit 64 banks whatever
//            the hop (441 takes s = 3, 147 s = 1, a multiple of 32 s = 4), except where a hop boundary falls inside the four.
//   waves    with four or more row tiles (G = 1) row tile t belongs to wave t mod 4, a wave holds up to five accumulators and makes
//            as many passes over the span as that takes; with fewer (G = 4: L = 1, 2, 3, 7 ...) every wave holds all row tiles
//            and takes its own group of 16 blocks of the 64 the workgroup staged: no idle wave, no reduction across waves.
//   store    accumulator to int16 (rint, saturate) or fp32, outputs of [m0, m0 + count) only, plain vector stores.
// Touches no ring, column or session; works inside and outside slot mode.
#pragma once

#include <hip/hip_runtime.h>

#include "slots_session.hpp"

namespace wn {

// one request (nvw_resample_req)
struct ResampleReq {
    const void* in;          // device memory, nIn samples of inType bits (16: int16, 32: fp32): absolute inputs first .. first + nIn - 1
    int inType;
    long long first;
    int nIn;
    int last;                // 1: the stream ends at first + nIn
    void* out;               // device memory, count samples of outType bits: outputs m0 .. m0 + count - 1
    int outType;
    long long m0;
    int count;
};
// ... as the kernel sees it
struct ResampleJob {
    const void* in;
    void* out;
    long long first, m0;
    long long block0;        // m0 / Q
    int nIn, count;
    int blocks;              // of the range: (m0 + count - 1) / Q - block0 + 1
    int tile0;               // its first tile among those of the call
    int inType, outType;
};
static_assert(sizeof(ResampleJob) == 64, "ResampleJob layout");

constexpr int kResampleLdsMax = 160 * 1024;      // of a workgroup (gfx950)
constexpr int kResampleFactorMax = 640;           // 48 kHz <-> 44.1 kHz is 160 / 147, 8 kHz <-> 44.1 kHz 441 / 80

// what follows from (L, M, T) alone
struct ResampleGeom {
    int q, Q, hop;           // blocks of Q = L q outputs, q M inputs apart
    int j0, wp;              // the first input of block 0; W'
    int rowTiles;            // ceil(Q / 16)
    int groups;              // G: 16-block groups of a workgroup, 4 with fewer than four row tiles, else 1
    int spare;               // s
    long long spanWords;     // words of LDS: (16 G - 1) hop + W' + s (that / hop + 1)
};
ResampleGeom resampleGeom(int up, int down, int nTaps);
struct ResampleTab;      // (resample_core.hpp)

// The engine-owned side: the table of one ratio and the requests' staging.  Calls of one engine are issued on one stream, or ordered
// by the caller.
class Resampler {
public:
    Resampler() {}
    Resampler(const Resampler&) = delete;
    ~Resampler() { clear(); }
    // the factors and the caller's taps (host memory, float64).  Builds the table in float64, rounds to fp32, uploads; synchronises.
    // false, with the previous contents kept: up or down outside 1 .. 640 or not coprime, nTaps even or < 1, no taps, or a span
    // beyond the LDS of a workgroup.
    bool set(int up, int down, const double* taps, int nTaps);
    bool ready() const { return m_tab != NULL; }
    // ceil(n up / down); 0 when not set or n < 1
    long long count(long long n) const { return ready() && n > 0 ? (n * m_up + m_down - 1) / m_down : 0; }
    // what run() refuses, without touching the GPU's queues
    bool acceptable(const ResampleReq* reqs, int count) const;
    // count requests in one launch, asynchronously on `stream`.  false with nothing written or launched: a refused request.
    bool run(const ResampleReq* reqs, int count, hipStream_t stream);
    // what another kernel over the same table needs (slot mode's rate delivery, slots_deliver_rate.hpp): the factors, the centre,
    // the geometry, the table as the GEMM core reads it, and CH of the kernel variant (resample_core.hpp)
    int up() const { return m_up; }
    int down() const { return m_down; }
    int centre() const { return m_centre; }
    const ResampleGeom& geom() const { return m_g; }
    ResampleTab tab() const;
    int tilesPerPass() const;

private:
    void clear();
    int m_up = 0, m_down = 0, m_centre = 0;
    ResampleGeom m_g = {};
    float* m_tab = NULL;         // [rowTiles][W' / 16][64 lanes] x 4
    ResampleJob* m_jobs = NULL;
    int m_jobCap = 0;
    bool m_ldsReady = false;     // the dynamic-LDS opt-in of this ratio's kernel has been made on this engine's device
    StageRing m_stage;
};

}  // namespace wn
