// slots_prime.hpp -- primed generation: forced sample prefixes.
//
// An utterance may carry a prime y[0 .. n): its local samples k < n ARE y[k] -- delivered, fed back into the history and the
// embeddings like any drawn sample --, and from k = n on it draws as always.  A forced sample travels in the selector the generation
// kernel loads anyway: the value -(1 + y) (exact in fp32 for every alphabet the engine has) means "the sample is y", and
// wavenet_wg<.., RAW = 3> decodes it behind softmax_pick when Params::forced is set for the launch.  ONLY the two kernels below write
// such values, and both clamp y into 0 .. A-1 first, so that nothing from caller memory can index the embedding tables out of range;
// a launch without a forced sample in its range has forced = 0 and reads every selector as the draw it is.
// The kernels (slots_prime.hip) are compiled once for both precisions.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "slots.hpp"
#include "slots_mel.hpp"

namespace wn {

// the selector that stands for the forced sample y of an alphabet of A values
__host__ __device__ inline float prime_selector(int y, int A) { return -(float)(1 + (y < 0 ? 0 : y >= A ? A - 1 : y)); }

// ---- slot mode ----
// One primed column: entry of the device table (at most maxBatch entries, packed).  The host's values are the authority; the table
// is rewritten from them, through pinned staging, by the first step after the set of primed columns has changed -- a prime given,
// moved, dropped or run out -- and by no other: a step whose columns are all where they were reads the table it finds.
struct SlotPrime {
    const int* y;            // the prime, device memory (the caller's; read in stream order by the steps)
    int n;                   // its length
    int column;
};
static_assert(sizeof(SlotPrime) == 16, "SlotPrime layout");

// For every entry, with k0 = counter - start of its column's utterance (from the column's descriptor: desc, or melDesc -- NULL: no
// mel columns -- for a mel column), and every i < count with 0 <= k = k0 + i < n: sel[((T + i) mod W) * maxBatch + column] =
// prime_selector(y[k], A).  Runs behind the descriptor updates, the window feed and the mel feed, whose draws it replaces.  Entries
// with a column outside the batch or without an utterance are skipped.  Asynchronous on `stream`.
bool slots_prime(hipStream_t stream, float* sel, int maxBatch, long long counter, int T, int W, int count, const SlotPrime* tab, int n,
                 const SlotDesc* desc, const MelDesc* melDesc, int A);

// ---- lockstep ----
// The primes of a lockstep engine (setPrime): the host keeps n per column, the device a copy of the values and the second selector
// table that a launch reads while its range holds a forced sample.  Nothing exists until the first prime.
struct PrimeTable {
    explicit PrimeTable(int columns) : columns(columns) {}
    ~PrimeTable();
    PrimeTable(const PrimeTable&) = delete;      // (owns its device buffers)
    bool any() const { return maxN > 0; }
    // column b < batch takes the first n[b] values of y + b * stride (host or device memory; copied); synchronises
    void set(const int* y, const int* n, int batch, int maxLen, long long stride, int maxSamples);
    void clear();                                // no column primed (the buffers stay)

    const int columns;
    std::vector<int> n;                     // [columns] (empty: none)
    int maxN = 0;                           // the longest prime in force
    int primed = 0;                         // columns with n > 0
    int* yDev = NULL;                       // [columns][yStride] the primes' values
    int yStride = 0;
    int* nDev = NULL;                       // [columns]
    float* sel = NULL;                      // [maxSamples][columns] the engine-owned second selector table
};

// Rows [first, first + count) of out ([.][maxBatch]), columns b < batch: prime_selector(y[b * yStride + t], A) for t < n[b], otherwise
// what the launch would have used -- philox_selector(seed, {t, b}) when useRng, else selIn[t * maxBatch + b] (a value <= -1 of the
// caller's, which is no draw, is passed on as -0.5: every negative selector picks index 0, and none of the caller's is decoded).
// selIn is only read.  Asynchronous on `stream`.
bool prime_selectors(hipStream_t stream, float* out, int first, int count, int batch, int maxBatch, const int* y, int yStride, const int* n,
                     int useRng, unsigned long long seed, const float* selIn, int A);

}  // namespace wn
