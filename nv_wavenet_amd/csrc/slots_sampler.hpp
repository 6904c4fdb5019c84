// slots_sampler.hpp -- the sampling temperature of every column.
//
// The generation kernel's softmax computes exp2(x c - m c) with c = log2(e) / T (softmax_pick; Params::softScale, [maxBatch] floats
// on the device, read by wavenet_wg<.., RAW = 3>).  The host keeps T per column and is the authority; the device table follows it:
// a lockstep caller uploads it whole (setTemperatures), a slot-mode step whose columns changed -- starts, sets, moves, resumes --
// scatters {column, c} pairs into it with one small launch ahead of the generation launch.  T = 1 gives c = log2(e) exactly, and
// for T a power of two c and m c are exact scalings: the samples are those of the same model with Wza / T and Bza / T.
// The kernel (slots_sampler.hip) is compiled once for both precisions.
#pragma once

#include <hip/hip_runtime.h>

#include <string.h>

#include <vector>

namespace wn {

constexpr float kSoftScaleUnit = 1.44269504088896340736f;      // log2(e): T = 1 (wn::kLog2e of wn_kernels.hpp)
constexpr float kTemperatureMin = 0x1p-10f, kTemperatureMax = 0x1p10f;

// finite and within [2^-10, 2^10] (a NaN fails both comparisons).  Greedy decoding is not a temperature: a very small T approaches
// the argmax but keeps drawing between logits that tie at the maximum.
inline bool temperature_ok(float T) { return T >= kTemperatureMin && T <= kTemperatureMax; }
inline float temperature_scale(float T) { return kSoftScaleUnit * (1.0f / T); }
// The word that carries T in a state blob (SlotStateHeader::pad[0]): the bits of the float; T = 1 is all-zero bits, so that blobs
// of utterances at T = 1 are byte for byte what they were before temperatures existed.
inline int temperature_word(float T) {
    int w = 0;
    if (T != 1.0f) memcpy(&w, &T, sizeof(w));
    return w;
}
// false: the word is neither zero nor a valid temperature
inline bool temperature_of_word(int w, float& T) {
    T = 1.0f;
    if (w != 0) memcpy(&T, &w, sizeof(T));
    return temperature_ok(T);
}

// The table itself, lockstep and slot mode: the host's values are the authority, the device table follows them.  Nothing is
// allocated, and Params::softScale stays NULL, until a temperature other than 1 has been set: an engine that never uses the
// feature launches what it launched before.
struct TemperatureTable {
    explicit TemperatureTable(int columns) : columns(columns) {}
    ~TemperatureTable();
    TemperatureTable(const TemperatureTable&) = delete;      // (owns the device table)
    // the temperature in force for column b (1 when none was ever set)
    float get(int b) const { return (b >= 0 && b < (int)T.size()) ? T[b] : 1.0f; }
    // the host's value of column b; the first value other than 1 makes the device table (filled with log2(e); synchronises)
    void set(int b, float t);
    // every column back to T = 1, on the host and in the table (synchronises when the table has to be rewritten: a value other
    // than 1 is in force, or deviceBehind -- the table holds values the host has since taken back)
    void reset(bool deviceBehind);
    // the whole table from the host's values, when it exists (blocking copy)
    void upload();

    const int columns;
    std::vector<float> T;                   // [columns] T per column (empty: 1 everywhere)
    int nonUnit = 0;                        // columns with T != 1
    float* softScale = NULL;                // [columns] log2(e) / T on the device, made at the first use and filled with log2(e)
};

// one changed column of a step
struct SlotScale {
    int column;
    float scale;             // log2(e) / T
};
static_assert(sizeof(SlotScale) == 8, "SlotScale layout");

// table[upd[i].column] = upd[i].scale for the n entries (device memory; columns pairwise distinct, each below `columns`; an entry
// outside the table is skipped).  Asynchronous.
bool slots_set_scales(hipStream_t stream, float* table, int columns, const SlotScale* upd, int n);

}  // namespace wn
