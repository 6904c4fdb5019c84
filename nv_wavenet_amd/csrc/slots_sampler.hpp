// slots_sampler.hpp -- the sampling temperature and the probability floor (min-p, §6m) of every column.
//
// The generation kernel's softmax computes exp2(x c - m c) with c = log2(e) / T (softmax_pick; Params::softScale, [maxBatch] floats
// on the device, read by wavenet_wg<.., RAW = 3>).  The host keeps T per column and is the authority; the device table follows it:
// a lockstep caller uploads it whole (setTemperatures), a slot-mode step whose columns changed -- starts, sets, moves, resumes --
// scatters {column, c} pairs into it with one small launch ahead of the generation launch.  T = 1 gives c = log2(e) exactly, and
// for T a power of two c and m c are exact scalings: the samples are those of the same model with Wza / T and Bza / T.
// The floor tau of a column drops the bins whose tempered probability is below tau times that of the most probable bin: the kernel
// zeroes e = exp2(x c - m c) < tau before the sum (softmax_pick).  The floors are the second half of the same table,
// softScale[columns + b], read only by a launch whose Params::floorOn is set; they travel exactly as the scales do.
// The tail cuts of a column (top-k and top-p, §6n) are two more thresholds on the same e: the kernel finds them by a bisection over
// the bit patterns of e (cut_threshold) and floors at the largest of the three.  Top-k (an integer, as its bits) and top-p are the
// third and fourth quarter of the table, read only by a launch whose Params::floorOn has bit 1 set.
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

// The probability floor: finite and within [0, 0.5] (a NaN fails both comparisons).  0.5 is where the guarantee ends that the most
// probable bin survives: its e is 2^(rounding error of m c), at least 2^-0.5 while |m c| < 2^23.
constexpr float kMinPMax = 0.5f;
inline bool min_p_ok(float p) { return p >= 0.0f && p <= kMinPMax; }
// The word that carries the floor in a state blob (SlotStateHeader::pad[1]): the bits of the float; 0 (and -0) is all-zero bits.
inline int min_p_word(float p) {
    int w = 0;
    if (p != 0.0f) memcpy(&w, &p, sizeof(w));
    return w;
}
// false: the word is neither zero nor a valid floor (the bits of -0 among them: min_p_word never writes them)
inline bool min_p_of_word(int w, float& p) {
    p = 0.0f;
    if (w == 0) return true;
    memcpy(&p, &w, sizeof(p));
    return min_p_ok(p) && p != 0.0f;
}

// Top-k: an integer in [0, A]; 0 is off (every bin stays), and so in effect is A.
inline bool top_k_ok(int k, int A) { return k >= 0 && k <= A; }
// The word that carries top-k in a state blob (SlotStateHeader::pad[2]): the integer itself.
inline int top_k_word(int k) { return k; }
// false: the word is outside [0, A]
inline bool top_k_of_word(int w, int A, int& k) {
    k = 0;
    if (!top_k_ok(w, A)) return false;
    k = w;
    return true;
}
// Top-p (nucleus): finite and within (0, 1] (a NaN fails both comparisons); 1 is off.
inline bool top_p_ok(float p) { return p > 0.0f && p <= 1.0f; }
// The word that carries top-p in a state blob (SlotStateHeader::pad[3]): the bits of the float, all-zero bits for 1.
inline int top_p_word(float p) {
    int w = 0;
    if (p != 1.0f) memcpy(&w, &p, sizeof(w));
    return w;
}
// false: the word is neither zero nor a valid top-p (the bits of 1.0 among them: top_p_word never writes them)
inline bool top_p_of_word(int w, float& p) {
    p = 1.0f;
    if (w == 0) return true;
    memcpy(&p, &w, sizeof(p));
    return top_p_ok(p) && p != 1.0f;
}
// a table entry that holds top-k: the integer's bits in the float's place
inline float top_k_entry(int k) {
    float f;
    memcpy(&f, &k, sizeof(f));
    return f;
}

// A column's sampling: the four values above, each off by default.  Their order here is the order of the kinds everywhere: kind i is
// header word SlotStateHeader::pad[i] of a state blob and quarter i of the device table (entry i * columns + b for column b).
struct Sampling {
    float temperature = 1;
    float minP = 0;
    int topK = 0;
    float topP = 1;
};
enum { kTemperature, kMinP, kTopK, kTopP, kSamplingKinds };
inline bool operator==(const Sampling& a, const Sampling& b) {
    return a.temperature == b.temperature && a.minP == b.minP && a.topK == b.topK && a.topP == b.topP;
}
inline bool sampling_ok(const Sampling& s, int A) {
    return temperature_ok(s.temperature) && min_p_ok(s.minP) && top_k_ok(s.topK, A) && top_p_ok(s.topP);
}
// the four header words; a kind's word is zero exactly when the kind is off
inline void sampling_words(const Sampling& s, int pad[4]) {
    pad[kTemperature] = temperature_word(s.temperature);
    pad[kMinP] = min_p_word(s.minP);
    pad[kTopK] = top_k_word(s.topK);
    pad[kTopP] = top_p_word(s.topP);
}
// false: one of the words is not valid (s holds what the valid ones say, off for the others)
inline bool sampling_of_words(const int pad[4], int A, Sampling& s) {
    const bool t = temperature_of_word(pad[kTemperature], s.temperature), p = min_p_of_word(pad[kMinP], s.minP);
    const bool k = top_k_of_word(pad[kTopK], A, s.topK), q = top_p_of_word(pad[kTopP], s.topP);
    return t && p && k && q;
}
// the four table entries
inline void sampling_entries(const Sampling& s, float out[4]) {
    out[kTemperature] = temperature_scale(s.temperature);
    out[kMinP] = s.minP;
    out[kTopK] = top_k_entry(s.topK);
    out[kTopP] = s.topP;
}

// The table itself, lockstep and slot mode: the host's values are the authority, the device table follows them.  Nothing is
// allocated, and Params::softScale stays NULL, until a value that is not off has been set: an engine that uses none launches what
// it launched before.  The device table is [4][columns]: the scales, the floors, top-k (integers) and top-p.
struct SamplingTable {
    explicit SamplingTable(int columns) : columns(columns) {}
    ~SamplingTable();
    SamplingTable(const SamplingTable&) = delete;      // (owns the device table)
    // the values in force for column b (off when none was ever set)
    Sampling get(int b) const { return (b >= 0 && b < (int)rows.size()) ? rows[b] : Sampling{}; }
    // the host's values of column b; the first value that is not off makes the device table (filled with off; synchronises)
    void set(int b, const Sampling& s);
    // columns with a cut in force
    int cutting() const { return on[kTopK] + on[kTopP]; }
    // one value of every column back to off on the host (the caller uploads): the lockstep setters, each of which leaves the others' alone
    template <class V>
    void resetKind(V Sampling::*field) {
        for (int b = 0; b < (int)rows.size(); b++) {
            Sampling s = rows[b];
            s.*field = Sampling{}.*field;
            set(b, s);
        }
    }
    // every column back to off, on the host and in the table (synchronises when the table has to be rewritten: a value that is not
    // off is in force, or deviceBehind -- the table holds values the host has since taken back)
    void reset(bool deviceBehind);
    // the whole table from the host's values, when it exists (blocking copy)
    void upload();

    const int columns;
    std::vector<Sampling> rows;             // [columns] (empty: off everywhere)
    int on[kSamplingKinds] = {};            // per kind, the columns whose value is not off
    float* softScale = NULL;                // [4][columns] on the device, made at the first use: log2(e) / T, filled with log2(e); then
                                            // the floors, filled with 0; top-k as integers, filled with 0; top-p, filled with 1
private:
    void make();
};

// one changed table entry of a step
struct SlotScale {
    int column;              // the entry: b for the scale of column b, columns + b for its floor, 2 columns + b for its top-k,
                             // 3 columns + b for its top-p
    float scale;             // log2(e) / T, the floor, top-k (top_k_entry) or top-p
};
static_assert(sizeof(SlotScale) == 8, "SlotScale layout");

// table[upd[i].column] = upd[i].scale for the n entries (device memory; entries pairwise distinct, each below `columns`, the
// length of the table -- four times the engine's batch; an entry outside the table is skipped).  Asynchronous.
bool slots_set_scales(hipStream_t stream, float* table, int columns, const SlotScale* upd, int n);

}  // namespace wn
