// slots_state.hpp -- slot mode: a column's state as a value: moved to another column, saved into a blob, resumed
// from one -- in another column, at another counter, in another engine of the same model and seed.
//
// Between steps an utterance owns on the device its column's share of the dilation ring (lanes 16g + j of every 1-KiB fragment of
// every slot of its tile, the bytes slot_reset_kernel zeroes), two history words and its descriptor; the window carries nothing
// forward.  The ring slot of layer l at engine counter t is off_l + (t mod d_l): a column's ring is phased to the engine's counter.
// A blob holds layer l's d_l slots rotated so that blob slot off_l + (k mod d_l) is the one local sample k reads and writes -- the
// ring the utterance would have had if it had started at counter 0: save reads ring slot off_l + ((i + start) mod d_l) into blob
// slot off_l + i, load writes blob slot off_l + i to ring slot off_l + ((i + start') mod d_l), start' = counter of the resuming step
// - done.  Slots not yet written (k < d_l) are zero on either side.  16-byte moves only: nothing is converted or recomputed.
// The kernels (slots_state.hip) are compiled once for both precisions.
#pragma once

#include <hip/hip_runtime.h>

#include "slots.hpp"
#include "slots_mel.hpp"

namespace wn {

constexpr unsigned kSlotStateMagic = 0x5453574Eu;      // "NWST"
constexpr unsigned kSlotStateVersion = 1;

// the head of a blob (64 bytes; the payload follows: ringSlots x fragsPerSlot x 4 pieces of 16 bytes, [slot][fragment][g])
struct SlotStateHeader {
    unsigned magic, version;
    int precision;           // 32 | 16: the engine's T_data
    int R, numLayers, maxDilation;
    int done;                // local samples generated so far
    unsigned uid;
    int yInPrev, yInCur;     // the column's sample history
    int pad[6];              // pad[0]: the sampling temperature as the bits of the float, all-zero bits for T = 1 (slots_sampler.hpp:
                             // blobs of utterances at T = 1 are what they were before temperatures existed); pad[1]: the probability floor likewise,
                             // all-zero bits for floor 0; pad[2]: top-k, the integer (0: off); pad[3]: top-p as the bits of the float, all-zero
                             // bits for 1 (off); the rest zero
};
static_assert(sizeof(SlotStateHeader) == 64, "SlotStateHeader layout");

inline size_t slots_state_bytes(int ringSlots, int fragsPerSlot) {
    return sizeof(SlotStateHeader) + (size_t)ringSlots * fragsPerSlot * 4 * 16;
}

// the schedule per ring slot: x = first slot of the slot's layer, y = its dilation (a power of two)
typedef int2 SlotLayer;

struct SlotMove {
    int from, to;
};
// one resumed column: its blob and the rotation start' mod (largest dilation)
struct SlotLoad {
    const void* state;
    int column;
    int rot;
};
static_assert(sizeof(SlotLoad) == 16, "SlotLoad layout");
// one saved column of a list: where its blob goes (device memory, or the device-side address of mapped pinned host memory), the
// rotation start mod (largest dilation), and the header fields that differ per column
struct SlotSave {
    void* dst;
    int column;
    int rot;
    int done;
    unsigned uid;
    int temp;                // header word 10 (pad[0]): the bits of the column's sampling temperature, 0 for T = 1 (slots_sampler.hpp)
    int minp;                // header word 11 (pad[1]): the bits of the column's probability floor, 0 for floor 0
};
static_assert(sizeof(SlotSave) == 32, "SlotSave layout");
// ... and its tail cuts, in an array beside the entries (SlotSave is full): x = header word 12 (pad[2]), top-k; y = header word 13
// (pad[3]), the top-p word
typedef int2 SlotSaveCut;

// what the host reports per column of a list save, and one request of a list resume (nvw_slot_saved, nvw_slot_resume_req)
struct SlotSaved {
    int slot;
    unsigned uid;
    int done;
    int mel;
};
struct SlotResumeReq {
    int slot;
    int mel;                 // 0: features (slotResume), != 0: mel frames (slotResumeMel)
    const void* src;
    int precision;
    long long cStride, tStride;
    int length;              // feature columns: samples; mel columns: frames
    int final;               // mel columns only
};
static_assert(sizeof(SlotResumeReq) == 48, "SlotResumeReq layout");

// nMoves (from, to) pairs -- sources pairwise distinct, destinations pairwise distinct, no destination a source --: ring share,
// history and descriptors (mel: NULL when the session has no mel columns) of `from` into `to`; `from` goes idle.  Asynchronous.
bool slots_move(hipStream_t stream, const SlotMove* moves, int nMoves, void* ring, int ringSlots, int fragsPerSlot, int* yInPrev,
                int* yInCur, SlotDesc* desc, MelDesc* mel);
// Column `column`, whose utterance started at counter `rot` (mod the largest dilation), into the blob `dst` in canonical order,
// with its header (hdr: everything but the history, which the kernel reads).  Asynchronous.
bool slots_save(hipStream_t stream, void* dst, SlotStateHeader hdr, int column, int rot, const SlotLayer* layers, const void* ring,
                int ringSlots, int fragsPerSlot, const int* yInPrev, const int* yInCur);
// slots_save for nSaves columns in one launch: entry i's column into entry i's dst, hdr = the fields every blob shares (done, uid and
// the history are filled per entry; cuts: entry i's words 12 and 13, NULL when no saved column has a cut -- both words zero).  The
// destinations are pairwise disjoint.  Asynchronous.
bool slots_save_list(hipStream_t stream, const SlotSave* saves, const SlotSaveCut* cuts, int nSaves, SlotStateHeader hdr, const SlotLayer* layers, const void* ring,
                     int ringSlots, int fragsPerSlot, const int* yInPrev, const int* yInCur);
// The nLoads blobs into their columns with the inverse rotation; the history from their headers.  Asynchronous.
bool slots_load(hipStream_t stream, const SlotLoad* loads, int nLoads, const SlotLayer* layers, void* ring, int ringSlots,
                int fragsPerSlot, int* yInPrev, int* yInCur);

}  // namespace wn
