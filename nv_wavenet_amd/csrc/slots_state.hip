// slots_state.hip -- the kernels that take a column's state out of a column and put it into another (slots_state.hpp): move, save
// (one column, a list), load.  Compiled once, both precisions.  Bandwidth kernels over the pieces slot_reset_kernel zeroes: piece r of a column is lanes
// 16g + j (g = r & 3) of fragment r >> 2 of its tile's ring, 16 bytes in a 128-byte line of its own (8 columns share a line, the
// four pieces of a fragment are 256 bytes apart) -- the ring side of every copy is strided whatever the thread order, so the
// threads walk the pieces in blob order and the blob side is one contiguous run of 16-byte vector accesses per wave.
#include "slots_state.hpp"
#include "wn_kernels.hpp"

namespace wn {

// the ring piece of (ring slot, piece within the slot: fragment * 4 + g), in 16-byte units from the column's base
__device__ __forceinline__ int ring_piece(int slot, int q, int pshift) { return (((slot << pshift) + q) >> 2) * 64 + (q & 3) * 16; }

// Column move.  blockIdx.y walks the pairs, x the pieces (the grid of slot_reset_kernel).  Same engine, same counter: no rotation.
// Blocks of column 0 then move the history and the descriptors (`to` takes `from`'s with start unchanged, `from` goes idle).
__global__ __launch_bounds__(256) void slot_move_kernel(const SlotMove* __restrict__ moves, int nMoves, uintx4* __restrict__ ring,
                                                        int ringSlots, int fragsPerSlot, int* __restrict__ yInPrev,
                                                        int* __restrict__ yInCur, SlotDesc* __restrict__ desc, MelDesc* __restrict__ mel) {
    const int per = ringSlots * fragsPerSlot * 4;
    const size_t perTile = (size_t)ringSlots * fragsPerSlot * 64;
    for (int m = blockIdx.y; m < nMoves; m += gridDim.y) {
        const SlotMove mv = moves[m];
        const uintx4* const src = ring + (size_t)(mv.from >> 4) * perTile + (mv.from & 15);
        uintx4* const dst = ring + (size_t)(mv.to >> 4) * perTile + (mv.to & 15);
        for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < per; r += gridDim.x * blockDim.x) {
            const int at = (r >> 2) * 64 + (r & 3) * 16;
            dst[at] = src[at];
        }
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int m = blockIdx.y; m < nMoves; m += gridDim.y) {
        const SlotMove mv = moves[m];
        yInPrev[mv.to] = yInPrev[mv.from];
        yInCur[mv.to] = yInCur[mv.from];
        // (48-byte descriptors as three 16-byte pieces: registers, no private copy)
        const uintx4* const ds = (const uintx4*)(desc + mv.from);
        uintx4* const dd = (uintx4*)(desc + mv.to);
        const uintx4 d0 = ds[0], d1 = ds[1], d2 = ds[2];
        dd[0] = d0;
        dd[1] = d1;
        dd[2] = d2;
        desc[mv.from].active = 0;
        if (mel != NULL) {
            const uintx4* const ms = (const uintx4*)(mel + mv.from);
            uintx4* const md = (uintx4*)(mel + mv.to);
            const uintx4 m0 = ms[0], m1 = ms[1], m2 = ms[2];
            md[0] = m0;
            md[1] = m1;
            md[2] = m2;
            mel[mv.from].state = 0;
        }
    }
}

// Column save: blob piece r = (canonical slot s, q) <- ring slot off + ((s - off + rot) & (d - 1)) of the slot's layer {off, d}.
__global__ __launch_bounds__(256) void slot_save_kernel(uintx4* __restrict__ blob, SlotStateHeader hdr, int column, int rot,
                                                        const SlotLayer* __restrict__ layers, const uintx4* __restrict__ ring,
                                                        int ringSlots, int pshift, const int* __restrict__ yInPrev,
                                                        const int* __restrict__ yInCur) {
    const int per = ringSlots << pshift;
    const uintx4* const src = ring + (size_t)(column >> 4) * ((size_t)per * 16) + (column & 15);
    uintx4* const out = blob + sizeof(SlotStateHeader) / 16;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < per; r += gridDim.x * blockDim.x) {
        const int s = r >> pshift, q = r & ((1 << pshift) - 1);
        const SlotLayer l = layers[s];
        out[r] = src[ring_piece(l.x + ((s - l.x + rot) & (l.y - 1)), q, pshift)];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr.yInPrev = yInPrev[column];
        hdr.yInCur = yInCur[column];
        *(SlotStateHeader*)blob = hdr;
    }
}

// Column save for a list: slot_save_kernel per entry, blockIdx.y striding over the entries (the grid of slot_load_kernel).  The common
// header fields are one argument, done, uid, the temperature word and the floor word come from the entry, the cut words from the array beside them (NULL: zero); every destination is device memory or the device-side address
// of mapped pinned host memory -- the blob side stays contiguous 16-byte stores either way.
__global__ __launch_bounds__(256) void slot_save_list_kernel(const SlotSave* __restrict__ saves, const SlotSaveCut* __restrict__ cuts,
                                                             int nSaves, SlotStateHeader hdr,
                                                             const SlotLayer* __restrict__ layers, const uintx4* __restrict__ ring,
                                                             int ringSlots, int pshift, const int* __restrict__ yInPrev,
                                                             const int* __restrict__ yInCur) {
    const int per = ringSlots << pshift;
    for (int c = blockIdx.y; c < nSaves; c += gridDim.y) {
        const SlotSave sv = saves[c];
        const uintx4* const src = ring + (size_t)(sv.column >> 4) * ((size_t)per * 16) + (sv.column & 15);
        uintx4* const out = (uintx4*)sv.dst + sizeof(SlotStateHeader) / 16;
        for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < per; r += gridDim.x * blockDim.x) {
            const int s = r >> pshift, q = r & ((1 << pshift) - 1);
            const SlotLayer l = layers[s];
            out[r] = src[ring_piece(l.x + ((s - l.x + sv.rot) & (l.y - 1)), q, pshift)];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            SlotStateHeader h = hdr;
            h.done = sv.done;
            h.uid = sv.uid;
            h.pad[0] = sv.temp;
            h.pad[1] = sv.minp;
            if (cuts != nullptr) {
                const SlotSaveCut cut = cuts[c];
                h.pad[2] = cut.x;
                h.pad[3] = cut.y;
            }
            h.yInPrev = yInPrev[sv.column];
            h.yInCur = yInCur[sv.column];
            *(SlotStateHeader*)sv.dst = h;
        }
    }
}

// Column load: blockIdx.y walks the resumed columns; the inverse of the save -- blob piece (s, q) -> ring slot
// off + ((s - off + rot') & (d - 1)) -- and the history from the header.  Every piece of the column is written.
__global__ __launch_bounds__(256) void slot_load_kernel(const SlotLoad* __restrict__ loads, int nLoads, const SlotLayer* __restrict__ layers,
                                                        uintx4* __restrict__ ring, int ringSlots, int pshift, int* __restrict__ yInPrev,
                                                        int* __restrict__ yInCur) {
    const int per = ringSlots << pshift;
    for (int c = blockIdx.y; c < nLoads; c += gridDim.y) {
        const SlotLoad ld = loads[c];
        const uintx4* const in = (const uintx4*)ld.state + sizeof(SlotStateHeader) / 16;
        uintx4* const dst = ring + (size_t)(ld.column >> 4) * ((size_t)per * 16) + (ld.column & 15);
        for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < per; r += gridDim.x * blockDim.x) {
            const int s = r >> pshift, q = r & ((1 << pshift) - 1);
            const SlotLayer l = layers[s];
            dst[ring_piece(l.x + ((s - l.x + ld.rot) & (l.y - 1)), q, pshift)] = in[r];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const SlotStateHeader* const h = (const SlotStateHeader*)ld.state;
            yInPrev[ld.column] = h->yInPrev;
            yInCur[ld.column] = h->yInCur;
        }
    }
}

static int gridOf(int n, int cap) {
    const int g = (n + 255) / 256;
    return g > cap ? cap : (g ? g : 1);
}
// log2 of the pieces of a ring slot (fragsPerSlot x 4); -1 when that is no power of two
static int pieceShift(int fragsPerSlot) {
    const int n = fragsPerSlot * 4;
    int s = 0;
    while ((1 << s) < n) s++;
    return (1 << s) == n ? s : -1;
}

bool slots_move(hipStream_t stream, const SlotMove* moves, int nMoves, void* ring, int ringSlots, int fragsPerSlot, int* yInPrev,
                int* yInCur, SlotDesc* desc, MelDesc* mel) {
    if (nMoves <= 0) return true;
    hipLaunchKernelGGL(slot_move_kernel, dim3(gridOf(ringSlots * fragsPerSlot * 4, 64), nMoves > 1024 ? 1024 : nMoves), dim3(256), 0, stream,
                       moves, nMoves, (uintx4*)ring, ringSlots, fragsPerSlot, yInPrev, yInCur, desc, mel);
    return hipGetLastError() == hipSuccess;
}

bool slots_save(hipStream_t stream, void* dst, SlotStateHeader hdr, int column, int rot, const SlotLayer* layers, const void* ring,
                int ringSlots, int fragsPerSlot, const int* yInPrev, const int* yInCur) {
    const int pshift = pieceShift(fragsPerSlot);
    if (pshift < 0) return false;
    hipLaunchKernelGGL(slot_save_kernel, dim3(gridOf(ringSlots << pshift, 64)), dim3(256), 0, stream, (uintx4*)dst, hdr, column, rot, layers,
                       (const uintx4*)ring, ringSlots, pshift, yInPrev, yInCur);
    return hipGetLastError() == hipSuccess;
}

bool slots_save_list(hipStream_t stream, const SlotSave* saves, const SlotSaveCut* cuts, int nSaves, SlotStateHeader hdr, const SlotLayer* layers, const void* ring,
                     int ringSlots, int fragsPerSlot, const int* yInPrev, const int* yInCur) {
    const int pshift = pieceShift(fragsPerSlot);
    if (pshift < 0) return false;
    if (nSaves <= 0) return true;
    hipLaunchKernelGGL(slot_save_list_kernel, dim3(gridOf(ringSlots << pshift, 64), nSaves > 1024 ? 1024 : nSaves), dim3(256), 0, stream, saves,
                       cuts, nSaves, hdr, layers, (const uintx4*)ring, ringSlots, pshift, yInPrev, yInCur);
    return hipGetLastError() == hipSuccess;
}

bool slots_load(hipStream_t stream, const SlotLoad* loads, int nLoads, const SlotLayer* layers, void* ring, int ringSlots,
                int fragsPerSlot, int* yInPrev, int* yInCur) {
    const int pshift = pieceShift(fragsPerSlot);
    if (pshift < 0) return false;
    if (nLoads <= 0) return true;
    hipLaunchKernelGGL(slot_load_kernel, dim3(gridOf(ringSlots << pshift, 64), nLoads > 1024 ? 1024 : nLoads), dim3(256), 0, stream, loads,
                       nLoads, layers, (uintx4*)ring, ringSlots, pshift, yInPrev, yInCur);
    return hipGetLastError() == hipSuccess;
}

}  // namespace wn
