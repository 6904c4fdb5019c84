// time_pass.hpp -- the host side that the time-parallel passes share: prefill (prefill.hpp), scoring (score.hpp, §6j)
// and scoring with carried state (score_carry.hpp, §6l) are uses of ONE pass (time_kernels.hpp).
//
// The pass runs the model over a chunk [k0, k0 + n) of an utterance whose samples are all known: 16 consecutive samples in the MFMA N
// dimension, one launch per layer ordered by the stream -- no grid-wide barrier, no flag, nothing that waits for another workgroup.
// A request optionally has an in-state (a blob at done = k0: the dilated taps and the two history words from before the chunk; without
// one they are zero and 128, a start from silence), an out-state (the blob at done = k0 + n) and the skip path with the head.
//   * plain scoring: k0 = 0, no states;
//   * prefill: the chunk [t0, n) of a prime, no in-state, an out-state, no skip path and no last layer (its residual is in no ring);
//   * scoring with carried state: all of it.
// Lane column r = 16 * tile + j of a request is local sample k = k0 + r and scratch row row0 + r; y and x of a job start at the chunk.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include "slots_session.hpp"

namespace wn {

// one request as the kernels see it
struct TimeJob {
    const int* y;            // y[r]: local sample k0 + r, clamped into 0 .. A-1 as slot_prime_kernel clamps
    const void* x;           // x[c * cStride + r * tStride]: feature column k0 + r
    long long cStride, tStride;
    const char* in;          // the in-state, NULL without
    char* out;               // the out-state, NULL without
    float* logp;             // (head) n floats
    float* rows;             // (head) NULL, or n * A floats
    long long row0;          // first scratch row of the request
    int n, tiles, precision, k0;
    unsigned uid;            // header of the out-state
    int temp;                // ... its word 10
    int yInPrev, yInCur;     // y(k0 - 2), y(k0 - 1) where y does not hold them: the in-state's history words, 128 from silence
    int yBefore;             // samples readable in front of y: 2 for a prefill window with t0 > 0, else 0
    float scale;             // (head) log2(e) / T
};
static_assert(sizeof(TimeJob) == 112, "TimeJob layout");
// one layer's launch: where its matrices start in a wave's stream (1-KiB fragments), its dilation and first blob slot, and the ring
// of the layer it produces the input of
struct TimeLayer {
    unsigned cond, prev, cur, res, skip;
    int d, off;
    int dOut, offOut;
};
// the model as the engine holds it
struct TimeModel {
    bool f16;
    int R, S, A, numLayers, maxDilation, ringSlots, nCond, tanhEmbed;
    const void* wblob;       // NW per-wave streams with the conditioning weights (m_wblobF)
    size_t waveStreamFrags;
    unsigned headZs, headZa; // where Wzs and Wza start in a wave's stream
    const float* bias;       // [L][biasL]: Bh + bcond | Bres | Bskip, then Bzs[A], Bza[A] (m_biasF)
    int biasL;
    const void *embPrev, *embCur;
    TimeLayer layers[128];
};

inline long long padded_samples(int n) { return ((long long)n + 15) & ~15LL; }
inline int time_row_bytes(const TimeModel& m) { return m.R * (m.f16 ? 2 : 4); }
inline size_t time_blob_bytes(const TimeModel& m) { return sizeof(SlotStateHeader) + (size_t)m.ringSlots * time_row_bytes(m); }

// device memory (-> p) or mapped pinned host memory (-> its device-side address); NULL for anything else
inline void* store_target(void* p) {
    const int type = pointer_type(p);
    if (type == hipMemoryTypeDevice || type == hipMemoryTypeManaged) return p;
    if (type != hipMemoryTypeHost) return NULL;
    void* d = NULL;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
        (void)hipGetLastError();
        return NULL;
    }
    return d;
}

// what every pass refuses of a call and of a request's inputs.  ownX: x lies in the engine's own feature rows (mel_time.hpp) and is
// not looked at.
inline bool time_call_ok(const TimeModel& m, const void* reqs, int count) { return m.nCond > 0 && reqs != NULL && count >= 1 && count <= 65535; }
inline bool time_inputs_ok(const int* y, int n, const void* x, int precision, long long cStride, long long tStride, float temperature, bool ownX) {
    if (n < 1 || y == NULL || (precision != 32 && precision != 16) || cStride <= 0 || tStride <= 0 || !temperature_ok(temperature) ||
        !is_device_ptr(y))
        return false;
    return ownX || (x != NULL && is_device_ptr(x));
}

// the header of an out-state but for the words the finish step takes from the job
inline SlotStateHeader time_blob_header(const TimeModel& m) {
    SlotStateHeader hdr = {};
    hdr.magic = kSlotStateMagic;
    hdr.version = kSlotStateVersion;
    hdr.precision = m.f16 ? 16 : 32;
    hdr.R = m.R;
    hdr.numLayers = m.numLayers;
    hdr.maxDilation = m.maxDilation;
    return hdr;
}

// The scratch of one call, [cells padded samples] each: the fp32 running residual, two T_data images of x laid out as blob slots
// are ([fragment][g] pieces of 16 bytes), and -- with the skip path -- the fp32 skip sum.
inline size_t time_scratch_bytes(bool f16, int R, int S) { return (size_t)R * 4 + 2 * (size_t)R * (f16 ? 2 : 4) + (size_t)S * 4; }
struct TimeScratch {
    float* xf;
    char *xd0, *xd1;
    float* skf;
};
inline TimeScratch time_carve(char* base, size_t cells, const TimeModel& m) {
    TimeScratch s;
    s.xf = (float*)base;
    s.xd0 = base + cells * m.R * 4;
    s.xd1 = s.xd0 + cells * time_row_bytes(m);
    s.skf = (float*)(s.xd1 + cells * time_row_bytes(m));
    return s;
}

// A buffer that grows on demand (and then synchronises: an earlier call may still be using what is replaced).
class GrowBuffer {
public:
    GrowBuffer() {}
    GrowBuffer(const GrowBuffer&) = delete;
    ~GrowBuffer() {
        if (m_p) gpuErrChk(hipFree(m_p));
    }
    char* atLeast(size_t need) {
        if (need > m_bytes) {
            gpuErrChk(hipDeviceSynchronize());
            if (m_p) gpuErrChk(hipFree(m_p));
            m_p = NULL;
            m_bytes = 0;
            gpuErrChk(hipMalloc((void**)&m_p, need));
            m_bytes = need;
        }
        return m_p;
    }
    char* data() const { return m_p; }

private:
    char* m_p = NULL;
    size_t m_bytes = 0;
};

// The jobs of a call on their way to the device: filled in pinned staging, two halves (and two device arrays) used by alternate
// calls, as a list save stages its entries.
class TimeJobs {
public:
    // `count` zeroed jobs to fill
    TimeJob* begin(int count) {
        if (count > m_cap) {
            m_dev.atLeast(2 * (size_t)count * sizeof(TimeJob));
            m_stage.make(2, (size_t)count * sizeof(TimeJob));
            m_cap = count;
        }
        m_half = m_stage.at();
        TimeJob* const host = (TimeJob*)m_stage.acquire();
        memset(host, 0, (size_t)count * sizeof(TimeJob));
        return host;
    }
    // ... queued for the device on `stream`: where the kernels read them
    const TimeJob* send(const TimeJob* host, int count, hipStream_t stream) {
        TimeJob* const dev = (TimeJob*)m_dev.data() + (size_t)m_half * m_cap;
        gpuErrChk(hipMemcpyAsync(dev, host, (size_t)count * sizeof(TimeJob), hipMemcpyHostToDevice, stream));
        m_stage.release(stream);
        return dev;
    }

private:
    GrowBuffer m_dev;
    StageRing m_stage;
    int m_cap = 0, m_half = 0;
};

}  // namespace wn
