// prefill.hip -- the host side of wn::Prefill (prefill.hpp) and its instantiations of the time-parallel pass: no skip path,
// R in {32, 64, 128, 256}, both precisions.
#include "prefill.hpp"

#include "time_kernels.hpp"

namespace wn {

bool Prefill::acceptable(const TimeModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, bool ownX) {
    if (!time_call_ok(m, reqs, count)) return false;
    if (m.R != 32 && m.R != 64 && m.R != 128 && m.R != 256) return false;
    const size_t blobBytes = time_blob_bytes(m);
    if (dst == NULL || ((size_t)dst & 15) != 0 || (stride & 15) != 0 || stride < (long long)blobBytes) return false;
    char* const first = (char*)store_target(dst);
    const size_t span = (size_t)(count - 1) * (size_t)stride + blobBytes - 16;
    if (first == NULL || (char*)store_target((char*)dst + span) != first + span) return false;
    for (int i = 0; i < count; i++) {
        const PrefillReq& q = reqs[i];
        if (!time_inputs_ok(q.y, q.n, q.x, q.precision, q.cStride, q.tStride, q.temperature, ownX)) return false;
    }
    return true;
}

bool Prefill::run(const TimeModel& m, const PrefillReq* reqs, int count, void* dst, long long stride, hipStream_t stream, bool ownX) {
    if (!acceptable(m, reqs, count, dst, stride, ownX)) return false;
    char* const first = (char*)store_target(dst);
    const int W = prefill_window(m.ringSlots);
    TimeJob* const jobs = m_jobs.begin(count);
    int maxTiles = 0;
    long long total = 0;
    for (int i = 0; i < count; i++) {
        const PrefillReq& q = reqs[i];
        TimeJob& jb = jobs[i];
        // the chunk [t0, n): y and x from its first sample on; its history words lie in front of y when t0 > 0
        const int t0 = prefill_first(q.n, W);
        jb.y = q.y + t0;
        jb.x = ownX ? q.x : (const char*)q.x + (long long)t0 * q.tStride * (q.precision / 8);
        jb.cStride = q.cStride;
        jb.tStride = q.tStride;
        jb.out = first + (size_t)i * (size_t)stride;
        jb.row0 = total;
        jb.n = q.n - t0;
        jb.tiles = (int)(padded_samples(jb.n) / 16);
        jb.precision = q.precision;
        jb.k0 = t0;
        jb.uid = q.uid;
        jb.temp = temperature_word(q.temperature);
        jb.yInPrev = jb.yInCur = 128;
        jb.yBefore = t0 > 0 ? 2 : 0;
        total += padded_samples(jb.n);
        if (jb.tiles > maxTiles) maxTiles = jb.tiles;
    }
    const TimeScratch sc = time_carve(m_scratch.atLeast((size_t)total * time_scratch_bytes(m.f16, m.R, 0)), (size_t)total, m);
    const TimeJob* const dev = m_jobs.send(jobs, count, stream);

    bool ok = false;
#define WN_PREFILL_CASE(RR)                                                                                                    \
    case RR:                                                                                                                   \
        ok = m.f16 ? time_launch<true, RR, 0, false>(m, dev, count, maxTiles, true, sc, stream)                                \
                   : time_launch<false, RR, 0, false>(m, dev, count, maxTiles, true, sc, stream);                              \
        break;
    switch (m.R) {
        WN_PREFILL_CASE(32)
        WN_PREFILL_CASE(64)
        WN_PREFILL_CASE(128)
        WN_PREFILL_CASE(256)
    }
#undef WN_PREFILL_CASE
    return ok;
}

}  // namespace wn
