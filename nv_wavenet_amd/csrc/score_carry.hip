// score_carry.hip -- the host side of scoring with carried state (score_carry.hpp), Score::chunksCheck and Score::runChunks, and
// scoring's instantiations of the time-parallel pass, for the whole pass too: the skip path and the states, the (R, S) of the built
// shapes, both precisions.  The head is score.hip's.
#include "score_carry.hpp"

#include <limits.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "time_kernels.hpp"

namespace wn {

namespace {

// the device-side address of `bytes` of device or mapped pinned memory at p, 16-byte aligned; NULL for anything else
char* blobTarget(const void* p, size_t bytes, bool* pinned) {
    if (p == NULL || ((size_t)p & 15) != 0) return NULL;
    const int type = pointer_type(p);
    if (type != hipMemoryTypeDevice && type != hipMemoryTypeManaged && type != hipMemoryTypeHost) return NULL;
    *pinned = type == hipMemoryTypeHost;
    char* const first = (char*)store_target((void*)p);
    if (first == NULL || (char*)store_target((char*)p + bytes - 16) != first + bytes - 16) return NULL;
    return first;
}

bool headerFits(const TimeModel& m, const SlotStateHeader& h) {
    float T, P, Q;      // (word 10: zero, or the bits of a valid temperature; word 11: zero, or the bits of a valid probability floor;
    int K;              // word 12: top-k within the alphabet; word 13: zero, or the bits of a valid top-p -- checked, then ignored)
    return h.magic == kSlotStateMagic && h.version == kSlotStateVersion && h.precision == (m.f16 ? 16 : 32) && h.R == m.R &&
           h.numLayers == m.numLayers && h.maxDilation == m.maxDilation && h.done >= 0 && temperature_of_word(h.pad[0], T) &&
           min_p_of_word(h.pad[1], P) && top_k_of_word(h.pad[2], m.A, K) && top_p_of_word(h.pad[3], Q);
}

}  // namespace

bool Score::chunksCheck(const TimeModel& m, const ScoreChunkReq* reqs, int count, bool ownX, std::vector<ScoreChunkIn>& in) {
    if (!time_call_ok(m, reqs, count)) return false;
    // everything the whole pass refuses
    {
        std::vector<ScoreReq> plain(count);
        for (int i = 0; i < count; i++) {
            const ScoreChunkReq& q = reqs[i];
            plain[i] = ScoreReq{q.y, q.n, q.x, q.precision, q.cStride, q.tStride, q.temperature, q.logp, q.rows};
        }
        if (!acceptable(m, plain.data(), count, ownX)) return false;
    }
    const size_t bytes = time_blob_bytes(m);
    in.assign(count, ScoreChunkIn{NULL, NULL, 0, 0u, 128, 128});
    // the blobs' ranges: every out-state clear of every in-state and of every other out-state (equal lengths: neighbours by address)
    std::vector<std::pair<size_t, int>> spans;      // (device-side address, 1: out-state)
    std::vector<const void*> devStates;             // distinct in-states in device memory, in order of appearance
    std::vector<std::pair<const void*, SlotStateHeader>> seen;      // every distinct in-state once
    std::unordered_map<const void*, size_t> index;
    for (int i = 0; i < count; i++) {
        const ScoreChunkReq& q = reqs[i];
        if (q.state != NULL) {
            bool pinned = false;
            in[i].in = blobTarget(q.state, bytes, &pinned);
            if (in[i].in == NULL) return false;
            if (index.find(q.state) == index.end()) {
                index[q.state] = seen.size();
                SlotStateHeader h = {};
                if (pinned) memcpy(&h, q.state, sizeof(h));
                else devStates.push_back(q.state);
                seen.push_back(std::make_pair(q.state, h));
                spans.push_back(std::make_pair((size_t)in[i].in, 0));
            }
        }
        if (q.stateOut != NULL) {
            bool pinned = false;
            in[i].out = blobTarget(q.stateOut, bytes, &pinned);
            if (in[i].out == NULL) return false;
            spans.push_back(std::make_pair((size_t)in[i].out, 1));
        }
    }
    std::sort(spans.begin(), spans.end());
    for (size_t s = 1; s < spans.size(); s++)
        if (spans[s].first - spans[s - 1].first < bytes && (spans[s].second || spans[s - 1].second)) return false;
    // the headers of the device blobs: blocking copies on the null stream (a save on a non-blocking stream must have been ordered
    // before this call, as for nvw_slot_resume); an arithmetic progression inside one allocation -- the rows of one earlier call --
    // takes one 2-D copy
    if (!devStates.empty()) {
        const size_t nd = devStates.size();
        std::vector<SlotStateHeader> hdr(nd);
        bool rows = nd >= 2 && (const char*)devStates[1] > (const char*)devStates[0];
        const size_t step = rows ? (size_t)((const char*)devStates[1] - (const char*)devStates[0]) : 0;
        for (size_t s = 2; s < nd && rows; s++) rows = (const char*)devStates[s] == (const char*)devStates[0] + s * step;
        if (rows) {
            void* base = NULL;
            size_t size = 0;
            if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)devStates[0]) != hipSuccess) {
                (void)hipGetLastError();
                rows = false;
            } else {
                rows = (const char*)devStates[nd - 1] + bytes <= (const char*)base + size;
            }
        }
        if (rows) {
            gpuErrChk(hipMemcpy2D(hdr.data(), sizeof(SlotStateHeader), devStates[0], step, sizeof(SlotStateHeader), nd, hipMemcpyDeviceToHost));
        } else {
            for (size_t s = 0; s < nd; s++) gpuErrChk(hipMemcpy(&hdr[s], devStates[s], sizeof(SlotStateHeader), hipMemcpyDeviceToHost));
        }
        size_t at = 0;
        for (size_t s = 0; s < seen.size() && at < nd; s++)
            if (seen[s].first == devStates[at]) seen[s].second = hdr[at++];
    }
    for (size_t s = 0; s < seen.size(); s++)
        if (!headerFits(m, seen[s].second)) return false;
    for (int i = 0; i < count; i++) {
        const ScoreChunkReq& q = reqs[i];
        in[i].uid = q.uid;
        if (q.state == NULL) continue;
        const SlotStateHeader& h = seen[index[q.state]].second;
        if ((long long)h.done + q.n > (long long)INT_MAX - 16) return false;
        in[i].k0 = h.done;
        in[i].uid = h.uid;
        in[i].yInPrev = h.yInPrev;
        in[i].yInCur = h.yInCur;
    }
    return true;
}

bool Score::launchLayers(const TimeModel& m, const TimeJob* jobs, int count, int maxTiles, bool anyOut, const TimeScratch& sc, hipStream_t stream) {
    bool ok = false;
#define WN_SCORE_LAYERS(RR, SS, AA)                                                                                            \
    if (m.R == RR && m.S == SS && m.A == AA)                                                                                   \
        ok = m.f16 ? time_launch<true, RR, SS, true>(m, jobs, count, maxTiles, anyOut, sc, stream)                             \
                   : time_launch<false, RR, SS, true>(m, jobs, count, maxTiles, anyOut, sc, stream);
    WN_SCORE_SHAPES(WN_SCORE_LAYERS)
#undef WN_SCORE_LAYERS
    return ok;
}

bool Score::runChunks(const TimeModel& m, const ScoreChunkReq* reqs, int count, const std::vector<ScoreChunkIn>& in, hipStream_t stream) {
    if (reqs == NULL || count < 1 || (int)in.size() != count) return false;
    TimeJob* const jobs = m_jobs.begin(count);
    int maxTiles = 0;
    bool anyOut = false;
    long long total = 0;
    for (int i = 0; i < count; i++) {
        const ScoreChunkReq& q = reqs[i];
        TimeJob& jb = jobs[i];
        jb.y = q.y;
        jb.x = q.x;
        jb.cStride = q.cStride;
        jb.tStride = q.tStride;
        jb.in = in[i].in;
        jb.out = in[i].out;
        jb.logp = (float*)store_target(q.logp);
        jb.rows = q.rows;
        jb.row0 = total;
        jb.n = q.n;
        jb.tiles = (int)(padded_samples(q.n) / 16);
        jb.precision = q.precision;
        jb.k0 = in[i].k0;
        jb.uid = in[i].uid;
        jb.temp = temperature_word(q.temperature);
        jb.yInPrev = in[i].yInPrev;
        jb.yInCur = in[i].yInCur;
        jb.scale = temperature_scale(q.temperature);
        total += padded_samples(q.n);
        if (jb.tiles > maxTiles) maxTiles = jb.tiles;
        anyOut = anyOut || jb.out != NULL;
    }
    const TimeScratch sc = time_carve(m_scratch.atLeast((size_t)total * time_scratch_bytes(m.f16, m.R, m.S)), (size_t)total, m);
    const TimeJob* const dev = m_jobs.send(jobs, count, stream);

    return launchLayers(m, dev, count, maxTiles, anyOut, sc, stream) && score_launch_head(m, dev, count, maxTiles, sc.skf, stream);
}

}  // namespace wn
