// slots_session.hip -- wn::SlotSession and wn::StageRing (slots_session.hpp): the host half of slot mode.  Compiled once.
#include "slots_session.hpp"

namespace wn {

namespace {
template <class T> void allocZero(T*& p, size_t bytes) {
    gpuErrChk(hipMalloc((void**)&p, bytes));
    gpuErrChk(hipMemset(p, 0, bytes));
}
template <class... T> void freeDev(T*&... p) {
    for (void* q : {(void*)p...})
        if (q) gpuErrChk(hipFree(q));
    ((p = NULL), ...);
}
// The address the device stores through for an output of slotsStepRagged: the pointer itself for device memory, the mapped
// address for pinned host memory (hipHostMalloc, hipHostRegister); NULL for anything else (pageable host memory).
void* deliverTarget(void* p, bool* pinned = NULL) {
    const int type = pointer_type(p);
    if (pinned && type >= 0) *pinned = type == hipMemoryTypeHost;
    if (type == hipMemoryTypeDevice || type == hipMemoryTypeManaged) return p;
    if (type != hipMemoryTypeHost) return NULL;
    void* d = NULL;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
        (void)hipGetLastError();
        return NULL;
    }
    return d;
}
// the fields of a blob's header that every blob of an engine shares
SlotStateHeader headerCommon(const SlotFacts& f) {
    SlotStateHeader h = {};
    h.magic = kSlotStateMagic;
    h.version = kSlotStateVersion;
    h.precision = f.f16 ? 16 : 32;
    h.R = f.R;
    h.numLayers = f.numLayers;
    h.maxDilation = f.maxDilation;
    return h;
}
bool headerOk(const SlotFacts& f, const SlotStateHeader& h) {
    Sampling s;      // (word 10: zero, or the bits of a valid temperature; word 11: zero, or the bits of a valid floor; word 12: top-k,
                     // within the alphabet; word 13: zero, or the bits of a valid top-p)
    return h.magic == kSlotStateMagic && h.version == kSlotStateVersion && h.precision == (f.f16 ? 16 : 32) && h.R == f.R &&
           h.numLayers == f.numLayers && h.maxDilation == f.maxDilation && h.done >= 0 && sampling_of_words(h.pad, f.A, s);
}
}  // namespace

// ---- StageRing ----
void StageRing::make(int n, size_t bytes) {
    reset();
    m_buf.assign(n, NULL);
    m_ev.assign(n, NULL);
    for (int i = 0; i < n; i++) {
        gpuErrChk(hipHostMalloc(&m_buf[i], bytes, hipHostMallocDefault));
        gpuErrChk(hipEventCreateWithFlags(&m_ev[i], hipEventDisableTiming));
    }
}
void StageRing::reset() {
    for (size_t i = 0; i < m_buf.size(); i++) {
        gpuErrChk(hipHostFree(m_buf[i]));
        gpuErrChk(hipEventDestroy(m_ev[i]));
    }
    m_buf.clear();
    m_ev.clear();
    m_uses = 0;
}
void* StageRing::acquire() {
    const int i = at();
    if (m_uses >= m_buf.size()) gpuErrChk(hipEventSynchronize(m_ev[i]));
    return m_buf[i];
}
void StageRing::release(hipStream_t stream) {
    gpuErrChk(hipEventRecord(m_ev[at()], stream));
    m_uses++;
}

// ---- SlotSession ----
SlotSession::SlotSession(const SlotFacts& facts, SlotHost& host, SamplingTable& temps) : f(facts), m_host(host), m_temps(temps) {
    for (int l = 0, d = 1; l < f.numLayers; l++) {
        if (d > m_largestD) m_largestD = d;
        d <<= 1;
        if (d > f.maxDilation) d = 1;
    }
}
SlotSession::~SlotSession() {
    end();
    freeDev(m_slotLayers);
}
bool SlotSession::begin(int window) {
    if (!f.supported || m_host.slotLive().nCond <= 0 || window <= 0 || window % largestDilation() != 0) return false;
    end();
    m_slotW = window;
    m_slotCounter = 0;
    m_slotHost.assign(f.maxBatch, SlotDesc{});
    m_slotPending.assign(f.maxBatch, 0);
    m_melHost.assign(f.maxBatch, MelDesc{});
    m_melDirty.assign(f.maxBatch, 0);
    m_slotResume.assign(f.maxBatch, NULL);
    m_slotResumeDone.assign(f.maxBatch, 0);
    m_slotMoveEnd.assign(f.maxBatch, 0);
    m_temps.reset(false);      // (every column at T = 1, floor 0 and no cut, a lockstep run's values included)
    m_primeY.clear();
    m_primeN.clear();
    m_primeListed.clear();
    m_primeList.clear();
    const size_t cells = (size_t)window * f.maxBatch;
    allocZero(m_slotDesc, (size_t)f.maxBatch * sizeof(SlotDesc));
    allocZero(m_slotFeat, featBytes(window));
    allocZero(m_slotSel, cells * sizeof(float));
    allocZero(m_slotY, cells * sizeof(int));
    allocZero(m_slotPcm, cells * sizeof(short));
    gpuErrChk(hipMalloc((void**)&m_slotUpd, slotUpdBytes()));
    m_slotStage.make(2, slotUpdBytes());
    gpuErrChk(hipMalloc((void**)&m_dlvDev, (size_t)f.maxBatch * sizeof(DeliverPiece)));
    m_dlv.make(kSlotTickets, (size_t)f.maxBatch * sizeof(DeliverPiece));
    m_mulaw = m_host.slotMulaw();
    gpuErrChk(hipDeviceSynchronize());
    return true;
}
bool SlotSession::start(int slot, const void* x, int precision, long long cStride, long long tStride, int length, unsigned uid) {
    if (!slotStartOk(slot, x, precision, cStride, tStride, length)) return false;
    slotDropMel(slot);
    slotDropResume(slot);
    SlotDesc& d = m_slotHost[slot];
    d.x = x;
    d.cStride = cStride;
    d.tStride = tStride;
    d.start = 0;          // (the step that applies the start sets it)
    d.length = length;
    d.uid = uid;
    d.precision = precision;
    d.active = 1;
    slotMarkPending(slot, 1);
    slotSamplingSet(slot, Sampling{});
    slotPrimeSet(slot, NULL, 0);
    return true;
}
bool SlotSession::stop(int slot) {
    if (!inBatch(slot)) return false;
    slotDropMel(slot);
    slotDropResume(slot);
    m_slotHost[slot].active = 0;
    slotMarkPending(slot, 2);
    slotPrimeSet(slot, NULL, 0);
    slotSamplingSet(slot, Sampling{});      // (an idle column holds no value: the launches go back to Params::floorOn = 0 with the last floored or cutting utterance)
    return true;
}
bool SlotSession::startMel(int slot, const void* mel, int precision, long long cStride, long long fStride, int frames, int final, unsigned uid) {
    if (!slotStartMelOk(slot, mel, precision, cStride, fStride, frames, final, m_host.slotLive().upStride)) return false;
    if (!m_melDesc) melAllocate();
    slotDropResume(slot);
    MelDesc& d = m_melHost[slot];
    if (!d.state) m_melColumns++;
    d.mel = mel;
    d.cStride = cStride;
    d.fStride = fStride;
    d.start = 0;          // (the step that applies the start sets it)
    d.frames = frames;
    d.uid = uid;
    d.precision = precision;
    d.state = final ? 2 : 1;
    melMarkDirty(slot);
    m_melTilesDirty = true;
    m_slotHost[slot].active = 0;      // (its SlotDesc goes idle: the feed writes zeros into its lanes, the mel feed overwrites them)
    slotMarkPending(slot, 1);
    slotSamplingSet(slot, Sampling{});
    slotPrimeSet(slot, NULL, 0);
    return true;
}
bool SlotSession::melFrames(int slot, int frames, int final) {
    if (!inBatch(slot)) return false;
    MelDesc& d = m_melHost[slot];
    if (d.state != 1 || frames < d.frames || (final && frames == 0) || (long long)frames * m_host.slotLive().upStride > 0x7fffffffLL) return false;
    d.frames = frames;
    if (final) d.state = 2;
    melMarkDirty(slot);
    return true;
}
bool SlotSession::setTemperature(int slot, float T) {
    Sampling s = m_temps.get(slot);
    s.temperature = T;
    return slotSamplingChange(slot, s);
}
bool SlotSession::setMinP(int slot, float p) {
    Sampling s = m_temps.get(slot);
    s.minP = p;
    return slotSamplingChange(slot, s);
}
bool SlotSession::setTopK(int slot, int k) {
    Sampling s = m_temps.get(slot);
    s.topK = k;
    return slotSamplingChange(slot, s);
}
bool SlotSession::setTopP(int slot, float p) {
    Sampling s = m_temps.get(slot);
    s.topP = p;
    return slotSamplingChange(slot, s);
}
bool SlotSession::prime(int slot, const int* y, int n) {
    if (!inBatch(slot) || m_slotPending[slot] != 1 || y == NULL || n < 1 || !is_device_ptr(y)) return false;
    const MelDesc& m = m_melHost[slot];
    if (m.state == 2 && n > (long long)m.frames * m_host.slotLive().upStride) return false;
    if (m.state == 0 && n > m_slotHost[slot].length) return false;
    slotPrimeSet(slot, y, n);
    return true;
}
bool SlotSession::move(int from, int to) {
    if (!inBatch(from) || !inBatch(to) || from == to) return false;
    if (!slotHolds(from) || m_slotPending[from] == 1 || m_slotMoveEnd[from]) return false;
    if (slotHolds(to) || m_slotPending[to] == 1 || m_slotMoveEnd[to]) return false;
    m_slotHost[to] = m_slotHost[from];
    m_slotHost[from].active = 0;
    if (m_melHost[from].state) {
        m_melHost[to] = m_melHost[from];
        m_melHost[from].state = 0;
        if (m_melDirty[from]) melMarkDirty(to);      // (frames announced since the last step: the update path writes them after the move)
        m_melTilesDirty = true;
    }
    m_slotMoveEnd[from] = 1;
    m_slotMoveEnd[to] = 2;
    m_slotMoves.push_back(SlotMove{from, to});
    slotSamplingSet(to, m_temps.get(from));
    slotSamplingSet(from, Sampling{});      // (as stop())
    if (primed(from)) {
        slotPrimeSet(to, m_primeY[from], m_primeN[from]);
        slotPrimeSet(from, NULL, 0);
    }
    return true;
}
int SlotSession::save(int slot, void* dst, hipStream_t stream) {
    if (!inBatch(slot) || !slotHolds(slot) || m_slotPending[slot] == 1 || m_slotMoveEnd[slot] ||
        dst == NULL || ((size_t)dst & 15) != 0 || !is_device_ptr(dst))
        return -1;
    const bool mel = m_melHost[slot].state != 0;
    const long long start = mel ? m_melHost[slot].start : m_slotHost[slot].start, done = m_slotCounter - start;
    if (done < 0 || done > 0x7fffffffLL) return -1;
    SlotStateHeader h = headerCommon(f);
    h.done = (int)done;
    h.uid = mel ? m_melHost[slot].uid : m_slotHost[slot].uid;
    sampling_words(m_temps.get(slot), h.pad);
    if (!slots_save(stream, dst, h, slot, slotRotation(start), slotLayers(), f.ring, f.ringSlots, f.ringFragsPerSlot, f.yInPrev, f.yInCur))
        return -1;
    return (int)done;
}
bool SlotSession::resume(int slot, const void* state, const void* x, int precision, long long cStride, long long tStride, int length) {
    SlotStateHeader h;
    if (m_slotW <= 0 || !slotStateHeader(state, h) || h.done >= length) return false;
    if (!start(slot, x, precision, cStride, tStride, length, h.uid)) return false;
    slotSetResume(slot, state, h);
    return true;
}
bool SlotSession::resumeMel(int slot, const void* state, const void* mel, int precision, long long cStride, long long fStride, int frames, int final) {
    SlotStateHeader h;
    if (m_slotW <= 0) return false;
    const int upStride = m_host.slotLive().upStride;
    if (upStride <= 0 || !slotStateHeader(state, h) || (final && h.done >= (long long)frames * upStride)) return false;
    if (!startMel(slot, mel, precision, cStride, fStride, frames, final, h.uid)) return false;
    slotSetResume(slot, state, h);
    return true;
}
int SlotSession::saveList(const int* slots, int n, void* dst, long long stride, SlotSaved* saved, hipStream_t stream) {
    if (m_slotW <= 0 || slots == NULL || saved == NULL || n < 1 || n > f.maxBatch) return -1;
    bool pinned = false;
    char* const out = (char*)slotBlobRange(dst, n, stride, &pinned);
    if (out == NULL) return -1;
    m_listMark.assign(f.maxBatch, 0);
    for (int i = 0; i < n; i++) {
        const int b = slots[i];
        if (b < 0 || b >= f.maxBatch || m_listMark[b] || !slotHolds(b) || m_slotPending[b] == 1 || m_slotMoveEnd[b]) return -1;
        m_listMark[b] = i + 1;
        const bool mel = m_melHost[b].state != 0;
        const long long done = m_slotCounter - (mel ? m_melHost[b].start : m_slotHost[b].start);
        if (done < 0 || done > 0x7fffffffLL) return -1;
    }
    // (a half of the staging and of the device buffer: maxBatch entries, then their maxBatch pairs of cut words)
    const size_t saveHalf = (size_t)f.maxBatch * (sizeof(SlotSave) + sizeof(SlotSaveCut));
    if (!m_saveDev) {
        gpuErrChk(hipMalloc((void**)&m_saveDev, 2 * saveHalf));
        m_saveStage.make(2, saveHalf);
    }
    const SlotLayer* const layers = slotLayers();
    SlotSave* const dev = (SlotSave*)((char*)m_saveDev + (size_t)m_saveStage.at() * saveHalf);
    SlotSave* const stage = (SlotSave*)m_saveStage.acquire();
    SlotSaveCut* const cutStage = (SlotSaveCut*)(stage + f.maxBatch);
    bool anyCut = false;
    for (int i = 0; i < n; i++) {
        const int b = slots[i];
        const bool mel = m_melHost[b].state != 0;
        const long long start = mel ? m_melHost[b].start : m_slotHost[b].start;
        const unsigned uid = mel ? m_melHost[b].uid : m_slotHost[b].uid;
        const int done = (int)(m_slotCounter - start);
        int w[kSamplingKinds];
        sampling_words(m_temps.get(b), w);
        stage[i] = SlotSave{out + (size_t)i * (size_t)stride, b, slotRotation(start), done, uid, w[kTemperature], w[kMinP]};
        cutStage[i] = SlotSaveCut{w[kTopK], w[kTopP]};
        anyCut = anyCut || cutStage[i].x != 0 || cutStage[i].y != 0;
        saved[i] = SlotSaved{b, uid, done, mel ? 1 : 0};
    }
    gpuErrChk(hipMemcpyAsync(dev, stage, (size_t)n * sizeof(SlotSave), hipMemcpyHostToDevice, stream));
    SlotSaveCut* const cutDev = (SlotSaveCut*)(dev + f.maxBatch);
    if (anyCut) gpuErrChk(hipMemcpyAsync(cutDev, cutStage, (size_t)n * sizeof(SlotSaveCut), hipMemcpyHostToDevice, stream));
    const bool ok = slots_save_list(stream, dev, anyCut ? cutDev : NULL, n, headerCommon(f), layers, f.ring, f.ringSlots, f.ringFragsPerSlot, f.yInPrev, f.yInCur);
    m_saveStage.release(stream);
    return ok ? n : -1;
}
int SlotSession::resumeList(const SlotResumeReq* reqs, int n, const void* states, long long stride) {
    if (m_slotW <= 0 || reqs == NULL || n < 1 || n > f.maxBatch) return 0;
    bool pinned = false;
    const char* const dev = (const char*)slotBlobRange(states, n, stride, &pinned);
    if (dev == NULL) return 0;
    std::vector<SlotStateHeader> hdr(n);
    if (pinned)
        for (int i = 0; i < n; i++) memcpy(&hdr[i], (const char*)states + (size_t)i * (size_t)stride, sizeof(SlotStateHeader));
    else
        gpuErrChk(hipMemcpy2D(hdr.data(), sizeof(SlotStateHeader), states, (size_t)stride, sizeof(SlotStateHeader), n, hipMemcpyDeviceToHost));
    const int upStride = m_host.slotLive().upStride;
    m_listMark.assign(f.maxBatch, 0);
    for (int i = 0; i < n; i++) {
        const SlotResumeReq& q = reqs[i];
        const SlotStateHeader& h = hdr[i];
        if (!headerOk(f, h)) return 0;
        if (q.mel ? !slotStartMelOk(q.slot, q.src, q.precision, q.cStride, q.tStride, q.length, q.final, upStride)
                  : !slotStartOk(q.slot, q.src, q.precision, q.cStride, q.tStride, q.length))
            return 0;
        if (q.mel ? (q.final && h.done >= (long long)q.length * upStride) : h.done >= q.length) return 0;
        if (m_listMark[q.slot] || slotHolds(q.slot) || m_slotPending[q.slot] == 1) return 0;
        m_listMark[q.slot] = i + 1;
    }
    for (int i = 0; i < n; i++) {
        const SlotResumeReq& q = reqs[i];
        const bool ok = q.mel ? startMel(q.slot, q.src, q.precision, q.cStride, q.tStride, q.length, q.final, hdr[i].uid)
                              : start(q.slot, q.src, q.precision, q.cStride, q.tStride, q.length, hdr[i].uid);
        assert(ok);
        (void)ok;
        slotSetResume(q.slot, dev + (size_t)i * (size_t)stride, hdr[i]);
    }
    return n;
}
int SlotSession::headroom() const {
    if (m_slotW <= 0) return 0;
    long long h = m_slotW;
    if (m_melColumns > 0) {
        const int upStride = m_host.slotLive().upStride;
        for (int b = 0; b < f.maxBatch; b++) {
            const MelDesc& d = m_melHost[b];
            if (d.state != 1) continue;
            const long long next = m_slotPending[b] == 1 ? m_slotResumeDone[b] : m_slotCounter - d.start;      // (a resumed column goes on from done)
            const long long left = (long long)d.frames * upStride - next;
            if (left < h) h = left;
        }
    }
    return h < 0 ? 0 : (int)h;
}
bool SlotSession::getFeatures(void* dst, long long first, int count) {
    if (m_slotW <= 0 || dst == NULL || count <= 0 || first < m_slotCounter - m_slotW || first < 0 || first + count > m_slotCounter)
        return false;
    gpuErrChk(hipDeviceSynchronize());
    for (int done = 0, row, c; done < count; done += c) {
        c = rowsFrom(first + done, count - done, row);
        gpuErrChk(hipMemcpy((char*)dst + featBytes(done), m_slotFeat + featBytes(row), featBytes(c), hipMemcpyDefault));
    }
    return true;
}
bool SlotSession::step(int count, int* yOut, short* pcm, hipStream_t stream) {
    if (m_slotW <= 0 || count <= 0 || count > m_slotW) return false;
    if (m_melColumns > 0 && (m_host.slotLive().upStride <= 0 || count > headroom())) return false;      // (mel columns short of frames)
    const int T = (int)(m_slotCounter % m_slotW);
    int cols = 0;
    bool ok = generate(count, cols, stream);
    for (int done = 0, t0, c; cols > 0 && pcm != NULL && done < count; done += c) {
        c = rowsFrom(T + done, count - done, t0);
        ok = slots_pcm(stream, m_slotY, m_slotPcm, m_mulaw, cols, m_slotW, t0, c) && ok;
    }
    for (int done = 0, t0, c; done < count; done += c) {
        c = rowsFrom(T + done, count - done, t0);
        copyRows(t0, c, done, count, yOut, pcm, stream);
    }
    m_slotCounter += count;
    if ((yOut != NULL && !is_device_ptr(yOut)) || (pcm != NULL && !is_device_ptr(pcm))) gpuErrChk(hipStreamSynchronize(stream));
    return ok;
}
// window rows [t0, t0 + c) of every column into columns [done, done + c) of yOut / pcm ([maxBatch][count]; NULL: none)
void SlotSession::copyRows(int t0, int c, int done, int count, int* yOut, short* pcm, hipStream_t stream) {
    const size_t W = m_slotW;
    if (yOut != NULL)
        gpuErrChk(hipMemcpy2DAsync(yOut + done, (size_t)count * sizeof(int), m_slotY + t0, W * sizeof(int), (size_t)c * sizeof(int), f.maxBatch,
                                   hipMemcpyDefault, stream));
    if (pcm != NULL)
        gpuErrChk(hipMemcpy2DAsync(pcm + done, (size_t)count * sizeof(short), m_slotPcm + t0, W * sizeof(short), (size_t)c * sizeof(short),
                                   f.maxBatch, hipMemcpyDefault, stream));
}
bool SlotSession::generate(int count, int& cols, hipStream_t stream) {
    const int W = m_slotW;
    bool ok = true;
    if (!m_slotMoves.empty()) ok = slotApplyMoves(stream);
    if (!m_melDirtyList.empty() || m_melTilesDirty) ok = melApplyPending(stream) && ok;      // (before the starts: it reads the pending ones)
    if (!m_slotPendingList.empty()) ok = slotApplyPending(stream) && ok;
    if (!m_tempDirtyList.empty()) ok = slotApplyTemperatures(stream) && ok;      // (the host's values: whatever moved or started above)
    cols = 0;
    for (int b = f.maxBatch - 1; b >= 0; b--)
        if (m_slotHost[b].active || (m_melColumns > 0 && m_melHost[b].state)) {
            cols = b + 1;
            break;
        }
    const int T = (int)(m_slotCounter % W);
    if (cols > 0) {
        const SlotLive v = m_host.slotLive();
        m_host.slotFeatStreamReady(stream);
        ok = (f.f16 ? slots_feed<true> : slots_feed<false>)(stream, m_slotFeat, m_slotSel, m_slotDesc, cols, f.maxBatch, f.tiles, v.nCond,
                                                           m_slotCounter, T, W, count, v.seed) && ok;
        if (m_melTiles > 0) {
            char* const stage = melStage(count, v);
            ok = (f.f16 ? slots_mel_feed<true> : slots_mel_feed<false>)(stream, m_slotFeat, m_slotSel, stage, stage + m_melRecOff, m_melColInfo,
                                                                       m_melDesc, (const int*)(m_melUpd + melTileOff()), m_melTiles, f.maxBatch,
                                                                       f.tiles, v.nCond, v.upTab, v.upBias, v.upWindow / v.upStride, v.upStride,
                                                                       m_slotCounter, T, W, count, v.seed) && ok;
        }
        bool forced = false;
        if (!m_primeList.empty()) ok = slotApplyPrimes(count, forced, stream) && ok;      // (behind the feeds: it replaces their draws)
        for (int done = 0, t0, c; done < count; done += c) {      // (two launches where the window rows wrap)
            c = rowsFrom(T + done, count - done, t0);
            ok = m_host.slotGenerate(m_slotFeat, m_slotSel, m_slotY, W, t0, c, cols, forced, stream) && ok;
        }
    }
    return ok;
}
// The pieces a step of `count` samples delivers, from what the host knows (the descriptors with the pending starts, resumes and
// moves already in them, the counter): one per column holding an utterance with a sample in this step, ascending.  first = the
// local index of its first sample; n = min(count, length - first) for a feature column and a final mel column, count for a
// non-final mel column (the headroom rule); offsets packed, each rounded up to kDeliverAlign elements.  out may be NULL (count
// only).  Returns the number of pieces; total = the end of the last one.
int SlotSession::slotPieces(int count, SlotPiece* out, int maxOut, long long& total, int upStride) const {
    int n = 0;
    long long off = 0;
    total = 0;
    for (int b = 0; b < f.maxBatch; b++) {
        const bool mel = m_melColumns > 0 && m_melHost[b].state != 0;
        if (!mel && !m_slotHost[b].active) continue;
        const long long start = mel ? m_melHost[b].start : m_slotHost[b].start;
        const long long first = m_slotPending[b] == 1 ? m_slotResumeDone[b] : m_slotCounter - start;
        long long len = count, left = count;
        bool bounded = true;
        if (!mel) len = m_slotHost[b].length;
        else if (m_melHost[b].state == 2) len = (long long)m_melHost[b].frames * upStride;
        else bounded = false;
        if (bounded) left = len - first;
        if (left <= 0) continue;      // (ended in an earlier step and not stopped since)
        const int k = left < count ? (int)left : count;
        if (out != NULL && n < maxOut) {
            SlotPiece& p = out[n];
            p.slot = b;
            p.uid = mel ? m_melHost[b].uid : m_slotHost[b].uid;
            p.first = first;
            p.n = k;
            p.finished = bounded && first + k == len ? 1 : 0;
            p.offset = off;
        }
        n++;
        total = off + k;
        off = (total + kDeliverAlign - 1) / kDeliverAlign * kDeliverAlign;
    }
    return n;
}
long long SlotSession::stepRagged(int count, int* samples, short* pcm, long long capacity, SlotPiece* pieces, int maxPieces, int* nPieces,
                                  unsigned long long* ticket, hipStream_t stream) {
    if (m_slotW <= 0 || count <= 0 || count > m_slotW || (samples == NULL && pcm == NULL) || pieces == NULL || nPieces == NULL ||
        ticket == NULL)
        return -1;
    const int upStride = m_host.slotLive().upStride;
    if (m_melColumns > 0 && (upStride <= 0 || count > headroom())) return -1;
    int* const dSamples = samples ? (int*)deliverTarget(samples) : NULL;
    short* const dPcm = pcm ? (short*)deliverTarget(pcm) : NULL;
    if ((samples && !dSamples) || (pcm && !dPcm)) return -1;
    long long total = 0;
    const int n = slotPieces(count, NULL, 0, total, upStride);
    if (n > maxPieces || total > capacity) return -1;
    slotPieces(count, pieces, maxPieces, total, upStride);
    *nPieces = n;
    const int T = (int)(m_slotCounter % m_slotW);
    DeliverPiece* const stage = (DeliverPiece*)m_dlv.acquire();
    int cols = 0;
    bool ok = generate(count, cols, stream);
    if (n > 0) {
        for (int i = 0; i < n; i++) stage[i] = DeliverPiece{pieces[i].slot, pieces[i].n, pieces[i].offset};
        gpuErrChk(hipMemcpyAsync(m_dlvDev, stage, (size_t)n * sizeof(DeliverPiece), hipMemcpyHostToDevice, stream));
        ok = slots_deliver(stream, m_slotY, m_mulaw, T, m_slotW, count, m_dlvDev, n, dSamples, dPcm) && ok;
    }
    m_dlv.release(stream);
    m_slotCounter += count;
    *ticket = m_dlv.uses();
    return ok ? total : -2;
}
float SlotSession::timeOutputs(bool ragged, int count, int* samples, short* pcm, long long capacity, int reps, hipStream_t stream) {
    if (m_slotW <= 0 || count <= 0 || count > m_slotW || count > m_slotCounter || samples == NULL || pcm == NULL || reps <= 0) return -1.f;
    int* const dSamples = (int*)deliverTarget(samples);
    short* const dPcm = (short*)deliverTarget(pcm);
    if (!dSamples || !dPcm) return -1.f;
    const int W = m_slotW, T = (int)((m_slotCounter - count) % W);
    gpuErrChk(hipDeviceSynchronize());
    DeliverPiece* const stage = (DeliverPiece*)m_dlv.buffer(0);
    int n = 0, cols = 0;
    long long off = 0, total = 0;
    for (int b = 0; b < f.maxBatch; b++) {
        const bool mel = m_melColumns > 0 && m_melHost[b].state != 0;
        if ((!mel && !m_slotHost[b].active) || m_slotPending[b] == 1) continue;
        cols = b + 1;
        const long long done = m_slotCounter - (mel ? m_melHost[b].start : m_slotHost[b].start);
        if (done <= 0) continue;
        const int k = done < count ? (int)done : count;
        stage[n++] = DeliverPiece{b, k, off};
        total = off + k;
        off = (total + kDeliverAlign - 1) / kDeliverAlign * kDeliverAlign;
    }
    if (n == 0 || (ragged ? total : (long long)f.maxBatch * count) > capacity) return -1.f;
    gpuErrChk(hipMemcpyAsync(m_dlvDev, stage, (size_t)n * sizeof(DeliverPiece), hipMemcpyHostToDevice, stream));
    hipEvent_t t0, t1;
    gpuErrChk(hipEventCreate(&t0));
    gpuErrChk(hipEventCreate(&t1));
    bool ok = true;
    gpuErrChk(hipEventRecord(t0, stream));
    for (int r = 0; r < reps; r++) {
        if (ragged) ok = slots_deliver(stream, m_slotY, m_mulaw, T, W, count, m_dlvDev, n, dSamples, dPcm) && ok;
        for (int done = 0, t0, c; !ragged && done < count; done += c) {
            c = rowsFrom(T + done, count - done, t0);
            ok = slots_pcm(stream, m_slotY, m_slotPcm, m_mulaw, cols, W, t0, c) && ok;
            copyRows(t0, c, done, count, samples, pcm, stream);
        }
    }
    gpuErrChk(hipEventRecord(t1, stream));
    gpuErrChk(hipEventSynchronize(t1));
    float ms = 0.f;
    gpuErrChk(hipEventElapsedTime(&ms, t0, t1));
    gpuErrChk(hipEventDestroy(t0));
    gpuErrChk(hipEventDestroy(t1));
    return ok ? ms : -1.f;
}
bool SlotSession::wait(unsigned long long ticket) {
    const int state = done(ticket);
    if (state == 0) gpuErrChk(hipEventSynchronize(m_dlv.event((int)((ticket - 1) % kSlotTickets))));
    return state >= 0;
}
int SlotSession::done(unsigned long long ticket) {
    if (m_slotW <= 0 || ticket == 0 || ticket > m_dlv.uses()) return -1;
    if (m_dlv.uses() - ticket >= (unsigned long long)kSlotTickets) return 1;
    const hipError_t e = hipEventQuery(m_dlv.event((int)((ticket - 1) % kSlotTickets)));
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        return 0;
    }
    gpuErrChk(e);
    return 1;
}
void SlotSession::end() {
    if (m_slotW <= 0) return;
    gpuErrChk(hipDeviceSynchronize());
    freeDev(m_slotDesc, m_slotFeat, m_slotSel, m_slotY, m_slotPcm, m_slotUpd, m_dlvDev, m_saveDev, m_scaleDev, m_primeDev, m_melDesc, m_melUpd,
            m_melColInfo, m_melStage);
    m_melStageBytes = 0;
    m_slotStage.reset();
    m_dlv.reset();
    m_saveStage.reset();
    m_scaleStage.reset();
    m_primeStage.reset();
    m_primeDevN = 0;
    m_primeDirty = false;
    m_primeY.clear();
    m_primeN.clear();
    m_primeListed.clear();
    m_primeList.clear();
    m_melStageHost.reset();
    m_slotW = 0;
    m_slotPendingList.clear();      // (the per-column tables keep their storage: the next begin() fills them afresh)
    m_slotMoves.clear();
    m_temps.reset(!m_tempDirtyList.empty());
    m_tempDirty.clear();
    m_tempDirtyList.clear();
    m_melDirtyList.clear();
    m_melColumns = 0;
    m_melTiles = 0;
    m_melTilesDirty = false;
}
bool SlotSession::slotStartOk(int slot, const void* x, int precision, long long cStride, long long tStride, int length) const {
    return inBatch(slot) && x != NULL && (precision == 32 || precision == 16) && cStride > 0 && tStride > 0 && length > 0 && is_device_ptr(x) &&
           m_slotMoveEnd[slot] != 2;
}
bool SlotSession::slotStartMelOk(int slot, const void* mel, int precision, long long cStride, long long fStride, int frames, int final,
                                 int upStride) const {
    return upStride > 0 && frames >= 0 && !(final && frames == 0) && (long long)frames * upStride <= 0x7fffffffLL &&
           slotStartOk(slot, mel, precision, cStride, fStride, 1);
}
// n blobs of `stride` bytes from `base`: 16-byte aligned device memory (-> base) or mapped pinned host memory (-> its device-side
// address; *pinned set), the last blob in the same range as the first; NULL for anything else or a bad stride
void* SlotSession::slotBlobRange(const void* base, int n, long long stride, bool* pinned) const {
    if (base == NULL || ((size_t)base & 15) != 0 || (stride & 15) != 0 || stride < (long long)stateBytes()) return NULL;
    char* const first = (char*)deliverTarget((void*)base, pinned);
    const size_t span = (size_t)(n - 1) * (size_t)stride;
    if (first == NULL || (char*)deliverTarget((char*)base + span + stateBytes() - 16) != first + span + stateBytes() - 16) return NULL;
    return first;
}
// {first slot, dilation} of its layer for every ring slot, on the device
const SlotLayer* SlotSession::slotLayers() {
    if (!m_slotLayers) {
        std::vector<SlotLayer> tab;
        int d = 1;
        for (int l = 0, off = 0; l < f.numLayers; l++) {
            for (int i = 0; i < d; i++) tab.push_back(make_int2(off, d));
            off += d;
            d <<= 1;
            if (d > f.maxDilation) d = 1;
        }
        assert((int)tab.size() == f.ringSlots);
        gpuErrChk(hipMalloc((void**)&m_slotLayers, tab.size() * sizeof(SlotLayer)));
        gpuErrChk(hipMemcpy(m_slotLayers, tab.data(), tab.size() * sizeof(SlotLayer), hipMemcpyHostToDevice));
    }
    return m_slotLayers;
}
// the header of a blob, read back (blocking) and checked against this engine
bool SlotSession::slotStateHeader(const void* state, SlotStateHeader& h) const {
    if (state == NULL || ((size_t)state & 15) != 0 || !is_device_ptr(state)) return false;
    gpuErrChk(hipMemcpy(&h, state, sizeof(h), hipMemcpyDeviceToHost));
    return headerOk(f, h);
}
// the pending moves -> pinned staging -> device, then one slot_move_kernel launch (staging halves as slotApplyPending)
bool SlotSession::slotApplyMoves(hipStream_t stream) {
    char* const stage = (char*)m_slotStage.acquire();
    SlotMove* const mv = (SlotMove*)(stage + slotMoveOff());
    const int n = (int)m_slotMoves.size();
    for (int i = 0; i < n; i++) {
        mv[i] = m_slotMoves[i];
        m_slotMoveEnd[mv[i].from] = 0;
        m_slotMoveEnd[mv[i].to] = 0;
        slotTouchTile(mv[i].to);
    }
    m_slotMoves.clear();
    gpuErrChk(hipMemcpyAsync(m_slotUpd + slotMoveOff(), mv, (size_t)n * sizeof(SlotMove), hipMemcpyHostToDevice, stream));
    m_slotStage.release(stream);
    return slots_move(stream, (const SlotMove*)(m_slotUpd + slotMoveOff()), n, f.ring, f.ringSlots, f.ringFragsPerSlot, f.yInPrev, f.yInCur,
                      m_slotDesc, m_melDesc);
}
void SlotSession::slotMarkPending(int slot, int what) {
    if (!m_slotPending[slot]) m_slotPendingList.push_back(slot);
    m_slotPending[slot] = what;
}
// the pending starts and stops -> pinned staging -> device, then one slot_reset_kernel launch (ring + history of the started
// columns, every changed descriptor); the staging half is reused two steps later, once its copy has completed
bool SlotSession::slotApplyPending(hipStream_t stream) {
    char* const stage = (char*)m_slotStage.acquire();
    SlotUpdate* const upd = (SlotUpdate*)stage;
    const size_t colOff = slotColOff();
    int* const cols = (int*)(stage + colOff);
    SlotLoad* const loads = (SlotLoad*)(stage + slotLoadOff());
    int nUpd = 0, nCols = 0, nLoads = 0;
    for (int b : m_slotPendingList) {
        SlotUpdate u = {};
        u.column = b;
        u.reset = m_slotPending[b] == 1 ? 1 : 0;
        if (u.reset && m_slotResume[b] != NULL) {      // a resume: ring and history from the blob, local sample `done` by this step
            m_slotHost[b].start = m_slotCounter - m_slotResumeDone[b];
            loads[nLoads++] = SlotLoad{m_slotResume[b], b, slotRotation(m_slotHost[b].start)};
            slotTouchTile(b);
            slotDropResume(b);
            u.reset = 0;
        } else if (u.reset) {
            m_slotHost[b].start = m_slotCounter;      // local sample 0 is generated by this step
            cols[nCols++] = b;
        }
        u.d = m_slotHost[b];
        upd[nUpd++] = u;
        m_slotPending[b] = 0;
    }
    m_slotPendingList.clear();
    gpuErrChk(hipMemcpyAsync(m_slotUpd, upd, (size_t)nUpd * sizeof(SlotUpdate), hipMemcpyHostToDevice, stream));
    if (nCols) gpuErrChk(hipMemcpyAsync(m_slotUpd + colOff, cols, (size_t)nCols * sizeof(int), hipMemcpyHostToDevice, stream));
    if (nLoads) gpuErrChk(hipMemcpyAsync(m_slotUpd + slotLoadOff(), loads, (size_t)nLoads * sizeof(SlotLoad), hipMemcpyHostToDevice, stream));
    m_slotStage.release(stream);
    bool ok = slots_reset(stream, m_slotDesc, (const SlotUpdate*)m_slotUpd, nUpd, (const int*)(m_slotUpd + colOff), nCols, f.ring, f.ringSlots,
                          f.ringFragsPerSlot, f.yInPrev, f.yInCur);
    if (nLoads)
        ok = slots_load(stream, (const SlotLoad*)(m_slotUpd + slotLoadOff()), nLoads, slotLayers(), f.ring, f.ringSlots, f.ringFragsPerSlot,
                        f.yInPrev, f.yInCur) && ok;
    return ok;
}
// ---- a column's sampling (slots_sampler.hpp): the next step writes the column's four table entries when a value changes ----
bool SlotSession::slotSamplingChange(int slot, const Sampling& s) {
    if (!inBatch(slot) || !slotHolds(slot) || !sampling_ok(s, f.A)) return false;
    slotSamplingSet(slot, s);
    return true;
}
void SlotSession::slotSamplingSet(int slot, const Sampling& s) {
    if (m_temps.get(slot) == s) return;
    m_temps.set(slot, s);
    if (m_tempDirty.empty()) m_tempDirty.assign(f.maxBatch, 0);
    if (!m_tempDirty[slot]) m_tempDirtyList.push_back(slot);
    m_tempDirty[slot] = 1;
}
// the pending start of column `slot` resumes from the blob `state`, whose (checked) header is h
void SlotSession::slotSetResume(int slot, const void* state, const SlotStateHeader& h) {
    slotLayers();
    m_slotResume[slot] = state;
    m_slotResumeDone[slot] = h.done;
    Sampling s;
    const bool ok = sampling_of_words(h.pad, f.A, s);      // (headerOk has checked them)
    assert(ok);
    (void)ok;
    slotSamplingSet(slot, s);
}
// the changed columns -> pinned staging -> device, then one slot_scale_kernel launch (staging halves as slotApplyPending, made
// by the first step that needs them)
bool SlotSession::slotApplyTemperatures(hipStream_t stream) {
    if (!m_temps.softScale) {      // (only columns that went back to 1 before anything else was set: the table does not exist)
        for (int b : m_tempDirtyList) m_tempDirty[b] = 0;
        m_tempDirtyList.clear();
        return true;
    }
    if (!m_scaleDev) {
        gpuErrChk(hipMalloc((void**)&m_scaleDev, 4 * (size_t)f.maxBatch * sizeof(SlotScale)));      // (a column's scale, floor, top-k and top-p)
        m_scaleStage.make(2, 4 * (size_t)f.maxBatch * sizeof(SlotScale));
    }
    SlotScale* const stage = (SlotScale*)m_scaleStage.acquire();
    int n = 0;
    for (int b : m_tempDirtyList) {
        float entry[kSamplingKinds];
        sampling_entries(m_temps.get(b), entry);
        for (int k = 0; k < kSamplingKinds; k++) stage[n++] = SlotScale{k * f.maxBatch + b, entry[k]};
        m_tempDirty[b] = 0;
    }
    m_tempDirtyList.clear();
    gpuErrChk(hipMemcpyAsync(m_scaleDev, stage, (size_t)n * sizeof(SlotScale), hipMemcpyHostToDevice, stream));
    m_scaleStage.release(stream);
    return slots_set_scales(stream, m_temps.softScale, 4 * f.maxBatch, m_scaleDev, n);
}
// ---- primed generation (slots_prime.hpp) ----
void SlotSession::slotPrimeSet(int slot, const int* y, int n) {
    if (m_primeN.empty()) {
        if (n == 0) return;
        m_primeY.assign(f.maxBatch, NULL);
        m_primeN.assign(f.maxBatch, 0);
        m_primeListed.assign(f.maxBatch, 0);
    }
    if (m_primeN[slot] != 0 || n != 0) m_primeDirty = true;
    m_primeY[slot] = y;
    m_primeN[slot] = n;
    if (n > 0 && !m_primeListed[slot]) {      // (a column that lost its prime leaves the list at the next step)
        m_primeList.push_back(slot);
        m_primeListed[slot] = 1;
    }
}
// A step of `count` samples from the counter with primed columns.  When the set of primed columns has changed since the table was
// written: the columns inside their prime in this step -> pinned staging -> device (staging halves as slotApplyPending, made by the
// first step that needs them).  Then one slot_prime_kernel launch over the window rows of the step, which takes every column's
// local sample from its descriptor; forced: it writes a forced sample.  Runs behind slotApplyPending and the feeds.  A column whose
// prime ends within the step has none afterwards, and the table is rewritten without it before it is read again.
bool SlotSession::slotApplyPrimes(int count, bool& forced, hipStream_t stream) {
    if (!m_primeDev) {
        gpuErrChk(hipMalloc((void**)&m_primeDev, (size_t)f.maxBatch * sizeof(SlotPrime)));
        m_primeStage.make(2, (size_t)f.maxBatch * sizeof(SlotPrime));
    }
    m_primeScratch.clear();
    size_t kept = 0;
    bool dropped = false;
    for (int b : m_primeList) {
        const int len = m_primeN[b];
        const long long k0 = m_slotCounter - (m_melHost[b].state ? m_melHost[b].start : m_slotHost[b].start);
        if (len > 0 && slotHolds(b) && k0 >= 0 && k0 < len) m_primeScratch.push_back(SlotPrime{m_primeY[b], len, b});
        if (len > 0 && slotHolds(b) && k0 >= 0 && k0 + count < len) {
            m_primeList[kept++] = b;
            continue;
        }
        m_primeY[b] = NULL;
        m_primeN[b] = 0;
        m_primeListed[b] = 0;
        dropped = true;
    }
    m_primeList.resize(kept);
    const int n = (int)m_primeScratch.size();
    forced = n > 0;
    if (n > 0 && (m_primeDirty || n != m_primeDevN)) {
        SlotPrime* const stage = (SlotPrime*)m_primeStage.acquire();
        memcpy(stage, m_primeScratch.data(), (size_t)n * sizeof(SlotPrime));
        gpuErrChk(hipMemcpyAsync(m_primeDev, stage, (size_t)n * sizeof(SlotPrime), hipMemcpyHostToDevice, stream));
        m_primeStage.release(stream);
        m_primeDevN = n;
        m_primeDirty = false;
    }
    if (dropped) m_primeDirty = true;      // (the table still names a column that has left its prime: rewritten before its next use)
    if (n == 0) return true;
    return slots_prime(stream, m_slotSel, f.maxBatch, m_slotCounter, (int)(m_slotCounter % m_slotW), m_slotW, count, m_primeDev, m_primeDevN, m_slotDesc,
                       m_melDesc, f.A);
}
// ---- mel columns (slots_mel.hpp) ----
void SlotSession::melMarkDirty(int slot) {
    if (!m_melDirty[slot]) m_melDirtyList.push_back(slot);
    m_melDirty[slot] = 1;
}
// a column that is started or stopped stops being a mel column
void SlotSession::slotDropMel(int slot) {
    if (!m_melHost[slot].state) return;
    m_melHost[slot].state = 0;
    m_melColumns--;
    melMarkDirty(slot);
    m_melTilesDirty = true;
}
void SlotSession::melAllocate() {
    allocZero(m_melDesc, (size_t)f.maxBatch * sizeof(MelDesc));
    const size_t bytes = melTileOff() + (size_t)f.tiles * sizeof(int);
    gpuErrChk(hipMalloc((void**)&m_melUpd, bytes));
    gpuErrChk(hipMalloc((void**)&m_melColInfo, (size_t)f.tiles * 16 * 2 * sizeof(int)));
    m_melStageHost.make(2, bytes);
    if (!m_melPrepared) m_melPrepared = f.f16 ? slots_mel_prepare<true>() : slots_mel_prepare<false>();
    gpuErrChk(hipDeviceSynchronize());
}
// the stage and records of a step of `count` samples (grown when a longer step needs more; the steps before it are waited for)
char* SlotSession::melStage(int count, const SlotLive& v) {
    m_melRecOff = featBytes(slots_mel_stage_frames(count, v.upStride, v.upWindow / v.upStride));
    const size_t need = m_melRecOff + featBytes(count);
    if (need > m_melStageBytes) {
        gpuErrChk(hipDeviceSynchronize());
        freeDev(m_melStage);
        gpuErrChk(hipMalloc((void**)&m_melStage, need));
        m_melStageBytes = need;
    }
    return m_melStage;
}
// the changed mel descriptors (a start takes the counter of this step) and, when it changed, the list of tiles holding mel
// columns -> pinned staging -> device, and one slot_mel_apply_kernel launch; the staging half is reused two steps later
bool SlotSession::melApplyPending(hipStream_t stream) {
    char* const stage = (char*)m_melStageHost.acquire();
    MelUpdate* const upd = (MelUpdate*)stage;
    int* const tileList = (int*)(stage + melTileOff());
    int nUpd = 0;
    for (int b : m_melDirtyList) {
        MelDesc& d = m_melHost[b];
        if (d.state && m_slotPending[b] == 1) d.start = m_slotCounter - m_slotResumeDone[b];      // local sample 0 (resumed: done) is generated by this step
        upd[nUpd].column = b;
        upd[nUpd].pad = 0;
        upd[nUpd].d = d;
        nUpd++;
        m_melDirty[b] = 0;
    }
    m_melDirtyList.clear();
    bool ok = true;
    if (nUpd) {
        gpuErrChk(hipMemcpyAsync(m_melUpd, upd, (size_t)nUpd * sizeof(MelUpdate), hipMemcpyHostToDevice, stream));
        ok = slots_mel_apply(stream, m_melDesc, (const MelUpdate*)m_melUpd, nUpd);
    }
    if (m_melTilesDirty) {
        int n = 0;
        for (int tile = 0; tile * 16 < f.maxBatch; tile++)
            for (int j = 0; j < 16 && tile * 16 + j < f.maxBatch; j++)
                if (m_melHost[tile * 16 + j].state) {
                    tileList[n++] = tile;
                    break;
                }
        if (n) gpuErrChk(hipMemcpyAsync(m_melUpd + melTileOff(), tileList, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
        m_melTiles = n;
        m_melTilesDirty = false;
    }
    m_melStageHost.release(stream);
    return ok;
}

}  // namespace wn
