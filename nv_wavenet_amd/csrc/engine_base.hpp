// engine_base.hpp -- type-erased door onto nvWavenetInfer<...> instantiations for the C ABI
// (include/nv_wavenet_c.h).  One translation unit per instantiation (engine_inst.hip) so the
// big kernel templates compile in parallel.
#pragma once
#include "../../include/nv_wavenet_c.h"
#include "nv_wavenet.hpp"

struct nvw_engine {
    virtual ~nvw_engine() {}
    virtual void setEmbeddings(float*, float*) = 0;
    virtual void setLayerWeights(int, float*, float*, float*, float*, float*, float*, float*) = 0;
    virtual void setOutWeights(float*, float*, float*, float*) = 0;
    virtual void setInputs(float*, float*, int) = 0;
    virtual void setConditioning(float*, int) = 0;
    virtual void packConditioning(float*, int, int, hipStream_t) = 0;
    virtual void setConditioningDirect(const void*, int, int) = 0;
    virtual void setConditioningPacked(const void*, int) = 0;
    virtual int condTiles() = 0;
    virtual bool setConditioningWeights(const float*, const float*, int) = 0;
    virtual int featureFragments() = 0;
    virtual size_t featureElems(int) = 0;
    virtual void setConditioningFeatures(const void*, int) = 0;
    virtual void packFeatures(const void*, int, long long, long long, long long, int, int, hipStream_t) = 0;
    virtual void setFeatures(const void*, int, long long, long long, long long, int) = 0;
    virtual int conditioningChannels() = 0;
    virtual bool setUpsampling(const float*, const float*, int, int) = 0;
    virtual int upsamplingStride() = 0;
    virtual int melSamples() = 0;
    virtual bool hasFeatureBuffer() = 0;
    virtual int maxBatch() = 0;
    virtual void getFeatures(void*, int, int) = 0;
    virtual void setMel(const void*, int, long long, long long, long long, int) = 0;
    virtual void upsampleFeatures(int, int, hipStream_t) = 0;
    virtual bool run_stream(int, nvw_consume_fn, void*, int, int, int*, hipStream_t) = 0;
    virtual size_t condPackedElems(int) = 0;
    virtual void setSelectors(float*, int) = 0;
    virtual bool run_range(int, int, int, int, hipStream_t) = 0;
    virtual void resetHistory(hipStream_t) = 0;
    virtual bool supported() = 0;
    virtual unsigned chainStatus() = 0;
    virtual unsigned chainFallbacks() = 0;
    virtual unsigned chainLastTimeout() = 0;
    virtual void setChainTimeoutMs(double) = 0;
    virtual void setClockProbe(bool) = 0;
    virtual void setRingInLds(int) = 0;
    virtual void setCompiledSchedule(int) = 0;
    virtual double lastLaunchClockGHz() = 0;
    virtual int precisionBits() = 0;
    virtual int maxSamples() = 0;
    virtual void setSelectorSeed(unsigned long long) = 0;
    virtual void setAudioOut(short*, size_t) = 0;
    virtual void kernelInfo(int, bool, char*, int) = 0;
    virtual bool run(int, int, int*, int, bool, hipStream_t) = 0;
    virtual bool run_partial(int, int, int, int*, int, bool, hipStream_t) = 0;
    virtual bool run_chunks(int, nvw_consume_fn, void*, int, int, int*, int, bool, hipStream_t) = 0;
    virtual void getXtOut(int, float*) = 0;
    virtual void getSkipOut(int, float*) = 0;
    virtual void getZs(float*) = 0;
    virtual void getZa(float*) = 0;
    virtual void getP(float*) = 0;
    virtual void getYOut(int*, int, int, hipStream_t) = 0;
    virtual bool setTemperatures(const float*, int) = 0;
    virtual bool setMinP(const float*, int) = 0;
    virtual bool setTopK(const int*, int) = 0;
    virtual bool setTopP(const float*, int) = 0;
    virtual int samplerMask() = 0;
    virtual bool setPrime(const int*, const int*, int, int, long long) = 0;
    virtual int prefillWindow() = 0;
    virtual int prefillStates(const wn::PrefillReq*, int, void*, long long, hipStream_t) = 0;
    virtual int scoreMaxSamples() = 0;
    virtual int scoreSamples(const wn::ScoreReq*, int, hipStream_t) = 0;
    virtual int upsampleRowElems() = 0;
    virtual int upsampleRequests(const wn::MelTimeReq*, int, hipStream_t) = 0;
    virtual int prefillStatesMel(const wn::PrefillMelReq*, int, void*, long long, hipStream_t) = 0;
    virtual int scoreSamplesMel(const wn::ScoreMelReq*, int, hipStream_t) = 0;
    virtual int scoreChunks(const wn::ScoreChunkReq*, int, hipStream_t) = 0;
    virtual int scoreChunksMel(const wn::ScoreChunkMelReq*, int, hipStream_t) = 0;
    virtual wn::SlotSession& slots() = 0;      // slot mode is the session's: the C functions call it directly
};
static_assert(sizeof(nvw_slot_piece) == sizeof(wn::SlotPiece) && offsetof(nvw_slot_piece, slot) == offsetof(wn::SlotPiece, slot) &&
              offsetof(nvw_slot_piece, uid) == offsetof(wn::SlotPiece, uid) && offsetof(nvw_slot_piece, finished) == offsetof(wn::SlotPiece, finished) &&
              offsetof(nvw_slot_piece, first) == offsetof(wn::SlotPiece, first) &&
              offsetof(nvw_slot_piece, n) == offsetof(wn::SlotPiece, n) && offsetof(nvw_slot_piece, offset) == offsetof(wn::SlotPiece, offset),
              "nvw_slot_piece is wn::SlotPiece");

static_assert(sizeof(nvw_slot_saved) == sizeof(wn::SlotSaved) && offsetof(nvw_slot_saved, slot) == offsetof(wn::SlotSaved, slot) &&
              offsetof(nvw_slot_saved, uid) == offsetof(wn::SlotSaved, uid) && offsetof(nvw_slot_saved, done) == offsetof(wn::SlotSaved, done) &&
              offsetof(nvw_slot_saved, mel) == offsetof(wn::SlotSaved, mel),
              "nvw_slot_saved is wn::SlotSaved");
static_assert(sizeof(nvw_slot_resume_req) == sizeof(wn::SlotResumeReq) && offsetof(nvw_slot_resume_req, slot) == offsetof(wn::SlotResumeReq, slot) &&
              offsetof(nvw_slot_resume_req, mel) == offsetof(wn::SlotResumeReq, mel) && offsetof(nvw_slot_resume_req, src) == offsetof(wn::SlotResumeReq, src) &&
              offsetof(nvw_slot_resume_req, precision) == offsetof(wn::SlotResumeReq, precision) &&
              offsetof(nvw_slot_resume_req, c_stride) == offsetof(wn::SlotResumeReq, cStride) &&
              offsetof(nvw_slot_resume_req, t_stride) == offsetof(wn::SlotResumeReq, tStride) &&
              offsetof(nvw_slot_resume_req, length) == offsetof(wn::SlotResumeReq, length) &&
              offsetof(nvw_slot_resume_req, final) == offsetof(wn::SlotResumeReq, final),
              "nvw_slot_resume_req is wn::SlotResumeReq");

static_assert(sizeof(nvw_prefill_req) == sizeof(wn::PrefillReq) && offsetof(nvw_prefill_req, y) == offsetof(wn::PrefillReq, y) &&
              offsetof(nvw_prefill_req, n) == offsetof(wn::PrefillReq, n) && offsetof(nvw_prefill_req, x) == offsetof(wn::PrefillReq, x) &&
              offsetof(nvw_prefill_req, precision) == offsetof(wn::PrefillReq, precision) &&
              offsetof(nvw_prefill_req, c_stride) == offsetof(wn::PrefillReq, cStride) &&
              offsetof(nvw_prefill_req, t_stride) == offsetof(wn::PrefillReq, tStride) && offsetof(nvw_prefill_req, uid) == offsetof(wn::PrefillReq, uid) &&
              offsetof(nvw_prefill_req, temperature) == offsetof(wn::PrefillReq, temperature),
              "nvw_prefill_req is wn::PrefillReq");

static_assert(sizeof(nvw_score_req) == sizeof(wn::ScoreReq) && offsetof(nvw_score_req, y) == offsetof(wn::ScoreReq, y) &&
              offsetof(nvw_score_req, n) == offsetof(wn::ScoreReq, n) && offsetof(nvw_score_req, x) == offsetof(wn::ScoreReq, x) &&
              offsetof(nvw_score_req, precision) == offsetof(wn::ScoreReq, precision) &&
              offsetof(nvw_score_req, c_stride) == offsetof(wn::ScoreReq, cStride) &&
              offsetof(nvw_score_req, t_stride) == offsetof(wn::ScoreReq, tStride) &&
              offsetof(nvw_score_req, temperature) == offsetof(wn::ScoreReq, temperature) &&
              offsetof(nvw_score_req, logp) == offsetof(wn::ScoreReq, logp) && offsetof(nvw_score_req, rows) == offsetof(wn::ScoreReq, rows),
              "nvw_score_req is wn::ScoreReq");
static_assert(sizeof(nvw_upsample_req) == sizeof(wn::MelTimeReq) && offsetof(nvw_upsample_req, mel) == offsetof(wn::MelTimeReq, mel) &&
              offsetof(nvw_upsample_req, precision) == offsetof(wn::MelTimeReq, precision) &&
              offsetof(nvw_upsample_req, c_stride) == offsetof(wn::MelTimeReq, cStride) &&
              offsetof(nvw_upsample_req, f_stride) == offsetof(wn::MelTimeReq, fStride) &&
              offsetof(nvw_upsample_req, frames) == offsetof(wn::MelTimeReq, frames) &&
              offsetof(nvw_upsample_req, first_sample) == offsetof(wn::MelTimeReq, first) &&
              offsetof(nvw_upsample_req, count) == offsetof(wn::MelTimeReq, count) && offsetof(nvw_upsample_req, dst) == offsetof(wn::MelTimeReq, dst),
              "nvw_upsample_req is wn::MelTimeReq");
static_assert(sizeof(nvw_prefill_mel_req) == sizeof(wn::PrefillMelReq) && offsetof(nvw_prefill_mel_req, y) == offsetof(wn::PrefillMelReq, y) &&
              offsetof(nvw_prefill_mel_req, n) == offsetof(wn::PrefillMelReq, n) && offsetof(nvw_prefill_mel_req, mel) == offsetof(wn::PrefillMelReq, mel) &&
              offsetof(nvw_prefill_mel_req, precision) == offsetof(wn::PrefillMelReq, precision) &&
              offsetof(nvw_prefill_mel_req, c_stride) == offsetof(wn::PrefillMelReq, cStride) &&
              offsetof(nvw_prefill_mel_req, f_stride) == offsetof(wn::PrefillMelReq, fStride) &&
              offsetof(nvw_prefill_mel_req, frames) == offsetof(wn::PrefillMelReq, frames) &&
              offsetof(nvw_prefill_mel_req, uid) == offsetof(wn::PrefillMelReq, uid) &&
              offsetof(nvw_prefill_mel_req, temperature) == offsetof(wn::PrefillMelReq, temperature),
              "nvw_prefill_mel_req is wn::PrefillMelReq");
static_assert(sizeof(nvw_score_mel_req) == sizeof(wn::ScoreMelReq) && offsetof(nvw_score_mel_req, y) == offsetof(wn::ScoreMelReq, y) &&
              offsetof(nvw_score_mel_req, n) == offsetof(wn::ScoreMelReq, n) && offsetof(nvw_score_mel_req, mel) == offsetof(wn::ScoreMelReq, mel) &&
              offsetof(nvw_score_mel_req, precision) == offsetof(wn::ScoreMelReq, precision) &&
              offsetof(nvw_score_mel_req, c_stride) == offsetof(wn::ScoreMelReq, cStride) &&
              offsetof(nvw_score_mel_req, f_stride) == offsetof(wn::ScoreMelReq, fStride) &&
              offsetof(nvw_score_mel_req, frames) == offsetof(wn::ScoreMelReq, frames) &&
              offsetof(nvw_score_mel_req, temperature) == offsetof(wn::ScoreMelReq, temperature) &&
              offsetof(nvw_score_mel_req, logp) == offsetof(wn::ScoreMelReq, logp) && offsetof(nvw_score_mel_req, rows) == offsetof(wn::ScoreMelReq, rows),
              "nvw_score_mel_req is wn::ScoreMelReq");
static_assert(sizeof(nvw_score_chunk_req) == sizeof(wn::ScoreChunkReq) && offsetof(nvw_score_chunk_req, state) == offsetof(wn::ScoreChunkReq, state) &&
              offsetof(nvw_score_chunk_req, y) == offsetof(wn::ScoreChunkReq, y) && offsetof(nvw_score_chunk_req, n) == offsetof(wn::ScoreChunkReq, n) &&
              offsetof(nvw_score_chunk_req, x) == offsetof(wn::ScoreChunkReq, x) &&
              offsetof(nvw_score_chunk_req, precision) == offsetof(wn::ScoreChunkReq, precision) &&
              offsetof(nvw_score_chunk_req, c_stride) == offsetof(wn::ScoreChunkReq, cStride) &&
              offsetof(nvw_score_chunk_req, t_stride) == offsetof(wn::ScoreChunkReq, tStride) &&
              offsetof(nvw_score_chunk_req, uid) == offsetof(wn::ScoreChunkReq, uid) &&
              offsetof(nvw_score_chunk_req, temperature) == offsetof(wn::ScoreChunkReq, temperature) &&
              offsetof(nvw_score_chunk_req, logp) == offsetof(wn::ScoreChunkReq, logp) &&
              offsetof(nvw_score_chunk_req, rows) == offsetof(wn::ScoreChunkReq, rows) &&
              offsetof(nvw_score_chunk_req, state_out) == offsetof(wn::ScoreChunkReq, stateOut),
              "nvw_score_chunk_req is wn::ScoreChunkReq");
static_assert(sizeof(nvw_score_chunk_mel_req) == sizeof(wn::ScoreChunkMelReq) &&
              offsetof(nvw_score_chunk_mel_req, state) == offsetof(wn::ScoreChunkMelReq, state) &&
              offsetof(nvw_score_chunk_mel_req, y) == offsetof(wn::ScoreChunkMelReq, y) &&
              offsetof(nvw_score_chunk_mel_req, n) == offsetof(wn::ScoreChunkMelReq, n) &&
              offsetof(nvw_score_chunk_mel_req, mel) == offsetof(wn::ScoreChunkMelReq, mel) &&
              offsetof(nvw_score_chunk_mel_req, precision) == offsetof(wn::ScoreChunkMelReq, precision) &&
              offsetof(nvw_score_chunk_mel_req, c_stride) == offsetof(wn::ScoreChunkMelReq, cStride) &&
              offsetof(nvw_score_chunk_mel_req, f_stride) == offsetof(wn::ScoreChunkMelReq, fStride) &&
              offsetof(nvw_score_chunk_mel_req, frames) == offsetof(wn::ScoreChunkMelReq, frames) &&
              offsetof(nvw_score_chunk_mel_req, uid) == offsetof(wn::ScoreChunkMelReq, uid) &&
              offsetof(nvw_score_chunk_mel_req, temperature) == offsetof(wn::ScoreChunkMelReq, temperature) &&
              offsetof(nvw_score_chunk_mel_req, logp) == offsetof(wn::ScoreChunkMelReq, logp) &&
              offsetof(nvw_score_chunk_mel_req, rows) == offsetof(wn::ScoreChunkMelReq, rows) &&
              offsetof(nvw_score_chunk_mel_req, state_out) == offsetof(wn::ScoreChunkMelReq, stateOut),
              "nvw_score_chunk_mel_req is wn::ScoreChunkMelReq");

template <typename Tw, typename Td, int R, int S, int A>
struct EngineImpl : nvw_engine {
    nvWavenetInfer<Tw, Td, R, S, A> eng;
    int cap;
    EngineImpl(int L, int maxD, int B, int N, int impl, bool tanhEmbed, int org) : eng(L, maxD, B, N, impl, tanhEmbed, org), cap(N) {}
    void setEmbeddings(float* p, float* c) override { eng.setEmbeddings(p, c); }
    void setLayerWeights(int l, float* a, float* b, float* c, float* d, float* e, float* f, float* g) override {
        eng.setLayerWeights(l, a, b, c, d, e, f, g);
    }
    void setOutWeights(float* a, float* b, float* c, float* d) override { eng.setOutWeights(a, b, c, d); }
    void setInputs(float* Lh, float* sel, int n) override { eng.setInputs(Lh, sel, n); }
    void setConditioning(float* Lh, int n) override { eng.setConditioning(Lh, n); }
    void packConditioning(float* Lh, int first, int count, hipStream_t s) override { eng.packConditioning(Lh, first, count, s); }
    void setConditioningDirect(const void* Lh, int n, int prec) override { eng.setConditioningDirect(Lh, n, prec); }
    void setConditioningPacked(const void* frags, int n) override { eng.setConditioningPacked(frags, n); }
    int condTiles() override { return eng.condTiles(); }
    bool setConditioningWeights(const float* W, const float* b, int n) override { return eng.setConditioningWeights(W, b, n); }
    int featureFragments() override { return eng.featureFragments(); }
    size_t featureElems(int n) override { return eng.featureElems(n); }
    void setConditioningFeatures(const void* f, int n) override { eng.setConditioningFeatures(f, n); }
    void packFeatures(const void* x, int prec, long long bS, long long cS, long long tS, int first, int count, hipStream_t s) override {
        eng.packFeatures(x, prec, bS, cS, tS, first, count, s);
    }
    void setFeatures(const void* x, int prec, long long bS, long long cS, long long tS, int n) override { eng.setFeatures(x, prec, bS, cS, tS, n); }
    int conditioningChannels() override { return eng.conditioningChannels(); }
    bool setUpsampling(const float* W, const float* b, int window, int stride) override { return eng.setUpsampling(W, b, window, stride); }
    int upsamplingStride() override { return eng.upsamplingStride(); }
    int melSamples() override { return eng.melSamples(); }
    bool hasFeatureBuffer() override { return eng.hasFeatureBuffer(); }
    int maxBatch() override { return eng.maxBatch(); }
    void getFeatures(void* d, int first, int count) override { eng.getFeatures(d, first, count); }
    void setMel(const void* mel, int prec, long long bS, long long cS, long long fS, int frames) override { eng.setMel(mel, prec, bS, cS, fS, frames); }
    void upsampleFeatures(int first, int count, hipStream_t s) override { eng.upsampleFeatures(first, count, s); }
    bool run_stream(int chunk, nvw_consume_fn fn, void* user, int n, int b, int* y, hipStream_t s) override {
        return eng.run_stream(chunk, [fn, user](int* yo, int i, int c) { if (fn) fn(yo, i, c, user); }, n, b, y, s);
    }
    size_t condPackedElems(int n) override { return eng.condPackedElems(n); }
    void setSelectors(float* sel, int n) override { eng.setSelectors(sel, n); }
    bool run_range(int i, int c, int n, int b, hipStream_t s) override { return eng.run_range(i, c, n, b, s); }
    void resetHistory(hipStream_t s) override { eng.resetHistory(s); }
    bool supported() override { return eng.supported(); }
    unsigned chainStatus() override { return eng.chainStatus(); }
    unsigned chainFallbacks() override { return eng.chainFallbacks(); }
    unsigned chainLastTimeout() override { return eng.chainLastTimeout(); }
    void setChainTimeoutMs(double ms) override { eng.setChainTimeoutMs(ms); }
    void setClockProbe(bool on) override { eng.setClockProbe(on); }
    void setRingInLds(int mode) override { eng.setRingInLds(mode); }
    void setCompiledSchedule(int mode) override { eng.setCompiledSchedule(mode); }
    double lastLaunchClockGHz() override { return eng.lastLaunchClockGHz(); }
    int precisionBits() override { return std::is_same<Td, float>::value ? 32 : 16; }
    int maxSamples() override { return cap; }
    void setSelectorSeed(unsigned long long seed) override { eng.setSelectorSeed(seed); }
    void setAudioOut(short* pcm, size_t n) override { eng.setAudioOut(pcm, n); }
    void kernelInfo(int b, bool dump, char* buf, int n) override { eng.kernelInfo(b, dump, buf, n); }
    bool run(int n, int b, int* y, int bspb, bool dump, hipStream_t s) override {
        return eng.run(n, b, y, bspb, dump, s);
    }
    bool run_partial(int i, int n, int b, int* y, int bspb, bool dump, hipStream_t s) override {
        return eng.run_partial(i, n, b, y, bspb, dump, s);
    }
    bool run_chunks(int chunk, nvw_consume_fn fn, void* user, int n, int b, int* y, int bspb, bool dump,
                    hipStream_t s) override {
        return eng.run_chunks(chunk, [fn, user](int* yo, int i, int c) { if (fn) fn(yo, i, c, user); }, n, b, y,
                              bspb, dump, s);
    }
    void getXtOut(int l, float* d) override { eng.getXtOut(l, d); }
    void getSkipOut(int l, float* d) override { eng.getSkipOut(l, d); }
    void getZs(float* d) override { eng.getZs(d); }
    void getZa(float* d) override { eng.getZa(d); }
    void getP(float* d) override { eng.getP(d); }
    void getYOut(int* y, int off, int size, hipStream_t s) override { eng.getYOut(y, off, size, s); }
    bool setTemperatures(const float* T, int n) override { return eng.setTemperatures(T, n); }
    bool setMinP(const float* p, int n) override { return eng.setMinP(p, n); }
    bool setTopK(const int* k, int n) override { return eng.setTopK(k, n); }
    bool setTopP(const float* p, int n) override { return eng.setTopP(p, n); }
    int samplerMask() override { return eng.floorMask(); }
    bool setPrime(const int* y, const int* n, int batch, int maxN, long long stride) override { return eng.setPrime(y, n, batch, maxN, stride); }
    int prefillWindow() override { return eng.prefillWindow(); }
    int prefillStates(const wn::PrefillReq* reqs, int count, void* dst, long long stride, hipStream_t s) override {
        return eng.prefillStates(reqs, count, dst, stride, s);
    }
    int scoreMaxSamples() override { return eng.scoreMaxSamples(); }
    int scoreSamples(const wn::ScoreReq* reqs, int count, hipStream_t s) override { return eng.scoreSamples(reqs, count, s); }
    int upsampleRowElems() override { return eng.upsampleRowElems(); }
    int upsampleRequests(const wn::MelTimeReq* reqs, int count, hipStream_t s) override { return eng.upsampleRequests(reqs, count, s); }
    int prefillStatesMel(const wn::PrefillMelReq* reqs, int count, void* dst, long long stride, hipStream_t s) override {
        return eng.prefillStatesMel(reqs, count, dst, stride, s);
    }
    int scoreSamplesMel(const wn::ScoreMelReq* reqs, int count, hipStream_t s) override { return eng.scoreSamplesMel(reqs, count, s); }
    int scoreChunks(const wn::ScoreChunkReq* reqs, int count, hipStream_t s) override { return eng.scoreChunks(reqs, count, s); }
    int scoreChunksMel(const wn::ScoreChunkMelReq* reqs, int count, hipStream_t s) override { return eng.scoreChunksMel(reqs, count, s); }
    wn::SlotSession& slots() override { return eng.slots(); }
};

typedef nvw_engine* (*nvw_factory_fn)(int L, int maxD, int B, int N, int impl, int tanhEmbed, int organisation);

#define WN_CAT2(a, b) a##b
#define WN_CAT(a, b) WN_CAT2(a, b)
#define WN_FACTORY_NAME(R, S, A, P) WN_CAT(WN_CAT(WN_CAT(WN_CAT(WN_CAT(WN_CAT(WN_CAT(nvw_make_, R), _), S), _), A), _p), P)
