// slots_session.hpp -- the host half of slot mode (slots.hpp; DESIGN.md "Slot mode", §6c-§6h): wn::SlotSession keeps the window, the
// descriptor tables, the pending lists, the staging copies and the tickets, and issues the slot kernels.  It is bookkeeping around
// kernels that are compiled once for both precisions, so it is compiled once as well (slots_session.hip): the precision is a
// run-time fact, and what belongs to the engine -- the model, the ring, the generation launch -- is reached through wn::SlotHost.
// The comments name the calls as the C ABI and the Python wrapper do: slotStart is start(), slotsStepRagged is stepRagged(), ...
#pragma once

#include <assert.h>

#include <vector>

#include "gpu_check.hpp"
#include "slots.hpp"
#include "slots_deliver.hpp"
#include "slots_mel.hpp"
#include "slots_prime.hpp"
#include "slots_sampler.hpp"
#include "slots_state.hpp"

namespace wn {

// what is fixed when the engine has been constructed
struct SlotFacts {
    int maxBatch, tiles, numLayers, maxDilation, ringSlots;
    int ringFragsPerSlot;      // 1-KiB fragments of one ring slot of one tile
    int R;
    bool f16;                  // the engine's T_data: selects the <F16> launchers and gives the element size
    size_t featRowElems;       // elements (T_data) of one sample's feature row, all tiles (featureElems(1))
    bool supported;            // the shape fits a CU
    void* ring;                // the engine's dilation ring and sample history
    int *yInPrev, *yInCur;
    int A;                     // the alphabet: a forced sample is clamped into 0 .. A-1 (slots_prime.hpp)
};
// what a call reads afresh (the caller may hand over weights, an upsampling or a seed between two calls)
struct SlotLive {
    int nCond;                 // channels of the model's features (0: no conditioning weights yet)
    const void* upTab;         // the table, bias, window and stride of setUpsampling (stride 0: none)
    const float* upBias;
    int upWindow, upStride;
    unsigned long long seed;   // of setSelectorSeed
};
// the engine as a session sees it
struct SlotHost {
    virtual SlotLive slotLive() const = 0;
    virtual const short* slotMulaw() = 0;      // the PCM value of every sample index, on the device (made once)
    // the weight stream that carries the conditioning weights is up to date on `stream`
    virtual void slotFeatStreamReady(hipStream_t stream) = 0;
    // launches have written the rings of the leading `tiles` tiles
    virtual void slotRingsDirty(int tiles) = 0;
    // wavenet_wg<.., RAW=3> on window rows [t0, t0 + count) of the first `cols` columns: features feat [W][tiles][KFC], selector
    // table sel [W][maxBatch], samples into y [maxBatch][W]; forced: the rows hold forced samples (Params::forced; slots_prime.hpp)
    virtual bool slotGenerate(const void* feat, const float* sel, int* y, int W, int t0, int count, int cols, bool forced,
                              hipStream_t stream) = 0;
};

// n pinned host buffers with an event each, used in turn: acquire() hands out the next buffer, waiting first for the work that
// buffer carried n uses ago (a buffer that has carried none waits for nothing); the caller fills it and queues its copy;
// release(stream) records the buffer's event behind that copy and moves on.
class StageRing {
public:
    StageRing() {}
    StageRing(const StageRing&) = delete;      // (owns its buffers and events)
    ~StageRing() { reset(); }
    void make(int n, size_t bytes);
    void reset();                                                      // frees; uses() back to 0
    int at() const { assert(!m_buf.empty()); return (int)(m_uses % m_buf.size()); }      // the index of the next use (of a made ring)
    void* buffer(int i) const { return m_buf[i]; }
    hipEvent_t event(int i) const { return m_ev[i]; }
    unsigned long long uses() const { return m_uses; }                 // release() calls so far
    void* acquire();
    void release(hipStream_t stream);

private:
    std::vector<void*> m_buf;
    std::vector<hipEvent_t> m_ev;
    unsigned long long m_uses = 0;
};

class SlotSession {
public:
    SlotSession(const SlotFacts& facts, SlotHost& host, SamplingTable& temps);
    ~SlotSession();

    // ---- slot mode: continuous batching (slots.hpp; DESIGN.md "Slot mode") ------------------------------------------------------
    // Every column holds one utterance that starts and stops on its own while the others go on.  An utterance's samples depend on
    // its features, its uid, the seed, the model, the temperature in force at each local sample (slotSetTemperature; 1 by default)
    // and its prime (prime(); none by default) only: local sample k draws philox_selector(seed, {k, uid}) -- column uid of a
    // lockstep setFeatures + setSelectorSeed run --, its rings start at zero and its history at 128.  The state between steps lives
    // in a window of W samples that wraps; the generation kernel is wavenet_wg<.., RAW=3> as the features path launches it, on
    // window rows, reading the selectors from a table (useRng = 0).  Needs setConditioningWeights; the seed is the one of
    // setSelectorSeed (0 if none was set).  Steps of a session are issued on one stream (they share the window and the rings).
    int largestDilation() const { return m_largestD; }      // of the schedule: the window is a multiple of it, so that t mod W keeps t & (d - 1)
    // Enters slot mode with a window of `window` samples (ends a session in progress; every column idle).  false: no conditioning
    // weights yet, or the window is not a positive multiple of largestDilation().  Synchronises.
    bool begin(int window);
    bool active() const { return m_slotW > 0; }
    // Column `slot` takes a new utterance at the next step: its upsampled features x[c * cStride + k * tStride] (device memory,
    // `precision`-bit floats, n_cond channels x `length` samples; kept alive and unchanged while the column runs), its uid.  Replaces
    // whatever the column held.  false (nothing changes): not in slot mode, slot outside the batch, non-device x, bad precision,
    // non-positive strides or length; or the column is the destination of a pending move (the start would silently drop the
    // utterance on its way in: stop it, or step first).
    bool start(int slot, const void* x, int precision, long long cStride, long long tStride, int length, unsigned uid);
    // Column `slot` goes idle at the next step (its features are no longer read from then on); its sampling values go back to off.
    bool stop(int slot);
    // Column `slot` takes a mel utterance at the next step: its frames mel[c * cStride + f * fStride] (device memory,
    // `precision`-bit floats, n_cond channels; kept alive while the column runs), `frames` of them available so far, final != 0: no
    // more will come (its length is frames x stride), its uid.  Upsampled with the table of setUpsampling in the steps that generate
    // them.  Replaces whatever the column held.  false (nothing changes): not in slot mode, no upsampling, slot outside the batch,
    // non-device mel, bad precision, non-positive strides, frames < 0, 0 frames of a final utterance, or the column is the destination
    // of a pending move.
    bool startMel(int slot, const void* mel, int precision, long long cStride, long long fStride, int frames, int final, unsigned uid);
    // More frames of the mel utterance of column `slot` are available in the same buffer (written by the caller, ordered before the
    // next step on the step stream); final != 0: no more will come.  false (nothing changes): not a mel column, already final, the
    // count decreases, or 0 frames made final.
    bool melFrames(int slot, int frames, int final);
    // The utterance of column `slot` samples from softmax(logits / T) from the next step on, from that step's first sample (the
    // local sample the column has reached then); T as for setTemperatures.  slotStart / slotStartMel put the column back to 1, so
    // the order is start, then set; slotsBegin and slotsEnd put every column back to 1.  Moves, saves and resumes carry the value
    // (a blob holds it in SlotStateHeader::pad[0]).  A step with changed columns issues one small launch (slots_set_scales) ahead
    // of its generation launch.  false (nothing changes): not in slot mode, slot outside the batch, a column that holds no
    // utterance and has no pending start or resume, or a bad value.
    bool setTemperature(int slot, float T);
    // the host's value for column `slot`; 0 when it holds no utterance (or outside slot mode, or outside the batch)
    float temperature(int slot) const { return inBatch(slot) && slotHolds(slot) ? m_temps.get(slot).temperature : 0.f; }
    // The utterance of column `slot` draws without the bins whose tempered probability is below p times that of the most probable
    // bin (min-p), from the next step on, from that step's first sample; p as for setMinP.  Everything else as
    // setTemperature: starts put the column back to 0, moves, saves and resumes carry the value (SlotStateHeader::pad[1]), and the
    // step's one small launch writes the changed floors with the changed scales.  false (nothing changes): as setTemperature.
    bool setMinP(int slot, float p);
    // the host's value for column `slot`; -1 when it holds no utterance (0 is a valid floor)
    float minP(int slot) const { return inBatch(slot) && slotHolds(slot) ? m_temps.get(slot).minP : -1.f; }
    // The utterance of column `slot` draws from the k most probable bins of its tempered distribution (top-k; 0: off), or from the
    // smallest set of most probable bins whose mass reaches p (top-p; 1: off), ties at either boundary included, from
    // the next step on; the cuts and the floor intersect.  Everything else as setMinP: starts put the column back to off, moves, saves
    // and resumes carry the values (SlotStateHeader::pad[2], pad[3]), the step's one small launch writes them.  false (nothing
    // changes): as setTemperature; k outside [0, A]; p not finite or outside (0, 1].
    bool setTopK(int slot, int k);
    bool setTopP(int slot, float p);
    // the host's values for column `slot`; -1 when it holds no utterance
    int topK(int slot) const { return inBatch(slot) && slotHolds(slot) ? m_temps.get(slot).topK : -1; }
    float topP(int slot) const { return inBatch(slot) && slotHolds(slot) ? m_temps.get(slot).topP : -1.f; }
    // ---- primed generation (slots_prime.hpp) ----
    // The utterance whose start or resume is pending on column `slot` carries the prime y[0 .. n) (device memory, int32; kept alive and
    // unchanged until local sample n has been generated): its local samples k < n are y[k], clamped into the alphabet, delivered and
    // fed back like drawn ones; from k = n on it draws {k, uid} as always.  Order: start (or resume), then prime -- slotStart /
    // slotStartMel / slotResume* put the column back to "no prime", slotStop, slotsBegin and slotsEnd drop it, slotMove carries it.  A
    // resumed column whose blob has done < n is primed again with the same y, n: the samples below done are never reached.  A step
    // with a column inside its prime issues one small launch (slot_prime_kernel) between the feed and the generation, whose launches
    // then decode forced selectors; a step without issues what it issued before.  false (nothing changes): not in slot mode, slot
    // outside the batch, no pending start or resume on the column, y not device memory, n < 1, or n above the utterance's length
    // (a non-final mel column: unbounded -- a forced sample still needs its features, slotsHeadroom governs as before).
    bool prime(int slot, const int* y, int n);
    // n of the prime in force on column `slot` (host state: until the step that generates local sample n - 1 has been issued); 0: none
    int primed(int slot) const { return inBatch(slot) && !m_primeN.empty() ? m_primeN[slot] : 0; }
    // ---- a column's state as a value (slots_state.hpp) ----
    // bytes of one column's state blob for this engine's shape and precision (header + its share of its tile's ring)
    size_t stateBytes() const { return slots_state_bytes(f.ringSlots, f.ringFragsPerSlot); }
    // The utterance of column `from` goes on in column `to` from the next step (queued; applied first in that step, so `from` may
    // take a new start in the same step): ring share, history and descriptors move, start unchanged.  The host's view changes at
    // once.  false (nothing changes): not in slot mode; an index outside the batch or from == to; `from` holds no utterance or has a
    // pending start or resume; `to` holds an utterance or has a pending start, resume or move; `from` is an endpoint of a pending
    // move.  A pending stop on `to` is superseded.
    bool move(int from, int to);
    // The state of column `slot` after the steps issued so far into dst (device memory, 16-byte aligned, slotStateBytes() bytes),
    // asynchronously on `stream` -- the stream of the session's steps, or one ordered after them.  The column goes on running.
    // Returns done, the local samples it has generated; -1 (nothing written): not in slot mode, slot outside the batch, no
    // utterance, a pending start, resume or move on the column, or a bad dst.
    int save(int slot, void* dst, hipStream_t stream = 0);
    // slotStart / slotStartMel, but the column continues from the blob `state` (of slotSave, device memory): at the next step its
    // ring share and history are loaded from it in place of the zeroing, and start = that step's counter - done; uid and done come
    // from the blob's header, which is read here with a small blocking copy on the null stream: the call waits for a save issued
    // on the null stream or on a stream that synchronises with it; a save on a non-blocking stream must have completed (or have
    // been ordered before this call by the caller) first.  The features / frames are those of the saved utterance, handed over again by the caller; `state` stays unchanged until
    // the next step has been issued (it reads it in stream order).  false (nothing changes): wrong magic or layout version, a shape
    // or precision that is not this engine's, done >= length (final mel: done >= frames x stride), or what slotStart / slotStartMel
    // refuse.
    bool resume(int slot, const void* state, const void* x, int precision, long long cStride, long long tStride, int length);
    bool resumeMel(int slot, const void* state, const void* mel, int precision, long long cStride, long long fStride, int frames, int final);
    // ---- lists of columns ----
    // slotSave for the n columns slots[0 .. n): blob i at dst + i * stride, ONE launch after one small staging copy, asynchronously on
    // `stream`; never synchronises the stream and waits for nothing already queued on it: the entries go through two staging
    // halves, each released by an event recorded behind its launch, so only a third list save in a row waits -- for the first to
    // have completed.  The first list save of a session allocates the halves (two small device and two pinned host buffers, once).  dst: 16-byte aligned device memory or pinned host memory (mapped as the outputs of slotsStepRagged);
    // stride: a multiple of 16, at least slotStateBytes().  saved[i] is filled before the call returns, from host state.  The columns
    // go on running.  Returns n; -1 with nothing written and nothing launched: not in slot mode, n outside 1..maxBatch, a slot out of
    // range or listed twice, a slot without an utterance or with a pending start, resume or move, a bad dst or stride.
    int saveList(const int* slots, int n, void* dst, long long stride, SlotSaved* saved, hipStream_t stream = 0);
    // slotResume / slotResumeMel for n requests at once, all or nothing: the blob of reqs[i] is states + i * stride (memory and stride
    // as for slotsSaveList).  The n headers are read at once -- device memory: one blocking 2-D copy on the null stream (the ordering
    // rule of slotResume); pinned memory: in place, so the save must have completed -- and checked as slotResume checks them; each
    // request is then refused for what slotResume / slotResumeMel refuse, and also when its column holds an utterance or has a
    // pending start or resume (a list never replaces one), or is named twice.  Any refusal: 0, and the session is exactly as before.
    // Otherwise n: every column has its pending resume, loaded by the next step in its one slot_load_kernel launch.  The blobs stay
    // unchanged until that step has been issued.
    int resumeList(const SlotResumeReq* reqs, int n, const void* states, long long stride);
    // The largest count the next step accepts: W, or the fewest samples a non-final mel column has frames for beyond its next
    // sample (0 when one has none).
    int headroom() const;
    // debug getter: the window's feature fragments of engine samples [first, first + count) -- within the last W generated -- in the
    // order of getFeatures (synchronises).  false: outside that range.
    bool getFeatures(void* dst, long long first, int count);
    // Order within a step (fixed): the pending moves (one launch); then the descriptor updates with the resets of started columns
    // (one launch) and the loads of resumed ones (one launch); then the feed.  A column that is the source of a move may therefore
    // take a new start in the same step.  A session that never moves or resumes launches what it launched before these existed.
    // One step of `count` <= W samples, asynchronously on `stream`: the pending starts and stops (one reset launch), the window feed
    // (one launch), the generation -- two launches where the window rows wrap -- up to the tile of the highest active column, the PCM
    // when pcm != NULL, and the copies of the step's samples / PCM into yOut / pcm ([maxBatch][count], host or device; NULL: none).
    // Columns without an utterance hold unspecified values.  Synchronises the stream when an output is host memory.  With mel columns
    // also their descriptor updates and their feed (slots_mel.hpp: three launches after the window feed); false (nothing changes)
    // when count exceeds slotsHeadroom().
    bool step(int count, int* yOut, short* pcm, hipStream_t stream = 0);
    // ---- ragged delivery (slots_deliver.hpp) ----
    // slotsStep, delivering pieces in place of rows, and never synchronising: the launches of slotsStep up to and including the
    // generation, then ONE slot_deliver_kernel launch that writes each piece's n samples at its offset of `samples` (int32) and / or
    // their PCM at the same offset of `pcm` (int16) -- device memory or pinned host memory, `capacity` elements each, NULL: not
    // wanted --, then an event record.  pieces[0 .. *nPieces) (host) is filled before anything is launched.  *ticket names the step
    // for slotsWait / slotsDone.  Returns the ragged size (end of the last piece; 0 when no column delivers); -2 when a launch
    // failed (the step was issued and has its ticket, but its outputs are not to be read: slotsStep returns false there); or -1 with
    // nothing changed: not in slot mode, count out of range or above the headroom, both outputs NULL, an output that is neither device
    // nor pinned memory, capacity or maxPieces too small.  Mixes freely with slotsStep.  (A step that reuses a ticket slot waits for
    // the step kSlotTickets before it: with at most that many steps in flight it waits for nothing.)
    long long stepRagged(int count, int* samples, short* pcm, long long capacity, SlotPiece* pieces, int maxPieces, int* nPieces,
                         unsigned long long* ticket, hipStream_t stream = 0);
    // Measurement only (scripts/slots_perf.py --serve): `reps` back-to-back output passes over the last `count` samples generated,
    // timed with events on `stream`; returns milliseconds for all of them, < 0 when refused.  ragged = false: what slotsStep
    // issues after the generation -- the PCM launches and the 2-D copies into samples / pcm [maxBatch][count]; ragged = true: the
    // delivery launch for every column holding an utterance (n = min(count, its samples so far)) into samples / pcm of `capacity`
    // elements.  Device or pinned outputs, both given.  Synchronises the device; changes nothing of the session.
    float timeOutputs(bool ragged, int count, int* samples, short* pcm, long long capacity, int reps, hipStream_t stream = 0);
    // Blocks until the outputs of the step with that ticket are complete (true), at once for a ticket older than the events kept;
    // false: no such ticket.
    bool wait(unsigned long long ticket);
    // 1: complete, 0: not yet, -1: no such ticket.  Never blocks.
    int done(unsigned long long ticket);
    // Leaves slot mode and frees its buffers (synchronises).  The rings it wrote are cleared by the next resetHistory, as after any run.
    void end();

private:
    const SlotFacts f;
    SlotHost& m_host;
    int m_largestD = 1;
    SamplingTable& m_temps;                 // the engine's (slots_sampler.hpp), shared with lockstep setTemperatures

    int m_slotW = 0;                        // window (samples); 0: not in slot mode
    long long m_slotCounter = 0;            // samples generated since slotsBegin: window row of the next step = counter mod W
    std::vector<SlotDesc> m_slotHost;       // the columns' descriptors as the host has set them ...
    std::vector<int> m_slotPending;         // ... and what the next step applies per column: 0 nothing, 1 start, 2 stop
    std::vector<int> m_slotPendingList;
    SlotDesc* m_slotDesc = NULL;            // [maxBatch] on the device
    char* m_slotFeat = NULL;                // [W][tiles][KFC] feature fragments
    float* m_slotSel = NULL;                // [W][maxBatch] selectors
    int* m_slotY = NULL;                    // [maxBatch][W] samples
    short* m_slotPcm = NULL;                // [maxBatch][W] int16 PCM
    char* m_slotUpd = NULL;                 // device copy of a step's updates + restarted columns
    StageRing m_slotStage;                  // pinned host staging of them: two halves, used by alternate steps
    const short* m_mulaw = NULL;            // the engine's PCM table
    // ... and its mel columns (slots_mel.hpp): utterances handed over as frames, upsampled step by step
    std::vector<MelDesc> m_melHost;         // the columns' mel descriptors as the host has set them (state 0: not a mel column) ...
    std::vector<char> m_melDirty;           // ... and the columns whose descriptor the next step writes
    std::vector<int> m_melDirtyList;
    int m_melColumns = 0;                   // columns with state != 0
    bool m_melTilesDirty = false;           // the tile list changes at the next step
    int m_melTiles = 0;                     // tiles in the device's list
    bool m_melPrepared = false;             // slots_mel_prepare done for this engine
    MelDesc* m_melDesc = NULL;              // [maxBatch] on the device (made by the first mel start of a session)
    char* m_melUpd = NULL;                  // device: a step's updates [maxBatch] + the list of tiles with mel columns [tiles]
    StageRing m_melStageHost;               // pinned host staging of them: two halves, as m_slotStage
    char* m_melStage = NULL;                // the step's frames in fragment order, [stage frames][mel tiles][KFC], then at m_melRecOff
    size_t m_melStageBytes = 0;             // the step's upsampled samples per column, [mel tiles * 16][count] of KFC KiB / 16
    size_t m_melRecOff = 0;                 // (bytes)
    int* m_melColInfo = NULL;               // [tiles * 16] int2: per column, phase of its first sample and samples it stores
    // ... and columns' states as values (slots_state.hpp): moved, saved, resumed
    std::vector<const void*> m_slotResume;  // per column: the blob its pending start resumes from (NULL: a new utterance) ...
    std::vector<int> m_slotResumeDone;      // ... and the local samples that blob has behind it (0: a new utterance)
    std::vector<char> m_slotMoveEnd;        // per column: 1 source, 2 destination of a pending move
    std::vector<SlotMove> m_slotMoves;      // the pending moves
    SlotLayer* m_slotLayers = NULL;         // the schedule per ring slot on the device (built by the first save or resume, kept)
    // ... and lists of columns saved in one launch: the entries' staging, made by the first list save
    SlotSave* m_saveDev = NULL;             // [2] x ([maxBatch] entries, then [maxBatch] SlotSaveCut) on the device, used by alternate list saves ...
    StageRing m_saveStage;                  // ... their pinned host staging: two halves
    std::vector<int> m_listMark;            // scratch of the list calls: per column, the index + 1 of the entry that names it
    // ... and ragged delivery (slots_deliver.hpp): a step's valid samples piece by piece, completion by ticket
    static constexpr int kSlotTickets = 4;  // events kept: a ticket older than that is complete (the stream is ordered)
    DeliverPiece* m_dlvDev = NULL;          // [maxBatch] on the device: the pieces of the step being delivered
    StageRing m_dlv;                        // pinned host staging of them, one per ticket in flight; its uses() is the last ticket
                                            // given out (they count from 1)
    // ... and the sampling temperatures (slots_sampler.hpp)
    std::vector<char> m_tempDirty;          // the columns whose table entry the next step writes
    std::vector<int> m_tempDirtyList;
    SlotScale* m_scaleDev = NULL;           // [4 maxBatch] on the device: a step's changed entries (made by the first step that needs it)
    StageRing m_scaleStage;                 // ... their pinned host staging: two halves
    // ... and the primes (slots_prime.hpp)
    std::vector<const int*> m_primeY;       // per column: the prime in force (made by the first prime of a session) ...
    std::vector<int> m_primeN;              // ... and its length (0: none)
    std::vector<char> m_primeListed;
    std::vector<int> m_primeList;           // the columns with one (and those that lost theirs since the last step)
    SlotPrime* m_primeDev = NULL;           // [maxBatch] on the device: the primed columns, m_primeDevN of them ...
    int m_primeDevN = 0;
    std::vector<SlotPrime> m_primeScratch;  // (the columns inside their prime in the step being issued, before they are staged)
    bool m_primeDirty = false;              // ... which the next step with a column inside its prime rewrites: the set has changed
    StageRing m_primeStage;                 // ... through pinned host staging: two halves

    size_t elemBytes() const { return f.f16 ? 2 : 4; }
    size_t featBytes(long long samples) const { return (size_t)samples * f.featRowElems * elemBytes(); }
    // a step's staging: the descriptor updates, the loads of resumed columns, the moves, the restarted columns -- [maxBatch] each
    size_t slotLoadOff() const { return (size_t)f.maxBatch * sizeof(SlotUpdate); }
    size_t slotMoveOff() const { return slotLoadOff() + (size_t)f.maxBatch * sizeof(SlotLoad); }
    size_t slotColOff() const { return slotMoveOff() + (size_t)f.maxBatch * sizeof(SlotMove); }
    size_t slotUpdBytes() const { return slotColOff() + (size_t)f.maxBatch * sizeof(int); }
    size_t melTileOff() const { return (size_t)f.maxBatch * sizeof(MelUpdate); }
    bool inBatch(int slot) const { return m_slotW > 0 && slot >= 0 && slot < f.maxBatch; }      // in slot mode, and a column of the batch
    bool slotHolds(int slot) const { return m_slotHost[slot].active || m_melHost[slot].state; }
    // The launches of a step up to and including the generation (the order above), shared by slotsStep and slotsStepRagged: the
    // columns they cover -> cols.  The counter is the caller's to advance.
    bool generate(int count, int& cols, hipStream_t stream);
    void copyRows(int t0, int c, int done, int count, int* yOut, short* pcm, hipStream_t stream);
    // the run of at most `left` window rows from sample counter t on that does not wrap: its first row -> row, returns its length
    int rowsFrom(long long t, int left, int& row) const {
        row = (int)(t % m_slotW);
        return left < m_slotW - row ? left : m_slotW - row;
    }
    int slotPieces(int count, SlotPiece* out, int maxOut, long long& total, int upStride) const;
    // what slotStart / slotStartMel refuse (shared with slotsResumeList, which checks every request before it changes anything)
    bool slotStartOk(int slot, const void* x, int precision, long long cStride, long long tStride, int length) const;
    bool slotStartMelOk(int slot, const void* mel, int precision, long long cStride, long long fStride, int frames, int final, int upStride) const;
    void* slotBlobRange(const void* base, int n, long long stride, bool* pinned) const;
    void slotDropResume(int slot) { m_slotResume[slot] = NULL; m_slotResumeDone[slot] = 0; }
    // start mod the largest dilation (every dilation divides it), non-negative: the rotation of a column's ring against its blob
    int slotRotation(long long start) const { return (int)((start % m_largestD + m_largestD) % m_largestD); }
    void slotTouchTile(int slot) { m_host.slotRingsDirty((slot >> 4) + 1); }
    const SlotLayer* slotLayers();
    bool slotStateHeader(const void* state, SlotStateHeader& h) const;
    bool slotApplyMoves(hipStream_t stream);
    void slotMarkPending(int slot, int what);
    bool slotApplyPending(hipStream_t stream);
    bool slotSamplingChange(int slot, const Sampling& s);      // (the public setters: checked)
    void slotSamplingSet(int slot, const Sampling& s);
    void slotSetResume(int slot, const void* state, const SlotStateHeader& h);
    bool slotApplyTemperatures(hipStream_t stream);
    void slotPrimeSet(int slot, const int* y, int n);
    bool slotApplyPrimes(int count, bool& forced, hipStream_t stream);
    void melMarkDirty(int slot);
    void slotDropMel(int slot);
    void melAllocate();
    char* melStage(int count, const SlotLive& v);
    bool melApplyPending(hipStream_t stream);
};

}  // namespace wn
