// wavenet_capi.hip -- the C-ABI surface of libwavenet_infer.so:
//   include/wavenet_infer.h  (the reference's pytorch/wavenet_infer.h, symbol for symbol)
//   include/nv_wavenet_c.h   (handle API over every instantiation built into the library)
#include <stdlib.h>

#include <vector>

#include "../../include/wavenet_infer.h"
#include "engine_base.hpp"

// ---- registry of instantiations (WN_INSTANCES comes from the Makefile) ----------------------
#define X(R, S, A, P) nvw_engine* WN_FACTORY_NAME(R, S, A, P)(int, int, int, int, int, int, int);
WN_INSTANCES
#undef X

namespace {
struct Entry { int R, S, A, P; nvw_factory_fn make; };
#define X(R, S, A, P) {R, S, A, P, WN_FACTORY_NAME(R, S, A, P)},
const Entry kEntries[] = {WN_INSTANCES};
#undef X
const int kNumEntries = sizeof(kEntries) / sizeof(kEntries[0]);

const Entry* findEntry(int R, int S, int A, int P) {
    for (int i = 0; i < kNumEntries; i++)
        if (kEntries[i].R == R && kEntries[i].S == S && kEntries[i].A == A && kEntries[i].P == P) return &kEntries[i];
    return NULL;
}
}  // namespace

extern "C" {

int nvw_abi_version(void) { return NVW_ABI_VERSION; }
int nvw_supported(int R, int S, int A, int precision) { return findEntry(R, S, A, precision) != NULL; }

int nvw_list_supported(int* out, int max) {
    for (int i = 0; i < kNumEntries && i < max; i++) {
        out[4 * i] = kEntries[i].R; out[4 * i + 1] = kEntries[i].S;
        out[4 * i + 2] = kEntries[i].A; out[4 * i + 3] = kEntries[i].P;
    }
    return kNumEntries;
}

nvw_engine* nvw_create_ex(int R, int S, int A, int precision, int num_layers, int max_dilation, int batch_size,
                          int num_samples, int implementation, int tanh_embed, int organisation) {
    const Entry* e = findEntry(R, S, A, precision);
    if (!e) {
        fprintf(stderr, "nvw_create: no nvWavenetInfer instantiation for R=%d S=%d A=%d fp%d in this build\n", R, S, A,
                precision);
        return NULL;
    }
    if (implementation < 0 || implementation > 4) {
        fprintf(stderr, "nvw_create: implementation %d out of range 0..4\n", implementation);
        return NULL;
    }
    if (organisation < NVW_ORG_AUTO || organisation > NVW_ORG_LAST || (organisation >= NVW_ORG_RETIRED7 && organisation <= NVW_ORG_RETIRED9)) {
        fprintf(stderr, "nvw_create: organisation %d out of range 0..%d\n", organisation, (int)NVW_ORG_LAST);
        return NULL;
    }
    // (the class asserts these: refused here, before any HIP call, so that a host process gets a NULL instead of an abort --
    //  and, built with NDEBUG, instead of a schedule written past Params::dil)
    if (num_layers < 2 || num_layers > wn::kMaxLayers || max_dilation < 1 || batch_size < 1 || num_samples < 1) {
        fprintf(stderr, "nvw_create: refused (%d layers, 2..%d supported; maxDilation %d, batch %d and %d samples, each >= 1)\n", num_layers,
                (int)wn::kMaxLayers, max_dilation, batch_size, num_samples);
        return NULL;
    }
    nvw_engine* w = e->make(num_layers, max_dilation, batch_size, num_samples, implementation, tanh_embed, organisation);
    if (w && !w->supported()) {   // the shape does not fit a CU in this organisation (message already printed)
        delete w;
        return NULL;
    }
    return w;
}
nvw_engine* nvw_create(int R, int S, int A, int precision, int num_layers, int max_dilation, int batch_size,
                       int num_samples, int implementation, int tanh_embed) {
    return nvw_create_ex(R, S, A, precision, num_layers, max_dilation, batch_size, num_samples, implementation, tanh_embed,
                         NVW_ORG_AUTO);
}
void nvw_destroy(nvw_engine* e) { delete e; }

void nvw_set_embeddings(nvw_engine* e, float* p, float* c) { e->setEmbeddings(p, c); }
void nvw_set_layer_weights(nvw_engine* e, int layer, float* Wprev, float* Wcur, float* Bh, float* Wres, float* Bres,
                           float* Wskip, float* Bskip) {
    e->setLayerWeights(layer, Wprev, Wcur, Bh, Wres, Bres, Wskip, Bskip);
}
void nvw_set_out_weights(nvw_engine* e, float* Wzs, float* Bzs, float* Wza, float* Bza) {
    e->setOutWeights(Wzs, Bzs, Wza, Bza);
}
void nvw_set_inputs(nvw_engine* e, float* Lh, float* sel) { e->setInputs(Lh, sel, e->maxSamples()); }
void nvw_set_inputs_n(nvw_engine* e, float* Lh, float* sel, int num_samples) { e->setInputs(Lh, sel, num_samples); }
void nvw_set_conditioning(nvw_engine* e, float* Lh) { e->setConditioning(Lh, e->maxSamples()); }
void nvw_set_conditioning_n(nvw_engine* e, float* Lh, int num_samples) { e->setConditioning(Lh, num_samples); }
void nvw_pack_conditioning(nvw_engine* e, float* Lh, int first_sample, int count, void* stream) {
    e->packConditioning(Lh, first_sample, count, (hipStream_t)stream);
}
void nvw_set_conditioning_direct(nvw_engine* e, float* Lh, int num_samples) { e->setConditioningDirect(Lh, num_samples, 32); }
int nvw_set_conditioning_direct_t(nvw_engine* e, const void* Lh, int num_samples, int precision) {
    if (precision != 32 && !(precision == 16 && e->precisionBits() == 16)) {
        fprintf(stderr, "nvw_set_conditioning_direct_t: a %d-bit tensor cannot be read in place by an fp%d engine\n", precision,
                e->precisionBits());
        return 0;
    }
    if (precision == 16) {      // (a host tensor can only take the packing path, which reads fp32)
        if (!wn::is_device_ptr(Lh)) {
            fprintf(stderr, "nvw_set_conditioning_direct_t: an fp16 tensor must be device memory to be read in place\n");
            return 0;
        }
    }
    e->setConditioningDirect(Lh, num_samples, precision);
    return 1;
}
void nvw_set_conditioning_packed(nvw_engine* e, const void* frags, int num_samples) { e->setConditioningPacked(frags, num_samples); }
int nvw_set_conditioning_packed_n(nvw_engine* e, const void* frags, int num_samples, size_t elems) {
    if (num_samples <= 0 || elems < e->condPackedElems(num_samples)) {
        fprintf(stderr, "nvw_set_conditioning_packed_n: %zu elements cannot hold %d samples (+1) in this engine's fragment order (%zu needed)\n",
                elems, num_samples, num_samples > 0 ? e->condPackedElems(num_samples) : (size_t)0);
        return 0;
    }
    e->setConditioningPacked(frags, num_samples);
    return 1;
}
int nvw_cond_tiles(nvw_engine* e) { return e->condTiles(); }
// ---- conditioning computed in the generation kernel from the upsampled features ------------------------------------------------
int nvw_max_cond_channels(void) { return wn::kCondChannelsMax; }
int nvw_set_conditioning_weights(nvw_engine* e, const float* Wcond, const float* bcond, int n_cond) {
    if (!e->setConditioningWeights(Wcond, bcond, n_cond)) {
        fprintf(stderr, "nvw_set_conditioning_weights: %d feature channels; the kernels are built for 1..%d (use the Lh path)\n", n_cond,
                wn::kCondChannelsMax);
        return 0;
    }
    return 1;
}
int nvw_feature_fragments(nvw_engine* e) { return e->featureFragments(); }
size_t nvw_feature_elems(nvw_engine* e, int num_samples) { return e->featureElems(num_samples); }
static bool featArgsOk(nvw_engine* e, const char* who, const void* p, int first, int count) {
    if (e->conditioningChannels() <= 0) {
        fprintf(stderr, "%s: call nvw_set_conditioning_weights first\n", who);
        return false;
    }
    if (!wn::is_device_ptr(p)) {
        fprintf(stderr, "%s: the features must be device memory\n", who);
        return false;
    }
    if (first < 0 || count <= 0 || first + count > e->maxSamples()) {
        fprintf(stderr, "%s: samples [%d, %d) outside the engine's %d\n", who, first, first + count, e->maxSamples());
        return false;
    }
    return true;
}
int nvw_set_conditioning_features(nvw_engine* e, const void* frags, int num_samples, size_t elems) {
    if (!featArgsOk(e, "nvw_set_conditioning_features", frags, 0, num_samples)) return 0;
    if (elems < e->featureElems(num_samples)) {
        fprintf(stderr, "nvw_set_conditioning_features: %zu elements cannot hold %d samples of feature fragments (%zu needed)\n", elems,
                num_samples, e->featureElems(num_samples));
        return 0;
    }
    e->setConditioningFeatures(frags, num_samples);
    return 1;
}
int nvw_pack_features(nvw_engine* e, const void* x, int precision, long long b_stride, long long c_stride, long long t_stride,
                      int first_sample, int count, void* stream) {
    if (!featArgsOk(e, "nvw_pack_features", x, first_sample, count) || (precision != 32 && precision != 16)) return 0;
    e->packFeatures(x, precision, b_stride, c_stride, t_stride, first_sample, count, (hipStream_t)stream);
    return 1;
}
int nvw_set_upsampling(nvw_engine* e, const float* up_w, const float* up_b, int window, int stride) {
    if (!e->setUpsampling(up_w, up_b, window, stride)) {
        fprintf(stderr, "nvw_set_upsampling: window %d / stride %d (a multiple of the stride, at most 5 strides; nvw_set_conditioning_weights first)\n",
                window, stride);
        return 0;
    }
    return 1;
}
int nvw_set_mel(nvw_engine* e, const void* mel, int precision, long long b_stride, long long c_stride, long long f_stride, int frames) {
    const int stride = e->upsamplingStride();
    if (stride <= 0 || !wn::is_device_ptr(mel) || (precision != 32 && precision != 16) || frames <= 0 || (long long)frames * stride > e->maxSamples()) {
        fprintf(stderr, "nvw_set_mel: refused (nvw_set_upsampling first; device memory; 16- or 32-bit floats; frames * stride <= the engine's %d samples)\n",
                e->maxSamples());
        return 0;
    }
    e->setMel(mel, precision, b_stride, c_stride, f_stride, frames);
    return 1;
}
int nvw_upsample_features(nvw_engine* e, int first_sample, int count, void* stream) {
    if (e->upsamplingStride() <= 0 || e->melSamples() <= 0) {
        fprintf(stderr, "nvw_upsample_features: refused (nvw_set_upsampling and nvw_set_mel first)\n");
        return 0;
    }
    if (first_sample < 0 || count <= 0 || (long long)first_sample + count > e->melSamples()) {
        fprintf(stderr, "nvw_upsample_features: samples [%d, %lld) outside the %d the mel frames upsample to\n", first_sample,
                (long long)first_sample + count, e->melSamples());
        return 0;
    }
    e->upsampleFeatures(first_sample, count, (hipStream_t)stream);
    return 1;
}
int nvw_get_features(nvw_engine* e, void* dst, int first_sample, int count) {
    if (!e->hasFeatureBuffer() || dst == NULL || first_sample < 0 || count <= 0 || (long long)first_sample + count > e->maxSamples()) {
        fprintf(stderr, "nvw_get_features: refused (no features packed or upsampled by this engine yet, or samples [%d, %lld) outside its %d)\n",
                first_sample, (long long)first_sample + count, e->maxSamples());
        return 0;
    }
    e->getFeatures(dst, first_sample, count);
    return 1;
}
int nvw_generate_stream(nvw_engine* e, int num_samples_per_chunk, nvw_consume_fn consume, void* user, int num_samples, int batch_size, int* yOut,
                        void* stream) {
    if (e->upsamplingStride() <= 0 || e->melSamples() <= 0) {
        fprintf(stderr, "nvw_generate_stream: refused (nvw_set_upsampling and nvw_set_mel first)\n");
        return 0;
    }
    if (num_samples_per_chunk <= 0 || num_samples <= 0 || num_samples > e->melSamples() || num_samples > e->maxSamples()) {
        fprintf(stderr, "nvw_generate_stream: %d samples in chunks of %d: the mel frames upsample to %d, the engine holds %d\n", num_samples,
                num_samples_per_chunk, e->melSamples(), e->maxSamples());
        return 0;
    }
    if (batch_size <= 0 || batch_size > e->maxBatch()) {
        fprintf(stderr, "nvw_generate_stream: batch %d outside 1..%d\n", batch_size, e->maxBatch());
        return 0;
    }
    return e->run_stream(num_samples_per_chunk, consume, user, num_samples, batch_size, yOut, (hipStream_t)stream) ? 1 : 0;
}
int nvw_set_features(nvw_engine* e, const void* x, int precision, long long b_stride, long long c_stride, long long t_stride,
                     int num_samples) {
    if (!featArgsOk(e, "nvw_set_features", x, 0, num_samples) || (precision != 32 && precision != 16)) return 0;
    e->setFeatures(x, precision, b_stride, c_stride, t_stride, num_samples);
    return 1;
}
void nvw_set_selectors(nvw_engine* e, float* sel, int num_samples) { e->setSelectors(sel, num_samples); }
unsigned nvw_chain_status(nvw_engine* e) { return e->chainStatus(); }
unsigned nvw_chain_fallbacks(nvw_engine* e) { return e->chainFallbacks(); }
unsigned nvw_chain_last_timeout(nvw_engine* e) { return e->chainLastTimeout(); }
void nvw_set_chain_timeout_ms(nvw_engine* e, double ms) { e->setChainTimeoutMs(ms); }
void nvw_set_clock_probe(nvw_engine* e, int on) { e->setClockProbe(on != 0); }
void nvw_set_ring_in_lds(nvw_engine* e, int mode) { e->setRingInLds(mode); }
void nvw_set_compiled_schedule(nvw_engine* e, int mode) { e->setCompiledSchedule(mode); }
double nvw_last_launch_clock_ghz(nvw_engine* e) { return e->lastLaunchClockGHz(); }
int nvw_run_range(nvw_engine* e, int init_sample, int count, int num_samples, int batch_size, void* stream) {
    return e->run_range(init_sample, count, num_samples, batch_size, (hipStream_t)stream) ? 1 : 0;
}
void nvw_reset_history(nvw_engine* e, void* stream) { e->resetHistory((hipStream_t)stream); }
void nvw_set_selector_seed(nvw_engine* e, unsigned long long seed) { e->setSelectorSeed(seed); }
void nvw_set_audio_out(nvw_engine* e, short* pcmOut) { e->setAudioOut(pcmOut, 0); }
void nvw_set_audio_out_n(nvw_engine* e, short* pcmOut, size_t elems) { e->setAudioOut(pcmOut, elems); }
void nvw_kernel_info(nvw_engine* e, int batch_size, int dump_activations, char* buf, int buf_size) {
    e->kernelInfo(batch_size, dump_activations != 0, buf, buf_size);
}

int nvw_run(nvw_engine* e, int num_samples, int batch_size, int* yOut, int bspb, int dump, void* stream) {
    return e->run(num_samples, batch_size, yOut, bspb, dump != 0, (hipStream_t)stream) ? 1 : 0;
}
int nvw_run_partial(nvw_engine* e, int init_sample, int num_samples, int batch_size, int* yOut, int bspb, int dump,
                    void* stream) {
    return e->run_partial(init_sample, num_samples, batch_size, yOut, bspb, dump != 0, (hipStream_t)stream) ? 1 : 0;
}
int nvw_run_chunks(nvw_engine* e, int chunk, nvw_consume_fn consume, void* user, int num_samples, int batch_size,
                   int* yOut, int bspb, int dump, void* stream) {
    return e->run_chunks(chunk, consume, user, num_samples, batch_size, yOut, bspb, dump != 0, (hipStream_t)stream) ? 1
                                                                                                                   : 0;
}

void nvw_get_xt_out(nvw_engine* e, int layer, float* d) { e->getXtOut(layer, d); }
void nvw_get_skip_out(nvw_engine* e, int layer, float* d) { e->getSkipOut(layer, d); }
void nvw_get_zs(nvw_engine* e, float* d) { e->getZs(d); }
void nvw_get_za(nvw_engine* e, float* d) { e->getZa(d); }
void nvw_get_p(nvw_engine* e, float* d) { e->getP(d); }
void nvw_get_y_out(nvw_engine* e, int* yOut, int offset, int size, void* stream) {
    e->getYOut(yOut, offset, size, (hipStream_t)stream);
}

// ---- slot mode: continuous batching (ABI 7) --------------------------------------------------------------------------------------
int nvw_slots_begin(nvw_engine* e, int window) {
    if (e->conditioningChannels() <= 0) {
        fprintf(stderr, "nvw_slots_begin: call nvw_set_conditioning_weights first\n");
        return 0;
    }
    if (e->slots().begin(window)) return 1;
    fprintf(stderr, "nvw_slots_begin: window %d is not a positive multiple of the largest dilation\n", window);
    return 0;
}
int nvw_slot_start(nvw_engine* e, int slot, const void* x, int precision, long long c_stride, long long t_stride, int length,
                   unsigned uid) {
    if (e->slots().start(slot, x, precision, c_stride, t_stride, length, uid)) return 1;
    fprintf(stderr, "nvw_slot_start: refused (nvw_slots_begin first; slot %d of %d; device features of 16 or 32 bits; strides %lld, %lld "
            "and length %d positive)\n", slot, e->maxBatch(), c_stride, t_stride, length);
    return 0;
}
int nvw_slot_stop(nvw_engine* e, int slot) {
    if (e->slots().stop(slot)) return 1;
    fprintf(stderr, "nvw_slot_stop: refused (nvw_slots_begin first; slot %d of %d)\n", slot, e->maxBatch());
    return 0;
}
int nvw_slots_step(nvw_engine* e, int count, int* yOut, short* pcm, void* stream) {
    return e->slots().step(count, yOut, pcm, (hipStream_t)stream) ? 1 : 0;
}
void nvw_slots_end(nvw_engine* e) { e->slots().end(); }
// ---- slot mode from mel frames (additive within ABI 7) ---------------------------------------------------------------------------
int nvw_slot_start_mel(nvw_engine* e, int slot, const void* mel, int precision, long long c_stride, long long f_stride, int frames,
                       int final, unsigned uid) {
    if (e->slots().startMel(slot, mel, precision, c_stride, f_stride, frames, final, uid)) return 1;
    fprintf(stderr, "nvw_slot_start_mel: refused (nvw_slots_begin and nvw_set_upsampling first; slot %d of %d; device frames of 16 or 32 "
            "bits; strides %lld, %lld positive; frames %d >= 0, > 0 when final)\n", slot, e->maxBatch(), c_stride, f_stride, frames);
    return 0;
}
int nvw_slot_mel_frames(nvw_engine* e, int slot, int frames, int final) {
    if (e->slots().melFrames(slot, frames, final)) return 1;
    fprintf(stderr, "nvw_slot_mel_frames: refused (slot %d of %d: not a running mel column, already final, or %d frames is fewer than "
            "before)\n", slot, e->maxBatch(), frames);
    return 0;
}
int nvw_slots_headroom(nvw_engine* e) { return e->slots().headroom(); }
int nvw_slots_get_features(nvw_engine* e, void* dst, long long first_sample, int count) {
    if (e->slots().getFeatures(dst, first_sample, count)) return 1;
    fprintf(stderr, "nvw_slots_get_features: refused (samples [%lld, %lld) are not among the last window of samples generated)\n",
            first_sample, first_sample + count);
    return 0;
}
// ---- slot mode: a column's state as a value (additive within ABI 7) --------------------------------------------------------------
size_t nvw_slot_state_bytes(nvw_engine* e) { return e->slots().stateBytes(); }
int nvw_slot_move(nvw_engine* e, int from, int to) {
    if (e->slots().move(from, to)) return 1;
    fprintf(stderr, "nvw_slot_move: refused (nvw_slots_begin first; %d -> %d of %d columns: a running column without a pending start, "
            "resume or move into an idle one without them)\n", from, to, e->maxBatch());
    return 0;
}
int nvw_slot_save(nvw_engine* e, int slot, void* dst, void* stream) {
    const int done = e->slots().save(slot, dst, (hipStream_t)stream);
    if (done < 0)
        fprintf(stderr, "nvw_slot_save: refused (nvw_slots_begin first; slot %d of %d: a running column without a pending start, resume or "
                "move; dst 16-byte aligned device memory)\n", slot, e->maxBatch());
    return done;
}
int nvw_slot_resume(nvw_engine* e, int slot, const void* state, const void* x, int precision, long long c_stride, long long t_stride,
                    int length) {
    if (e->slots().resume(slot, state, x, precision, c_stride, t_stride, length)) return 1;
    fprintf(stderr, "nvw_slot_resume: refused (a state of nvw_slot_save for this shape and precision with fewer than %d samples done, "
            "device memory; otherwise as nvw_slot_start: slot %d of %d)\n", length, slot, e->maxBatch());
    return 0;
}
int nvw_slot_resume_mel(nvw_engine* e, int slot, const void* state, const void* mel, int precision, long long c_stride,
                        long long f_stride, int frames, int final) {
    if (e->slots().resumeMel(slot, state, mel, precision, c_stride, f_stride, frames, final)) return 1;
    fprintf(stderr, "nvw_slot_resume_mel: refused (a state of nvw_slot_save for this shape and precision, device memory, with fewer "
            "samples done than %d final frames hold; otherwise as nvw_slot_start_mel: slot %d of %d)\n", frames, slot, e->maxBatch());
    return 0;
}
// ---- slot mode: lists of columns saved and resumed (additive within ABI 7) --------------------------------------------------------
int nvw_slots_save_list(nvw_engine* e, const int* slots, int n, void* dst, long long stride, nvw_slot_saved* saved, void* stream) {
    const int got = e->slots().saveList(slots, n, dst, stride, (wn::SlotSaved*)saved, (hipStream_t)stream);
    if (got < 0)
        fprintf(stderr, "nvw_slots_save_list: refused (nvw_slots_begin first; %d slots of %d, each once: running columns without a pending "
                "start, resume or move; dst 16-byte aligned device or pinned memory; stride %lld a multiple of 16, at least %zu)\n", n,
                e->maxBatch(), stride, e->slots().stateBytes());
    return got;
}
int nvw_slots_resume_list(nvw_engine* e, const nvw_slot_resume_req* reqs, int n, const void* states, long long stride) {
    const int got = e->slots().resumeList((const wn::SlotResumeReq*)reqs, n, states, stride);
    if (got != n || n < 1)
        fprintf(stderr, "nvw_slots_resume_list: refused, nothing changed (%d requests of %d columns, each column once, idle and without a "
                "pending start; states of nvw_slot_save / nvw_slots_save_list for this shape and precision in device or pinned memory, "
                "stride %lld a multiple of 16, at least %zu; otherwise as nvw_slot_resume / nvw_slot_resume_mel)\n", n, e->maxBatch(),
                stride, e->slots().stateBytes());
    return got;
}
// ---- sampling temperature per utterance, lockstep and in slot mode (additive within ABI 7) ---------------------------------------
int nvw_set_temperatures(nvw_engine* e, const float* T, int n) {
    if (e->setTemperatures(T, n)) return 1;
    fprintf(stderr, "nvw_set_temperatures: refused, nothing changed (not in slot mode; %d values for %d columns; every value finite and in "
            "[2^-10, 2^10])\n", n, e->maxBatch());
    return 0;
}
int nvw_slot_set_temperature(nvw_engine* e, int slot, float T) {
    if (e->slots().setTemperature(slot, T)) return 1;
    fprintf(stderr, "nvw_slot_set_temperature: refused, nothing changed (nvw_slots_begin first; slot %d of %d: a column with an utterance or "
            "a pending start or resume; T = %g finite and in [2^-10, 2^10])\n", slot, e->maxBatch(), (double)T);
    return 0;
}
float nvw_slot_temperature(nvw_engine* e, int slot) { return e->slots().temperature(slot); }
// ---- probability floor (min-p) per utterance, lockstep and in slot mode (additive within ABI 7) -----------------------------------
int nvw_set_min_p(nvw_engine* e, const float* p, int n) {
    if (e->setMinP(p, n)) return 1;
    fprintf(stderr, "nvw_set_min_p: refused, nothing changed (not in slot mode; %d values for %d columns; every value finite and in "
            "[0, 0.5])\n", n, e->maxBatch());
    return 0;
}
int nvw_slot_set_min_p(nvw_engine* e, int slot, float p) {
    if (e->slots().setMinP(slot, p)) return 1;
    fprintf(stderr, "nvw_slot_set_min_p: refused, nothing changed (nvw_slots_begin first; slot %d of %d: a column with an utterance or "
            "a pending start or resume; p = %g finite and in [0, 0.5])\n", slot, e->maxBatch(), (double)p);
    return 0;
}
float nvw_slot_min_p(nvw_engine* e, int slot) { return e->slots().minP(slot); }
// ---- tail cuts (top-k, top-p) per utterance, lockstep and in slot mode (additive within ABI 7) -------------------------------------
int nvw_set_top_k(nvw_engine* e, const int* k, int n) {
    if (e->setTopK(k, n)) return 1;
    fprintf(stderr, "nvw_set_top_k: refused, nothing changed (not in slot mode; %d values for %d columns; every value in [0, A])\n", n,
            e->maxBatch());
    return 0;
}
int nvw_set_top_p(nvw_engine* e, const float* p, int n) {
    if (e->setTopP(p, n)) return 1;
    fprintf(stderr, "nvw_set_top_p: refused, nothing changed (not in slot mode; %d values for %d columns; every value finite and in "
            "(0, 1])\n", n, e->maxBatch());
    return 0;
}
int nvw_slot_set_top_k(nvw_engine* e, int slot, int k) {
    if (e->slots().setTopK(slot, k)) return 1;
    fprintf(stderr, "nvw_slot_set_top_k: refused, nothing changed (nvw_slots_begin first; slot %d of %d: a column with an utterance or "
            "a pending start or resume; k = %d in [0, A])\n", slot, e->maxBatch(), k);
    return 0;
}
int nvw_slot_set_top_p(nvw_engine* e, int slot, float p) {
    if (e->slots().setTopP(slot, p)) return 1;
    fprintf(stderr, "nvw_slot_set_top_p: refused, nothing changed (nvw_slots_begin first; slot %d of %d: a column with an utterance or "
            "a pending start or resume; p = %g finite and in (0, 1])\n", slot, e->maxBatch(), (double)p);
    return 0;
}
int nvw_slot_top_k(nvw_engine* e, int slot) { return e->slots().topK(slot); }
float nvw_slot_top_p(nvw_engine* e, int slot) { return e->slots().topP(slot); }
int nvw_sampler_mask(nvw_engine* e) { return e->samplerMask(); }
// ---- primed generation: forced sample prefixes, lockstep and in slot mode (additive within ABI 7) -----------------------------------
int nvw_set_prime(nvw_engine* e, const int* y, const int* n, int batch, int max_n, long long stride) {
    if (e->setPrime(y, n, batch, max_n, stride)) return 1;
    fprintf(stderr, "nvw_set_prime: refused, nothing changed (not in slot mode; batch %d of 1 .. %d; every n[b] in 0 .. max_n = %d, max_n "
            "within the engine's samples, stride %lld >= max_n; host values in 0 .. A-1)\n", batch, e->maxBatch(), max_n, stride);
    return 0;
}
int nvw_slot_prime(nvw_engine* e, int slot, const int* y, int n) {
    if (e->slots().prime(slot, y, n)) return 1;
    fprintf(stderr, "nvw_slot_prime: refused, nothing changed (nvw_slots_begin first; slot %d of %d: a column with a pending start or "
            "resume; y in device memory; n = %d in 1 .. the utterance's length)\n", slot, e->maxBatch(), n);
    return 0;
}
int nvw_slot_primed(nvw_engine* e, int slot) { return e->slots().primed(slot); }
// ---- prefill: a prime's state blob from a time-parallel pass (additive within ABI 7) -----------------------------------------------
int nvw_prefill_window(nvw_engine* e) { return e->prefillWindow(); }
int nvw_prefill_states(nvw_engine* e, const nvw_prefill_req* reqs, int count, void* dst, long long stride, void* stream) {
    const int got = e->prefillStates((const wn::PrefillReq*)reqs, count, dst, stride, (hipStream_t)stream);
    if (got != count || count < 1)
        fprintf(stderr, "nvw_prefill_states: refused, nothing written (nvw_set_conditioning_weights first; %d requests of 1 .. 65535; every n "
                ">= 1, y and x in device memory, precision 32 or 16, positive strides, temperature in [2^-10, 2^10]; dst 16-byte aligned "
                "device or pinned memory, stride %lld a multiple of 16, at least %zu)\n", count, stride, e->slots().stateBytes());
    return got;
}
// ---- scoring: per-sample log-likelihoods from a time-parallel pass (additive within ABI 7) ------------------------------------------
int nvw_score_max_samples(nvw_engine* e) { return e->scoreMaxSamples(); }
int nvw_score_samples(nvw_engine* e, const nvw_score_req* reqs, int count, void* stream) {
    const int got = e->scoreSamples((const wn::ScoreReq*)reqs, count, (hipStream_t)stream);
    if (got != count || count < 1)
        fprintf(stderr, "nvw_score_samples: refused, nothing written (nvw_set_conditioning_weights first; %d requests of 1 .. 65535; every n "
                ">= 1, y and x in device memory, precision 32 or 16, positive strides, temperature in [2^-10, 2^10]; logp device or pinned "
                "memory, rows NULL or 16-byte aligned device memory; at most %d samples, each n rounded up to 16)\n", count,
                e->scoreMaxSamples());
    return got;
}
// ---- prefill and scoring from mel frames: a time-parallel upsampling pass (additive within ABI 7) -----------------------------------
int nvw_upsample_row_elems(nvw_engine* e) { return e->upsampleRowElems(); }
int nvw_upsample_requests(nvw_engine* e, const nvw_upsample_req* reqs, int count, void* stream) {
    const int got = e->upsampleRequests((const wn::MelTimeReq*)reqs, count, (hipStream_t)stream);
    if (got != count || count < 1)
        fprintf(stderr, "nvw_upsample_requests: refused, nothing written (nvw_set_upsampling first; %d requests of 1 .. 65535; mel in device "
                "memory, precision 32 or 16, positive strides, first_sample >= 0, count >= 1, frames * stride covering the range; dst 16-byte "
                "aligned device memory)\n", count);
    return got;
}
int nvw_prefill_states_mel(nvw_engine* e, const nvw_prefill_mel_req* reqs, int count, void* dst, long long stride, void* stream) {
    const int got = e->prefillStatesMel((const wn::PrefillMelReq*)reqs, count, dst, stride, (hipStream_t)stream);
    if (got != count || count < 1)
        fprintf(stderr, "nvw_prefill_states_mel: refused, nothing written (nvw_set_conditioning_weights and nvw_set_upsampling first; %d "
                "requests of 1 .. 65535; every n >= 1, y and mel in device memory, precision 32 or 16, positive strides, frames * stride >= n, "
                "temperature in [2^-10, 2^10]; dst 16-byte aligned device or pinned memory, stride %lld a multiple of 16, at least %zu)\n",
                count, stride, e->slots().stateBytes());
    return got;
}
int nvw_score_samples_mel(nvw_engine* e, const nvw_score_mel_req* reqs, int count, void* stream) {
    const int got = e->scoreSamplesMel((const wn::ScoreMelReq*)reqs, count, (hipStream_t)stream);
    if (got != count || count < 1)
        fprintf(stderr, "nvw_score_samples_mel: refused, nothing written (nvw_set_conditioning_weights and nvw_set_upsampling first; %d "
                "requests of 1 .. 65535; every n >= 1, y and mel in device memory, precision 32 or 16, positive strides, frames * stride >= n, "
                "temperature in [2^-10, 2^10]; logp device or pinned memory, rows NULL or 16-byte aligned device memory; at most %d samples, "
                "each n rounded up to 16)\n", count, e->scoreMaxSamples());
    return got;
}
// ---- scoring with carried state: time chunks, from and to a state blob (additive within ABI 7) --------------------------------------
int nvw_score_chunks(nvw_engine* e, const nvw_score_chunk_req* reqs, int count, void* stream) {
    const int got = e->scoreChunks((const wn::ScoreChunkReq*)reqs, count, (hipStream_t)stream);
    if (got != count || count < 1)
        fprintf(stderr, "nvw_score_chunks: refused, nothing written (as nvw_score_samples, at most %d samples, each n rounded up to 16; state "
                "NULL or a blob of this engine's shape, precision and layout in 16-byte aligned device or pinned memory, done + n <= INT_MAX "
                "- 16; state_out NULL or %zu bytes of 16-byte aligned device or pinned memory that overlap no state and no other state_out "
                "of the %d requests)\n", e->scoreMaxSamples(), e->slots().stateBytes(), count);
    return got;
}
int nvw_score_chunks_mel(nvw_engine* e, const nvw_score_chunk_mel_req* reqs, int count, void* stream) {
    const int got = e->scoreChunksMel((const wn::ScoreChunkMelReq*)reqs, count, (hipStream_t)stream);
    if (got != count || count < 1)
        fprintf(stderr, "nvw_score_chunks_mel: refused, nothing written (as nvw_score_samples_mel and nvw_score_chunks: %d requests, frames * "
                "stride >= done + n, states and state_out of %zu bytes)\n", count, e->slots().stateBytes());
    return got;
}
// ---- slot mode: ragged delivery, steps that never block (additive within ABI 7) ---------------------------------------------------
long long nvw_slots_step_ragged(nvw_engine* e, int count, int* samples, short* pcm, long long capacity, nvw_slot_piece* pieces,
                                int max_pieces, int* n_pieces, unsigned long long* ticket, void* stream) {
    return e->slots().stepRagged(count, samples, pcm, capacity, (wn::SlotPiece*)pieces, max_pieces, n_pieces, ticket, (hipStream_t)stream);
}
float nvw_slots_time_outputs(nvw_engine* e, int ragged, int count, int* samples, short* pcm, long long capacity, int reps, void* stream) {
    return e->slots().timeOutputs(ragged != 0, count, samples, pcm, capacity, reps, (hipStream_t)stream);
}
int nvw_slots_wait(nvw_engine* e, unsigned long long ticket) { return e->slots().wait(ticket) ? 1 : 0; }
int nvw_slots_done(nvw_engine* e, unsigned long long ticket) { return e->slots().done(ticket) > 0 ? 1 : 0; }
void* nvw_pinned_alloc(size_t bytes) {
    void* p = NULL;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return NULL;
    }
    return p;
}
void nvw_pinned_free(void* p) {
    if (p) gpuErrChk(hipHostFree(p));
}

void nvw_device_synchronize(void) { gpuErrChk(hipDeviceSynchronize()); }

float nvw_time_runs(nvw_engine* e, int reps, int num_samples, int batch_size, int bspb, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t t0, t1;
    gpuErrChk(hipEventCreate(&t0));
    gpuErrChk(hipEventCreate(&t1));
    gpuErrChk(hipEventRecord(t0, s));
    for (int i = 0; i < reps; i++) e->run(num_samples, batch_size, NULL, bspb, false, s);
    gpuErrChk(hipEventRecord(t1, s));
    gpuErrChk(hipEventSynchronize(t1));
    float ms = 0.f;
    gpuErrChk(hipEventElapsedTime(&ms, t0, t1));
    gpuErrChk(hipEventDestroy(t0));
    gpuErrChk(hipEventDestroy(t1));
    return ms;
}

// ---- the reference's PyTorch-path ABI (pytorch/wavenet_infer.cu:34-149) ----------------------
#ifndef WAVENET_INFER_R
#define WAVENET_INFER_R 64
#define WAVENET_INFER_S 256
#define WAVENET_INFER_A 256
#endif

int get_R(void) { return WAVENET_INFER_R; }
int get_S(void) { return WAVENET_INFER_S; }
int get_A(void) { return WAVENET_INFER_A; }

void wavenet_infer(int sample_count, int batch_size, float* embedding_prev, float* embedding_curr, int num_layers,
                   int max_dilation, float** in_layer_weights_prev, float** in_layer_weights_curr,
                   float** in_layer_biases, float** res_layer_weights, float** res_layer_biases,
                   float** skip_layer_weights, float** skip_layer_biases, float* conv_out_weight,
                   float* conv_end_weight, int use_embed_tanh, float* cond_input, int implementation, int* samples) {
    assert(samples);
    // uniform draws in the reference's rand() order: Matrix(batch, samples).randomize(0.5, 1.0)
    // iterates rows (utterances) outer, columns (samples) inner, two rand() per element, and
    // stores column-major = [sample][batch] (wavenet_infer.cu:92-94, matrix.cpp:38-55).  Drawn
    // before any HIP call: the HIP runtime itself consumes libc rand() while loading code
    // objects, which would make the sequence depend on runtime internals.
    std::vector<float> sel((size_t)sample_count * batch_size);
    for (int b = 0; b < batch_size; b++) {
        for (int s = 0; s < sample_count; s++) {
            (void)rand();
            float r = static_cast<float>(rand()) / static_cast<float>(RAND_MAX);
            r -= 0.5;
            r = r * 1.0f + 0.5f;
            sel[(size_t)s * batch_size + b] = r;
        }
    }
    nvw_engine* w = nvw_create(WAVENET_INFER_R, WAVENET_INFER_S, WAVENET_INFER_A, 32, num_layers, max_dilation,
                               batch_size, sample_count, implementation, use_embed_tanh);
    if (!w) exit(1);
    w->setEmbeddings(embedding_prev, embedding_curr);
    for (int l = 0; l < num_layers; l++)
        w->setLayerWeights(l, in_layer_weights_prev[l], in_layer_weights_curr[l], in_layer_biases[l],
                           res_layer_weights[l], res_layer_biases[l], skip_layer_weights[l], skip_layer_biases[l]);
    // no biases on the two output layers (wavenet_infer.cu:75-82)
    std::vector<float> zeroBias(WAVENET_INFER_A, 0.f);
    w->setOutWeights(conv_out_weight, zeroBias.data(), conv_end_weight, zeroBias.data());
    w->setInputs(cond_input, sel.data(), sample_count);
    const int bspb = ((batch_size % 4) == 0) ? 4 : ((batch_size % 2) == 0) ? 2 : 1;
    // The reference passes dumpActivations = true here (pytorch/wavenet_infer.cu:97), but no entry of this ABI can read the dump
    // (pytorch/wavenet_infer.h:33-58 has no getter) and the engine is destroyed below: the dump-free kernel generates the same
    // samples (tests/test_parity_gpu.py::test_wavenet_infer_c_abi_and_python_wrapper, ..::test_reference_pybind_extension_on_this_library)
    // without the accumulator read-outs the dump code costs in every layer.
    bool ok = w->run(sample_count, batch_size, samples, bspb, false, 0);
    assert(ok);
    (void)ok;
    gpuErrChk(hipDeviceSynchronize());
    // a multi-CU launch that gave up is re-run on wavenet_wg in stream order; a code left here means that could not be done
    // (this entry point has no status to return: fail like every other error of the path does, nv_wavenet_util.cuh:34-40)
    if (const unsigned st = w->chainStatus()) {
        fprintf(stderr, "wavenet_infer: multi-CU launch gave up (status 0x%x) and could not be re-run\n", st);
        exit(1);
    }
    delete w;
}

}  // extern "C"
