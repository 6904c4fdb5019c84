/*
 * nv_wavenet_c.h -- C ABI onto every nvWavenetInfer<T_weight,T_data,R,S,A> instantiation that
 * libwavenet_infer.so carries.  One handle = one engine object; each call maps 1:1 onto the
 * member of the same name of the reference class (/root/reference/nv_wavenet.cuh:220-640):
 *
 *   nvw_create            <- nvWavenetInfer(numLayers, maxDilation, batchSize, numSamples, impl,
 *                                           tanhEmbed)                        nv_wavenet.cuh:311
 *   nvw_set_embeddings    <- setEmbeddings                                   nv_wavenet.cuh:396-399
 *   nvw_set_layer_weights <- setLayerWeights                                 nv_wavenet.cuh:400-409
 *   nvw_set_out_weights   <- setOutWeights                                   nv_wavenet.cuh:410-415
 *   nvw_set_inputs        <- setInputs                                       nv_wavenet.cuh:417-422
 *   nvw_run / nvw_run_partial / nvw_run_chunks <- run / run_partial / run_chunks
 *                                                                            nv_wavenet.cuh:445-639
 *   nvw_get_*             <- getXtOut/getSkipOut/getZs/getZa/getP/getYOut    nv_wavenet.cuh:424-444
 *
 * The reference has no such header: its only FFI is pytorch/wavenet_infer.h, which hard-wires one
 * instantiation (see include/wavenet_infer.h).  This one exists so that non-C++ hosts (Python
 * ctypes, tests, bench.py) can reach fp16, other channel counts, chunked streaming and the
 * debug getters without a compiler.  Plain pointers and ints only; `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  Pointers may be host or device memory wherever the
 * reference accepts both.  Precision is 32 (<float,float>) or 16 (<half2,half>).
 *
 * Errors: unsupported (R,S,A,precision) -> nvw_create returns NULL; so do num_layers outside
 * 2..128, max_dilation < 1 (any value >= 1 is a schedule: d doubles per layer and restarts at 1
 * past it), batch_size < 1 and num_samples < 1 -- one line on stderr, no HIP call made, no
 * abort; run calls return 1 on
 * success and 0 when the launch failed (the reference's bool); HIP failures print
 * "GPUassert: ..." and exit like the reference's gpuErrChk.
 */
#ifndef NV_WAVENET_C_H
#define NV_WAVENET_C_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nvw_engine nvw_engine;

/* consumer callback of nvw_run_chunks: (yOut, first sample of the chunk, samples in it, user) */
typedef void (*nvw_consume_fn)(int* yOut, int init_sample, int count, void* user);

/* Revision of this interface.  It changes whenever an entry point or the meaning of an argument does -- in particular the
 * organisation codes of nvw_create_ex, which were renumbered once (round 3) and lost code 9 in round 4: a caller built against
 * another revision should check this instead of finding a different kernel behind a number.  5 = round 5 (the
 * feature-conditioning entry points below); 6 = this header (round 6: nvw_get_features returns int; nvw_upsample_features,
 * nvw_generate_stream and nvw_get_features check their ranges and refuse with 0 instead of reaching the class's asserts;
 * organisation 10; nvw_set_ring_in_lds); 7 = slot mode (nvw_slots_begin .. nvw_slots_end, below), and since, additively within 7
 * (every earlier entry unchanged), slot mode from mel frames (nvw_slot_start_mel .. nvw_slots_get_features). */
#define NVW_ABI_VERSION 7
int nvw_abi_version(void);
int nvw_supported(int R, int S, int A, int precision);
/* writes up to `max` (R,S,A,precision) quadruples into out[4*i..], returns how many exist */
int nvw_list_supported(int* out, int max);

nvw_engine* nvw_create(int R, int S, int A, int precision, int num_layers, int max_dilation,
                       int batch_size, int num_samples, int implementation, int tanh_embed);
/* The same with an explicit kernel organisation (the last, optional argument of this repo's nvWavenetInfer
 * constructor; 0 = from `implementation` and the batch size like nvw_create):
 *   1 wavenet_wg (1 to 4 tiles of 16 utterances per workgroup by batch size)   2 / 3 / 4 wavenet_wg with exactly 1 / 2 / 3
 *   (three: fp16, R <= 64; two tiles otherwise)   5 wavenet_chain (multi-CU, resident weights, fewest CUs)
 *   6 wavenet_chain with one layer per CU   7, 8, 9 retired (were wavenet_bcast -- every wave the whole network for its own
 *   tile, weights broadcast through an LDS ring -- and its variants; removed in round 5): refused like any number out of range
 *   10 wavenet_wg with four tiles per workgroup (round 6: fp16, R <= 64, dump-free launches with packed conditioning;
 *   other launches of such an engine take three).
 * Returns NULL when the shape does not fit a CU in that organisation (the reference's variants print
 * and return false for shapes they do not support, nv_wavenet_singleblock.cuh:273-286). */
nvw_engine* nvw_create_ex(int R, int S, int A, int precision, int num_layers, int max_dilation,
                          int batch_size, int num_samples, int implementation, int tanh_embed,
                          int organisation);
void nvw_destroy(nvw_engine* e);

void nvw_set_embeddings(nvw_engine* e, float* embed_prev, float* embed_cur);
void nvw_set_layer_weights(nvw_engine* e, int layer, float* Wprev, float* Wcur, float* Bh,
                           float* Wres, float* Bres, float* Wskip, float* Bskip);
void nvw_set_out_weights(nvw_engine* e, float* Wzs, float* Bzs, float* Wza, float* Bza);
void nvw_set_inputs(nvw_engine* e, float* Lh, float* output_selectors);

/* Extensions beyond the reference class (its "next" list: selectors drawn on the device instead of
 * the host rand() table of pytorch/wavenet_infer.cu:92-94; mu-law expansion of pytorch/utils.py:62-70
 * + pytorch/inference.py:58-60 done on the device):
 *   nvw_set_conditioning   the conditioning half of setInputs (Lh [N][L][B][2R]; history := 128)
 *   nvw_set_selector_seed  selectors = Philox4x32-10(counter {sample, utterance, 0, 0}, key = seed),
 *                          top 24 bits of word 0 / 2^24; stays in force until the next nvw_set_inputs
 *   nvw_set_audio_out      pcm_out: caller-owned [batch][samples] int16 (host or device), filled by
 *                          the run calls wherever yOut is: int16(32768 * mu_law_decode(y, A)); NULL
 *                          switches it off */
void nvw_set_conditioning(nvw_engine* e, float* Lh);
/* Utterances shorter than the engine's capacity: num_samples <= the num_samples of nvw_create rows of
 * Lh / output_selectors (both layouts are sample-major, so a prefix is a complete input) */
void nvw_set_inputs_n(nvw_engine* e, float* Lh, float* output_selectors, int num_samples);
void nvw_set_conditioning_n(nvw_engine* e, float* Lh, int num_samples);
/* Conditioning streamed chunk by chunk: packs samples [first_sample, first_sample + count) (Lh points at
 * sample first_sample, device memory) asynchronously on `stream`, e.g. behind nvw_run_partial of the
 * previous chunk on another stream.  Does not touch the sample history. */
void nvw_pack_conditioning(nvw_engine* e, float* Lh, int first_sample, int count, void* stream);
/* Device-resident conditioning consumed IN PLACE (no packed copy; pytorch/README.md:44 recommends keeping cond_input on
 * the device, wavenet_infer.cu:124-143 still copies it): Lh is fp32 [num_samples][L][batch_size][2R] in device memory --
 * batch_size is the ENGINE's, the capacity given to nvw_create, exactly as for nvw_set_inputs and the selectors: a run of fewer
 * utterances reads the first columns of every [batch_size][2R] row and never touches the others -- owned by
 * the caller and kept alive and unchanged until the run calls that follow have completed.  Resets the history like
 * nvw_set_inputs; pair with nvw_set_selector_seed.  Same samples as the packed path, bit for bit. */
void nvw_set_conditioning_direct(nvw_engine* e, float* Lh, int num_samples);
/* The same for a tensor of `precision` bits per element: 32 (float) or -- fp16 engines only -- 16 (IEEE half, the engine's
 * T_data: the reference keeps its conditioning in T_data, nv_wavenet.cuh:326; half the bytes of the fp32 tensor).  Returns 0
 * (and changes nothing) when the engine cannot read that element type in place. */
int nvw_set_conditioning_direct_t(nvw_engine* e, const void* Lh, int num_samples, int precision);
/* Conditioning PRODUCED in the engine's own fragment order by the caller (device memory, the engine's T_data):
 * [num_samples + 1][L][nvw_cond_tiles(e)][wave][fragment][lane][8 (fp16) | 4 (fp32)] with the gate rows pre-scaled, i.e. what
 * nvw_pack_conditioning writes (order: pack_cond_tiled_kernel in wn_kernels.hpp; nv_wavenet_amd/nv_wavenet.py:cond_fragment_order
 * gives it as a channel permutation + scale, which a model folds into its conditioning convolution for free).  The generation
 * kernels run their packed path on that buffer: no copy, no second pass.  One padding sample past the last; the buffer stays
 * alive and unchanged until the run calls that follow have completed.  Resets the history like nvw_set_inputs. */
void nvw_set_conditioning_packed(nvw_engine* e, const void* frags, int num_samples);
/* the same with the buffer's size stated (elements of the engine's T_data): returns 0 and changes nothing unless it holds
 * (num_samples + 1) x layers x nvw_cond_tiles(e) x 16 x 2R elements.  Either way the run calls that follow refuse (assert, like
 * the other preconditions of the path) to generate more samples than were handed over here. */
int nvw_set_conditioning_packed_n(nvw_engine* e, const void* frags, int num_samples, size_t elems);
int nvw_cond_tiles(nvw_engine* e);
/* The PRODUCER of such a buffer for fp16 engines (role of the model's `cond_layers` 1x1 convolution, pytorch/wavenet.py:190-202, with
 * the engine's channel order and gate pre-scale folded into its weights): one MFMA kernel from the upsampled features straight
 * into fragment order, no intermediate tensor, no permuting copy.  All pointers are device memory:
 *   x      [tiles*16][num_samples][32*kfrags] fp16: upsampled features, channels last, zero-padded to whole 32-feature fragments
 *   wfrag  [num_layers][nwf][2][kfrags][64][8] fp16 and bias [num_layers][nwf*32] fp32: the convolution's weights and bias as
 *          nv_wavenet_amd/nv_wavenet.py:cond_producer_weights arranges them (nwf = 2R/32 fragments per tile)
 *   out    [num_samples][num_layers][tiles][nwf][64][8] fp16: `num_samples` samples of the buffer handed to
 *          nvw_set_conditioning_packed_n (tiles = nvw_cond_tiles(e))
 * Asynchronous on `stream`; returns 0 when the arguments are out of range (1 <= kfrags <= 4) or the launch failed. */
int nvw_produce_conditioning_f16(const void* x, const void* wfrag, const float* bias, void* out, int tiles, int num_samples,
                                 int num_layers, int kfrags, int nwf, void* stream);
/* CONDITIONING COMPUTED IN THE GENERATION KERNEL (round 5).  The reference's pipeline builds cond_input = cond_layers(upsample(
 * features)) -- [2R][B][L][N], 2R*L values per utterance and sample -- in PyTorch and hands it to the engine
 * (pytorch/wavenet.py:190-202, inference.py:52-53).  Here the 1x1 convolution `cond_layers` moves INTO the generation kernel: the
 * caller hands over its weights once and, per utterance, only the upsampled features (n_cond values per utterance and sample);
 * Lh[t][l] = Wcond[l] c[t] + bcond[l] is computed where it is consumed (n_cond more k steps of the gate GEMM), and the
 * [N][L][B][2R] tensor is never built.  An additional contract beside nvw_set_inputs / nvw_set_conditioning*, which stay as they are.
 *   nvw_max_cond_channels          feature channels the kernels are built for (80 = the reference's config.json)
 *   nvw_set_conditioning_weights   Wcond [L][2R][n_cond] (cond_layers.weight, [2R*L][n_cond][1] as it is), bcond [L][2R]; fp32, host
 *                                  or device, copied.  0 when n_cond is out of range (nothing changes).
 *   nvw_set_features               the upsampled features of the whole utterance from a device tensor of `precision`-bit floats
 *                                  (32 | 16) addressed x[b*b_stride + c*c_stride + t*t_stride] (upsample output [B][n_cond][T]:
 *                                  strides n_cond*T, T, 1); copied into the engine's fragment order; resets the history like
 *                                  nvw_set_inputs; pair with nvw_set_selector_seed or nvw_set_selectors.
 *   nvw_pack_features              samples [first_sample, first_sample + count) only (x points at sample first_sample),
 *                                  asynchronously on `stream`, history untouched: streaming chunk by chunk like nvw_pack_conditioning
 *   nvw_set_conditioning_features  features the caller produced in fragment order itself, used in place:
 *                                  [num_samples][nvw_cond_tiles(e)][nvw_feature_fragments(e)][64][8 fp16 | 4 fp32] of the engine's
 *                                  T_data; fragment kf, lane (g, j), element e = channel (kf*TPF + (e>>2))*16 + 4g + (e&3) of utterance
 *                                  tile*16 + j (TPF = 2 fp16 | 1 fp32), zero beyond n_cond; `elems` = the buffer's size
 * All return 1 on success, 0 (after a message) when refused.  Runs that follow launch wn::wavenet_wg<.., RAW=3> whatever the
 * engine's organisation. */
int nvw_max_cond_channels(void);
int nvw_set_conditioning_weights(nvw_engine* e, const float* Wcond, const float* bcond, int n_cond);
int nvw_feature_fragments(nvw_engine* e);
size_t nvw_feature_elems(nvw_engine* e, int num_samples);
int nvw_set_conditioning_features(nvw_engine* e, const void* frags, int num_samples, size_t elems);
int nvw_pack_features(nvw_engine* e, const void* x, int precision, long long b_stride, long long c_stride, long long t_stride,
                      int first_sample, int count, void* stream);
int nvw_set_features(nvw_engine* e, const void* x, int precision, long long b_stride, long long c_stride, long long t_stride,
                     int num_samples);
/* FEATURES IN, AUDIO OUT (round 5; role of pytorch/inference.py:40-62 around run_chunks, nv_wavenet.cuh:445-497).  The other half of
 * WaveNet.get_cond_input -- the `upsample` ConvTranspose1d and the trimming of its tail, pytorch/wavenet.py:195-197 -- on the engine's
 * own MFMA kernel, writing the feature fragments the generation kernel reads:
 *   nvw_set_upsampling      upsample.weight [n_cond][n_cond][window] and .bias [n_cond] (fp32, host or device, copied); window a multiple
 *                           of stride, at most 5 strides (the reference: 800 / 200); after nvw_set_conditioning_weights
 *   nvw_set_mel             the utterances' frames before upsampling, device tensor of 16- or 32-bit floats addressed
 *                           x[b*b_stride + c*c_stride + f*f_stride] ([B][n_cond][frames]: strides n_cond*frames, frames, 1); copied;
 *                           frames * stride <= the engine's samples; resets the history like nvw_set_inputs (start of a batch)
 *   nvw_upsample_features   samples [first_sample, first_sample + count) of the upsampled features, asynchronously on `stream`
 *   nvw_generate_stream     the whole loop: per chunk of num_samples_per_chunk samples the upsampling, the generation launch, the copy of
 *                           the chunk's samples to yOut ([batch][num_samples] int32, host or device; may be NULL) and of the int16 PCM to
 *                           the buffer of nvw_set_audio_out on a second stream, and consume(yOut, first, count, user) on the calling
 *                           thread; selectors: nvw_set_selector_seed / nvw_set_selectors.  Returns when the last chunk is consumed.
 * All return 1 on success, 0 when refused. */
int nvw_set_upsampling(nvw_engine* e, const float* up_w, const float* up_b, int window, int stride);
int nvw_set_mel(nvw_engine* e, const void* mel, int precision, long long b_stride, long long c_stride, long long f_stride, int frames);
int nvw_upsample_features(nvw_engine* e, int first_sample, int count, void* stream);
/* debug getter: samples [first_sample, first_sample + count) of the engine's feature buffer (what nvw_pack_features / nvw_upsample_features
 * wrote: fragment order, the engine's T_data, nvw_feature_elems(e, count) elements) -> dst (host or device); synchronises.
 * 1, or 0 when refused: no feature buffer yet, or the range lies outside the engine's samples (ABI 6: returned void before) */
int nvw_get_features(nvw_engine* e, void* dst, int first_sample, int count);
int nvw_generate_stream(nvw_engine* e, int num_samples_per_chunk, nvw_consume_fn consume, void* user, int num_samples, int batch_size, int* yOut,
                        void* stream);
/* the selector half of nvw_set_inputs ([num_samples][batch] uniform draws, host or device); conditioning and history untouched */
void nvw_set_selectors(nvw_engine* e, float* output_selectors, int num_samples);
/* Multi-CU (wavenet_chain) launches need all their workgroups resident at once; when other work holds CUs a launch gives up
 * after a bounded wait and the engine re-runs its samples on wavenet_wg from the state the launch started with, in stream
 * order, so the samples delivered are the right ones either way.  nvw_chain_status: 0, or the code of a give-up that could
 * not be repaired; nvw_chain_fallbacks: launches that were re-run; nvw_chain_last_timeout: code of the latest of those
 * (0x100+stage x hand-off, 0x200+stage skip sums, 0x300 head, 0x400+ placement exchange).  All three synchronise the device.
 * nvw_set_chain_timeout_ms: the bound of every hand-off wait (default 1500 ms). */
unsigned nvw_chain_status(nvw_engine* e);
unsigned nvw_chain_fallbacks(nvw_engine* e);
unsigned nvw_chain_last_timeout(nvw_engine* e);
void nvw_set_chain_timeout_ms(nvw_engine* e, double ms);
/* Measurement aid: with the probe on, workgroup 0 of every single-workgroup-organisation launch records the shader-clock and the
 * constant-rate wall-clock counters at its start and end; nvw_last_launch_clock_ghz returns shader ticks per wall second of the
 * latest launch, i.e. the clock the chip granted it under its power budget (0 when nothing was probed); synchronises the device. */
void nvw_set_clock_probe(nvw_engine* e, int on);
/* The dilation ring on chip (round 6; the reference stages x[t-d] through shared memory out of a global ring, nv_wavenet.cuh:96-127,
 * 334-335): single-workgroup launches keep the ring slots of the layers with the shortest dilations in the LDS their tables leave
 * free, loaded from / spilled to the HBM ring at the launch's ends (1-KiB rows).  mode >= 0 (default): as many layers as fit -- a model
 * whose whole ring fits has no ring traffic to HBM during the launch; -1: never.  Same samples either way. */
void nvw_set_ring_in_lds(nvw_engine* e, int mode);
/* The dilation schedule compiled into the kernel: a three-tile fp16 launch with packed conditioning of a model whose dilations run
 * 1 .. 512 in whole cycles of ten layers, with ring slots in LDS, runs a kernel that knows every layer's dilation and slot placement at
 * compile time (nvw_kernel_info ends in `sched=cycle10`).  mode >= 0 (default): where eligible; -1: never.  Same samples and ring
 * either way: launches of both kinds mix within an utterance. */
void nvw_set_compiled_schedule(nvw_engine* e, int mode);
double nvw_last_launch_clock_ghz(nvw_engine* e);
/* Samples [init_sample, init_sample + count) of a num_samples-long utterance, asynchronously on `stream`
 * (one chunk of run_chunks, for hosts that drive the chunks themselves); nvw_reset_history starts a new
 * utterance -- sample history back to 128, dilation rings back to zero -- like nvw_set_inputs does, without
 * touching the conditioning. */
int nvw_run_range(nvw_engine* e, int init_sample, int count, int num_samples, int batch_size, void* stream);
void nvw_reset_history(nvw_engine* e, void* stream);
void nvw_set_selector_seed(nvw_engine* e, unsigned long long seed);
void nvw_set_audio_out(nvw_engine* e, short* pcm_out);
/* the same with the buffer's size in int16 values stated: every run call then checks batch * num_samples <= elems */
void nvw_set_audio_out_n(nvw_engine* e, short* pcm_out, size_t elems);
/* Introspection: the device code nvw_run(e, n, batch_size, ..., dump_activations, ...) launches, e.g.
 * "wn::wavenet_wg<fp16,64,256,256,BT=2,EMBLDS=1,DUMP=0> tiles/wg=2 wgs=256 lds=149120"; in slot mode, what a step launches
 * while the highest active column is batch_size - 1 (dump_activations 0) */
void nvw_kernel_info(nvw_engine* e, int batch_size, int dump_activations, char* buf, int buf_size);

int nvw_run(nvw_engine* e, int num_samples, int batch_size, int* yOut, int batch_size_per_block,
            int dump_activations, void* stream);
int nvw_run_partial(nvw_engine* e, int init_sample, int num_samples, int batch_size, int* yOut,
                    int batch_size_per_block, int dump_activations, void* stream);
int nvw_run_chunks(nvw_engine* e, int num_samples_per_chunk, nvw_consume_fn consume, void* user,
                   int num_samples, int batch_size, int* yOut, int batch_size_per_block,
                   int dump_activations, void* stream);

void nvw_get_xt_out(nvw_engine* e, int layer, float* dst);     /* [maxBatch][R] */
void nvw_get_skip_out(nvw_engine* e, int layer, float* dst);   /* [maxBatch][S] */
void nvw_get_zs(nvw_engine* e, float* dst);                    /* [maxBatch][A] */
void nvw_get_za(nvw_engine* e, float* dst);                    /* [maxBatch][A] */
void nvw_get_p(nvw_engine* e, float* dst);                     /* [maxBatch][A] */
void nvw_get_y_out(nvw_engine* e, int* yOut, int offset, int size, void* stream);

/* SLOT MODE: CONTINUOUS BATCHING (ABI 7).  Every column of the batch holds one utterance that starts and stops on its own while
 * the others go on; the samples of an utterance depend on its upsampled features, its uid, the seed of nvw_set_selector_seed (0 if
 * none was set), the model and the sampling temperature in force at each local sample (1 unless nvw_slot_set_temperature says
 * otherwise; see SAMPLING TEMPERATURE below) and its prime (none unless nvw_slot_prime gives one; see PRIMED GENERATION below) only
 * -- not on its column, the step it joined at, its neighbours or the chunk sizes.  Local sample k
 * draws its selector from Philox4x32-10 with counter {k, uid, 0, 0}: an utterance with uid = b reproduces column b of a lockstep
 * nvw_set_features + nvw_set_selector_seed run.  Needs nvw_set_conditioning_weights (the conditioning is computed in the kernel).
 *   nvw_slots_begin  enters slot mode with a window of `window` samples, a positive multiple of the largest dilation of the schedule
 *                    (state of the generation between steps, sized by the window and not by the engine's num_samples: an utterance
 *                    may be of any length); every column idle; synchronises.  0 when refused (no conditioning weights, bad window).
 *   nvw_slot_start   column `slot` takes a new utterance at the next step: features x[c*c_stride + k*t_stride] (device memory,
 *                    `precision` = 16 | 32 bits, n_cond channels x `length` samples, kept alive and unchanged while the column
 *                    runs), its uid; sample history 128 and dilation rings zero as for a new lockstep utterance.  0 when refused
 *                    (not in slot mode, slot outside 0..batch-1, host memory, bad precision, non-positive strides or length).
 *   nvw_slot_stop    column `slot` goes idle at the next step.  0 when refused (not in slot mode, slot out of range).
 *   nvw_slots_step   `count` (1..window) samples of every column, asynchronously on `stream`: pending starts and stops, the window
 *                    feed, the generation launches up to the highest active column's tile, the PCM when pcm != NULL, and the step's
 *                    samples / PCM into yOut / pcm, [batch][count] int32 / int16, host or device, either may be NULL (synchronises
 *                    the stream when one is host memory).  Idle columns and samples past an utterance's length hold unspecified
 *                    values.  0 when refused (not in slot mode, count out of range; nothing changes) or a launch failed.  The steps
 *                    of a session are issued on one stream.
 *   nvw_slots_end    leaves slot mode and frees its buffers (synchronises); lockstep calls work as before afterwards. */
int nvw_slots_begin(nvw_engine* e, int window);
int nvw_slot_start(nvw_engine* e, int slot, const void* x, int precision, long long c_stride, long long t_stride, int length,
                   unsigned uid);
int nvw_slot_stop(nvw_engine* e, int slot);
int nvw_slots_step(nvw_engine* e, int count, int* yOut, short* pcm, void* stream);
void nvw_slots_end(nvw_engine* e);

/* SLOT MODE FROM MEL FRAMES (additive within ABI 7).  A column may hold a mel utterance instead of upsampled features: its frames
 * before upsampling, upsampled by the engine (the table of nvw_set_upsampling) in the steps that generate them.  Its samples are bit
 * for bit those of column uid of a lockstep nvw_set_mel + nvw_generate_stream run with the same seed, whatever the column, the join
 * step, the step sizes, the neighbours, and however its frames were handed over.  Frames may arrive while the column runs (the
 * upsampling is causal: sample k reads frames k / stride - j, j < window / stride): a step never goes past the frames available.
 *   nvw_slot_start_mel     column `slot` takes a mel utterance at the next step: frames mel[c*c_stride + f*f_stride] (device memory,
 *                          `precision` = 16 | 32 bits, n_cond channels, kept alive while the column runs), `frames` of them written
 *                          so far, final != 0: no more will come (the utterance is frames x stride samples long), its uid.  0 when
 *                          refused (not in slot mode, no nvw_set_upsampling, slot out of range, host memory, bad precision,
 *                          non-positive strides, frames < 0, or 0 frames with final).
 *   nvw_slot_mel_frames    `frames` frames of column `slot`'s utterance are now written in the same buffer, ordered before the next
 *                          step on the step stream; final != 0: no more will come.  0 when refused (not a mel column, already final,
 *                          fewer frames than before, 0 frames with final; nothing changes).
 *   nvw_slots_headroom     the largest count the next nvw_slots_step accepts: the window, or the minimum over non-final mel columns
 *                          of frames x stride minus their next local sample (may be 0).  nvw_slots_step refuses a larger count and
 *                          changes nothing; only sessions with mel columns can meet this refusal.
 *   nvw_slots_get_features debug getter: the window's feature fragments of engine samples [first_sample, first_sample + count), which
 *                          must lie within the last window of samples generated, in the order of nvw_get_features (synchronises).
 *                          0 when refused. */
int nvw_slot_start_mel(nvw_engine* e, int slot, const void* mel, int precision, long long c_stride, long long f_stride, int frames,
                       int final, unsigned uid);
int nvw_slot_mel_frames(nvw_engine* e, int slot, int frames, int final);
int nvw_slots_headroom(nvw_engine* e);
int nvw_slots_get_features(nvw_engine* e, void* dst, long long first_sample, int count);

/* SLOT MODE: A COLUMN'S STATE AS A VALUE (additive within ABI 7).  What an utterance owns on the device between steps -- its column's
 * share of the dilation ring, two history words, its descriptor -- can be moved to another column, saved into a blob, and resumed
 * from the blob in any column, at any step, in any engine with the same model and seed; the utterance's samples stay those of
 * column uid of its lockstep run.  The blob is nvw_slot_state_bytes(e) bytes: a 64-byte header (magic, layout version, precision, R,
 * layers, max_dilation, done = local samples generated, uid, the two history words) and the ring share in canonical order -- layer
 * l's d_l slots rotated so that slot k mod d_l is the one local sample k uses, i.e. the ring of an utterance started at counter 0 --
 * so it does not depend on the column, the join step, window wraps or the engine.  It holds neither the features / frames (handed
 * over again on resume) nor the seed or the model.
 *   nvw_slot_state_bytes  size of one column's blob for this engine's shape and precision.
 *   nvw_slot_move         the utterance of column `from` goes on in column `to` (queued; the next nvw_slots_step applies its moves
 *                         first -- one launch for all of them -- so `from` may take a new start in the same step).  0 when refused
 *                         (not in slot mode; an index out of range or from == to; `from` holds no utterance or has a pending start
 *                         or resume; `to` holds an utterance or has a pending start, resume or move; `from` is an endpoint of a
 *                         pending move; nothing changes).  A pending stop on `to` is superseded.  Until the step has applied the move,
 *                         nvw_slot_start / _start_mel / _resume / _resume_mel on `to` are refused (they would drop the utterance on
 *                         its way in); nvw_slot_stop on `to` is not.
 *   nvw_slot_save         the state of column `slot` after the steps issued so far into dst (device memory, 16-byte aligned),
 *                         asynchronously on `stream` (the stream of the steps, or one ordered after them); the column goes on.
 *                         Returns done >= 0, or -1 when refused (not in slot mode, no utterance, a pending start, resume or move on
 *                         the column, bad dst; nothing is written).
 *   nvw_slot_resume       nvw_slot_start, continuing from `state`: uid and done come from its header (read here with a small
 *                         blocking copy on the null stream: it waits for a save issued on the null stream or on a stream that
 *                         synchronises with it; a save on a non-blocking stream must have completed, or been ordered before this
 *                         call by the caller); at the next step the column's
 *                         ring and history are loaded from it and local sample `done` is generated.  x and length are the whole
 *                         utterance's, as at its start.  `state` stays unchanged until the next step has been issued.  0 when
 *                         refused (wrong magic or layout version, another shape or precision, done >= length, or what
 *                         nvw_slot_start refuses; nothing changes).
 *   nvw_slot_resume_mel   the same for a mel utterance (nvw_slot_start_mel); refused also when final and done >= frames x stride. */
size_t nvw_slot_state_bytes(nvw_engine* e);
int nvw_slot_move(nvw_engine* e, int from, int to);
int nvw_slot_save(nvw_engine* e, int slot, void* dst, void* stream);
int nvw_slot_resume(nvw_engine* e, int slot, const void* state, const void* x, int precision, long long c_stride, long long t_stride,
                    int length);
int nvw_slot_resume_mel(nvw_engine* e, int slot, const void* state, const void* mel, int precision, long long c_stride,
                        long long f_stride, int frames, int final);

/* SLOT MODE: LISTS OF COLUMNS SAVED AND RESUMED, BLOBS IN PINNED MEMORY (additive within ABI 7).  Draining an engine, rebalancing
 * between engines and checkpointing take many columns at once: one call saves a list of them with one launch, one call resumes a
 * list after reading every header at once.  The blobs are those of nvw_slot_save, byte for byte, rows of one buffer: blob i at
 * base + i * stride, base 16-byte aligned, stride a multiple of 16 and at least nvw_slot_state_bytes(e).  The buffer is device
 * memory or pinned host memory (hipHostMalloc, a registered range, nvw_pinned_alloc, torch pin_memory), which the device writes and
 * reads in place -- a drained engine's state leaves the GPU without a further copy.  (nvw_slot_save, nvw_slot_resume and
 * nvw_slot_resume_mel keep refusing host memory.)
 *   nvw_slots_save_list    the states of the n columns slots[0 .. n) after the steps issued so far, asynchronously on `stream`: one
 *                          small staging copy of the entries and one launch; never synchronises the stream and waits for nothing
 *                          queued on it (only a third list save in a row waits, for the first to have completed; the first of a
 *                          session allocates two small staging buffers on either side, once).  saved[i] = {slot, uid, done, mel != 0 for a mel column}
 *                          is filled before the call returns, from host state.  The columns go on running.  Returns n; -1 with
 *                          nothing written and nothing launched when not in slot mode, n outside 1..batch, a slot out of range or
 *                          listed twice, a slot without an utterance or with a pending start, resume or move, dst NULL, misaligned
 *                          or pageable host memory, a bad stride.
 *   nvw_slots_resume_list  n resumes, all or nothing: reqs[i] names the column, the kind (mel != 0: nvw_slot_resume_mel, length =
 *                          frames, final as there; mel == 0: nvw_slot_resume, length = samples, final ignored), the features / frames
 *                          (src, precision, c_stride, t_stride) and continues from the blob states + i * stride.  The n headers are
 *                          read at once: device memory with one blocking 2-D copy on the null stream (the ordering rule of
 *                          nvw_slot_resume); pinned memory in place, so the save must have completed.  Each request is refused for
 *                          what nvw_slot_resume / nvw_slot_resume_mel refuse, and also when its column holds an utterance or has a
 *                          pending start or resume (a list never replaces one) or is named twice.  Any refusal: 0, and the session
 *                          is exactly as before.  Otherwise n: the next step loads all of them in its one load launch and generates
 *                          each column's local sample `done`.  The blobs stay unchanged until that step has been issued. */
typedef struct {
    int slot;
    unsigned uid;
    int done;
    int mel;
} nvw_slot_saved;
int nvw_slots_save_list(nvw_engine* e, const int* slots, int n, void* dst, long long stride, nvw_slot_saved* saved, void* stream);
typedef struct {
    int slot;
    int mel;
    const void* src;
    int precision;
    long long c_stride, t_stride;
    int length; /* feature columns: samples; mel columns: frames */
    int final;
} nvw_slot_resume_req;
int nvw_slots_resume_list(nvw_engine* e, const nvw_slot_resume_req* reqs, int n, const void* states, long long stride);

/* SLOT MODE: RAGGED DELIVERY, STEPS THAT NEVER BLOCK (additive within ABI 7).  nvw_slots_step copies [batch][count] rows, idle columns
 * and the samples past an utterance's end included, and synchronises when an output is host memory.  A ragged step delivers pieces:
 * one per column that holds an utterance with at least one sample in this step, in ascending column order; a piece's n samples lie
 * contiguously at element `offset` of `samples` (int32) and their PCM at the same offset of `pcm` (int16).  Every offset is a
 * multiple of 8 elements; the 0 to 7 elements between a piece's end and the next piece's start are not written.
 *   nvw_slots_step_ragged  the launches of nvw_slots_step up to and including the generation, one delivery launch, an event record;
 *                          never synchronises.  samples / pcm: device memory or pinned host memory (hipHostMalloc, a registered
 *                          range, nvw_pinned_alloc, torch pin_memory), `capacity` elements each; either may be NULL.  pieces[0 ..
 *                          *n_pieces) (host memory, room for max_pieces) is filled before the call returns, from what the host
 *                          knows: first = local index of the piece's first sample; n = min(count, length - first) for a feature
 *                          column and a final mel column, count for a non-final mel column; finished != 0: the piece ends the
 *                          utterance (the column is NOT stopped: nvw_slot_stop stays the caller's call); uid of the utterance.
 *                          *ticket (1, 2, ...) names the step.  Returns the ragged size in elements (the end of the last piece; 0
 *                          when no column delivers); -2 when a launch failed (the step was issued and has its ticket, its outputs
 *                          are not to be read: nvw_slots_step returns 0 there); or -1 with nothing changed: not in slot mode, count outside 1..window or above
 *                          nvw_slots_headroom, both outputs NULL, an output in pageable host memory, capacity or max_pieces too
 *                          small (batch x (count rounded up to 8) elements and batch pieces always suffice).  Ragged and plain
 *                          steps may be mixed.  The outputs of a step are complete once its ticket is.
 *   nvw_slots_wait         blocks until the outputs of the step with that ticket are complete; 1, or 0 for a ticket never given.
 *                          The engine keeps the events of the last 4 tickets: an older one is complete (a fifth step in flight
 *                          waits for the first) and the call returns at once.
 *   nvw_slots_done         the same question without blocking: 1 complete, 0 not yet (or never given).
 *   nvw_pinned_alloc/free  pinned host memory for hosts without a HIP binding (NULL when it cannot be had).
 *   nvw_slots_time_outputs measurement only (as nvw_time_runs): `reps` output passes over the last `count` samples generated, timed
 *                          with events on `stream`, milliseconds for all of them.  ragged = 0: what nvw_slots_step issues after the
 *                          generation (PCM launches + 2-D copies into samples / pcm [batch][count]); ragged != 0: the delivery
 *                          launch for every column holding an utterance.  Both outputs given, device or pinned, `capacity` elements.
 *                          Synchronises the device, changes nothing of the session; < 0 when refused. */
typedef struct {
    int slot;
    unsigned uid;
    long long first;
    int n;
    int finished;
    long long offset;
} nvw_slot_piece;
long long nvw_slots_step_ragged(nvw_engine* e, int count, int* samples, short* pcm, long long capacity, nvw_slot_piece* pieces,
                                int max_pieces, int* n_pieces, unsigned long long* ticket, void* stream);
int nvw_slots_wait(nvw_engine* e, unsigned long long ticket);
float nvw_slots_time_outputs(nvw_engine* e, int ragged, int count, int* samples, short* pcm, long long capacity, int reps, void* stream);
int nvw_slots_done(nvw_engine* e, unsigned long long ticket);
void* nvw_pinned_alloc(size_t bytes);
void nvw_pinned_free(void* p);

/* SAMPLING TEMPERATURE PER UTTERANCE, LOCKSTEP AND IN SLOT MODE (additive within ABI 7).  The last step of the network draws from
 * softmax(logits / T): T = 1 is the model as trained, a smaller T sharpens the distribution (less noise, towards muffled), a larger
 * one flattens it.  The softmax computes exp2(x c - m c) with c = log2(e) / T per column in place of the constant log2(e): the
 * instructions per sample are the same, T = 1 is bit-identical to a run without these calls, and for T a power of two the samples
 * and probabilities are bit for bit those of the same model with Wza / T and Bza / T handed to nvw_set_out_weights.  T is finite
 * and in [2^-10, 2^10].  Greedy (argmax) decoding is not offered: T = 2^-10 approaches it, but still draws between logits that tie
 * at the maximum.  Only the launches that compute the conditioning in the kernel read the temperatures (nvw_set_features,
 * nvw_pack_features, nvw_set_conditioning_features, nvw_set_mel + nvw_generate_stream, slot mode); the probability dump
 * (nvw_get_p) reports the tempered probabilities, nvw_get_za the raw logits.
 * This extends the contract of slot mode: an utterance's samples depend on its features (or frames), its uid, the seed, the model
 * AND THE TEMPERATURE IN FORCE AT EACH LOCAL SAMPLE -- and on nothing else.  With uid = b and the same temperatures at the same
 * local samples it reproduces column b of a lockstep run, bit for bit, in both precisions.
 *   nvw_set_temperatures      lockstep: column b < n samples at T[b] (host array, 1 <= n <= batch) in the runs that follow; columns
 *                             past n, and every column with T == NULL, at 1.  The values stay in force across nvw_set_features,
 *                             nvw_set_mel, nvw_reset_history and between nvw_run_partial / nvw_run_range chunks until the next call;
 *                             a call between two chunks takes effect at the next chunk and leaves the history alone.  While any
 *                             column's T is not 1, a run on packed or in-place conditioning or on a multi-CU (chain) engine
 *                             prints one line and returns 0: nothing is generated, nothing is silently ignored.  Synchronises.
 *                             0 when refused (in slot mode, n out of range, a bad value); nothing changes.
 *   nvw_slot_set_temperature  slot mode: the utterance of column `slot` samples at T from the next step on, from that step's first
 *                             sample.  nvw_slot_start / _start_mel put the column back to 1, so the order is start, then set;
 *                             nvw_slots_begin and nvw_slots_end put every column back to 1.  nvw_slot_move, the saves and the
 *                             resumes carry the value: a blob holds it in word 10 of its header as the bits of the float, all-zero
 *                             bits for T = 1, so blobs of utterances at T = 1 are byte for byte what they were; a resume refuses a
 *                             header whose word is neither zero nor a valid temperature.  A step with changed columns issues one
 *                             small launch ahead of its generation launch.  0 when refused (not in slot mode, slot out of range,
 *                             a column without an utterance or a pending start or resume, a bad value); nothing changes.
 *   nvw_slot_temperature      the value in force for column `slot` (host state); 0 when the column holds no utterance. */
int nvw_set_temperatures(nvw_engine* e, const float* T, int n);
int nvw_slot_set_temperature(nvw_engine* e, int slot, float T);
float nvw_slot_temperature(nvw_engine* e, int slot);

/* PROBABILITY FLOOR (MIN-P) PER UTTERANCE, LOCKSTEP AND IN SLOT MODE (additive within ABI 7).  The second sampling control: a column
 * with floor p draws from its TEMPERED distribution (temperature first, then floor) without the bins whose probability is below p
 * times that of the most probable bin, renormalised.  In the kernel: after e = exp2(x c - m c) -- which is prob / max prob up to the
 * rounding of m c -- a bin with e < p gets e = 0 before the sum, the scan and the row search; nothing else changes.  p is finite and in
 * [0, 0.5]; p = 0 keeps every bin and is bit-identical to a run without these calls; 0.5 is where the guarantee ends that the most
 * probable bin survives the rounding of m c.  A forced sample (a prime) stays forced.  nvw_get_p reports the floored, renormalised
 * probabilities (dropped bins read exactly 0), nvw_get_za the raw logits.  Scoring (nvw_score_*) is NOT changed: it stays the model's
 * own distribution.  Top-k and top-p are the next section.  A launch with no floor in force executes the same instructions per logit
 * as before; one with a floor in force adds a compare and a select per logit.
 * This extends the contract of slot mode once more: an utterance's samples depend on its features (or frames), its uid, the seed,
 * the model, the temperature AND THE FLOOR IN FORCE AT EACH LOCAL SAMPLE -- and on nothing else.
 *   nvw_set_min_p       lockstep: column b < n at floor p[b] (host array, 1 <= n <= batch) in the runs that follow; columns past n,
 *                       and every column with p == NULL, at 0.  In force across nvw_set_features, nvw_set_mel, nvw_reset_history
 *                       and between nvw_run_partial / nvw_run_range chunks until the next call; a call between two chunks takes
 *                       effect at the next chunk.  Independent of nvw_set_temperatures: neither call resets the other's values.
 *                       While any column's floor is not 0, a run on packed or in-place conditioning or on a multi-CU (chain) engine
 *                       not on the features path prints one line and returns 0.  Synchronises.  0 when refused (in slot mode, n out
 *                       of range, a bad value); nothing changes.
 *   nvw_slot_set_min_p  slot mode: the utterance of column `slot` draws with floor p from the next step on, from that step's first
 *                       sample.  nvw_slot_start / _start_mel put the column back to 0, so the order is start, then set;
 *                       nvw_slots_begin and nvw_slots_end put every column back to 0.  nvw_slot_move, the saves and the resumes
 *                       carry the value: a blob holds it in word 11 of its header as the bits of the float, all-zero bits for 0, so
 *                       blobs of utterances at floor 0 are byte for byte what they were; a resume refuses a header whose word 11 is
 *                       neither zero nor a valid floor.  The blobs that nvw_prefill_* and the scoring chunks write leave word 11
 *                       zero: set the floor after resuming from one.  The step's one small launch that writes changed temperatures
 *                       writes the changed floors as well.  0 when refused (not in slot mode, slot out of range, a column without
 *                       an utterance or a pending start or resume, a bad value); nothing changes.
 *   nvw_slot_min_p      the value in force for column `slot` (host state); -1 when the column holds no utterance (0 is a valid
 *                       floor). */
int nvw_set_min_p(nvw_engine* e, const float* p, int n);
int nvw_slot_set_min_p(nvw_engine* e, int slot, float p);
float nvw_slot_min_p(nvw_engine* e, int slot);

/* TAIL CUTS (TOP-K, TOP-P) PER UTTERANCE, LOCKSTEP AND IN SLOT MODE (additive within ABI 7).  Two more sampling controls, both
 * thresholds on the quantity the floor compares, e = exp2(x c - m c) = prob / max prob of the TEMPERED distribution:
 *   top-k = k  keeps the bins with e >= theta_k, theta_k the k-th largest e: the k most probable bins, and every bin that ties with
 *              the k-th.  k is an integer in [0, A]; 0 is off (and k = A keeps every bin: bit-identical to off).
 *   top-p = p  keeps the bins with e >= theta_p, theta_p the largest threshold whose kept mass (summed in float32, as the kernel sums)
 *              still reaches p times the whole mass: the smallest set of most probable bins whose mass reaches p, ties at its edge
 *              included.  p is finite and in (0, 1]; 1 is off.
 * The kernel finds both thresholds by a bisection over the bit patterns of e -- no sort --, floors at max(theta_k, theta_p, min-p)
 * and goes on as for the floor: the kept set is the INTERSECTION of the three cuts, each defined on the full tempered distribution
 * (not the sequential "top-p of the renormalised top-k" some samplers apply).  The most probable bin always stays.  top-k = 1 is
 * greedy decoding: the argmax, with only exact ties in e drawn between.  A forced sample stays forced; nvw_get_p reports the cut,
 * renormalised probabilities (dropped bins read exactly 0), nvw_get_za the raw logits; scoring (nvw_score_*) is NOT changed.  A
 * launch with every column off executes what it executed before these calls existed; one with a cut in force adds the search: 31
 * steps, each with one compare per logit that serves both cuts, an add-with-carry (the count), a select and an add (the mass) --
 * about a third of a sample at the headline shape, in every column of the launch, whatever the values.
 * An utterance's samples depend on its features (or frames), its uid, the seed, the model, the temperature, the floor AND THE CUTS IN
 * FORCE AT EACH LOCAL SAMPLE -- and on nothing else.
 *   nvw_set_top_k, nvw_set_top_p            lockstep, as nvw_set_min_p: column b < n at k[b] / p[b] (host arrays, 1 <= n <= batch),
 *                       columns past n, and every column with a NULL array, off.  None of nvw_set_temperatures, nvw_set_min_p and
 *                       these two resets another's values.  While any column has a cut, a run on packed or in-place conditioning or
 *                       on a multi-CU (chain) engine not on the features path prints one line and returns 0.  Synchronises.  0 when
 *                       refused (in slot mode, n out of range, a bad value); nothing changes.
 *   nvw_slot_set_top_k, nvw_slot_set_top_p  slot mode, as nvw_slot_set_min_p: from the next step on.  Starts put the column back to
 *                       off; nvw_slot_move, the saves and the resumes carry the values: a blob holds top-k in word 12 of its header
 *                       as the integer, top-p in word 13 as the bits of the float, all-zero bits for 1, so blobs of utterances
 *                       without a cut are byte for byte what they were; a resume refuses a header whose word 12 is outside [0, A] or
 *                       whose word 13 is neither zero nor a valid p.  The blobs that nvw_prefill_* and the scoring chunks write leave
 *                       both words zero.  nvw_slot_stop and the source of a move go back to off.  0 when refused; nothing changes.
 *   nvw_slot_top_k, nvw_slot_top_p          the value in force for column `slot` (host state); -1 when it holds no utterance.
 *   nvw_sampler_mask    what the next features-path launch pays for (host state): bit 0, some column's floor is not 0 (a compare and
 *                       a select per logit); bit 1, some column has a cut (the search).  0: the launches of an engine that never
 *                       heard of floors and cuts.  A session whose floored and cutting utterances have all ended reads 0 again. */
int nvw_set_top_k(nvw_engine* e, const int* k, int n);
int nvw_set_top_p(nvw_engine* e, const float* p, int n);
int nvw_slot_set_top_k(nvw_engine* e, int slot, int k);
int nvw_slot_set_top_p(nvw_engine* e, int slot, float p);
int nvw_slot_top_k(nvw_engine* e, int slot);
float nvw_slot_top_p(nvw_engine* e, int slot);
int nvw_sampler_mask(nvw_engine* e);

/* PRIMED GENERATION: FORCED SAMPLE PREFIXES, LOCKSTEP AND IN SLOT MODE (additive within ABI 7).  An utterance may carry a prime, n
 * sample indices y[0 .. n) in 0 .. A-1: its local sample k < n IS y[k] -- written to the outputs (samples, PCM, ragged pieces) like
 * any other, fed back into the history and through the embeddings, so the rings evolve exactly as if it had been drawn --, and its
 * local sample k >= n is drawn as always, with selector {k, uid} of the seed (or row k of an uploaded table) at the temperature in
 * force.  Forced samples consume no draw and shift no counter.  So a prime made of the first n samples of an unprimed run
 * continues that run bit for bit, and the samples are a second, portable form of a state blob: a column primed with the `done`
 * samples of an interrupted utterance saves the blob the uninterrupted one would have saved.  Only the launches that compute the
 * conditioning in the kernel honour a prime (as for the temperatures).  At a forced sample nvw_get_p still reports the model's
 * (tempered) probabilities and nvw_get_za its logits: only the pick is replaced.
 * The contract of slot mode grows by one clause: an utterance's samples depend on its features (or frames), its uid, the seed, the
 * model, the temperatures AND ITS PRIME -- and on nothing else.
 *   nvw_set_prime    lockstep: column b < batch is primed with the first n[b] (0 .. max_n; 0: not primed) values of y + b * stride
 *                    (int32, host or device, max_n values readable per column, stride >= max_n; copied); y == NULL clears.  In force
 *                    across nvw_set_features / nvw_set_mel / nvw_reset_history and between chunks, like the temperatures; applies
 *                    to nvw_run*, nvw_run_range and nvw_generate_stream on the features path.  A launch whose range holds a forced
 *                    sample is preceded by one small launch that fills its rows of an engine-owned second selector table; the
 *                    caller's own table is never written, and a launch past every prime is exactly what it was.  While any column
 *                    is primed, a run on packed or in-place conditioning or on a multi-CU (chain) engine off the features path
 *                    prints one line and returns 0.  Values in device memory are clamped into 0 .. A-1.  Synchronises.  0 when
 *                    refused (slot mode, batch outside 1 .. the engine's batch, an n[b] outside 0 .. max_n, max_n above the engine's
 *                    samples, stride < max_n, a host value outside 0 .. A-1); nothing changes.
 *   nvw_slot_prime   slot mode: the utterance whose start or resume is pending on column `slot` is primed with y[0 .. n) (device
 *                    memory, kept alive and unchanged until local sample n has been generated; values clamped into 0 .. A-1).
 *                    Order: start (or resume), then prime -- nvw_slot_start / _start_mel / _resume* put the column back to "no
 *                    prime", nvw_slot_stop and nvw_slots_begin / _end drop it, nvw_slot_move carries it.  State blobs know nothing
 *                    of primes: a blob saved at done < n is resumed by nvw_slot_resume* followed by nvw_slot_prime with the same
 *                    y, n.  A step with a column inside its prime issues one small launch between the feed and the generation.
 *                    0 when refused (not in slot mode, slot out of range, no pending start or resume on the column, host memory,
 *                    n < 1, n above the utterance's length -- a non-final mel column is not bounded by its frames so far, and
 *                    nvw_slots_headroom governs as before); nothing changes.
 *   nvw_slot_primed  n of the prime in force on column `slot` (host state: until the step that generates local sample n - 1 has
 *                    been issued), 0 when none. */
int nvw_set_prime(nvw_engine* e, const int* y, const int* n, int batch, int max_n, long long stride);
int nvw_slot_prime(nvw_engine* e, int slot, const int* y, int n);
int nvw_slot_primed(nvw_engine* e, int slot);

/* PREFILL: A PRIME'S STATE BLOB FROM A TIME-PARALLEL PASS (additive within ABI 7).  A prime of n samples costs n samples of
 * generation when it is forced through a column.  Every forced sample is known, though, so the state behind the prime can be
 * computed layer by layer over 16 samples at a time, without the skip path, the head or the softmax: one launch per layer over the
 * last W = nvw_prefill_window samples of the prime, which are all the state depends on -- a prime of ten seconds costs what one of W
 * samples costs.  The result is the blob of nvw_slot_save: prefill(y[0 .. n), features, uid, temperature) EQUALS, BYTE FOR BYTE,
 * header and payload, in fp16 and in fp32, what nvw_slot_start, nvw_slot_set_temperature, nvw_slot_prime(y, n), steps up to local
 * sample n and nvw_slot_save produce with the same features, uid and temperature -- the samples that follow a resume do not depend on
 * how the state was made.  The pass reads the engine's own weight streams and touches no ring, column or session.
 *   nvw_prefill_window  W: the number of trailing samples that determine a state (the sum of the dilations + the two history samples
 *                       the embedding reads); 0 when the engine has no conditioning weights.
 *   nvw_prefill_states  `count` requests with one set of layer launches, blob i to dst + i * stride: device memory or pinned host
 *                       memory, 16-byte aligned, stride a multiple of 16 and at least nvw_slot_state_bytes.  y: the prime, int32 in
 *                       device memory, n >= 1 values (clamped into 0 .. A-1 as nvw_slot_prime clamps them); x, precision, c_stride,
 *                       t_stride: the utterance's features as for nvw_slot_start, of which only columns [t0, n) are read, t0 =
 *                       max(0, n - W) rounded down to a multiple of 16; uid and temperature go into the header (word 10: the bits of
 *                       the temperature, zero for 1).  Asynchronous on `stream`: y and x stay alive until it has run, and the blobs
 *                       are complete when the stream has passed it (nvw_slot_resume / nvw_slots_resume_list read headers with
 *                       the ordering rules stated there).  Works inside and outside slot mode; calls of one engine share its
 *                       scratch (grown on demand, sized by W and count, freed with the engine): issue them on one stream, or order
 *                       them.  Needs nvw_set_conditioning_weights.  Returns count; 0 with nothing written: no conditioning weights,
 *                       count outside 1 .. 65535, an n < 1, a temperature outside [2^-10, 2^10], a bad precision, pointer,
 *                       alignment or stride.
 * A prefill from mel frames is nvw_prefill_states_mel (FROM MEL FRAMES, below).  Lockstep engines taking a prefilled state are not
 * offered; the per-sample log-likelihoods of a prime are a pass of their own (SCORING, below). */
typedef struct {
    const int* y;
    int n;
    const void* x;
    int precision;
    long long c_stride, t_stride;
    unsigned uid;
    float temperature;
} nvw_prefill_req;
int nvw_prefill_window(nvw_engine* e);
int nvw_prefill_states(nvw_engine* e, const nvw_prefill_req* reqs, int count, void* dst, long long stride, void* stream);

/* SCORING: PER-SAMPLE LOG-LIKELIHOODS FROM A TIME-PARALLEL PASS (additive within ABI 7).  What probability the model gives to a
 * waveform: logp[t] = log softmax(Za_t / T)[y[t]] (natural logarithm, fp32) for every t in [0, n), where Za_t are the logits of sample
 * t of a column that started from silence (history 128, 128), was fed y[0 .. t) and reads feature column t -- the logits the
 * generation kernel hands to its sampler at that sample when y is forced.  Every sample is known, so the pass runs layer by layer
 * over 16 samples at a time like the prefill pass, but over all of [0, n), through every layer, with the skip path, the head and the
 * softmax; it reads the engine's own weight streams and touches no ring, column or session.
 *   nvw_score_max_samples  the largest sum of n, each rounded up to a multiple of 16, that one call accepts: the scratch of a call
 *                          (per sample the fp32 residual, two T_data images of x and the fp32 skip sum) stays under 1 GiB.  0 when
 *                          the engine has no conditioning weights.
 *   nvw_score_samples      `count` requests with one set of layer launches.  y: the samples, int32 in device memory, n >= 1 values
 *                          (clamped into 0 .. A-1 as nvw_slot_prime clamps them); x, precision, c_stride, t_stride: the utterance's
 *                          features as for nvw_slot_start, columns [0, n); temperature: T.  logp: n floats, device memory or pinned
 *                          host memory, 4-byte aligned.  rows: NULL, or n * A floats in device memory, 16-byte aligned:
 *                          rows[t * A + a] = log softmax(Za_t / T)[a], and rows[t * A + y[t]] is logp[t] bit for bit.  Nothing is
 *                          written past n.  Asynchronous on `stream`: y, x and the outputs stay alive until it has run.  Works
 *                          inside and outside slot mode; calls of one engine share its scratch (grown on demand, freed with the
 *                          engine): issue them on one stream, or order them.  Needs nvw_set_conditioning_weights.  Returns count;
 *                          0 with nothing written and nothing launched: no conditioning weights, count outside 1 .. 65535, an
 *                          n < 1, a temperature outside [2^-10, 2^10], a bad precision or stride, y or x not in device memory, a
 *                          misaligned or unreachable output, a total over nvw_score_max_samples.
 * Scoring from mel frames is nvw_score_samples_mel (FROM MEL FRAMES, below); scoring in time chunks with carried state (utterances
 * past the cap, candidates behind a shared prefix, streams) is nvw_score_chunks (SCORING WITH CARRIED STATE, below).  Scoring on the
 * packed, in-place and chain conditioning paths is not offered. */
typedef struct {
    const int* y;
    int n;
    const void* x;
    int precision;
    long long c_stride, t_stride;
    float temperature;
    float* logp;
    float* rows;
} nvw_score_req;
int nvw_score_max_samples(nvw_engine* e);
int nvw_score_samples(nvw_engine* e, const nvw_score_req* reqs, int count, void* stream);

/* PREFILL AND SCORING FROM MEL FRAMES: A TIME-PARALLEL UPSAMPLING PASS (additive within ABI 7).  The two passes above read upsampled
 * features; the path that ships end to end (nvw_generate_stream, nvw_slot_start_mel) takes mel frames.  This pass upsamples by
 * REQUEST and SAMPLE RANGE: for frames mel[c * c_stride + f * f_stride] (`precision`-bit floats in device memory, n_cond channels,
 * `frames` of them written) and a range [first_sample, first_sample + count) it writes
 *     dst[(t - first_sample) * row + c] = b[c] + sum_{j < m} sum_ci mel[ci][f - j] W[ci][c][j * stride + r],   t = f * stride + r,
 * in the engine's precision, row = nvw_upsample_row_elems elements, channels >= n_cond exactly zero -- BIT FOR BIT what
 * nvw_upsample_features stores for that utterance and sample, and what a mel column's feed computes: the pass reads the engine's own
 * operand table and bias (no second copy of the weights) and sums in the same order.  Frames max(0, first_sample / stride - (m - 1))
 * .. (first_sample + count - 1) / stride are read, in place, and no others.  One launch per call.
 *   nvw_upsample_row_elems  16 * ceil(n_cond / 16); 0 without nvw_set_upsampling.
 *   nvw_upsample_requests   `count` requests (1 .. 65535); dst: count rows, 16-byte aligned device memory.  The rows are features as
 *                           nvw_prefill_states / nvw_score_samples / nvw_slot_start take them with precision = the engine's,
 *                           c_stride = 1, t_stride = row (for a range that starts at first_sample: x = dst - first_sample * row
 *                           elements).  Asynchronous on `stream`; mel and dst stay alive until it has run.
 *   nvw_prefill_states_mel  nvw_prefill_states from frames: the samples [t0, n) of every request are upsampled into an engine-owned
 *                           scratch (grown on demand, (n - t0) * row elements per request, freed with the engine), then the prefill
 *                           launches run on those rows.  The blob EQUALS, BYTE FOR BYTE, what nvw_slot_start_mel,
 *                           nvw_slot_set_temperature, nvw_slot_prime(y, n), steps up to local sample n and nvw_slot_save produce.
 *   nvw_score_samples_mel   nvw_score_samples from frames, range [0, n): accepts what nvw_score_max_samples accepts.  The feature
 *                           rows are an allocation of their own, row * sizeof(T_data) bytes per sample (160 B in fp16, 320 B in fp32
 *                           at 80 channels): at most nvw_score_max_samples * that, beside the 1 GiB of the scoring scratch.
 * Each returns count, or 0 with nothing written and nothing launched (every request check of both passes comes before the upsampling is
 * queued; should the feature pass itself then fail -- its scratch cannot be allocated, a launch is rejected -- the two mel entries
 * return 0 with the engine-owned rows already written, and nothing of the caller's): everything nvw_prefill_states / nvw_score_samples refuse, and
 * no nvw_set_upsampling, mel not in device memory, a non-positive stride, frames * stride short of the range (< first_sample + count,
 * or < n), first_sample < 0 or count < 1, dst not 16-byte aligned device memory.  All three work inside and outside slot mode, touch
 * no ring, column or session, and share the engine's scratch: issue them on one stream, or order them.  Scoring a time chunk of a mel
 * utterance from and to a state blob is nvw_score_chunks_mel (SCORING WITH CARRIED STATE, below). */
typedef struct {
    const void* mel;
    int precision;
    long long c_stride, f_stride;
    int frames;
    int first_sample, count;
    void* dst;
} nvw_upsample_req;
typedef struct {
    const int* y;
    int n;
    const void* mel;
    int precision;
    long long c_stride, f_stride;
    int frames;
    unsigned uid;
    float temperature;
} nvw_prefill_mel_req;
typedef struct {
    const int* y;
    int n;
    const void* mel;
    int precision;
    long long c_stride, f_stride;
    int frames;
    float temperature;
    float* logp;
    float* rows;
} nvw_score_mel_req;
int nvw_upsample_row_elems(nvw_engine* e);
int nvw_upsample_requests(nvw_engine* e, const nvw_upsample_req* reqs, int count, void* stream);
int nvw_prefill_states_mel(nvw_engine* e, const nvw_prefill_mel_req* reqs, int count, void* dst, long long stride, void* stream);
int nvw_score_samples_mel(nvw_engine* e, const nvw_score_mel_req* reqs, int count, void* stream);

/* SCORING WITH CARRIED STATE: TIME CHUNKS, FROM AND TO A STATE BLOB (additive within ABI 7).  nvw_score_samples starts from silence at
 * local sample 0 and leaves nothing behind.  Here a request is a CHUNK: y[0 .. n) are local samples done .. done + n - 1 of an
 * utterance, where done is that of `state` -- a blob of nvw_slot_save / nvw_slots_save_list / nvw_prefill_states* / this call -- or 0
 * when state is NULL (from silence).  The blob holds exactly what the chunk needs from before it (every layer's last d_l inputs and
 * the two history words), and everything else of the pass is per sample, so each sample is computed with the operands of the whole
 * pass in its order: logp and rows are BIT FOR BIT those nvw_score_samples gives for these samples in one pass over [0, done + n),
 * and state_out, where not NULL, is BYTE FOR BYTE the blob nvw_prefill_states gives for the first done + n samples (uid: the
 * in-state's, or the request's from silence; word 10: the request's temperature) -- it resumes, and scores on, like any other.
 *   nvw_score_chunks      `count` requests with one set of layer launches.  x holds the CHUNK's feature columns (column done + i at
 *                         index i).  done need not be a multiple of 16.  States are read only, and several requests may point at
 *                         one (candidates behind a shared prefix).  The headers of the states are read before anything is queued:
 *                         pinned ones in place, device ones with blocking copies on the null stream, each distinct pointer once,
 *                         pointers in an arithmetic progression (the rows of one earlier call) with one 2-D copy -- a state written
 *                         on a non-blocking stream must have been ordered before this call, as for nvw_slot_resume.  The pass uses
 *                         the scoring scratch: nvw_score_max_samples bounds the sum of n, each rounded up to 16, of a chunk call too.
 *                         Asynchronous on `stream`.  Returns count; 0 with nothing written and nothing launched: everything
 *                         nvw_score_samples refuses; a state with a wrong magic or layout version, of another precision, R, layer
 *                         count or largest dilation, with a header word 10 that is neither zero nor a valid temperature; a state
 *                         that is not device or pinned memory, or not 16-byte aligned; done + n beyond INT_MAX - 16; a state_out
 *                         that is misaligned, unreachable, or overlaps any state or another state_out of the call.
 *   nvw_score_chunks_mel  the same from frames: mel, precision, c_stride, f_stride, frames are the utterance's frames from frame 0
 *                         as nvw_score_samples_mel takes them; samples [done, done + n) are upsampled into the engine-owned rows.
 *                         Refuses what nvw_score_samples_mel and nvw_score_chunks refuse, and frames * stride < done + n. */
typedef struct {
    const void* state;
    const int* y;
    int n;
    const void* x;
    int precision;
    long long c_stride, t_stride;
    unsigned uid;
    float temperature;
    float* logp;
    float* rows;
    void* state_out;
} nvw_score_chunk_req;
typedef struct {
    const void* state;
    const int* y;
    int n;
    const void* mel;
    int precision;
    long long c_stride, f_stride;
    int frames;
    unsigned uid;
    float temperature;
    float* logp;
    float* rows;
    void* state_out;
} nvw_score_chunk_mel_req;
int nvw_score_chunks(nvw_engine* e, const nvw_score_chunk_req* reqs, int count, void* stream);
int nvw_score_chunks_mel(nvw_engine* e, const nvw_score_chunk_mel_req* reqs, int count, void* stream);

/* hipDeviceSynchronize() for hosts without a HIP binding */
void nvw_device_synchronize(void);
/* time `reps` back-to-back nvw_run() launches with HIP events on `stream`; returns milliseconds
 * for all reps (used by bench.py: events on the stream the kernel is launched on) */
float nvw_time_runs(nvw_engine* e, int reps, int num_samples, int batch_size, int batch_size_per_block,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
