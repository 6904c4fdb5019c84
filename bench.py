#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X WaveNet inference engine.

Metric (BASELINE.json): samples/sec/GPU and max real-time batch @24 kHz at R=64/S=256/A=256,
20 layers, maxDilation 512, fp16.  One "step" = one run() launch of the hot path generating
SAMPLES_PER_STEP samples for every utterance of the batch (synthetic conditioning / selectors /
random-init weights already resident in HBM).  `value` = utterances x samples / second over all
GPUs, measured at the largest batch whose per-utterance rate stays >= 24 kHz AT STEADY STATE: the
reference times N = 16 384 samples with maxDilation 512 (nv_wavenet_perf.cu:195-199), where every
dilated tap is live and every ring has wrapped, so a batch counts as real time only if samples
640 .. 1151 of an utterance (all d = 512 taps live) are generated at >= 24 kHz (`steady_state`; found
by a bounded bisection over the number of 16-utterance tiles before the timed region; override with
--batch), and the timed steps themselves continue one long utterance from sample 640 on.

Beside it (rank 0, N = 1 only) the reference's own measurement is reproduced for the BASELINE configs
C2 / C3 / C4 (`reference_definition`): nv_wavenet_perf.cu:67-87 -- 16 384 samples through run_chunks in
chunks of 2 048 with the per-chunk copies of the samples to pinned host memory inside the timed region,
kHz per utterance = samples / elapsed ms -- for the single-workgroup and the multi-CU organisation; and
`end_to_end`: the largest real-time batch when the conditioning is NOT pre-packed but streamed chunk by
chunk (fp32 [N][L][B][2R] on the device -> fragment order, packed on a second stream behind the
generation of the previous chunk).

Multi-GPU: `python bench.py --gpus N` spawns its own N ranks (torch.distributed.run, one process per
GPU, 127.0.0.1 rendezvous) unless it already runs under a launcher (WORLD_SIZE set).  Utterances shard
with no data-path collective (weak scaling: every GPU runs the same per-GPU batch; `--config c5`: the
BASELINE C5 point, global batch 64 split over the ranks); each step ends with ONE RCCL all_gather of
the [B/G][N] int32 sample blocks, overlapped with the next step.  n_gpus is reported only after an
all_gather of the ranks' device ids proved that N distinct processes took part.

Timing: W warm-up steps, then barrier + synchronize, K timed steps, synchronize + barrier, MAX
over ranks.  The dominant kernel's launch duration is measured live with HIP events on the stream
it is launched on, and feeds `roofline`.  `cpu_baseline` times the reference's own CPU
implementation (oracle/_ref when present, else the C restatement oracle/) on one host core over a
bounded sample of the same workload shape (rank 0, N=1 only).

Plain run and --full: `bench.py --gpus 1 --steps K --warmup W` does only what the headline needs -- it
builds the engine, warms up, times the K steps and prints the result line (`value`, `ms_per_step`,
`khz_per_utterance`, ...).  Its batch is three tiles of 16 utterances per CU (48 x CUs; 12 288 on an
MI355X), the batch the real-time sweep settles on, so that the same arguments always time the same
workload.  `--full` adds everything else as before: the real-time batch sweep (and times the batch
it picks), `reference_definition`, `end_to_end`, `dropin_fp32`, `oversubscribed`, the socket-power
reading, `roofline` and `cpu_baseline`.
--dump-outputs DIR: after the timed steps, the samples of the last timed step (what a caller of the
timed path receives, [batch][samples per step]) go to DIR/samples.npy as float32; above 64 MB, a
fixed, seeded sample of utterances (their indices in DIR/samples_rows.npy).  Weights, conditioning
and selectors are seeded: the same arguments give the same inputs on every run.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

REALTIME_KHZ = 24.0
HBM_PEAK_GBS = 8000.0                         # MI355X_MICROARCH.md: 8 TB/s spec
MFMA_F16_PEAK_TFLOPS = 2500.0                 # dense fp16/bf16 MFMA peak
L2_PEAK_GBS = 34500.0                         # aggregate L2 bandwidth (guide, measured)
LDS_PEAK_GBS = 256 * 256 * 2.4                # 256 B/clk/CU x 256 CUs x 2.4 GHz (guide, LDS section)


class Shape:
    """A BASELINE.json config: channel counts, depth, dilation range."""

    def __init__(self, name, R, S, A, L, maxD, B):
        self.name, self.R, self.S, self.A, self.L, self.maxD, self.B = name, R, S, A, L, maxD, B
        # algorithmic work per sample per utterance (SURVEY.md 8d / BASELINE.md)
        self.macs = L * (5 * R * R + S * R) + A * S + A * A
        self.flops = 2 * self.macs
        self.weight_bytes = 2 * self.macs                 # fp16 weights touched per tile pass
        self.hbm_bytes = 2 * 2 * R * L + 4 + 4            # cond (fp16) + selector + yOut


C2 = Shape("C2", 64, 128, 256, 20, 512, 4)
C3 = Shape("C3", 64, 256, 256, 20, 512, 16)
C4 = Shape("C4", 128, 256, 256, 30, 512, 8)
HEAD = C3                                     # the shape the headline metric is quoted on
R, S, A, L, MAXD = HEAD.R, HEAD.S, HEAD.A, HEAD.L, HEAD.maxD
# the device code the engine launches for the headline point (asserted against nvw_kernel_info, and pinned
# by tests/test_parity_gpu.py::test_benchmarked_launch_*: the timed kernel is the parity-tested one)
HEADLINE_KERNELS = {2: "wn::wavenet_wg<fp16,64,256,256,BT=2,EMBLDS=1,DUMP=0,RAW=0,LR=1>",     # by tiles per workgroup
                    3: "wn::wavenet_wg<fp16,64,256,256,BT=3,EMBLDS=1,DUMP=0,RAW=0,LR=1>",
                    4: "wn::wavenet_wg<fp16,64,256,256,BT=4,EMBLDS=0,DUMP=0,RAW=0,LR=1>"}
HEADLINE_KERNEL = HEADLINE_KERNELS[2]


def lds_bytes_per_sample(bt=1):
    """Algorithmic LDS bytes moved per generated sample per WORKGROUP (C3 shape, fp16).
    wg kernel (4 waves on bt tiles): per layer every wave reads the x, x[t-d] and h fragment images
    (R/32 KiB each) and its bias quads, and writes its quarter of h, x and the dilated tap; the head
    moves skip / zs images (S/32, A/32 KiB, read by all 4 waves) and the fp32 logits once each way."""
    kf = lambda n: n // 32 * 1024
    per_layer = bt * (4 * 3 * kf(R) + 3 * kf(R)) + 4 * 64 * 16 * 3        # exchanges + bias quads
    head = bt * (5 * kf(S) + 5 * kf(A) + 2 * 16 * A * 4 + 2 * kf(R)) + 4 * 64 * 16 * (S // 64 + 2 * A // 64)
    return L * per_layer + head


COND_STD = 0.5                                # conditioning: uniform with this standard deviation


def make_weights(sh=HEAD, seed=3):
    """Random-init weights at the magnitudes of a trained network (uniform draws, fan-in scaled like the parity tests'
    O(1) recipe, tests/util.py:o1_recipe): activations and logits of order one in every layer, all 256 bins in play --
    under the reference's +-0.25/rows recipe (nv_wavenet_test.cu:36-111) the logits are a constant and the output a
    uniform distribution whatever the network computes."""
    rng = np.random.default_rng(seed)
    R, S, A, L = sh.R, sh.S, sh.A, sh.L
    u = lambda std, *s: ((rng.random(s, dtype=np.float32) - 0.5) * (std * np.sqrt(12.0))).astype(np.float32)
    w = dict(embP=u(0.45, A, R), embC=u(0.45, A, R),
             Wprev=u(0.55 / np.sqrt(R), L, R, 2 * R), Wcur=u(0.55 / np.sqrt(R), L, R, 2 * R), Bh=u(0.3, L, 2 * R),
             Wres=u(0.5 / np.sqrt(R), L, R, R), Bres=u(0.05, L, R), Wskip=u(1.5 / np.sqrt(R * L), L, R, S), Bskip=u(0.3 / np.sqrt(L), L, S),
             Wzs=u(1.6 / np.sqrt(S), S, A), Bzs=u(0.2, A), Wza=u(1.5 / np.sqrt(A), A, A), Bza=u(0.2, A))
    return w


N_COND = 80                                   # feature channels of the reference's model (pytorch/config.json: n_cond_channels)


def make_cond_layers(sh=HEAD, seed=4):
    """The model's conditioning convolution (cond_layers: [2R*L][n_cond] + bias) at magnitudes that give the conditioning the
    standard deviation COND_STD for features of unit variance."""
    rng = np.random.default_rng(seed)
    u = lambda std, *s: ((rng.random(s, dtype=np.float32) - 0.5) * (std * np.sqrt(12.0))).astype(np.float32)
    return u(COND_STD / np.sqrt(N_COND), 2 * sh.R * sh.L, N_COND), u(0.1, 2 * sh.R * sh.L)


def build_engine(w, B, N, sh=HEAD, precision=16, impl=0, organisation=0):
    from nv_wavenet_amd import WavenetEngine
    e = WavenetEngine(sh.R, sh.S, sh.A, sh.L, sh.maxD, B, N, impl=impl, tanhEmbed=True, precision=precision,
                      organisation=organisation)
    e.setEmbeddings(w["embP"], w["embC"])
    for l in range(sh.L):
        e.setLayerWeights(l, w["Wprev"][l], w["Wcur"][l], w["Bh"][l], w["Wres"][l], w["Bres"][l], w["Wskip"][l],
                          w["Bskip"][l])
    e.setOutWeights(w["Wzs"], w["Bzs"], w["Wza"], w["Bza"])
    return e


def device_inputs(B, N, seed, sh=HEAD):
    """Synthetic conditioning [N][L][B][2R] (uniform, standard deviation COND_STD) and selectors [N][B] in HBM."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    Lh = torch.empty(N, sh.L, B, 2 * sh.R, dtype=torch.float32, device="cuda")
    hw = COND_STD * 3.0 ** 0.5
    Lh.uniform_(-hw, hw, generator=g)
    sel = torch.rand(N, B, dtype=torch.float32, device="cuda", generator=g)
    return Lh, sel


def samples_per_step_for(B):
    # keep the packed conditioning of STEADY_FROM + n samples under ~60 GB
    per_sample = L * B * 2 * R * 2
    n = int(60e9 // per_sample) - STEADY_FROM
    n = max(64, min(2048, n // 64 * 64))
    return n


def measure_khz(w, B, N, seed=11, organisation=0):
    """per-utterance kHz of one launch of N samples FROM SAMPLE 0 at batch B with pre-packed conditioning (HIP events on
    the launch stream).  organisation: 0 = the engine's own choice, else a forced nvwOrganisation."""
    import torch
    e = build_engine(w, B, N, organisation=organisation)
    Lh, sel = device_inputs(B, N, seed)
    e.setInputs(Lh, sel)
    del Lh
    torch.cuda.synchronize()
    e.time_runs(1, min(N, 64), B)
    ms = e.time_runs(1, N, B)
    info = e.kernelInfo(B, False)
    e.close()
    torch.cuda.empty_cache()
    return N / ms, info


# ---- steady state ----------------------------------------------------------------------------------------------------
# The reference's figure is N = 16 384 samples with maxDilation 512 (nv_wavenet_perf.cu:67-87,195-199): after the first
# 512 samples every dilated tap is live and every ring has wrapped.  A launch restarted at t = 0 never loads the taps with
# d >= its length.  So: an engine of capacity STEADY_FROM + n, conditioning for all of it, samples 0 .. STEADY_FROM-1
# generated untimed, and what is timed is samples STEADY_FROM .. STEADY_FROM+n-1.
STEADY_FROM = 640
COND_BLOCK = 64                               # samples per reused fp32 source block of synthetic conditioning


def steady_engine(w, B, n_timed, seed=11, in_place=None, organisation=0, sh=None, impl=0):
    """Engine at batch B with samples 0 .. STEADY_FROM-1 behind it.  in_place: None = conditioning packed (chunk-wise from
    one reused COND_BLOCK-sample fp32 block: the packed copy of STEADY_FROM + n_timed samples is what stays in HBM, 5 120 B
    per utterance and sample), or torch.float32 / torch.float16 = a full [N][L][B][2R] tensor of that type consumed in
    place.  Returns (engine, total samples, keep-alive)."""
    import torch
    N = STEADY_FROM + n_timed
    sh = sh or HEAD                           # (shapes other than the headline's: packed conditioning only)
    assert sh is HEAD or in_place is None
    e = build_engine(w, B, N, sh=sh, organisation=organisation, impl=impl)
    block, _ = device_inputs(B, COND_BLOCK, seed, sh=sh)
    e.setSelectorSeed(seed)
    keep = None
    if in_place is None:
        e.resetHistory()
        for first in range(0, N, COND_BLOCK):
            e.packConditioning(block[:min(COND_BLOCK, N - first)], first, min(COND_BLOCK, N - first))
    elif in_place == "features":
        # the conditioning computed in the generation kernel (round 5): the engine gets cond_layers once and, per sample and
        # utterance, N_COND upsampled feature values (unit variance, one reused COND_BLOCK-sample block)
        Wc, bc = make_cond_layers()
        e.setConditioningWeights(Wc, bc)
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + 1)
        xb = torch.randn(B, N_COND, COND_BLOCK, dtype=torch.float32, device="cuda", generator=g).half()
        e.resetHistory()
        for first in range(0, N, COND_BLOCK):
            e.packFeatures(xb[:, :, :min(COND_BLOCK, N - first)], first)
        del xb
    elif in_place == "fragments":
        # the caller's own buffer in the engine's fragment order (what a model's conditioning convolution emits with the
        # channel permutation and the gate pre-scale folded into its weights: nv_wavenet.py get_cond_input(layout="packed"))
        from nv_wavenet_amd.nv_wavenet import pack_cond_input
        tiles = e.condTiles()
        keep = torch.zeros(N + 1, L, tiles, 2 * R // 32, 4, 16, 8, dtype=torch.float16, device="cuda")
        for first in range(0, N, COND_BLOCK):
            n = min(COND_BLOCK, N - first)
            keep[first:first + n].copy_(pack_cond_input(block[:n], 16, tiles)[:n])
        e.setConditioningPacked(keep, N)
    else:
        keep = torch.empty(N, L, B, 2 * R, dtype=in_place, device="cuda")
        for first in range(0, N, COND_BLOCK):
            keep[first:first + COND_BLOCK].copy_(block[:min(COND_BLOCK, N - first)])
        e.setConditioningDirect(keep)
    del block
    torch.cuda.synchronize()
    assert e.run_partial_chunk(0, STEADY_FROM, N, B)
    e.synchronize()
    return e, N, keep


def time_range(e, first, count, N, B, reps=1):
    """HIP-event milliseconds per launch of samples [first, first + count) on torch's current stream"""
    import torch
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        assert e.run_partial_chunk(first, count, N, B, st.cuda_stream)
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure_steady_khz(w, B, n_timed=512, seed=11, in_place=None, organisation=0, sh=None, impl=0):
    """per-utterance kHz over samples STEADY_FROM .. STEADY_FROM + n_timed - 1 (all taps live, all rings wrapped)"""
    import torch
    e, N, keep = steady_engine(w, B, n_timed, seed, in_place, organisation, sh, impl)
    ms = time_range(e, STEADY_FROM, n_timed, N, B)
    info = e.kernelInfo(B, False)
    ok = e.chainStatus() == 0
    e.close()
    del keep
    torch.cuda.empty_cache()
    return (n_timed / ms) if ok else 0.0, info


def reference_definition_khz(sh, impl, N=16384, chunk=2048):
    """nv_wavenet_perf.cu:67-87: N samples through run_chunks in chunks of `chunk`, per-chunk copies of the
    samples into pinned host memory, wall clock around it; kHz per utterance = N / elapsed ms."""
    import torch
    w = make_weights(sh, seed=1)
    e = build_engine(w, sh.B, N, sh=sh, impl=impl)
    Lh, sel = device_inputs(sh.B, N, 1, sh=sh)
    e.setInputs(Lh, sel)
    y = torch.zeros(sh.B, N, dtype=torch.int32).pin_memory()
    e.run(min(N, 64), sh.B)                    # warm-up (code objects, clocks)
    e.synchronize()
    e.setInputs(Lh, sel)
    e.setClockProbe(True)
    del Lh
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ok = e.run_chunks(chunk, None, N, sh.B, y.numpy(), 1)
    e.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    info = e.kernelInfo(sh.B, False)
    ghz = e.lastLaunchClockGHz()
    ok = ok and e.chainStatus() == 0 and int(y.min()) >= 0 and int(y.max()) < sh.A and int(torch.unique(y).numel()) > 8
    e.close()
    torch.cuda.empty_cache()
    return {"khz_per_utterance": (N / ms) if ok else 0.0, "samples_per_sec": (sh.B * N / ms * 1e3) if ok else 0.0,
            "kernel": info, "samples": N, "chunk": chunk, "batch": sh.B, "shader_clock_ghz": round(ghz, 3)}


def dropin_fp32(sh, L=None, maxD=None, B=8, N=10000):
    """The reference's own PyTorch entry, timed as its user calls it: NVWaveNet(**export_weights()).infer(cond, impl)
    -> nv_wavenet_ext.infer -> wavenet_infer() of libwavenet_infer.so (pytorch/nv_wavenet.py:172-196, wavenet_infer.cu:105-143) -- fp32,
    the engine built, loaded and destroyed INSIDE the call, the conditioning a CUDA tensor, libc rand() selectors -- on the workload of
    pytorch/integration_test.py:37-52 (batch 8, 10 000 samples, conditioning of zeros there, seeded here).  Wall clock around infer(),
    after one short call that loads the code objects; kHz per utterance = N / elapsed ms like nv_wavenet_perf.cu:87."""
    import torch
    from nv_wavenet_amd.nv_wavenet import NVWaveNet, Impl
    L = L or sh.L
    maxD = maxD or sh.maxD
    R, S, A = sh.R, sh.S, sh.A
    g = torch.Generator().manual_seed(5)
    u = lambda std, *shape: ((torch.rand(*shape, generator=g) - 0.5) * (std * 12.0 ** 0.5)).cuda()
    kw = dict(embedding_prev=u(0.45, A, R), embedding_curr=u(0.45, A, R), conv_out_weight=u(1.6 / S ** 0.5, A, S, 1),
              conv_end_weight=u(1.5 / A ** 0.5, A, A, 1), dilate_weights=[u(0.55 / R ** 0.5, 2 * R, R, 2) for _ in range(L)],
              dilate_biases=[u(0.3, 2 * R) for _ in range(L)], max_dilation=maxD,
              res_weights=[u(0.5 / R ** 0.5, R, R, 1) for _ in range(L - 1)], res_biases=[u(0.05, R) for _ in range(L - 1)],
              skip_weights=[u(1.5 / (R * L) ** 0.5, S, R, 1) for _ in range(L)], skip_biases=[u(0.3 / L ** 0.5, S) for _ in range(L)],
              use_embed_tanh=True)
    model = NVWaveNet(**kw)
    out = {"definition": "NVWaveNet(**weights).infer(cond_input, impl) of the reference's PyTorch path on this library: fp32, engine construction + "
                         "weight upload + conditioning pack + generation + teardown inside the call (wavenet_infer()); R%d S%d A%d, %d layers, "
                         "maxDilation %d, batch %d, %d samples (pytorch/integration_test.py:37-52); wall clock, kHz per utterance"
                         % (R, S, A, L, maxD, B, N)}
    hw = COND_STD * 3.0 ** 0.5
    cond = (torch.rand(2 * R, B, L, N, generator=g) * 2 - 1).mul_(hw).cuda()
    for name, impl in (("persistent", Impl.PERSISTENT), ("auto", Impl.AUTO), ("single_block", Impl.SINGLE_BLOCK), ("manyblock", 4)):
        model.infer(cond[:, :, :, :64].contiguous(), impl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = model.infer(cond, impl)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        ok = int(y.min()) >= 0 and int(y.max()) < A and int(torch.unique(y).numel()) > 8
        out[name] = {"khz_per_utterance": (N / ms) if ok else 0.0, "ms": ms, "samples_per_sec": (B * N / ms * 1e3) if ok else 0.0}
    del cond
    # ... and the generation alone, for scale: the same fp32 engine through the handle API, run() of N samples (dump-free kernel)
    w = make_weights(Shape(sh.name, R, S, A, L, maxD, B), seed=1)
    shl = Shape(sh.name, R, S, A, L, maxD, B)
    e = build_engine(w, B, N, sh=shl, precision=32, impl=3)
    Lh, sel = device_inputs(B, N, 1, sh=shl)
    e.setInputs(Lh, sel)
    e.run(64, B)
    e.synchronize()
    e.setInputs(Lh, sel)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run(N, B)
    e.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    out["generation_only"] = {"khz_per_utterance": N / ms, "ms": ms, "kernel": e.kernelInfo(B, False)}
    e.close()
    del Lh, sel
    torch.cuda.empty_cache()
    best = max(("persistent", "auto", "single_block", "manyblock"), key=lambda k: out[k]["khz_per_utterance"])
    out["khz_per_utterance"] = out["persistent"]["khz_per_utterance"]      # (what integration_test.py asks for: Impl.PERSISTENT)
    out["best_implementation"] = best
    return out


def end_to_end_khz(w, B, chunk=256, chunks=4, seed=21):
    """Conditioning streamed per chunk: the fp32 [chunk][L][B][2R] block of chunk j+1 is packed into fragment
    order on a second stream while chunk j is generated; the samples of every chunk are copied to the host.
    Returns kHz per utterance over chunks*chunk samples (the first chunk's pack is inside the timed region)."""
    import torch
    N = chunk * chunks
    e = build_engine(w, B, N)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    blocks = [torch.empty(chunk, L, B, 2 * R, dtype=torch.float32, device="cuda").uniform_(-COND_STD * 3.0 ** 0.5, COND_STD * 3.0 ** 0.5, generator=g)
              for _ in range(2)]                       # two source buffers, refilled round-robin (synthetic)
    sel = torch.rand(N, B, dtype=torch.float32, device="cuda", generator=g)
    e.setSelectorSeed(seed)
    del sel
    gen, pack = torch.cuda.Stream(), torch.cuda.Stream()
    y = torch.zeros(B, N, dtype=torch.int32, device="cuda")
    # warm-up: one chunk through both paths
    e.packConditioning(blocks[0], 0, chunk, pack.cuda_stream)
    pack.synchronize()
    e.run_partial_chunk(0, chunk, N, B, gen.cuda_stream)
    gen.synchronize()
    e.resetHistory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    packed = [torch.cuda.Event() for _ in range(chunks)]
    done = [torch.cuda.Event() for _ in range(chunks)]
    e.packConditioning(blocks[0], 0, chunk, pack.cuda_stream)
    packed[0].record(pack)
    for j in range(chunks):
        gen.wait_event(packed[j])
        e.run_partial_chunk(j * chunk, chunk, N, B, gen.cuda_stream)
        done[j].record(gen)
        if j + 1 < chunks:
            if j >= 1:
                pack.wait_event(done[j - 1])      # (the source buffer of chunk j+1 was read by the pack of chunk j-1)
            e.packConditioning(blocks[(j + 1) % 2], (j + 1) * chunk, chunk, pack.cuda_stream)
            packed[j + 1].record(pack)
    gen.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    e.getYOut(y, 0, N, None)
    torch.cuda.synchronize()
    ok = int(torch.unique(y).numel()) > 8
    e.close()
    del blocks
    torch.cuda.empty_cache()
    return (N / ms) if ok else 0.0


UP_STRIDE, UP_WINDOW = 256, 1024             # upsampling of the synthetic model (the reference's is 200 / 800: the same four taps)


def features_in_khz(w, B, chunk=256, chunks=8, seed=41):
    """The deployable loop of round 5: FEATURES IN, SAMPLES OUT through one C-ABI call (nvw_generate_stream).  The engine holds the
    model's `upsample` and `cond_layers` (pytorch/wavenet.py:70-74); per chunk of `chunk` samples it upsamples the mel-like frames
    [B][80][frames] (fp16) with its own MFMA kernel into feature fragments, runs the generation launch -- which computes the
    conditioning itself, wavenet_wg<.., RAW=3> -- and copies the chunk's samples out on a second stream.  Nothing else touches the
    GPU: no [N][L][B][2R] tensor exists.  Wall clock around the call; returns (kHz per utterance, kernel)."""
    import torch
    N = chunk * chunks
    e = build_engine(w, B, N)
    Wc, bc = make_cond_layers()
    e.setConditioningWeights(Wc, bc)
    rng = np.random.default_rng(seed)
    up_w = ((rng.random((N_COND, N_COND, UP_WINDOW), dtype=np.float32) - 0.5) * (np.sqrt(12.0) / np.sqrt(4 * N_COND))).astype(np.float32)
    e.setUpsampling(up_w, np.zeros(N_COND, dtype=np.float32), UP_STRIDE)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mel = torch.randn(B, N_COND, N // UP_STRIDE, device="cuda", generator=g).half()
    e.setSelectorSeed(seed)
    y = torch.zeros(B, N, dtype=torch.int32, device="cuda")
    e.setMel(mel)
    assert e.generate_stream(min(64, chunk), None, min(64, chunk), B, None)       # warm-up (code objects, buffers)
    e.setMel(mel)                                                                 # (history back to the start)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ok = e.generate_stream(chunk, None, N, B, y)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    info = e.kernelInfo(B, False)
    ok = ok and int(torch.unique(y).numel()) > 8 and "RAW=3" in info
    e.close()
    del mel, y
    torch.cuda.empty_cache()
    return ((N / ms) if ok else 0.0), info


def with_producer_khz(w, B, chunk=256, chunks=4, seed=31):
    """The deployable loop with the conditioning PRODUCER in it (VERDICT r3 #3 i): a WaveNet's conditioning is the output of its
    own upsampling + 1x1 `cond_layers` convolution (pytorch/wavenet.py:190-202).  Per chunk of `chunk` samples,
    nv_wavenet.get_cond_input(layout="packed", out=...) runs that model part on the GPU (mel-like features [B][80][frames],
    fp16 weights with the engine's channel permutation and gate pre-scale folded in) and lands its output in the engine's
    fragment order inside the buffer the generation kernel reads (setConditioningPacked): no re-layout, no second pass.  Every
    CU holds a generation workgroup for a whole launch, so the producer of chunk j+1 can only run BETWEEN the generation
    launches of chunks j and j+1, on the same stream; chunk 0's production is inside the timed region as well.
    Returns kHz per utterance over chunks * chunk samples."""
    import torch
    from nv_wavenet_amd.nv_wavenet import get_cond_input
    N = chunk * chunks
    n_cond, stride, window = 80, 256, 1024
    assert chunk % stride == 0
    frames = chunk // stride
    e = build_engine(w, B, N)
    tiles = e.condTiles()
    Bp = tiles * 16
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    h = torch.float16
    feats = [(torch.rand(Bp, n_cond, frames, device="cuda", generator=g) - 0.5).to(h) for _ in range(2)]
    up_w = ((torch.rand(n_cond, n_cond, window, device="cuda", generator=g) - 0.5) * 0.05).to(h)
    up_b = torch.zeros(n_cond, device="cuda", dtype=h)
    cw = ((torch.rand(2 * R * L, n_cond, 1, device="cuda", generator=g) - 0.5) * 0.5).to(h)
    cb = torch.zeros(2 * R * L, device="cuda", dtype=h)
    frags = torch.zeros(N + 1, L, tiles, 2 * R // 32, 4, 16, 8, dtype=h, device="cuda")

    def produce(j):
        get_cond_input(feats[j % 2], up_w, up_b, stride, cw, cb, L, layout="packed", precision=16, tiles=tiles,
                       out=frags[j * chunk:(j + 1) * chunk])
    produce(0)                                   # warm-up of both paths (kernels, workspaces)
    torch.cuda.synchronize()
    e.setConditioningPacked(frags, N)
    e.setSelectorSeed(seed)
    st = torch.cuda.current_stream()
    e.run_partial_chunk(0, min(64, chunk), N, B, st.cuda_stream)
    torch.cuda.synchronize()
    e.resetHistory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    produce(0)
    for j in range(chunks):
        assert e.run_partial_chunk(j * chunk, chunk, N, B, st.cuda_stream)
        if j + 1 < chunks:
            produce(j + 1)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    y = torch.zeros(B, N, dtype=torch.int32, device="cuda")
    e.getYOut(y, 0, N, None)
    torch.cuda.synchronize()
    ok = int(torch.unique(y).numel()) > 8
    e.close()
    del frags, feats
    torch.cuda.empty_cache()
    return (N / ms) if ok else 0.0


def cpu_run_once(w, n, B=16, seed=5):
    """n samples of the C3 shape at batch B on the calling core: (seconds, kind)."""
    from oracle import oracle as O
    kind = "reference" if O.have_ref() else "port"
    cls = O.RefOracle if kind == "reference" else O.Oracle
    rng = np.random.default_rng(seed)

    class T:
        pass
    t = T()
    for k, v in w.items():
        setattr(t, k, v)
    Lh = ((rng.random((n, L, B, 2 * R), dtype=np.float32) - 0.5) * (COND_STD * np.sqrt(12.0))).astype(np.float32)
    sel = rng.random((n, B), dtype=np.float32) * 0.999
    o = cls(L, B, n, R, S, A, MAXD)
    o.set_model(t)
    o.set_inputs(Lh, sel)
    t0 = time.perf_counter()
    o.run(n)
    dt = time.perf_counter() - t0
    o.close()
    return dt, kind


def cpu_baseline(w, budget_s=20.0):
    """The reference's CPU implementation (nv_wavenet_reference.cpp built into oracle/_ref), C3 shape,
    batch 16, bounded sample: on ONE host core (the reference's own single-threaded path = the reported
    value), then one instance per host core on independent batch slices, as
    sub-object all_cores."""
    import subprocess
    B = 16
    dt, kind = cpu_run_once(w, 4)
    n = int(max(8, min(512, budget_s / (dt / 4))))
    dt, kind = cpu_run_once(w, n)
    out = dict(value=B * n / dt, unit="samples/s", cores=1, kind=kind,
               sample="R%d/S%d/A%d L%d maxD%d fp32, batch %d x %d samples (%.1f s)" % (R, S, A, L, MAXD, B, n, dt),
               khz_per_utterance=n / dt / 1e3)
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = min(cores, 64)
    if cores > 1:
        # separate interpreters (no torch, no HIP): a fork of this process would carry the GPU runtime
        n2 = max(8, n // 4)
        t0 = time.perf_counter()
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(n2), "--cpu-seed", str(i)],
                                  stdout=subprocess.PIPE, cwd=ROOT) for i in range(cores)]
        ok = 0
        for pr in procs:
            so, _ = pr.communicate()
            ok += pr.returncode == 0 and b"cpu_worker_seconds" in so
        wall = time.perf_counter() - t0
        if ok == cores:
            out["all_cores"] = dict(value=cores * B * n2 / wall, unit="samples/s", cores=cores,
                                    sample="%d processes x batch %d x %d samples, wall %.1f s incl. start-up" % (cores, B, n2, wall))
    return out


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(args):
    """`python bench.py --gpus N` outside a launcher: run torch.distributed.run with N local ranks as a child process
    (a fresh process, not an exec of this one, which may already have opened the GPU runtime) and exit with its status."""
    if args.backend == "nccl":
        import torch
        have = torch.cuda.device_count()
        if have < args.gpus:
            sys.exit("bench.py: --gpus %d but only %d GPU(s) are visible" % (args.gpus, have))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd)
    sys.exit(rc if rc >= 0 else 128 - rc)          # (a child killed by signal s: 128 + s, like a shell)


def prove_world(dist, world, rank, local_rank, backend):
    """All ranks exchange (rank, pid, device) through the collective backend: the job really has `world`
    distinct processes (and, under RCCL, distinct devices).  Returns the gathered table on every rank."""
    import torch
    dev = "cuda" if backend == "nccl" else "cpu"
    mine = torch.tensor([rank, os.getpid(), local_rank], dtype=torch.int64, device=dev)
    flat = torch.zeros(world * 3, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(flat, mine)
    table = flat.cpu().reshape(world, 3)
    ranks = sorted(int(x) for x in table[:, 0])
    assert ranks == list(range(world)), "rendezvous incomplete: ranks %s of %d" % (ranks, world)
    assert len(set(int(x) for x in table[:, 1])) == world, "ranks share a process"
    if backend == "nccl":
        assert len(set(int(x) for x in table[:, 2])) == world, "ranks share a GPU"
    return table


def selftest_dist(args, world, rank, local_rank):
    """Launcher / rendezvous / gather plumbing without the engine (no GPU needed): every rank contributes a
    [b][n] block of its own rank number through nv_wavenet_amd.sharding.gather_samples; prints one JSON line."""
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(args.backend)
        prove_world(dist, world, rank, local_rank, args.backend)
    sys.path.insert(0, ROOT)
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvw_sharding", os.path.join(ROOT, "nv_wavenet_amd", "sharding.py"))
    sharding = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sharding)
    b, n = 8, 32
    y = torch.full((b, n), rank, dtype=torch.int32)
    full = y
    if world > 1:
        full, _ = sharding.gather_samples(y, b * world)
        dist.barrier()
    ok = full.shape == (b * world, n) and all(int(full[r * b, 0]) == r for r in range(world))
    if rank == 0:
        print(json.dumps({"metric": "selftest (launcher + rendezvous + gather, no engine)", "n_gpus": world,
                          "gathered_rows": int(full.shape[0]), "ok": bool(ok)}))
    if world > 1:
        dist.destroy_process_group()
    if not ok:
        sys.exit(1)


def energy_roofline(power, kern_ms, B, N, bt, features=False, ring_layers_in_hbm=None):
    """The roof that binds the full-chip launch: the socket's power limit.  At the limit a sample takes
    (joules it costs) / (watts the socket grants), so the figure of merit is energy per utterance-sample against the energy the
    ALGORITHM needs at this chip's prices -- the marginal energy of an MFMA, a vector instruction, a transcendental, an LDS / L2 / HBM
    byte, measured by scripts/energy_ubench.py at the headline kernel's occupancy (profiles/r06_energy_ubench.json/.txt).
      achieved_uj = (socket W while the timed launch repeats - socket W of resident, idle waves) x seconds per launch / utterance-samples
      floor_uj    = SURVEY.md 8(d)'s algorithmic counts per utterance-sample x those prices: MACs (as 16x16x32 MFMAs), transcendentals,
                    the vector operations of gate / ReLU / softmax / conversions, LDS bytes of the activation exchanges, the weight
                    stream of this organisation (weights per pass / utterances per pass), compulsory HBM bytes
    and `floor_with_ring_uj` adds the dilation ring this design keeps in HBM (read x[t-d], write x[t])."""
    path = os.path.join(ROOT, "profiles", "r06_energy_ubench.json")
    if not power or "socket_w" not in power or not os.path.exists(path):
        return None
    try:
        doc = json.load(open(path))
        pr = doc["prices"]["256"]
        nj = lambda k: pr[k]["pj_per_op"] * 1e-3                       # nJ per op
        base_w = pr["loop"]["socket_w"]
        units = B * N
        achieved_total = power["socket_w"] * power["ms_per_launch"] * 1e-3 / units * 1e6
        achieved = (power["socket_w"] - base_w) * power["ms_per_launch"] * 1e-3 / units * 1e6
        sh = HEAD
        mfma = sh.macs / 8192.0                                          # v_mfma_f32_16x16x32_f16 per utterance-sample
        trans = (2 * sh.R * sh.L + sh.R + sh.A) / 64.0                   # wave instructions (64 lanes)
        # vector operations per utterance-sample: gate (two adds, an fma, a product per output), fp16 conversions of x / h / skip / zs,
        # ReLUs, softmax (fma, add, compare, add per logit)
        valu = (4 * sh.R * sh.L + 2 * sh.R * sh.L + 2 * (sh.S + sh.A) + 4 * sh.A) / 64.0
        lds_b = lds_bytes_per_sample(bt) / (16.0 * bt)
        w_b = sh.weight_bytes / (16.0 * bt)
        hbm_r = (2 * 96 + 4) if features else (sh.hbm_bytes - 4)
        ring_b = 2 * sh.R * (sh.L if ring_layers_in_hbm is None else ring_layers_in_hbm)      # read, and as much written
        parts = {"mfma": mfma * nj("mfma16") * 1e-3, "transcendental": trans * nj("trans") * 1e-3, "valu": valu * nj("valu") * 1e-3,
                 "lds": lds_b / 1024.0 * nj("lds") * 1e-3, "l2_weight_stream": w_b / 1024.0 * nj("l2") * 1e-3,
                 "hbm_compulsory": (hbm_r / 1024.0 * nj("hbm") + 4 / 1024.0 * nj("hbmw")) * 1e-3}
        ring = (ring_b / 1024.0 * nj("hbm") + ring_b / 1024.0 * nj("hbmw")) * 1e-3
        floor = sum(parts.values())
        return {"unit": "uJ per utterance-sample", "achieved_uj": achieved, "achieved_total_uj": achieved_total, "floor_uj": floor,
                "frac": floor / achieved, "floor_with_ring_uj": floor + ring, "frac_with_ring": (floor + ring) / achieved,
                "floor_parts_uj": {k: round(v, 4) for k, v in parts.items()}, "ring_uj": round(ring, 4),
                "idle_resident_waves_w": base_w, "socket_w": power["socket_w"], "limit_w": power.get("limit_w"),
                "prices_nj": {k: round(nj(k), 3) for k in ("mfma16", "mfma32", "valu", "trans", "lds", "l2", "hbm", "hbmw") if k in pr},
                "prices_source": "profiles/r06_energy_ubench.json (scripts/energy_ubench.py: marginal socket energy per operation, 256 workgroups of "
                                 "four waves; prices at 2.06-2.39 GHz, the launch itself runs at %.2f GHz)" % (power.get("shader_clock_ghz") or 0.0),
                "counts_per_utterance_sample": {"mfma_16x16x32": mfma, "transcendental_wave_instr": trans, "valu_wave_instr": valu,
                                                "lds_bytes": lds_b, "weight_stream_bytes": w_b, "hbm_compulsory_bytes": hbm_r + 4, "ring_bytes": 2 * ring_b}}
    except Exception as ex:
        return {"error": str(ex)[:200]}


def power_reading(e, N, NTOT, B, sptr, seconds=3.0):
    """Socket power while the timed launch runs back to back for `seconds` (outside the timed region): the SMU's gpu_metrics table
    through `rocm-smi --showmetrics`, polled by scripts/clock_probe.py's sampler (~5 polls per second), beside the kernel's own clock
    probe.  The full-chip launch sits at the socket's power limit (profiles/r05_power_clock.txt): its rate is set by the joules an
    utterance-sample costs, which is what `uj_per_utterance_sample` reports.  None when the box offers no such telemetry."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "scripts"))
    try:
        import clock_probe
        if "power_w" not in clock_probe.read_metrics():
            return None
        smp = clock_probe.Sampler("metrics")
        smp.start()
        t0 = time.perf_counter()
        launches = 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        while time.perf_counter() - t0 < seconds:
            for _ in range(8):
                assert e.run_partial_chunk(STEADY_FROM, N, NTOT, B, sptr)
            launches += 8
            torch.cuda.synchronize()
        b.record()
        b.synchronize()
        t1 = time.perf_counter()
        smp.stop = True
        smp.join()
        busy = clock_probe.summarise(smp.samples, t0, t1)
        if "power_w" not in busy:
            return None
        ms = a.elapsed_time(b) / launches
        out = {"socket_w": round(busy["power_w"], 1), "sclk_mhz": round(busy.get("sclk_mhz", 0.0), 1), "hotspot_c": busy.get("hotspot_c_max"),
               "polls": busy["polls"], "seconds": round(t1 - t0, 2), "launches": launches, "ms_per_launch": ms,
               "shader_clock_ghz": e.lastLaunchClockGHz(), "uj_per_utterance_sample": busy["power_w"] * ms * 1e-3 / (B * N) * 1e6,
               "source": "rocm-smi --showmetrics (gpu_metrics: current_socket_power, current_gfxclks) while the timed launch repeats, "
                         "outside the timed region"}
        if "power_w_from_energy_accumulator" in busy:
            out["socket_w_from_energy_accumulator"] = round(busy["power_w_from_energy_accumulator"], 1)
        try:
            r = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showmaxpower", "--json"], capture_output=True, text=True, timeout=20)
            out["limit_w"] = float(json.loads(r.stdout)["card0"]["Max Graphics Package Power (W)"])
        except Exception:
            pass
        return out
    except Exception as ex:                          # telemetry is a courtesy of the box: never fail the benchmark for it
        return {"error": str(ex)[:200]}


DUMP_MAX_BYTES = 64 << 20                     # --dump-outputs: at most this much in all


def dump_outputs(out_dir, y, max_bytes=DUMP_MAX_BYTES, seed=0):
    """--dump-outputs: the samples of the last timed step, y [batch][samples] (integers), as out_dir/samples.npy in float32 (exact
    for sample indices).  Above max_bytes, a fixed, seeded sample of utterances (rows) in ascending order, whose indices go to
    out_dir/samples_rows.npy (float64); the two files together stay within max_bytes.  Returns the paths written."""
    y = np.asarray(y)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    rows_keep = max(1, (max_bytes - 512) // (4 * y.shape[1] + 8))       # (float32 samples and a float64 index per row, two .npy headers)
    if y.shape[0] > rows_keep:
        rows = np.sort(np.random.default_rng(seed).choice(y.shape[0], size=rows_keep, replace=False))
        y = y[rows]
        paths.append(os.path.join(out_dir, "samples_rows.npy"))
        np.save(paths[-1], rows.astype(np.float64))
    paths.append(os.path.join(out_dir, "samples.npy"))
    np.save(paths[-1], y.astype(np.float32))
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=0, help="utterances per GPU (0 = 48 per CU; with --full, the real-time batch the sweep picks)")
    ap.add_argument("--samples", type=int, default=0, help="samples per step (0 = auto)")
    ap.add_argument("--config", default="headline", choices=["headline", "c5"],
                    help="c5: BASELINE configs[4], global batch 64 sharded over the ranks (8 x 8 on 8 GPUs)")
    ap.add_argument("--conditioning", default="packed", choices=["packed", "features"],
                    help="what the timed launches read: conditioning pre-packed in fragment order (the reference harness's setInputs outside "
                         "the timed region; the headline), or the upsampled features, the conditioning computed in the kernel (profiling aid)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: the real-time batch sweep (the timed batch is the one it picks), "
                         "reference_definition / end_to_end / dropin_fp32 / oversubscribed, socket power, roofline, cpu_baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the samples of the last timed step to DIR/samples.npy (float32; a seeded sample of utterances above 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip cpu_baseline")
    ap.add_argument("--no-power", action="store_true", help="(--full) skip the 3-second socket-power reading behind the timed steps")
    ap.add_argument("--no-extras", action="store_true", help="(--full) skip reference_definition / end_to_end / oversubscribed")
    ap.add_argument("--extras-budget", type=float, default=240.0,
                    help="(--full) seconds of wall clock the entries beside the headline may take together; what does not fit is "
                         "reported as skipped")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for smoke runs)")
    ap.add_argument("--selftest-dist", action="store_true", help="launcher / rendezvous / gather plumbing only (no GPU)")
    ap.add_argument("--cpu-worker", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-seed", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    t_main = time.perf_counter()

    def note(msg):                               # progress on stderr (stdout carries the one JSON line)
        print("[bench %6.1f s] %s" % (time.perf_counter() - t_main, msg), file=sys.stderr, flush=True)

    def extras_left():
        return args.extras_budget - (time.perf_counter() - t_main)
    if args.cpu_worker:
        dt, _ = cpu_run_once(make_weights(), args.cpu_worker, seed=5 + args.cpu_seed)
        print(json.dumps({"cpu_worker_seconds": dt}))
        return

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)                      # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    if args.selftest_dist:
        return selftest_dist(args, world, rank, local_rank)

    import torch
    import torch.distributed as dist
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    if args.backend == "nccl" and torch.cuda.device_count() < world:
        sys.exit("bench.py: %d ranks but only %d GPU(s) are visible" % (world, torch.cuda.device_count()))
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend)
        prove_world(dist, world, rank, local_rank, args.backend)

    from nv_wavenet_amd.sharding import gather_samples, shard_range
    w = make_weights()
    ncu = torch.cuda.get_device_properties(local_rank).multi_processor_count
    extras = world == 1 and args.full and not args.no_extras and args.config == "headline"

    # ---- workload: the largest per-GPU batch that stays real time (bounded bisection, rank 0; --full only) ----
    sweep = {}
    max_rt = [None, None]                 # the largest real-time batch of the sweep and its kHz per utterance (rank 0)
    c3_b16_khz = None
    if args.config == "c5":
        B = shard_range(64, world, rank)[1]          # 8 per GPU on 8 GPUs
        assert B > 0, "more ranks than utterances"
    elif args.batch:
        B = args.batch
    elif not args.full:
        B = 48 * ncu                      # three tiles per CU on every CU: the real-time batch the sweep below settles on
    else:
        choice = torch.zeros(1, dtype=torch.int64, device="cuda")
        if rank == 0:
            c3_b16_khz, _ = measure_khz(w, 16, 1024)
            sweep[16] = c3_b16_khz
            # every probe is a steady-state one: samples 640 .. 1151 of an utterance (measure_steady_khz)
            lo, hi = 1, None                      # in tiles of 16 utterances: lo is real time, hi is not
            for tiles in (ncu, 2 * ncu, 3 * ncu, 4 * ncu):
                khz, _ = measure_steady_khz(w, 16 * tiles)
                sweep[16 * tiles] = khz
                if khz >= REALTIME_KHZ:
                    lo = tiles
                else:
                    hi = tiles
                    break
            while hi is not None and hi - lo > 16:  # bisect to 16 tiles (256 utterances)
                mid = (lo + hi) // 2 // 4 * 4
                if mid <= lo:
                    break
                khz, _ = measure_steady_khz(w, 16 * mid)
                sweep[16 * mid] = khz
                if khz >= REALTIME_KHZ:
                    lo = mid
                else:
                    hi = mid
            # the chosen batch three more times: it must hold 24 kHz in every probe, else one notch (16 tiles) down -- a box 3 % slower
            # than the next must not flip the headline between runs
            while lo > 16:
                reps = [measure_steady_khz(w, 16 * lo)[0] for _ in range(3)]
                sweep["%d (3 more probes)" % (16 * lo)] = reps
                if min(reps) >= REALTIME_KHZ:
                    break
                lo -= 16
            # Round 6: beyond three tiles per CU the engine launches FOUR tiles per workgroup on fewer CUs (216 x 4 tiles at 13 824), which the
            # socket's power limit clocks higher than 256 busy CUs: the largest real-time batch grew, but its aggregate rate (B x kHz) is
            # below that of three tiles on every CU.  The timed workload is the real-time batch with the highest aggregate rate; the largest
            # real-time batch is reported beside it (`max_realtime_batch_per_gpu`, with the kHz of its three extra probes).
            max_rt[0], max_rt[1] = 16 * lo, (min(sweep["%d (3 more probes)" % (16 * lo)]) if "%d (3 more probes)" % (16 * lo) in sweep else sweep.get(16 * lo))
            best_b, best_rate = 16 * lo, 16 * lo * (max_rt[1] or 0.0)
            for tiles in (3 * ncu, 2 * ncu):
                k = sweep.get(16 * tiles)
                if k is not None and k >= REALTIME_KHZ and tiles < lo and 16 * tiles * k > best_rate:
                    best_b, best_rate = 16 * tiles, 16 * tiles * k
            choice[0] = best_b
        if world > 1:
            if args.backend != "nccl":
                choice = choice.cpu()
            dist.broadcast(choice, 0)
        B = int(choice.item())
    N = args.samples or (2048 if args.config == "c5" else samples_per_step_for(B))      # samples per step

    # ---- beside the headline (rank 0, one GPU): the reference's own measurement on C2 / C3 / C4, the
    #      throughput organisation, and the real-time batch with conditioning streamed per chunk ----
    refdef, thr, e2e, dropin = None, None, None, None
    skipped = []
    note("workload: %d utterances per GPU, %d samples per step" % (B, N))
    if extras and rank == 0:
        refdef = {}
        for sh in (C2, C3, C4):
            if extras_left() < 30:
                skipped.append("reference_definition.%s" % sh.name)
                continue
            note("reference_definition %s" % sh.name)
            refdef[sh.name] = {"single_workgroup": reference_definition_khz(sh, 1),
                               "multi_cu_chain": reference_definition_khz(sh, 3),
                               "auto": reference_definition_khz(sh, 0)}
            # ... and the largest batch the multi-CU organisation serves at once: one chain of `stages` CUs per 16 utterances, all
            # of them resident together (what bounds it: CUs / stages chains)
            import re
            m = re.search(r"stages=(\d+)", refdef[sh.name]["multi_cu_chain"]["kernel"])
            if m:
                chains = ncu // int(m.group(1))
                big = Shape(sh.name, sh.R, sh.S, sh.A, sh.L, sh.maxD, 16 * chains)
                r = reference_definition_khz(big, 3, N=4096, chunk=2048)
                refdef[sh.name]["multi_cu_chain_full_gpu"] = r
                best_mc = big.B if r["khz_per_utterance"] >= REALTIME_KHZ and "wavenet_chain" in r["kernel"] else None
                if sh is C4:
                    # round 5: batches beyond the resident chains ride the same chains, several tiles per chain (the stages work
                    # through them in turn; nv_wavenet_persistent.cuh:110 loops its blocks over the whole batch): the largest that
                    # stays real time, found at steady state (samples 640.., conditioning packed block by block) and then measured by
                    # the reference's definition
                    sweep_mc = {}
                    best_steady = None
                    for tpc in (6, 5, 4, 3, 2):
                        if extras_left() < 40:
                            skipped.append("reference_definition.%s.tiles_per_chain_%d" % (sh.name, tpc))
                            continue
                        note("reference_definition %s, %d tiles per chain" % (sh.name, tpc))
                        shb = Shape(sh.name, sh.R, sh.S, sh.A, sh.L, sh.maxD, 16 * chains * tpc)
                        k, info_k = measure_steady_khz(make_weights(shb, seed=1), shb.B, 1024, sh=shb, impl=3)
                        sweep_mc[str(shb.B)] = k
                        if k >= REALTIME_KHZ and "wavenet_chain" in info_k:
                            n_rd = 4096
                            while n_rd > 512 and n_rd * shb.L * shb.B * 2 * shb.R * 4 > 70e9:      # (the harness hands over the whole fp32 tensor)
                                n_rd //= 2
                            r = reference_definition_khz(shb, 3, N=n_rd, chunk=n_rd // 2)
                            r["steady_state_khz_per_utterance"] = k
                            r["mfma_frac_of_dense_fp16_peak"] = shb.flops * shb.B * k * 1e3 / (MFMA_F16_PEAK_TFLOPS * 1e12)
                            # the organisation's own roofline (steady state): algorithmic flops of the shape x utterance-samples per second
                            # against the dense fp16 MFMA peak; what bounds it is the per-stage latency of the dependent chain, not a roof
                            r["roofline"] = dict(bound="mfma", achieved=shb.flops * shb.B * k * 1e3 / 1e12, peak=MFMA_F16_PEAK_TFLOPS, unit="TFLOP/s",
                                                 frac=shb.flops * shb.B * k * 1e3 / (MFMA_F16_PEAK_TFLOPS * 1e12),
                                                 hbm=dict(achieved=shb.B * k * 1e3 * (shb.hbm_bytes + 2 * 2 * shb.R * shb.L) / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                                                          bytes_per_utterance_sample=shb.hbm_bytes + 2 * 2 * shb.R * shb.L,
                                                          note="conditioning + ring, algorithmic; the hand-off granules add 46 KB written per "
                                                               "utterance-sample (profiles/r05_chain_c4_tiles_per_chain.txt)"),
                                                 flops_per_utterance_sample=shb.flops, kernel=r["kernel"].split(" ")[0])
                            r["tiles_per_chain"] = tpc
                            if best_steady is None:
                                best_steady = shb.B
                                refdef[sh.name]["multi_cu_chain_tiles_per_chain_steady_state"] = r
                            # real time by the reference's definition as well (its 2 048 - 4 096 samples include the start of the utterance,
                            # 3 - 4 % below the steady state): else one tile per chain fewer
                            if r["khz_per_utterance"] >= REALTIME_KHZ:
                                refdef[sh.name]["multi_cu_chain_tiles_per_chain"] = r
                                best_mc = shb.B
                                break
                    refdef[sh.name]["tiles_per_chain_sweep_steady_khz"] = sweep_mc
                    refdef[sh.name]["max_realtime_batch_multi_cu_steady_state"] = best_steady
                refdef[sh.name]["max_realtime_batch_multi_cu"] = best_mc
        dropin = None
        if extras_left() > 30:
            note("dropin_fp32")
            try:
                dropin = dropin_fp32(C3)
                dropin["integration_test_model"] = dropin_fp32(C3, L=16, maxD=128)["persistent"]      # pytorch/config.json: 16 layers, maxDilation 128
            except Exception as ex:              # (an entry beside the headline must not take the run down)
                dropin = {"error": str(ex)[:200]}
        else:
            skipped.append("dropin_fp32")
        bt = 64 * ncu                                 # four tiles per CU: not real time
        # beyond three tiles per CU a launch has more three-tile wavenet_wg workgroups than CUs (whole rounds): throughput, not real
        # time; reported at four and at six tiles per CU (= two full rounds)
        thr = {"definition": "batches beyond the real-time capacity: more utterances per GPU at a lower rate per utterance "
                             "(steady state, samples 640..1151; the engine's own choice of organisation)", "points": []}
        note("oversubscribed")
        for bt_ in (bt, 96 * ncu):
            if extras_left() < 20:
                skipped.append("oversubscribed.%d" % bt_)
                continue
            khz_t, info_t = measure_steady_khz(w, bt_, 256)
            thr["points"].append({"batch_per_gpu": bt_, "khz_per_utterance": khz_t, "samples_per_sec_per_gpu": bt_ * khz_t * 1e3,
                                  "kernel": info_t.split(" ")[0], "real_time": bool(khz_t >= REALTIME_KHZ)})
        if thr["points"]:
            best_t = max(thr["points"], key=lambda q: q["samples_per_sec_per_gpu"])
            thr.update({k: best_t[k] for k in ("batch_per_gpu", "khz_per_utterance", "samples_per_sec_per_gpu", "kernel", "real_time")})
        e2e = {"definition": "conditioning fp32 [N][L][B][2R] in HBM, packed per chunk of 256 samples on a second stream "
                             "behind the generation of the previous chunk; Philox selectors; samples left in HBM",
               "sweep_khz": {}}
        best = None
        for cand in sorted(set([B // 4, B * 3 // 8, B // 2, B * 3 // 4, B] + [c for c in (16 * ncu, 24 * ncu, 32 * ncu) if c <= B]),
                           reverse=True):
            cand = max(16, cand // 64 * 64)
            if extras_left() < 20:
                skipped.append("end_to_end.%d" % cand)
                break
            note("end_to_end %d" % cand)
            k = end_to_end_khz(w, cand)
            e2e["sweep_khz"][str(cand)] = k
            if k >= REALTIME_KHZ:
                best = cand
                break
        e2e["max_realtime_batch_per_gpu"] = best
        # ... and with the producer of that conditioning in the loop (the model's own upsampling + conditioning convolution, run on
        # the GPU between the generation launches, landing in fragment order): what a deployment gets end to end
        fin = {"definition": "FEATURES IN, SAMPLES OUT (round 5): one nvw_generate_stream call over mel-like frames [B][80][frames] fp16 resident in "
                             "HBM; per chunk of 256 samples the engine upsamples them with its own MFMA kernel (ConvTranspose1d, window 1024 / "
                             "stride 256) into 160 B of features per utterance and sample, and the generation launch computes the conditioning "
                             "Lh = Wcond c + bcond itself (wn::wavenet_wg<.., RAW=3>); samples copied out per chunk on a second stream; wall "
                             "clock around the call, 8 chunks from sample 0", "sweep_khz": {}}
        best_fin = None
        Bf = min(B, 48 * ncu)                   # (the kernels that compute the conditioning take at most three tiles per workgroup)
        for cand in sorted(set([Bf + 16 * ncu // 4, Bf, Bf - 16 * ncu // 4, Bf - 16 * ncu // 2, Bf * 3 // 4, Bf // 2]), reverse=True):
            cand = max(16, cand // 64 * 64)
            if cand > 48 * ncu or str(cand) in fin["sweep_khz"]:
                continue
            if extras_left() < 20:
                skipped.append("end_to_end.with_producer.%d" % cand)
                break
            note("with_producer (features in) %d" % cand)
            ks = []
            for _ in range(3 if best_fin is None else 1):                      # three probes: a 3 % box must not flip the entry
                k, info_fin = features_in_khz(w, cand)
                ks.append(k)
            fin["sweep_khz"][str(cand)] = ks
            if min(ks) >= REALTIME_KHZ:
                best_fin = cand
                fin["kernel"] = info_fin.split(" ")[0]
                fin["khz_per_utterance"] = min(ks)
                fin["realtime_margin"] = min(ks) / REALTIME_KHZ - 1.0
                break
        fin["max_realtime_batch_per_gpu"] = best_fin
        e2e["with_producer"] = fin
        wp = {"definition": "(round 4's producer, kept for comparison) per chunk of 256 samples: get_cond_input(layout='packed') (upsampling of [B][80][frames] fp16 features as matrix "
                            "products, then the 1x1 conditioning convolution -- the engine's channel order and gate pre-scale folded into its "
                            "weights -- by the engine's own MFMA producer kernel, nvw_produce_conditioning_f16) writes the engine's fragment "
                            "order in place, then the generation launch "
                            "of that chunk; same stream (every CU holds a generation workgroup for a whole launch); 4 chunks, the first "
                            "production inside the timed region", "sweep_khz": {}}
        best_wp = None
        for cand in sorted(set([28 * ncu, B // 2]), reverse=True):
            cand = max(16, cand // 64 * 64)
            if extras_left() < 60:
                skipped.append("end_to_end.with_lh_producer.%d" % cand)
                break
            note("with_lh_producer %d" % cand)
            try:
                k = with_producer_khz(w, cand)
            except Exception as ex:             # (e.g. out of memory in the producer's workspaces at the largest batch: an entry beside the headline must not take the run down)
                wp["sweep_khz"][str(cand)] = "failed: %s" % str(ex)[:80]
                torch.cuda.empty_cache()
                continue
            wp["sweep_khz"][str(cand)] = k
            if k >= REALTIME_KHZ:
                best_wp = cand
                break
        wp["max_realtime_batch_per_gpu"] = best_wp
        e2e["with_lh_producer"] = wp
        # ... and with no pack at all: the kernels read the caller's tensor in place (setConditioningDirect), fp16 (the
        # engine's T_data) or fp32; steady state like the headline, at the headline batch, then at two / one tile per CU
        # until it is real time
        e2e["in_place"] = {}
        for name, dt in (("fragment_order", "fragments"), ("fp16_tensor", torch.float16), ("fp32_tensor", torch.float32)):
            ip_sweep = {}
            k_ip, info_ip = 0.0, ""
            for cand in [B] + [c for c in (44 * ncu, 40 * ncu, 36 * ncu, 32 * ncu, 16 * ncu) if c < B]:
                if extras_left() < 20:
                    skipped.append("end_to_end.in_place.%s.%d" % (name, cand))
                    break
                note("in_place %s %d" % (name, cand))
                k_ip, info_ip = measure_steady_khz(w, cand, in_place=dt)
                ip_sweep[str(cand)] = k_ip
                if k_ip >= REALTIME_KHZ:
                    break
            e2e["in_place"][name] = {"definition": ("conditioning PRODUCED by the caller in the engine's fragment order (fp16; a model folds the "
                                                    "channel permutation and the gate pre-scale into its conditioning convolution), used in place by "
                                                    "the packed path of the generation kernel (nvw_set_conditioning_packed): no copy, no second "
                                                    "pass, no conversion; samples 640..1151") if dt == "fragments" else
                                                   "conditioning %s [N][L][B][2R] in HBM read in place by the generation kernel "
                                                   "(nvw_set_conditioning_direct_t): no packed copy, no second pass; samples 640..1151" % name,
                                     "batch_per_gpu": cand, "khz_per_utterance": k_ip, "kernel": info_ip.split(" ")[0],
                                     "real_time": bool(k_ip >= REALTIME_KHZ), "sweep_khz": ip_sweep}

    # ---- the timed workload: every step generates samples STEADY_FROM .. STEADY_FROM+N-1 (all dilated taps live, all rings
    #      wrapped, conditioning rows of exactly those samples) for every utterance (re-run per step on the rings the previous step left:
    #      timing only, see config.workload)
    note("timed steps")
    e, NTOT, _keep = steady_engine(w, B, N, 100 + rank, "features" if args.conditioning == "features" else None)
    e.setClockProbe(True)                       # workgroup 0 of every launch records shader / wall clock counters
    kinfo = e.kernelInfo(B, False)
    torch.cuda.empty_cache()
    ybuf = [torch.zeros(B, NTOT, dtype=torch.int32, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream()
    sptr = stream.cuda_stream
    gathered = [None]                           # (world > 1) the last finished gather: [total_batch][N]
    total_batch = 64 if args.config == "c5" else B * world

    pending = []

    def step(i, events=None):
        y = ybuf[i % 2]
        # the gather of step i overlaps the kernel of step i+1 (RCCL runs on its own stream); the gather
        # of step i-2 read the buffer this step overwrites, so it is completed first
        while len(pending) > 1:
            gathered[0] = pending.pop(0)()
        if events is not None:
            events[0].record(stream)
        assert e.run_partial_chunk(STEADY_FROM, N, NTOT, B, sptr)
        if events is not None:
            events[1].record(stream)
        e.getYOut(y, STEADY_FROM, N, sptr)               # the step's samples, device to device
        if world > 1:
            _, fin = gather_samples(y[:, STEADY_FROM:].contiguous(), total_batch, async_op=True)
            pending.append(fin)

    for i in range(args.warmup):
        step(i)
    while pending:
        gathered[0] = pending.pop(0)()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i, evs[i])
    while pending:
        gathered[0] = pending.pop(0)()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        assert gathered[0].shape[0] == total_batch, "the gather returned %d rows, expected %d" % (gathered[0].shape[0], total_batch)
    kern_ms = sum(a.elapsed_time(b) for a, b in evs) / args.steps
    ylast = ybuf[(args.steps - 1) % 2][:, STEADY_FROM:]
    hist = int(torch.unique(ylast).numel())
    status = e.chainStatus()
    clock_ghz = e.lastLaunchClockGHz()          # the clock the last timed launch ran at (the chip clocks to its power budget)
    if args.dump_outputs and rank == 0:
        note("dump outputs to %s" % args.dump_outputs)
        dump_outputs(args.dump_outputs, (gathered[0] if world > 1 else ylast).cpu().numpy())
    power = None
    if args.full and rank == 0 and world == 1 and not args.no_power:
        note("socket power of the timed launch")
        power = power_reading(e, N, NTOT, B, sptr)
    e.close()

    if rank == 0:
        assert status == 0, "multi-CU hand-off timed out: 0x%x" % status
        ms_per_step = 1e3 * dt / args.steps
        value = total_batch * N / (dt / args.steps)
        khz = N / kern_ms
        units = B * N                                   # utterance-samples per launch
        flops = units * HEAD.flops
        tiles = (B + 15) // 16
        kname = kinfo.split(" ")[0]                             # what the engine reports it launches
        chain_mode = "wavenet_chain" in kname
        bt = 4 if "BT=4" in kname else 3 if "BT=3" in kname else 2 if "BT=2" in kname else 1
        if not args.batch and args.config == "headline" and tiles > ncu:
            assert kname == HEADLINE_KERNELS[bt].replace("RAW=0", "RAW=3" if args.conditioning == "features" else "RAW=0"), kinfo     # the launches the parity tests pin
        # ---- --full: the roofline of the timed launch (counter files of profiled rounds, the code objects' instruction streams,
        #      socket power) ----
        roofline = None
        if args.full:
            # workgroups (weight-stream passes) per sample
            passes = (tiles + bt - 1) // bt
            traffic, lds_counter, traffic_file, counters = None, None, None, None
            # HBM and LDS bytes per launch from the PMC passes of the latest profiled round (profiles/traffic_rNN.json, written
            # by scripts/make_profiles_r*.py from rocprofv3 counters); only valid for the launch shape it was measured on
            # ... AND for the device code it was measured on: the file carries the kernel's name and the sha256 of its instruction stream
            # (scripts/isa_stats.py sha); a kernel that has changed since drops the counters (the algorithmic bytes are reported, and why)
            import glob
            traffic_note = "no counter file for this launch shape (batch %d, %d samples): algorithmic bytes only" % (B, N)
            sha_now = None
            try:
                sys.path.insert(0, os.path.join(ROOT, "scripts"))
                import isa_stats
                sub = isa_stats.kernel_sub_of(kname)
                sha_now = isa_stats.kernel_sha("inst_%d_%d_%d_p16.o" % (HEAD.R, HEAD.S, HEAD.A), sub) if sub else None
            except Exception:
                sha_now = None
            for tf in sorted(glob.glob(os.path.join(ROOT, "profiles", "traffic_r*.json")), reverse=True):
                try:
                    tj = json.load(open(tf))
                    if tj.get("batch") == B and tj.get("samples") == N:
                        if tj.get("kernel") != kname or not sha_now or tj.get("kernel_sha256") != sha_now:
                            traffic_note = ("%s was measured on %s, code %s; this run launches %s, code %s: counters dropped" %
                                            (os.path.relpath(tf, ROOT), tj.get("kernel"), str(tj.get("kernel_sha256"))[:12], kname, str(sha_now)[:12]))
                            break
                        traffic = tj.get("hbm_bytes_per_launch")
                        lds_counter = tj.get("lds_bytes_per_launch")
                        counters = tj
                        traffic_file = os.path.relpath(tf, ROOT)
                        traffic_note = "rocprofv3 counters of this launch shape and this device code (%s)" % traffic_file
                        break
                except Exception:
                    pass
            # compulsory HBM bytes per utterance and sample: the conditioning (2R x L fp16 values) or, computed in the kernel, the features
            # it is computed from (feature fragments: 96 fp16 values), + selector + sample
            hbm_alg = (2 * 96 + 8) if args.conditioning == "features" else HEAD.hbm_bytes
            roofline = dict(bound="mfma", achieved=flops / (kern_ms * 1e-3) / 1e12, peak=MFMA_F16_PEAK_TFLOPS,
                            unit="TFLOP/s", traffic=traffic, traffic_source=traffic_note, kernel=kname, kernel_sha256=sha_now, launch=kinfo,
                            kernel_ms=kern_ms,
                            hbm=dict(achieved=units * hbm_alg / (kern_ms * 1e-3) / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                                     bytes_per_utterance_sample=hbm_alg))
            roofline["frac"] = roofline["achieved"] / roofline["peak"]
            # measured inside the kernel (s_memtime ticks over s_memrealtime ticks of workgroup 0): under full load the chip
            # runs this launch below its 2.4 GHz maximum -- power-limited, profiles/r04_clock_*.json -- and `frac` is against the
            # peak at 2.4 GHz; frac_at_measured_clock prices the same work against the matrix peak at the clock actually granted
            if clock_ghz > 0:
                roofline["shader_clock_ghz"] = clock_ghz
                roofline["shader_cycles_per_sample"] = kern_ms * 1e-3 / N * clock_ghz * 1e9
                roofline["frac_at_measured_clock"] = roofline["frac"] * 2.4 / clock_ghz
            # (round 6: the layers whose dilation is at most the `ring_in_lds=d<=N` of the launch keep their slots in LDS for the whole launch)
            import re as _re
            m_ring = _re.search(r"ring_in_lds=d<=(\d+)", kinfo)
            ring_d = int(m_ring.group(1)) if m_ring else 0
            d_, ring_layers = 1, 0
            for _l in range(HEAD.L):
                ring_layers += 1 if d_ > ring_d else 0
                d_ = 1 if d_ * 2 > HEAD.maxD else d_ * 2
            if power:
                roofline["power"] = power
                en = energy_roofline(power, kern_ms, B, N, bt, args.conditioning == "features", ring_layers_in_hbm=ring_layers)
                if en:
                    roofline["energy"] = en
                    # ... and the same price list on what the launch ACTUALLY issued and moved (rocprofv3 counters of this kernel and launch shape,
                    # profiles/traffic_rNN.json): does the sum of the priced operations explain the energy the socket reports?
                    if counters and "prices_nj" in en and not chain_mode:
                        try:
                            pn = en["prices_nj"]
                            mf = HEAD.macs / 8192.0
                            act = {"mfma": mf * pn["mfma16"], "valu_and_transcendental": counters["valu_per_mfma"] * mf * pn["valu"],
                                   "lds": counters["lds_bytes_per_workgroup_sample"] / (16.0 * bt) / 1024.0 * pn["lds"],
                                   "l2_weight_stream": HEAD.weight_bytes / (16.0 * bt) / 1024.0 * pn["l2"],
                                   "hbm_read": counters["hbm_read_bytes_per_utterance_sample"] / 1024.0 * pn["hbm"],
                                   "hbm_write": counters["hbm_write_bytes_per_utterance_sample"] / 1024.0 * pn["hbmw"]}
                            en["priced_counters_uj"] = sum(act.values()) * 1e-3
                            en["priced_counters_parts_uj"] = {k: round(v * 1e-3, 4) for k, v in act.items()}
                            en["priced_counters_over_achieved"] = en["priced_counters_uj"] / en["achieved_uj"]
                            en["priced_counters_note"] = ("the price list applied to the instructions issued and bytes moved per utterance-sample (SQ_INSTS_VALU / SQ_INSTS_MFMA, "
                                                          "SQ_INSTS_LDS_*_BANDWIDTH, FETCH_SIZE x2, WRITE_SIZE of %s): how much of the measured dynamic energy the priced operations explain" % traffic_file)
                        except Exception:
                            pass
                # what binds: with every CU busy the socket sits at its power limit and gives the clock away -- the launch is
                # bound by joules per utterance-sample, not by the matrix pipe nor by HBM
                if power.get("limit_w") and power.get("socket_w", 0) >= 0.95 * power["limit_w"]:
                    roofline["bound"] = "power"
                    roofline["bound_evidence"] = ("socket %.0f W of %.0f W with the clock at %.2f GHz (2.4 GHz unconstrained); the MFMA figures below are "
                                                  "kept as the FLOP accounting the harness asks for" % (power["socket_w"], power["limit_w"], power.get("shader_clock_ghz") or 0.0))
            roofline["hbm"]["frac"] = roofline["hbm"]["achieved"] / HBM_PEAK_GBS
            # ... and with the dilation ring, which this design keeps in HBM (read x[t-d], write x[t]: 2 x 2R bytes per layer, utterance and
            # sample): the bytes the kernel actually asks of the memory system (what `traffic` measures), and the roof it is nearest to
            ring_bytes = 2 * 2 * HEAD.R * ring_layers
            roofline["ring_layers_in_hbm"] = ring_layers
            roofline["hbm_with_ring"] = dict(achieved=units * (hbm_alg + ring_bytes) / (kern_ms * 1e-3) / 1e9, peak=HBM_PEAK_GBS, unit="GB/s",
                                             bytes_per_utterance_sample=hbm_alg + ring_bytes)
            roofline["hbm_with_ring"]["frac"] = roofline["hbm_with_ring"]["achieved"] / HBM_PEAK_GBS
            if not chain_mode:                                      # (the chain reads no weights after its prologue)
                roofline["l2_weight_stream"] = dict(achieved=passes * N * HEAD.weight_bytes / (kern_ms * 1e-3) / 1e9,
                                                    peak=L2_PEAK_GBS, unit="GB/s")
                roofline["l2_weight_stream"]["frac"] = roofline["l2_weight_stream"]["achieved"] / L2_PEAK_GBS
                lds_alg = passes * N * lds_bytes_per_sample(bt)
                # rocprof-reported when this launch shape was profiled: (SQ_INSTS_LDS_LOAD_BANDWIDTH + SQ_INSTS_LDS_STORE_BANDWIDTH) x 64 B
                roofline["lds"] = dict(achieved=(lds_counter or lds_alg) / (kern_ms * 1e-3) / 1e9, peak=LDS_PEAK_GBS, unit="GB/s",
                                       bytes_per_launch=lds_counter or lds_alg, algorithmic_bytes_per_launch=lds_alg,
                                       source=("rocprofv3 counters of this launch shape (%s)" % traffic_file)
                                       if lds_counter else "algorithmic bytes (exchange images, bias quads, logits): this launch shape was not profiled")
                roofline["lds"]["frac"] = roofline["lds"]["achieved"] / LDS_PEAK_GBS
        out = {
            "metric": "samples/sec (all GPUs) in real time (every utterance >= 24 kHz) and max real-time batch @24kHz, R64/S256/A256 20L fp16",
            "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong" if args.config == "c5" else "weak",
            "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": "C3: R=64 S=256 A=256 L=20 maxDilation=512 fp16, autoregressive generation at steady state "
                                   "(each step = samples %d..%d of every utterance: all dilated taps live, all rings wrapped; the steps re-run that sample "
                                   "range -- same launch, same memory traffic -- so from the second step on the rings hold the previous step's "
                                   "values: a timing workload, not one long utterance)" % (STEADY_FROM, STEADY_FROM + N - 1)
                       if args.config == "headline" else
                       "C5: C3 shape, global batch 64 sharded over the ranks, RCCL gather of the samples",
                       "batch_per_gpu": B, "global_batch": total_batch, "samples_per_step": N,
                       "parallelism": "batch-sharded x%d, final RCCL all_gather" % world},
            "samples_per_sec_per_gpu": value / world,
            "khz_per_utterance": khz,
            "realtime_margin": khz / REALTIME_KHZ - 1.0,
            "distinct_samples_in_last_step": hist,
        }
        if args.full:
            out.update({
                "max_realtime_batch_per_gpu": (max_rt[0] if max_rt[0] and max_rt[0] > B else B) if khz >= REALTIME_KHZ else None,
                "max_realtime_batch_khz_per_utterance": max_rt[1] if max_rt[0] and max_rt[0] > B else khz,
                "timed_batch_note": (None if not max_rt[0] or max_rt[0] == B else
                                     "the timed steps run the real-time batch with the highest aggregate rate (%d utterances, three tiles per workgroup on every CU); "
                                     "the largest real-time batch is %d (four tiles per workgroup on %d CUs, %.2f kHz per utterance in its slowest probe = %.1f M samples/s)"
                                     % (B, max_rt[0], (max_rt[0] // 16 + 3) // 4, max_rt[1], max_rt[0] * max_rt[1] / 1e3)),
                "max_realtime_batch_definition": "(found by bisection in steps of 256 utterances, the chosen batch probed three more times) "
                                                 "largest batch whose samples 640..1151 (steady state: nv_wavenet_perf.cu:195-199 times "
                                                 "N=16384 at maxDilation 512) are generated at >= 24 kHz per utterance; conditioning pre-packed in HBM "
                                                 "(setInputs outside the timed region, like the reference's harness); see end_to_end for "
                                                 "conditioning streamed per chunk or read in place",
                "realtime_sweep_khz": {str(k): v for k, v in sorted(sweep.items(), key=lambda kv: str(kv[0]))},
                "c3_b16": {"khz_per_utterance": c3_b16_khz, "samples_per_sec": None if c3_b16_khz is None else 16e3 * c3_b16_khz},
                "reference_definition": refdef,
                "end_to_end": e2e,
                "dropin_fp32": dropin,
                "oversubscribed": thr,
                "extras_skipped_for_time": skipped,
                "roofline": roofline,
            })
        if args.full and world == 1 and not args.no_cpu_baseline:
            note("cpu_baseline")
            out["cpu_baseline"] = cpu_baseline(w)
        note("done")
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
