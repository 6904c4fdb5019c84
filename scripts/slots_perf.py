"""Slot mode (continuous batching) against lockstep generation at the same batch: steady-state time per step.

C3 shape (bench.py: R 64, S 256, A 256, 20 layers, maxDilation 512), fp16, 80 feature channels, in one process:
  lockstep   per chunk: nvw_pack_features of the chunk's features + nvw_run_range (the features path of a batch that started
             together)
  slots      per chunk: nvw_slots_step with every column busy and the utterances staggered -- lengths of 8 192 to 16 384 samples
             and random progress at the start, so that columns end and are restarted (ring reset) in every step -- samples copied
             to device memory
Both read their features from one shared fp16 tensor (every utterance a different window of it).  Prints one JSON line per chunk
size with ms per step of each and their ratio (slots / lockstep rate).

--mel adds, on an engine with the upsampling of bench.py's synthetic model (window 1024, stride 256):
  mel        per chunk: nvw_slots_step with every column a MEL column -- each with frames of its own (distinct fp16 [80][64] per
             column, 126 MiB in all; its features upsampled in the step), the same lengths and restarts -- and
             the columns' phases staggered: the 16 columns of a tile join 17 samples apart, so that no two of a tile share a
             phase (the feed's stores are then as scattered as they get)
and reports its rate against the feature-fed slot step (mel_rate_vs_slots).

--compact times, instead, what moving columns buys a fragmented batch, in one process, back to back:
  every column starts, then all but one column of every tile (column 5 of each: 1/16 of the batch, scattered over all tiles)
  stop -- the survivors of a burst.  Per round: steps of 2048 and 256 samples as they lie (the launch covers every tile), the
  survivors moved into the front columns (nvw_slot_move, one launch), the same steps compacted, and the survivors moved back.
  The move launch, and the loads of resumed columns, are isolated as the difference between a step of ONE sample that carries them
  and plain steps of one sample around it; saves are timed directly (events around nvw_slot_save calls).  Prints one JSON line
  with the medians, the run-to-run spread over the rounds (min .. max), the tiles launched, and save / load GB/s against the
  bytes of the blobs (read + written) and against the 128-byte lines the ring side touches (one per 16-byte piece).

--serve times the door a caller uses, at full load and at 1/16 load, per chunk size, cases back to back in one
process, `--rounds` rounds each (min / median / max of the per-step means):
  engine      (i)   nvw_slots_step into device buffers, columns restarted as they end: device time per step (events)
  step        (ii)  SlotStream.step(): wall time per step, requests resubmitted as they finish -- the baseline
  step_async  (iii) SlotStream.step_async() two deep, the same service: wall time per step
  delivery    (iv)  the output paths alone over a step's samples (nvw_slots_time_outputs: events around the launches): the PCM
                    launch + 2-D copies of plain rows to device and to pinned memory, the delivery launch to device and to pinned
                    memory (direct stores), and the delivery to device + one contiguous copy to pinned memory (staging)
Prints one JSON line per (load, chunk).

--drain times saving and resuming many columns at once on the setup of --compact -- every column starts, all but
column 5 of every tile stop, the survivors are compacted to the front --, in one process, `--rounds` rounds back to back.  Per round:
  save    the survivors with ONE nvw_slots_save_list into device memory; the same into pinned host memory; and with one
          nvw_slot_save per column (the comparand: what a drain cost before) -- events around the calls, and the host's wall time
  resume  from each of the three: the columns stopped, then a one-sample step that carries the loads minus the plain one-sample
          steps around it (the device side: the load launch reading device or pinned blobs), and the wall time of the host calls
          that queue the resumes (one nvw_slots_resume_list against one nvw_slot_resume, i.e. one blocking header copy, per column)
Prints one JSON line with medians, min .. max over the rounds, GB/s of blob bytes (read + written), and the verdict on the claim
that the list save into device memory beats the single saves by more than the run-to-run spread.

--parent times the slot step of this commit against the PARENT commit's (a libwavenet_infer.so built from it, --parent-lib; loaded
beside this commit's and driven through the same ctypes calls) in one process, `--rounds` rounds, the cases alternating within a
round: the plain step (nvw_slots_step into a device buffer) and the ragged step into pinned memory (nvw_slots_step_ragged, waited
for at the end of each round's steps), each on both libraries.  Every column runs one long utterance (no restarts: the same work
in every case and round).  Prints one JSON line per chunk size with the per-round ms per step of each case, the medians, the
parent's run-to-run spread (max - min over median) and the verdict per kind of step: this commit's median not above the parent's
by more than twice that spread.  The order of the two libraries within a round alternates from round to round.  The wall time
the host spends inside the calls is recorded beside the time of a step (host_us_per_call, with the same verdict): at --batch 16
--chunks 16 a step is one 16-sample launch on one CU, the GPU side is constant and the host's bookkeeping is what can differ.
--temperature is the same comparison for what the per-column sampling temperature costs a step: the parent's plain
step, this commit's with every T = 1 (no table, the kernel argument NULL) and with mixed T (0.7, 0.85, 1, 1.2 cycling over the
columns: the table and its scatter launch); a parent that has the temperature entries is simply run at T = 1.
--min-p is that comparison for the probability floor: the parent's plain step, this commit's with every floor 0
(set explicitly: no table, Params::floorOn = 0 -- the launches the parent issues) and with mixed floors (0, 0.05, 0.1, 0.25, 0.5
cycling over the columns: the table, its scatter launch and a compare and a select per logit).  The verdict is about the all-zero
case -- not above the parent by more than twice the parent's own spread --; the mixed case is reported beside it, not barred.
--cut is that comparison for the tail cuts (top-k and top-p), seven cases: the parent's plain step and its step with
mixed floors; this commit's with every control off (set explicitly: no table, Params::floorOn = 0), with the same mixed floors only
(floorOn = 1: the launches the parent issues for them), with top-k only (0, 1, 4, 32, A cycling over the columns), with top-p only
(1, 0.5, 0.8, 0.9 cycling) and with both (floorOn bit 1: the search, 31 steps of one compare per logit with an add-with-carry, a select and an add).  The
verdict: the all-off case not above the parent's plain step, and the floors-only case not above the parent's floors-only step, each
by more than twice the spread of the parent's case it is held to; the three cutting cases are reported, not barred.
--prime is that comparison for primed generation: the parent's plain step, this commit's with no prime anywhere
(Params::forced = 0: the launches the parent issues) and with every column inside a prime for the whole measurement (one
slot_prime_kernel launch per step and the select behind softmax_pick in every sample).  The verdict is about the case without a
prime -- not above the parent by more than twice the parent's own spread --; the primed case is reported beside it, not barred.
--prefill times what a prime costs before its utterance draws its first sample, C3 fp16, one process: the
sequential path -- nvw_slot_start + nvw_slot_prime for every request, steps of at most the window up to local sample n, one
nvw_slots_save_list -- against nvw_prefill_states on the same primes and features, for 1 request and for 256, at n = W / 2, W, 4 W and
24 000 (W = nvw_prefill_window); `--rounds` rounds, the two paths alternating, events around each path and a check that the two
sets of blobs are equal bytes.  Prints one JSON line with the per-round milliseconds, the medians, the ratio, the 4 W against W
prefill time and the verdict on the one fixed bar: one request at n = W is faster prefilled than sequential.  With --parent-lib
it then prints the --parent comparison of the plain step (nothing on that path changes: a guard, not a goal).
--score times scoring, C3 fp16, one process: nvw_score_samples for 1 and 256 requests at n = 2 048 and 24 000, with
and without rows (a set of requests over nvw_score_max_samples goes in as many calls as it needs, like NVWaveNetEngine.score), and
beside it -- with --parent-lib -- the only way the parent commit can teacher-force: the same samples forced through primed columns
of the PARENT's library (nvw_slot_start + nvw_slot_prime for every request, steps of the window up to sample n).  Prints one JSON
line with the per-round milliseconds, the medians, the time per sample of both, the fraction of the fp16 MFMA peak the 256-request
cases reach (useful multiply-adds of the model over the dense peak of 2.5 PFLOP/s) and the verdict on the one fixed bar: scoring
256 utterances costs less than forcing them.  With --parent-lib it then prints nvw_prefill_states of both libraries (256 requests
at n = W) and the --parent comparison of the plain step: nothing on their paths changes, so both are guards, held to the spread
the parent itself shows.
--score-chunks times scoring with carried state, C3 fp16, one process: nvw_score_samples of this commit against the
parent's over 256 requests of 24 000 samples (a guard); nvw_score_chunks over the same samples in time chunks of 2 048 and 16 384
against the whole pass; one request of 1 500 000 samples, which the whole pass refuses, in chunks of 65 536; and 64 candidates of
256 samples behind one prefix of 24 000 against 64 whole scorings of 24 256.  Every result is checked bit for bit against the whole
pass before it is timed.  With --parent-lib it then prints the nvw_prefill_states and plain-step comparisons as --score does.

--prefill-mel and --score-mel time the same two passes fed from mel frames, C3 fp16, window 1024 / stride 256, one
process: nvw_prefill_states_mel (1 and 256 requests at n = W / 2, W, 4 W, 24 000) and nvw_score_samples_mel (n = 2 048, 24 000)
beside the feature entries of this commit on rows upsampled beforehand -- the difference is the upsampling's share -- and beside
nvw_upsample_requests alone; with --parent-lib the primes are also forced through mel columns of the PARENT's library
(nvw_slot_start_mel + nvw_slot_prime, steps of the window up to sample n), the only way the parent can prime from frames.  The
results of the paths are checked to be equal bytes.  One JSON line each: median and min .. max of the rounds per path.

    python scripts/slots_perf.py [--batch 12288] [--chunks 256,2048] [--steps 6] [--mel]
    python scripts/slots_perf.py --prefill-mel [--parent-lib PATH] [--rounds 5]
    python scripts/slots_perf.py --score-mel [--rounds 5]
    python scripts/slots_perf.py --score-chunks [--parent-lib PATH] [--rounds 5]
    python scripts/slots_perf.py --score [--parent-lib PATH] [--batch 12288] [--chunks 256] [--rounds 5]
    python scripts/slots_perf.py --prefill [--parent-lib PATH] [--batch 12288] [--chunks 256] [--rounds 5]
    python scripts/slots_perf.py --parent --parent-lib PATH [--batch 12288] [--chunks 256] [--rounds 5]
    python scripts/slots_perf.py --temperature --parent-lib PATH [--batch 12288] [--chunks 256,2048] [--rounds 5]
    python scripts/slots_perf.py --min-p --parent-lib PATH [--batch 12288] [--chunks 256,2048] [--rounds 5]
    python scripts/slots_perf.py --cut --parent-lib PATH [--batch 12288] [--chunks 256,2048] [--rounds 5]
    python scripts/slots_perf.py --prime --parent-lib PATH [--batch 12288] [--chunks 256,2048] [--rounds 5]
    python scripts/slots_perf.py --compact [--batch 12288] [--rounds 5]
    python scripts/slots_perf.py --serve [--batch 12288] [--chunks 256,2048] [--rounds 5]
    python scripts/slots_perf.py --drain [--batch 12288] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12288)
    ap.add_argument("--chunks", default="256,2048")
    ap.add_argument("--steps", type=int, default=6, help="timed steps per chunk size (after two warm-up steps)")
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--mel", action="store_true", help="also time slot steps fed with mel frames (distinct per column)")
    ap.add_argument("--only-mel", action="store_true", help="time the mel-fed slot steps only (e.g. under a profiler)")
    ap.add_argument("--compact", action="store_true", help="time a fragmented batch with and without compaction, moves, saves and loads")
    ap.add_argument("--rounds", type=int, default=5, help="--compact, --serve, --drain: rounds of measurements")
    ap.add_argument("--drain", action="store_true", help="time list saves (device, pinned) and list resumes against one call per column")
    ap.add_argument("--serve", action="store_true", help="time SlotStream.step / step_async against the engine-level step, and the delivery paths")
    ap.add_argument("--temperature", action="store_true", help="time the slot step of the parent commit, of this one at T = 1 and at mixed T")
    ap.add_argument("--prime", action="store_true", help="time the slot step of the parent commit, of this one without a prime and with every column primed")
    ap.add_argument("--prefill", action="store_true", help="time the sequential prime against nvw_prefill_states, 1 and 256 requests")
    ap.add_argument("--score", action="store_true", help="time nvw_score_samples against forcing the samples through primed columns of the parent")
    ap.add_argument("--score-chunks", action="store_true", help="time nvw_score_chunks against the whole pass, a request past the cap, and candidates behind a shared prefix")
    ap.add_argument("--prefill-mel", action="store_true", help="time nvw_prefill_states_mel against nvw_prefill_states on rows upsampled beforehand and against mel columns of the parent")
    ap.add_argument("--score-mel", action="store_true", help="time nvw_score_samples_mel against nvw_score_samples on rows upsampled beforehand")
    ap.add_argument("--parent", action="store_true", help="time the plain and the ragged slot step of the parent commit and of this one")
    ap.add_argument("--min-p", action="store_true", help="time the slot step of the parent commit, of this one at floor 0 and at mixed probability floors")
    ap.add_argument("--cut", action="store_true", help="time the slot step of the parent commit (plain, mixed floors) and of this one with everything off, floors only, top-k, top-p and both")
    ap.add_argument("--parent-lib", default=None, help="--parent, --temperature, --min-p, --cut, --prime: a libwavenet_infer.so built from the parent commit")
    args = ap.parse_args()
    import torch
    import bench
    from nv_wavenet_amd._lib import lib

    B, W = args.batch, args.window
    w = bench.make_weights()
    Wc, bc = bench.make_cond_layers()
    if args.prefill_mel or args.score_mel:
        if args.prefill_mel:
            print(json.dumps(time_prefill_mel(args, w, Wc, bc)), flush=True)
        if args.score_mel:
            print(json.dumps(time_score_mel(args, w, Wc, bc)), flush=True)
        return
    if args.score_chunks:
        print(json.dumps(time_score_chunks(args, w, Wc, bc)), flush=True)
        if not args.parent_lib:
            return
        print(json.dumps(time_prefill_against_parent(args, w, Wc, bc)), flush=True)
        args.parent = True
    if args.score:
        print(json.dumps(time_score(args, w, Wc, bc)), flush=True)
        if not args.parent_lib:
            return
        print(json.dumps(time_prefill_against_parent(args, w, Wc, bc)), flush=True)
        args.parent = True
    if args.prefill:
        print(json.dumps(time_prefill(args, w, Wc, bc)), flush=True)
        if not args.parent_lib:
            return
        args.parent = True
    if args.temperature or args.parent or args.prime or args.min_p or args.cut:
        assert args.parent_lib or not (args.parent or args.cut), "--parent and --cut need --parent-lib"
        for chunk in [int(c) for c in args.chunks.split(",")]:
            print(json.dumps(time_against_parent(args, w, Wc, bc, chunk)), flush=True)
        return
    if args.compact:
        print(json.dumps(time_compact(args, w, Wc, bc)), flush=True)
        return
    if args.drain:
        print(json.dumps(time_drain(args, w, Wc, bc)), flush=True)
        return
    if args.serve:
        for load in (B, max(16, B // 16)):
            for chunk in [int(c) for c in args.chunks.split(",")]:
                print(json.dumps(time_serve(args, w, Wc, bc, load, chunk)), flush=True)
        return
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    T_SRC = 65536
    LEN_MIN, LEN_MAX = 8192, 16384      # utterance lengths (0.4 to 0.7 s at 22 kHz): at chunk 256 a few hundred columns restart per step
    src = torch.randn(bench.N_COND, T_SRC, device="cuda", generator=g).half()          # the shared features
    rng = np.random.default_rng(3)
    for chunk in [int(c) for c in args.chunks.split(",")]:
        warm, steps = 2, max(2, args.steps * 256 // chunk)      # (the lockstep engine's feature buffer holds every step: 2.4 MiB per sample)
        n = (warm + steps) * chunk
        assert n <= T_SRC and chunk <= W
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        if args.only_mel:
            mel_ms, mel_restarts = time_mel(args, w, Wc, bc, chunk, warm, steps, rng)
            print(json.dumps({"batch": B, "chunk": chunk, "window": W, "mel_ms_per_step": round(mel_ms, 3)}), flush=True)
            continue

        # ---- lockstep: pack the chunk's features, generate it ----
        e = bench.build_engine(w, B, n)
        e.setConditioningWeights(Wc, bc)
        e.setSelectorSeed(5)
        s = torch.cuda.current_stream().cuda_stream
        for k in range(warm + steps):
            if k == warm:
                torch.cuda.synchronize()
                ev[0].record()
            x = src[:, k * chunk:(k + 1) * chunk]
            assert lib.nvw_pack_features(e._h, x.data_ptr(), 16, 0, x.stride(0), x.stride(1), k * chunk, chunk, s)   # (batch stride 0)
            assert lib.nvw_run_range(e._h, k * chunk, chunk, n, B, s)
        ev[1].record()
        torch.cuda.synchronize()
        lock_ms = ev[0].elapsed_time(ev[1]) / steps
        info = e.kernelInfo(B, False)
        e.close()
        torch.cuda.empty_cache()

        # ---- slots: every column busy, utterances staggered, restarted as they end ----
        e = bench.build_engine(w, B, W)
        e.setConditioningWeights(Wc, bc)
        e.setSelectorSeed(5)
        e.slotsBegin(W)
        left = np.zeros(B, dtype=np.int64)
        uid = 0
        y = torch.empty(B, chunk, dtype=torch.int32, device="cuda")
        restarts = 0
        t_host = 0.0
        for k in range(warm + steps):
            if k == warm:
                torch.cuda.synchronize()
                ev[0].record()
                restarts = 0
            h0 = time.perf_counter()
            for b in np.nonzero(left <= 0)[0]:
                length = int(rng.integers(LEN_MIN, LEN_MAX))
                off = int(rng.integers(0, T_SRC - length))
                e.slotStart(int(b), src[:, off:off + length], uid)
                uid += 1
                left[b] = length
                restarts += 1
            if k == 0:      # staggered: the first utterances are already part-way through
                left -= rng.integers(0, LEN_MIN, size=B)
                left[left <= 0] = 1
            assert e.slotsStep(chunk, y)
            left -= chunk
            t_host += time.perf_counter() - h0
        ev[1].record()
        torch.cuda.synchronize()
        slot_ms = ev[0].elapsed_time(ev[1]) / steps
        e.slotsEnd()
        e.close()
        torch.cuda.empty_cache()
        res = {"batch": B, "chunk": chunk, "window": W, "lockstep_ms_per_step": round(lock_ms, 3),
               "slots_ms_per_step": round(slot_ms, 3), "slots_rate_vs_lockstep": round(lock_ms / slot_ms, 4),
               "restarts_per_timed_step": round(restarts / steps, 1), "host_ms_per_step": round(1e3 * t_host / (warm + steps), 2),
               "kernel": info, "device": torch.cuda.get_device_name(0)}
        if args.mel:
            mel_ms, mel_restarts = time_mel(args, w, Wc, bc, chunk, warm, steps, rng)
            res.update({"mel_ms_per_step": round(mel_ms, 3), "mel_rate_vs_slots": round(slot_ms / mel_ms, 4),
                        "mel_restarts_per_timed_step": round(mel_restarts / steps, 1)})
        print(json.dumps(res), flush=True)


def time_against_parent(args, w, Wc, bc, chunk):
    """The --parent / --temperature / --min-p / --cut / --prime measurement (module docstring) for steps of `chunk` samples.  A case is (library,
    temperatures or primes, kind of step); the cases of one library and setting share an engine."""
    import ctypes as C
    import torch
    import bench
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import SLOT_PIECE
    B, W = args.batch, args.window
    sh = bench.HEAD
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    sigs = {"nvw_create_ex": (vp, [ci] * 11), "nvw_destroy": (None, [vp]), "nvw_set_embeddings": (None, [vp, vp, vp]),
            "nvw_set_layer_weights": (None, [vp, ci] + [vp] * 7), "nvw_set_out_weights": (None, [vp] * 5),
            "nvw_set_conditioning_weights": (ci, [vp, vp, vp, ci]), "nvw_set_selector_seed": (None, [vp, C.c_ulonglong]),
            "nvw_slots_begin": (ci, [vp, ci]), "nvw_slot_start": (ci, [vp, ci, vp, ci, ll, ll, ci, C.c_uint]),
            "nvw_slots_step": (ci, [vp, ci, vp, vp, vp]), "nvw_slots_end": (None, [vp]), "nvw_kernel_info": (None, [vp, ci, ci, C.c_char_p, ci]),
            "nvw_slots_step_ragged": (ll, [vp, ci, vp, vp, ll, vp, ci, vp, vp, vp]), "nvw_slots_wait": (ci, [vp, C.c_ulonglong])}

    def load(path):
        h = C.CDLL(path)
        for name, (res, argt) in sigs.items():
            getattr(h, name).restype, getattr(h, name).argtypes = res, argt
        return h

    here = load(_lib.LIB_PATH)
    here.nvw_slot_set_temperature.restype, here.nvw_slot_set_temperature.argtypes = ci, [vp, ci, C.c_float]
    here.nvw_slot_prime.restype, here.nvw_slot_prime.argtypes = ci, [vp, ci, vp, ci]
    here.nvw_slot_set_min_p.restype, here.nvw_slot_set_min_p.argtypes = ci, [vp, ci, C.c_float]
    here.nvw_slot_set_top_k.restype, here.nvw_slot_set_top_k.argtypes = ci, [vp, ci, ci]
    here.nvw_slot_set_top_p.restype, here.nvw_slot_set_top_p.argtypes = ci, [vp, ci, C.c_float]
    libs = ({"unit": here, "mixed": here} if args.temperature else {"zero": here, "floored": here} if args.min_p else
            {"off": here, "floors": here, "top_k": here, "top_p": here, "both": here} if args.cut else
            {"noprime": here, "primed": here} if args.prime else {"here": here})
    single = args.temperature or args.prime or args.min_p or args.cut      # (one kind of step, several settings of this commit)
    if args.parent_lib:
        parent = load(args.parent_lib)
        libs = dict({"parent": parent}, **libs)
        if args.cut:      # (the parent has the floors: its own floors-only step is what this commit's is held to)
            parent.nvw_slot_set_min_p.restype, parent.nvw_slot_set_min_p.argtypes = ci, [vp, ci, C.c_float]
            libs = dict({"parent": parent, "parent_floors": parent}, **{k: v for k, v in libs.items() if k != "parent"})
    kinds = ("step",) if single else ("step", "ragged")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    warm, steps = 2, max(2, args.steps * 256 // chunk)
    need = (warm + args.rounds * steps) * chunk * (1 if single else 2)      # (--parent: plain and ragged steps)
    T_SRC = need + 4096
    src = torch.randn(bench.N_COND, T_SRC, device="cuda", generator=g).half()
    rng = np.random.default_rng(3)
    offs = rng.integers(0, 4096, size=B)
    mixed = (0.7, 0.85, 1.0, 1.2)
    floors = (0.0, 0.05, 0.1, 0.25, 0.5)
    top_ks, top_ps = (0, 1, 4, 32, sh.A), (1.0, 0.5, 0.8, 0.9)
    forced = torch.randint(0, sh.A, (need,), device="cuda", generator=g, dtype=torch.int32)      # one prime for every column, as long as the run
    a = lambda x: np.ascontiguousarray(x, dtype=np.float32).ctypes.data
    engines, info = {}, {}
    for case, h in libs.items():
        e = h.nvw_create_ex(sh.R, sh.S, sh.A, 16, sh.L, sh.maxD, B, W, 0, 1, 0)
        assert e, case
        h.nvw_set_embeddings(e, a(w["embP"]), a(w["embC"]))
        for l in range(sh.L):
            h.nvw_set_layer_weights(e, l, *[a(w[k][l]) for k in ("Wprev", "Wcur", "Bh", "Wres", "Bres", "Wskip", "Bskip")])
        h.nvw_set_out_weights(e, a(w["Wzs"]), a(w["Bzs"]), a(w["Wza"]), a(w["Bza"]))
        assert h.nvw_set_conditioning_weights(e, a(Wc), a(bc), bench.N_COND)
        h.nvw_set_selector_seed(e, 5)
        assert h.nvw_slots_begin(e, W)
        for b in range(B):
            x = src[:, int(offs[b]):int(offs[b]) + need]
            assert h.nvw_slot_start(e, b, x.data_ptr(), 16, x.stride(0), x.stride(1), need, b)
            if case == "mixed":
                assert h.nvw_slot_set_temperature(e, b, mixed[b % len(mixed)])
            if case in ("zero", "floored"):
                assert h.nvw_slot_set_min_p(e, b, floors[b % len(floors)] if case == "floored" else 0.0)
            if case in ("parent_floors", "floors"):
                assert h.nvw_slot_set_min_p(e, b, floors[b % len(floors)])
            if case == "off":
                assert h.nvw_slot_set_min_p(e, b, 0.0) and h.nvw_slot_set_top_k(e, b, 0) and h.nvw_slot_set_top_p(e, b, 1.0)
            if case in ("top_k", "both"):
                assert h.nvw_slot_set_top_k(e, b, top_ks[b % len(top_ks)])
            if case in ("top_p", "both"):
                assert h.nvw_slot_set_top_p(e, b, top_ps[b % len(top_ps)])
            if case == "primed":
                assert h.nvw_slot_prime(e, b, forced.data_ptr(), need)
        buf = C.create_string_buffer(256)
        h.nvw_kernel_info(e, B, 0, buf, 256)
        engines[case], info[case] = e, buf.value.decode()
    y = torch.empty(B, chunk, dtype=torch.int32, device="cuda")
    yp = torch.empty(B * ((chunk + 7) // 8 * 8), dtype=torch.int32, pin_memory=True)      # (every piece starts at a multiple of 8)
    pieces, n_pieces, ticket = np.empty(B, dtype=SLOT_PIECE), ci(0), C.c_ulonglong(0)
    s = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(case, kind, n):
        h, e = libs[case], engines[case]
        for _ in range(n):
            if kind == "step":
                assert h.nvw_slots_step(e, chunk, y.data_ptr(), None, s)
            else:
                assert h.nvw_slots_step_ragged(e, chunk, yp.data_ptr(), None, yp.numel(), pieces.ctypes.data, B, C.byref(n_pieces),
                                               C.byref(ticket), s) > 0

    for case in libs:
        for kind in kinds:
            run(case, kind, warm)
    torch.cuda.synchronize()
    ms = {(case, kind): [] for case in libs for kind in kinds}
    host_us = {k: [] for k in ms}      # wall time of the host inside the calls (they return before the GPU has run them)
    for r in range(args.rounds):
        for kind in kinds:
            for case in (list(libs) if r % 2 == 0 else list(libs)[::-1]):      # (the order within a round alternates)
                ev[0].record()
                h0 = time.perf_counter()
                run(case, kind, steps)
                h1 = time.perf_counter()
                ev[1].record()
                if kind == "ragged":
                    assert libs[case].nvw_slots_wait(engines[case], ticket.value)
                torch.cuda.synchronize()
                ms[(case, kind)].append(ev[0].elapsed_time(ev[1]) / steps)
                host_us[(case, kind)].append(1e6 * (h1 - h0) / steps)
    for case, h in libs.items():
        h.nvw_slots_end(engines[case])
        h.nvw_destroy(engines[case])
    torch.cuda.empty_cache()
    name = lambda k: k[0] if single else "%s_%s" % k
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"batch": B, "chunk": chunk, "window": W, "rounds": args.rounds, "steps_per_round": steps,
           "ms_per_step": {name(k): [round(v, 4) for v in vs] for k, vs in ms.items()}, "median_ms_per_step": {name(k): round(v, 4) for k, v in med.items()},
           "host_us_per_call": {name(k): [round(v, 2) for v in vs] for k, vs in host_us.items()},
           "kernel": info["unit" if args.temperature else "zero" if args.min_p else "off" if args.cut else "noprime" if args.prime else "here"], "device": torch.cuda.get_device_name(0)}
    if args.temperature:
        res["mixed_temperatures"] = mixed
    if args.min_p or args.cut:
        res["mixed_floors"] = floors
    if args.cut:
        res["top_ks"], res["top_ps"] = top_ks, top_ps
    if "parent" not in libs:
        res["parent"] = "not measured (no --parent-lib)"
        return res
    res["parent_kernel"] = info["parent"]
    for what, v in (("", ms), ("host_", host_us)):      # the same rule for the time of a step and for the host's time inside the call
        for kind in kinds:
            p = ("parent", kind)
            m = {k: float(np.median(x)) for k, x in v.items()}
            spread = (max(v[p]) - min(v[p])) / m[p]
            ratios = {case: m[(case, kind)] / m[p] for case in libs if case != "parent"}
            if args.cut:      # (off against the parent's plain step, floors against the parent's floors-only step; the cutting cases are reported)
                pf = ("parent_floors", kind)
                spread_f = (max(v[pf]) - min(v[pf])) / m[pf]
                floors_ratio = m[("floors", kind)] / m[pf]
                res[what + kind] = dict({"parent_median": round(m[p], 4), "parent_spread": round(spread, 4),
                                         "parent_floors_median": round(m[pf], 4), "parent_floors_spread": round(spread_f, 4),
                                         "floors_vs_parent_floors": round(floors_ratio, 4),
                                         "within_twice_the_parent_spread": bool(ratios["off"] <= 1.0 + 2.0 * spread and
                                                                                floors_ratio <= 1.0 + 2.0 * spread_f)},
                                        **{case + "_vs_parent": round(r, 4) for case, r in ratios.items()})
                continue
            barred = [r for case, r in ratios.items() if case not in ("primed", "floored")]      # (--prime, --min-p: the primed and the floored case are reported, not barred)
            res[what + kind] = dict({"parent_median": round(m[p], 4), "parent_spread": round(spread, 4),
                                     "within_twice_the_parent_spread": bool(max(barred) <= 1.0 + 2.0 * spread)},
                                    **{case + "_vs_parent": round(r, 4) for case, r in ratios.items()})
    return res


def time_prefill(args, w, Wc, bc):
    """The --prefill measurement (module docstring)."""
    import torch
    import bench
    sh = bench.HEAD
    window = 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"shape": "R%d S%d A%d L%d maxD%d fp16" % (sh.R, sh.S, sh.A, sh.L, sh.maxD), "rounds": args.rounds, "window": window,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for count in (1, 256):
        e = bench.build_engine(w, count, window)
        e.setConditioningWeights(Wc, bc)
        e.setSelectorSeed(5)
        W = e.prefillWindow()
        res["W"] = W
        lengths = (W // 2, W, 4 * W, 24000)
        top = max(lengths)
        src = torch.randn(bench.N_COND, top + count, device="cuda", generator=g).half()
        xs = [src[:, b:b + top] for b in range(count)]                      # a request's features: the shared ones, shifted by b
        ys = torch.randint(0, sh.A, (count, top), device="cuda", generator=g, dtype=torch.int32)
        seq_out = torch.empty((count, e.slotStateBytes()), dtype=torch.uint8, device="cuda")
        pre_out = torch.empty_like(seq_out)
        s = torch.cuda.current_stream().cuda_stream

        def sequential(n):
            e.slotsBegin(window)
            for b in range(count):
                e.slotStart(b, xs[b], b, n)
                e.slotPrime(b, ys[b, :n])
            done = 0
            while done < n:
                c = min(window, n - done)
                assert e.slotsStep(c, stream=s)
                done += c
            e.slotsSaveList(range(count), stream=s, out=seq_out)

        def prefilled(n):
            e.prefillStates([(ys[b, :n], xs[b], b, 1.0) for b in range(count)], stream=s, out=pre_out)

        for n in lengths:
            ms = {"sequential": [], "prefill": []}
            for r in range(args.rounds + 1):                                # (round 0 warms both paths up: allocations, first launches)
                for name, fn in ((("sequential", sequential), ("prefill", prefilled)) if r % 2 else (("prefill", prefilled), ("sequential", sequential))):
                    torch.cuda.synchronize()
                    ev[0].record()
                    fn(n)
                    ev[1].record()
                    torch.cuda.synchronize()
                    if r:
                        ms[name].append(ev[0].elapsed_time(ev[1]))
                    if name == "sequential":
                        e.slotsEnd()
                assert torch.equal(seq_out, pre_out), "count %d, n %d: the prefilled blobs are not the sequential ones" % (count, n)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res["cases"]["%d x %d" % (count, n)] = {"sequential_ms": [round(v, 3) for v in ms["sequential"]], "prefill_ms": [round(v, 3) for v in ms["prefill"]],
                                                   "median_sequential_ms": round(med["sequential"], 3), "median_prefill_ms": round(med["prefill"], 3),
                                                   "sequential_over_prefill": round(med["sequential"] / med["prefill"], 2)}
        c = res["cases"]
        res["prefill_4W_over_W_%d" % count] = round(c["%d x %d" % (count, 4 * W)]["median_prefill_ms"] / c["%d x %d" % (count, W)]["median_prefill_ms"], 3)
        e.close()
        torch.cuda.empty_cache()
    one = res["cases"]["1 x %d" % res["W"]]
    res["one_request_at_W_faster_prefilled"] = bool(one["median_prefill_ms"] < one["median_sequential_ms"])
    return res


def _c_engine(path, w, Wc, bc, columns, window):
    """(library, engine handle) of the C3 fp16 engine through the C ABI of the library at `path` (this commit's or a parent's)"""
    import ctypes as C
    import bench
    sh = bench.HEAD
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    sigs = {"nvw_create_ex": (vp, [ci] * 11), "nvw_destroy": (None, [vp]), "nvw_set_embeddings": (None, [vp, vp, vp]),
            "nvw_set_layer_weights": (None, [vp, ci] + [vp] * 7), "nvw_set_out_weights": (None, [vp] * 5),
            "nvw_set_conditioning_weights": (ci, [vp, vp, vp, ci]), "nvw_set_selector_seed": (None, [vp, C.c_ulonglong]),
            "nvw_slots_begin": (ci, [vp, ci]), "nvw_slot_start": (ci, [vp, ci, vp, ci, ll, ll, ci, C.c_uint]),
            "nvw_slots_step": (ci, [vp, ci, vp, vp, vp]), "nvw_slots_end": (None, [vp]), "nvw_slot_prime": (ci, [vp, ci, vp, ci]),
            "nvw_prefill_window": (ci, [vp]), "nvw_prefill_states": (ci, [vp, vp, ci, vp, ll, vp]), "nvw_slot_state_bytes": (C.c_size_t, [vp])}
    more = {"nvw_score_max_samples": (ci, [vp]), "nvw_score_samples": (ci, [vp, vp, ci, vp]), "nvw_score_chunks": (ci, [vp, vp, ci, vp])}
    h = C.CDLL(path)
    for name, (res, argt) in sigs.items():
        getattr(h, name).restype, getattr(h, name).argtypes = res, argt
    for name, (res, argt) in more.items():          # (a parent's library may lack the later entries)
        if hasattr(h, name):
            getattr(h, name).restype, getattr(h, name).argtypes = res, argt
    a = lambda x: np.ascontiguousarray(x, dtype=np.float32).ctypes.data
    e = h.nvw_create_ex(sh.R, sh.S, sh.A, 16, sh.L, sh.maxD, columns, window, 0, 1, 0)
    assert e, path
    h.nvw_set_embeddings(e, a(w["embP"]), a(w["embC"]))
    for l in range(sh.L):
        h.nvw_set_layer_weights(e, l, *[a(w[k][l]) for k in ("Wprev", "Wcur", "Bh", "Wres", "Bres", "Wskip", "Bskip")])
    h.nvw_set_out_weights(e, a(w["Wzs"]), a(w["Bzs"]), a(w["Wza"]), a(w["Bza"]))
    assert h.nvw_set_conditioning_weights(e, a(Wc), a(bc), bench.N_COND)
    h.nvw_set_selector_seed(e, 5)
    return h, e


def time_score(args, w, Wc, bc):
    """The --score measurement (module docstring)."""
    import torch
    import bench
    from nv_wavenet_amd._lib import lib
    from nv_wavenet_amd.engine import SCORE_REQ
    sh = bench.HEAD
    window = 4096
    peak = 2.5e15                                   # dense fp16 MFMA, FLOP/s
    macs = sh.L * (2 * 2 * sh.R * sh.R + 2 * sh.R * bench.N_COND + sh.R * sh.S) + (sh.L - 1) * sh.R * sh.R + sh.A * sh.S + sh.A * sh.A
    g = torch.Generator(device="cuda")
    g.manual_seed(13)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    s = torch.cuda.current_stream().cuda_stream
    res = {"shape": "R%d S%d A%d L%d maxD%d fp16" % (sh.R, sh.S, sh.A, sh.L, sh.maxD), "rounds": args.rounds, "window": window,
           "multiply_adds_per_sample": macs, "device": torch.cuda.get_device_name(0), "cases": {}}
    for count in (1, 256):
        e = bench.build_engine(w, count, window)
        e.setConditioningWeights(Wc, bc)
        cap = e.scoreMaxSamples()
        res["score_max_samples"] = cap
        parent = _c_engine(args.parent_lib, w, Wc, bc, count, window) if args.parent_lib else None
        lengths = (2048, 24000)
        top = max(lengths)
        src = torch.randn(bench.N_COND, top + count, device="cuda", generator=g).half()
        xs = [src[:, b:b + top] for b in range(count)]                      # a request's features: the shared ones, shifted by b
        ys = torch.randint(0, sh.A, (count, top), device="cuda", generator=g, dtype=torch.int32)
        logp = torch.empty((count, top), dtype=torch.float32, device="cuda")
        for n in lengths:
            per_call = max(1, min(count, cap // (-(-n // 16) * 16)))
            rows = torch.empty((per_call, n, sh.A), dtype=torch.float32, device="cuda")      # (of one call: the next one writes over it)
            calls = []
            for with_rows in (False, True):
                groups = []
                for b0 in range(0, count, per_call):
                    reqs = np.zeros(per_call, dtype=SCORE_REQ)
                    k = min(per_call, count - b0)
                    for i in range(k):
                        b = b0 + i
                        reqs[i] = (ys[b].data_ptr(), n, xs[b].data_ptr(), 16, xs[b].stride(0), xs[b].stride(1), 1.0, logp[b].data_ptr(),
                                   rows[i].data_ptr() if with_rows else 0)
                    groups.append((reqs, k))
                calls.append(groups)

            def score(groups):
                for reqs, k in groups:
                    assert lib.nvw_score_samples(e._h, reqs.ctypes.data, k, s) == k

            def forced():
                h, pe = parent
                assert h.nvw_slots_begin(pe, window)
                for b in range(count):
                    assert h.nvw_slot_start(pe, b, xs[b].data_ptr(), 16, xs[b].stride(0), xs[b].stride(1), n, b)
                    assert h.nvw_slot_prime(pe, b, ys[b].data_ptr(), n)
                done = 0
                while done < n:
                    c = min(window, n - done)
                    assert h.nvw_slots_step(pe, c, None, None, s)
                    done += c

            paths = [("score", lambda: score(calls[0])), ("score_rows", lambda: score(calls[1]))] + ([("parent_forced", forced)] if parent else [])
            ms = {name: [] for name, _ in paths}
            for r in range(args.rounds + 1):                                # (round 0 warms every path up: allocations, first launches)
                for name, fn in (paths if r % 2 else paths[::-1]):
                    torch.cuda.synchronize()
                    ev[0].record()
                    fn()
                    ev[1].record()
                    torch.cuda.synchronize()
                    if r:
                        ms[name].append(ev[0].elapsed_time(ev[1]))
                    if name == "parent_forced":
                        parent[0].nvw_slots_end(parent[1])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            case = {"calls": len(calls[0]), "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                    "median_ms": {k: round(v, 3) for k, v in med.items()},
                    "us_per_sample": {k: round(1e3 * v / (count * n), 4) for k, v in med.items()},
                    "fraction_of_fp16_mfma_peak": round(2.0 * macs * count * n / (1e-3 * med["score"]) / peak, 4)}
            if parent:
                case["parent_forced_over_score"] = round(med["parent_forced"] / med["score"], 2)
            res["cases"]["%d x %d" % (count, n)] = case
            del rows
        if parent:
            parent[0].nvw_destroy(parent[1])
        e.close()
        torch.cuda.empty_cache()
    if args.parent_lib:
        res["scoring_256_costs_less_than_forcing_them"] = bool(all(c["median_ms"]["score"] < c["median_ms"]["parent_forced"]
                                                                    for k, c in res["cases"].items() if k.startswith("256 ")))
    return res


def time_score_chunks(args, w, Wc, bc):
    """The --score-chunks measurement (C3 fp16, one process, medians of --rounds rounds with every round listed):
    nvw_score_samples of this commit's library against the parent's over 256 requests of 24 000 samples (a guard, held to twice the
    parent's own spread); nvw_score_chunks over the same samples in time chunks of 2 048 and 16 384 against the whole pass (the
    blocking reads of the in-states' headers included); one request of 1 500 000 samples, which the whole pass refuses, in chunks
    of 65 536; and 64 candidates of 256 samples behind one prefix of 24 000 -- the candidates alone behind a state at hand, the
    prefix scored once with its out-state and then the candidates, and the only way without carried state: 64 whole scorings of
    24 256."""
    import torch
    import bench
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import SCORE_CHUNK_REQ, SCORE_REQ
    sh = bench.HEAD
    count, n, window = 256, 24000, 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(19)
    s = torch.cuda.current_stream().cuda_stream
    libs = {"here": _c_engine(_lib.LIB_PATH, w, Wc, bc, count, window)}
    if args.parent_lib:
        libs["parent"] = _c_engine(args.parent_lib, w, Wc, bc, count, window)
    h, e = libs["here"]
    cap = h.nvw_score_max_samples(e)
    nbytes = int(h.nvw_slot_state_bytes(e))
    src = torch.randn(bench.N_COND, n + 256 + count, device="cuda", generator=g).half()
    xs = [src[:, b:b + n + 256] for b in range(count)]
    ys = torch.randint(0, sh.A, (count, n + 256), device="cuda", generator=g, dtype=torch.int32)
    logp = torch.empty((count, n + 256), dtype=torch.float32, device="cuda")
    keep = logp.clone()
    states = [torch.empty((count, nbytes), dtype=torch.uint8, device="cuda") for _ in range(2)]
    res = {"shape": "R%d S%d A%d L%d maxD%d fp16" % (sh.R, sh.S, sh.A, sh.L, sh.maxD), "rounds": args.rounds, "score_max_samples": cap,
           "state_bytes": nbytes, "device": torch.cuda.get_device_name(0)}

    def pad(k):
        return -(-k // 16) * 16

    def whole_calls(length, first=0, many=count):
        per, out = max(1, min(many, cap // pad(length))), []
        for b0 in range(0, many, per):
            k = min(per, many - b0)
            reqs = np.zeros(k, dtype=SCORE_REQ)
            for i in range(k):
                b = first + b0 + i
                reqs[i] = (ys[b].data_ptr(), length, xs[b].data_ptr(), 16, xs[b].stride(0), xs[b].stride(1), 1.0, logp[b].data_ptr(), 0)
            out.append((reqs, k))
        return out

    def whole(lib, calls):
        for reqs, k in calls:
            assert lib[0].nvw_score_samples(lib[1], reqs.ctypes.data, k, s) == k

    def chunk_calls(step):
        """[(requests, count)] of all of [0, n) in time chunks of `step`, every request from the out-state of its previous chunk"""
        per, out = max(1, min(count, cap // pad(step))), []
        for si, k0 in enumerate(range(0, n, step)):
            m = min(step, n - k0)
            src_st, dst_st = states[(si + 1) % 2], states[si % 2]
            for b0 in range(0, count, per):
                k = min(per, count - b0)
                reqs = np.zeros(k, dtype=SCORE_CHUNK_REQ)
                for i in range(k):
                    b = b0 + i
                    reqs[i] = (src_st[b].data_ptr() if si else 0, ys[b].data_ptr() + 4 * k0, m, xs[b].data_ptr() + 2 * k0 * xs[b].stride(1), 16,
                               xs[b].stride(0), xs[b].stride(1), b, 1.0, logp[b].data_ptr() + 4 * k0, 0, dst_st[b].data_ptr())
                out.append((reqs, k))
        return out

    def chunks(calls):
        for reqs, k in calls:
            assert h.nvw_score_chunks(e, reqs.ctypes.data, k, s) == k

    calls = whole_calls(n)
    by_step = {step: chunk_calls(step) for step in (2048, 16384)}
    paths = [("whole_here", lambda: whole(libs["here"], calls))] + ([("whole_parent", lambda: whole(libs["parent"], calls))] if args.parent_lib else [])
    paths += [("chunks_%d" % step, (lambda c: lambda: chunks(c))(c)) for step, c in by_step.items()]
    whole(libs["here"], calls)
    torch.cuda.synchronize()
    keep.copy_(logp)
    for step, c in by_step.items():
        logp.zero_()
        chunks(c)
        torch.cuda.synchronize()
        assert torch.equal(logp[:, :n].view(torch.int32), keep[:, :n].view(torch.int32)), "chunks of %d differ from the whole pass" % step
    ms = _timed_rounds(paths, args.rounds)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    case = {"calls": {"whole": len(calls), **{"chunks_%d" % st: len(c) for st, c in by_step.items()}},
            "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "median_ms": {k: round(v, 3) for k, v in med.items()},
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
            "chunks_over_whole": {k: round(med[k] / med["whole_here"], 4) for k in med if k.startswith("chunks_")}, "bit_equal": True}
    if args.parent_lib:
        spread = (max(ms["whole_parent"]) - min(ms["whole_parent"])) / med["whole_parent"]
        case.update(parent_spread=round(spread, 4), here_vs_parent=round(med["whole_here"] / med["whole_parent"], 4),
                    within_twice_the_parent_spread=bool(med["whole_here"] / med["whole_parent"] <= 1.0 + 2.0 * spread))
    res["256 x 24000"] = case

    # one request past the cap
    long_n, step = 1500000, 65536
    assert pad(long_n) > cap
    lx = torch.randn(bench.N_COND, long_n, device="cuda", generator=g).half()
    ly = torch.randint(0, sh.A, (long_n,), device="cuda", generator=g, dtype=torch.int32)
    ll = torch.empty(long_n, dtype=torch.float32, device="cuda")
    one = np.zeros(1, dtype=SCORE_REQ)
    one[0] = (ly.data_ptr(), long_n, lx.data_ptr(), 16, lx.stride(0), lx.stride(1), 1.0, ll.data_ptr(), 0)
    refused = {name: lib[0].nvw_score_samples(lib[1], one.ctypes.data, 1, s) == 0 for name, lib in libs.items()}
    lcalls = []
    for si, k0 in enumerate(range(0, long_n, step)):
        m = min(step, long_n - k0)
        reqs = np.zeros(1, dtype=SCORE_CHUNK_REQ)
        reqs[0] = (states[(si + 1) % 2][0].data_ptr() if si else 0, ly.data_ptr() + 4 * k0, m, lx.data_ptr() + 2 * k0 * lx.stride(1), 16,
                   lx.stride(0), lx.stride(1), 1, 1.0, ll.data_ptr() + 4 * k0, 0, states[si % 2][0].data_ptr())
        lcalls.append((reqs, 1))
    ms = _timed_rounds([("chunks_65536", lambda: chunks(lcalls))], args.rounds)
    m0 = float(np.median(ms["chunks_65536"]))
    # (its first 24 000 samples are what the whole pass gives for them)
    head = np.zeros(1, dtype=SCORE_REQ)
    head[0] = (ly.data_ptr(), n, lx.data_ptr(), 16, lx.stride(0), lx.stride(1), 1.0, logp[0].data_ptr(), 0)
    assert h.nvw_score_samples(e, head.ctypes.data, 1, s) == 1
    torch.cuda.synchronize()
    res["1 x 1500000"] = {"whole_pass_refuses": refused, "calls": len(lcalls), "ms": [round(x, 3) for x in ms["chunks_65536"]], "median_ms": round(m0, 3),
                          "us_per_sample": round(1e3 * m0 / long_n, 4), "seconds_of_24_kHz_audio": round(long_n / 24000.0, 1),
                          "first_24000_bit_equal_to_the_whole_pass": bool(torch.equal(ll[:n].view(torch.int32), logp[0, :n].view(torch.int32)))}
    del lx, ly, ll

    # 64 candidates of 256 behind one prefix of 24 000 (utterance 0's; candidate c = the samples of utterance c behind it)
    K, m = 64, 256
    prefix = np.zeros(1, dtype=SCORE_CHUNK_REQ)
    prefix[0] = (0, ys[0].data_ptr(), n, xs[0].data_ptr(), 16, xs[0].stride(0), xs[0].stride(1), 0, 1.0, logp[0].data_ptr(), 0, states[0][0].data_ptr())
    cand_y = ys[:K, n:n + m].contiguous()
    cand_lp = torch.empty((K, m), dtype=torch.float32, device="cuda")
    cands = np.zeros(K, dtype=SCORE_CHUNK_REQ)
    for c in range(K):
        cands[c] = (states[0][0].data_ptr(), cand_y[c].data_ptr(), m, xs[0].data_ptr() + 2 * n * xs[0].stride(1), 16, xs[0].stride(0), xs[0].stride(1),
                    0, 1.0, cand_lp[c].data_ptr(), 0, 0)
    full_y = torch.cat([ys[0, :n].unsqueeze(0).expand(K, n), cand_y], dim=1).contiguous()
    full_lp = torch.empty((K, n + m), dtype=torch.float32, device="cuda")
    per = max(1, min(K, cap // pad(n + m)))
    fcalls = []
    for b0 in range(0, K, per):
        k = min(per, K - b0)
        reqs = np.zeros(k, dtype=SCORE_REQ)
        for i in range(k):
            reqs[i] = (full_y[b0 + i].data_ptr(), n + m, xs[0].data_ptr(), 16, xs[0].stride(0), xs[0].stride(1), 1.0, full_lp[b0 + i].data_ptr(), 0)
        fcalls.append((reqs, k))
    paths = [("candidates_behind_a_state", lambda: chunks([(cands, K)])), ("prefix_then_candidates", lambda: chunks([(prefix, 1), (cands, K)])),
             ("whole_scorings", lambda: whole(libs["parent" if args.parent_lib else "here"], fcalls))]
    chunks([(prefix, 1), (cands, K)])
    whole(libs["here"], fcalls)
    torch.cuda.synchronize()
    assert torch.equal(cand_lp.view(torch.int32), full_lp[:, n:].view(torch.int32)), "the candidates' tails differ from the whole scorings"
    ms = _timed_rounds(paths, args.rounds)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res["64 x 256 behind 24000"] = {"whole_scorings_by": "parent" if args.parent_lib else "here", "whole_calls": len(fcalls),
                                    "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "median_ms": {k: round(v, 3) for k, v in med.items()},
                                    "whole_over_prefix_then_candidates": round(med["whole_scorings"] / med["prefix_then_candidates"], 2),
                                    "whole_over_candidates_behind_a_state": round(med["whole_scorings"] / med["candidates_behind_a_state"], 2),
                                    "bit_equal": True}
    for lib in libs.values():
        lib[0].nvw_destroy(lib[1])
    return res


def time_prefill_against_parent(args, w, Wc, bc):
    """nvw_prefill_states of the parent's library and of this one, 256 requests at n = W, alternating rounds (a guard: nothing on
    that path changes)."""
    import torch
    import bench
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import PREFILL_REQ
    sh = bench.HEAD
    count, window = 256, 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    libs = {"parent": _c_engine(args.parent_lib, w, Wc, bc, count, window), "here": _c_engine(_lib.LIB_PATH, w, Wc, bc, count, window)}
    W = libs["here"][0].nvw_prefill_window(libs["here"][1])
    src = torch.randn(bench.N_COND, W + count, device="cuda", generator=g).half()
    ys = torch.randint(0, sh.A, (count, W), device="cuda", generator=g, dtype=torch.int32)
    nbytes = int(libs["here"][0].nvw_slot_state_bytes(libs["here"][1]))
    out = {k: torch.empty((count, nbytes), dtype=torch.uint8, device="cuda") for k in libs}
    reqs = np.zeros(count, dtype=PREFILL_REQ)
    for b in range(count):
        x = src[:, b:b + W]
        reqs[b] = (ys[b].data_ptr(), W, x.data_ptr(), 16, x.stride(0), x.stride(1), b, 1.0)
    s = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in libs}
    for r in range(args.rounds + 1):
        for name in (list(libs) if r % 2 else list(libs)[::-1]):
            h, e = libs[name]
            torch.cuda.synchronize()
            ev[0].record()
            assert h.nvw_prefill_states(e, reqs.ctypes.data, count, out[name].data_ptr(), nbytes, s) == count
            ev[1].record()
            torch.cuda.synchronize()
            if r:
                ms[name].append(ev[0].elapsed_time(ev[1]))
    assert torch.equal(out["parent"], out["here"]), "the prefilled blobs of the two libraries differ"
    for h, e in libs.values():
        h.nvw_destroy(e)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = (max(ms["parent"]) - min(ms["parent"])) / med["parent"]
    return {"prefill_256_at_W": W, "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}, "median_ms": {k: round(v, 3) for k, v in med.items()},
            "parent_spread": round(spread, 4), "here_vs_parent": round(med["here"] / med["parent"], 4),
            "within_twice_the_parent_spread": bool(med["here"] / med["parent"] <= 1.0 + 2.0 * spread), "blobs_equal": True}


def _up_weights():
    """the upsampling of time_mel: window 1024 / stride 256"""
    import bench
    r = np.random.default_rng(11)
    up_w = ((r.random((bench.N_COND, bench.N_COND, bench.UP_WINDOW), dtype=np.float32) - 0.5) *
            (np.sqrt(12.0) / np.sqrt(4 * bench.N_COND))).astype(np.float32)
    return up_w, np.zeros(bench.N_COND, dtype=np.float32)


def _timed_rounds(paths, rounds, after=None):
    """{name: [ms per round]} of the paths, alternating their order; round 0 warms every path up and is dropped"""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {name: [] for name, _ in paths}
    for r in range(rounds + 1):
        for name, fn in (paths if r % 2 else paths[::-1]):
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if r:
                ms[name].append(ev[0].elapsed_time(ev[1]))
            if after:
                after(name)
    return ms


def time_prefill_mel(args, w, Wc, bc):
    """The --prefill-mel measurement (C3 fp16, window 1024 / stride 256, one process): nvw_prefill_states_mel for 1 and 256 requests
    at n = W/2, W, 4W and 24 000, beside nvw_prefill_states of this commit on rows upsampled beforehand (the difference is the
    upsampling's share), beside nvw_upsample_requests alone, and -- with --parent-lib -- beside the same primes forced through mel
    columns of the PARENT's library (nvw_slot_start_mel + nvw_slot_prime, steps of the window up to sample n): the only way the
    parent can do it."""
    import ctypes as C
    import torch
    import bench
    from nv_wavenet_amd._lib import lib
    from nv_wavenet_amd.engine import PREFILL_MEL_REQ, PREFILL_REQ, UPSAMPLE_REQ
    sh = bench.HEAD
    window, stride = 4096, bench.UP_STRIDE
    up_w, up_b = _up_weights()
    g = torch.Generator(device="cuda")
    g.manual_seed(19)
    s = torch.cuda.current_stream().cuda_stream
    res = {"shape": "R%d S%d A%d L%d maxD%d fp16" % (sh.R, sh.S, sh.A, sh.L, sh.maxD), "upsampling": "%d / %d" % (bench.UP_WINDOW, stride),
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "cases": {}}
    for count in (1, 256):
        e = bench.build_engine(w, count, window)
        e.setConditioningWeights(Wc, bc)
        e.setUpsampling(up_w, up_b, stride)
        e.setSelectorSeed(5)
        W, row = e.prefillWindow(), e.upsampleRowElems()
        res["W"] = W
        parent = None
        if args.parent_lib:
            parent = _c_engine(args.parent_lib, w, Wc, bc, count, window)
            h = parent[0]
            h.nvw_set_upsampling.restype, h.nvw_set_upsampling.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            h.nvw_slot_start_mel.restype = C.c_int
            h.nvw_slot_start_mel.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_uint]
            assert h.nvw_set_upsampling(parent[1], up_w.ctypes.data, up_b.ctypes.data, bench.UP_WINDOW, stride)
        lengths = (W // 2, W, 4 * W, 24000)
        top = max(lengths)
        frames = -(-top // stride)
        mel = torch.randn(count, bench.N_COND, frames, device="cuda", generator=g).half()      # distinct frames for every request
        ys = torch.randint(0, sh.A, (count, top), device="cuda", generator=g, dtype=torch.int32)
        nbytes = e.slotStateBytes()
        out = {k: torch.empty((count, nbytes), dtype=torch.uint8, device="cuda") for k in ("mel", "rows")}
        for n in lengths:
            t0 = (max(0, n - W) // 16) * 16
            # (a feature pass indexes by the absolute sample: t0 rows of padding in front keep every derived base inside the buffer)
            buf = torch.empty((t0 + count * (n - t0), row), dtype=torch.float16, device="cuda")
            rows = buf[t0:].view(count, n - t0, row)
            rm, rr, ru = np.zeros(count, dtype=PREFILL_MEL_REQ), np.zeros(count, dtype=PREFILL_REQ), np.zeros(count, dtype=UPSAMPLE_REQ)
            for b in range(count):
                m = mel[b]
                rm[b] = (ys[b].data_ptr(), n, m.data_ptr(), 16, m.stride(0), m.stride(1), frames, b, 1.0)
                ru[b] = (m.data_ptr(), 16, m.stride(0), m.stride(1), frames, t0, n - t0, rows[b].data_ptr())
                rr[b] = (ys[b].data_ptr(), n, rows[b].data_ptr() - t0 * row * 2, 16, 1, row, b, 1.0)

            def from_mel():
                assert lib.nvw_prefill_states_mel(e._h, rm.ctypes.data, count, out["mel"].data_ptr(), nbytes, s) == count

            def from_rows():
                assert lib.nvw_prefill_states(e._h, rr.ctypes.data, count, out["rows"].data_ptr(), nbytes, s) == count

            def upsample():
                assert lib.nvw_upsample_requests(e._h, ru.ctypes.data, count, s) == count

            def forced():
                h, pe = parent
                assert h.nvw_slots_begin(pe, window)
                for b in range(count):
                    assert h.nvw_slot_start_mel(pe, b, mel[b].data_ptr(), 16, mel[b].stride(0), mel[b].stride(1), frames, 1, b)
                    assert h.nvw_slot_prime(pe, b, ys[b].data_ptr(), n)
                done = 0
                while done < n:
                    c = min(window, n - done)
                    assert h.nvw_slots_step(pe, c, None, None, s)
                    done += c

            upsample()
            paths = [("prefill_mel", from_mel), ("prefill_rows", from_rows), ("upsample", upsample)] + ([("parent_forced", forced)] if parent else [])
            ms = _timed_rounds(paths, args.rounds, lambda name: parent[0].nvw_slots_end(parent[1]) if name == "parent_forced" else None)
            assert torch.equal(out["mel"], out["rows"]), "count %d, n %d: the blobs from mel are not those from the rows" % (count, n)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            case = {"ms": {k: _stats(v) for k, v in ms.items()}, "upsampling_share": round((med["prefill_mel"] - med["prefill_rows"]) / med["prefill_mel"], 3)}
            if parent:
                case["parent_forced_over_prefill_mel"] = round(med["parent_forced"] / med["prefill_mel"], 2)
            res["cases"]["%d x %d" % (count, n)] = case
            del rows, buf
        if parent:
            parent[0].nvw_destroy(parent[1])
        e.close()
        torch.cuda.empty_cache()
    return res


def time_score_mel(args, w, Wc, bc):
    """The --score-mel measurement: nvw_score_samples_mel for 1 and 256 requests at n = 2 048 and 24 000 beside nvw_score_samples of
    this commit on rows upsampled beforehand, and nvw_upsample_requests alone; calls split at nvw_score_max_samples as --score does."""
    import torch
    import bench
    from nv_wavenet_amd._lib import lib
    from nv_wavenet_amd.engine import SCORE_MEL_REQ, SCORE_REQ, UPSAMPLE_REQ
    sh = bench.HEAD
    window, stride = 4096, bench.UP_STRIDE
    up_w, up_b = _up_weights()
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    s = torch.cuda.current_stream().cuda_stream
    res = {"shape": "R%d S%d A%d L%d maxD%d fp16" % (sh.R, sh.S, sh.A, sh.L, sh.maxD), "upsampling": "%d / %d" % (bench.UP_WINDOW, stride),
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "cases": {}}
    for count in (1, 256):
        e = bench.build_engine(w, count, window)
        e.setConditioningWeights(Wc, bc)
        e.setUpsampling(up_w, up_b, stride)
        cap, row = e.scoreMaxSamples(), e.upsampleRowElems()
        lengths = (2048, 24000)
        top = max(lengths)
        frames = -(-top // stride)
        mel = torch.randn(count, bench.N_COND, frames, device="cuda", generator=g).half()
        ys = torch.randint(0, sh.A, (count, top), device="cuda", generator=g, dtype=torch.int32)
        logp = {k: torch.empty((count, top), dtype=torch.float32, device="cuda") for k in ("mel", "rows")}
        for n in lengths:
            per_call = max(1, min(count, cap // (-(-n // 16) * 16)))
            rows = torch.empty((count, n, row), dtype=torch.float16, device="cuda")
            groups = []
            for b0 in range(0, count, per_call):
                k = min(per_call, count - b0)
                rm, rr, ru = np.zeros(k, dtype=SCORE_MEL_REQ), np.zeros(k, dtype=SCORE_REQ), np.zeros(k, dtype=UPSAMPLE_REQ)
                for i in range(k):
                    b = b0 + i
                    m = mel[b]
                    rm[i] = (ys[b].data_ptr(), n, m.data_ptr(), 16, m.stride(0), m.stride(1), frames, 1.0, logp["mel"][b].data_ptr(), 0)
                    ru[i] = (m.data_ptr(), 16, m.stride(0), m.stride(1), frames, 0, n, rows[b].data_ptr())
                    rr[i] = (ys[b].data_ptr(), n, rows[b].data_ptr(), 16, 1, row, 1.0, logp["rows"][b].data_ptr(), 0)
                groups.append((rm, rr, ru, k))

            def from_mel():
                for rm, rr, ru, k in groups:
                    assert lib.nvw_score_samples_mel(e._h, rm.ctypes.data, k, s) == k

            def from_rows():
                for rm, rr, ru, k in groups:
                    assert lib.nvw_score_samples(e._h, rr.ctypes.data, k, s) == k

            def upsample():
                for rm, rr, ru, k in groups:
                    assert lib.nvw_upsample_requests(e._h, ru.ctypes.data, k, s) == k

            upsample()
            ms = _timed_rounds([("score_mel", from_mel), ("score_rows", from_rows), ("upsample", upsample)], args.rounds)
            assert torch.equal(logp["mel"][:, :n], logp["rows"][:, :n]), "count %d, n %d: the scores from mel are not those from the rows" % (count, n)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res["cases"]["%d x %d" % (count, n)] = {"calls": len(groups), "ms": {k: _stats(v) for k, v in ms.items()},
                                                   "upsampling_share": round((med["score_mel"] - med["score_rows"]) / med["score_mel"], 3),
                                                   "upsample_GB_per_s_written": round(count * n * row * 2 / (1e-3 * med["upsample"]) / 1e9, 1)}
            del rows
        e.close()
        torch.cuda.empty_cache()
    return res


def time_mel(args, w, Wc, bc, chunk, warm, steps, rng):
    """ms per slot step with every column a mel column of its own frames (module docstring); restarts in the timed steps."""
    import torch
    import bench
    B, W = args.batch, args.window
    LEN_MIN, LEN_MAX = 8192, 16384
    stride, frames_max = bench.UP_STRIDE, 16384 // bench.UP_STRIDE
    e = bench.build_engine(w, B, W)
    e.setConditioningWeights(Wc, bc)
    r = np.random.default_rng(11)
    up_w = ((r.random((bench.N_COND, bench.N_COND, bench.UP_WINDOW), dtype=np.float32) - 0.5) *
            (np.sqrt(12.0) / np.sqrt(4 * bench.N_COND))).astype(np.float32)
    e.setUpsampling(up_w, np.zeros(bench.N_COND, dtype=np.float32), stride)
    e.setSelectorSeed(5)
    e.slotsBegin(W)
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    mel = torch.randn(B, bench.N_COND, frames_max, device="cuda", generator=g).half()      # distinct frames for every column
    y = torch.empty(B, chunk, dtype=torch.int32, device="cuda")
    left = np.zeros(B, dtype=np.int64)
    uid = 0

    def start(b):
        nonlocal uid
        frames = int(rng.integers(LEN_MIN, LEN_MAX)) // stride
        e.slotStartMel(int(b), mel[b], uid, frames=frames)
        uid += 1
        left[b] = frames * stride

    # staggered phases: column j of every tile joins after j steps of 17 samples
    for j in range(16):
        for b in range(j, B, 16):
            start(b)
        assert e.slotsStep(17, y)
        left[left > 0] -= 17
    left -= rng.integers(0, LEN_MIN // 2, size=B)      # (and their ends spread: restarts in every step, as for the features)
    left[left <= 0] = 1
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    restarts = 0
    for k in range(warm + steps):
        if k == warm:
            torch.cuda.synchronize()
            ev[0].record()
            restarts = 0
        for b in np.nonzero(left <= 0)[0]:
            start(b)
            restarts += 1
        assert e.slotsStep(chunk, y)
        left -= chunk
    ev[1].record()
    torch.cuda.synchronize()
    e.slotsEnd()
    e.close()
    del mel
    torch.cuda.empty_cache()
    return ev[0].elapsed_time(ev[1]) / steps, restarts


def _stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def time_serve(args, w, Wc, bc, load, chunk):
    """The --serve measurement (module docstring) with `load` utterances in flight on args.batch columns."""
    import torch
    import bench
    from nv_wavenet_amd._lib import lib
    from nv_wavenet_amd.slots import SlotStream
    B, W = args.batch, args.window
    T_SRC, LEN_MIN, LEN_MAX = 65536, 8192, 16384
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    src = torch.randn(bench.N_COND, T_SRC, device="cuda", generator=g).half()
    steps = max(2, 3 * 2048 // chunk // (1 if chunk >= 1024 else 2))      # per round: 3 of 2048, 12 of 256
    warm = 2
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"batch": B, "load": load, "chunk": chunk, "window": W, "rounds": args.rounds, "steps_per_round": steps,
           "realtime_budget_ms": round(1e3 * chunk / 24000.0, 2), "device": torch.cuda.get_device_name(0)}

    def engine():
        e = bench.build_engine(w, B, W)
        e.setConditioningWeights(Wc, bc)
        e.setSelectorSeed(5)
        return e

    def window_of(rng, first):
        length = int(rng.integers(256 if first else LEN_MIN, LEN_MAX))      # (the first wave ends staggered)
        off = int(rng.integers(0, T_SRC - length))
        return src[:, off:off + length], length

    # ---- (i) engine level, and (iv) the delivery paths on the same session ----
    rng = np.random.default_rng(3)
    e = engine()
    e.slotsBegin(W)
    left = np.zeros(B, dtype=np.int64)
    left[load:] = 1 << 60
    uid = [0]
    y = torch.empty(B, chunk, dtype=torch.int32, device="cuda")
    pcm = torch.empty(B, chunk, dtype=torch.int16, device="cuda")
    cap = B * ((chunk + 7) & ~7)
    dev = (torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int16, device="cuda"))
    pin = e.slotsPinned(cap)
    first = [True]

    def restart():
        for b in np.nonzero(left <= 0)[0]:
            x, length = window_of(rng, first[0])
            e.slotStart(int(b), x, uid[0])
            uid[0] += 1
            left[b] = length
        first[0] = False

    def timed(n):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(n):
            restart()
            assert e.slotsStep(chunk, y)
            left[:load] -= chunk
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    def outputs(is_ragged, ys, ps, reps=3):
        """ms per pass of the output path alone over the last step's samples (nvw_slots_time_outputs: events around the launches)"""
        ms = lib.nvw_slots_time_outputs(e._h, 1 if is_ragged else 0, chunk, ys.data_ptr(), ps.data_ptr(), ys.numel(), reps, None)
        assert ms >= 0
        return ms / reps

    def staging_copy(total, reps=3):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            pin[0][:total].copy_(dev[0][:total], non_blocking=True)
            pin[1][:total].copy_(dev[1][:total], non_blocking=True)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    timed(warm)
    rows_pin = (torch.empty(B * chunk, dtype=torch.int32, pin_memory=True), torch.empty(B * chunk, dtype=torch.int16, pin_memory=True))
    keys = ("plain_rows_to_device", "plain_rows_to_pinned", "ragged_to_device", "ragged_to_pinned_direct", "staging_copy_alone")
    t = {k: [] for k in keys}
    t_engine = []
    total = 0
    for _ in range(args.rounds):
        t_engine.append(timed(steps))
        restart()
        total, pieces, ticket = e.slotsStepRagged(chunk, *dev)      # (the ragged size of this load, and a step whose rows the passes read)
        left[:load] -= chunk
        t["plain_rows_to_device"].append(outputs(False, y.view(-1), pcm.view(-1)))
        t["plain_rows_to_pinned"].append(outputs(False, *rows_pin))
        t["ragged_to_device"].append(outputs(True, *dev))
        t["ragged_to_pinned_direct"].append(outputs(True, *pin))
        t["staging_copy_alone"].append(staging_copy(total))
    res["engine_ms_per_step"] = _stats(t_engine)
    res["output_path_ms"] = {k: _stats(v) for k, v in t.items()}
    res["output_path_ms"]["ragged_to_device_then_copy_to_pinned"] = _stats([a + b for a, b in zip(t["ragged_to_device"], t["staging_copy_alone"])])
    res["delivered_bytes_per_step"] = {"plain": B * chunk * 6, "ragged": int(total) * 6}
    del rows_pin
    torch.cuda.synchronize()
    e.slotsEnd()
    e.close()
    del y, pcm, dev, pin
    torch.cuda.empty_cache()

    # ---- (ii) SlotStream.step and (iii) SlotStream.step_async two deep: the same service ----
    for name in ("step", "step_async"):
        rng = np.random.default_rng(3)
        st = SlotStream(engine(), W, pcm=True, owns_engine=True)
        for _ in range(load):
            st.submit(window_of(rng, True)[0])

        def resubmit():
            for _ in st.finished():
                st.submit(window_of(rng, False)[0])

        rounds = []
        if name == "step":
            for r in range(args.rounds + 1):
                n = warm if r == 0 else steps
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    out = st.step(chunk)
                    resubmit()
                torch.cuda.synchronize()
                if r:
                    rounds.append(1e3 * (time.perf_counter() - t0) / n)
        else:
            pending = st.step_async(chunk)
            for r in range(args.rounds + 1):
                n = warm if r == 0 else steps
                t0 = time.perf_counter()
                for _ in range(n):
                    nxt = st.step_async(chunk)
                    out = pending.result()
                    int(out.samples[:1].sum())      # (the consumer touches what arrived)
                    resubmit()
                    pending = nxt
                if r:
                    rounds.append(1e3 * (time.perf_counter() - t0) / n)
            pending.result()
        res[name + "_wall_ms_per_step"] = _stats(rounds)
        st.close()
        torch.cuda.empty_cache()
    eng_ms = res["engine_ms_per_step"]["median"]
    res["step_vs_engine"] = round(res["step_wall_ms_per_step"]["median"] / eng_ms, 4)
    res["step_async_vs_engine"] = round(res["step_async_wall_ms_per_step"]["median"] / eng_ms, 4)
    res["step_async_kHz_per_utterance"] = round(chunk / res["step_async_wall_ms_per_step"]["median"], 2)
    res["engine_kHz_per_utterance"] = round(chunk / eng_ms, 2)
    return res


def time_compact(args, w, Wc, bc):
    """The --compact measurement (module docstring)."""
    import torch
    import bench
    from nv_wavenet_amd._lib import lib
    B, W = args.batch, args.window
    T_SRC = 262144      # (longer than everything the rounds generate: a resume needs done < length)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    src = torch.randn(bench.N_COND, T_SRC, device="cuda", generator=g).half()
    e = bench.build_engine(w, B, W)
    e.setConditioningWeights(Wc, bc)
    e.setSelectorSeed(5)
    e.slotsBegin(W)
    surv = [b for b in range(B) if b % 16 == 5]
    n = len(surv)
    bound = 16 * ((n + 15) // 16)
    for b in range(B):
        e.slotStart(b, src, b)
    y = torch.empty(B, 2048, dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(count, steps, before=None):
        """ms per step of `steps` steps of `count` samples; before(): host calls that the first step applies (inside the timing)."""
        torch.cuda.synchronize()
        if before:
            before()
        ev[0].record()
        for _ in range(steps):
            assert e.slotsStep(count, y)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps

    timed(256, 1)
    for b in range(B):
        if b % 16 != 5:
            e.slotStop(b)
    timed(256, 1)
    # SlotStream.compact()'s rule: the survivors at or beyond the bound, highest first, into the free columns below it, lowest first
    sources = sorted((b for b in surv if b >= bound), reverse=True)
    targets = [b for b in range(bound) if b % 16 != 5][:len(sources)]
    pairs = list(zip(sources, targets))

    def info(top):
        s = e.kernelInfo(top + 1)
        return {"tiles": (top + 16) // 16, "workgroups": int(s.split("wgs=")[1].split()[0]), "tiles_per_wg": int(s.split("tiles/wg=")[1].split()[0])}

    res = {"batch": B, "window": W, "running": n, "moves": len(pairs), "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "launch_scattered": info(max(surv)), "launch_compacted": info(bound - 1)}
    keys = ("scattered_2048", "scattered_256", "compacted_2048", "compacted_256", "plain_1_scattered", "plain_1_compacted",
            "move_step_1", "move_back_step_1")
    t = {k: [] for k in keys}
    for _ in range(args.rounds):
        timed(2048, 1)
        t["scattered_2048"].append(timed(2048, 2))
        t["scattered_256"].append(timed(256, 4))
        t["plain_1_scattered"].append(timed(1, 8))
        t["move_step_1"].append(timed(1, 1, lambda: [e.slotMove(a, b) for a, b in pairs]))
        t["plain_1_compacted"].append(timed(1, 8))
        timed(2048, 1)
        t["compacted_2048"].append(timed(2048, 2))
        t["compacted_256"].append(timed(256, 4))
        t["move_back_step_1"].append(timed(1, 1, lambda: [e.slotMove(b, a) for a, b in pairs]))

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}

    res["ms_per_step"] = {k: stats(v) for k, v in t.items()}
    # the move launch alone: a one-sample step that carries the moves minus the plain one-sample steps of the launch it runs with
    mv = [a - b for a, b in zip(t["move_step_1"], t["plain_1_compacted"])] + [a - b for a, b in zip(t["move_back_step_1"], t["plain_1_scattered"])]
    res["move_launch_ms"] = stats(mv)
    res["move_launch_vs_compacted_256_step"] = round(float(np.median(mv)) / float(np.median(t["compacted_256"])), 4)
    res["speedup_2048"] = round(float(np.median(t["scattered_2048"])) / float(np.median(t["compacted_2048"])), 3)
    res["speedup_256"] = round(float(np.median(t["scattered_256"])) / float(np.median(t["compacted_256"])), 3)
    # ---- saves and loads (compacted: the survivors are in columns 0 .. bound - 1) ----
    for a, b in pairs:
        e.slotMove(a, b)
    timed(1, 1)
    cols = sorted(set(surv) - set(sources)) + targets
    nbytes = e.slotStateBytes()
    payload = nbytes - 64
    blobs = torch.empty(len(cols), nbytes, dtype=torch.uint8, device="cuda")
    s0 = torch.cuda.current_stream().cuda_stream

    def save(which):
        torch.cuda.synchronize()
        ev[0].record()
        for i in which:
            assert lib.nvw_slot_save(e._h, cols[i], blobs[i].data_ptr(), s0) >= 0
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    save(range(len(cols)))
    one = [save([i]) for i in range(args.rounds)]
    bulk = [save(range(len(cols))) for _ in range(args.rounds)]
    plain = [timed(1, 8) for _ in range(args.rounds)]

    def resume(which):
        for i in which:
            e.slotResume(cols[i], blobs[i], src)

    load_one, load_bulk = [], []
    for r in range(args.rounds):
        save(range(len(cols)))
        e.slotStop(cols[r])
        timed(1, 1)
        load_one.append(timed(1, 1, lambda: resume([r])) - float(np.median(plain)))
        save(range(len(cols)))
        for c in cols:
            e.slotStop(c)
        timed(1, 1)
        load_bulk.append(timed(1, 1, lambda: resume(range(len(cols)))) - float(np.median(plain)))

    def gbs(ms, columns, lines=False):
        per = payload * (1 + (8 if lines else 1))
        return round(columns * per / (ms * 1e-3) / 1e9, 1) if ms > 0 else None

    res["state_bytes"] = nbytes
    res["save_ms"] = {"one_column": stats(one), "bulk_%d_columns" % len(cols): stats(bulk),
                      "bulk_GBps_blob_bytes": gbs(float(np.median(bulk)), len(cols)), "bulk_GBps_lines_touched": gbs(float(np.median(bulk)), len(cols), True),
                      "one_GBps_blob_bytes": gbs(float(np.median(one)), 1)}
    res["load_ms"] = {"one_column_step_difference": stats(load_one), "bulk_%d_columns_step_difference" % len(cols): stats(load_bulk),
                      "bulk_GBps_blob_bytes": gbs(float(np.median(load_bulk)), len(cols)),
                      "bulk_GBps_lines_touched": gbs(float(np.median(load_bulk)), len(cols), True),
                      "note": "differences of two one-sample steps: the one-column figure lies within their spread"}
    res["plain_1_step_ms_for_loads"] = stats(plain)
    e.slotsEnd()
    e.close()
    return res


def time_drain(args, w, Wc, bc):
    """The --drain measurement (module docstring)."""
    import torch
    import bench
    from nv_wavenet_amd._lib import lib
    B, W = args.batch, args.window
    T_SRC = 65536
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    src = torch.randn(bench.N_COND, T_SRC, device="cuda", generator=g).half()
    e = bench.build_engine(w, B, W)
    e.setConditioningWeights(Wc, bc)
    e.setSelectorSeed(5)
    e.slotsBegin(W)
    for b in range(B):
        e.slotStart(b, src, b)
    y = torch.empty(B, 256, dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(count, steps, before=None):
        """(ms per step of `steps` steps of `count` samples, host ms of before()); before(): host calls the first step applies."""
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        if before:
            before()
        host = 1e3 * (time.perf_counter() - h0)
        ev[0].record()
        for _ in range(steps):
            assert e.slotsStep(count, y)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps, host

    timed(256, 1)
    surv = [b for b in range(B) if b % 16 == 5]
    for b in range(B):
        if b % 16 != 5:
            e.slotStop(b)
    timed(256, 1)
    n = len(surv)
    bound = 16 * ((n + 15) // 16)
    sources = sorted((b for b in surv if b >= bound), reverse=True)
    targets = [b for b in range(bound) if b % 16 != 5][:len(sources)]
    for a, b in zip(sources, targets):
        e.slotMove(a, b)
    timed(1, 1)
    cols = sorted(set(surv) - set(sources)) + targets
    nbytes = e.slotStateBytes()
    dev = torch.empty(n, nbytes, dtype=torch.uint8, device="cuda")
    pin = torch.empty(n, nbytes, dtype=torch.uint8, pin_memory=True)
    one = torch.empty(n, nbytes, dtype=torch.uint8, device="cuda")
    s0 = torch.cuda.current_stream().cuda_stream

    def save(how):
        """(device ms, host ms) of saving all the columns one way."""
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        ev[0].record()
        if how == "single":
            for i in range(n):
                assert lib.nvw_slot_save(e._h, cols[i], one[i].data_ptr(), s0) >= 0
        else:
            e.slotsSaveList(cols, stream=s0, out=dev if how == "list_device" else pin)
        ev[1].record()
        host = 1e3 * (time.perf_counter() - h0)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), host

    def resume(how):
        if how == "single":
            for i in range(n):
                e.slotResume(cols[i], one[i], src)
        else:
            e.slotsResumeList(cols, dev if how == "list_device" else pin, [src] * n)

    ways = ("list_device", "list_pinned", "single")
    for how in ways:
        save(how)      # (warm-up: the first launch of a kernel, the staging buffers)
    assert torch.equal(dev, one) and torch.equal(pin.cuda(), one), "the three ways must write the same bytes"
    sv = {how: [] for how in ways}
    sv_host = {how: [] for how in ways}
    ld = {how: [] for how in ways}
    ld_host = {how: [] for how in ways}
    plain = []
    for _ in range(args.rounds):
        for how in ways:
            ms, host = save(how)
            sv[how].append(ms)
            sv_host[how].append(host)
        plain.append(timed(1, 8)[0])
        for how in ways:
            save(how)
            for c in cols:
                e.slotStop(c)
            timed(1, 1)
            ms, host = timed(1, 1, lambda: resume(how))
            ld[how].append(ms - plain[-1])
            ld_host[how].append(host)

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}

    def gbs(ms):
        return round(n * 2 * (nbytes - 64) / (ms * 1e-3) / 1e9, 1) if ms > 0 else None

    res = {"batch": B, "window": W, "columns": n, "rounds": args.rounds, "state_bytes": nbytes, "device": torch.cuda.get_device_name(0),
           "save_ms": {how: stats(sv[how]) for how in ways}, "save_host_ms": {how: stats(sv_host[how]) for how in ways},
           "save_GBps_blob_bytes": {how: gbs(float(np.median(sv[how]))) for how in ways},
           "load_step_difference_ms": {how: stats(ld[how]) for how in ways},
           "load_GBps_blob_bytes": {how: gbs(float(np.median(ld[how]))) for how in ways},
           "resume_calls_host_ms": {how: stats(ld_host[how]) for how in ways}, "plain_1_step_ms": stats(plain)}
    a, b = sv["single"], sv["list_device"]
    gain = float(np.median(a)) - float(np.median(b))
    spread = max(max(a) - min(a), max(b) - min(b))
    res["claim_list_save_faster_than_single_saves_beyond_spread"] = {
        "median_gain_ms": round(gain, 4), "largest_min_max_spread_ms": round(spread, 4), "speedup": round(float(np.median(a)) / float(np.median(b)), 2),
        "holds": bool(gain > spread and max(b) < min(a))}
    e.slotsEnd()
    e.close()
    return res


if __name__ == "__main__":
    main()
