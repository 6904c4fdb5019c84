"""WavenetEngine: the nvWavenetInfer<T_weight,T_data,R,S,A> class surface
(/root/reference/nv_wavenet.cuh:220-640) reached through the C ABI (include/nv_wavenet_c.h).

Method names, argument order, defaults and layouts are the reference's; arrays may be numpy
(host) or torch (host or device) -- the engine copies them, like the reference does.
"""
import ctypes as C

import numpy as np

from ._lib import lib, addr, CONSUME_FN

# nvw_slot_piece of include/nv_wavenet_c.h: one delivered piece of a ragged slot step
SLOT_PIECE = np.dtype([("slot", "<i4"), ("uid", "<u4"), ("first", "<i8"), ("n", "<i4"), ("finished", "<i4"), ("offset", "<i8")])
assert SLOT_PIECE.itemsize == 32
# ... nvw_slot_saved and nvw_slot_resume_req of nvw_slots_save_list / nvw_slots_resume_list
SLOT_SAVED = np.dtype([("slot", "<i4"), ("uid", "<u4"), ("done", "<i4"), ("mel", "<i4")])
SLOT_RESUME_REQ = np.dtype({"names": ["slot", "mel", "src", "precision", "c_stride", "t_stride", "length", "final"],
                            "formats": ["<i4", "<i4", "<u8", "<i4", "<i8", "<i8", "<i4", "<i4"],
                            "offsets": [0, 4, 8, 16, 24, 32, 40, 44], "itemsize": 48})
assert SLOT_SAVED.itemsize == 16
# ... nvw_prefill_req of nvw_prefill_states
PREFILL_REQ = np.dtype({"names": ["y", "n", "x", "precision", "c_stride", "t_stride", "uid", "temperature"],
                        "formats": ["<u8", "<i4", "<u8", "<i4", "<i8", "<i8", "<u4", "<f4"],
                        "offsets": [0, 8, 16, 24, 32, 40, 48, 52], "itemsize": 56})
# ... nvw_score_req of nvw_score_samples
SCORE_REQ = np.dtype({"names": ["y", "n", "x", "precision", "c_stride", "t_stride", "temperature", "logp", "rows"],
                      "formats": ["<u8", "<i4", "<u8", "<i4", "<i8", "<i8", "<f4", "<u8", "<u8"],
                      "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 64], "itemsize": 72})
# ... nvw_upsample_req, nvw_prefill_mel_req and nvw_score_mel_req of the entries that take mel frames
UPSAMPLE_REQ = np.dtype({"names": ["mel", "precision", "c_stride", "f_stride", "frames", "first_sample", "count", "dst"],
                         "formats": ["<u8", "<i4", "<i8", "<i8", "<i4", "<i4", "<i4", "<u8"],
                         "offsets": [0, 8, 16, 24, 32, 36, 40, 48], "itemsize": 56})
PREFILL_MEL_REQ = np.dtype({"names": ["y", "n", "mel", "precision", "c_stride", "f_stride", "frames", "uid", "temperature"],
                            "formats": ["<u8", "<i4", "<u8", "<i4", "<i8", "<i8", "<i4", "<u4", "<f4"],
                            "offsets": [0, 8, 16, 24, 32, 40, 48, 52, 56], "itemsize": 64})
SCORE_MEL_REQ = np.dtype({"names": ["y", "n", "mel", "precision", "c_stride", "f_stride", "frames", "temperature", "logp", "rows"],
                          "formats": ["<u8", "<i4", "<u8", "<i4", "<i8", "<i8", "<i4", "<f4", "<u8", "<u8"],
                          "offsets": [0, 8, 16, 24, 32, 40, 48, 52, 56, 64], "itemsize": 72})
# ... nvw_score_chunk_req and nvw_score_chunk_mel_req of scoring with carried state
SCORE_CHUNK_REQ = np.dtype({"names": ["state", "y", "n", "x", "precision", "c_stride", "t_stride", "uid", "temperature", "logp", "rows",
                                      "state_out"],
                            "formats": ["<u8", "<u8", "<i4", "<u8", "<i4", "<i8", "<i8", "<u4", "<f4", "<u8", "<u8", "<u8"],
                            "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80], "itemsize": 88})
SCORE_CHUNK_MEL_REQ = np.dtype({"names": ["state", "y", "n", "mel", "precision", "c_stride", "f_stride", "frames", "uid", "temperature",
                                          "logp", "rows", "state_out"],
                                "formats": ["<u8", "<u8", "<i4", "<u8", "<i4", "<i8", "<i8", "<i4", "<u4", "<f4", "<u8", "<u8", "<u8"],
                                "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80, 88], "itemsize": 96})


class Impl:
    """nvWavenetInfer::Implementation (nv_wavenet.cuh:223-229). The reference's Python enum
    (pytorch/nv_wavenet.py:53) stops at PERSISTENT; MANYBLOCK is exposed here as well."""
    AUTO = 0
    SINGLE_BLOCK = 1
    DUAL_BLOCK = 2
    PERSISTENT = 3
    MANYBLOCK = 4


class Org:
    """Kernel organisations (nvwOrganisation in nv_wavenet.hpp; last argument of nvw_create_ex)."""
    AUTO = 0        # from the Implementation value and the batch size
    WG = 1          # wn::wavenet_wg, 1, 2 or 3 tiles of 16 utterances per workgroup by batch size
    WG1 = 2
    WG2 = 3
    WG3 = 4         # three tiles per workgroup (fp16, R <= 64; else two)
    CHAIN = 5       # wn::wavenet_chain: multi-CU, weights resident, fewest CUs
    CHAIN1 = 6      # wn::wavenet_chain, one layer per CU
    # (7, 8, 9 were wn::wavenet_bcast and its variants, removed in round 5: refused by nvw_create_ex)
    WG4 = 10        # four tiles per workgroup (round 6: fp16, R <= 64, dump-free launches; else three)
    BY_NAME = {None: 0, "auto": 0, "wg": 1, "wg1": 2, "wg2": 3, "wg3": 4, "chain": 5, "chain1": 6, "wg4": 10}


def supported_configs():
    buf = (C.c_int * 256)()
    n = lib.nvw_list_supported(buf, 64)
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(min(n, 64))]


def _f32(x):
    if hasattr(x, "data_ptr"):
        import torch
        assert x.dtype == torch.float32, "expected float32"
        return x
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x


class WavenetEngine:
    def __init__(self, R, S, A, numLayers, maxDilation, batchSize, numSamples, impl=0, tanhEmbed=True,
                 precision=32, organisation=0):
        if not lib.nvw_supported(R, S, A, precision):
            raise ValueError("no nvWavenetInfer<%s,R=%d,S=%d,A=%d> in this build; have %s" %
                             ("half2,half" if precision == 16 else "float,float", R, S, A, supported_configs()))
        if impl not in (0, 1, 2, 3, 4):
            raise ValueError("implementation must be 0..4")
        self.R, self.S, self.A = R, S, A
        self.numLayers, self.maxDilation = numLayers, maxDilation
        self.maxBatch, self.maxSamples = batchSize, numSamples
        self.precision = precision
        if isinstance(organisation, str) or organisation is None:
            organisation = Org.BY_NAME[organisation]
        if organisation not in set(Org.BY_NAME.values()):
            raise ValueError("organisation must be one of %s" % sorted(set(Org.BY_NAME.values())))
        self._h = lib.nvw_create_ex(R, S, A, precision, numLayers, maxDilation, batchSize, numSamples, impl,
                                    1 if tanhEmbed else 0, organisation)
        if not self._h:
            raise RuntimeError("nvw_create failed: shape not supported in this organisation")
        self._cb_keep = None

    def close(self):
        if getattr(self, "_h", None):
            lib.nvw_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- model ------------------------------------------------------------------------------
    def setEmbeddings(self, embedPrev, embedCur):
        p, c = _f32(embedPrev), _f32(embedCur)
        lib.nvw_set_embeddings(self._h, addr(p), addr(c))

    def setLayerWeights(self, layer, Wprev, Wcur, Bh, Wres, Bres, Wskip, Bskip):
        a = [_f32(x) for x in (Wprev, Wcur, Bh, Wres, Bres, Wskip, Bskip)]
        lib.nvw_set_layer_weights(self._h, layer, *[addr(x) for x in a])

    def setOutWeights(self, Wzs, Bzs, Wza, Bza):
        a = [_f32(x) for x in (Wzs, Bzs, Wza, Bza)]
        lib.nvw_set_out_weights(self._h, *[addr(x) for x in a])

    def setInputs(self, Lh, outputSelectors, numSamples=None):
        """Lh [numSamples][L][maxBatch][2R] fp32, outputSelectors [numSamples][maxBatch] fp32;
        numSamples defaults to the engine's capacity (the reference's setInputs), may be smaller."""
        Lh, sel = _f32(Lh), _f32(outputSelectors)
        ns = self.maxSamples if numSamples is None else int(numSamples)
        assert 0 < ns <= self.maxSamples
        n = ns * self.numLayers * self.maxBatch * 2 * self.R
        assert (Lh.numel() if hasattr(Lh, "numel") else Lh.size) == n, "Lh has the wrong size"
        assert (sel.numel() if hasattr(sel, "numel") else sel.size) == ns * self.maxBatch
        self._cond_keep = None
        lib.nvw_set_inputs_n(self._h, addr(Lh), addr(sel), ns)

    # ---- beyond the reference class (include/nv_wavenet_c.h, "extensions") ---------------------
    def setConditioning(self, Lh, numSamples=None):
        """The conditioning half of setInputs; pair with setSelectorSeed (no selector matrix)."""
        Lh = _f32(Lh)
        ns = self.maxSamples if numSamples is None else int(numSamples)
        assert 0 < ns <= self.maxSamples
        n = ns * self.numLayers * self.maxBatch * 2 * self.R
        assert (Lh.numel() if hasattr(Lh, "numel") else Lh.size) == n, "Lh has the wrong size"
        self._cond_keep = None
        lib.nvw_set_conditioning_n(self._h, addr(Lh), ns)

    def setConditioningDirect(self, Lh, numSamples=None):
        """Device-resident conditioning consumed in place: Lh is a CUDA tensor [numSamples][L][maxBatch][2R], float32 or
        -- fp16 engines -- float16 (the engine's T_data: half the bytes); no packed copy is made and the kernels read it
        directly.  The tensor is kept referenced here until the next conditioning call; do not modify it while runs
        are in flight."""
        import torch
        assert hasattr(Lh, "data_ptr") and Lh.is_cuda and Lh.is_contiguous(), "setConditioningDirect takes contiguous device tensors"
        bits = {torch.float32: 32, torch.float16: 16}.get(Lh.dtype)
        if bits is None or (bits == 16 and self.precision != 16):
            raise TypeError("an fp%d engine cannot read a %s tensor in place" % (self.precision, Lh.dtype))
        ns = self.maxSamples if numSamples is None else int(numSamples)
        assert Lh.numel() == ns * self.numLayers * self.maxBatch * 2 * self.R, "Lh has the wrong size"
        self._cond_keep = Lh
        if not lib.nvw_set_conditioning_direct_t(self._h, addr(Lh), ns, bits):
            raise ValueError("nvw_set_conditioning_direct_t refused a %d-bit tensor of %d samples" % (bits, ns))

    def condTiles(self):
        """Tiles of 16 utterances per (sample, layer) row of the packed conditioning (the batch rounded up to whole workgroups)."""
        return int(lib.nvw_cond_tiles(self._h))

    def setConditioningPacked(self, frags, numSamples=None):
        """Conditioning already in the engine's fragment order: a contiguous CUDA tensor
        [numSamples + 1][L][condTiles()][waves][fragments][64][8 fp16 | 4 fp32] of the engine's T_data with the gate rows
        pre-scaled (nv_wavenet.py: pack_cond_input / get_cond_input(layout="packed") build it); used in place by the packed
        path of the generation kernels -- no copy, no conversion.  Kept referenced here until the next conditioning call."""
        import torch
        assert hasattr(frags, "data_ptr") and frags.is_cuda and frags.is_contiguous(), "setConditioningPacked takes contiguous device tensors"
        want = torch.float16 if self.precision == 16 else torch.float32
        if frags.dtype != want:
            raise TypeError("an fp%d engine reads %s fragments" % (self.precision, want))
        ns = self.maxSamples if numSamples is None else int(numSamples)
        assert 0 < ns <= self.maxSamples
        assert frags.numel() == (ns + 1) * self.numLayers * self.condTiles() * 16 * 2 * self.R, "fragment tensor has the wrong size"
        self._cond_keep = frags
        if not lib.nvw_set_conditioning_packed_n(self._h, addr(frags), ns, frags.numel()):
            raise ValueError("the fragment tensor is too small for %d samples" % ns)

    # ---- conditioning computed in the generation kernel from the upsampled features (include/nv_wavenet_c.h, round 5) ----------
    def setConditioningWeights(self, Wcond, bcond):
        """The model's `cond_layers` 1x1 convolution (pytorch/wavenet.py:73-74): Wcond [2R*L][n_cond] (or [2R*L][n_cond][1], or
        [L][2R][n_cond]), bcond [2R*L]; fp32, numpy or torch, host or device; copied."""
        W, b = _f32(Wcond), _f32(bcond)
        nW = W.numel() if hasattr(W, "numel") else W.size
        nb = b.numel() if hasattr(b, "numel") else b.size
        assert nb == self.numLayers * 2 * self.R and nW % nb == 0, "Wcond / bcond do not match L x 2R"
        self.nCond = nW // nb
        if not lib.nvw_set_conditioning_weights(self._h, addr(W), addr(b), self.nCond):
            raise ValueError("%d feature channels: the kernels are built for 1..%d" % (self.nCond, lib.nvw_max_cond_channels()))

    def featureFragments(self):
        return int(lib.nvw_feature_fragments(self._h))

    @staticmethod
    def _feat_args(x):
        import torch
        assert hasattr(x, "data_ptr") and x.is_cuda and x.dim() == 3, "features: a CUDA tensor [batch][n_cond][samples] (any strides)"
        bits = {torch.float32: 32, torch.float16: 16}.get(x.dtype)
        assert bits, "features must be float32 or float16"
        return bits, x.stride(0), x.stride(1), x.stride(2)

    def setFeatures(self, x, numSamples=None):
        """The upsampled features of the whole utterance: CUDA tensor [maxBatch][n_cond][numSamples] (the model's upsample
        output; any strides, e.g. a channels-last tensor transposed).  Copied into fragment order; resets the history."""
        bits, sb, sc, st = self._feat_args(x)
        ns = x.size(2) if numSamples is None else int(numSamples)
        assert x.size(0) == self.maxBatch and x.size(1) == self.nCond and x.size(2) >= ns
        self._cond_keep = None
        if not lib.nvw_set_features(self._h, x.data_ptr(), bits, sb, sc, st, ns):
            raise ValueError("nvw_set_features refused %s (%d samples)" % (tuple(x.shape), ns))

    def packFeatures(self, x, firstSample, stream=None):
        """Samples [firstSample, firstSample + x.size(2)) of the features, asynchronously on `stream`; history untouched."""
        bits, sb, sc, st = self._feat_args(x)
        assert x.size(0) == self.maxBatch and x.size(1) == self.nCond
        self._cond_keep = None
        if not lib.nvw_pack_features(self._h, x.data_ptr(), bits, sb, sc, st, int(firstSample), x.size(2), stream):
            raise ValueError("nvw_pack_features refused samples [%d, %d)" % (firstSample, firstSample + x.size(2)))

    def setConditioningFeatures(self, frags, numSamples=None):
        """Features already in fragment order: CUDA tensor [numSamples][condTiles()][featureFragments()][64][8 fp16 | 4 fp32] of the
        engine's T_data (nv_wavenet.py:feature_fragments builds it); used in place."""
        import torch
        assert hasattr(frags, "data_ptr") and frags.is_cuda and frags.is_contiguous()
        want = torch.float16 if self.precision == 16 else torch.float32
        assert frags.dtype == want, "an fp%d engine reads %s fragments" % (self.precision, want)
        ns = frags.size(0) if numSamples is None else int(numSamples)
        self._cond_keep = frags
        if not lib.nvw_set_conditioning_features(self._h, addr(frags), ns, frags.numel()):
            raise ValueError("the feature fragment tensor does not fit %d samples" % ns)

    # ---- features in, samples out: the upsampling on the engine's own kernel and the streaming loop ---------------------------
    def setUpsampling(self, upW, upB, stride):
        """The model's `upsample` ConvTranspose1d (pytorch/wavenet.py:70-72): weight [n_cond][n_cond][window], bias [n_cond]."""
        W, b = _f32(upW), _f32(upB)
        window = int(W.shape[2])
        assert tuple(W.shape[:2]) == (self.nCond, self.nCond), "upsample weight must be [n_cond][n_cond][window]"
        if not lib.nvw_set_upsampling(self._h, addr(W), addr(b), window, int(stride)):
            raise ValueError("upsampling window %d / stride %d not supported" % (window, stride))
        self.upStride = int(stride)

    def setMel(self, mel):
        """The utterances' frames before upsampling: CUDA tensor [maxBatch][n_cond][frames], float32 or float16, any strides.  Copied;
        resets the history (the start of an utterance batch)."""
        bits, sb, sc, sf = self._feat_args(mel)
        assert mel.size(0) == self.maxBatch and mel.size(1) == self.nCond
        self._cond_keep = None
        if not lib.nvw_set_mel(self._h, mel.data_ptr(), bits, sb, sc, sf, mel.size(2)):
            raise ValueError("nvw_set_mel refused %s" % (tuple(mel.shape),))
        self.melFrames = mel.size(2)

    def upsampleFeatures(self, firstSample, count, stream=None):
        if not lib.nvw_upsample_features(self._h, int(firstSample), int(count), stream):
            raise ValueError("nvw_upsample_features refused samples [%d, %d)" % (firstSample, firstSample + count))

    def getFeatures(self, firstSample, count):
        """Debug getter: the engine's own feature fragments of samples [firstSample, firstSample + count) as a CUDA tensor
        [count][condTiles()][featureFragments()][4][16][8 | 4]."""
        import torch
        epl = 8 if self.precision == 16 else 4
        out = torch.empty(count, self.condTiles(), self.featureFragments(), 4, 16, epl, device="cuda",
                          dtype=torch.float16 if self.precision == 16 else torch.float32)
        if not lib.nvw_get_features(self._h, out.data_ptr(), int(firstSample), int(count)):
            raise ValueError("nvw_get_features refused samples [%d, %d)" % (firstSample, firstSample + count))
        return out

    def generate_stream(self, num_samples_per_chunk, consume, num_samples, batch_size, yOut=None, stream=None):
        """Features in, samples out: per chunk the upsampling, the generation launch and the copy of the chunk's samples (and PCM);
        consume(yOut, first, count) on this thread for every finished chunk."""
        def _cb(_ptr, init, count, _user):
            if consume is not None:
                consume(yOut, init, count)
        cb = CONSUME_FN(_cb)
        self._cb_keep = cb
        return bool(lib.nvw_generate_stream(self._h, int(num_samples_per_chunk), cb, None, int(num_samples), int(batch_size),
                                            self._yout(yOut, num_samples), stream))

    def setSelectors(self, outputSelectors, numSamples=None):
        """The selector half of setInputs: [numSamples][maxBatch] uniform draws; conditioning and history untouched."""
        sel = _f32(outputSelectors)
        ns = self.maxSamples if numSamples is None else int(numSamples)
        assert (sel.numel() if hasattr(sel, "numel") else sel.size) == ns * self.maxBatch
        lib.nvw_set_selectors(self._h, addr(sel), ns)

    def packConditioning(self, Lh, firstSample, count, stream=None):
        """Conditioning streamed chunk by chunk: Lh [count][L][maxBatch][2R] fp32 ON THE DEVICE holds samples
        firstSample .. firstSample+count-1; packed asynchronously on `stream` (history untouched)."""
        Lh = _f32(Lh)
        assert hasattr(Lh, "data_ptr") and Lh.is_cuda, "packConditioning takes device tensors"
        assert Lh.numel() == count * self.numLayers * self.maxBatch * 2 * self.R
        self._cond_keep = None
        lib.nvw_pack_conditioning(self._h, addr(Lh), int(firstSample), int(count), stream)

    def run_partial_chunk(self, init_sample, count, num_samples, batch_size, stream=None):
        """Samples [init_sample, init_sample+count) of a num_samples-long utterance, asynchronously on `stream`."""
        return bool(lib.nvw_run_range(self._h, int(init_sample), int(count), int(num_samples), int(batch_size), stream))

    def resetHistory(self, stream=None):
        lib.nvw_reset_history(self._h, stream)

    def chainStatus(self):
        """0, or the code of a multi-CU launch that gave up and could not be re-run (synchronises)."""
        return int(lib.nvw_chain_status(self._h))

    def chainFallbacks(self):
        """Multi-CU launches that gave up (not all workgroups resident in time) and were re-run on wavenet_wg."""
        return int(lib.nvw_chain_fallbacks(self._h))

    def chainLastTimeout(self):
        return int(lib.nvw_chain_last_timeout(self._h))

    def setChainTimeoutMs(self, ms):
        lib.nvw_set_chain_timeout_ms(self._h, float(ms))

    def setRingInLds(self, mode=0):
        """The dilation ring on chip: mode >= 0 (default) = single-workgroup launches keep the ring slots of as many short-dilation layers
        as fit in LDS; -1 = never.  Same samples either way."""
        lib.nvw_set_ring_in_lds(self._h, int(mode))

    def setCompiledSchedule(self, mode=0):
        """The dilation schedule compiled into the kernel: mode >= 0 (default) = eligible launches (three tiles, fp16, packed conditioning,
        maxDilation 512, whole cycles of ten layers, ring slots in LDS) run it, kernelInfo then ends in `sched=cycle10`; -1 = never.  Same
        samples either way."""
        lib.nvw_set_compiled_schedule(self._h, int(mode))

    def setClockProbe(self, on=True):
        """Measurement aid: workgroup 0 of every wavenet_wg launch that follows records shader and wall clock counters."""
        lib.nvw_set_clock_probe(self._h, 1 if on else 0)

    def lastLaunchClockGHz(self):
        """Shader clock the latest probed launch actually ran at (GHz; 0.0 if none was probed); synchronises."""
        return float(lib.nvw_last_launch_clock_ghz(self._h))

    def kernelInfo(self, batch_size=None, dumpActivations=False):
        """The device code run(n, batch_size, ..., dumpActivations) launches (kernel + template arguments)."""
        import ctypes
        buf = ctypes.create_string_buffer(256)
        lib.nvw_kernel_info(self._h, self.maxBatch if batch_size is None else batch_size, 1 if dumpActivations else 0,
                            buf, 256)
        return buf.value.decode()

    def setSelectorSeed(self, seed):
        """Selectors are drawn in-kernel (Philox4x32-10, counter {sample, utterance, 0, 0}, key=seed)."""
        lib.nvw_set_selector_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF)

    def setAudioOut(self, pcmOut):
        """pcmOut: int16 [batch][num_samples] of the run calls that follow (numpy or CUDA tensor) filled wherever yOut is with
        int16(32768 * mu_law_decode(y, A)); None switches it off."""
        if pcmOut is not None:
            if hasattr(pcmOut, "data_ptr"):
                import torch
                assert pcmOut.dtype == torch.int16
            else:
                assert pcmOut.dtype == np.int16 and pcmOut.flags["C_CONTIGUOUS"]
            n = pcmOut.numel() if hasattr(pcmOut, "numel") else pcmOut.size
            self._pcm_keep = pcmOut
            lib.nvw_set_audio_out_n(self._h, addr(pcmOut), n)   # every run call checks batch * num_samples <= n
        else:
            self._pcm_keep = None
            lib.nvw_set_audio_out(self._h, None)

    # ---- slot mode: continuous batching (include/nv_wavenet_c.h, ABI 7; nv_wavenet_amd/slots.py schedules requests onto it) -----
    def slotsBegin(self, window):
        """Enters slot mode with a window of `window` samples (a multiple of the largest dilation); every column idle.  Needs
        setConditioningWeights; the selectors are drawn from the seed of setSelectorSeed."""
        if not lib.nvw_slots_begin(self._h, int(window)):
            raise ValueError("nvw_slots_begin refused window %d (conditioning weights first; a multiple of the largest dilation)" % window)
        self.slotWindow = int(window)
        self._slot_keep = {}

    def slotStart(self, slot, x, uid, length=None):
        """Column `slot` takes a new utterance at the next step: x = its upsampled features, CUDA tensor [n_cond][T] (float32 or
        float16, any strides), the first `length` (default T) samples; uid = the Philox counter word of its selectors."""
        import torch
        assert hasattr(x, "data_ptr") and x.is_cuda and x.dim() == 2, "features: a CUDA tensor [n_cond][samples]"
        bits = {torch.float32: 32, torch.float16: 16}.get(x.dtype)
        assert bits, "features must be float32 or float16"
        n = x.size(1) if length is None else int(length)
        assert x.size(0) == self.nCond and 0 < n <= x.size(1), "features [%d][>= %d] expected, got %s" % (self.nCond, n, tuple(x.shape))
        if not lib.nvw_slot_start(self._h, int(slot), x.data_ptr(), bits, x.stride(0), x.stride(1), n, int(uid) & 0xFFFFFFFF):
            raise ValueError("nvw_slot_start refused slot %d" % slot)
        self._slot_keep[int(slot)] = x      # (read by the steps while the column runs; let go when the column starts again)

    def slotStop(self, slot):
        """Column `slot` goes idle at the next step."""
        if not lib.nvw_slot_stop(self._h, int(slot)):
            raise ValueError("nvw_slot_stop refused slot %d" % slot)

    def slotsStep(self, count, yOut=None, pcm=None, stream=None):
        """`count` samples of every column: yOut int32 / pcm int16 [maxBatch][count] (numpy or CUDA tensors; None: not copied)."""
        for a, name in ((yOut, "yOut"), (pcm, "pcm")):
            if a is not None:
                n = a.numel() if hasattr(a, "numel") else a.size
                assert n >= self.maxBatch * count, "%s must hold [maxBatch][count]" % name
        if yOut is not None:
            self._yout(yOut, count)
        if pcm is not None and not hasattr(pcm, "data_ptr"):
            assert pcm.dtype == np.int16 and pcm.flags["C_CONTIGUOUS"]
        return bool(lib.nvw_slots_step(self._h, int(count), addr(yOut), addr(pcm), stream))

    def slotsStepRagged(self, count, samples=None, pcm=None, stream=None):
        """`count` samples of every column, delivered piece by piece, without ever waiting (nvw_slots_step_ragged): samples int32 /
        pcm int16, 1-D CUDA or pinned tensors (slotsPinned; either may be None), take each running utterance's valid samples
        contiguously at an offset that is a multiple of 8.  Returns (total, pieces, ticket): the ragged size in elements, a numpy
        structured array (SLOT_PIECE: slot, uid, first, n, finished, offset) with one record per delivering column in ascending
        column order -- known at once, from the host's bookkeeping --, and the ticket for slotsWait / slotsDone, after which the
        outputs hold the step.  ValueError when refused (nothing changed)."""
        cap = None
        for a, dt, name in ((samples, "int32", "samples"), (pcm, "int16", "pcm")):
            if a is not None:
                assert hasattr(a, "data_ptr") and (a.is_cuda or a.is_pinned()) and a.is_contiguous() and str(a.dtype) == "torch." + dt, \
                    "%s: a contiguous CUDA or pinned %s tensor" % (name, dt)
                cap = a.numel() if cap is None else min(cap, a.numel())
        pieces = np.empty(self.maxBatch, dtype=SLOT_PIECE)
        n, ticket = C.c_int(0), C.c_ulonglong(0)
        total = lib.nvw_slots_step_ragged(self._h, int(count), addr(samples), addr(pcm), cap or 0, pieces.ctypes.data, self.maxBatch,
                                          C.byref(n), C.byref(ticket), stream)
        if total == -2:
            raise RuntimeError("nvw_slots_step_ragged: a launch of the step of %d samples failed" % count)
        if total < 0:
            raise ValueError("nvw_slots_step_ragged refused a step of %d samples into %s elements" % (count, cap))
        return int(total), pieces[:n.value], int(ticket.value)

    def slotsWait(self, ticket):
        """Blocks until the outputs of the ragged step with that ticket are complete."""
        if not lib.nvw_slots_wait(self._h, int(ticket)):
            raise ValueError("nvw_slots_wait: no ticket %d" % ticket)

    def slotsDone(self, ticket):
        """Whether the outputs of the ragged step with that ticket are complete (never blocks)."""
        return bool(lib.nvw_slots_done(self._h, int(ticket)))

    def slotsPinned(self, elems, pcm=True):
        """(samples, pcm) pinned host tensors of `elems` int32 / int16 for slotsStepRagged (pcm None when not wanted)."""
        import torch
        return (torch.empty(int(elems), dtype=torch.int32, pin_memory=True),
                torch.empty(int(elems), dtype=torch.int16, pin_memory=True) if pcm else None)

    def slotStartMel(self, slot, mel, uid, frames=None, final=True):
        """Column `slot` takes a mel utterance at the next step: mel = its frames before upsampling, CUDA tensor [n_cond][capacity]
        (float32 or float16, any strides), of which the first `frames` (default: all) are written; final: no more will come (its
        length is frames x stride).  More frames go into the same tensor, announced with slotMelFrames.  Needs setUpsampling."""
        import torch
        assert hasattr(mel, "data_ptr") and mel.is_cuda and mel.dim() == 2, "mel: a CUDA tensor [n_cond][frames]"
        bits = {torch.float32: 32, torch.float16: 16}.get(mel.dtype)
        assert bits, "mel must be float32 or float16"
        n = mel.size(1) if frames is None else int(frames)
        assert mel.size(0) == self.nCond and 0 <= n <= mel.size(1), "mel [%d][>= %d] expected, got %s" % (self.nCond, n, tuple(mel.shape))
        if not lib.nvw_slot_start_mel(self._h, int(slot), mel.data_ptr(), bits, mel.stride(0), mel.stride(1), n, 1 if final else 0,
                                      int(uid) & 0xFFFFFFFF):
            raise ValueError("nvw_slot_start_mel refused slot %d" % slot)
        self._slot_keep[int(slot)] = mel      # (read by the steps while the column runs; let go when the column starts again)

    def slotMelFrames(self, slot, frames, final=False):
        """The first `frames` frames of column `slot`'s mel tensor are written (ordered before the next step); final: no more."""
        if not lib.nvw_slot_mel_frames(self._h, int(slot), int(frames), 1 if final else 0):
            raise ValueError("nvw_slot_mel_frames refused slot %d, %d frames" % (slot, frames))

    def slotsHeadroom(self):
        """The largest count the next slotsStep accepts (the window unless a running mel column is short of frames)."""
        return int(lib.nvw_slots_headroom(self._h))

    def slotsGetFeatures(self, first, count):
        """Debug getter: the window's feature fragments of engine samples [first, first + count) (within the last window generated)
        as a CUDA tensor [count][condTiles()][featureFragments()][4][16][8 | 4], the layout of getFeatures."""
        import torch
        epl = 8 if self.precision == 16 else 4
        out = torch.empty(count, self.condTiles(), self.featureFragments(), 4, 16, epl, device="cuda",
                          dtype=torch.float16 if self.precision == 16 else torch.float32)
        if not lib.nvw_slots_get_features(self._h, out.data_ptr(), int(first), int(count)):
            raise ValueError("nvw_slots_get_features refused samples [%d, %d)" % (first, first + count))
        return out

    # ---- ... a column's state as a value: moved, saved, resumed ----
    def slotStateBytes(self):
        """Bytes of one column's state blob for this engine's shape and precision."""
        return int(lib.nvw_slot_state_bytes(self._h))

    def slotMove(self, src, dst):
        """The utterance of column `src` goes on in the idle column `dst` from the next step (which applies its moves first)."""
        if not lib.nvw_slot_move(self._h, int(src), int(dst)):
            raise ValueError("nvw_slot_move refused %d -> %d" % (src, dst))
        self._slot_keep[int(dst)] = self._slot_keep.pop(int(src), None)      # (the steps now read the tensor for column dst)

    def slotSave(self, slot, stream=None):
        """The state of column `slot` after the steps issued so far: (CUDA uint8 tensor of slotStateBytes(), done = its local samples
        generated).  Asynchronous on `stream` (the stream of the steps); the column goes on running."""
        import torch
        blob = torch.empty(self.slotStateBytes(), dtype=torch.uint8, device="cuda")
        done = lib.nvw_slot_save(self._h, int(slot), blob.data_ptr(), stream)
        if done < 0:
            raise ValueError("nvw_slot_save refused slot %d" % slot)
        return blob, int(done)

    def slotResume(self, slot, state, x, length=None):
        """slotStart, continuing from `state` (a blob of slotSave of an engine with the same model and seed): x = the whole
        utterance's features as at its start; uid and done come from the blob.  Reads the blob's header on the null stream (a save
        on a non-blocking stream must have been ordered before this call); the blob
        is kept until the column starts again."""
        import torch
        assert hasattr(x, "data_ptr") and x.is_cuda and x.dim() == 2, "features: a CUDA tensor [n_cond][samples]"
        assert state.is_cuda and state.dtype == torch.uint8 and state.is_contiguous(), "state: a CUDA uint8 tensor of slotSave"
        bits = {torch.float32: 32, torch.float16: 16}.get(x.dtype)
        assert bits, "features must be float32 or float16"
        n = x.size(1) if length is None else int(length)
        assert x.size(0) == self.nCond and 0 < n <= x.size(1), "features [%d][>= %d] expected, got %s" % (self.nCond, n, tuple(x.shape))
        if state.numel() != self.slotStateBytes() or not lib.nvw_slot_resume(self._h, int(slot), state.data_ptr(), x.data_ptr(), bits,
                                                                             x.stride(0), x.stride(1), n):
            raise ValueError("nvw_slot_resume refused slot %d" % slot)
        self._slot_keep[int(slot)] = (x, state)

    def slotResumeMel(self, slot, state, mel, frames=None, final=True):
        """slotStartMel, continuing from `state` (see slotResume); mel, frames, final as for slotStartMel."""
        import torch
        assert hasattr(mel, "data_ptr") and mel.is_cuda and mel.dim() == 2, "mel: a CUDA tensor [n_cond][frames]"
        assert state.is_cuda and state.dtype == torch.uint8 and state.is_contiguous(), "state: a CUDA uint8 tensor of slotSave"
        bits = {torch.float32: 32, torch.float16: 16}.get(mel.dtype)
        assert bits, "mel must be float32 or float16"
        n = mel.size(1) if frames is None else int(frames)
        assert mel.size(0) == self.nCond and 0 <= n <= mel.size(1), "mel [%d][>= %d] expected, got %s" % (self.nCond, n, tuple(mel.shape))
        if state.numel() != self.slotStateBytes() or not lib.nvw_slot_resume_mel(self._h, int(slot), state.data_ptr(), mel.data_ptr(), bits,
                                                                                 mel.stride(0), mel.stride(1), n, 1 if final else 0):
            raise ValueError("nvw_slot_resume_mel refused slot %d" % slot)
        self._slot_keep[int(slot)] = (mel, state)

    # ---- ... lists of columns saved and resumed at once, blobs on the GPU or in pinned memory ----
    def slotsSaveList(self, slots, pinned=False, stream=None, out=None):
        """The states of the columns `slots` after the steps issued so far, with one launch: (blobs, saved).  blobs = a uint8 tensor
        [n][stride] on the GPU, or in pinned host memory (pinned=True: the device writes it in place), row i the blob of slots[i]
        (stride = slotStateBytes(), which is a multiple of 16); out = a buffer of that kind the caller keeps -- a drain buffer
        allocated once, a registered range -- to write into instead of a new one ([>= n][stride >= slotStateBytes()], stride a
        multiple of 16).  saved = a numpy structured array (SLOT_SAVED: slot, uid, done, mel), known at once.  Asynchronous on `stream` (the
        stream of the steps): the blobs hold the states once the stream has got there -- torch.cuda.synchronize(), or any later
        blocking call, before the host reads a pinned buffer.  The columns go on running.  ValueError when refused (nothing
        written): see nvw_slots_save_list."""
        import torch
        idx = np.ascontiguousarray(np.asarray(list(slots), dtype=np.int32))
        n = int(idx.size)
        if out is None:
            out = torch.empty((max(n, 1), self.slotStateBytes()), dtype=torch.uint8, device=None if pinned else "cuda", pin_memory=bool(pinned))
        assert out.dtype == torch.uint8 and out.dim() == 2 and out.stride(1) == 1 and out.size(0) >= n and (out.is_cuda or out.is_pinned()), \
            "out: a uint8 CUDA or pinned tensor [>= n][stride]"
        saved = np.zeros(max(n, 1), dtype=SLOT_SAVED)
        got = lib.nvw_slots_save_list(self._h, idx.ctypes.data, n, out.data_ptr(), out.stride(0), saved.ctypes.data, stream)
        if got != n or n == 0:
            raise ValueError("nvw_slots_save_list refused %d slots" % n)
        return out[:n], saved[:n]

    def slotsResumeList(self, slots, blobs, sources, lengths_or_frames=None, finals=None):
        """slotResume / slotResumeMel for many columns at once, all or nothing: column slots[i] continues from row i of `blobs` (a
        uint8 tensor [n][stride] of slotsSaveList, on the GPU or pinned; a pinned one is read in place and its save must have
        completed) with sources[i], its whole features [n_cond][T] -- or its mel frames, where finals[i] is True or False (None: a
        feature column); lengths_or_frames[i] = samples / frames written (None: all of the tensor).  ValueError when any request is
        refused (the session is as before): see nvw_slots_resume_list.  `blobs` and the sources are kept until the columns start
        again."""
        import torch
        slots = [int(c) for c in slots]
        n = len(slots)
        assert blobs.dtype == torch.uint8 and blobs.dim() == 2 and blobs.stride(1) == 1 and blobs.size(0) >= n and \
            (blobs.is_cuda or blobs.is_pinned()), "blobs: a uint8 CUDA or pinned tensor [n][stride]"
        assert len(sources) == n and blobs.size(1) >= self.slotStateBytes()
        reqs = np.zeros(max(n, 1), dtype=SLOT_RESUME_REQ)
        for i, (col, x) in enumerate(zip(slots, sources)):
            assert hasattr(x, "data_ptr") and x.is_cuda and x.dim() == 2 and x.size(0) == self.nCond, "sources: CUDA tensors [n_cond][...]"
            bits = {torch.float32: 32, torch.float16: 16}.get(x.dtype)
            assert bits, "sources must be float32 or float16"
            final = finals[i] if finals is not None else None
            count = lengths_or_frames[i] if lengths_or_frames is not None else None
            count = x.size(1) if count is None else int(count)
            assert 0 <= count <= x.size(1)
            reqs[i] = (col, 0 if final is None else 1, x.data_ptr(), bits, x.stride(0), x.stride(1), count, 1 if final else 0)
        got = lib.nvw_slots_resume_list(self._h, reqs.ctypes.data, n, blobs.data_ptr(), blobs.stride(0))
        if got != n or n == 0:
            raise ValueError("nvw_slots_resume_list refused %d requests" % n)
        for col, x in zip(slots, sources):
            self._slot_keep[col] = (x, blobs)

    def slotsEnd(self):
        lib.nvw_slots_end(self._h)
        self._slot_keep = {}

    # ---- a column's sampling: one helper behind the lockstep setters, one behind the slot setters, one behind the slot getters ----
    def _set_sampling(self, symbol, values, integer=False):
        """values: None (every column off), a scalar of any kind, a 0-d array or tensor (every column), or 1..maxBatch values (the
        columns past them off); integer: whole numbers that fit 32 bits only.  ValueError when refused (nothing changes)."""
        if values is None:
            ok = getattr(lib, symbol)(self._h, None, 0)
        else:
            dtype = np.int32 if integer else np.float32
            a = np.asarray(values, dtype=None if integer else dtype)
            if integer and (a.dtype.kind not in "iu" or np.any(a != a.astype(dtype))):
                raise ValueError("%s refused %r" % (symbol, values))
            t = np.ascontiguousarray(np.full(self.maxBatch, a, dtype=dtype) if a.ndim == 0 else a.astype(dtype).reshape(-1))
            ok = getattr(lib, symbol)(self._h, t.ctypes.data, int(t.size))
        if not ok:
            raise ValueError("%s refused %r" % (symbol, values))

    def _slot_set_sampling(self, symbol, slot, value, name, cast=float):
        if not getattr(lib, symbol)(self._h, int(slot), cast(value)):
            raise ValueError("%s refused slot %d, %s = %r" % (symbol, slot, name, value))

    def _slot_sampling(self, symbol, slot, cast=float):
        return cast(getattr(lib, symbol)(self._h, int(slot)))

    # ---- sampling temperature per utterance (include/nv_wavenet_c.h, "SAMPLING TEMPERATURE") ----
    def setTemperatures(self, T=None):
        """Lockstep: column b of the features-path runs that follow samples from softmax(logits / T[b]).  T: None (every column at
        1), a float (every column), or a sequence of 1..maxBatch floats (the columns past it at 1), each finite and in
        [2^-10, 2^10].  In force until the next call; a call between two chunks takes effect at the next chunk.  While any
        column's T is not 1, runs on packed or in-place conditioning and on chain engines return False.  ValueError when refused
        (nothing changes)."""
        self._set_sampling("nvw_set_temperatures", T)

    def slotSetTemperature(self, slot, T):
        """Slot mode: the utterance of column `slot` samples at temperature T from the next step on (after slotStart / slotResume,
        which put the column back to 1 / to the blob's value).  ValueError when refused (nothing changes)."""
        self._slot_set_sampling("nvw_slot_set_temperature", slot, T, "T")

    def slotTemperature(self, slot):
        """The temperature in force for column `slot` (host state); 0.0 when the column holds no utterance."""
        return self._slot_sampling("nvw_slot_temperature", slot)

    # ---- probability floor (min-p) per utterance (include/nv_wavenet_c.h, "PROBABILITY FLOOR") ----
    def setMinP(self, p=None):
        """Lockstep: column b of the features-path runs that follow draws from its tempered distribution without the bins whose
        probability is below p[b] times that of the most probable bin.  p: None (every column at 0), a float (every column), or a
        sequence of 1..maxBatch floats (the columns past it at 0), each finite and in [0, 0.5].  In force until the next call; a
        call between two chunks takes effect at the next chunk.  While any column's floor is not 0, runs on packed or in-place
        conditioning and on chain engines return False.  ValueError when refused (nothing changes)."""
        self._set_sampling("nvw_set_min_p", p)

    def slotSetMinP(self, slot, p):
        """Slot mode: the utterance of column `slot` draws with floor p from the next step on (after slotStart / slotResume, which
        put the column back to 0 / to the blob's value).  ValueError when refused (nothing changes)."""
        self._slot_set_sampling("nvw_slot_set_min_p", slot, p, "p")

    def slotMinP(self, slot):
        """The floor in force for column `slot` (host state); -1.0 when the column holds no utterance (0 is a valid floor)."""
        return self._slot_sampling("nvw_slot_min_p", slot)

    # ---- tail cuts, top-k and top-p, per utterance (include/nv_wavenet_c.h, "TAIL CUTS") ----
    def setTopK(self, k=None):
        """Lockstep: column b of the features-path runs that follow draws from the k[b] most probable bins of its tempered
        distribution, ties with the k-th included.  k: None (every column off), an int (every column), or a sequence of
        1..maxBatch ints (the columns past it off), each in [0, A]; 0 is off, 1 is greedy decoding.  In force until the next call,
        independent of setTemperatures, setMinP and setTopP; the kept set is the intersection of the cuts and the floor.  While any
        column has a cut, runs on packed or in-place conditioning and on chain engines return False.  ValueError when refused
        (nothing changes)."""
        self._set_sampling("nvw_set_top_k", k, integer=True)

    def setTopP(self, p=None):
        """Lockstep: column b draws from the smallest set of most probable bins of its tempered distribution whose mass reaches
        p[b], ties at its edge included.  p: None (every column off), a float (every column), or a sequence of 1..maxBatch floats
        (the columns past it off), each finite and in (0, 1]; 1 is off.  Everything else as setTopK."""
        self._set_sampling("nvw_set_top_p", p)

    def slotSetTopK(self, slot, k):
        """Slot mode: the utterance of column `slot` draws with top-k = k from the next step on (after slotStart / slotResume, which
        put the column back to off / to the blob's value).  ValueError when refused (nothing changes)."""
        if int(k) != k or not -2**31 <= int(k) < 2**31:
            raise ValueError("nvw_slot_set_top_k refused slot %d, k = %r" % (slot, k))
        self._slot_set_sampling("nvw_slot_set_top_k", slot, k, "k", int)

    def slotSetTopP(self, slot, p):
        """Slot mode: likewise with top-p = p."""
        self._slot_set_sampling("nvw_slot_set_top_p", slot, p, "p")

    def slotTopK(self, slot):
        """Top-k in force for column `slot` (host state); -1 when the column holds no utterance."""
        return self._slot_sampling("nvw_slot_top_k", slot, int)

    def slotTopP(self, slot):
        """Top-p in force for column `slot` (host state); -1.0 when the column holds no utterance."""
        return self._slot_sampling("nvw_slot_top_p", slot)

    def samplerMask(self):
        """What the next features-path launch pays for (host state): bit 0, some column's floor is not 0; bit 1, some column has a
        cut (the threshold search, in every column of the launch).  0: the launches of an engine without floors and cuts."""
        return int(lib.nvw_sampler_mask(self._h))

    # ---- primed generation: forced sample prefixes (include/nv_wavenet_c.h, "PRIMED GENERATION") ----
    def setPrime(self, y=None, lengths=None):
        """Lockstep: column b of the features-path runs that follow starts with the forced samples y[b][:lengths[b]] and draws from
        there on as always.  y: None (no column primed) or a [batch][n] integer array -- numpy (values checked against 0..A-1) or a
        CUDA int32 tensor (values clamped into it by the kernel); lengths: None (n for every column) or `batch` values in 0..n.
        In force until the next call.  While any column is primed, runs on packed or in-place conditioning and chain launches
        return False.  ValueError when refused (nothing changes)."""
        if y is None:
            if not lib.nvw_set_prime(self._h, None, None, 0, 0, 0):
                raise ValueError("nvw_set_prime refused to clear")
            return
        if hasattr(y, "data_ptr"):
            if y.dim() != 2 or str(y.dtype) != "torch.int32" or not y.is_cuda or y.stride(1) != 1:
                raise ValueError("a prime tensor is [batch][n] int32 on the GPU with unit stride along n")
            batch, n, ptr, stride = int(y.size(0)), int(y.size(1)), y.data_ptr(), int(y.stride(0))
        else:
            y = np.ascontiguousarray(np.asarray(y, dtype=np.int32))
            if y.ndim != 2:
                raise ValueError("a prime is [batch][n]")
            batch, n, ptr, stride = y.shape[0], y.shape[1], y.ctypes.data, y.shape[1]
        ln = np.full(batch, n, dtype=np.int32) if lengths is None else np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
        if ln.size != batch:
            raise ValueError("%d prime lengths for %d columns" % (ln.size, batch))
        if n == 0 or not lib.nvw_set_prime(self._h, ptr, ln.ctypes.data, batch, n, stride):
            raise ValueError("nvw_set_prime refused a prime of %d columns x %d samples" % (batch, n))

    def slotPrime(self, slot, y):
        """Slot mode: the utterance whose start or resume is pending on column `slot` starts with the forced samples y (a 1-D int32
        tensor, contiguous; a CPU tensor is uploaded; kept alive here while the column runs; values clamped into 0..A-1).  Order:
        slotStart / slotResume, then slotPrime.  ValueError when refused (nothing changes)."""
        if not hasattr(y, "data_ptr") or y.dim() != 1 or str(y.dtype) != "torch.int32" or not y.is_contiguous():
            raise ValueError("a slot prime is a contiguous 1-D int32 tensor")
        if not y.is_cuda:
            y = y.cuda()
        if not lib.nvw_slot_prime(self._h, int(slot), y.data_ptr(), int(y.numel())):
            raise ValueError("nvw_slot_prime refused slot %d, n = %d" % (slot, y.numel()))
        self._slot_keep[int(slot)] = (self._slot_keep.get(int(slot)), y)      # (beside the source: it moves and goes with it)

    def slotPrimed(self, slot):
        """n of the prime in force on column `slot` (host state; 0 when none, or once its last forced sample has been issued)."""
        return int(lib.nvw_slot_primed(self._h, int(slot)))

    # ---- prefill: a prime's state blob from a time-parallel pass (include/nv_wavenet_c.h, "PREFILL") ----
    def prefillWindow(self):
        """W: the trailing samples of a prime that determine the state behind it; 0 without conditioning weights."""
        return int(lib.nvw_prefill_window(self._h))

    def prefillStates(self, requests, pinned=False, stream=None, out=None):
        """The state blobs behind primes, with one set of layer launches: requests = [(y, x, uid, temperature), ...] with y the
        prime (1-D contiguous int32 CUDA tensor, n >= 1 values) and x the utterance's features (CUDA tensor [n_cond][>= n], float32
        or float16, any strides).  Returns a uint8 tensor [n][stride] on the GPU, or in pinned host memory (pinned=True), or `out`
        (as for slotsSaveList): row i is byte for byte the blob that slotStart(x, uid) + slotSetTemperature + slotPrime(y), steps up
        to local sample len(y) and slotSave produce.  Asynchronous on `stream`; the tensors of `requests` must stay alive until it
        has run.  Works in and outside slot mode.  ValueError when refused (nothing written): see nvw_prefill_states."""
        import torch
        requests = list(requests)
        n = len(requests)
        if out is None:
            out = torch.empty((max(n, 1), self.slotStateBytes()), dtype=torch.uint8, device=None if pinned else "cuda", pin_memory=bool(pinned))
        assert out.dtype == torch.uint8 and out.dim() == 2 and out.stride(1) == 1 and out.size(0) >= n and (out.is_cuda or out.is_pinned()), \
            "out: a uint8 CUDA or pinned tensor [>= n][stride]"
        reqs = np.zeros(max(n, 1), dtype=PREFILL_REQ)
        for i, (y, x, uid, T) in enumerate(requests):
            if not hasattr(y, "data_ptr") or y.dim() != 1 or str(y.dtype) != "torch.int32" or not y.is_contiguous() or not y.is_cuda:
                raise ValueError("a prime is a contiguous 1-D int32 CUDA tensor")
            assert hasattr(x, "data_ptr") and x.is_cuda and x.dim() == 2 and x.size(0) == self.nCond, "features: CUDA tensors [n_cond][samples]"
            bits = {torch.float32: 32, torch.float16: 16}.get(x.dtype)
            assert bits, "features must be float32 or float16"
            if y.numel() > x.size(1):
                raise ValueError("a prime of %d samples against features of %d" % (y.numel(), x.size(1)))
            reqs[i] = (y.data_ptr(), y.numel(), x.data_ptr(), bits, x.stride(0), x.stride(1), int(uid) & 0xFFFFFFFF, float(T))
        got = lib.nvw_prefill_states(self._h, reqs.ctypes.data, n, out.data_ptr(), out.stride(0), stream)
        if got != n or n == 0:
            raise ValueError("nvw_prefill_states refused %d requests" % n)
        return out[:n]

    # ---- scoring: per-sample log-likelihoods from a time-parallel pass (include/nv_wavenet_c.h, "SCORING") ----
    def scoreMaxSamples(self):
        """The largest sum of n, each rounded up to a multiple of 16, that one scoreSamples call accepts; 0 without conditioning weights."""
        return int(lib.nvw_score_max_samples(self._h))

    def scoreSamples(self, requests, rows=False, stream=None):
        """Per-sample log-likelihoods with one set of layer launches: requests = [(y, x, temperature), ...] with y the samples (1-D
        contiguous int32 CUDA tensor, n >= 1 values, clamped into 0 .. A-1) and x the utterance's features (CUDA tensor
        [n_cond][>= n], float32 or float16, any strides).  Returns a list of float32 CUDA tensors [n]: logp[t] = log softmax(Za_t /
        temperature)[y[t]] with Za_t the logits of sample t of a column started from silence and fed y[0 .. t); with rows=True a
        list of pairs (logp, rows [n][A]): the whole log-distribution of every step.  Asynchronous on `stream`; the tensors of
        `requests` must stay alive until it has run.  Works in and outside slot mode, touches no column.  ValueError when refused
        (nothing written, nothing launched): see nvw_score_samples."""
        import torch
        requests = list(requests)
        n = len(requests)
        if not getattr(self, "nCond", 0):
            raise ValueError("scoring needs setConditioningWeights")
        reqs = np.zeros(max(n, 1), dtype=SCORE_REQ)
        out = []
        for i, (y, x, T) in enumerate(requests):
            if not hasattr(y, "data_ptr") or y.dim() != 1 or str(y.dtype) != "torch.int32" or not y.is_contiguous() or not y.is_cuda or y.numel() < 1:
                raise ValueError("samples to score are a contiguous 1-D int32 CUDA tensor of at least one value")
            assert hasattr(x, "data_ptr") and x.is_cuda and x.dim() == 2 and x.size(0) == self.nCond, "features: CUDA tensors [n_cond][samples]"
            bits = {torch.float32: 32, torch.float16: 16}.get(x.dtype)
            assert bits, "features must be float32 or float16"
            if y.numel() > x.size(1):
                raise ValueError("%d samples against features of %d" % (y.numel(), x.size(1)))
            logp = torch.empty(y.numel(), dtype=torch.float32, device="cuda")
            full = torch.empty((y.numel(), self.A), dtype=torch.float32, device="cuda") if rows else None
            reqs[i] = (y.data_ptr(), y.numel(), x.data_ptr(), bits, x.stride(0), x.stride(1), float(T), logp.data_ptr(),
                       full.data_ptr() if rows else 0)
            out.append((logp, full) if rows else logp)
        got = lib.nvw_score_samples(self._h, reqs.ctypes.data, n, stream)
        if got != n or n == 0:
            raise ValueError("nvw_score_samples refused %d requests" % n)
        return out

    # ---- prefill and scoring from mel frames (include/nv_wavenet_c.h, "FROM MEL FRAMES") ----
    def upsampleRowElems(self):
        """Elements of a row of upsampleRequests: 16 * ceil(n_cond / 16); 0 without setUpsampling."""
        return int(lib.nvw_upsample_row_elems(self._h))

    def _mel_args(self, mel, frames=None):
        import torch
        assert hasattr(mel, "data_ptr") and mel.is_cuda and mel.dim() == 2 and mel.size(0) == self.nCond, "mel: a CUDA tensor [n_cond][frames]"
        bits = {torch.float32: 32, torch.float16: 16}.get(mel.dtype)
        assert bits, "mel must be float32 or float16"
        frames = mel.size(1) if frames is None else int(frames)
        assert 0 <= frames <= mel.size(1), "frames: at most the tensor's"
        return bits, mel.stride(0), mel.stride(1), frames

    def upsampleRequests(self, requests, stream=None):
        """Upsampled features by request and sample range, one launch: requests = [(mel, first_sample, count), ...] with mel an
        utterance's frames (CUDA tensor [n_cond][frames], float32 or float16, any strides).  Returns a list of CUDA tensors
        [count][upsampleRowElems()] of the engine's dtype: row t - first_sample holds the features of sample t, bit for bit those of
        setMel + upsampleFeatures, channels >= n_cond zero; rows.t()[:n_cond] is a [n_cond][count] view that prefillStates and
        scoreSamples take as it is.  Asynchronous on `stream`.  ValueError when refused (nothing written): see nvw_upsample_requests."""
        import torch
        requests = list(requests)
        n = len(requests)
        row = self.upsampleRowElems()
        if not row:
            raise ValueError("upsampleRequests needs setUpsampling")
        reqs = np.zeros(max(n, 1), dtype=UPSAMPLE_REQ)
        out = []
        for i, (mel, first, count) in enumerate(requests):
            bits, sc, sf, frames = self._mel_args(mel)
            if int(count) < 1 or int(first) < 0:
                raise ValueError("a range is first_sample >= 0, count >= 1")
            dst = torch.empty((int(count), row), dtype=torch.float16 if self.precision == 16 else torch.float32, device="cuda")
            reqs[i] = (mel.data_ptr(), bits, sc, sf, frames, int(first), int(count), dst.data_ptr())
            out.append(dst)
        got = lib.nvw_upsample_requests(self._h, reqs.ctypes.data, n, stream)
        if got != n or n == 0:
            raise ValueError("nvw_upsample_requests refused %d requests" % n)
        return out

    def prefillStatesMel(self, requests, pinned=False, stream=None, out=None):
        """prefillStates from frames: requests = [(y, mel, uid, temperature[, frames]), ...] with mel the utterance's frames (CUDA
        tensor [n_cond][capacity], float32 or float16, any strides) of which the first `frames` (default: all) are written and
        frames x stride >= len(y).  Row i is byte for byte the blob that slotStartMel(mel, uid) + slotSetTemperature + slotPrime(y),
        steps up to local sample len(y) and slotSave produce.  Otherwise as prefillStates.  ValueError when refused (nothing
        written): see nvw_prefill_states_mel."""
        import torch
        requests = list(requests)
        n = len(requests)
        if out is None:
            out = torch.empty((max(n, 1), self.slotStateBytes()), dtype=torch.uint8, device=None if pinned else "cuda", pin_memory=bool(pinned))
        assert out.dtype == torch.uint8 and out.dim() == 2 and out.stride(1) == 1 and out.size(0) >= n and (out.is_cuda or out.is_pinned()), \
            "out: a uint8 CUDA or pinned tensor [>= n][stride]"
        reqs = np.zeros(max(n, 1), dtype=PREFILL_MEL_REQ)
        for i, rq in enumerate(requests):
            y, mel, uid, T = rq[:4]
            if not hasattr(y, "data_ptr") or y.dim() != 1 or str(y.dtype) != "torch.int32" or not y.is_contiguous() or not y.is_cuda:
                raise ValueError("a prime is a contiguous 1-D int32 CUDA tensor")
            bits, sc, sf, frames = self._mel_args(mel, rq[4] if len(rq) > 4 else None)
            reqs[i] = (y.data_ptr(), y.numel(), mel.data_ptr(), bits, sc, sf, frames, int(uid) & 0xFFFFFFFF, float(T))
        got = lib.nvw_prefill_states_mel(self._h, reqs.ctypes.data, n, out.data_ptr(), out.stride(0), stream)
        if got != n or n == 0:
            raise ValueError("nvw_prefill_states_mel refused %d requests" % n)
        return out[:n]

    def scoreSamplesMel(self, requests, rows=False, stream=None):
        """scoreSamples from frames: requests = [(y, mel, temperature[, frames]), ...], mel as for prefillStatesMel.  Returns what
        scoreSamples returns -- bit for bit what it returns for the upsampled features of those frames.  ValueError when refused
        (nothing written, nothing launched): see nvw_score_samples_mel."""
        import torch
        requests = list(requests)
        n = len(requests)
        if not getattr(self, "nCond", 0):
            raise ValueError("scoring needs setConditioningWeights")
        reqs = np.zeros(max(n, 1), dtype=SCORE_MEL_REQ)
        out = []
        for i, rq in enumerate(requests):
            y, mel, T = rq[:3]
            if not hasattr(y, "data_ptr") or y.dim() != 1 or str(y.dtype) != "torch.int32" or not y.is_contiguous() or not y.is_cuda or y.numel() < 1:
                raise ValueError("samples to score are a contiguous 1-D int32 CUDA tensor of at least one value")
            bits, sc, sf, frames = self._mel_args(mel, rq[3] if len(rq) > 3 else None)
            logp = torch.empty(y.numel(), dtype=torch.float32, device="cuda")
            full = torch.empty((y.numel(), self.A), dtype=torch.float32, device="cuda") if rows else None
            reqs[i] = (y.data_ptr(), y.numel(), mel.data_ptr(), bits, sc, sf, frames, float(T), logp.data_ptr(), full.data_ptr() if rows else 0)
            out.append((logp, full) if rows else logp)
        got = lib.nvw_score_samples_mel(self._h, reqs.ctypes.data, n, stream)
        if got != n or n == 0:
            raise ValueError("nvw_score_samples_mel refused %d requests" % n)
        return out

    # ---- scoring with carried state (include/nv_wavenet_c.h, "SCORING WITH CARRIED STATE") ----
    def _score_chunks(self, requests, mel, rows, states, pinned, stream, out=None):
        import torch
        requests = list(requests)
        n = len(requests)
        if not getattr(self, "nCond", 0):
            raise ValueError("scoring needs setConditioningWeights")
        reqs = np.zeros(max(n, 1), dtype=SCORE_CHUNK_MEL_REQ if mel else SCORE_CHUNK_REQ)
        blobs = out
        if out is not None:
            assert out.dtype == torch.uint8 and out.dim() == 2 and out.stride(1) == 1 and out.size(0) >= n and \
                out.size(1) >= self.slotStateBytes() and (out.is_cuda or out.is_pinned()), "out: a uint8 CUDA or pinned tensor [>= n][stride]"
            states = True
        elif states:
            blobs = torch.empty((max(n, 1), self.slotStateBytes()), dtype=torch.uint8, device=None if pinned else "cuda", pin_memory=bool(pinned))
        out = []
        for i, rq in enumerate(requests):
            state, y, src, uid, T = rq[:5]
            if not hasattr(y, "data_ptr") or y.dim() != 1 or str(y.dtype) != "torch.int32" or not y.is_contiguous() or not y.is_cuda or y.numel() < 1:
                raise ValueError("samples to score are a contiguous 1-D int32 CUDA tensor of at least one value")
            if state is not None and (not hasattr(state, "data_ptr") or state.dtype != torch.uint8 or not state.is_contiguous() or
                                      state.numel() != self.slotStateBytes() or not (state.is_cuda or state.is_pinned())):
                raise ValueError("a state is a contiguous uint8 CUDA or pinned tensor of slotStateBytes()")
            logp = torch.empty(y.numel(), dtype=torch.float32, device="cuda")
            full = torch.empty((y.numel(), self.A), dtype=torch.float32, device="cuda") if rows else None
            tail = (int(uid) & 0xFFFFFFFF, float(T), logp.data_ptr(), full.data_ptr() if rows else 0, blobs[i].data_ptr() if states else 0)
            if mel:
                bits, sc, sf, frames = self._mel_args(src, rq[5] if len(rq) > 5 else None)
                reqs[i] = (state.data_ptr() if state is not None else 0, y.data_ptr(), y.numel(), src.data_ptr(), bits, sc, sf, frames) + tail
            else:
                assert hasattr(src, "data_ptr") and src.is_cuda and src.dim() == 2 and src.size(0) == self.nCond, \
                    "features: CUDA tensors [n_cond][samples]"
                bits = {torch.float32: 32, torch.float16: 16}.get(src.dtype)
                assert bits, "features must be float32 or float16"
                if y.numel() > src.size(1):
                    raise ValueError("%d samples against features of %d" % (y.numel(), src.size(1)))
                reqs[i] = (state.data_ptr() if state is not None else 0, y.data_ptr(), y.numel(), src.data_ptr(), bits, src.stride(0),
                           src.stride(1)) + tail
            out.append((logp, full) if rows else logp)
        name = "nvw_score_chunks_mel" if mel else "nvw_score_chunks"
        got = getattr(lib, name)(self._h, reqs.ctypes.data, n, stream)
        if got != n or n == 0:
            raise ValueError("%s refused %d requests" % (name, n))
        return (out, blobs[:n]) if states else out

    def scoreChunks(self, requests, rows=False, states=False, pinned=False, stream=None, out=None):
        """scoreSamples over time chunks with carried state: requests = [(state, y, x, uid, temperature), ...] with state a uint8
        CUDA or pinned tensor of slotStateBytes() -- a blob of slotSave / slotsSaveList / prefillStates* / this call -- or None (from
        silence at local sample 0), y the chunk's samples = local samples done .. done + n - 1 of the utterance (done: the
        state's), and x the CHUNK's features [n_cond][>= n]: column i belongs to sample done + i.  Returns what scoreSamples
        returns, bit for bit what it gives for these samples in one pass over [0, done + n); with states=True the pair (that,
        blobs): a uint8 tensor [n][slotStateBytes()] on the GPU, or in pinned host memory (pinned=True), row i byte for byte the
        blob of prefillStates for the first done + n samples (uid: the state's, or the request's from silence).  States are read
        only and may be shared by several requests; their headers are read on the null stream before anything is queued (a save
        on a non-blocking stream must have been ordered before this call).  Asynchronous on `stream`; the tensors of `requests`
        must stay alive until it has run.  out: a buffer the caller keeps for the blobs, as for prefillStates (implies states).
        ValueError when refused (nothing written, nothing launched): see nvw_score_chunks."""
        return self._score_chunks(requests, False, rows, states, pinned, stream, out)

    def scoreChunksMel(self, requests, rows=False, states=False, pinned=False, stream=None, out=None):
        """scoreChunks from frames: requests = [(state, y, mel, uid, temperature[, frames]), ...] with mel the utterance's frames
        from frame 0, as scoreSamplesMel takes them; the engine upsamples samples [done, done + n) itself.  Bit for bit what
        scoreSamplesMel returns for these samples; the blobs byte for byte those of prefillStatesMel.  ValueError when refused: see
        nvw_score_chunks_mel."""
        return self._score_chunks(requests, True, rows, states, pinned, stream, out)

    # ---- run --------------------------------------------------------------------------------
    def _yout(self, yOut, need=None):
        if yOut is None:
            return None
        if hasattr(yOut, "data_ptr"):
            import torch
            assert yOut.dtype == torch.int32
        else:
            assert yOut.dtype == np.int32 and yOut.flags["C_CONTIGUOUS"]
        n = yOut.numel() if hasattr(yOut, "numel") else yOut.size
        assert n >= self.maxBatch * (self.maxSamples if need is None else need), "yOut must hold [maxBatch][num_samples] int32"
        return addr(yOut)

    def run(self, num_samples, batch_size, yOut=None, batch_size_per_block=1, dumpActivations=False, stream=None):
        ok = lib.nvw_run(self._h, num_samples, batch_size, self._yout(yOut, num_samples), batch_size_per_block,
                         1 if dumpActivations else 0, stream)
        return bool(ok)

    def run_partial(self, init_sample, num_samples, batch_size, yOut=None, batch_size_per_block=1,
                    dumpActivations=False, stream=None):
        ok = lib.nvw_run_partial(self._h, init_sample, num_samples, batch_size, self._yout(yOut, num_samples),
                                 batch_size_per_block, 1 if dumpActivations else 0, stream)
        return bool(ok)

    def run_chunks(self, num_samples_per_chunk, consume, num_samples, batch_size, yOut=None,
                   batch_size_per_block=1, dumpActivations=False, stream=None):
        """consume(yOut, init_sample, count) is called on this thread for every finished chunk."""
        def _cb(_ptr, init, count, _user):
            if consume is not None:
                consume(yOut, init, count)
        cb = CONSUME_FN(_cb)
        self._cb_keep = cb
        ok = lib.nvw_run_chunks(self._h, num_samples_per_chunk, cb, None, num_samples, batch_size,
                                self._yout(yOut, num_samples), batch_size_per_block, 1 if dumpActivations else 0, stream)
        return bool(ok)

    # ---- getters (host numpy, reference layouts) ----------------------------------------------
    def _get(self, fn, shape, *pre):
        out = np.zeros(shape, dtype=np.float32)
        fn(self._h, *pre, addr(out))
        return out

    def getXtOut(self, layer):
        return self._get(lib.nvw_get_xt_out, (self.maxBatch, self.R), layer)

    def getSkipOut(self, layer):
        return self._get(lib.nvw_get_skip_out, (self.maxBatch, self.S), layer)

    def getZs(self):
        return self._get(lib.nvw_get_zs, (self.maxBatch, self.A))

    def getZa(self):
        return self._get(lib.nvw_get_za, (self.maxBatch, self.A))

    def getP(self):
        return self._get(lib.nvw_get_p, (self.maxBatch, self.A))

    def getYOut(self, yOut, offset, size, stream=None):
        lib.nvw_get_y_out(self._h, self._yout(yOut), offset, size, stream)

    def time_runs(self, reps, num_samples, batch_size, batch_size_per_block=1, stream=None):
        """HIP-event milliseconds for `reps` back-to-back run() launches on `stream`."""
        return float(lib.nvw_time_runs(self._h, reps, num_samples, batch_size, batch_size_per_block, stream))

    @staticmethod
    def synchronize():
        lib.nvw_device_synchronize()
