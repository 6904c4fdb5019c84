"""CPU tests of the time-parallel upsampling pass (no GPU): the new entries are declared, bound and exported; the
kernels of the built object use no scratch memory and spill nothing; and the frame-range rule the kernel gathers by
(mel_time_cases.frames_read) is held to a float64 transposed convolution -- a frame outside the rule changes no sample of the
range, the first and the last frame inside it change one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mel_time_cases as MT
from test_code_objects_cpu import BUILD, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nvw_upsample_row_elems", "nvw_upsample_requests", "nvw_prefill_states_mel", "nvw_score_samples_mel")


def _fields(header, name):
    m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header)
    assert m, name
    return [f.strip() for f in m.group(1).split(";") if f.strip()]


def test_the_mel_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert re.search(r"int nvw_upsample_row_elems\(nvw_engine\* e\);", header)
    assert re.search(r"int nvw_upsample_requests\(nvw_engine\* e, const nvw_upsample_req\* reqs, int count, void\* stream\);", header)
    assert re.search(r"int nvw_prefill_states_mel\(nvw_engine\* e, const nvw_prefill_mel_req\* reqs, int count, void\* dst, long long stride, "
                     r"void\* stream\);", header)
    assert re.search(r"int nvw_score_samples_mel\(nvw_engine\* e, const nvw_score_mel_req\* reqs, int count, void\* stream\);", header)
    assert _fields(header, "nvw_upsample_req") == ["const void* mel", "int precision", "long long c_stride, f_stride", "int frames",
                                                   "int first_sample, count", "void* dst"]
    assert _fields(header, "nvw_prefill_mel_req") == ["const int* y", "int n", "const void* mel", "int precision", "long long c_stride, f_stride",
                                                      "int frames", "unsigned uid", "float temperature"]
    assert _fields(header, "nvw_score_mel_req") == ["const int* y", "int n", "const void* mel", "int precision", "long long c_stride, f_stride",
                                                    "int frames", "float temperature", "float* logp", "float* rows"]
    assert "Mel frames (a prefill that upsamples)" not in header and "Scoring from mel frames, in time chunks" not in header
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import PREFILL_MEL_REQ, SCORE_MEL_REQ, UPSAMPLE_REQ, WavenetEngine
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert UPSAMPLE_REQ.itemsize == 56 and [UPSAMPLE_REQ.fields[k][1] for k in UPSAMPLE_REQ.names] == [0, 8, 16, 24, 32, 36, 40, 48]
    assert PREFILL_MEL_REQ.itemsize == 64 and [PREFILL_MEL_REQ.fields[k][1] for k in PREFILL_MEL_REQ.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56]
    assert SCORE_MEL_REQ.itemsize == 72 and [SCORE_MEL_REQ.fields[k][1] for k in SCORE_MEL_REQ.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 64]
    for name in ("upsampleRowElems", "upsampleRequests", "prefillStatesMel", "scoreSamplesMel"):
        assert callable(getattr(WavenetEngine, name)), name
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    from nv_wavenet_amd.slots import SlotStream
    assert callable(NVWaveNetEngine.score_mel) and callable(SlotStream.prefill_mel) and callable(SlotStream.score_mel)


def test_the_mel_time_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "mel_time.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table("mel_time.o") if "mel_time_upsample_kernel" in r[0]]
    assert len(rows) == 4, [r[0] for r in rows]          # the operand in LDS or from L2, two precisions
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr + agpr <= 512, (name, vgpr, agpr, scratch, spill)
    # ... scalar registers included (kernel_table's last column counts vector registers only): the code object's notes themselves
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_stats
    notes = subprocess.run([isa_stats.LLVM + "llvm-readelf", "--notes", isa_stats.code_object("mel_time.o")], capture_output=True, text=True).stdout
    spills = {}
    for blk in notes.split(".agpr_count:")[1:]:
        name = next((n for n in re.findall(r"\.name:\s*(\S+)", blk) if "mel_time_upsample_kernel" in n), None)      # (arguments have names too)
        if name:
            spills[name] = (int(re.search(r"\.sgpr_spill_count:\s*(\d+)", blk).group(1)),
                                     int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1)))
    assert len(spills) == 4 and all(v == (0, 0) for v in spills.values()), spills


HOPS = [(8, 2), (12, 4), (10, 5), (16, 8), (48, 16), (4, 4)]


def _upsampled(mel, w, b, stride):
    return F.conv_transpose1d(mel[None], w, b, stride=stride)[0, :, :mel.shape[1] * stride]


@pytest.mark.parametrize("hop", HOPS, ids=lambda h: "%d_%d" % h)
def test_the_frame_range_rule_against_a_float64_transposed_convolution(hop):
    """For ranges that cut frames: perturbing any frame outside frames_read(a, b) changes no sample of [a, b) of the float64
    transposed convolution; perturbing the first or the last frame inside it changes one."""
    window, stride = hop
    frames, C = 9, 3
    N = frames * stride
    rng = np.random.RandomState(window * 100 + stride)
    mel = torch.from_numpy(rng.standard_normal((C, frames)))
    w = torch.from_numpy(rng.standard_normal((C, C, window)) + 3.0)          # (no weight is zero: every tap counts)
    b = torch.from_numpy(rng.standard_normal(C))
    base = _upsampled(mel, w, b, stride)
    assert base.shape == (C, N)
    seen_low_clamp = False
    for a, c in MT.ranges(N, stride) + [(N - stride - 1, 3), (2 * stride, stride)]:
        lo, hi = MT.frames_read(a, a + c, window, stride)
        assert 0 <= lo <= hi < frames and hi * stride < a + c <= (hi + 1) * stride
        seen_low_clamp |= a // stride - (window // stride - 1) < 0
        for f in range(frames):
            moved = mel.clone()
            moved[:, f] += 1.0
            changed = bool((_upsampled(moved, w, b, stride)[:, a:a + c] != base[:, a:a + c]).any())
            if f < lo or f > hi:
                assert not changed, "range [%d, %d): frame %d outside [%d, %d] reaches it" % (a, a + c, f, lo, hi)
            elif f in (lo, hi):
                assert changed, "range [%d, %d): frame %d, an end of [%d, %d], does not reach it" % (a, a + c, f, lo, hi)
    assert seen_low_clamp or window == stride          # (with one tap no range reaches before frame 0)
