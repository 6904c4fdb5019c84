"""CPU tests of slot mode's denoised delivery at the caller's rate (no GPU): the composed count against a brute-force
enumeration of the two definitions, the three entries declared, bound and exported, and the new object's kernels free of scratch
and spills."""
import os
import re
import subprocess

import numpy as np
import pytest

from nv_wavenet_amd.slots import SlotState, denoise_rate_delivered
from test_code_objects_cpu import BUILD, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nvw_slots_set_denoise_rate", "nvw_slots_denoise_rate_capacity", "nvw_slots_step_ragged_denoise_rate")


@pytest.mark.parametrize("L, M, c", [(2, 1, 9), (1, 3, 13), (147, 80, 588), (3, 2, 0)])
@pytest.mark.parametrize("n_fft, hop", [(64, 16), (64, 8), (32, 4)])
def test_the_composed_count_against_the_enumerated_definitions(n_fft, hop, L, M, c):
    half, K = n_fft // 2, 3 * n_fft + hop + 3
    frames = range(K // hop + 2)
    top = lambda f: max(f * hop + half - 1, half if f == 0 else 0)      # the highest sample frame f reads (frame 0: by reflection)
    for k in range(K + 1):
        # a cleaned sample is ready when every frame that covers it is complete; an output when all its inputs are ready samples
        clean = lambda t: all(top(f) < k for f in frames if f * hop <= t + half < f * hop + n_fft)
        ready = next(t for t in range(K + 1) if not clean(t))
        inputs = lambda m: [i for i in range(-(-(m * M - c) // L), (m * M + c) // L + 1) if i >= 0]
        out = next(m for m in range((K + 2) * L // M + 3) if any(i >= ready for i in inputs(m)))
        assert denoise_rate_delivered(k, n_fft, hop, L, M, c) == out, (k, ready)


def test_a_state_carries_its_tail_and_its_denoise_state_through_bytes():
    src, tail, state = object(), np.array([3, -4, 5], dtype=np.int16), np.arange(37, dtype=np.uint8)
    both = SlotState.from_bytes(SlotState(None, src, 9, 0, "features", tail=tail, denoise=state).to_bytes(), src)
    assert np.array_equal(both.tail, tail) and np.array_equal(both.denoise, state) and both.uid == 9
    with pytest.raises(ValueError):
        SlotState.from_bytes(SlotState(None, src, 9, 0, "features", tail=tail, denoise=state).to_bytes()[:-2], src)


def test_the_entries_are_declared_bound_and_exported():
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import WavenetEngine
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    so = os.path.join(ROOT, "nv_wavenet_amd", "libwavenet_infer.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout if os.path.exists(so) else None
    for name in NAMES:
        assert re.search(r"\b%s\(nvw_engine\* e" % name, header) and name in _lib.SIGNATURES, name
        assert exported is None or re.search(r" T %s$" % name, exported, re.M), name
    assert _lib.SIGNATURES["nvw_slots_step_ragged_denoise_rate"] == _lib.SIGNATURES["nvw_slots_step_ragged_rate"]
    for name in ("slotsSetDenoiseRate", "slotsDenoiseRateCapacity", "slotsStepRaggedDenoiseRate"):
        assert callable(getattr(WavenetEngine, name)), name


def test_the_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "slots_deliver_denoise_rate.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table(obj) if "slot_deliver_denoise_rate_kernel" in r[0]]
    assert len(rows) == 72, len(rows)      # nine variants of the front half x eight of the rate GEMM
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr + agpr <= 512 and sgpr <= 106, (name, vgpr, agpr, sgpr, scratch, spill)
