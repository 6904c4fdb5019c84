"""CPU tests of slot mode's denoised delivery (no GPU): D(k) and the two state lengths against a brute-force
enumeration of the definition of denoise.hpp, the state record's optional denoise state, and the new entries declared, bound and
exported."""
import os

import numpy as np
import pytest
import torch

from nv_wavenet_amd.slots import SlotState, denoise_acc_len, denoise_delivered, denoise_hist_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_fft, hop", [(1024, 256), (800, 200), (64, 16), (64, 8)])
def test_delivered_and_state_lengths_against_the_enumerated_definition(n_fft, hop):
    half, K = n_fft // 2, 3 * n_fft + hop + 3
    # frame f reads samples f hop - half .. f hop + half - 1, frame 0 through the reflection sample `half` as its highest
    top = lambda f: max(f * hop + half - 1, half if f == 0 else 0)
    ready, back = 0, 0
    for k in range(K + 1):
        complete = [f for f in range(K // hop + 2) if top(f) < k]
        assert complete == list(range(len(complete)))                    # a prefix of the frames
        q = len(complete)
        # output t, padded position t + half, is covered by the frames f with f hop <= t + half < f hop + n_fft; the complete frames
        # only grow with k, so the leading outputs that are ready do too
        while all(f in complete for f in range(K // hop + 2) if f * hop <= ready + half < f * hop + n_fft):
            ready += 1
        assert denoise_delivered(k, n_fft, hop) == ready, k
        # the first incomplete frame starts less than hist samples back ...
        back = max(back, k - max(q * hop - half, 0))
        # ... and the complete ones reach acc padded positions beyond the last complete hop, which begins at q hop
        assert q == 0 or max(f * hop + n_fft for f in complete) - q * hop == denoise_acc_len(n_fft, hop), k
    assert denoise_hist_len(n_fft) - hop <= back < denoise_hist_len(n_fft) == n_fft


def test_a_state_carries_its_denoise_state_as_a_trailing_optional_record():
    src = object()
    state = np.arange(37, dtype=np.uint8)
    plain = SlotState(None, src, 9, 0, "features")
    with_state = SlotState(None, src, 9, 0, "features", denoise=state)
    assert with_state.to_bytes() == plain.to_bytes() + SlotState.DENOISE.pack(SlotState.DENOISE_MAGIC, 37) + state.tobytes()
    back = SlotState.from_bytes(with_state.to_bytes(), src)
    assert np.array_equal(back.denoise, state) and back.uid == 9 and back.tail is None
    old = SlotState.from_bytes(plain.to_bytes(), src)                    # a blob without the record reads as before
    assert old.denoise is None and old.tail is None
    tailed = SlotState.from_bytes(SlotState(None, src, 9, 0, "features", tail=np.array([1, -2], dtype=np.int16)).to_bytes(), src)
    assert tailed.tail.tolist() == [1, -2] and tailed.denoise is None
    primed = SlotState(None, src, 9, 0, "features", prime=torch.arange(1, 7, dtype=torch.int32), denoise=state)
    back = SlotState.from_bytes(primed.to_bytes(), src)
    assert np.array_equal(back.denoise, state) and back.prime.tolist() == [1, 2, 3, 4, 5, 6]
    with pytest.raises(ValueError):
        SlotState.from_bytes(with_state.to_bytes()[:-2], src)


def test_the_denoise_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import WavenetEngine
    for name in ("nvw_slots_set_denoise", "nvw_slot_set_denoise_strength", "nvw_slots_denoise_capacity", "nvw_slots_step_ragged_denoise",
                 "nvw_slots_denoise_state_bytes", "nvw_slot_denoise_state_get", "nvw_slot_denoise_state_set"):
        assert " %s(nvw_engine* e" % name in header and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "#define NVW_ABI_VERSION 7" in header
    assert _lib.SIGNATURES["nvw_slots_step_ragged_denoise"] == _lib.SIGNATURES["nvw_slots_step_ragged_rate"]
    for name in ("slotsSetDenoise", "slotSetDenoiseStrength", "slotsDenoiseCapacity", "slotsStepRaggedDenoise", "slotsDenoiseStateBytes",
                 "slotDenoiseStateGet", "slotDenoiseStateSet"):
        assert callable(getattr(WavenetEngine, name)), name
