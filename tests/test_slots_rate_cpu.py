"""CPU tests of slot mode's delivery at the caller's rate (no GPU): the piece arithmetic -- D(k), a piece's m0 and
count, the history H -- against a brute-force enumeration of the definition of resample.hpp, the state record's optional history,
and the new entries declared, bound and exported."""
import os

import numpy as np
import pytest
import torch

from nv_wavenet_amd.slots import SlotState, rate_delivered, rate_piece, rate_tail_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(m, L, M, c):
    """[lo, hi] of the inputs with a tap on output m, by trying every tap k = c + m M - i L in [0, 2 c]"""
    hit = [i for i in range((m * M - c) // L - 2, (m * M + c) // L + 3) if 0 <= c + m * M - i * L <= 2 * c]
    return hit[0], hit[-1]


@pytest.mark.parametrize("L, M", [(2, 1), (1, 3), (2, 3), (147, 80)])
@pytest.mark.parametrize("zeros", [1, 4])
def test_piece_arithmetic_against_the_enumerated_definition(L, M, zeros):
    c = zeros * max(L, M)                                   # the centre of resample_taps' T = 2 zeros max(L, M) + 1 taps
    H, K = rate_tail_len(L, c), 3 * (2 * c // L + 1)        # k up to three filter lengths
    assert H == -(-2 * c // L)
    spans = [_inputs(m, L, M, c) for m in range(K * L // M + 2 * c + 2)]
    assert all(a[1] <= b[1] for a, b in zip(spans, spans[1:]))          # the last input grows with m: D counts a prefix
    brute = [sum(1 for lo, hi in spans if hi < k) for k in range(K + 1)]
    assert [rate_delivered(k, L, M, c) for k in range(K + 1)] == brute
    for f in range(K):
        assert spans[brute[f]][0] >= f - H, (f, spans[brute[f]])       # the first output of a piece reaches back over H at the most
        for n in {1, min(2, K - f), K - f}:
            assert rate_piece(f, n, False, L, M, c) == (brute[f], brute[f + n] - brute[f])
            assert rate_piece(f, n, True, L, M, c) == (brute[f], -(-(f + n) * L // M) - brute[f])


def test_a_state_carries_its_history_as_a_trailing_optional_field():
    src = object()
    tail = np.array([3, -4, 32767, -32768, 0], dtype=np.int16)
    plain = SlotState(None, src, 9, 0, "features")
    with_tail = SlotState(None, src, 9, 0, "features", tail=tail)
    assert with_tail.to_bytes() == plain.to_bytes() + SlotState.TAIL.pack(SlotState.TAIL_MAGIC, 5) + tail.tobytes()
    back = SlotState.from_bytes(with_tail.to_bytes(), src)
    assert np.array_equal(back.tail, tail) and back.uid == 9 and SlotState.from_bytes(plain.to_bytes(), src).tail is None
    primed = SlotState(None, src, 9, 0, "features", prime=torch.arange(1, 7, dtype=torch.int32), tail=tail)
    back = SlotState.from_bytes(primed.to_bytes(), src)
    assert np.array_equal(back.tail, tail) and back.prime.tolist() == [1, 2, 3, 4, 5, 6]
    with pytest.raises(ValueError):
        SlotState.from_bytes(with_tail.to_bytes()[:-2], src)


def test_the_rate_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import SLOT_RATE_PIECE, WavenetEngine
    for name in ("nvw_slots_set_delivery", "nvw_slots_tail_len", "nvw_slots_rate_capacity", "nvw_slots_step_ragged_rate", "nvw_slot_tail_get",
                 "nvw_slot_tail_set"):
        assert " %s(nvw_engine* e" % name in header and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "} nvw_slot_rate_piece;" in header and "#define NVW_ABI_VERSION 7" in header
    assert SLOT_RATE_PIECE.itemsize == 24 and [SLOT_RATE_PIECE.fields[k][1] for k in SLOT_RATE_PIECE.names] == [0, 8, 12, 16]
    for name in ("slotsSetDelivery", "slotsStepRaggedRate", "slotTailGet", "slotTailSet", "slotsTailLen", "slotsRateCapacity"):
        assert callable(getattr(WavenetEngine, name)), name
