"""CPU tests of slot mode from mel frames (no GPU): the new entry points within ABI 7, the mel-feed kernels in the shipped code
object, and the SlotStream bookkeeping of mel requests (headroom, admission, streamed frames) against a fake engine."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_code_objects_cpu import BUILD, kernel_table

MEL_SYMBOLS = ("nvw_slot_start_mel", "nvw_slot_mel_frames", "nvw_slots_headroom", "nvw_slots_get_features")


def test_mel_entries_are_declared_exported_and_bound_within_abi_7():
    from nv_wavenet_amd import _lib
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(BUILD), "..", "..", "include", "nv_wavenet_c.h")).read()
    assert "#define NVW_ABI_VERSION 7" in header
    for name in MEL_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name


def test_mel_feed_kernels_use_no_scratch():
    obj = os.path.join(BUILD, "slots_mel.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    names = {r[0].replace(" ", "").split("(")[0]: r for r in kernel_table(obj)}
    for name in ("wn::slot_mel_apply_kernel", "wn::slot_mel_stage_kernel<true>", "wn::slot_mel_stage_kernel<false>",
                 "wn::slot_mel_place_kernel<true>", "wn::slot_mel_place_kernel<false>",
                 "wn::slot_mel_upsample_kernel<true>", "wn::slot_mel_upsample_kernel<false>"):
        assert name in names, (name, sorted(names))
        _, vgpr, agpr, sgpr, scratch, spill = names[name]
        assert scratch == 0 and spill == 0, names[name]


class MelFakeEngine:
    """Slot mode by the rules of nvWavenetInfer, with mel columns: column samples are 1000 * uid + local sample; a step above the
    headroom is refused; a mel column's samples past its available frames are an error (-5)."""

    upStride = 4

    def __init__(self, columns, window=64):
        self.maxBatch = columns
        self.window = window
        self.calls = []
        self.active = {}           # col -> [uid, start, mel record or None]
        self.pending = set()
        self.t = 0

    def slotsBegin(self, window):
        self.calls.append(("begin", window))

    def slotStart(self, col, x, uid, length=None):
        self.calls.append(("start", col, uid))
        self.active[col] = [uid, None, None]
        self.pending.add(col)

    def slotStartMel(self, col, mel, uid, frames=None, final=True):
        self.calls.append(("start_mel", col, uid, frames, final))
        self.active[col] = [uid, None, [frames, final]]
        self.pending.add(col)

    def slotMelFrames(self, col, frames, final=False):
        rec = self.active[col][2]
        assert rec is not None and not rec[1] and frames >= rec[0]
        self.calls.append(("frames", col, frames, final))
        rec[0], rec[1] = frames, final

    def slotStop(self, col):
        self.calls.append(("stop", col))
        self.active.pop(col)

    def _next(self, col):
        return 0 if col in self.pending else self.t - self.active[col][1]

    def slotsHeadroom(self):
        h = self.window
        for col, (uid, start, mel) in self.active.items():
            if mel is not None and not mel[1]:
                h = min(h, mel[0] * self.upStride - self._next(col))
        return max(h, 0)

    def slotsStep(self, count, y, pcm):
        assert 0 < count <= self.window
        if any(rec[2] is not None for rec in self.active.values()):
            assert count <= self.slotsHeadroom(), "a step above the headroom"
        self.calls.append(("step", count))
        for col in self.pending:
            self.active[col][1] = self.t
        self.pending = set()
        y[:] = -1
        for col, (uid, start, mel) in self.active.items():
            k = (self.t - start) + np.arange(count)
            y[col] = 1000 * uid + k
            if mel is not None:
                y[col][k >= mel[0] * self.upStride] = -5
            if pcm is not None:
                pcm[col] = y[col] % 1000
        self.t += count
        return True

    def slotsEnd(self):
        self.calls.append(("end",))


def _steps(eng):
    return [c[1] for c in eng.calls if c[0] == "step"]


def test_headroom_clamps_a_step_and_zero_headroom_makes_no_engine_call():
    from nv_wavenet_amd.slots import SlotStream
    eng = MelFakeEngine(2)
    st = SlotStream(eng, 64)
    h = st.submit_mel(torch.zeros(80, 10), frames=3, final=False)      # 12 samples available
    out = st.step(8)
    assert list(out) == [h] and np.array_equal(out[h][0], 1000 * 0 + np.arange(8))
    out = st.step(8)                                                   # clamped to the 4 left
    assert np.array_equal(out[h][0], np.arange(8, 12)) and _steps(eng) == [8, 4]
    n = len(eng.calls)
    assert st.step(8) == {} and len(eng.calls) == n                    # no frames beyond: no engine call at all
    st.extend_mel(h, 5)
    assert np.array_equal(st.step(16)[h][0], np.arange(12, 20))
    st.extend_mel(h, 10, final=True)
    out = st.step(64)
    assert np.array_equal(out[h][0], np.arange(20, 40)) and st.finished() == [h]
    assert not st.busy() and st.finished() == []
    st.close()


def test_admission_waits_for_frames_and_keeps_fifo_order():
    from nv_wavenet_amd.slots import SlotStream
    eng = MelFakeEngine(3)
    st = SlotStream(eng, 64)
    a = st.submit(torch.zeros(80, 6))                                   # features, uid 0
    b = st.submit_mel(torch.zeros(80, 8), frames=1, final=False)        # 4 samples: not enough for a step of 8
    c = st.submit(torch.zeros(80, 5))                                   # features behind it wait too (FIFO)
    d = st.submit_mel(torch.zeros(80, 1), frames=1)                     # final: 4 samples <= any step
    out = st.step(8)
    assert set(out) == {a} and st.waiting() == 3                        # b not admitted: it would shorten the step
    st.extend_mel(b, 2)                                                 # extended while queued: 8 samples
    out = st.step(8)
    assert set(out) == {b, c, d} and _steps(eng) == [8, 8]
    assert [x[0] for x in eng.calls if x[0].startswith("start")] == ["start", "start_mel", "start", "start_mel"]
    assert ("start_mel", 0, 1, 2, False) in eng.calls                  # admitted with the frames written by then
    assert np.array_equal(out[d][0], 3000 + np.arange(4)) and d in st.finished()
    st.extend_mel(b, 8, final=True)                                     # extended while running
    while st.busy():
        for h, (y, _) in st.step(8).items():
            assert (y >= 0).all()
    st.close()


def test_a_streamed_request_completes_exactly_once_after_final():
    from nv_wavenet_amd.slots import SlotStream
    eng = MelFakeEngine(1)
    st = SlotStream(eng, 64)
    h = st.submit_mel(torch.zeros(80, 6), frames=2, final=False)
    got, done = [], []
    for frames, final in ((2, False), (4, False), (6, False), (6, True)):
        if frames != 2 or final:
            st.extend_mel(h, frames, final=final)
        for _ in range(3):
            out = st.step(16)
            if h in out:
                got.append(out[h][0])
            done += st.finished()
        assert done == ([h] if final else [])
    assert np.array_equal(np.concatenate(got), np.arange(24))
    assert not st.busy() and [c for c in eng.calls if c[0] == "stop"] == [("stop", 0)]
    with pytest.raises(KeyError):
        st.extend_mel(h, 7)
    st.close()


def test_feature_only_streams_never_ask_for_headroom():
    """(the fake engine of test_slots_cpu has no slotsHeadroom: a stream without mel requests must not need one)"""
    from nv_wavenet_amd.slots import SlotStream
    eng = MelFakeEngine(2)
    eng.slotsHeadroom = None
    st = SlotStream(eng, 64)
    h = st.submit(torch.zeros(80, 5))
    assert np.array_equal(st.step(8)[h][0], np.arange(5))
    st.close()
