"""CPU tests of the sampling temperature (no GPU): the three entry points within ABI 7, the scatter kernel in the
shipped code object, the temperature word of a state blob through SlotState.to_bytes / from_bytes, and the SlotStream bookkeeping
-- submit(temperature=), set_temperature, compact, suspend / resume -- against a stub engine that models slotSetTemperature by the
rules of nvWavenetInfer (a start puts the column back to 1, a move carries the value, a resume takes the blob's)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_code_objects_cpu import BUILD, kernel_table
from test_slots_state_cpu import HEADER_BYTES, StateFakeEngine, schedule, to_canonical

TEMPERATURE_SYMBOLS = ("nvw_set_temperatures", "nvw_slot_set_temperature", "nvw_slot_temperature")
WORD = 10                                    # of the blob's header: the temperature as the bits of the float, zero for 1.0


def _bits(T):
    return int(np.array([T], dtype="<f4").view("<u4")[0])


# ---- ABI and code object ----------------------------------------------------------------------------------------------------------

def test_temperature_entries_are_declared_exported_and_bound_within_abi_7():
    from nv_wavenet_amd import _lib, engine, slots
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(BUILD), "..", "..", "include", "nv_wavenet_c.h")).read()
    assert "#define NVW_ABI_VERSION 7" in header
    for name in TEMPERATURE_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert _lib.SIGNATURES["nvw_slot_temperature"][0] is ctypes.c_float
    assert _lib.SIGNATURES["nvw_slot_set_temperature"][1][-1] is ctypes.c_float
    for name in ("setTemperatures", "slotSetTemperature", "slotTemperature"):
        assert hasattr(engine.WavenetEngine, name), name
    assert hasattr(slots.SlotStream, "set_temperature")


def test_the_scatter_kernel_is_in_the_shipped_code_object_and_uses_no_scratch():
    obj = os.path.join(BUILD, "slots_sampler.o")
    assert os.path.exists(obj), "no slots_sampler.o: build the library first (__graft_entry__.build())"
    names = {r[0].replace(" ", "").split("(")[0]: r for r in kernel_table(obj)}
    assert "wn::slot_scale_kernel" in names, sorted(names)
    _, vgpr, agpr, sgpr, scratch, spill = names["wn::slot_scale_kernel"]
    assert scratch == 0 and spill == 0 and vgpr <= 32 and agpr == 0, names["wn::slot_scale_kernel"]


# ---- SlotState ---------------------------------------------------------------------------------------------------------------------

def _synthetic_blob(layers, max_dilation, done, uid, temperature=None, piece_bytes=32):
    """A blob as slot_save_kernel writes it: the 64-byte header (word 10: zero for T = 1, else the bits of T), then the payload."""
    slots = sum(d for _, d in schedule(layers, max_dilation))
    ring = np.random.default_rng(done).integers(0, 256, (slots, piece_bytes), dtype=np.uint8)
    hdr = np.zeros(16, dtype="<u4")
    hdr[:10] = [0x5453574E, 1, 16, 32, layers, max_dilation, done, uid, 128, 77]
    if temperature is not None:
        hdr[WORD] = _bits(temperature)
    return torch.from_numpy(np.concatenate([hdr.view(np.uint8), to_canonical(ring, layers, max_dilation, 3).reshape(-1)]))


def test_the_temperature_survives_to_bytes_and_from_bytes():
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    R = SlotState.RECORD_BYTES
    # word 10 zero reads as 1.0; a blob made at T = 1 keeps word 10 zero through the trip
    blob = _synthetic_blob(5, 8, 13, 4)
    s1 = SlotState(blob, src, 4, 13, "features")
    assert s1.temperature == 1.0
    data = s1.to_bytes()
    assert np.frombuffer(data, dtype="<u4", count=16, offset=R)[WORD] == 0
    back = SlotState.from_bytes(data, src)
    assert back.temperature == 1.0 and torch.equal(back.blob, blob)
    # a tempered blob: the value is read from the header, and the bytes are unchanged
    for T in (0.8, 0.25, 4.0, 2.0 ** -10, 2.0 ** 10):
        T = float(np.float32(T))
        blob = _synthetic_blob(5, 8, 13, 4, T)
        data = SlotState(blob, src, 4, 13, "mel", 9, False, temperature=T).to_bytes()
        assert data[R:] == blob.numpy().tobytes()
        back = SlotState.from_bytes(data, src)
        assert back.temperature == T and (back.kind, back.frames, back.final, back.done) == ("mel", 9, False, 13)
        assert back.to_bytes() == data
    # the bits of 1.0 in the word are a valid temperature too
    assert SlotState.from_bytes(SlotState(_synthetic_blob(5, 8, 13, 4, 1.0), src, 4, 13, "features").to_bytes(), src).temperature == 1.0
    # a request that had not started: the record alone at T = 1 (as before), the record and a bare header otherwise
    assert len(SlotState(None, src, 3, 0, "features").to_bytes()) == R
    data = SlotState(None, src, 3, 0, "mel", 2, False, temperature=0.5).to_bytes()
    assert len(data) == R + HEADER_BYTES
    back = SlotState.from_bytes(data, src)
    assert back.blob is None and back.temperature == 0.5 and (back.uid, back.done, back.kind, back.frames, back.final) == (3, 0, "mel", 2, False)
    assert back.to_bytes() == data


@pytest.mark.parametrize("word", [_bits(-0.0), _bits(-1.0), _bits(float("nan")), _bits(float("inf")), _bits(2.0 ** -11), _bits(2049.0), 1])
def test_from_bytes_refuses_a_bad_temperature_word(word):
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    blob = _synthetic_blob(5, 8, 9, 2)
    blob.numpy().view("<u4")[WORD] = word
    data = SlotState.RECORD.pack(b"NWSS", 1, 0, 0, 0, 2, 9, blob.numel()) + blob.numpy().tobytes()
    with pytest.raises(ValueError):
        SlotState.from_bytes(data, src)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), 2.0 ** -11, 1025.0, "warm", None])
def test_bad_values_raise_everywhere_and_change_nothing(bad):
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = TemperatureFakeEngine(4)
    st = SlotStream(eng, 64)
    x = torch.zeros(80, 30)
    with pytest.raises(ValueError):
        st.submit(x, temperature=bad)
    with pytest.raises(ValueError):
        st.submit_mel(torch.zeros(80, 5), temperature=bad)
    assert not st.busy() and st._next_handle == 0
    h = st.submit(x, temperature=2.0)
    with pytest.raises(ValueError):
        st.set_temperature(h, bad)                  # waiting
    st.step(4)
    with pytest.raises(ValueError):
        st.set_temperature(h, bad)                  # running
    assert st.temperature(h) == 2.0 and eng.temp[0] == 2.0
    assert [c for c in eng.calls if c[0] == "temperature"] == [("temperature", 0, 2.0)]
    with pytest.raises(ValueError):
        SlotState(None, x, 0, 0, "features", temperature=bad)
    with pytest.raises(KeyError):
        st.set_temperature(99, 1.0)
    st.close()


# ---- SlotStream against a stub engine ----------------------------------------------------------------------------------------------

class TemperatureFakeEngine(StateFakeEngine):
    """StateFakeEngine with the temperature by the engine's rules: per column, 1 after a start, the blob's after a resume, carried by
    a move; slotSetTemperature needs an utterance (or a pending start or resume) in the column.  Blobs are ("blob", uid, done, T).
    temps_at_step[i]: {uid: T} in force for step i."""

    def __init__(self, columns, window=64):
        super().__init__(columns, window)
        self.temp = {}
        self.temps_at_step = []

    def slotStart(self, col, x, uid, length=None):
        super().slotStart(col, x, uid, length)
        self.temp[col] = 1.0

    def slotStartMel(self, col, mel, uid, frames=None, final=True):
        super().slotStartMel(col, mel, uid, frames, final)
        self.temp[col] = 1.0

    def slotResume(self, col, blob, x, length=None):
        super().slotResume(col, blob, x, length)
        self.temp[col] = blob[3]

    def slotResumeMel(self, col, blob, mel, frames=None, final=True):
        super().slotResumeMel(col, blob, mel, frames, final)
        self.temp[col] = blob[3]

    def slotStop(self, col):
        super().slotStop(col)
        self.temp.pop(col)

    def slotMove(self, src, dst):
        super().slotMove(src, dst)
        self.temp[dst] = self.temp.pop(src)

    def slotSave(self, col, stream=None):
        blob, done = super().slotSave(col, stream)
        return blob + (self.temp[col],), done

    def slotSetTemperature(self, col, T):
        assert col in self.active, "a temperature for a column without an utterance"
        assert 2.0 ** -10 <= T <= 2.0 ** 10
        self.calls.append(("temperature", col, T))
        self.temp[col] = T

    def slotStateBytes(self):
        return 0

    def slotsStep(self, count, y, pcm):
        self.temps_at_step.append({self.active[c][0]: self.temp[c] for c in self.active})
        return super().slotsStep(count, y, pcm)


def _kinds(eng, since=0):
    return [c[0] for c in eng.calls[since:]]


def test_submit_with_a_temperature_sets_it_after_the_start_and_before_the_step():
    from nv_wavenet_amd.slots import SlotStream
    eng = TemperatureFakeEngine(3)
    st = SlotStream(eng, 64)
    a = st.submit(torch.zeros(80, 12), temperature=0.5)
    b = st.submit(torch.zeros(80, 12))                                   # T = 1: no call at all
    c = st.submit_mel(torch.zeros(80, 3), temperature=1.3)
    d = st.submit(torch.zeros(80, 8), temperature=4.0)                   # waits for a column
    st.step(4)
    assert _kinds(eng) == ["begin", "start", "start", "start_mel", "temperature", "temperature", "step"]
    T13 = float(np.float32(1.3))
    assert [x for x in eng.calls if x[0] == "temperature"] == [("temperature", 0, 0.5), ("temperature", 2, T13)]
    assert eng.temps_at_step[0] == {0: 0.5, 1: 1.0, 2: T13}
    assert (st.temperature(a), st.temperature(b), st.temperature(c), st.temperature(d)) == (0.5, 1.0, T13, 4.0)
    # a running request: at once, in force from the next step
    st.set_temperature(b, 2.0)
    assert eng.calls[-1] == ("temperature", 1, 2.0)
    st.step(4)
    assert eng.temps_at_step[1] == {0: 0.5, 1: 2.0, 2: T13}
    # a waiting request: when it is admitted, after its start
    st.set_temperature(d, 0.25)
    assert eng.calls[-1][0] == "step"
    st.step(4)                                                           # a, b and c (3 frames x 4) end here
    before = len(eng.calls)
    st.step(4)
    assert _kinds(eng, before)[-3:] == ["start", "temperature", "step"] and eng.calls[-2] == ("temperature", 0, 0.25)
    assert eng.temps_at_step[3] == {3: 0.25}
    while st.busy():
        st.step(4)
    assert st._sampling == {}                                                # nothing is kept of a finished request
    st.close()


def test_compact_and_suspend_and_resume_keep_the_temperature():
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = TemperatureFakeEngine(40)
    st = SlotStream(eng, 64)
    hs = [st.submit(torch.zeros(80, 4 if i < 38 else 40), temperature=1.0 if i < 38 else (0.5, 2.0)[i - 38]) for i in range(40)]
    st.step(4)
    assert st.compact() == 2                                             # 39 -> 0, 38 -> 1: the engine's move carries the value
    n_set = len([c for c in eng.calls if c[0] == "temperature"])
    st.step(4)
    assert eng.temps_at_step[-1] == {39: 2.0, 38: 0.5} and (eng.temp[0], eng.temp[1]) == (2.0, 0.5)
    assert len([c for c in eng.calls if c[0] == "temperature"]) == n_set, "a move needs no new call"
    # suspend: the state carries it; resume in another stream: the engine takes it from the blob, no call
    state = st.suspend(hs[39])
    assert state.temperature == 2.0 and state.blob[3] == 2.0 and state.done == 8
    other_eng = TemperatureFakeEngine(2)
    other = SlotStream(other_eng, 64)
    h2 = other.resume(state)
    assert other.temperature(h2) == 2.0
    other.step(4)
    assert other_eng.temps_at_step[0] == {39: 2.0} and "temperature" not in _kinds(other_eng)
    # ... unless it was changed while it waited, or on the state: then start / resume, then set
    state = other.suspend(h2)
    state.temperature = 0.25
    h3 = other.resume(state)
    assert other.temperature(h3) == 0.25
    other.step(4)
    assert _kinds(other_eng)[-3:] == ["resume", "temperature", "step"] and other_eng.temps_at_step[-1] == {39: 0.25}
    # a request suspended before it started keeps it too (through bytes as well)
    w = other.submit(torch.zeros(80, 6), temperature=0.5)
    w2 = other.submit(torch.zeros(80, 6))
    w3 = other.submit(torch.zeros(80, 6), temperature=8.0)
    waiting = other.suspend(w3)
    assert waiting.blob is None and waiting.temperature == 8.0
    again = SlotState.from_bytes(waiting.to_bytes(), waiting.source)
    assert again.blob is None and again.temperature == 8.0
    h4 = st.resume(again)
    st.step(4)
    assert eng.temps_at_step[-1][again.uid] == 8.0 and st.temperature(h4) == 8.0
    states = [other.suspend(h) for h in (h3, w, w2)]
    assert [s.temperature for s in states] == [0.25, 0.5, 1.0]
    assert other._sampling == {}
    other.close()
    st.close()
