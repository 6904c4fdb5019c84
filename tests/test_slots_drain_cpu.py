"""CPU tests of lists of columns saved and resumed (no GPU): the two entry points within ABI 7, the list-save kernel in
the shipped code object, SlotState.to_bytes / from_bytes against the blob layout of test_slots_state_cpu, and the SlotStream
bookkeeping of suspend_many(), drain() and resume_many() against the fake engine of test_slots_state_cpu extended by the two list
calls."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

from test_code_objects_cpu import BUILD, kernel_table
from test_slots_state_cpu import HEADER_BYTES, StateFakeEngine, from_canonical, schedule, to_canonical

LIST_SYMBOLS = ("nvw_slots_save_list", "nvw_slots_resume_list")


# ---- ABI and code object ----------------------------------------------------------------------------------------------------------

def test_list_entries_are_declared_exported_and_bound_within_abi_7():
    from nv_wavenet_amd import _lib, engine
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(BUILD), "..", "..", "include", "nv_wavenet_c.h")).read()
    assert "#define NVW_ABI_VERSION 7" in header
    for name in LIST_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert "} nvw_slot_saved;" in header and "} nvw_slot_resume_req;" in header
    # the numpy mirrors of the two structs: {int, unsigned, int, int} and {int, int, pointer, int, (pad), 2 x long long, int, int}
    assert engine.SLOT_SAVED.itemsize == 16 and [engine.SLOT_SAVED.fields[k][1] for k in ("slot", "uid", "done", "mel")] == [0, 4, 8, 12]
    assert engine.SLOT_RESUME_REQ.itemsize == 48
    assert [engine.SLOT_RESUME_REQ.fields[k][1] for k in ("slot", "mel", "src", "precision", "c_stride", "t_stride", "length", "final")] == \
        [0, 4, 8, 16, 24, 32, 40, 44]


def test_the_list_save_kernel_is_in_the_shipped_code_object_and_uses_no_scratch():
    obj = os.path.join(BUILD, "slots_state.o")
    assert os.path.exists(obj), "no slots_state.o: build the library first (__graft_entry__.build())"
    names = {r[0].replace(" ", "").split("(")[0]: r for r in kernel_table(obj)}
    assert "wn::slot_save_list_kernel" in names, sorted(names)
    _, vgpr, agpr, sgpr, scratch, spill = names["wn::slot_save_list_kernel"]
    assert scratch == 0 and spill == 0, names["wn::slot_save_list_kernel"]
    assert vgpr <= 32 and agpr == 0, names["wn::slot_save_list_kernel"]          # (a bandwidth kernel: full occupancy)


# ---- SlotState.to_bytes / from_bytes ------------------------------------------------------------------------------------------------

def _synthetic_blob(layers, max_dilation, start, done, uid, piece_bytes=32):
    """(blob bytes as a uint8 tensor, the ring [slots][piece_bytes] it canonicalises): a 64-byte header as slot_save_kernel writes
    it and the payload of a column started at counter `start`."""
    slots = sum(d for _, d in schedule(layers, max_dilation))
    ring = np.random.default_rng(done).integers(0, 256, (slots, piece_bytes), dtype=np.uint8)
    hdr = np.zeros(16, dtype="<u4")
    hdr[:10] = [0x5453574E, 1, 16, 32, layers, max_dilation, done, uid, 128, 77]
    raw = np.concatenate([hdr.view(np.uint8), to_canonical(ring, layers, max_dilation, start).reshape(-1)])
    return torch.from_numpy(raw), ring


def test_to_bytes_is_a_record_then_the_blob_and_from_bytes_brings_it_back():
    from nv_wavenet_amd.slots import SlotState
    L, D, start, done, uid = 5, 8, 7, 13, 0xFFFFFFF0          # dilations 1 2 4 8 1: unequal {off, d} rows; a uid near 2^32
    blob, ring = _synthetic_blob(L, D, start, done, uid)
    src = torch.zeros(80, 40)
    data = SlotState(blob, src, uid, done, "features").to_bytes()
    R = SlotState.RECORD_BYTES
    assert R == 32 and len(data) == R + blob.numel()
    assert struct.unpack_from("<4sIIiiIiI", data) == (b"NWSS", 1, 0, 0, 0, uid, done, blob.numel())
    assert data[R:R + HEADER_BYTES] == blob.numpy()[:HEADER_BYTES].tobytes()             # the blob's header, unchanged ...
    payload = np.frombuffer(data, dtype=np.uint8, offset=R + HEADER_BYTES).reshape(ring.shape)
    assert np.array_equal(payload, to_canonical(ring, L, D, start))                       # ... then its payload in canonical order
    assert np.array_equal(from_canonical(payload, L, D, start), ring)
    back = SlotState.from_bytes(data, src, pinned=False)
    assert (back.uid, back.done, back.kind, back.frames, back.final) == (uid, done, "features", None, None) and back.source is src
    assert not back.blob.is_cuda and back.buffer is None and torch.equal(back.blob, blob)
    assert back.to_bytes() == data
    # the mel fields, streamed and final
    for frames, final in ((4, False), (20, True)):
        m = SlotState.from_bytes(SlotState(blob, src, uid, done, "mel", frames, final).to_bytes(), src)
        assert (m.kind, m.frames, m.final, m.uid, m.done) == ("mel", frames, final, uid, done) and torch.equal(m.blob, blob)
    # a request that had not started: the record alone
    empty = SlotState(None, src, 3, 0, "mel", 2, False).to_bytes()
    assert len(empty) == R
    e = SlotState.from_bytes(empty, src)
    assert e.blob is None and (e.uid, e.done, e.kind, e.frames, e.final) == (3, 0, "mel", 2, False)


def test_from_bytes_rejects_truncated_and_foreign_data():
    from nv_wavenet_amd.slots import SlotState
    blob, _ = _synthetic_blob(5, 8, 0, 9, 2)
    src = torch.zeros(80, 40)
    data = SlotState(blob, src, 2, 9, "features").to_bytes()
    R = SlotState.RECORD_BYTES
    for bad in (b"", data[:R - 1], data[:R], data[:R + HEADER_BYTES - 1], data[:-1], data[:-16], data + b"\0",
                b"XXXX" + data[4:],                                                        # not a record
                data[:4] + struct.pack("<I", 2) + data[8:],                                # another record version
                data[:R] + b"\0\0\0\0" + data[R + 4:],                                     # the blob's magic gone
                data[:20] + struct.pack("<I", 3) + data[24:]):                             # the record's uid is not the blob's
        with pytest.raises(ValueError):
            SlotState.from_bytes(bad, src)
    assert SlotState.from_bytes(data, src).done == 9


# ---- SlotStream against a fake engine ------------------------------------------------------------------------------------------------

class DrainFakeEngine(StateFakeEngine):
    """StateFakeEngine with the two list calls by the rules of nvw_slots_save_list / nvw_slots_resume_list: a buffer is a Python list
    of ("blob", uid, done) rows; the refusals are assertions."""

    def slotsSaveList(self, slots, pinned=False, stream=None):
        from nv_wavenet_amd.engine import SLOT_SAVED
        slots = [int(c) for c in slots]
        assert slots and len(set(slots)) == len(slots)
        for col in slots:
            assert col in self.active and col not in self.pending and col not in self.move_ends, col
        self.calls.append(("save_list", tuple(slots), bool(pinned)))
        saved = np.zeros(len(slots), dtype=SLOT_SAVED)
        rows = []
        for i, col in enumerate(slots):
            uid, start, mel = self.active[col]
            saved[i] = (col, uid, self.t - start, 0 if mel is None else 1)
            rows.append(("blob", uid, self.t - start))
        return rows, saved

    def slotsResumeList(self, slots, blobs, sources, lengths_or_frames=None, finals=None):
        slots = [int(c) for c in slots]
        assert slots and len(set(slots)) == len(slots) == len(blobs) == len(sources)
        for col in slots:
            assert col not in self.active and col not in self.pending and col not in self.move_ends, "a list resume never replaces"
        self.calls.append(("resume_list", tuple(slots), tuple(b[1] for b in blobs), tuple(b[2] for b in blobs)))
        for i, col in enumerate(slots):
            blob, final = blobs[i], finals[i]
            if final is None:
                assert blob[2] < lengths_or_frames[i] == sources[i].size(1)
                self.active[col] = [blob[1], None, None]
            else:
                assert not (final and blob[2] >= lengths_or_frames[i] * self.upStride)
                self.active[col] = [blob[1], None, [lengths_or_frames[i], final]]
            self.pending[col] = blob[2]


def _collect(got, stream, out):
    for h, (y, _) in out.items():
        got.setdefault((id(stream), h), []).append(y)


def test_drain_is_one_save_and_resume_many_one_resume_per_step_and_every_sample_comes_once():
    from nv_wavenet_amd.slots import SlotStream
    e1, e2 = DrainFakeEngine(4), DrainFakeEngine(3)
    s1, s2 = SlotStream(e1, 64), SlotStream(e2, 64)
    h0 = s1.submit(torch.zeros(80, 30))
    h1 = s1.submit(torch.zeros(80, 9))
    hm = s1.submit_mel(torch.zeros(80, 20), frames=5, final=False)                  # streamed: 4 samples a frame, uid 2
    h3 = s1.submit(torch.zeros(80, 22))
    h4 = s1.submit(torch.zeros(80, 15))                                              # waits: four columns
    got = {}
    _collect(got, s1, s1.step(7))
    _collect(got, s1, s1.step(4))                                                    # the 9-sample request ends ...
    _collect(got, s1, s1.step(4))                                                    # ... and the queued one takes its column
    assert s1.running() == {h0: 0, hm: 2, h3: 3, h4: 1} and s1.finished() == [h1]
    late = s1.submit(torch.zeros(80, 6))                                             # queued when the drain comes
    before = len(e1.calls)
    states = s1.drain(pinned=True)
    assert [c for c in e1.calls[before:] if c[0] != "stop"] == [("save_list", (0, 2, 3, 1), True)]      # handle order: ONE save
    assert sorted(c[1] for c in e1.calls[before:] if c[0] == "stop") == [0, 1, 2, 3]
    assert not s1.busy() and sorted(s1._free) == [0, 1, 2, 3] and s1.compact() == 0 and s1.running() == {}
    assert [(st.uid, st.done, st.kind) for st in states] == [(0, 15, "features"), (2, 15, "mel"), (3, 15, "features"), (4, 4, "features"),
                                                             (5, 0, "features")]
    assert (states[1].frames, states[1].final) == (5, False) and states[4].blob is None
    assert all(st.buffer is states[0].buffer and st.row == i for i, st in enumerate(states[:4]))      # rows of one buffer
    s2.submit(torch.zeros(80, 3))                                                    # something already waits there
    back = s2.resume_many(states)
    assert [item[0] for item in s2._queue][:5] == back                               # at the front, in the order given
    s2.extend_mel(back[1], 10, final=True)
    before = len(e2.calls)
    _collect(got, s2, s2.step(5))
    assert [c for c in e2.calls[before:] if c[0] != "step"] == [("resume_list", (0, 1, 2), (0, 2, 3), (15, 15, 15))]      # ONE resume
    while s2.busy():
        _collect(got, s2, s2.step(5))
        s2.finished()
    assert [c[2:] for c in e2.calls if c[0] == "resume_list"][1] == ((4,), (4,))     # the fourth row, in a later step
    for h_old, h_new, uid, n in ((h0, back[0], 0, 30), (hm, back[1], 2, 40), (h3, back[2], 3, 22), (h4, back[3], 4, 15), (late, back[4], 5, 6)):
        y = np.concatenate(got.get((id(s1), h_old), []) + got[(id(s2), h_new)])
        assert np.array_equal(y, 1000 * uid + np.arange(n)), (uid, y)
    s1.close(), s2.close()


def test_suspend_many_keeps_the_order_of_its_handles_and_refuses_before_it_changes_anything():
    from nv_wavenet_amd.slots import SlotStream
    eng = DrainFakeEngine(48)
    st = SlotStream(eng, 64)
    handles = [st.submit(torch.zeros(80, 1000 if c in (3, 17, 30, 40) else 4)) for c in range(48)]
    waiting = st.submit(torch.zeros(80, 50))                                         # no column for it in the first step
    st.step(4)
    assert st.waiting() == 1 and sorted(st.running().values()) == [3, 17, 30, 40]
    assert st.compact() == 3                                                         # 40 -> 0, 30 -> 1, 17 -> 2: pending until the next step

    def snapshot():
        return (dict(st.running()), sorted(st._free), dict(st._src), [item[0] for item in st._queue], len(eng.calls))

    before = snapshot()
    with pytest.raises(RuntimeError):
        st.suspend_many([handles[3], waiting, handles[40]])                          # the last one is on its way to column 0
    with pytest.raises(KeyError):
        st.suspend_many([handles[3], 12345])
    with pytest.raises(ValueError):
        st.suspend_many([handles[3], waiting, handles[3]])
    assert snapshot() == before, "a refused suspend_many changed the stream"
    q, r = st.suspend_many([waiting, handles[3]])                                    # a queued and a running one, in the order asked for
    assert (q.blob, q.done, q.uid) == (None, 0, 48) and (r.done, r.uid, r.row) == (4, 3, 0) and r.blob == ("blob", 3, 4)
    assert eng.calls[-2:] == [("save_list", (3,), False), ("stop", 3)] and st.waiting() == 0 and 3 in st._free
    st.step(4)                                                                       # applies the moves
    rest = st.suspend_many()                                                         # everything: handle order
    assert [s.uid for s in rest] == [17, 30, 40] and [s.done for s in rest] == [8, 8, 8]
    assert ("save_list", (2, 1, 0), False) in eng.calls and not st.busy() and sorted(st._free) == list(range(48))
    assert st.suspend_many() == [] and st.drain() == []                              # an empty stream: no engine call
    st.close()


def test_resume_refuses_a_blob_of_another_size_before_it_queues_anything():
    from nv_wavenet_amd.slots import SlotState, SlotStream

    class Sized(DrainFakeEngine):
        def slotStateBytes(self):
            return 128

    st = SlotStream(Sized(2), 64)
    src = torch.zeros(80, 40)
    good = SlotState(torch.zeros(128, dtype=torch.uint8), src, 1, 3, "features")
    other = SlotState(torch.zeros(192, dtype=torch.uint8), src, 2, 3, "features")
    with pytest.raises(ValueError):
        st.resume(other)
    with pytest.raises(ValueError):
        st.resume_many([good, other])                                                # the good one is not queued either
    assert st.waiting() == 0 and not st.busy() and st._next_handle == 0
    st.close()
