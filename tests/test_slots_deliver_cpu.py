"""CPU tests of ragged delivery and pipelined steps (no GPU): the new entry points are exported and declared, the
delivery kernel in the shipped code object uses no scratch, and the bookkeeping of SlotStream.step_async against a stub engine:
admission order, retirement, the headroom with steps pending, the two-deep limit, and that finished() follows collection."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_code_objects_cpu import BUILD, kernel_table

SYMBOLS = ("nvw_slots_step_ragged", "nvw_slots_wait", "nvw_slots_done", "nvw_pinned_alloc", "nvw_pinned_free")


def test_the_ragged_entries_are_exported_and_declared_within_abi_7():
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import SLOT_PIECE
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(BUILD), "..", "..", "include", "nv_wavenet_c.h")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert "} nvw_slot_piece;" in header
    # the structured dtype is the C struct: int slot; unsigned uid; long long first; int n; int finished; long long offset;
    assert SLOT_PIECE.itemsize == 32
    assert [SLOT_PIECE.fields[f][1] for f in ("slot", "uid", "first", "n", "finished", "offset")] == [0, 4, 8, 16, 20, 24]


def test_the_delivery_kernel_is_in_the_shipped_code_object_and_uses_no_scratch():
    obj = os.path.join(BUILD, "slots_deliver.o")
    assert os.path.exists(obj), "csrc/Makefile did not build slots_deliver.o (the library this file's first test loads is built from it)"
    rows = kernel_table(obj)
    names = {r[0].replace(" ", "").split("(")[0]: r for r in rows}
    assert "wn::slot_deliver_kernel" in names, sorted(names)
    _, vgpr, agpr, sgpr, scratch, spill = names["wn::slot_deliver_kernel"]
    assert scratch == 0 and spill == 0, names
    assert vgpr <= 64 and agpr == 0, names          # (a memory-bound kernel, in the range of the slots_state kernels)
    state = [r for r in kernel_table(os.path.join(BUILD, "slots_state.o")) if "slot_" in r[0]]
    assert state and vgpr <= 2 * max(r[1] for r in state) + 16, (vgpr, state)


PIECE = np.dtype([("slot", "<i4"), ("uid", "<u4"), ("first", "<i8"), ("n", "<i4"), ("finished", "<i4"), ("offset", "<i8")])


class StubEngine:
    """Stands in for WavenetEngine in slot mode with the ragged entries: sample k of the utterance with uid u is 1000 u + k, its PCM
    k mod 1000.  A step's outputs are written only when its ticket is waited for, as if the GPU were that late."""
    upStride = 4

    def __init__(self, columns):
        self.maxBatch = columns
        self.calls = []
        self.cols = {}          # column -> [uid, next local sample, length or None, frames (mel) or None]
        self.stopped = set()
        self.tickets = {}
        self.ticket = 0

    def slotsBegin(self, window):
        self.window = window

    def slotStart(self, col, x, uid):
        self.calls.append(("start", col, uid))
        self.cols[col] = [uid, 0, x.size(1), None]

    def slotStartMel(self, col, mel, uid, frames, final):
        self.calls.append(("start_mel", col, uid))
        self.cols[col] = [uid, 0, frames * self.upStride if final else None, frames]

    def slotMelFrames(self, col, frames, final):
        self.cols[col][3] = frames
        if final:
            self.cols[col][2] = frames * self.upStride

    def slotStop(self, col):
        self.calls.append(("stop", col))
        del self.cols[col]

    def slotsHeadroom(self):
        h = self.window
        for uid, k, length, frames in self.cols.values():
            if length is None:
                h = min(h, frames * self.upStride - k)
        return max(h, 0)

    def slotsPinned(self, elems, pcm=True):
        return np.full(elems, -1, dtype=np.int32), (np.full(elems, -1, dtype=np.int16) if pcm else None)

    def slotsStepRagged(self, count, samples, pcm, stream=None):
        assert 0 < count <= self.slotsHeadroom()
        rows, off, writes = [], 0, []
        for col in sorted(self.cols):
            uid, k, length, frames = self.cols[col]
            n = count if length is None else min(count, length - k)
            if n <= 0:
                continue
            rows.append((col, uid, k, n, int(length is not None and k + n == length), off))
            writes.append((off, 1000 * uid + k + np.arange(n)))
            self.cols[col][1] += n
            off = (off + n + 7) // 8 * 8
        total = rows[-1][5] + rows[-1][3] if rows else 0
        assert total <= samples.size
        self.ticket += 1
        self.tickets[self.ticket] = (samples, pcm, writes)
        self.calls.append(("ragged", count, self.ticket))
        return total, np.array(rows, dtype=PIECE), self.ticket

    def slotsWait(self, ticket):
        samples, pcm, writes = self.tickets.pop(ticket, (None, None, []))
        for off, v in writes:
            samples[off:off + len(v)] = v
            if pcm is not None:
                pcm[off:off + len(v)] = v % 1000
        self.calls.append(("wait", ticket))

    def slotsDone(self, ticket):
        return ticket not in self.tickets

    def slotsEnd(self):
        self.calls.append(("end",))


def test_step_async_admission_retirement_and_collection_two_deep():
    from nv_wavenet_amd.slots import SlotStream
    eng = StubEngine(3)
    st = SlotStream(eng, 64)
    lengths = [10, 3, 10, 5, 1, 20, 4]
    handles = [st.submit(torch.zeros(80, n)) for n in lengths]
    got = {h: [] for h in handles}
    finished, pending, steps = [], [], 0
    while st.busy() or pending:
        if st.busy():
            pending.append(st.step_async(4))
        if len(pending) == 2:
            with pytest.raises(RuntimeError):
                st.step_async(4)                       # a third: refused before anything changes
        assert len([c for c in eng.calls if c[0] == "wait"]) == steps      # issuing waits for nothing
        while len(pending) > (1 if st.busy() else 0):
            before = st.finished()
            assert before == []                        # nothing is reported before its step is collected
            out = pending.pop(0).result()
            assert np.all(out.offsets % 8 == 0)
            for h, (y, pcm) in out.items():
                got[h].append(y.copy())
                assert np.array_equal(pcm, y % 1000)
                assert np.array_equal(out[h][0], y)
            assert sorted(out.finished) == sorted(h for h in out.handles if sum(len(v) for v in got[h]) == lengths[h])
            finished += st.finished()
            steps += 1
        assert steps < 100
    assert sorted(finished) == sorted(handles) and len(finished) == len(set(finished)) and st.finished() == []
    for h, parts in got.items():
        assert np.array_equal(np.concatenate(parts), 1000 * h + np.arange(lengths[h])), h
    # FIFO admission, lowest free column first; a column is started again only after its utterance was stopped
    starts = [c for c in eng.calls if c[0] == "start"]
    assert [s[2] for s in starts] == list(range(7)) and [s[1] for s in starts[:3]] == [0, 1, 2] and starts[3][1] == 1
    owner = {}
    for c in eng.calls:
        if c[0] == "start":
            assert c[1] not in owner
            owner[c[1]] = c[2]
        elif c[0] == "stop":
            owner.pop(c[1])
    assert owner == {}
    # the same admissions as the synchronous scheduler makes
    from test_slots_cpu import FakeEngine
    ref = FakeEngine(3)
    st_ref = SlotStream(ref, 64)
    for n in lengths:
        st_ref.submit(torch.zeros(80, n))
    while st_ref.busy():
        st_ref.step(4)
    assert [c for c in ref.calls if c[0] in ("start", "stop")] == [c for c in eng.calls if c[0] in ("start", "stop")]
    st.close()


def test_step_async_headroom_counts_the_steps_pending():
    """A streamed mel request with 5 frames of 4 samples: two pending steps of 8 have used 16 of its 20 samples before any has been
    waited for, so the third is clamped to 4 and a fourth generates nothing until frames arrive."""
    from nv_wavenet_amd.slots import SlotStream
    eng = StubEngine(2)
    st = SlotStream(eng, 64)
    h = st.submit_mel(torch.zeros(80, 16), frames=5, final=False)
    hx = st.submit(torch.zeros(80, 40))
    a, b = st.step_async(8), st.step_async(8)
    assert not a.done() and not b.done() and not [c for c in eng.calls if c[0] == "wait"]
    parts = []
    oa = a.result()
    parts.append(oa[h][0].copy())                      # (views of a pinned buffer: valid until two more steps are issued)
    assert a.done() and list(oa.lengths) == [8, 8] and list(oa.offsets) == [0, 8] and list(oa.handles) == [h, hx]
    c = st.step_async(8)                               # headroom 20 - 16 = 4, with step b still pending
    assert eng.calls[-1][:2] == ("ragged", 4)
    ob = b.result()
    parts.append(ob[h][0].copy())
    d = st.step_async(8)                               # no frames left: nothing issued, an empty result
    assert [x[1] for x in eng.calls if x[0] == "ragged"] == [8, 8, 4] and len(d.result()) == 0 and d.done()
    st.extend_mel(h, 6, final=True)
    oc = c.result()
    assert list(oc.lengths) == [4, 4]
    parts.append(oc[h][0].copy())
    e = st.step_async(8)
    oe = e.result()
    assert list(oe.lengths) == [4, 8] and oe.finished == [h] and st.finished() == [h]
    parts.append(oe[h][0].copy())
    assert np.array_equal(np.concatenate(parts), 1000 * 0 + np.arange(24))
    with pytest.raises(RuntimeError):
        st.step_async(8), st.step_async(8), st.step(8)  # a synchronous step with steps pending
    st.close()
    assert eng.calls[-1] == ("end",) and not st._pending


def test_a_step_output_stays_valid_until_the_second_step_after_it_is_issued():
    """One deep, the order a simple caller uses -- collect step k, issue step k + 1, consume step k: nothing is pending when step
    k + 1 is issued, and it must still take the other buffer.  The views of step k are unchanged after step k + 1 has been issued
    and waited for, and change only with step k + 2 (the stub writes a step's samples when its ticket is waited for)."""
    from nv_wavenet_amd.slots import SlotStream
    eng = StubEngine(2)
    st = SlotStream(eng, 64)
    h = st.submit(torch.zeros(80, 100), uid=3)
    out0 = st.step_async(8).result()
    y0, p0 = out0[h]
    want_y, want_p = 3000 + np.arange(8), np.arange(8)
    assert np.array_equal(y0, want_y) and np.array_equal(p0, want_p) and not st._pending
    out1 = st.step_async(8).result()                   # issued with nothing pending, waited for
    assert np.array_equal(out1[h][0], 3008 + np.arange(8))
    assert np.array_equal(y0, want_y) and np.array_equal(p0, want_p), "step k + 1 was delivered into step k's buffer"
    assert not np.shares_memory(out0.samples, out1.samples) and not np.shares_memory(out0.pcm, out1.pcm)
    step2 = st.step_async(8)                           # the second step after step 0: its buffer is step 0's again
    assert np.array_equal(out1[h][0], 3008 + np.arange(8))
    step2.result()
    assert np.array_equal(y0, 3016 + np.arange(8)) and np.array_equal(out1[h][0], 3008 + np.arange(8))
    # ... and the same when the pipeline drains to nothing pending and refills two deep
    a, b = st.step_async(8), st.step_async(8)
    oa, ob = a.result(), b.result()
    assert not np.shares_memory(oa.samples, ob.samples)
    assert np.array_equal(oa[h][0], 3024 + np.arange(8)) and np.array_equal(ob[h][0], 3032 + np.arange(8))
    c = st.step_async(8)
    assert np.shares_memory(c.result().samples, oa.samples) and np.array_equal(ob[h][0], 3032 + np.arange(8))
    # a later step collected first collects the earlier one before it: finished() and the buffers keep the order of issue
    d, e = st.step_async(8), st.step_async(8)
    e.result()
    assert d.done() and not st._pending and [x[1] for x in eng.calls if x[0] == "wait"][-2:] == [d._ticket, e._ticket]
    st.close()
