"""CPU tests of a column's state as a value (no GPU): the new entry points within ABI 7, the move / save / load
kernels in the shipped code object, the canonical rotation restated in numpy (shared with tests/test_slots_state_gpu.py), and the
SlotStream bookkeeping of compact(), suspend() and resume() against a fake engine that models slotMove / slotSave / slotResume.

The canonical form.  The dilation ring has one slot per (layer, sample mod dilation): layer l with dilation d_l owns slots
off_l .. off_l + d_l - 1 (off_l = sum of the dilations before it), and at engine counter t it reads and then writes slot
off_l + (t mod d_l).  A column whose utterance started at counter `start` therefore keeps local sample k's value of layer l in
slot off_l + ((start + k) mod d_l).  The blob stores it at off_l + (k mod d_l): blob[off_l + i] = ring[off_l + ((i + start) mod
d_l)], and a resume at start' writes ring[off_l + ((i + start') mod d_l)] = blob[off_l + i]."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_code_objects_cpu import BUILD, kernel_table

STATE_SYMBOLS = ("nvw_slot_state_bytes", "nvw_slot_move", "nvw_slot_save", "nvw_slot_resume", "nvw_slot_resume_mel")
HEADER_BYTES = 64


# ---- the canonical rotation in numpy ---------------------------------------------------------------------------------------------

def schedule(layers, max_dilation):
    """(off, d) of every layer: d doubles per layer and returns to 1 past max_dilation."""
    out, d, off = [], 1, 0
    for _ in range(layers):
        out.append((off, d))
        off += d
        d = 1 if 2 * d > max_dilation else 2 * d
    return out


def ring_slot_of(layers, max_dilation, start):
    """src[s]: the ring slot that canonical (blob) slot s of a column started at counter `start` lives in."""
    src = []
    for off, d in schedule(layers, max_dilation):
        src += [off + ((i + start) % d) for i in range(d)]
    return np.array(src)


def to_canonical(ring, layers, max_dilation, start):
    """ring [slots][...] of a column started at `start` -> the blob's payload."""
    return ring[ring_slot_of(layers, max_dilation, start)]


def from_canonical(blob, layers, max_dilation, start):
    """the blob's payload -> the ring [slots][...] of a column resumed with start' = `start`."""
    ring = np.empty_like(blob)
    ring[ring_slot_of(layers, max_dilation, start)] = blob
    return ring


def _simulated_ring(layers, max_dilation, start, done):
    """What a column's ring holds after `done` local samples from counter `start`: per slot (layer, local sample written last), -1 = never."""
    sch = schedule(layers, max_dilation)
    ring = np.full((sum(d for _, d in sch), 2), -1)
    for k in range(done):
        for l, (off, d) in enumerate(sch):
            ring[off + (start + k) % d] = (l, k)
    return ring


@pytest.mark.parametrize("layers,max_dilation", [(20, 32), (20, 512), (7, 4), (8, 8)])
def test_the_canonical_form_does_not_depend_on_the_start(layers, max_dilation):
    for done in (0, 1, 3, max_dilation - 1, max_dilation + 5, 3 * max_dilation + 1):
        want = _simulated_ring(layers, max_dilation, 0, done)
        for start in (1, 7, max_dilation - 1, 4097, -3, -max_dilation - 1):
            ring = _simulated_ring(layers, max_dilation, start, done)
            blob = to_canonical(ring, layers, max_dilation, start)
            assert np.array_equal(blob, want), (done, start)
            # slots never written stay unwritten under the rotation (the zero-tap rule), and a resume elsewhere inverts it
            for start2 in (0, 5, -9):      # (start2: the utterance's start as the resuming engine sees it, its counter - done)
                assert np.array_equal(from_canonical(blob, layers, max_dilation, start2),
                                      _simulated_ring(layers, max_dilation, start2, done)), (done, start, start2)
    sch = schedule(layers, max_dilation)
    assert sch[0] == (0, 1) and max(d for _, d in sch) <= max_dilation
    assert [o for o, _ in sch] == list(np.cumsum([0] + [d for _, d in sch][:-1]))


def test_an_odd_offset_rotates_every_dilation_above_one():
    a, b = ring_slot_of(20, 32, 0), ring_slot_of(20, 32, 33)
    for off, d in schedule(20, 32):
        assert (a[off:off + d] != b[off:off + d]).all() == (d > 1), (off, d)


# ---- ABI and code object ----------------------------------------------------------------------------------------------------------

def test_state_entries_are_declared_exported_and_bound_within_abi_7():
    from nv_wavenet_amd import _lib
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(BUILD), "..", "..", "include", "nv_wavenet_c.h")).read()
    assert "#define NVW_ABI_VERSION 7" in header
    for name in STATE_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name


def test_state_kernels_are_in_the_shipped_code_object_and_use_no_scratch():
    obj = os.path.join(BUILD, "slots_state.o")
    if not os.path.exists(os.path.join(BUILD, "slots.o")):
        pytest.skip("build the library first (__graft_entry__.build())")
    assert os.path.exists(obj), "the library is built but has no slots_state.o"
    names = {r[0].replace(" ", "").split("(")[0]: r for r in kernel_table(obj)}
    for name in ("wn::slot_move_kernel", "wn::slot_save_kernel", "wn::slot_load_kernel"):
        assert name in names, (name, sorted(names))
        _, vgpr, agpr, sgpr, scratch, spill = names[name]
        assert scratch == 0 and spill == 0, names[name]
        assert vgpr <= 32 and agpr == 0, names[name]          # (bandwidth kernels: full occupancy)


# ---- SlotStream against a fake engine ------------------------------------------------------------------------------------------------

class StateFakeEngine:
    """Slot mode by the rules of nvWavenetInfer with moves, saves and resumes: local sample k of uid u is 1000 u + k; a mel column's
    samples past its frames are -5.  A blob is ("blob", uid, done).  The refusals of nvw_slot_move / save / resume are assertions."""

    upStride = 4

    def __init__(self, columns, window=64):
        self.maxBatch = columns
        self.window = window
        self.calls = []
        self.active = {}           # col -> [uid, start, mel record or None]
        self.pending = {}          # col -> done of a pending start (0) or resume
        self.move_ends = set()
        self.t = 0

    def slotsBegin(self, window):
        self.calls.append(("begin", window))

    def slotStart(self, col, x, uid, length=None):
        self.calls.append(("start", col, uid))
        self.active[col] = [uid, None, None]
        self.pending[col] = 0

    def slotStartMel(self, col, mel, uid, frames=None, final=True):
        self.calls.append(("start_mel", col, uid, frames, final))
        self.active[col] = [uid, None, [frames, final]]
        self.pending[col] = 0

    def slotResume(self, col, blob, x, length=None):
        assert blob[0] == "blob" and blob[2] < x.size(1)
        self.calls.append(("resume", col, blob[1], blob[2]))
        self.active[col] = [blob[1], None, None]
        self.pending[col] = blob[2]

    def slotResumeMel(self, col, blob, mel, frames=None, final=True):
        assert blob[0] == "blob" and not (final and blob[2] >= frames * self.upStride)
        self.calls.append(("resume_mel", col, blob[1], blob[2], frames, final))
        self.active[col] = [blob[1], None, [frames, final]]
        self.pending[col] = blob[2]

    def slotMelFrames(self, col, frames, final=False):
        rec = self.active[col][2]
        assert rec is not None and not rec[1] and frames >= rec[0]
        self.calls.append(("frames", col, frames, final))
        rec[0], rec[1] = frames, final

    def slotStop(self, col):
        self.calls.append(("stop", col))
        self.active.pop(col)
        self.pending.pop(col, None)

    def slotMove(self, src, dst):
        assert 0 <= src < self.maxBatch and 0 <= dst < self.maxBatch and src != dst
        assert src in self.active and src not in self.pending and src not in self.move_ends, "source of a move"
        assert dst not in self.active and dst not in self.pending and dst not in self.move_ends, "destination of a move"
        self.calls.append(("move", src, dst))
        self.active[dst] = self.active.pop(src)
        self.move_ends |= {src, dst}

    def slotSave(self, col, stream=None):
        assert col in self.active and col not in self.pending and col not in self.move_ends
        done = self.t - self.active[col][1]
        self.calls.append(("save", col, done))
        return ("blob", self.active[col][0], done), done

    def _next(self, col):
        return self.pending[col] if col in self.pending else self.t - self.active[col][1]

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
        self.calls.append(("step", count, max(self.active, default=-1) // 16 + 1))
        for col, done in self.pending.items():
            self.active[col][1] = self.t - done
        self.pending = {}
        self.move_ends = set()
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


def _occupy(columns, wanted, compact=False):
    """A stream whose running requests sit exactly in the columns `wanted` (long requests; the others were short and are gone)."""
    from nv_wavenet_amd.slots import SlotStream
    eng = StateFakeEngine(columns)
    st = SlotStream(eng, 64, compact=compact)
    handles = [st.submit(torch.zeros(80, 1000 if c in wanted else 4)) for c in range(columns)]
    st.step(4)
    assert sorted(st.running().values()) == sorted(wanted)
    return eng, st, handles


def _moves(eng):
    return [c[1:] for c in eng.calls if c[0] == "move"]


@pytest.mark.parametrize("columns,wanted,moves", [
    (48, [0, 1, 2], []),                                              # packed already: no engine call
    (48, [], []),
    (48, list(range(48)), []),                                        # a full batch
    (48, [3, 17, 40], [(40, 0), (17, 1)]),                            # n = 3: bound 16; highest source first, lowest free first
    (48, [0, 16, 47], [(47, 1), (16, 2)]),
    (48, list(range(16)) + [47], [(47, 16)]),                         # n = 17: bound 32
    (48, list(range(1, 17)), [(16, 0)]),                              # n = 16: bound 16, one column beyond it
    (40, [5, 39], [(39, 0)]),
    (64, [15, 31, 47, 63] + list(range(16, 30)), [(63, 0), (47, 1)]),   # n = 18: bound 32; 31 and 16..29 stay where they are
])
def test_compact_moves_exactly_what_the_rule_says(columns, wanted, moves):
    eng, st, handles = _occupy(columns, wanted)
    before = len(eng.calls)
    assert st.compact() == len(moves)
    assert _moves(eng) == moves
    if not moves:
        assert len(eng.calls) == before, "no engine call when there is nothing to move"
    n = len(wanted)
    bound = 16 * ((n + 15) // 16)
    assert all(c < bound for c in st.running().values()) and len(set(st.running().values())) == n
    assert sorted(st._free + list(st._running)) == list(range(columns))
    moved = dict(moves)
    for c in wanted:
        assert st.running()[handles[c]] == moved.get(c, c)
    assert st.compact() == 0                                          # idempotent
    # the requests go on where they were: samples continue without a gap or a repeat
    out = st.step(8)
    for c in wanted:
        assert np.array_equal(out[handles[c]][0], 1000 * c + 4 + np.arange(8)), c
    st.close()


def test_compact_true_runs_between_retirement_and_admission_and_false_never_moves():
    from nv_wavenet_amd.slots import SlotStream
    for compact in (False, True):
        eng = StateFakeEngine(48)
        st = SlotStream(eng, 64, compact=compact)
        lengths = [4] * 48
        for c in (20, 33, 47):
            lengths[c] = 40
        handles = [st.submit(torch.zeros(80, n)) for n in lengths]
        late = [st.submit(torch.zeros(80, 12)) for _ in range(2)]
        got = {h: [] for h in handles + late}
        while st.busy():
            for h, (y, _) in st.step(4).items():
                got[h].append(y)
            st.finished()
        for i, h in enumerate(handles + late):
            assert np.array_equal(np.concatenate(got[h]), 1000 * i + np.arange((lengths + [12, 12])[i])), i
        calls = eng.calls
        if not compact:
            assert not _moves(eng)
            assert [c[2] for c in calls if c[0] == "step"][1] == 3        # the survivors keep three tiles launched
            continue
        # step 2: the 45 stops of step 1 came first, then the moves, then the admissions -- into the packed front
        second = calls[[i for i, c in enumerate(calls) if c[0] == "step"][0] + 1:]
        kinds = [c[0] for c in second[:second.index(next(c for c in second if c[0] == "step"))]]
        assert kinds == ["stop"] * 45 + ["move"] * 3 + ["start"] * 2, kinds
        assert _moves(eng) == [(47, 0), (33, 1), (20, 2)]
        starts = [c for c in calls if c[0] == "start"][48:]
        assert [s[1] for s in starts] == [3, 4]
        assert all(c[2] == 1 for c in calls if c[0] == "step" and c is not calls[[i for i, c in enumerate(calls) if c[0] == "step"][0]])
        st.close()


def test_compact_moves_mel_requests_and_they_can_still_be_extended():
    from nv_wavenet_amd.slots import SlotStream
    eng = StateFakeEngine(40)
    st = SlotStream(eng, 64)
    hs = [st.submit(torch.zeros(80, 4)) for _ in range(38)]
    hm = st.submit_mel(torch.zeros(80, 50), frames=3, final=False)       # column 38
    hf = st.submit_mel(torch.zeros(80, 6))                               # column 39, final: 24 samples
    got = {hm: [], hf: []}

    def step(n):
        for h, (y, _) in st.step(n).items():
            if h in got:
                got[h].append(y)

    step(4)
    assert st.compact() == 2 and _moves(eng) == [(39, 0), (38, 1)]
    assert st.running() == {hf: 0, hm: 1}
    st.extend_mel(hm, 5)                                                 # goes to the new column
    assert ("frames", 1, 5, False) in eng.calls
    step(64)                                                             # clamped by the headroom: 5 * 4 - 4 = 16
    st.extend_mel(hm, 8, final=True)
    while st.busy():
        step(64)
    assert np.array_equal(np.concatenate(got[hm]), 1000 * 38 + np.arange(32))
    assert np.array_equal(np.concatenate(got[hf]), 1000 * 39 + np.arange(24))
    assert sorted(st.finished()) == sorted(hs + [hm, hf])
    st.close()


def test_suspend_and_resume_deliver_every_sample_once_and_resume_goes_to_the_front():
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = StateFakeEngine(2)
    st = SlotStream(eng, 64)
    a = st.submit(torch.zeros(80, 30))
    b = st.submit(torch.zeros(80, 30))
    c = st.submit(torch.zeros(80, 9))          # queued
    d = st.submit(torch.zeros(80, 9))          # queued
    got = {}

    def step(stream, n):
        for h, (y, _) in stream.step(n).items():
            got.setdefault((id(stream), h), []).append(y)

    step(st, 7)
    state = st.suspend(a)
    assert isinstance(state, SlotState) and state.done == 7 and state.uid == 0 and state.kind == "features" and state.blob[0] == "blob"
    assert a not in st.running() and eng.calls[-2:] == [("save", 0, 7), ("stop", 0)]
    empty = st.suspend(d)                       # a queued request: dequeued, an empty state
    assert empty.blob is None and empty.done == 0 and empty.uid == 3 and st.waiting() == 1
    step(st, 5)                                 # c takes the freed column 0
    assert st.running()[c] == 0
    a2 = st.resume(state)                       # in front of everything that waits
    d2 = st.resume(empty)                       # ... and this one in front of that
    assert [item[0] for item in st._queue] == [d2, a2]
    while st.busy():
        step(st, 5)
        st.finished()
    key = lambda h: (id(st), h)
    assert np.array_equal(np.concatenate(got[key(a)] + got[key(a2)]), np.arange(30))
    assert np.array_equal(np.concatenate(got[key(a)]), np.arange(7))
    assert np.array_equal(np.concatenate(got[key(b)]), 1000 + np.arange(30))
    assert np.array_equal(np.concatenate(got[key(c)]), 2000 + np.arange(9))
    assert np.array_equal(np.concatenate(got[key(d2)]), 3000 + np.arange(9))
    assert ("resume", 0, 0, 7) in eng.calls or ("resume", 1, 0, 7) in eng.calls
    assert [x for x in eng.calls if x[0] == "start" and x[2] == 3], "an empty state starts from sample 0"
    st.close()


def test_a_suspended_request_resumes_on_another_stream_and_a_streamed_mel_request_goes_on():
    from nv_wavenet_amd.slots import SlotStream
    e1, e2 = StateFakeEngine(3), StateFakeEngine(3)
    s1, s2 = SlotStream(e1, 64), SlotStream(e2, 64)
    x = s1.submit(torch.zeros(80, 40), uid=11)
    m = s1.submit_mel(torch.zeros(80, 20), uid=12, frames=4, final=False)
    first = {x: [], m: []}
    for n in (6, 3):
        for h, (y, _) in s1.step(n).items():
            first[h].append(y)
    sx, sm = s1.suspend(x), s1.suspend(m)
    assert not s1.busy() and (sx.done, sm.done, sm.kind, sm.frames, sm.final) == (9, 9, "mel", 4, False)
    s2.submit(torch.zeros(80, 3))                      # something already waits there
    m2, x2 = s2.resume(sm), s2.resume(sx)
    assert [item[0] for item in s2._queue][:2] == [x2, m2]
    rest = {x2: [], m2: []}
    out = s2.step(64)                                  # 4 * 4 - 9 = 7 samples of frames left: m2 is not admitted for a step of 64 ...
    assert m2 not in out and m2 not in s2.running()
    rest[x2].append(out[x2][0])
    out = s2.step(5)                                   # ... but for one of 5, counted from done
    assert len(out[m2][0]) == 5 and e2.slotsHeadroom() == 2
    rest[m2].append(out[m2][0])
    s2.extend_mel(m2, 10, final=True)                  # a resumed streamed request is extended under its new handle
    while s2.busy():
        for h, (y, _) in s2.step(64).items():
            if h in rest:
                rest[h].append(y)
    assert np.array_equal(np.concatenate(first[x] + rest[x2]), 11000 + np.arange(40))
    assert np.array_equal(np.concatenate(first[m] + rest[m2]), 12000 + np.arange(40))
    assert [c for c in e2.calls if c[0] == "resume_mel"][0][2:] == (12, 9, 4, False)
    s1.close(), s2.close()


def test_suspend_and_compact_while_moves_wait_for_their_step_leave_the_stream_whole():
    """compact() on demand leaves its columns endpoints of pending moves until the next step.  In that window suspend() of a moved
    request refuses before it has changed anything; suspend() of another request works; and a second compact() -- which with fewer
    running requests would pick a pending destination as a source -- waits.  Afterwards every request delivers every sample once."""
    eng, st, handles = _occupy(48, [3, 17, 30, 40])
    got = {handles[c]: [1000 * c + np.arange(4)] for c in (3, 17, 30, 40)}
    assert st.compact() == 3 and _moves(eng) == [(40, 0), (30, 1), (17, 2)]
    before = (dict(st.running()), sorted(st._free), dict(st._src), len(eng.calls))
    with pytest.raises(RuntimeError):
        st.suspend(handles[40])                          # in column 0 now, its move not yet applied
    assert (dict(st.running()), sorted(st._free), dict(st._src), len(eng.calls)) == before, "a refused suspend changed the stream"
    state = st.suspend(handles[3])                       # not moved: saved, stopped, its column free
    assert state.done == 4 and 3 in st._free
    assert st.compact() == 0 and len(_moves(eng)) == 3   # three running, bound 16: nothing to do, and nothing attempted
    eng2, st2, h2 = _occupy(48, list(range(16)) + [40])
    assert st2.compact() == 1 and _moves(eng2) == [(40, 16)]
    st2.suspend(h2[5])                                   # 16 running: the bound falls to 16 and column 16, a pending destination, is beyond it
    assert st2.compact() == 0 and _moves(eng2) == [(40, 16)]
    st2.step(4)
    assert st2.compact() == 1 and _moves(eng2)[-1] == (16, 5)
    st2.close()
    back = st.resume(state)
    got[back] = got.pop(handles[3])
    while st.busy():
        for h, (y, _) in st.step(64).items():
            got[h].append(y)
        st.compact()
    for c, h in ((3, back), (17, handles[17]), (30, handles[30]), (40, handles[40])):
        assert np.array_equal(np.concatenate(got[h]), 1000 * c + np.arange(1000)), c
    assert sorted(st._free) == list(range(48))
    st.close()
