"""CPU tests of slot mode (continuous batching; no GPU): the ABI revision and entry points, the window's wrap split, the SlotStream
bookkeeping against a fake engine, and the slot kernels in the shipped code object."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_code_objects_cpu import BUILD, kernel_table

SLOT_SYMBOLS = ("nvw_slots_begin", "nvw_slot_start", "nvw_slot_stop", "nvw_slots_step", "nvw_slots_end")


def test_abi_7_exports_the_slot_entries():
    from nv_wavenet_amd import _lib
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SLOT_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(BUILD), "..", "..", "include", "nv_wavenet_c.h")).read()
    assert "#define NVW_ABI_VERSION 7" in header
    for name in SLOT_SYMBOLS:
        assert name + "(" in header, name


def test_window_pieces_split_where_the_rows_wrap():
    from nv_wavenet_amd.slots import window_pieces
    assert window_pieces(0, 64, 64) == [(0, 64)]
    assert window_pieces(64, 64, 64) == [(0, 64)]
    assert window_pieces(7, 1, 64) == [(7, 1)]
    assert window_pieces(60, 7, 64) == [(60, 4), (0, 3)]
    assert window_pieces(63, 64, 64) == [(63, 1), (0, 63)]
    assert window_pieces(5 * 64 + 57, 7, 64) == [(57, 7)]
    assert window_pieces(5 * 64 + 58, 7, 64) == [(58, 6), (0, 1)]
    for counter in range(0, 300, 13):
        for count in (1, 7, 31, 64):
            p = window_pieces(counter, count, 64)
            rows = [r for (t0, n) in p for r in range(t0, t0 + n)]
            assert rows == [(counter + i) % 64 for i in range(count)]
            assert all(0 <= t0 and t0 + n <= 64 for t0, n in p)
    with pytest.raises(AssertionError):
        window_pieces(0, 65, 64)


class FakeEngine:
    """Stands in for WavenetEngine in slot mode: sample k of the utterance with uid u is 1000 u + k, its PCM k mod 1000."""

    def __init__(self, columns):
        self.maxBatch = columns
        self.calls = []
        self.active = {}
        self.t = 0

    def slotsBegin(self, window):
        self.calls.append(("begin", window))

    def slotStart(self, col, x, uid):
        assert 0 <= col < self.maxBatch
        self.calls.append(("start", col, uid))
        self.active[col] = (uid, self.t)

    def slotStop(self, col):
        self.calls.append(("stop", col))
        self.active.pop(col)

    def slotsStep(self, count, y, pcm):
        y[:] = -1
        for col, (uid, t0) in self.active.items():
            y[col] = 1000 * uid + (self.t - t0) + np.arange(count)
            if pcm is not None:
                pcm[col] = y[col] % 1000
        self.t += count
        return True

    def slotsEnd(self):
        self.calls.append(("end",))


def test_slot_stream_fifo_lowest_first_reuse_and_one_time_completion():
    from nv_wavenet_amd.slots import SlotStream
    eng = FakeEngine(3)
    st = SlotStream(eng, 64)
    lengths = [10, 3, 10, 5, 1, 20, 4]
    handles = [st.submit(torch.zeros(80, n)) for n in lengths]
    h_uid = st.submit(torch.zeros(80, 2), uid=42)
    h_next = st.submit(torch.zeros(80, 2))
    assert st.waiting() == 9
    got = {h: [] for h in handles + [h_uid, h_next]}
    finished = []
    steps = 0
    while st.busy():
        for h, (y, pcm) in st.step(4).items():
            got[h].append(y)
            assert np.array_equal(pcm, y % 1000)
        finished += st.finished()
        steps += 1
        assert steps < 100
    # every request once, in order of completion; nothing comes back twice
    assert sorted(finished) == sorted(got) and len(finished) == len(set(finished))
    assert st.finished() == []
    # samples: uid 0, 1, 2, ... by submission, explicit uids kept, the next default above them
    uids = {h: i for i, h in enumerate(handles)}
    uids.update({h_uid: 42, h_next: 43})
    want_len = dict(zip(handles, lengths))
    want_len.update({h_uid: 2, h_next: 2})
    for h, pieces in got.items():
        assert np.array_equal(np.concatenate(pieces), 1000 * uids[h] + np.arange(want_len[h])), h
    # FIFO admission, lowest free column first
    starts = [c for c in eng.calls if c[0] == "start"]
    assert [s[2] for s in starts] == [0, 1, 2, 3, 4, 5, 6, 42, 43]
    assert [s[1] for s in starts[:3]] == [0, 1, 2]
    # step 1 (4 samples): uid 1 (3 samples) ends in column 1 -> uid 3 takes column 1 at step 2
    assert starts[3][1] == 1
    # every start of a column follows the stop of its previous utterance; every utterance is stopped
    owner = {}
    for c in eng.calls:
        if c[0] == "start":
            assert c[1] not in owner
            owner[c[1]] = c[2]
        elif c[0] == "stop":
            owner.pop(c[1])
    assert owner == {}
    st.close()
    assert eng.calls[-1] == ("end",)


def test_slot_stream_reuses_the_lowest_free_column():
    from nv_wavenet_amd.slots import SlotStream
    eng = FakeEngine(4)
    st = SlotStream(eng, 64)
    for n in (8, 4, 8, 4, 1, 1):          # columns 1 and 3 free after the first step of 4 samples
        st.submit(torch.zeros(80, n))
    st.step(4)
    assert sorted(st.running().values()) == [0, 2]
    st.step(4)                             # the two waiting requests take columns 1 and 3, lowest first, in FIFO order
    starts = [c for c in eng.calls if c[0] == "start"]
    assert [(s[1], s[2]) for s in starts[4:]] == [(1, 4), (3, 5)]
    st.close()


def test_slot_kernels_are_in_the_shipped_code_object_and_use_no_scratch():
    obj = os.path.join(BUILD, "slots.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = kernel_table(obj)
    names = {r[0].replace(" ", "").split("(")[0]: r for r in rows}
    for name in ("wn::slot_reset_kernel", "wn::slot_feed_kernel<true>", "wn::slot_feed_kernel<false>"):
        assert name in names, (name, sorted(names))
        _, vgpr, agpr, sgpr, scratch, spill = names[name]
        assert scratch == 0 and spill == 0, names[name]
        assert vgpr <= 64, names[name]          # (a memory-bound kernel: occupancy, not registers)


def test_test_library_keeps_its_copy_of_the_slot_launchers_to_itself():
    """tests/cpp/wn_primitives.hip compiles the product's slots.hip for the kernel-level tests (test_slot_kernels_gpu.py).  Its
    copy of wn::slots_feed / wn::slots_reset must not be exported -- a process that loads both libraries would otherwise have two
    definitions of one symbol -- while the test entries are."""
    import shutil
    import subprocess
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "libwn_primitives.so")
    if not os.path.exists(path):
        pytest.skip("build the test library first (__graft_entry__.build())")
    nm = shutil.which("llvm-nm", path="/opt/rocm/llvm/bin") or shutil.which("nm")
    assert nm, "no nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", path], text=True)
    exported = [line.split()[-1] for line in out.splitlines() if line.strip()]
    for name in ("wnp_slot_feed", "wnp_slot_reset", "wnp_slot_desc_bytes", "wnp_slot_update_bytes"):
        assert name in exported, name
    leaked = [s for s in exported if "slots_feed" in s or "slots_reset" in s or "slot_feed_kernel" in s or "slot_reset_kernel" in s]
    assert not leaked, leaked
