"""GPU tests of a column's state as a value (`-m gpu`): utterances are moved between columns, saved, and resumed in
another column, at another counter, in another engine -- and their samples stay, bit for bit, those of column uid of the lockstep
nvw_set_features + nvw_set_selector_seed run (nvw_set_mel + nvw_generate_stream for mel utterances), fp16 and fp32, on the O(1)
inputs of the existing slot tests (where every sample depends on the whole network, so a ring slot in the wrong place shows)."""
import numpy as np
import pytest
import torch

import condgen
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.slots import SlotStream
from test_slots_gpu import FAMILIES, SEED, _edge, _engine, _lockstep, _synth
from test_slots_mel_gpu import _mel_engine, _mel_inputs, _mel_lockstep
from test_slots_state_cpu import HEADER_BYTES, schedule, to_canonical

pytestmark = pytest.mark.gpu


class Run:
    """A slot session driven by hand: columns -> utterances, samples collected per start (key = order of start) across moves,
    suspends and resumes -- also across engines: `into` shares the collection."""

    def __init__(self, e, xg, window=None, into=None, melg=None, stride=None):
        self.e, self.xg, self.melg, self.stride = e, xg, melg, stride
        self.cols = {}                    # column -> [key, uid, next local sample, length]
        self.got = into.got if into else {}
        self.uid_of = into.uid_of if into else {}
        self.moves = 0
        if window:
            e.slotsBegin(window)

    def start(self, col, uid, n=None):
        n = n or self.xg[uid].size(1)
        self.e.slotStart(col, self.xg[uid], uid, n)
        key = len(self.got)
        self.got[key], self.uid_of[key] = [], uid
        self.cols[col] = [key, uid, 0, n, "x"]
        return key

    def start_mel(self, col, uid, frames, final=True, total=None):
        self.e.slotStartMel(col, self.melg[uid], uid, frames, final)
        key = len(self.got)
        self.got[key], self.uid_of[key] = [], uid
        self.cols[col] = [key, uid, 0, (total or frames) * self.stride, "mel"]
        return key

    def move(self, a, b):
        self.e.slotMove(a, b)
        self.cols[b] = self.cols.pop(a)
        self.moves += 1

    def save(self, col):
        blob, done = self.e.slotSave(col)
        assert done == self.cols[col][2], (done, self.cols[col])
        return blob

    def suspend(self, col):
        blob = self.save(col)
        self.e.slotStop(col)
        return blob, self.cols.pop(col)

    def resume(self, col, blob, rec, frames=None, final=True):
        if rec[4] == "x":
            self.e.slotResume(col, blob, self.xg[rec[1]], rec[3])
        else:
            self.e.slotResumeMel(col, blob, self.melg[rec[1]], frames if frames is not None else rec[3] // self.stride, final)
        self.cols[col] = rec

    def step(self, c):
        y = np.full((self.e.maxBatch, c), -1, dtype=np.int32)
        assert self.e.slotsStep(c, y)
        for col in list(self.cols):
            rec = self.cols[col]
            k = min(c, rec[3] - rec[2])
            self.got[rec[0]].append(y[col, :k])
            rec[2] += k
            if rec[2] == rec[3]:
                self.e.slotStop(col)
                del self.cols[col]

    def check(self, y_lock, what, only=None):
        for key, parts in self.got.items():
            if only is not None and key not in only:
                continue
            y = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
            uid = self.uid_of[key]
            bad = np.nonzero(y != y_lock[uid, :len(y)])[0]
            assert bad.size == 0, "%s: start %d (utterance %d, %d samples) differs from its lockstep column first at sample %d" % (
                what, key, uid, len(y), bad[0])


def _finish(r, c=13):
    while r.cols:
        r.step(c)


# ---- move ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(16, "wg"), (16, "wg2"), (16, "wg3"), (32, "wg"), (32, "wg2")])
def test_moved_utterances_and_their_neighbours_equal_their_lockstep_columns(precision, mode):
    """C3, 40 columns (three tiles; one, two and three tiles per workgroup; the fp16 one-tile launch keeps its short-dilation ring
    slots in LDS).  Utterances move mid-run across tiles and within a tile, three in one step; a new utterance starts in a move's
    source column in the same step; one moves into a column whose stop is still pending.  Source and destination tiles are full of
    other utterances, which must not notice."""
    case, m, x, w, Lh, t = _edge(precision, N=96, B=8)
    s = case.shape
    y_lock = _lockstep(case, t, precision, mode, x, w, m["cond_b"])
    xg = torch.from_numpy(x).cuda()
    e = _engine(case, t, precision, mode, w, m["cond_b"], 40)
    r = Run(e, xg, 64)
    if precision == 16 and mode == "wg":
        assert "LR=1" in e.kernelInfo(), e.kernelInfo()
    for col, uid in {0: 0, 5: 1, 17: 2, 18: 3, 33: 4, 39: 5, 21: 6, 2: 7, 32: 1, 34: 2, 16: 3, 1: 4, 38: 0}.items():
        r.start(col, uid, 96 if col != 5 else 22)
    r.step(7)
    r.step(1)
    r.step(7)                                 # counter 15: odd
    r.move(39, 6)                             # across tiles
    r.move(33, 20)                            # across tiles
    r.move(17, 19)                            # within a tile
    late = r.start(39, 6, 50)                 # a move's source takes a new utterance in the same step
    r.step(7)                                 # the utterance of column 5 (22 samples) ends here: its stop is pending ...
    assert 5 not in r.cols
    r.move(21, 5)                             # ... when another moves in
    r.step(64)
    r.move(6, 39 if 39 not in r.cols else 37)
    r.move(5, 23)
    r.step(1)
    _finish(r)
    e.close()
    assert r.moves == 6 and len(r.got[late]) > 0
    r.check(y_lock, "fp%d/%s moves" % (precision, mode))


def _mel_setup(precision):
    cc = condgen.COND_BY_NAME["cond_C3_B16"]
    case, m, mel, up_w, w, t = _mel_inputs(cc, precision)
    y_lock = _mel_lockstep(case, t, precision, "wg", mel, w, m, up_w, cc.stride)
    return cc, case, m, up_w, w, t, y_lock, torch.from_numpy(mel).cuda()


def test_mel_columns_whole_and_streamed_move_save_and_resume():
    """Final mel columns and a streamed one (frames still arriving) move across tiles; the streamed one is
    extended in its new column, suspended, and resumed in another column with more frames: all equal the lockstep mel run."""
    cc, case, m, up_w, w, t, y_lock, melg = _mel_setup(16)
    s, stride = case.shape, cc.stride
    frames = s.N // stride
    e = _mel_engine(case, t, 16, "wg", w, m, up_w, stride, 36)
    r = Run(e, None, 64, melg=melg, stride=stride)
    r.start_mel(35, 3, frames)
    r.start_mel(2, 4, frames)
    k = r.start_mel(20, 5, 5, final=False, total=frames)          # 5 frames so far
    r.step(7)
    r.move(35, 1)
    r.move(20, 17)
    assert e.slotsHeadroom() == 5 * stride - 7
    e.slotMelFrames(17, 9)                                         # announced after the move was queued: reaches the new column
    r.step(9)
    r.move(17, 33)
    r.step(min(e.slotsHeadroom(), 11))
    blob, rec = r.suspend(33)
    r.step(5)                                                      # the others go on
    with pytest.raises(ValueError):
        e.slotResumeMel(4, blob, melg[5], rec[2] // stride, True)    # final with done >= frames x stride
    r.resume(4, blob, rec, frames=12, final=False)
    assert e.slotsHeadroom() == 12 * stride - rec[2]               # counted from done, before the resume is applied
    r.step(min(e.slotsHeadroom(), 8))
    e.slotMelFrames(4, frames, True)
    _finish(r)
    e.close()
    assert r.moves == 3 and len(np.concatenate(r.got[k])) == s.N
    r.check(y_lock, "mel moves")


# ---- canonical form --------------------------------------------------------------------------------------------------------------

def _payload(blob, slots):
    return blob.cpu().numpy()[HEADER_BYTES:].reshape(slots, -1)


@pytest.mark.parametrize("precision", [16, 32])
def test_blobs_of_one_utterance_from_two_columns_and_counters_are_byte_identical(precision):
    """The same utterance saved at the same `done` from column 3 (joined at counter 0) and column 21 (joined at counter 7: an odd
    difference, a non-trivial rotation for every d > 1) gives the same bytes -- with done = 50 > the largest dilation (32) and with
    done = 9 < it (slots never written stay zero under the rotation).  The header says what it should, and the payload of the
    column joined at counter 0 is its own canonical form (the numpy restatement with start 0 is the identity)."""
    case, m, x, w, Lh, t = _edge(precision, N=96, B=8)
    s = case.shape
    xg = torch.from_numpy(x).cuda()
    e = _engine(case, t, precision, "wg", w, m["cond_b"], 24)
    sch = schedule(s.L, s.maxD)
    slots = sum(d for _, d in sch)
    assert e.slotStateBytes() == HEADER_BYTES + slots * s.R * (2 if precision == 16 else 4)      # R elements of every ring slot
    for done in (50, 9):
        r = Run(e, xg, 64)
        r.start(3, 2)
        r.start(4, 5)
        r.step(7)
        r.start(21, 2)
        r.step(done - 7)
        a = r.save(3)
        r.step(7)
        b = r.save(21)
        torch.cuda.synchronize()
        assert torch.equal(a, b), "done = %d: the blob depends on the column or the join step" % done
        hdr = a.cpu().numpy()[:HEADER_BYTES].view(np.int32)
        assert list(hdr[2:8]) == [precision, s.R, s.L, s.maxD, done, 2], hdr
        pa = _payload(a, slots)
        assert pa.any() and np.array_equal(to_canonical(pa, s.L, s.maxD, 0), pa)
        if done == 9:                       # layers with d > 9: slots 9 .. d - 1 were never written
            for off, d in sch:
                assert not pa[off + done:off + d].any() and pa[off:off + min(d, done)].any(), (off, d)
        other = r.save(4)
        assert not torch.equal(other, a)
        _finish(r)
        e.slotsEnd()
    e.close()


# ---- save / resume -----------------------------------------------------------------------------------------------------------------

RESUME_SHAPES = [("edge", 16, "wg"), ("edge", 32, "wg"), ("edge", 16, "wg2"), ("edge", 16, "wg3"), ("C2_maxD512_W512", 16, "wg"),
                 ("oddL7", 16, "wg"), ("oddL7", 32, "wg2"), ("C1_R32", 16, "wg"), ("C4_R128_L30", 16, "wg"), ("C4_R128_L30", 32, "wg")]


@pytest.mark.parametrize("name,precision,mode", RESUME_SHAPES)
def test_suspended_utterances_resume_elsewhere_later_and_in_another_engine(name, precision, mode):
    """At every shape family of the ring (C3; maxD 512 on a window of 512; an odd layer count; R = 32 and R = 128; one to three
    tiles per workgroup): an utterance is suspended mid-run, its column and tile go on with other utterances, and it resumes in a
    different column (another tile) after an odd number of samples that crosses a window wrap -- and, from the same blob, in a
    second engine of the same weights and seed at a negative start.  What was delivered before plus the continuation equals the
    lockstep column.  A column that was saved but not stopped is unaffected by the save."""
    if name == "edge":
        case, m, x, w, Lh, t = _edge(precision, N=96, B=8)
        window = 64
    else:
        shape, window, seed = FAMILIES[name]
        case, m, x, w, Lh, t = _synth(name, shape, precision, seed)
    s = case.shape
    y_lock = _lockstep(case, t, precision, mode, x, w, m["cond_b"])
    xg = torch.from_numpy(x).cuda()
    columns = 36
    e = _engine(case, t, precision, mode, w, m["cond_b"], columns)
    r = Run(e, xg, window)
    n1 = max(3, min(s.N // 3, window // 2 + 1)) | 1                 # samples before the suspend (odd)
    gap = window - 1 if (window - 1) % 2 else window - 2            # odd, and with n1 beyond the window: the resume follows a wrap
    gap = min(gap, window)
    a = r.start(35, 0)
    kept = r.start(34, 1)
    r.start(2, 2)
    r.step(n1)
    keep_blob = r.save(34)                                          # saved, not stopped: goes on
    blob, rec = r.suspend(35)
    again = r.start(35, 3)                                          # its column and tile go on with other utterances
    for c in (gap // 2, gap - gap // 2):
        r.step(c)
    assert (n1 + gap) > window and gap % 2 == 1
    r.resume(17, blob, rec)
    _finish(r, max(1, min(window, 13)))
    r.check(y_lock, "%s fp%d/%s resume" % (name, precision, mode))
    assert len(np.concatenate(r.got[a])) == s.N and len(np.concatenate(r.got[kept])) == s.N and again in r.got
    e.slotsEnd()
    # a second engine built from the same weights and seed: the continuation from the same blob, and from the kept column's
    e2 = _engine(case, t, precision, mode, w, m["cond_b"], 20)
    r2 = Run(e2, xg, window)
    r2.start(0, 4)
    r2.step(4)
    ka, kb = len(r2.got), len(r2.got) + 1
    r2.got[ka], r2.uid_of[ka] = [y_lock[0, :n1]], 0
    r2.got[kb], r2.uid_of[kb] = [y_lock[1, :n1]], 1
    r2.resume(19, blob, [ka, 0, n1, s.N, "x"])                     # start' = 4 - n1 < 0
    r2.resume(3, keep_blob, [kb, 1, n1, s.N, "x"])
    _finish(r2, max(1, min(window, 7)))
    r2.check(y_lock, "%s fp%d/%s resume in a second engine" % (name, precision, mode))
    assert len(np.concatenate(r2.got[ka])) == s.N
    e2.close()
    e.close()


def test_a_resume_without_the_rotation_gives_other_samples():
    """Negative control: the blob pre-rotated by the numpy restatement so that the load's rotation cancels -- the ring then holds
    the canonical bytes verbatim at a start that is odd, i.e. a resume that skipped the rotation -- continues with different
    samples, while the untouched blob continues with the lockstep column's.  So these tests can see a wrong rotation."""
    case, m, x, w, Lh, t = _edge(16, N=96, B=8)
    s = case.shape
    y_lock = _lockstep(case, t, 16, "wg", x, w, m["cond_b"])
    xg = torch.from_numpy(x).cuda()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], 4)
    r = Run(e, xg, 64)
    r.start(0, 2)
    r.step(40)
    blob, rec = r.suspend(0)
    r.step(7)                                                       # resume at counter 47: start' = 7
    slots = sum(d for _, d in schedule(s.L, s.maxD))
    raw = blob.cpu().numpy().copy()
    raw[HEADER_BYTES:] = to_canonical(_payload(blob, slots), s.L, s.maxD, 47 - 40).reshape(-1)
    skipped = torch.from_numpy(raw).cuda()
    good = r.got[rec[0]]
    r.resume(1, blob, rec)
    bad_key = len(r.got)
    r.got[bad_key], r.uid_of[bad_key] = [], 2
    r.resume(2, skipped, [bad_key, 2, 40, 96, "x"])
    _finish(r)
    e.close()
    r.check(y_lock, "the untouched blob", only=[rec[0]])
    wrong = np.concatenate(r.got[bad_key])
    assert len(wrong) == 56 and not np.array_equal(wrong, y_lock[2, 40:]), "a resume without the rotation went unnoticed"
    assert len(np.concatenate(good)) == 96


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_return_zero_or_minus_one_and_change_nothing():
    case, m, x, w, Lh, t = _edge(16, N=96, B=8)
    s = case.shape
    y_lock = _lockstep(case, t, 16, "wg", x, w, m["cond_b"])
    xg = torch.from_numpy(x).cuda()
    x0 = xg[0]
    e = _engine(case, t, 16, "wg", w, m["cond_b"], 20)
    nbytes = e.slotStateBytes()
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    mv, sv = lib.nvw_slot_move, lib.nvw_slot_save

    def res(slot, state, xx=x0, length=96, prec=32):
        return lib.nvw_slot_resume(e._h, slot, state.data_ptr(), xx.data_ptr(), prec, xx.stride(0), xx.stride(1), length)

    assert mv(e._h, 0, 1) == 0 and sv(e._h, 0, buf.data_ptr(), None) == -1 and res(0, buf) == 0      # not in slot mode
    r = Run(e, xg, 64)
    r.start(0, 0)
    r.start(17, 1)
    r.start(10, 3)                                                  # runs plainly throughout: no pending start, no move
    r.start(12, 4)
    r.step(9)
    good = r.save(0)
    r.start(3, 2)                                                   # a pending start on 3
    r.move(17, 5)                                                   # a pending move 17 -> 5
    blob12, rec12 = r.suspend(12)
    r.resume(13, blob12, rec12)                                     # a pending resume on 13
    refused = [mv(e._h, -1, 1), mv(e._h, 0, 20), mv(e._h, 0, 0), mv(e._h, 1, 2),      # out of range, from == to, an idle source
               mv(e._h, 3, 4),                                      # a source with a pending start
               mv(e._h, 0, 3),                                      # a destination with a pending start
               mv(e._h, 0, 5), mv(e._h, 0, 17),                     # destinations that are endpoints of a pending move
               mv(e._h, 5, 6),                                      # a source that is an endpoint of a pending move
               mv(e._h, 0, 10),                                     # a destination that simply holds a running utterance
               mv(e._h, 13, 14), mv(e._h, 0, 13),                   # a source / a destination with a pending resume
               sv(e._h, 13, buf.data_ptr(), None) + 1,              # a save of a column with a pending resume
               res(5, good), lib.nvw_slot_start(e._h, 5, x0.data_ptr(), 32, x0.stride(0), x0.stride(1), 96, 7),   # into a pending move's destination
               sv(e._h, 3, buf.data_ptr(), None) + 1, sv(e._h, 5, buf.data_ptr(), None) + 1, sv(e._h, 17, buf.data_ptr(), None) + 1,
               sv(e._h, 9, buf.data_ptr(), None) + 1, sv(e._h, 20, buf.data_ptr(), None) + 1, sv(e._h, 0, None, None) + 1,
               sv(e._h, 0, buf.data_ptr() + 4, None) + 1]
    assert refused == [0] * len(refused), refused
    # blobs: a corrupted magic, another layout version, the other precision's, another shape's, done >= length; what slotStart refuses
    raw = good.cpu().numpy()
    def variant(word, value):
        v = raw.copy()
        v[:HEADER_BYTES].view(np.int32)[word] = value
        return torch.from_numpy(v).cuda()
    e32 = _engine(case, t, 32, "wg", w, m["cond_b"], 4)
    other_precision = torch.zeros(e32.slotStateBytes(), dtype=torch.uint8, device="cuda")
    r32 = Run(e32, xg, 64)
    r32.start(0, 0)
    r32.step(9)
    assert lib.nvw_slot_save(e32._h, 0, other_precision.data_ptr(), None) == 9
    torch.cuda.synchronize()
    host = np.zeros((80, 96), dtype=np.float32)
    bad = [res(8, variant(0, 0x12345678)), res(8, variant(1, 99)), res(8, other_precision[:nbytes].contiguous()), res(8, variant(3, 128)),
           res(8, variant(4, s.L + 1)), res(8, variant(5, 2 * s.maxD)), res(8, good, length=9), res(8, good, length=5),
           res(-1, good), res(20, good), res(8, good, prec=8), res(8, buf),
           lib.nvw_slot_resume(e._h, 8, good.data_ptr(), host.ctypes.data, 32, 96, 1, 96),
           lib.nvw_slot_resume(e._h, 8, raw.ctypes.data, x0.data_ptr(), 32, x0.stride(0), x0.stride(1), 96),
           lib.nvw_slot_resume_mel(e._h, 8, good.data_ptr(), x0.data_ptr(), 32, x0.stride(0), x0.stride(1), 10, 1)]      # no upsampling set
    assert bad == [0] * len(bad), bad
    assert lib.nvw_slot_resume(e32._h, 1, good.data_ptr(), x0.data_ptr(), 32, x0.stride(0), x0.stride(1), 96) == 0       # fp16 blob, fp32 engine
    e32.close()
    # nothing changed: column 8 stayed idle, and everything that runs equals its lockstep column
    assert sv(e._h, 8, buf.data_ptr(), None) == -1 and sv(e._h, 14, buf.data_ptr(), None) == -1 and e.slotsHeadroom() == 64
    r.step(5)
    _finish(r)
    e.close()
    r.check(y_lock, "after the refusals")
    assert len(r.got) == 5 and all(len(np.concatenate(v)) == 96 for v in r.got.values())


# ---- SlotStream(compact=True), and lockstep afterwards ------------------------------------------------------------------------

def _wgs(info):
    return int(info.split("wgs=")[1].split()[0])


@pytest.mark.parametrize("compact", [True, False])
def test_slot_stream_compaction_shrinks_the_launch_and_keeps_every_request(compact):
    """48 requests of mixed lengths on 48 columns, one tile per workgroup: every request equals its lockstep column, with and
    without compaction; once the short ones have finished, a compacting stream launches ceil(running / 16) tiles -- fewer than
    before, and fewer than the stream that does not compact, whose survivors keep all three tiles launched."""
    case, m, x, w, Lh, t = _edge(16, N=96, B=8)
    s = case.shape
    y_lock = _lockstep(case, t, 16, "wg", x, w, m["cond_b"])
    xg = torch.from_numpy(x).cuda()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], 48)
    st = SlotStream(e, 64, compact=compact)
    long_cols = (7, 20, 33, 47, 46)
    handles = {}
    for c in range(48):
        n = 96 if c in long_cols else 10 + c % 7
        handles[st.submit(xg[c % 8][:, :n], uid=c % 8)] = (c % 8, n)
    extra = st.submit(xg[3][:, :40], uid=3)                          # waits; admitted into the packed front
    handles[extra] = (3, 40)
    out = {h: [] for h in handles}
    tiles = []
    while st.busy():
        for h, (yy, _) in st.step(9).items():
            out[h].append(yy)
        st.finished()
        cols = st.running().values()
        if cols:
            tiles.append((_wgs(e.kernelInfo(max(cols) + 1)), len(cols)))
    for h, (uid, n) in handles.items():
        assert np.array_equal(np.concatenate(out[h]), y_lock[uid, :n]), "request %d (utterance %d)" % (h, uid)
    assert tiles[0][0] == 3
    late = [(wg, n) for wg, n in tiles[3:]]                          # the short requests (<= 16 samples) are gone after two steps
    assert late and all(n <= 6 for _, n in late)
    if compact:
        assert all(wg == (n + 15) // 16 == 1 for wg, n in late), late
        assert st.running() == {} and extra in out
    else:
        assert late[0][0] == 3, late                                 # column 47 still runs: three tiles
    st.close()
    e.close()


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2")])
def test_lockstep_after_a_session_that_moved_and_resumed_starts_from_clean_rings(precision, mode):
    """maxBatch 200: a slot session that moves an utterance into tile 12 and resumes one in tile 9 -- tiles no launch of the
    session would otherwise have reached after them --, slotsEnd, then a lockstep batch of 200: equal to a fresh engine's."""
    B = 200
    case, m, x, w, Lh, t = _edge(precision, N=64, B=B)
    s = case.shape
    xg = torch.from_numpy(x).cuda()

    def engine():
        e = _engine(case, t, precision, mode, w, m["cond_b"], B)
        e.setFeatures(xg)
        return e

    e = engine()
    r = Run(e, xg, 64)
    r.start(0, 0)
    r.start(17, 17)
    r.step(21)
    blob, rec = r.suspend(17)
    r.move(0, 199)
    r.step(8)
    r.resume(150, blob, rec)
    r.step(64)
    e.slotsEnd()
    e.setFeatures(xg)
    y = np.full((B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, B, y, 1, False)
    e.synchronize()
    e.close()
    f = engine()
    want = np.full((B, s.N), -1, dtype=np.int32)
    assert f.run(s.N, B, want, 1, False)
    f.synchronize()
    f.close()
    r.check(want, "the session itself")
    bad = np.nonzero((y != want).any(axis=1))[0]
    assert bad.size == 0, "columns %s differ from a fresh engine's run after a slot session with moves and resumes" % bad[:10]
