"""GPU tests of lists of columns saved and resumed (`-m gpu`): nvw_slots_save_list writes, with one launch, the bytes
nvw_slot_save writes per column -- into device or pinned memory, nothing outside the blobs --; nvw_slots_resume_list continues
utterances from such rows in other columns, at another counter, in another engine, and their samples stay those of column uid of
the lockstep run; a refusal of either changes nothing; SlotStream.drain empties a stream into states that survive to_bytes /
from_bytes and finish on another stream.  The small cases run on the R = 32 family (one fragment per ring slot in fp16, two in fp32;
dilations 1 2 4 8 1 2 4 8, window 16 = twice the largest) and on the odd-layer R = 64 one (1 2 4 1 2 4 1, window 8); the cases with
mel columns on the C3 conditioning record the mel tests use."""
import functools

import numpy as np
import pytest
import torch

import condgen
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import SLOT_RESUME_REQ, SLOT_SAVED
from nv_wavenet_amd.slots import SlotState, SlotStream
from test_features_gpu import _cond_inputs
from test_slots_gpu import FAMILIES, _engine, _lockstep, _synth
from test_slots_mel_gpu import _mel_engine, _mel_inputs, _mel_lockstep
from test_slots_state_cpu import HEADER_BYTES
from test_slots_state_gpu import Run, _finish

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 256
WINDOWS = {"C1_R32": 16, "oddL7": 8}          # twice the largest dilation (8, 4)


@functools.lru_cache(maxsize=None)
def _family(name, precision):
    """(case, model, features x [B][n_cond][N], cond weight, network, window, lockstep samples y [B][N]) -- computed once."""
    shape, _, seed = FAMILIES[name]
    case, m, x, w, Lh, t = _synth(name, shape, precision, seed)
    return case, m, x, w, t, WINDOWS[name], _lockstep(case, t, precision, "wg", x, w, m["cond_b"])


@functools.lru_cache(maxsize=None)
def _c3(precision):
    """The C3 conditioning record with its features and its mel frames, and the lockstep samples of both -- computed once."""
    cc = condgen.COND_BY_NAME["cond_C3_B16"]
    case, m, mel, up_w, w, t = _mel_inputs(cc, precision)
    _, _, x, wx, _ = _cond_inputs(cc, half=precision == 16)
    assert np.array_equal(w, wx)
    y_mel = _mel_lockstep(case, t, precision, "wg", mel, w, m, up_w, cc.stride)
    y_feat = _lockstep(case, t, precision, "wg", x, w, m["cond_b"])
    return cc, case, m, mel, up_w, w, t, x, y_mel, y_feat


def _buffer(nbytes, pinned):
    """GUARD + nbytes + GUARD bytes of canaries, on the GPU or pinned."""
    total = GUARD + nbytes + GUARD
    buf = torch.empty(total, dtype=torch.uint8, pin_memory=True) if pinned else torch.empty(total, dtype=torch.uint8, device="cuda")
    buf.fill_(CANARY)
    torch.cuda.synchronize()
    return buf


def _host(buf):
    torch.cuda.synchronize()
    return buf.cpu().numpy() if buf.is_cuda else buf.numpy()


def _save_list(e, slots, dst, stride, n=None):
    """nvw_slots_save_list, raw: (return value, saved)."""
    idx = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    saved = np.zeros(max(len(idx), 1), dtype=SLOT_SAVED)
    return lib.nvw_slots_save_list(e._h, idx.ctypes.data, len(idx) if n is None else n, dst, stride, saved.ctypes.data, None), saved


def _resume_list(e, reqs, states, stride):
    """nvw_slots_resume_list, raw: reqs = (slot, mel, source tensor, length | frames, final)."""
    arr = np.zeros(len(reqs), dtype=SLOT_RESUME_REQ)
    for i, (slot, mel, x, count, final) in enumerate(reqs):
        arr[i] = (slot, mel, x.data_ptr(), 32 if x.dtype == torch.float32 else 16, x.stride(0), x.stride(1), count, final)
    return lib.nvw_slots_resume_list(e._h, arr.ctypes.data, len(reqs), states, stride)


# ---- 1. byte identity with the single save -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,precision,pinned", [("C1_R32", 16, False), ("C1_R32", 32, False), ("C1_R32", 16, True), ("oddL7", 16, False)])
def test_list_saved_blobs_equal_the_single_saves_byte_for_byte_and_nothing_else_is_written(name, precision, pinned):
    """Columns 0, 15, 16, 17 and the last of a ragged batch of 37 join at counters 1, 3, 5, 7, 9 and run past a window wrap.  One
    list save in non-ascending order with a stride 48 bytes above the blob size: every row equals nvw_slot_save of that column at
    the same counter; the canaries in front, behind and in every gap are intact; saved[] says what the headers say.  The columns
    go on and finish as their lockstep columns."""
    case, m, x, w, t, window, y_lock = _family(name, precision)
    s = case.shape
    xg = torch.from_numpy(x).cuda()
    e = _engine(case, t, precision, "wg", w, m["cond_b"], 37)
    r = Run(e, xg, window)
    for i, col in enumerate((0, 15, 16, 17, 36)):
        r.step(1 if i == 0 else 2)
        r.start(col, (3 * i + 1) % s.B)
    r.step(window // 2 + 2)
    counter = 9 + window // 2 + 2
    assert counter > window and counter - 1 < s.N
    order = [17, 0, 36, 16, 15]
    nbytes = e.slotStateBytes()
    stride = nbytes + 48
    single = {col: r.save(col) for col in order}
    buf = _buffer(len(order) * stride, pinned)
    got, saved = _save_list(e, order, buf.data_ptr() + GUARD, stride)
    assert got == len(order)
    raw = _host(buf)
    assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + len(order) * stride:] == CANARY).all(), "written outside the buffer"
    for i, col in enumerate(order):
        row = raw[GUARD + i * stride:GUARD + (i + 1) * stride]
        assert np.array_equal(row[:nbytes], single[col].cpu().numpy()), "row %d (column %d) differs from nvw_slot_save's blob" % (i, col)
        assert (row[nbytes:] == CANARY).all(), "the gap behind row %d was written" % i
        hdr = row[:HEADER_BYTES].view(np.uint32)
        assert (saved["slot"][i], saved["done"][i], saved["uid"][i], saved["mel"][i]) == (col, hdr[6], hdr[7], 0), (saved[i], hdr[:8])
        assert hdr[6] == counter - (1 + 2 * (0, 15, 16, 17, 36).index(col))
    # the Python entry: rows of one tensor, the same bytes
    blobs, saved2 = e.slotsSaveList(order, pinned=pinned)
    assert tuple(blobs.shape) == (len(order), nbytes) and blobs.is_pinned() == pinned and np.array_equal(saved2, saved[:len(order)])
    rows = _host(blobs)
    for i, col in enumerate(order):
        assert np.array_equal(rows[i], single[col].cpu().numpy()), (i, col)
    _finish(r, 5)
    e.close()
    r.check(y_lock, "%s fp%d after the list saves" % (name, precision))


# ---- 2. the second pass of the grid's y stride ---------------------------------------------------------------------------------------

def test_a_list_of_more_than_1024_columns_is_saved_in_one_launch():
    """1 040 running columns in one list (the grid's y is capped at 1 024: entries 1 024 .. 1 039 are a block's second pass): the
    rows below, at and above index 1 024 equal single saves, and every row equals the row of the same utterance elsewhere (the
    canonical form: eight utterances, 130 columns each)."""
    case, m, x, w, t, window, y_lock = _family("C1_R32", 16)
    s = case.shape
    xg = torch.from_numpy(x).cuda()
    n = 1040
    e = _engine(case, t, 16, "wg", w, m["cond_b"], n)
    e.slotsBegin(window)
    for col in range(n):
        e.slotStart(col, xg[col % s.B], col % s.B)
    assert e.slotsStep(5)
    order = list(range(n - 1, -1, -1))
    blobs, saved = e.slotsSaveList(order)
    rows = _host(blobs)
    assert list(saved["slot"]) == order and (saved["done"] == 5).all() and list(saved["uid"]) == [c % s.B for c in order]
    for i in (0, 1, 1022, 1023, 1024, 1025, 1039):
        blob, done = e.slotSave(order[i])
        assert done == 5 and np.array_equal(rows[i], blob.cpu().numpy()), "row %d (column %d)" % (i, order[i])
    first = {}
    for i, col in enumerate(order):
        ref = first.setdefault(col % s.B, i)
        assert np.array_equal(rows[i], rows[ref]), "row %d (column %d) differs from row %d of the same utterance" % (i, col, ref)
    assert len({rows[i].tobytes() for i in first.values()}) == s.B
    e.close()


# ---- 3. resume from a list, elsewhere ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,pinned", [(16, False), (16, True), (32, False), (32, True)])
def test_a_list_of_feature_and_mel_columns_resumes_elsewhere_in_another_engine(precision, pinned):
    """Two feature columns, a whole mel column and a streamed one, saved at done = 25, 12, 18 and 7 with one list, resume from its
    rows (device or pinned) in other columns of a second engine at another counter; the streamed one gets more frames there.
    What the first engine delivered plus what the second delivers equals each utterance's lockstep column."""
    cc, case, m, mel, up_w, w, t, x, y_mel, y_feat = _c3(precision)
    s, stride = case.shape, cc.stride
    frames = s.N // stride
    xg, melg = torch.from_numpy(x).cuda(), torch.from_numpy(mel).cuda()
    e = _mel_engine(case, t, precision, "wg", w, m, up_w, stride, 36)
    r = Run(e, xg, 64, melg=melg, stride=stride)
    f0 = r.start(35, 0)
    r.step(7)
    m0 = r.start_mel(20, 3, frames)
    r.step(6)
    f1 = r.start(3, 1)
    r.step(5)
    m1 = r.start_mel(17, 5, 5, final=False, total=frames)             # 5 frames so far
    assert e.slotsHeadroom() == 5 * stride
    r.step(7)                                                         # counter 25, odd
    cols = [17, 35, 20, 3]
    blobs, saved = e.slotsSaveList(cols, pinned=pinned)
    assert list(saved["done"]) == [7, 25, 18, 12] and list(saved["mel"]) == [1, 0, 1, 0] and list(saved["uid"]) == [5, 0, 3, 1]
    recs = [r.cols.pop(c) for c in cols]
    for c in cols:
        e.slotStop(c)
    torch.cuda.synchronize()                                          # (a pinned list is read in place: the save has completed)
    e2 = _mel_engine(case, t, precision, "wg", w, m, up_w, stride, 24)
    r2 = Run(e2, xg, 64, into=r, melg=melg, stride=stride)
    other = r2.start(2, 7)
    r2.step(4)                                                        # another counter: 4
    to = [9, 0, 23, 16]
    e2.slotsResumeList(to, blobs, [melg[5], xg[0], melg[3], xg[1]], [9, None, frames, None], [False, None, True, None])
    for c, rec in zip(to, recs):
        r2.cols[c] = rec
    again = None
    x0 = xg[0]
    if not pinned:                                                    # a single nvw_slot_resume takes a row of the list as well
        again = len(r.got)
        r.got[again], r.uid_of[again] = [y_feat[0, :25]], 0
        e2.slotResume(5, blobs[1], x0)
        r2.cols[5] = [again, 0, 25, s.N, "x"]
    else:                                                             # ... and keeps refusing host memory
        assert lib.nvw_slot_resume(e2._h, 5, blobs[1].data_ptr(), x0.data_ptr(), 32, x0.stride(0), x0.stride(1), s.N) == 0
    assert e2.slotsHeadroom() == 9 * stride - 7                       # the streamed column, counted from done
    r2.step(8)
    e2.slotMelFrames(9, frames, True)
    _finish(r2)
    e2.close()
    e.close()
    what = "fp%d %s list" % (precision, "pinned" if pinned else "device")
    r.check(y_feat, what, only=[k for k in (f0, f1, other, again) if k is not None])
    r.check(y_mel, what, only=[m0, m1])
    assert all(len(np.concatenate(r.got[k])) == s.N for k in (f0, f1, m0, m1)), {k: len(np.concatenate(v)) for k, v in r.got.items()}


# ---- 4. refusals change nothing ------------------------------------------------------------------------------------------------------

def test_refused_list_saves_and_resumes_change_nothing():
    case, m, x, w, t, window, y_lock = _family("C1_R32", 16)
    s = case.shape
    xg = torch.from_numpy(x).cuda()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], 20)
    nbytes = e.slotStateBytes()
    buf = _buffer(4 * nbytes, False)
    dst = buf.data_ptr() + GUARD
    assert _save_list(e, [0], dst, nbytes)[0] == -1                   # not in slot mode
    r = Run(e, xg, window)
    for col, uid in ((0, 0), (17, 1), (10, 3), (12, 4), (14, 5)):
        r.start(col, uid)
    r.step(9)
    r.start(3, 2)                                                     # a pending start on 3
    r.move(17, 5)                                                     # a pending move 17 -> 5
    pageable = np.full(4 * nbytes + 64, CANARY, dtype=np.uint8)
    host = pageable.ctypes.data + (-pageable.ctypes.data % 16)
    refused = [_save_list(e, [0, 10, 0], dst, nbytes)[0],             # a slot listed twice
               _save_list(e, [0, 9], dst, nbytes)[0],                 # an idle slot
               _save_list(e, [0, 3], dst, nbytes)[0],                 # a pending start
               _save_list(e, [10, 17], dst, nbytes)[0], _save_list(e, [5, 10], dst, nbytes)[0],      # the endpoints of a pending move
               _save_list(e, [0, 10], dst, nbytes, n=0)[0],           # n = 0
               _save_list(e, list(range(21)), dst, nbytes)[0],        # n above the batch
               _save_list(e, [0, 20], dst, nbytes)[0], _save_list(e, [-1, 0], dst, nbytes)[0],       # out of range
               _save_list(e, [0, 10], dst, nbytes - 16)[0],           # a stride below the blob size
               _save_list(e, [0, 10], dst, nbytes + 8)[0],            # a stride that is no multiple of 16
               _save_list(e, [0, 10], dst + 8, nbytes)[0],            # a misaligned destination
               _save_list(e, [0, 10], None, nbytes)[0],
               _save_list(e, [0, 10], host, nbytes)[0]]               # pageable host memory
    assert refused == [-1] * len(refused), refused
    assert (_host(buf) == CANARY).all() and (pageable == CANARY).all(), "a refused list save wrote something"
    r.step(5)                                                         # the pending start and move are applied; everything goes on
    # good blobs of three columns, which then leave their columns; 3, 5 and 14 go on
    blobs, saved = e.slotsSaveList([0, 10, 12])
    recs = [r.cols.pop(c) for c in (0, 10, 12)]
    for c in (0, 10, 12):
        e.slotStop(c)
    done = int(saved["done"][0])
    assert list(saved["done"]) == [done] * 3 and done == 14
    raw = _host(blobs)

    def variant(row, word, value):
        v = raw.copy()
        v[row, :HEADER_BYTES].view(np.int32)[word] = value
        return torch.from_numpy(v).cuda()

    src = [xg[0], xg[3], xg[4]]
    good = lambda slots, lengths=(s.N,) * 3: [(c, 0, xx, n, 0) for c, xx, n in zip(slots, src, lengths)]
    magic, other_precision = variant(1, 0, 0x12345678), variant(2, 2, 32)
    bad = [_resume_list(e, good((6, 7, 8)), magic.data_ptr(), nbytes),                           # wrong magic in the middle one
           _resume_list(e, good((6, 7, 8)), other_precision.data_ptr(), nbytes),                 # another precision in the last
           _resume_list(e, good((6, 7, 8), (s.N, done, s.N)), blobs.data_ptr(), nbytes),         # done >= length
           _resume_list(e, good((6, 3, 8)), blobs.data_ptr(), nbytes),                           # an occupied slot
           _resume_list(e, good((6, 7, 6)), blobs.data_ptr(), nbytes),                           # one slot named twice
           _resume_list(e, good((6, 7, 20)), blobs.data_ptr(), nbytes),                          # a slot out of range
           _resume_list(e, good((6, 7, 8)), blobs.data_ptr(), nbytes - 16),                      # a bad stride
           _resume_list(e, good((6, 7, 8)), raw.ctypes.data, nbytes)]                            # pageable host memory
    assert bad == [0] * len(bad), bad
    # no column has a pending start: 6, 7 and 8 are idle destinations of moves (a pending start would refuse them) ...
    r.move(3, 6)
    r.move(5, 7)
    r.move(14, 8)
    # ... and the same blobs, asked for properly, resume
    assert _resume_list(e, good((11, 13, 15)), blobs.data_ptr(), nbytes) == 3
    for c, rec in zip((11, 13, 15), recs):
        r.cols[c] = rec
    _finish(r, 7)
    e.close()
    r.check(y_lock, "after the refusals")
    assert len(r.got) == 6 and all(len(np.concatenate(v)) == s.N for v in r.got.values())


# ---- 5. SlotStream.drain, end to end ---------------------------------------------------------------------------------------------------

def test_a_drained_stream_goes_on_elsewhere_through_bytes_and_leaves_a_clean_engine():
    """Stream A (24 columns) holds 40 requests of both kinds, one of them streamed, at different progress, with a queue and one
    step pending: drain(pinned=True) -> to_bytes -> from_bytes (pinned and not, alternating) -> resume_many on stream B (20 columns
    of a second engine) -> to the end.  Every request: what A delivered, then what B delivered, is its lockstep column."""
    precision = 16
    cc, case, m, mel, up_w, w, t, x, y_mel, y_feat = _c3(precision)
    s, stride = case.shape, cc.stride
    frames = s.N // stride
    xg, melg = torch.from_numpy(x).cuda(), torch.from_numpy(mel).cuda()
    ea = _mel_engine(case, t, precision, "wg", w, m, up_w, stride, 24)
    eb = _mel_engine(case, t, precision, "wg", w, m, up_w, stride, 20)
    A, B = SlotStream(ea, 64), SlotStream(eb, 64)
    want, ha = {}, {}                                                 # request -> its samples; A's handle -> request

    def submit(i):
        uid = i % s.B
        if i == 5:                                                    # streamed: 20 frames so far, the rest arrives on B
            ha[A.submit_mel(melg[uid], uid=uid, frames=20, final=False)] = i
            want[i] = y_mel[uid]
        elif i % 3 == 2:
            f = 10 + (i * 7) % (frames - 9)
            ha[A.submit_mel(melg[uid][:, :f], uid=uid)] = i
            want[i] = y_mel[uid, :f * stride]
        else:
            n = 15 + (i * 11) % (s.N - 14)
            ha[A.submit(xg[uid][:, :n], uid=uid)] = i
            want[i] = y_feat[uid, :n]
        got[i] = []

    got = {}

    def collect(out, handles):
        for h, (yy, _) in out.items():
            got[handles[h]].append(np.array(yy))

    # the requests arrive in waves, so that they join at counters 0, 9 and 16: 27, 18 and 11 samples done at the drain
    for c, wave in ((9, range(0, 12)), (7, range(12, 22)), (5, range(22, 32))):
        for i in wave:
            submit(i)
        collect(A.step_async(c).result(), ha)
        A.finished()
    for i in range(32, 40):
        submit(i)
    pend = A.step_async(6)                                            # pending while the stream is drained
    assert A.waiting() > 0 and len(A.running()) > 16
    order = sorted(A.running()) + sorted(item[0] for item in A._queue)
    states = A.drain(pinned=True)
    assert not A.busy() and sorted(A._free) == list(range(24)) and A.compact() == 0 and A.running() == {}
    collect(pend.result(), ha)
    A.finished()
    assert len(states) == len(order) and any(st.blob is None for st in states) and sum(st.blob is not None for st in states) > 16
    assert all(st.blob is None or st.blob.is_pinned() for st in states)
    assert len({st.done for st in states if st.blob is not None}) > 2, "the requests should be at different progress"
    data = [st.to_bytes() for st in states]
    back = [SlotState.from_bytes(d, st.source, pinned=(k % 2 == 0)) for k, (d, st) in enumerate(zip(data, states))]
    hb = dict(zip(B.resume_many(back), (ha[h] for h in order)))
    streamed = [h for h, i in hb.items() if i == 5][0]
    B.extend_mel(streamed, frames, final=True)
    while B.busy():
        collect(B.step(13), hb)
        B.finished()
    B.close()
    for i in want:
        y = np.concatenate(got[i]) if got[i] else np.zeros(0, dtype=np.int32)
        assert len(y) == len(want[i]) and np.array_equal(y, want[i]), "request %d (utterance %d): %d of %d samples" % (i, i % s.B, len(y), len(want[i]))
    # a request that compact() has just moved cannot be suspended before the step: RuntimeError, and nothing has changed
    C = SlotStream(eb, 64)
    hc = [C.submit(xg[c % s.B][:, :(60 if c in (17, 18) else 5)], uid=c % s.B) for c in range(20)]
    parts = {17: [], 18: []}
    for h, (yy, _) in C.step(5).items():
        if hc.index(h) in parts:
            parts[hc.index(h)].append(yy)
    assert sorted(C.running().values()) == [17, 18] and C.compact() == 2
    before = (dict(C.running()), sorted(C._free), len(C._queue))
    with pytest.raises(RuntimeError):
        C.suspend_many([hc[18]])
    assert (dict(C.running()), sorted(C._free), len(C._queue)) == before
    while C.busy():
        for h, (yy, _) in C.step(11).items():
            parts[hc.index(h)].append(yy)
    for c in (17, 18):
        assert np.array_equal(np.concatenate(parts[c]), y_feat[c % s.B, :60]), c
    C.close()
    eb.close()
    # the clean-ring rule: after slotsEnd a lockstep run on A's engine equals one on a fresh engine
    A.close()
    xfull = xg[torch.arange(24, device="cuda") % s.B].contiguous()      # utterance b % B in column b (uid b: other selectors from column B on)
    y = np.full((24, s.N), -1, dtype=np.int32)
    ea.setFeatures(xfull)
    assert ea.run(s.N, 24, y, 1, False)
    ea.synchronize()
    ea.close()
    fresh = _mel_engine(case, t, precision, "wg", w, m, up_w, stride, 24)
    fresh.setFeatures(xfull)
    ref = np.full((24, s.N), -1, dtype=np.int32)
    assert fresh.run(s.N, 24, ref, 1, False)
    fresh.synchronize()
    fresh.close()
    bad = np.nonzero((y != ref).any(axis=1))[0]
    assert bad.size == 0, "columns %s differ from a fresh engine's lockstep run after a drained slot session" % bad[:10]
    assert np.array_equal(ref[:s.B], y_feat)
