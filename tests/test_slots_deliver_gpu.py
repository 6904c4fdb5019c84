"""GPU tests of ragged delivery (`-m gpu`): nvw_slots_step_ragged against its twin.  Two engines of the same model and
seed are driven through the same schedule of starts, stops, mel appends, moves and a save / resume; one steps with nvw_slots_step
into device buffers [batch][count], the other with nvw_slots_step_ragged.  Every piece must equal the twin's row prefix bit for
bit, samples and PCM; the pieces must be the ones a numpy restatement of the rule predicts; nothing outside the pieces may be
written (canaries before offset 0, in every padding gap, after the total)."""
import ctypes as C

import numpy as np
import pytest
import torch

from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import SLOT_PIECE
from test_slots_gpu import FAMILIES, _edge, _engine, _synth

pytestmark = pytest.mark.gpu

CANARY = -7
GUARD = 8          # elements in front of offset 0 (keeps the 16-byte alignment of both outputs)
STRIDE = 4         # of test_slots_gpu._synth's upsampling


def _inputs(name, precision, N=None):
    if name == "edge":
        case, m, x, w, Lh, t = _edge(precision, N=N or 96, B=8)
        return case, m, x, w, t, 64
    shape, window, seed = FAMILIES[name]
    case, m, x, w, Lh, t = _synth(name, shape, precision, seed)
    return case, m, x, w, t, window


def _twin_engine(case, m, w, t, precision, columns, window):
    e = _engine(case, t, precision, "wg", w, m["cond_b"], columns)
    up_w = m["up_w"].astype(np.float16).astype(np.float32) if precision == 16 else m["up_w"]
    e.setUpsampling(up_w, m["up_b"], STRIDE)
    e.slotsBegin(window)
    return e


class Out:
    """The ragged outputs of one engine, device or pinned, with canaries around and between the pieces."""

    def __init__(self, elems, where, samples=True, pcm=True):
        kw = {"device": "cuda"} if where == "device" else {"pin_memory": True}
        self.y = torch.empty(elems + 2 * GUARD, dtype=torch.int32, **kw) if samples else None
        self.p = torch.empty(elems + 2 * GUARD, dtype=torch.int16, **kw) if pcm else None
        self.elems = elems

    def arm(self):
        for a in (self.y, self.p):
            if a is not None:
                a.fill_(CANARY)
        torch.cuda.synchronize()

    def ptrs(self):
        return (self.y[GUARD:].data_ptr() if self.y is not None else None, self.p[GUARD:].data_ptr() if self.p is not None else None)

    def host(self):
        return (self.y.cpu().numpy() if self.y is not None else None, self.p.cpu().numpy() if self.p is not None else None)


def ragged(e, count, out, capacity=None, max_pieces=None, ptrs=None):
    """nvw_slots_step_ragged, raw: (total, pieces, ticket)."""
    pieces = np.zeros(e.maxBatch, dtype=SLOT_PIECE)
    n, ticket = C.c_int(-1), C.c_ulonglong(0)
    y, p = ptrs if ptrs is not None else out.ptrs()
    total = lib.nvw_slots_step_ragged(e._h, count, y, p, out.elems if capacity is None else capacity, pieces.ctypes.data,
                                      e.maxBatch if max_pieces is None else max_pieces, C.byref(n), C.byref(ticket), None)
    return total, pieces[:max(n.value, 0)], ticket.value


class Model:
    """The numpy restatement of the rule of nvw_slots_step_ragged: what the host knows about every column."""

    def __init__(self):
        self.cols = {}          # column -> [uid, next local sample, length or None (a mel column that may still be extended)]

    def expect(self, count):
        rows, off = [], 0
        for col in sorted(self.cols):
            uid, first, length = self.cols[col]
            n = count if length is None else min(count, length - first)
            if n <= 0:
                continue
            rows.append((col, uid, first, n, int(length is not None and first + n == length), off))
            off = (off + n + 7) // 8 * 8
        total = rows[-1][5] + rows[-1][3] if rows else 0
        return np.array(rows, dtype=SLOT_PIECE), total

    def advance(self, pieces):
        for pc in pieces:
            self.cols[int(pc["slot"])][1] += int(pc["n"])


def check_step(e_plain, e_rag, model, count, out, what):
    """One step on both engines; the pieces against the model, the delivered samples against the twin's rows, the canaries.  Returns
    the pieces."""
    B = e_plain.maxBatch
    y0 = torch.full((B, count), -1, dtype=torch.int32, device="cuda")
    p0 = torch.zeros((B, count), dtype=torch.int16, device="cuda")
    assert e_plain.slotsStep(count, y0, p0)
    out.arm()
    want, want_total = model.expect(count)
    total, pieces, ticket = ragged(e_rag, count, out)
    assert total == want_total, (what, total, want_total)
    assert len(pieces) == len(want), (what, len(pieces), len(want))
    for f in SLOT_PIECE.names:
        assert np.array_equal(pieces[f], want[f]), (what, f, pieces[f][:8], want[f][:8])
    assert np.all(pieces["offset"] % 8 == 0) and np.all(np.diff(pieces["slot"]) > 0)
    assert lib.nvw_slots_wait(e_rag._h, ticket) == 1 and lib.nvw_slots_done(e_rag._h, ticket) == 1
    y0, p0 = y0.cpu().numpy(), p0.cpu().numpy()
    y1, p1 = out.host()
    covered = np.zeros(out.elems + 2 * GUARD, dtype=bool)
    for pc in pieces:
        a, n, col = GUARD + int(pc["offset"]), int(pc["n"]), int(pc["slot"])
        covered[a:a + n] = True
        if y1 is not None:
            assert np.array_equal(y1[a:a + n], y0[col, :n]), "%s: samples of column %d" % (what, col)
        if p1 is not None:
            assert np.array_equal(p1[a:a + n], p0[col, :n]), "%s: PCM of column %d" % (what, col)
    for a in (y1, p1):
        if a is not None:
            assert np.all(a[~covered] == CANARY), "%s: written outside the pieces at %s" % (what, np.nonzero(a[~covered] != CANARY)[0][:8])
    model.advance(pieces)
    return pieces


def stop_finished(engines, model, pieces):
    for pc in pieces[pieces["finished"] != 0]:
        for e in engines:
            e.slotStop(int(pc["slot"]))
        del model.cols[int(pc["slot"])]


@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("name,precision", [("edge", 16), ("edge", 32), ("C4_R128_L30", 16)])
def test_ragged_steps_equal_the_plain_steps_of_a_twin(name, precision, where):
    """C3-shaped (fp16, fp32) and R = 128: feature columns, a final and a streamed mel column in a ragged last tile with idle columns
    between busy ones; steps of 1, 7, 13 and W samples (13 and 7 do not divide W: rows wrap inside steps); utterances that end
    mid-step; a move, a suspend (save + stop) and a resume in another column."""
    case, m, x, w, t, W = _inputs(name, precision)
    s = case.shape
    N, frames = s.N, s.N // STRIDE
    columns = 36
    engines = [_twin_engine(case, m, w, t, precision, columns, W) for _ in range(2)]
    xg = torch.from_numpy(x).cuda()
    melg = torch.from_numpy(m["features"]).cuda()
    model = Model()
    out = Out(columns * ((W + 7) // 8 * 8), where)

    def both(fn):
        return [fn(e) for e in engines]

    def step(count, what):
        count = min(count, engines[0].slotsHeadroom())
        assert engines[1].slotsHeadroom() >= count > 0
        pieces = check_step(engines[0], engines[1], model, count, out, "%s fp%d %s, %s" % (name, precision, where, what))
        stop_finished(engines, model, pieces)
        return pieces

    n1, n4 = N // 2 + 2, N // 3 + 1
    both(lambda e: e.slotStart(0, xg[0], 0, N))
    both(lambda e: e.slotStart(35, xg[1], 1, n1))
    both(lambda e: e.slotStartMel(17, melg[2], 2, frames, True))
    both(lambda e: e.slotStartMel(3, melg[3], 3, 5, False))
    model.cols = {0: [0, 0, N], 35: [1, 0, n1], 17: [2, 0, frames * STRIDE], 3: [3, 0, None]}
    p = step(7, "first step")
    assert list(p["slot"]) == [0, 3, 17, 35] and list(p["offset"]) == [0, 8, 16, 24]
    step(1, "one sample")
    both(lambda e: e.slotMove(35, 1))
    model.cols[1] = model.cols.pop(35)
    both(lambda e: e.slotMelFrames(3, frames - 1, False))
    step(13, "after a move")
    blobs = both(lambda e: e.slotSave(0))
    assert blobs[0][1] == blobs[1][1] == 21
    both(lambda e: e.slotStop(0))
    saved = model.cols.pop(0)
    both(lambda e: e.slotStart(20, xg[4], 4, n4))
    model.cols[20] = [4, 0, n4]
    both(lambda e: e.slotMelFrames(3, frames, True))
    model.cols[3][2] = frames * STRIDE
    p = step(W, "a whole window")
    assert np.any(p["finished"] != 0) and np.any(p["n"] < p["n"].max())
    for e, (blob, done) in zip(engines, blobs):
        e.slotResume(34, blob, xg[0], N)
    model.cols[34] = saved
    both(lambda e: e.slotStart(2, xg[5], 5, N))
    model.cols[2] = [5, 0, N]
    for i in range(100):
        if not model.cols:
            break
        step((13, 1, W, 7)[i % 4], "step %d of the tail" % i)
    assert not model.cols
    both(lambda e: e.close())


def test_4112_columns_once():
    """257 tiles and a ragged 258th: every seventh column idle, lengths of 5 to N samples, device and pinned outputs by turns."""
    case, m, x, w, t, W = _inputs("edge", 16)
    s = case.shape
    columns = 4112
    engines = [_twin_engine(case, m, w, t, 16, columns, W) for _ in range(2)]
    xg = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(41)
    model = Model()
    for b in range(columns):
        if b % 7 == 3:
            continue
        n = int(rng.integers(5, s.N + 1))
        for e in engines:
            e.slotStart(b, xg[b % s.B], b, n)
        model.cols[b] = [b, 0, n]
    outs = [Out(columns * 64, "device"), Out(columns * 64, "pinned")]
    for i in range(100):
        if not model.cols:
            break
        count = (13, 64, 7, 1)[i % 4]
        pieces = check_step(engines[0], engines[1], model, count, outs[i % 2], "4112 columns, step %d" % i)
        stop_finished(engines, model, pieces)
    assert not model.cols
    for e in engines:
        e.close()


def test_refusals_return_minus_one_and_change_nothing():
    case, m, x, w, t, W = _inputs("edge", 16)
    s = case.shape
    frames = s.N // STRIDE
    xg = torch.from_numpy(x).cuda()
    melg = torch.from_numpy(m["features"]).cuda()
    out = Out(8 * 64, "pinned")
    cold = _engine(case, t, 16, "wg", w, m["cond_b"], 8)
    assert ragged(cold, 4, out)[0] == -1                                  # not in slot mode
    cold.close()
    engines = [_twin_engine(case, m, w, t, 16, 8, W) for _ in range(2)]
    model = Model()
    for e in engines:
        e.slotStart(1, xg[0], 0, s.N)
        e.slotStart(6, xg[1], 1, 30)
        e.slotStartMel(4, melg[2], 2, 3, False)
    model.cols = {1: [0, 0, s.N], 6: [1, 0, 30], 4: [2, 0, None]}
    check_step(engines[0], engines[1], model, 5, out, "before the refusals")
    e = engines[1]
    out.arm()
    pageable = np.zeros(8 * 64, dtype=np.int32)
    assert ragged(e, 0, out)[0] == -1                                     # count out of range
    assert ragged(e, W + 1, out)[0] == -1
    assert e.slotsHeadroom() == 3 * STRIDE - 5
    assert ragged(e, 3 * STRIDE - 4, out)[0] == -1                        # above the headroom
    assert ragged(e, 4, out, ptrs=(None, None))[0] == -1                  # both outputs NULL
    assert ragged(e, 4, out, ptrs=(pageable.ctypes.data, None))[0] == -1  # pageable host memory
    assert ragged(e, 4, out, ptrs=(out.ptrs()[0], pageable.ctypes.data))[0] == -1
    assert ragged(e, 4, out, capacity=19)[0] == -1                        # three pieces of 4 end at 20
    assert ragged(e, 4, out, max_pieces=2)[0] == -1
    assert lib.nvw_slots_wait(e._h, 99) == 0 and lib.nvw_slots_done(e._h, 99) == 0 and lib.nvw_slots_wait(e._h, 0) == 0
    torch.cuda.synchronize()
    y1, p1 = out.host()
    assert np.all(y1 == CANARY) and np.all(p1 == CANARY) and np.all(pageable == 0)
    total, pieces, ticket = ragged(e, 4, out, capacity=20, max_pieces=3)  # exactly enough
    assert total == 20 and len(pieces) == 3 and ticket == 2
    assert lib.nvw_slots_wait(e._h, ticket) == 1
    y0 = torch.empty((8, 4), dtype=torch.int32, device="cuda")
    assert engines[0].slotsStep(4, y0)
    y0, y1 = y0.cpu().numpy(), out.host()[0]
    for pc in pieces:
        a = GUARD + int(pc["offset"])
        assert np.array_equal(y1[a:a + 4], y0[int(pc["slot"])]), int(pc["slot"])
    model.advance(pieces)
    check_step(engines[0], engines[1], model, 3, out, "the next step after the refusals")      # (plain and ragged stay twins)
    for e in engines:
        e.close()


def test_steps_in_flight_two_deep_equal_a_run_that_waits_after_each():
    """Six steps of 2 048 samples alternate between two pinned buffers; step k + 1 -- with its starts and stops -- is issued before
    step k is waited for.  Every piece equals that of a second engine which waits after each step.  The last ticket is not complete
    right after its issue (a step of 2 048 samples takes tens of milliseconds, the query microseconds) and is after the wait."""
    case, m, x, w, t, _ = _inputs("edge", 16)
    s = case.shape
    W, count, K, columns = 2048, 2048, 6, 20
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    src = torch.randn(x.shape[1], K * count, device="cuda", generator=g).half()
    lengths = {0: K * count, 1: 3000, 2: 5000, 3: 2048, 4: 7001, 5: 100, 6: 4097, 7: 2500}

    def schedule(e, k):
        """the starts and stops before step k: utterance k + 2 joins in column 19 - k; column 0 is stopped before step 4"""
        if k == 0:
            for u in (0, 1):
                e.slotStart(u, src[:, u:], u, lengths[u])
        e.slotStart(19 - k, src[:, 7 * k:], k + 2, lengths[k + 2])
        if k == 4:
            e.slotStop(0)

    def collect(buf, pieces, total, got):
        y, p = buf
        for pc in pieces:
            a, n = int(pc["offset"]), int(pc["n"])
            got.setdefault(int(pc["uid"]), []).append((y[a:a + n].numpy().copy(), p[a:a + n].numpy().copy()))

    def run(pipelined):
        e = _twin_engine(case, m, w, t, 16, columns, W)
        bufs = [e.slotsPinned(columns * count) for _ in range(2)]
        got, issued, not_done = {}, [], 0

        def issue(k):
            schedule(e, k)
            total, pieces, ticket = e.slotsStepRagged(count, *bufs[k % 2])
            for pc in pieces[pieces["finished"] != 0]:
                e.slotStop(int(pc["slot"]))
            issued.append((total, pieces, ticket))
            return ticket

        if pipelined:
            issue(0)
            for k in range(K):
                if k + 1 < K:
                    last = issue(k + 1)
                    if k + 1 == K - 1:
                        not_done += not e.slotsDone(last)
                total, pieces, ticket = issued[k]
                e.slotsWait(ticket)
                assert e.slotsDone(ticket)
                collect(bufs[k % 2], pieces, total, got)
        else:
            for k in range(K):
                ticket = issue(k)
                e.slotsWait(ticket)
                collect(bufs[k % 2], issued[k][1], issued[k][0], got)
        assert [i[2] for i in issued] == list(range(1, K + 1))
        e.close()
        return got, not_done

    a, not_done = run(True)
    b, _ = run(False)
    assert not_done == 1, "the last step was complete right after it was issued"
    assert sorted(a) == sorted(b) == list(range(8))
    for uid in a:
        ya, pa = (np.concatenate([v[i] for v in a[uid]]) for i in (0, 1))
        yb, pb = (np.concatenate([v[i] for v in b[uid]]) for i in (0, 1))
        assert np.array_equal(ya, yb) and np.array_equal(pa, pb), uid
        want = min(lengths[uid], (K - max(uid - 2, 0)) * count) if uid else 4 * count
        assert len(ya) == want, (uid, len(ya), want)


@pytest.mark.parametrize("which", ["samples", "pcm"])
def test_a_call_for_one_output_writes_only_that(which):
    case, m, x, w, t, W = _inputs("edge", 16)
    s = case.shape
    engines = [_twin_engine(case, m, w, t, 16, 20, W) for _ in range(2)]
    xg = torch.from_numpy(x).cuda()
    model = Model()
    for col, uid, n in ((0, 0, s.N), (9, 1, 20), (19, 2, 41)):
        for e in engines:
            e.slotStart(col, xg[uid], uid, n)
        model.cols[col] = [uid, 0, n]
    for where in ("device", "pinned"):
        out = Out(20 * 64, where, samples=which == "samples", pcm=which == "pcm")
        for count in (13, 1, 7):
            pieces = check_step(engines[0], engines[1], model, count, out, "%s only, %s" % (which, where))
            stop_finished(engines, model, pieces)
    for e in engines:
        e.close()


def test_the_output_timing_entry_redelivers_the_last_step_and_changes_nothing():
    """nvw_slots_time_outputs (measurement only): its ragged pass writes what the last ragged step delivered, its plain pass the
    rows of nvw_slots_step, and the session goes on as its twin does."""
    case, m, x, w, t, W = _inputs("edge", 16)
    s = case.shape
    engines = [_twin_engine(case, m, w, t, 16, 20, W) for _ in range(2)]
    xg = torch.from_numpy(x).cuda()
    model = Model()
    for col, uid in ((0, 0), (9, 1), (19, 2)):
        for e in engines:
            e.slotStart(col, xg[uid], uid, s.N)
        model.cols[col] = [uid, 0, s.N]
    out = Out(20 * 64, "pinned")
    for count in (60, 13):                      # (the second step's rows wrap)
        check_step(engines[0], engines[1], model, count, out, "before the timing")
    y_step, p_step = (a.copy() for a in out.host())
    again = Out(20 * 64, "pinned")
    again.arm()
    e = engines[1]
    assert lib.nvw_slots_time_outputs(e._h, 1, 13, *again.ptrs(), again.elems, 2, None) >= 0
    y, p = again.host()
    assert np.array_equal(y, y_step) and np.array_equal(p, p_step)
    rows_y = torch.full((20, 13), -1, dtype=torch.int32, device="cuda")
    rows_p = torch.zeros((20, 13), dtype=torch.int16, device="cuda")
    assert lib.nvw_slots_time_outputs(e._h, 0, 13, rows_y.data_ptr(), rows_p.data_ptr(), 20 * 13, 2, None) >= 0
    for i, col in enumerate((0, 9, 19)):
        assert np.array_equal(rows_y[col].cpu().numpy(), y_step[GUARD + 16 * i:GUARD + 16 * i + 13])
    assert lib.nvw_slots_time_outputs(e._h, 1, 13, *again.ptrs(), 40, 2, None) < 0          # too little capacity
    check_step(engines[0], engines[1], model, 7, out, "after the timing")
    for e in engines:
        e.close()
