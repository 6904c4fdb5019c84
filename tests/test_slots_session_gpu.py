"""GPU test of the slot session's staging rings at wrap-around (`-m gpu`): the step updates, the list saves,
the temperature scales (two staging halves each) and the delivery tickets (four) are reused past their depth by calls that never
wait for one another.  (The mel updates go through the same class; no mel column runs here.)  Engine A issues eight ragged steps
into pinned memory -- each with a start and a temperature change, all but the first, which has no running column yet, with a
move --, three list saves in a row and a list resume without waiting in between; its twin B synchronises the device after every
call.  Everything either engine reports or writes must be equal byte for byte: same kernels, same inputs, no tolerance.  What the
test can see of the tickets is what the calls return: that A's calls did not block is not observable from here."""
import functools

import numpy as np
import pytest
import torch

from test_slots_gpu import FAMILIES, _engine, _synth

pytestmark = pytest.mark.gpu

COLUMNS = 17          # two tiles, the second with one column
WINDOW = 32           # four times the largest dilation of C1_R32 (8)
COUNT = 8
TEMPS = (0.5, 2.0, 0.8, 1.25, 4.0, 0.25)
# before step k: utterance k joins in column k; the utterance of column MOVES[k][0] goes on in column MOVES[k][1]
MOVES = ((10, 16), (11, 15), (0, 14), (1, 13), (2, 12), (3, 9))
SAVES = ((16, 4, 14), (15, 13), (12, 9, 5, 16))
RESUME_INTO = (0, 1, 2, 3)      # the columns of SAVES[2] go on a second time in these (idle since their moves)


@functools.lru_cache(maxsize=None)
def _inputs(precision):
    shape, _, seed = FAMILIES["C1_R32"]
    case, m, x, w, Lh, t = _synth("C1_R32", shape, precision, seed)
    assert shape.N >= 8 * COUNT and shape.B >= 8 and WINDOW % shape.maxD == 0
    return case, m, x, w, t


def _drive(precision, wait_after_every_call):
    """The schedule on a fresh engine; returns what it reported and wrote, and the ticket checks made before the final wait."""
    case, m, x, w, t = _inputs(precision)
    e = _engine(case, t, precision, "wg", w, m["cond_b"], COLUMNS)
    e.slotsBegin(WINDOW)
    xg = torch.from_numpy(x).cuda()
    outs, steps, blobs = [], [], []

    def sync():
        if wait_after_every_call:
            torch.cuda.synchronize()

    def step():
        out = e.slotsPinned(COLUMNS * COUNT)
        for a in out:
            a.fill_(-7)
        total, pieces, ticket = e.slotsStepRagged(COUNT, *out)
        sync()
        outs.append(out)
        steps.append((total, pieces.copy(), ticket))

    for col, uid in ((10, 6), (11, 7)):
        e.slotStart(col, xg[uid], uid)
        sync()
    e.slotSetTemperature(10, 3.0)
    sync()
    step()
    for k in range(6):
        e.slotStart(k, xg[k], k)
        sync()
        e.slotSetTemperature(k, TEMPS[k])
        sync()
        e.slotMove(*MOVES[k])
        sync()
        step()
    saved = []
    for cols in SAVES:
        b, s = e.slotsSaveList(cols)
        sync()
        blobs.append(b)
        saved.append(s.copy())
    uids = [int(u) for u in saved[2]["uid"]]
    e.slotsResumeList(RESUME_INTO, blobs[2], [xg[u] for u in uids])
    sync()
    e.slotStart(6, xg[4], 4)          # (the last step as the others: a start, a temperature change, a move)
    sync()
    e.slotSetTemperature(6, 1.5)
    sync()
    e.slotMove(4, 7)
    sync()
    step()
    tickets = [s[2] for s in steps]
    assert tickets == list(range(1, 9))
    # tickets older than the four events kept are complete by the stream's order: reported at once, before anything is waited for
    old = [(e.slotsDone(tk), e.slotsWait(tk) is None) for tk in tickets[:4]]
    e.slotsWait(tickets[-1])
    done = [e.slotsDone(tk) for tk in tickets]
    torch.cuda.synchronize()
    result = {
        "pieces": [(total, pieces.tobytes()) for total, pieces, _ in steps],
        "samples": [[(y[int(pc["offset"]):int(pc["offset"]) + int(pc["n"])].numpy().tobytes(),
                      p[int(pc["offset"]):int(pc["offset"]) + int(pc["n"])].numpy().tobytes()) for pc in pieces]
                    for (y, p), (_, pieces, _) in zip(outs, steps)],
        "saved": [s.tobytes() for s in saved],
        "blobs": [b.cpu().numpy().tobytes() for b in blobs],
        "temps": [e.slotTemperature(c) for c in range(COLUMNS)],
    }
    n_pieces = [len(pieces) for _, pieces, _ in steps]
    e.close()
    return result, old, done, n_pieces


@pytest.mark.parametrize("precision", [16, 32])
def test_calls_that_never_wait_reuse_the_staging_rings_and_equal_a_twin_that_always_waits(precision):
    a, old_a, done_a, n_a = _drive(precision, False)
    b, old_b, done_b, n_b = _drive(precision, True)
    assert n_a == n_b == [2, 3, 4, 5, 6, 7, 8, 13], n_a      # (every step delivers: the schedule ran as written)
    assert old_a == old_b == [(True, True)] * 4, "a ticket older than the ring did not report done"
    assert done_a == done_b == [True] * 8, "a ticket did not report done after the final wait"
    for key in ("pieces", "saved", "temps"):
        assert a[key] == b[key], key
    for k, (sa, sb) in enumerate(zip(a["samples"], b["samples"])):
        assert sa == sb, "delivered samples or PCM of step %d differ" % k
    for k, (ba, bb) in enumerate(zip(a["blobs"], b["blobs"])):
        assert ba == bb, "blobs of list save %d differ" % k
