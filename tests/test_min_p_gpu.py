"""GPU tests of the probability floor (min-p; `-m gpu`).  A column with floor tau draws from its tempered distribution
without the bins whose e = exp2(fma(z, c, -(m c))) is below tau.  Floor 0 is the run without the feature, bit for bit; the support
and the CDF of a floored run are checked against the engine's OWN scoring pass (scoreSamples(rows=True) at the column's
temperature) to the EPS derived in tests/min_p_cases.py, with the draws of oracle.philox_selectors_at; the same check applied to a
run made at floor 0 fails.  Shapes, floors and temperatures: tests/min_p_cases.py (those of tests/temperature_cases.py)."""
import numpy as np
import pytest
import torch

import cases
import min_p_cases as MP
import score_cases as SC
import temperature_cases as TC
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.slots import SlotState, SlotStream, min_p_rows
from oracle import oracle as O
from test_features_gpu import _run
from test_slots_gpu import SEED
from test_slots_mel_gpu import _mel_engine, _mel_inputs
from test_slots_state_gpu import Run, _finish
from test_temperature_gpu import K0, _column_of, _header, _inputs, _seeded, _slot_engine

pytestmark = pytest.mark.gpu

RUNS = [(16, "wg"), (16, "wg2"), (16, "wg3"), (32, "wg"), (32, "wg2")]      # one to three tiles per workgroup (fp32: one and two)
WORD = 11                                                                    # of a blob's header: the bits of the floor, zero for 0
_cache = {}


def _floored(cc, precision, mode, taus, temps, dump=True):
    """The run under test: column b at temperature temps[b] with floor taus[b]; once per argument list."""
    key = ("run", cc.name, precision, mode, tuple(taus), tuple(temps), dump)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(cc, precision)
        e = _seeded(case, t, precision, mode, m, x, w)
        e.setTemperatures(temps)
        e.setMinP(taus)
        _cache[key] = _run(e, case, dump=dump)
        e.close()
    return _cache[key]


def _mixed(cc, precision, mode):
    B = cases.BY_NAME[cc.case_name].shape.B
    return _floored(cc, precision, mode, MP.floors(B), MP.temperatures(B))


def _unfloored(cc, precision, mode):
    B = cases.BY_NAME[cc.case_name].shape.B
    return _floored(cc, precision, mode, [0.0] * B, MP.temperatures(B))


# ---- 1. floor 0 is the identity ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", RUNS)
def test_floor_zero_is_the_identity_in_lockstep(precision, mode):
    """Never setting a floor, setting all zeros -- before any other value was set (no table) and after one was (the table exists,
    its second half zero, Params::floorOn 0) --, and a floor set and taken back: the samples, the dumped P and Za of the engine that
    never heard of the feature.  At the mixed temperatures, so the table's first half is in use throughout."""
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps = MP.temperatures(s.B)
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps)
    plain = _run(e, case)
    for prepare in (lambda: e.setMinP([0.0] * s.B), lambda: (e.setMinP(MP.floors(s.B)), e.setMinP([0.0] * s.B)),
                    lambda: (e.setMinP(0.25), e.setMinP(None))):
        prepare()
        e.resetHistory()
        again = _run(e, case)
        assert np.array_equal(again["y"], plain["y"]) and np.array_equal(again["P"], plain["P"]) and np.array_equal(again["Za"], plain["Za"])
    e.close()
    assert np.array_equal(plain["y"], _unfloored(MP.COND, precision, mode)["y"])
    # ... and an engine without temperatures either: no table is ever made by zeros
    e = _seeded(case, t, precision, mode, m, x, w)
    bare = _run(e, case)
    e.setMinP([0.0] * s.B)
    e.resetHistory()
    again = _run(e, case)
    e.close()
    assert np.array_equal(again["y"], bare["y"]) and np.array_equal(again["P"], bare["P"])


def _slot_session(precision, mode, variant):
    """A slot session of 12 utterances over three tiles: samples per utterance and, after 21 samples, every column's blob (one list
    save).  variant 0: the floor is never mentioned; 1: set to 0 after every start; 2: set to 0.25 and back to 0 before the step."""
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps = MP.temperatures(s.B)
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    uids = (0, 1, 2, 3, 4, 7, 16, 21, 22, 33, 38, 39)
    for b in uids:
        r.start(b, b)
        e.slotSetTemperature(b, temps[b])
        if variant == 1:
            e.slotSetMinP(b, 0.0)
        if variant == 2:
            e.slotSetMinP(b, 0.25)
            e.slotSetMinP(b, 0.0)
        assert e.slotMinP(b) == 0.0
    r.step(5)
    r.step(16)
    blobs, saved = e.slotsSaveList(list(uids))
    raw = blobs.cpu().numpy().copy()
    _finish(r, 16)
    e.close()
    return {r.uid_of[k]: np.concatenate(v) for k, v in r.got.items()}, raw


@pytest.mark.parametrize("precision,mode", RUNS)
def test_floor_zero_is_the_identity_in_slot_mode(precision, mode):
    y0, blobs0 = _slot_session(precision, mode, 0)
    y_lock = _unfloored(MP.COND, precision, mode)["y"]
    for uid, y in y0.items():
        assert np.array_equal(y, y_lock[uid]), uid
    assert not blobs0.view("<u4").reshape(len(blobs0), -1)[:, WORD].any(), "word 11 of a blob at floor 0 is zero"
    for variant in (1, 2):
        y, blobs = _slot_session(precision, mode, variant)
        assert all(np.array_equal(y[uid], y0[uid]) for uid in y0), variant
        assert np.array_equal(blobs, blobs0), "variant %d: the blobs differ from those of a session that never heard of the floor" % variant


# ---- 2. support and CDF, against the engine's own scoring pass ---------------------------------------------------------------------

def _scored(cc, precision, mode, which):
    """(y [B][N], rows per column [N][A] float32 from scoreSamples at the column's temperature, eps per column, u [N][B]) of the mixed
    run (which = "mixed") or of the run at floor 0 with the same temperatures ("zero")."""
    key = ("scored", cc.name, precision, mode, which)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(cc, precision)
        s = case.shape
        temps = MP.temperatures(s.B)
        y = (_mixed if which == "mixed" else _unfloored)(cc, precision, mode)["y"]
        assert y.min() >= 0 and y.max() < s.A
        xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        e = _seeded(case, t, precision, mode, m, x, w)
        got = e.scoreSamples([(yg[b].contiguous(), xg[b], temps[b]) for b in range(s.B)], rows=True)
        e.synchronize()
        rows = [r.cpu().numpy() for _, r in got]
        e.close()
        eps = []
        for b in range(s.B):
            Za, _ = SC.reference(t, s, y[b], Lh[:, :, b, :])
            eps.append(MP.epsilon(temps[b], np.abs(Za).max(), np.abs(rows[b]).max()))
        k, uid = np.meshgrid(np.arange(s.N), np.arange(s.B), indexing="ij")
        _cache[key] = (y, rows, eps, O.philox_selectors_at(SEED, k, uid).astype(np.float64))
    return _cache[key]


SUPPORT_RUNS = [(MP.COND, p, mode) for p, mode in RUNS] + [(MP.COND_A512, 16, "wg"), (MP.COND_A1024, 16, "wg")]


@pytest.mark.parametrize("cc,precision,mode", SUPPORT_RUNS, ids=lambda v: getattr(v, "name", str(v)))
def test_floored_draws_stay_in_the_kept_set_and_in_their_bin_of_the_floored_cdf(cc, precision, mode):
    """Free run with the mixed floors and temperatures, every column's own samples scored by the engine: for every sample
    rows[t][y] - max rows[t] >= log tau - EPS, and u lies in the picked bin of the CDF of min_p_rows(rows, tau) -- every row but those
    with a bin within EPS of the floor, at most 1 % of them."""
    y, rows, eps, u = _scored(cc, precision, mode, "mixed")
    B = y.shape[0]
    tot = MP.check_run(lambda b: rows[b], y, u, MP.floors(B), lambda b: eps[b], min_p_rows)
    print("%s fp%d/%s: support violations %d, CDF violations %d, left out %d of %d rows; EPS %.2e .. %.2e" % (
        (cc.name, precision, mode) + tot + (min(eps), max(eps))))
    assert max(eps) < 1e-4, eps
    assert MP.accepted(tot), tot
    assert not np.array_equal(y, _unfloored(cc, precision, mode)["y"])


@pytest.mark.parametrize("cc,precision,mode", SUPPORT_RUNS, ids=lambda v: getattr(v, "name", str(v)))
def test_the_same_check_rejects_a_run_made_at_floor_zero(cc, precision, mode):
    """The negative control on the GPU: the run with the same temperatures and no floor, held to the floors of the mixed run."""
    y, rows, eps, u = _scored(cc, precision, mode, "zero")
    B = y.shape[0]
    tot = MP.check_run(lambda b: rows[b], y, u, MP.floors(B), lambda b: eps[b], min_p_rows)
    print("%s fp%d/%s at floor 0: support violations %d, CDF violations %d, left out %d of %d rows" % ((cc.name, precision, mode) + tot))
    assert not MP.accepted(tot) and tot[0] >= 0.05 * tot[3], tot
    # (held to floor 0 it passes: the check itself is sound)
    zero = MP.check_run(lambda b: rows[b], y, u, [0.0] * B, lambda b: eps[b], min_p_rows)
    assert MP.accepted(zero), zero


# ---- 3. exact zeros in the probability dump ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2"), (16, "wg")])
def test_dropped_bins_read_exactly_zero_in_the_probability_dump(precision, mode):
    """Every sample forced by a prime (so the histories agree): getP at the last sample with and without floors.  Every probability
    is exactly 0 or positive; the zero set is {a : p0_a / max p0 < tau} up to bins within EPS of the floor; the rest sums to 1 within
    4 A eps32 and is p0 renormalised; Za stays the raw logits; the forced samples stay forced."""
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), MP.floors(s.B)
    prime = _mixed(MP.COND, precision, mode)["y"]
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps)
    e.setPrime(prime)
    p0 = _run(e, case)
    e.setMinP(taus)
    e.resetHistory()
    p1 = _run(e, case)
    e.close()
    assert np.array_equal(p0["y"], prime) and np.array_equal(p1["y"], prime) and np.array_equal(p0["Za"], p1["Za"])
    dropped = 0
    for b, tau in enumerate(taus):
        P0, P1 = p0["P"][b].astype(np.float64), p1["P"][b].astype(np.float64)
        assert np.isfinite(P1).all() and (P1 >= 0).all()
        if tau == 0.0:
            assert np.array_equal(p0["P"][b], p1["P"][b])
            continue
        with np.errstate(divide="ignore"):
            rel = np.log(P0) - np.log(P0.max())
        eps = MP.epsilon(temps[b], np.abs(p0["Za"][b]).max(), np.abs(rel[np.isfinite(rel)]).max())
        clear = np.abs(rel - np.log(tau)) > eps
        assert np.array_equal((P1 == 0)[clear], (rel < np.log(tau))[clear]), "column %d, floor %g: the zero set" % (b, tau)
        assert P1[P0.argmax()] > 0
        assert abs(P1.sum() - 1.0) <= 4 * s.A * SC.EPS32, (b, P1.sum())
        keep = P1 > 0
        assert np.abs(P1[keep] - P0[keep] / P0[keep].sum()).max() <= 4 * s.A * SC.EPS32, b
        dropped += int((~keep).sum())
    assert dropped > s.B, "the floors dropped next to nothing: the inputs do not exercise the rule"


# ---- 4. slot mode = lockstep -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2"), (16, "wg")])
def test_slot_utterances_reproduce_their_lockstep_columns_at_their_floors(precision, mode):
    """Utterance b (uid = b, T_b, tau_b) joins at step b mod 4 in column 7 b + 3 mod 40, window = the largest dilation, steps of 5 and
    16 samples: bit for bit column b of the lockstep run of test 2."""
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), MP.floors(s.B)
    y_lock = _mixed(MP.COND, precision, mode)["y"]
    e = _slot_engine(precision, mode)
    assert e.slotMinP(0) == -1.0                              # outside slot mode
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    assert e.slotMinP(0) == -1.0                              # no utterance
    for step in range(64):
        for b in range(s.B):
            if b % 4 == step:
                col = _column_of(b, s.B)
                r.start(col, b)
                assert e.slotMinP(col) == 0.0                 # a start puts the column back to 0: start, then set
                e.slotSetTemperature(col, temps[b])
                e.slotSetMinP(col, taus[b])
                assert e.slotMinP(col) == float(np.float32(taus[b]))
        if not r.cols:
            break
        r.step((5, 16)[step % 2])
    e.close()
    assert len(r.got) == s.B and all(len(np.concatenate(v)) == s.N for v in r.got.values())
    r.check(y_lock, "fp%d/%s slot floors" % (precision, mode))


def test_mel_columns_reproduce_their_lockstep_columns_at_their_floors():
    """The same for mel utterances (frames upsampled in the steps), against nvw_set_mel + nvw_generate_stream with setMinP."""
    cc = MP.COND
    case, m, mel, up_w, w, t = _mel_inputs(cc, 16)
    s = case.shape
    temps, taus = MP.temperatures(s.B), MP.floors(s.B)
    melg = torch.from_numpy(mel).cuda()
    lock = _mel_engine(case, t, 16, "wg2", w, m, up_w, cc.stride, s.B)
    lock.setMel(melg)
    lock.setTemperatures(temps)
    lock.setMinP(taus)
    y_lock = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_lock)
    lock.setMinP(None)
    lock.setMel(melg)                                          # (the temperatures stay in force: setMinP leaves them alone)
    y_plain = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_plain)
    lock.close()
    assert np.array_equal(y_lock[0::5], y_plain[0::5]) and not np.array_equal(y_lock[4], y_plain[4])      # floor-0 columns are the plain run's
    e = _mel_engine(case, t, 16, "wg2", w, m, up_w, cc.stride, s.B)
    r = Run(e, None, s.maxD, melg=melg, stride=cc.stride)
    for step in range(64):
        for b in range(s.B):
            if b % 4 == step:
                r.start_mel(_column_of(b, s.B), b, s.N // cc.stride)
                e.slotSetTemperature(_column_of(b, s.B), temps[b])
                e.slotSetMinP(_column_of(b, s.B), taus[b])
        if not r.cols:
            break
        r.step((5, 16)[step % 2])
    e.close()
    assert len(r.got) == s.B
    r.check(y_lock, "mel slot floors")


def _two_chunks(precision, mode):
    """y [B][N] of: samples [0, K0) at floors tau_a, setMinP, [K0, N) at tau_b (the temperatures throughout)."""
    key = ("chunks", precision, mode)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(MP.COND, precision)
        s = case.shape
        ta, tb = MP.floors(s.B), MP.floors(s.B, 2)
        e = _seeded(case, t, precision, mode, m, x, w)
        e.setTemperatures(MP.temperatures(s.B))
        e.setMinP(ta)
        y = np.full((s.B, s.N), -1, dtype=np.int32)
        assert e.run_partial_chunk(0, K0, s.N, s.B)
        e.setMinP(tb)
        assert e.run_partial(K0, s.N, s.B, y, 1, False)
        e.synchronize()
        e.close()
        _cache[key] = (y, ta, tb)
    return _cache[key]


@pytest.mark.parametrize("precision,mode", [(16, "wg2"), (32, "wg")])
def test_a_floor_set_between_two_steps_equals_the_lockstep_run_with_set_min_p_between_the_chunks(precision, mode):
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    y, ta, tb = _two_chunks(precision, mode)
    # lockstep: the first chunk is the one-floor run's, the rest is not; the chunked run passes the support check chunk by chunk
    one = _mixed(MP.COND, precision, mode)["y"]
    assert np.array_equal(y[:, :K0], one[:, :K0]) and not np.array_equal(y[:, K0:], one[:, K0:])
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    temps = MP.temperatures(s.B)
    for b in range(s.B):
        r.start(_column_of(b, s.B), b)
        e.slotSetTemperature(_column_of(b, s.B), temps[b])
        assert lib.nvw_slot_set_min_p(e._h, _column_of(b, s.B), ta[b])
    for _ in range(K0 // 5):
        r.step(5)
    for b in range(s.B):
        assert lib.nvw_slot_set_min_p(e._h, _column_of(b, s.B), tb[b])
    r.step(16)
    _finish(r, 5)
    e.close()
    r.check(y, "fp%d/%s floor set at local sample %d" % (precision, mode, K0))


# ---- 5. the state carries the floor ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2")])
def test_moves_saves_and_resumes_carry_the_floor(precision, mode):
    """After some steps: slotMove across tiles, slotSave + slotResume into another column of a second engine -- both continue bit for
    bit; header word 11 holds the bits of the floor, zero for a column at floor 0; a damaged word 11 is refused with nothing changed."""
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), MP.floors(s.B)
    y_lock = _mixed(MP.COND, precision, mode)["y"]
    xg = torch.from_numpy(x).cuda()
    e = _slot_engine(precision, mode)
    r = Run(e, xg, s.maxD)
    for b in (0, 1, 2, 3, 4, 7, 21, 38):                     # floors 0, .05, .1, .25, .5, .1, .05, .25
        r.start(b + 1, b)
        e.slotSetTemperature(b + 1, temps[b])
        e.slotSetMinP(b + 1, taus[b])
    r.step(5)
    r.step(16)
    r.move(5, 30)                                             # uid 4 (floor 0.5) across tiles
    r.move(39, 0)                                             # uid 38 (floor 0.25) into the first tile
    assert (e.slotMinP(30), e.slotMinP(0), e.slotMinP(5), e.slotMinP(39)) == (0.5, 0.25, -1.0, -1.0)
    r.start(5, 9)                                             # the move's source takes a new utterance: back to 0
    assert e.slotMinP(5) == 0.0
    e.slotStop(5)
    del r.cols[5], r.got[len(r.got) - 1]
    r.step(5)
    e2 = _slot_engine(precision, mode, 24)
    r2 = Run(e2, xg, 2 * s.maxD, into=r)
    r2.start(3, 6)                                            # uid 6: floor 0.05
    e2.slotSetTemperature(3, temps[6])
    e2.slotSetMinP(3, taus[6])
    r2.step(7)
    for col, uid, to in ((4, 3, 17), (1, 0, 0), (2, 1, 5)):
        blob, rec = r.suspend(col)
        h = _header(blob)
        assert h[WORD] == MP.bits(float(np.float32(taus[uid]))) and not h[12:].any() and (h[6], h[7]) == (26, uid)
        r2.resume(to, blob, rec)
        assert e2.slotMinP(to) == float(np.float32(taus[uid])) and e2.slotTemperature(to) == temps[uid] and e.slotMinP(col) == -1.0
    blob, rec = r.suspend(8)                                  # uid 7, floor 0.1
    for word in (MP.bits(-0.1), MP.bits(0.6), MP.bits(float("nan")), MP.bits(float("inf")), 0x80000000):
        bad = blob.clone()
        bad[4 * WORD:4 * WORD + 4] = torch.from_numpy(np.array([word], dtype="<u4").view(np.uint8).copy()).cuda()
        assert not lib.nvw_slot_resume(e2._h, 9, bad.data_ptr(), xg[7].data_ptr(), 32, xg[7].stride(0), xg[7].stride(1), s.N)
        assert e2.slotMinP(9) == -1.0 and e2.slotTemperature(9) == 0.0
    r2.resume(9, blob, rec)
    assert e2.slotMinP(9) == float(np.float32(taus[7]))
    _finish(r, 16)
    _finish(r2, 5)
    e.close(), e2.close()
    assert len(r.got) == 9
    r.check(y_lock, "fp%d/%s moved, saved and resumed" % (precision, mode))


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2")])
def test_resumes_into_the_engine_that_saved_them_take_the_floor_of_the_blob(precision, mode):
    """Saved blobs go back into columns of the SAME engine that held other utterances before -- a higher floor, floor 0, the same
    floor, and a column never used --, singly (slotResume) and as a list (slotsSaveList + slotsResumeList): the column's floor is the
    blob's, whatever its table entry held, and every utterance continues bit for bit as its lockstep column."""
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), [float(np.float32(p)) for p in MP.floors(s.B)]
    y_lock = _mixed(MP.COND, precision, mode)["y"]
    xg = torch.from_numpy(x).cuda()
    e = _slot_engine(precision, mode)
    r = Run(e, xg, s.maxD)
    for b in (0, 1, 2, 3, 4, 7, 8):                          # floors 0, .05, .1, .25, .5, .1, .25 in columns b + 1
        r.start(b + 1, b)
        e.slotSetTemperature(b + 1, temps[b])
        e.slotSetMinP(b + 1, taus[b])
    r.step(5)
    r.step(16)
    # singly: uid 0 (floor 0) into the column that held 0.5, uid 4 (0.5) into the one that held 0, uid 3 (0.25) into one that held
    # 0.25, uid 8 into a column never used
    saved = {uid: r.suspend(uid + 1) for uid in (0, 4, 3, 8)}
    for uid, to in ((0, 5), (4, 1), (3, 9), (8, 20)):
        blob, rec = saved[uid]
        assert _header(blob)[WORD] == MP.bits(taus[uid]) and e.slotMinP(to) == -1.0
        r.resume(to, blob, rec)
        assert e.slotMinP(to) == taus[uid] and e.slotTemperature(to) == temps[uid]
    r.step(5)
    # as a list: uid 1 (0.05) into the column that held 0.1, uid 2 (0.1) into the one that held 0.05, uid 7 (0.1) into one that held 0.1
    cols, to = [2, 3, 8], [8, 2, 3]
    blobs, rec = e.slotsSaveList(cols)
    assert [int(v) for v in rec["uid"]] == [1, 2, 7] and [int(v) for v in rec["done"]] == [26, 26, 26]
    words = blobs.cpu().numpy().view("<u4").reshape(3, -1)[:, WORD]
    assert [int(v) for v in words] == [MP.bits(taus[1]), MP.bits(taus[2]), MP.bits(taus[7])]
    recs = []
    for col in cols:
        e.slotStop(col)
        recs.append(r.cols.pop(col))
        assert e.slotMinP(col) == -1.0
    e.slotsResumeList(to, blobs, [xg[1], xg[2], xg[7]])
    for col, uid, one in zip(to, (1, 2, 7), recs):
        r.cols[col] = one
        assert e.slotMinP(col) == taus[uid] and e.slotTemperature(col) == temps[uid]
    r.step(5)
    again, _ = e.slotsSaveList(to)                            # the saves of the resumed columns carry the floors on
    words = again.cpu().numpy().view("<u4").reshape(3, -1)[:, WORD]
    assert [int(v) for v in words] == [MP.bits(taus[1]), MP.bits(taus[2]), MP.bits(taus[7])]
    _finish(r, 16)
    e.close()
    assert len(r.got) == 7 and all(len(np.concatenate(v)) == s.N for v in r.got.values())
    r.check(y_lock, "fp%d/%s resumed into the engine that saved them" % (precision, mode))


def test_a_session_whose_floored_utterances_have_ended_launches_without_floors_again():
    """slotStop and slotMove leave no floor behind in the column they vacate: nvw_slot_min_p of the idle column is -1, the next
    utterance there starts at 0 and reproduces its lockstep column at floor 0."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), MP.floors(s.B)
    xg = torch.from_numpy(x).cuda()
    e = _slot_engine(precision, mode)
    r = Run(e, xg, s.maxD)
    for b in (3, 4):
        r.start(b, b)
        e.slotSetTemperature(b, temps[b])
        e.slotSetMinP(b, taus[b])
    r.step(5)
    r.move(3, 17)
    assert (e.slotMinP(3), e.slotMinP(17)) == (-1.0, 0.25)
    r.step(16)
    _finish(r, 16)                                            # both end: their columns stop
    assert e.slotMinP(4) == -1.0 and e.slotMinP(17) == -1.0
    for col, b in ((4, 5), (17, 10), (3, 15)):                # utterances at floor 0 take the vacated columns, nothing is set
        r.start(col, b)
        e.slotSetTemperature(col, temps[b])
        assert e.slotMinP(col) == 0.0
    _finish(r, 7)
    e.close()
    r.check(_mixed(MP.COND, precision, mode)["y"], "floor-0 utterances in vacated columns")


@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
def test_list_saves_and_list_resumes_carry_the_floor(pinned):
    """SlotStream: submit(min_p=), set_min_p, suspend_many -- one list save, the device writes word 11 of every header, into device or
    pinned memory --, to_bytes / from_bytes, resume_many in a stream on a second engine: every request's samples are its lockstep
    column's, and SlotState.min_p is the header's."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), [float(np.float32(p)) for p in MP.floors(s.B)]
    y_lock = _mixed(MP.COND, precision, mode)["y"]
    xg = torch.from_numpy(x).cuda()
    e, e2 = _slot_engine(precision, mode, 24), _slot_engine(precision, mode, 24)
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, s.maxD, pcm=False)
    uids = list(range(20))
    hs = {b: st.submit(xg[b], uid=b, temperature=temps[b], min_p=taus[b] if b % 2 else 0.0) for b in uids}
    got = {b: [] for b in uids}

    def step(stream, handles, n):
        for h, (y, _) in stream.step(n).items():
            got[handles[h]].append(y)

    for b in uids[::2]:
        st.set_min_p(hs[b], taus[b])                          # waiting: applied at admission
    step(st, {h: b for b, h in hs.items()}, 5)
    step(st, {h: b for b, h in hs.items()}, 16)
    states = st.suspend_many([hs[b] for b in uids], pinned=pinned)
    torch.cuda.synchronize()
    for b, state in zip(uids, states):
        assert state.min_p == taus[b] and state.temperature == temps[b] and state.done == 21 and state.blob.is_pinned() == pinned
        assert _header(state.blob)[WORD] == MP.bits(taus[b]), b
    back = [SlotState.from_bytes(state.to_bytes(), state.source) if b % 3 == 0 else state for b, state in zip(uids, states)]
    assert [sb.min_p for sb in back] == [taus[b] for b in uids]
    hs2 = dict(zip(st2.resume_many(back), uids))
    assert [st2.min_p(h) for h in hs2] == [taus[b] for b in hs2.values()]
    while st2.busy():
        step(st2, hs2, 5)
        st2.finished()
    st.close(), st2.close()
    e.close(), e2.close()
    for b in uids:
        y = np.concatenate(got[b])
        assert np.array_equal(y, y_lock[b]), "request %d (floor %g) differs from its lockstep column first at %d" % (
            b, taus[b], int(np.nonzero(y != y_lock[b, :len(y)])[0][0]) if len(y) == s.N else len(y))


def test_a_prefilled_state_resumed_with_a_floor_continues_as_the_sequentially_primed_column():
    """submit(prime=, prefill=True, min_p=): the pass leaves word 11 of the blob zero and the stream sets the floor after the resume;
    the samples behind the prime are those of the request that forces the same prime through its column with the same floor."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), MP.floors(s.B)
    xg = torch.from_numpy(x).cuda()
    prime = torch.from_numpy(_mixed(MP.COND, precision, mode)["y"][:, :17].copy()).cuda()
    e = _slot_engine(precision, mode, 24)
    st = SlotStream(e, 2 * s.maxD, pcm=False)
    uids = (3, 4, 5, 8, 9)                                    # floors .25, .5, 0, .25, .5
    seq = {b: st.submit(xg[b], uid=b, temperature=temps[b], prime=prime[b], min_p=taus[b]) for b in uids}
    pre = {b: st.submit(xg[b], uid=b, temperature=temps[b], prime=prime[b], prefill=True, min_p=taus[b]) for b in uids}
    state = st._queue[len(uids)][4]
    assert state.min_p == float(np.float32(taus[3])) and state._blob_sampling.min_p == 0.0 and _header(state.blob)[WORD] == 0
    got = {h: [] for h in list(seq.values()) + list(pre.values())}
    while st.busy():
        for h, (y, _) in st.step(7).items():
            got[h].append(y)
        st.finished()
    st.close()
    e.close()
    plain = _unfloored(MP.COND, precision, mode)["y"]
    for b in uids:
        a, c = np.concatenate(got[seq[b]]), np.concatenate(got[pre[b]])
        assert len(a) == s.N and len(c) == s.N - 17 and np.array_equal(a[:17], prime[b].cpu().numpy())
        assert np.array_equal(a[17:], c), "uid %d (floor %g): the prefilled request differs from the primed one" % (b, taus[b])
    assert any(not np.array_equal(np.concatenate(got[seq[b]]), plain[b]) for b in uids)


# ---- 6. refusals change nothing ----------------------------------------------------------------------------------------------------

def test_refused_floors_change_nothing():
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(MP.COND, precision)
    s = case.shape
    temps, taus = MP.temperatures(s.B), MP.floors(s.B)
    y_lock = _mixed(MP.COND, precision, mode)["y"]
    # lockstep: a refused call leaves the values in force
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps)
    e.setMinP(taus)
    for bad in MP.BAD_FLOORS:
        v = np.array(taus[:-1] + [bad], dtype=np.float32)
        assert not lib.nvw_set_min_p(e._h, v.ctypes.data, s.B)
        with pytest.raises(ValueError):
            e.setMinP(bad)
    v = np.array(taus + [0.0], dtype=np.float32)
    assert not lib.nvw_set_min_p(e._h, v.ctypes.data, s.B + 1) and not lib.nvw_set_min_p(e._h, v.ctypes.data, 0)
    assert not lib.nvw_slot_set_min_p(e._h, 0, 0.25) and lib.nvw_slot_min_p(e._h, 0) == -1.0      # outside slot mode
    assert np.array_equal(_run(e, case, dump=False)["y"], y_lock)
    e.close()
    # slot mode
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    v = np.zeros(s.B, dtype=np.float32)
    assert not lib.nvw_set_min_p(e._h, v.ctypes.data, s.B)                                         # the lockstep call, in slot mode
    for b in (1, 3, 4):
        r.start(_column_of(b, s.B), b)
        e.slotSetTemperature(_column_of(b, s.B), temps[b])
        e.slotSetMinP(_column_of(b, s.B), taus[b])
    r.step(5)
    col = _column_of(3, s.B)
    for bad in MP.BAD_FLOORS:
        assert not lib.nvw_slot_set_min_p(e._h, col, bad)
    assert not lib.nvw_slot_set_min_p(e._h, 5, 0.25)                                               # a column without an utterance
    assert not lib.nvw_slot_set_min_p(e._h, -1, 0.25) and not lib.nvw_slot_set_min_p(e._h, s.B, 0.25)
    assert lib.nvw_slot_min_p(e._h, 5) == -1.0 and lib.nvw_slot_min_p(e._h, s.B) == -1.0 and lib.nvw_slot_min_p(e._h, col) == taus[3]
    _finish(r, 16)
    e.slotsEnd()
    assert lib.nvw_slot_min_p(e._h, col) == -1.0
    e.close()
    r.check(y_lock, "slot mode after refusals")


@pytest.mark.parametrize("mode", ["wg2", "chain"])
def test_runs_that_cannot_honour_a_floor_return_0_and_run_again_at_0(mode):
    """Packed conditioning on wavenet_wg, and a chain engine: with some floor != 0 run() returns 0 and generates nothing; after
    setMinP(None) the same engine runs, and its samples are a fresh engine's."""
    case = cases.BY_NAME["C3_R64S256A256_L20_B16"]
    s = case.shape
    t = util.gen_o1(case, half=True)
    e = util.make_engine(case, t, precision=16, mode=mode)
    fresh = util.make_engine(case, t, precision=16, mode=mode)
    assert ("wavenet_chain" in e.kernelInfo()) == (mode == "chain"), e.kernelInfo()
    e.setMinP([0.0] * (s.B - 1) + [0.05])
    y = np.full((s.B, s.N), -7, dtype=np.int32)
    assert not e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    assert (y == -7).all()
    e.setMinP(None)
    assert e.run(s.N, s.B, y, 1, False)
    y_fresh = np.full((s.B, s.N), -1, dtype=np.int32)
    assert fresh.run(s.N, s.B, y_fresh, 1, False)
    e.synchronize()
    assert np.array_equal(y, y_fresh) and e.chainStatus() == 0
    e.close(), fresh.close()


def test_infer_features_takes_floors_and_infer_refuses_them():
    """NVWaveNetEngine.infer_features(min_p=): a list means column by column, a float every column; columns at floor 0 are the plain
    run's; the engine the wrapper keeps goes back to 0 afterwards; infer(..., min_p=...) raises and points to infer_features."""
    from nv_wavenet_amd import nv_wavenet as NW
    import test_parity_gpu as TP
    s = TC.CASE.shape
    _, dev, cond = TP._wrapper_model(s.R, s.S, s.A, s.L, s.B, s.N)
    g = torch.Generator().manual_seed(23)
    n_cond = 80
    x = torch.randn(s.B, n_cond, s.N, generator=g).cuda()
    cw = ((torch.rand(2 * s.R * s.L, n_cond, 1, generator=g) - 0.5) * (3.46 * 0.5 / np.sqrt(n_cond))).cuda()
    cb = ((torch.rand(2 * s.R * s.L, generator=g) - 0.5) * 0.2).cuda()
    dev["conv_end_weight"] = dev["conv_end_weight"] * 40.0      # (logits of order one: the floor must matter)
    taus = MP.floors(s.B)
    wrapper = NW.NVWaveNetEngine(**dev, precision=32)
    run = lambda **kw: wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, **kw).cpu().numpy()
    plain = run()
    y = run(min_p=taus)
    half = run(min_p=0.5)
    assert np.array_equal(run(min_p=np.float32(0.5)), half) and np.array_equal(run(min_p=torch.tensor(0.5)), half)      # scalars of any kind
    assert np.array_equal(run(), plain)
    with pytest.raises(ValueError, match="infer_features"):
        wrapper.infer(cond.cuda(), NW.Impl.SINGLE_BLOCK, seed=5, min_p=0.1)
    assert wrapper.infer(cond.cuda(), NW.Impl.SINGLE_BLOCK, seed=5).shape == (s.B, s.N)      # the shared engine is back at 0
    for bad in (taus[:-1], [0.6] * s.B, float("nan"), -0.1):
        with pytest.raises(ValueError):
            run(min_p=bad)
    assert np.array_equal(run(), plain)
    wrapper.close()
    assert np.array_equal(y[0::5], plain[0::5]) and not np.array_equal(y[4::5], plain[4::5])
    assert np.array_equal(half[4::5], y[4::5]) and not np.array_equal(half[0], plain[0])
