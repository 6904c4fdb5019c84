"""GPU tests of the tail cuts (top-k and top-p; `-m gpu`).  A column with top-k k and top-p p draws from its tempered
distribution without the bins whose e = exp2(fma(z, c, -(m c))) is below max(theta_k, theta_p, floor).  Off (k = 0 or A, p = 1) is
the run without the feature, bit for bit; a cutting run is held to the engine's OWN scoring pass (scoreSamples(rows=True) at the
column's temperature) by the candidate check of tests/cut_cases.py, with the draws of oracle.philox_selectors_at; the same check
applied to a run made with the cuts off fails.  Shapes, values and DELTA: tests/cut_cases.py (those of tests/min_p_cases.py)."""
import numpy as np
import pytest
import torch

import cases
import cut_cases as CC
import min_p_cases as MP
import score_cases as SC
import temperature_cases as TC
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.slots import SlotState, SlotStream, cut_rows
from oracle import oracle as O
from test_features_gpu import _run
from test_slots_gpu import SEED
from test_slots_mel_gpu import _mel_engine, _mel_inputs
from test_slots_state_gpu import Run, _finish
from test_temperature_gpu import K0, _column_of, _header, _inputs, _seeded, _slot_engine

pytestmark = pytest.mark.gpu

RUNS = [(16, "wg"), (16, "wg2"), (16, "wg3"), (32, "wg"), (32, "wg2")]      # one to three tiles per workgroup (fp32: one and two)
K_WORD, P_WORD = 12, 13                                                      # of a blob's header: top-k, and the bits of top-p (zero: 1)
_cache = {}


def _values(cc):
    s = cases.BY_NAME[cc.case_name].shape
    return CC.top_ks(s.B, s.A), CC.top_ps(s.B), CC.floors(s.B), CC.temperatures(s.B)


def _cut(cc, precision, mode, ks, ps, taus, temps, dump=True):
    """The run under test: column b at temperature temps[b] with floor taus[b], top-k ks[b], top-p ps[b]; once per argument list."""
    key = ("run", cc.name, precision, mode, tuple(ks), tuple(ps), tuple(taus), tuple(temps), dump)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(cc, precision)
        e = _seeded(case, t, precision, mode, m, x, w)
        e.setTemperatures(temps)
        e.setMinP(taus)
        e.setTopK(ks)
        e.setTopP(ps)
        _cache[key] = _run(e, case, dump=dump)
        e.close()
    return _cache[key]


def _mixed(cc, precision, mode):
    return _cut(cc, precision, mode, *_values(cc))


def _uncut(cc, precision, mode):
    """the same floors and temperatures, every cut off"""
    ks, ps, taus, temps = _values(cc)
    return _cut(cc, precision, mode, [0] * len(ks), [1.0] * len(ks), taus, temps)


def _off_columns(cc):
    ks, ps, _, _ = _values(cc)
    A = cases.BY_NAME[cc.case_name].shape.A
    return [b for b in range(len(ks)) if ks[b] in (0, A) and ps[b] == 1.0]


# ---- 1. off is the identity --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", RUNS)
def test_off_is_the_identity_in_lockstep(precision, mode):
    """Never setting a cut, setting every column to off -- before any other value was set and after --, cuts set and taken back,
    and k = A everywhere: the samples, the dumped P and Za of the engine that never heard of the feature, at the mixed floors and
    temperatures.  And a column that is off inside a launch that cuts is its column of the run without cuts, bit for bit."""
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps)
    e.setMinP(taus)
    plain = _run(e, case)
    for prepare in (lambda: (e.setTopK([0] * s.B), e.setTopP([1.0] * s.B)), lambda: (e.setTopK(ks), e.setTopP(ps), e.setTopK(0), e.setTopP(1.0)),
                    lambda: (e.setTopK(4), e.setTopP(0.5), e.setTopK(None), e.setTopP(None)), lambda: e.setTopK([s.A] * s.B)):
        prepare()
        e.resetHistory()
        again = _run(e, case)
        assert np.array_equal(again["y"], plain["y"]) and np.array_equal(again["P"], plain["P"]) and np.array_equal(again["Za"], plain["Za"])
    # the launch mask (Params::floorOn) follows the host's values, each cut alone; a 0-d array or tensor means every column
    assert e.samplerMask() == 3                               # (k = A keeps every bin, and still searches)
    e.setTopK(None)
    assert e.samplerMask() == 1
    for setter, on, off_ in ((e.setTopK, np.array(4), 0), (e.setTopP, np.array(0.5, dtype=np.float32), 1.0), (e.setTopP, torch.tensor(0.5), None),
                             (e.setTopK, torch.tensor(4), None)):
        setter(on)
        assert e.samplerMask() == 3
        setter(off_)
        assert e.samplerMask() == 1
    e.setTopP(np.array(0.5, dtype=np.float32))                # every column, not column 0 alone: the last column's samples change too
    e.resetHistory()
    half = _run(e, case)
    assert not np.array_equal(half["y"][s.B - 1], plain["y"][s.B - 1])
    e.setTopP(None), e.setMinP(None)
    assert e.samplerMask() == 0
    e.close()
    assert np.array_equal(plain["y"], _uncut(CC.COND, precision, mode)["y"])
    # ... and an engine with nothing else set: no table is ever made by values that are off
    e = _seeded(case, t, precision, mode, m, x, w)
    bare = _run(e, case)
    e.setTopK([0] * s.B)
    e.setTopP(1.0)
    e.resetHistory()
    again = _run(e, case)
    e.close()
    assert np.array_equal(again["y"], bare["y"]) and np.array_equal(again["P"], bare["P"])
    # an off column inside a cutting launch
    mixed, off = _mixed(CC.COND, precision, mode), _off_columns(CC.COND)
    assert len(off) >= 4 and s.A in [ks[b] for b in off] and 0 in [ks[b] for b in off]
    for b in off:
        assert np.array_equal(mixed["y"][b], plain["y"][b]) and np.array_equal(mixed["P"][b], plain["P"][b]), b
    assert np.array_equal(mixed["Za"][off], plain["Za"][off])


def _slot_session(precision, mode, variant):
    """A slot session of 12 utterances over three tiles: samples per utterance and, after 21 samples, every column's blob (one list
    save).  variant 0: the cuts are never mentioned; 1: set to off after every start; 2: set and taken back before the step; 3: k = A."""
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    _, _, taus, temps = _values(CC.COND)
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    uids = (0, 1, 2, 3, 4, 7, 16, 21, 22, 33, 38, 39)
    for b in uids:
        r.start(b, b)
        e.slotSetTemperature(b, temps[b])
        e.slotSetMinP(b, taus[b])
        if variant == 1:
            e.slotSetTopK(b, 0), e.slotSetTopP(b, 1.0)
        if variant == 2:
            e.slotSetTopK(b, 4), e.slotSetTopP(b, 0.5), e.slotSetTopK(b, 0), e.slotSetTopP(b, 1.0)
        if variant == 3:
            e.slotSetTopK(b, s.A)
        assert (e.slotTopK(b), e.slotTopP(b)) == (s.A if variant == 3 else 0, 1.0)
    r.step(5)
    r.step(16)
    blobs, saved = e.slotsSaveList(list(uids))
    raw = blobs.cpu().numpy().copy()
    _finish(r, 16)
    e.close()
    return {r.uid_of[k]: np.concatenate(v) for k, v in r.got.items()}, raw


@pytest.mark.parametrize("precision,mode", RUNS)
def test_off_is_the_identity_in_slot_mode(precision, mode):
    y0, blobs0 = _slot_session(precision, mode, 0)
    y_lock = _uncut(CC.COND, precision, mode)["y"]
    for uid, y in y0.items():
        assert np.array_equal(y, y_lock[uid]), uid
    words = blobs0.view("<u4").reshape(len(blobs0), -1)
    assert not words[:, K_WORD].any() and not words[:, P_WORD].any(), "words 12 and 13 of a blob without a cut are zero"
    for variant in (1, 2):
        y, blobs = _slot_session(precision, mode, variant)
        assert all(np.array_equal(y[uid], y0[uid]) for uid in y0), variant
        assert np.array_equal(blobs, blobs0), "variant %d: the blobs differ from those of a session that never heard of the cuts" % variant
    y, blobs = _slot_session(precision, mode, 3)                  # k = A: the same samples; the blob says A
    assert all(np.array_equal(y[uid], y0[uid]) for uid in y0)
    words = blobs.view("<u4").reshape(len(blobs), -1).copy()
    assert (words[:, K_WORD] == 256).all()
    words[:, K_WORD] = 0
    assert np.array_equal(words, blobs0.view("<u4").reshape(len(blobs0), -1))


# ---- 2. the candidate check, against the engine's own scoring pass -----------------------------------------------------------------

def _scored(cc, precision, mode, which):
    """(y [B][N], rows per column [N][A] float32 from scoreSamples at the column's temperature, DELTA per column, u [N][B]) of the
    mixed run (which = "mixed") or of the run with the same floors and temperatures and the cuts off ("uncut")."""
    key = ("scored", cc.name, precision, mode, which)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(cc, precision)
        s = case.shape
        temps = CC.temperatures(s.B)
        y = (_mixed if which == "mixed" else _uncut)(cc, precision, mode)["y"]
        assert y.min() >= 0 and y.max() < s.A
        xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        e = _seeded(case, t, precision, mode, m, x, w)
        got = e.scoreSamples([(yg[b].contiguous(), xg[b], temps[b]) for b in range(s.B)], rows=True)
        e.synchronize()
        rows = [r.cpu().numpy() for _, r in got]
        e.close()
        dlt = []
        for b in range(s.B):
            Za, _ = SC.reference(t, s, y[b], Lh[:, :, b, :])
            dlt.append(CC.delta(temps[b], np.abs(Za).max(), np.abs(rows[b]).max(), s.A))
        k, uid = np.meshgrid(np.arange(s.N), np.arange(s.B), indexing="ij")
        _cache[key] = (y, rows, dlt, O.philox_selectors_at(SEED, k, uid).astype(np.float64))
    return _cache[key]


CHECK_RUNS = [(CC.COND, p, mode) for p, mode in RUNS] + [(CC.COND_A512, 16, "wg"), (CC.COND_A1024, 16, "wg")]


@pytest.mark.parametrize("cc,precision,mode", CHECK_RUNS, ids=lambda v: getattr(v, "name", str(v)))
def test_cut_draws_lie_in_a_candidate_kept_set_and_in_their_bin_of_its_cdf(cc, precision, mode):
    """Free run with the mixed cuts, floors and temperatures, every column's own samples scored by the engine: every sample lies in
    the kept set of a candidate of its row, with u in the picked bin of that candidate's renormalised CDF; no row is left out, and
    at most 10 % of the rows have more than one candidate."""
    y, rows, dlt, u = _scored(cc, precision, mode, "mixed")
    ks, ps, taus, _ = _values(cc)
    tot = CC.check_run(lambda b: rows[b], y, u, ks, ps, taus, lambda b: dlt[b], cut_rows)
    print("%s fp%d/%s: violations %d, rows with more than one candidate %d of %d; DELTA %.2e .. %.2e" % (
        (cc.name, precision, mode) + tot + (min(dlt), max(dlt))))
    assert max(dlt) < 2e-4, dlt
    assert CC.accepted(tot), tot
    assert not np.array_equal(y, _uncut(cc, precision, mode)["y"])


@pytest.mark.parametrize("cc,precision,mode", CHECK_RUNS, ids=lambda v: getattr(v, "name", str(v)))
def test_the_same_check_rejects_a_run_made_with_the_cuts_off(cc, precision, mode):
    """The negative control on the GPU: the run with the same floors and temperatures and no cut, held to the cuts of the mixed run."""
    y, rows, dlt, u = _scored(cc, precision, mode, "uncut")
    ks, ps, taus, _ = _values(cc)
    B = len(ks)
    tot = CC.check_run(lambda b: rows[b], y, u, ks, ps, taus, lambda b: dlt[b], cut_rows)
    print("%s fp%d/%s with the cuts off: violations %d, rows with more than one candidate %d of %d" % ((cc.name, precision, mode) + tot))
    assert not CC.accepted(tot) and tot[0] >= 0.05 * tot[2], tot
    # (held to no cut it passes: the check itself is sound)
    off = CC.check_run(lambda b: rows[b], y, u, [0] * B, [1.0] * B, taus, lambda b: dlt[b], cut_rows)
    assert CC.accepted(off), off


@pytest.mark.parametrize("cc,precision,mode", CHECK_RUNS, ids=lambda v: getattr(v, "name", str(v)))
def test_top_k_one_is_the_argmax_wherever_the_top_gap_exceeds_delta(cc, precision, mode):
    y, rows, dlt, u = _scored(cc, precision, mode, "mixed")
    ks = _values(cc)[0]
    checked = 0
    for b in [b for b in range(len(ks)) if ks[b] == 1]:
        top2 = np.sort(rows[b].astype(np.float64), axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > dlt[b]
        assert np.array_equal(y[b][clear], rows[b].argmax(axis=1)[clear]), b
        checked += int(clear.sum())
    assert checked >= 0.9 * 48 * len([k for k in ks if k == 1]), checked


# ---- 3. exact zeros in the probability dump ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2"), (16, "wg")])
def test_dropped_bins_read_exactly_zero_in_the_probability_dump(precision, mode):
    """Every sample forced by a prime (so the histories agree): getP at the last sample with and without cuts.  Every probability is
    exactly 0 or positive; the zero set is the complement of a candidate kept set of the uncut P; the rest sums to 1 within
    4 A eps32 and is the uncut P renormalised; Za stays the raw logits; the forced samples stay forced."""
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    prime = _mixed(CC.COND, precision, mode)["y"]
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps)
    e.setPrime(prime)
    p0 = _run(e, case)
    e.setMinP(taus), e.setTopK(ks), e.setTopP(ps)
    e.resetHistory()
    p1 = _run(e, case)
    e.close()
    assert np.array_equal(p0["y"], prime) and np.array_equal(p1["y"], prime) and np.array_equal(p0["Za"], p1["Za"])
    dropped = 0
    for b in range(s.B):
        P0, P1 = p0["P"][b].astype(np.float64), p1["P"][b].astype(np.float64)
        assert np.isfinite(P1).all() and (P1 >= 0).all()
        if ks[b] in (0, s.A) and ps[b] == 1.0 and taus[b] == 0.0:
            assert np.array_equal(p0["P"][b], p1["P"][b])
            continue
        with np.errstate(divide="ignore"):
            logp = np.maximum(np.log(P0), -800.0)
        dlt = CC.delta(temps[b], np.abs(p0["Za"][b]).max(), np.abs(logp[P0 > 0]).max(), s.A)
        sets = CC.candidates(logp, ks[b], ps[b], taus[b], dlt)
        keep = P1 > 0
        assert any(np.array_equal(keep, m_) for m_ in sets), "column %d (k %d, p %g, floor %g): the zero set is no candidate's" % (b, ks[b], ps[b], taus[b])
        assert keep[P0.argmax()]
        assert abs(P1.sum() - 1.0) <= 4 * s.A * SC.EPS32, (b, P1.sum())
        assert np.abs(P1[keep] - P0[keep] / P0[keep].sum()).max() <= 4 * s.A * SC.EPS32, b
        if ks[b] == 1:
            assert keep.sum() == 1 or len(sets) > 1
        dropped += int((~keep).sum())
    assert dropped > 100 * s.B, "the cuts dropped next to nothing: the inputs do not exercise the rule"


# ---- 4. slot mode = lockstep -------------------------------------------------------------------------------------------------------

def _set_all(e, col, b, ks, ps, taus, temps):
    e.slotSetTemperature(col, temps[b])
    e.slotSetMinP(col, taus[b])
    e.slotSetTopK(col, ks[b])
    e.slotSetTopP(col, ps[b])


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2"), (16, "wg")])
def test_slot_utterances_reproduce_their_lockstep_columns_with_their_cuts(precision, mode):
    """Utterance b (uid = b and its values) joins at step b mod 4 in column 7 b + 3 mod 40, window = the largest dilation, steps of 5
    and 16 samples: bit for bit column b of the lockstep run of test 2."""
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    y_lock = _mixed(CC.COND, precision, mode)["y"]
    e = _slot_engine(precision, mode)
    assert (e.slotTopK(0), e.slotTopP(0)) == (-1, -1.0)       # outside slot mode
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    assert (e.slotTopK(0), e.slotTopP(0)) == (-1, -1.0)       # no utterance
    for step in range(64):
        for b in range(s.B):
            if b % 4 == step:
                col = _column_of(b, s.B)
                r.start(col, b)
                assert (e.slotTopK(col), e.slotTopP(col)) == (0, 1.0)      # a start puts the column back to off: start, then set
                _set_all(e, col, b, ks, ps, taus, temps)
                assert (e.slotTopK(col), e.slotTopP(col)) == (ks[b], float(np.float32(ps[b])))
        if not r.cols:
            break
        r.step((5, 16)[step % 2])
    e.close()
    assert len(r.got) == s.B and all(len(np.concatenate(v)) == s.N for v in r.got.values())
    r.check(y_lock, "fp%d/%s slot cuts" % (precision, mode))


def test_mel_columns_reproduce_their_lockstep_columns_with_their_cuts():
    """The same for mel utterances (frames upsampled in the steps), against nvw_set_mel + nvw_generate_stream with the lockstep calls."""
    cc = CC.COND
    case, m, mel, up_w, w, t = _mel_inputs(cc, 16)
    s = case.shape
    ks, ps, taus, temps = _values(cc)
    melg = torch.from_numpy(mel).cuda()
    lock = _mel_engine(case, t, 16, "wg2", w, m, up_w, cc.stride, s.B)
    lock.setMel(melg)
    lock.setTemperatures(temps), lock.setMinP(taus), lock.setTopK(ks), lock.setTopP(ps)
    y_lock = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_lock)
    lock.setTopK(None), lock.setTopP(None)
    lock.setMel(melg)                                          # (the floors and temperatures stay in force: the calls leave them alone)
    y_plain = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_plain)
    lock.close()
    off = _off_columns(cc)
    assert np.array_equal(y_lock[off], y_plain[off]) and not np.array_equal(y_lock[1], y_plain[1])
    e = _mel_engine(case, t, 16, "wg2", w, m, up_w, cc.stride, s.B)
    r = Run(e, None, s.maxD, melg=melg, stride=cc.stride)
    for step in range(64):
        for b in range(s.B):
            if b % 4 == step:
                r.start_mel(_column_of(b, s.B), b, s.N // cc.stride)
                _set_all(e, _column_of(b, s.B), b, ks, ps, taus, temps)
        if not r.cols:
            break
        r.step((5, 16)[step % 2])
    e.close()
    assert len(r.got) == s.B
    r.check(y_lock, "mel slot cuts")


def _two_chunks(precision, mode):
    """y [B][N] of: samples [0, K0) with the cuts of the mixed run, the lockstep setters, [K0, N) with the values shifted by two"""
    key = ("chunks", precision, mode)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(CC.COND, precision)
        s = case.shape
        ks, ps, taus, temps = _values(CC.COND)
        kb, pb = CC.top_ks(s.B, s.A, 2), CC.top_ps(s.B, 2)
        e = _seeded(case, t, precision, mode, m, x, w)
        e.setTemperatures(temps), e.setMinP(taus), e.setTopK(ks), e.setTopP(ps)
        y = np.full((s.B, s.N), -1, dtype=np.int32)
        assert e.run_partial_chunk(0, K0, s.N, s.B)
        e.setTopK(kb), e.setTopP(pb)
        assert e.run_partial(K0, s.N, s.B, y, 1, False)
        e.synchronize()
        e.close()
        _cache[key] = (y, kb, pb)
    return _cache[key]


@pytest.mark.parametrize("precision,mode", [(16, "wg2"), (32, "wg")])
def test_cuts_set_between_two_steps_equal_the_lockstep_run_with_the_setters_between_the_chunks(precision, mode):
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    y, kb, pb = _two_chunks(precision, mode)
    one = _mixed(CC.COND, precision, mode)["y"]
    assert np.array_equal(y[:, :K0], one[:, :K0]) and not np.array_equal(y[:, K0:], one[:, K0:])
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    for b in range(s.B):
        col = _column_of(b, s.B)
        r.start(col, b)
        e.slotSetTemperature(col, temps[b]), e.slotSetMinP(col, taus[b])
        assert lib.nvw_slot_set_top_k(e._h, col, ks[b]) and lib.nvw_slot_set_top_p(e._h, col, ps[b])
    for _ in range(K0 // 5):
        r.step(5)
    for b in range(s.B):
        assert lib.nvw_slot_set_top_k(e._h, _column_of(b, s.B), kb[b]) and lib.nvw_slot_set_top_p(e._h, _column_of(b, s.B), pb[b])
    r.step(16)
    _finish(r, 5)
    e.close()
    r.check(y, "fp%d/%s cuts set at local sample %d" % (precision, mode, K0))


# ---- 5. the state carries the cuts -------------------------------------------------------------------------------------------------

def _words(blob):
    h = _header(blob)
    return int(h[K_WORD]), int(h[P_WORD])


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2")])
def test_moves_saves_and_resumes_carry_the_cuts(precision, mode):
    """After some steps: slotMove across tiles, slotSave + slotResume into another column of a second engine -- both continue bit for
    bit; header words 12 and 13 hold top-k and the bits of top-p, zero for off; damaged words are refused with nothing changed."""
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    p32 = [float(np.float32(p)) for p in ps]
    y_lock = _mixed(CC.COND, precision, mode)["y"]
    xg = torch.from_numpy(x).cuda()
    e = _slot_engine(precision, mode)
    r = Run(e, xg, s.maxD)
    for b in (0, 1, 2, 3, 4, 7, 21, 38):                     # (k, p): (0,1) (1,.5) (4,.8) (32,.9) (A,1) (4,.9) (1,.5) (32,.8)
        r.start(b + 1, b)
        _set_all(e, b + 1, b, ks, ps, taus, temps)
    r.step(5)
    r.step(16)
    r.move(5, 30)                                             # uid 4 (k = A) across tiles
    r.move(39, 0)                                             # uid 38 (32, 0.8) into the first tile
    assert (e.slotTopK(30), e.slotTopK(0), e.slotTopK(5), e.slotTopK(39)) == (s.A, 32, -1, -1)
    assert (e.slotTopP(30), e.slotTopP(0), e.slotTopP(5), e.slotTopP(39)) == (1.0, p32[38], -1.0, -1.0)
    r.start(5, 9)                                             # the move's source takes a new utterance: back to off
    assert (e.slotTopK(5), e.slotTopP(5)) == (0, 1.0)
    e.slotStop(5)
    del r.cols[5], r.got[len(r.got) - 1]
    r.step(5)
    e2 = _slot_engine(precision, mode, 24)
    r2 = Run(e2, xg, 2 * s.maxD, into=r)
    r2.start(3, 6)                                            # uid 6: (1, 0.8)
    _set_all(e2, 3, 6, ks, ps, taus, temps)
    r2.step(7)
    for col, uid, to in ((4, 3, 17), (1, 0, 0), (2, 1, 5)):
        blob, rec = r.suspend(col)
        h = _header(blob)
        assert _words(blob) == (ks[uid], CC.p_bits(p32[uid])) and not h[14:].any() and (h[6], h[7]) == (26, uid)
        r2.resume(to, blob, rec)
        assert (e2.slotTopK(to), e2.slotTopP(to), e2.slotMinP(to)) == (ks[uid], p32[uid], float(np.float32(taus[uid]))) and e.slotTopK(col) == -1
    blob, rec = r.suspend(8)                                  # uid 7: (4, 0.9)
    bits = lambda v: int(np.array([v], dtype="<f4").view("<u4")[0])
    for word, value in ((K_WORD, s.A + 1), (K_WORD, 0xFFFFFFFF), (K_WORD, 0x80000000), (P_WORD, bits(1.0)), (P_WORD, bits(1.5)), (P_WORD, bits(-0.5)),
                        (P_WORD, bits(float("nan"))), (P_WORD, bits(float("inf"))), (P_WORD, 0x80000000)):
        bad = blob.clone()
        bad[4 * word:4 * word + 4] = torch.from_numpy(np.array([value], dtype="<u4").view(np.uint8).copy()).cuda()
        assert not lib.nvw_slot_resume(e2._h, 9, bad.data_ptr(), xg[7].data_ptr(), 32, xg[7].stride(0), xg[7].stride(1), s.N)
        assert (e2.slotTopK(9), e2.slotTopP(9), e2.slotTemperature(9)) == (-1, -1.0, 0.0)
    r2.resume(9, blob, rec)
    assert (e2.slotTopK(9), e2.slotTopP(9)) == (4, p32[7])
    _finish(r, 16)
    _finish(r2, 5)
    e.close(), e2.close()
    assert len(r.got) == 9
    r.check(y_lock, "fp%d/%s moved, saved and resumed" % (precision, mode))


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2")])
def test_resumes_into_the_engine_that_saved_them_take_the_cuts_of_the_blob(precision, mode):
    """Saved blobs go back into columns of the SAME engine that held other utterances before, singly (slotResume) and as a list
    (slotsSaveList + slotsResumeList): the column's cuts are the blob's, whatever its table entries held, and every utterance
    continues bit for bit as its lockstep column."""
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    p32 = [float(np.float32(p)) for p in ps]
    y_lock = _mixed(CC.COND, precision, mode)["y"]
    xg = torch.from_numpy(x).cuda()
    e = _slot_engine(precision, mode)
    r = Run(e, xg, s.maxD)
    for b in (0, 1, 2, 3, 4, 7, 8):                          # in columns b + 1
        r.start(b + 1, b)
        _set_all(e, b + 1, b, ks, ps, taus, temps)
    r.step(5)
    r.step(16)
    saved = {uid: r.suspend(uid + 1) for uid in (0, 4, 3, 8)}
    for uid, to in ((0, 5), (4, 1), (3, 9), (8, 20)):        # off into the column that held k = A, k = A into one that was off, ...
        blob, rec = saved[uid]
        assert _words(blob) == (ks[uid], CC.p_bits(p32[uid])) and e.slotTopK(to) == -1
        r.resume(to, blob, rec)
        assert (e.slotTopK(to), e.slotTopP(to)) == (ks[uid], p32[uid])
    r.step(5)
    cols, to = [2, 3, 8], [8, 2, 3]                          # as a list: uids 1, 2, 7 change places
    blobs, rec = e.slotsSaveList(cols)
    assert [int(v) for v in rec["uid"]] == [1, 2, 7] and [int(v) for v in rec["done"]] == [26, 26, 26]
    words = blobs.cpu().numpy().view("<u4").reshape(3, -1)
    assert [(int(a), int(b)) for a, b in words[:, [K_WORD, P_WORD]]] == [(ks[u], CC.p_bits(p32[u])) for u in (1, 2, 7)]
    recs = []
    for col in cols:
        e.slotStop(col)
        recs.append(r.cols.pop(col))
        assert (e.slotTopK(col), e.slotTopP(col)) == (-1, -1.0)
    e.slotsResumeList(to, blobs, [xg[1], xg[2], xg[7]])
    for col, uid, one in zip(to, (1, 2, 7), recs):
        r.cols[col] = one
        assert (e.slotTopK(col), e.slotTopP(col)) == (ks[uid], p32[uid])
    r.step(5)
    again, _ = e.slotsSaveList(to)                            # the saves of the resumed columns carry the cuts on
    words = again.cpu().numpy().view("<u4").reshape(3, -1)
    assert [(int(a), int(b)) for a, b in words[:, [K_WORD, P_WORD]]] == [(ks[u], CC.p_bits(p32[u])) for u in (1, 2, 7)]
    _finish(r, 16)
    e.close()
    assert len(r.got) == 7 and all(len(np.concatenate(v)) == s.N for v in r.got.values())
    r.check(y_lock, "fp%d/%s resumed into the engine that saved them" % (precision, mode))


def test_a_session_whose_cutting_utterances_have_ended_launches_without_the_search_again():
    """slotStop and slotMove leave no cut behind in the column they vacate: the getters of the idle column say -1, the next utterance
    there starts off and reproduces its column of the run without cuts."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    xg = torch.from_numpy(x).cuda()
    e = _slot_engine(precision, mode)
    r = Run(e, xg, s.maxD)
    for b in (2, 3):
        r.start(b, b)
        _set_all(e, b, b, ks, ps, taus, temps)
    assert e.samplerMask() & 2                                # (bit 1 of Params::floorOn: the launches search)
    r.step(5)
    r.move(3, 17)
    assert (e.slotTopK(3), e.slotTopK(17), e.slotTopP(17)) == (-1, 32, float(np.float32(0.9)))
    assert e.samplerMask() & 2
    r.step(16)
    _finish(r, 16)                                            # both end: their columns stop
    assert e.slotTopK(2) == -1 and e.slotTopK(17) == -1 and e.slotTopP(17) == -1.0
    assert e.samplerMask() == 0, "a count of cutting or floored columns leaked: every later launch would search"
    for col, b in ((2, 5), (17, 10), (3, 15)):                # utterances without cuts take the vacated columns, no cut is set
        r.start(col, b)
        e.slotSetTemperature(col, temps[b]), e.slotSetMinP(col, taus[b])
        assert (e.slotTopK(col), e.slotTopP(col)) == (0, 1.0)
    assert e.samplerMask() == 1                               # (their floors only: the launches the parent issues for them)
    _finish(r, 7)
    assert e.samplerMask() == 0
    e.close()
    r.check(_mixed(CC.COND, precision, mode)["y"], "the cutting utterances", only=(0, 1))
    r.check(_uncut(CC.COND, precision, mode)["y"], "utterances without cuts in vacated columns", only=(2, 3, 4))


def _bare(cc, precision, mode):
    """the run of a fresh engine with nothing set, once"""
    key = ("bare", cc.name, precision, mode)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(cc, precision)
        e = _seeded(case, t, precision, mode, m, x, w)
        _cache[key] = _run(e, case)
        e.close()
    return _cache[key]


def test_mode_changes_leave_no_value_behind():
    """One engine: lockstep with all four values in every column; a slot session begun over them, whose utterances run with every
    value off until theirs are set; the session ended while a set column still waits for its step; lockstep again with nothing set.
    Each change of mode puts the host's values and the device table back to off."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    xg = torch.from_numpy(x).cuda()
    bare = _bare(CC.COND, precision, mode)
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps), e.setMinP(taus), e.setTopK(ks), e.setTopP(ps)
    assert e.samplerMask() == 3
    assert np.array_equal(_run(e, case, dump=False)["y"], _mixed(CC.COND, precision, mode)["y"])
    r = Run(e, xg, s.maxD)                                    # slotsBegin over the lockstep values
    assert e.samplerMask() == 0
    uids = (2, 7, 17, 0)                                      # (the first three: all four values on; their columns' lockstep T was not 1)
    cols = [_column_of(b, s.B) for b in uids]
    assert all(temps[c] != 1.0 for c in cols) and all(ks[b] and ps[b] != 1.0 and taus[b] and temps[b] != 1.0 for b in uids[:3])
    for col, b in zip(cols, uids):
        r.start(col, b)
    assert e.samplerMask() == 0
    r.step(5)
    r.check(bare["y"], "begun over lockstep values, nothing set")
    for col, b in zip(cols[:2], uids[:2]):
        _set_all(e, col, b, ks, ps, taus, temps)
    r.step(5)
    r.check(bare["y"], "the columns nothing was set in", only=(2, 3))
    _set_all(e, cols[2], uids[2], ks, ps, taus, temps)        # no step follows: the column is still to be written at the end
    assert e.samplerMask() == 3
    e.slotsEnd()
    assert e.samplerMask() == 0
    e.setFeatures(xg)
    again = _run(e, case)
    assert e.samplerMask() == 0
    e.close()
    assert np.array_equal(again["y"], bare["y"]) and np.array_equal(again["P"], bare["P"]) and np.array_equal(again["Za"], bare["Za"])


@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
def test_list_saves_and_list_resumes_carry_the_cuts(pinned):
    """SlotStream: submit(top_k=, top_p=), set_top_k / set_top_p, suspend_many -- one list save, the device writes words 12 and 13 of
    every header, into device or pinned memory --, to_bytes / from_bytes, resume_many in a stream on a second engine: every request's
    samples are its lockstep column's, and SlotState.top_k / top_p are the header's."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    p32 = [float(np.float32(p)) for p in ps]
    y_lock = _mixed(CC.COND, precision, mode)["y"]
    xg = torch.from_numpy(x).cuda()
    e, e2 = _slot_engine(precision, mode, 24), _slot_engine(precision, mode, 24)
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, s.maxD, pcm=False)
    uids = list(range(20))
    hs = {b: st.submit(xg[b], uid=b, temperature=temps[b], min_p=taus[b], **(dict(top_k=ks[b], top_p=ps[b]) if b % 2 else {})) for b in uids}
    got = {b: [] for b in uids}

    def step(stream, handles, n):
        for h, (y, _) in stream.step(n).items():
            got[handles[h]].append(y)

    for b in uids[::2]:
        st.set_top_k(hs[b], ks[b]), st.set_top_p(hs[b], ps[b])          # waiting: applied at admission
    step(st, {h: b for b, h in hs.items()}, 5)
    step(st, {h: b for b, h in hs.items()}, 16)
    states = st.suspend_many([hs[b] for b in uids], pinned=pinned)
    torch.cuda.synchronize()
    for b, state in zip(uids, states):
        assert (state.top_k, state.top_p, state.done) == (ks[b], p32[b], 21) and state.blob.is_pinned() == pinned
        assert _words(state.blob) == (ks[b], CC.p_bits(p32[b])), b
    back = [SlotState.from_bytes(state.to_bytes(), state.source) if b % 3 == 0 else state for b, state in zip(uids, states)]
    assert [(sb.top_k, sb.top_p) for sb in back] == [(ks[b], p32[b]) for b in uids]
    hs2 = dict(zip(st2.resume_many(back), uids))
    assert [(st2.top_k(h), st2.top_p(h)) for h in hs2] == [(ks[b], p32[b]) for b in hs2.values()]
    while st2.busy():
        step(st2, hs2, 5)
        st2.finished()
    st.close(), st2.close()
    e.close(), e2.close()
    for b in uids:
        y = np.concatenate(got[b])
        assert np.array_equal(y, y_lock[b]), "request %d (k %d, p %g) differs from its lockstep column first at %d" % (
            b, ks[b], ps[b], int(np.nonzero(y != y_lock[b, :len(y)])[0][0]) if len(y) == s.N else len(y))


def test_a_list_save_without_a_cut_leaves_words_12_and_13_zero_after_one_with():
    """the parallel array of a list save is NULL when no saved column has a cut: blobs of such columns are the bytes they were, also
    right after a list save that carried cuts through the same staging"""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    for b in (0, 1, 2, 3):
        r.start(b, b)
    e.slotSetTopK(2, 7), e.slotSetTopP(3, 0.25)
    r.step(5)
    with_cuts, _ = e.slotsSaveList([2, 3, 0])
    without, _ = e.slotsSaveList([0, 1])
    e.close()
    w1, w0 = with_cuts.cpu().numpy().view("<u4").reshape(3, -1), without.cpu().numpy().view("<u4").reshape(2, -1)
    assert [(int(a), int(b)) for a, b in w1[:, [K_WORD, P_WORD]]] == [(7, 0), (0, CC.p_bits(0.25)), (0, 0)]
    assert not w0[:, 10:16].any() and np.array_equal(w0[0], w1[2])


def test_a_prefilled_state_resumed_with_cuts_continues_as_the_sequentially_primed_column():
    """submit(prime=, prefill=True, top_k=, top_p=): the pass leaves words 12 and 13 of the blob zero and the stream sets the cuts
    after the resume; the samples behind the prime are those of the request that forces the same prime through its column."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    xg = torch.from_numpy(x).cuda()
    prime = torch.from_numpy(_mixed(CC.COND, precision, mode)["y"][:, :17].copy()).cuda()
    e = _slot_engine(precision, mode, 24)
    st = SlotStream(e, 2 * s.maxD, pcm=False)
    uids = (1, 2, 3, 5, 6)
    kw = lambda b: dict(uid=b, temperature=temps[b], prime=prime[b], min_p=taus[b], top_k=ks[b], top_p=ps[b])
    seq = {b: st.submit(xg[b], **kw(b)) for b in uids}
    pre = {b: st.submit(xg[b], prefill=True, **kw(b)) for b in uids}
    state = st._queue[len(uids)][4]
    assert (state.top_k, state.top_p) == (1, 0.5) and state._blob_sampling[2:] == (0, 1.0) and _words(state.blob) == (0, 0)
    got = {h: [] for h in list(seq.values()) + list(pre.values())}
    while st.busy():
        for h, (y, _) in st.step(7).items():
            got[h].append(y)
        st.finished()
    st.close()
    e.close()
    y_lock = _mixed(CC.COND, precision, mode)["y"]
    for b in uids:
        a, c = np.concatenate(got[seq[b]]), np.concatenate(got[pre[b]])
        assert len(a) == s.N and len(c) == s.N - 17 and np.array_equal(a, y_lock[b])
        assert np.array_equal(a[17:], c), "uid %d: the prefilled request differs from the primed one" % b


# ---- 6. refusals change nothing ----------------------------------------------------------------------------------------------------

def test_refused_cuts_change_nothing():
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(CC.COND, precision)
    s = case.shape
    ks, ps, taus, temps = _values(CC.COND)
    y_lock = _mixed(CC.COND, precision, mode)["y"]
    bad_ks = (-1, s.A + 1, 2 ** 31 - 1, -2 ** 31)
    # lockstep: a refused call leaves the values in force
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps), e.setMinP(taus), e.setTopK(ks), e.setTopP(ps)
    for bad in bad_ks:
        v = np.array(ks[:-1] + [bad], dtype=np.int32)
        assert not lib.nvw_set_top_k(e._h, v.ctypes.data, s.B)
        with pytest.raises(ValueError):
            e.setTopK(bad)
    for bad in (2.5, "many", 2 ** 40):
        with pytest.raises(ValueError):
            e.setTopK(bad)
    for bad in CC.BAD_TOP_PS:
        v = np.array(ps[:-1] + [bad], dtype=np.float32)
        assert not lib.nvw_set_top_p(e._h, v.ctypes.data, s.B)
        with pytest.raises(ValueError):
            e.setTopP(bad)
    vk, vp = np.array(ks + [0], dtype=np.int32), np.array(ps + [1.0], dtype=np.float32)
    assert not lib.nvw_set_top_k(e._h, vk.ctypes.data, s.B + 1) and not lib.nvw_set_top_k(e._h, vk.ctypes.data, 0)
    assert not lib.nvw_set_top_p(e._h, vp.ctypes.data, s.B + 1) and not lib.nvw_set_top_p(e._h, vp.ctypes.data, 0)
    assert not lib.nvw_slot_set_top_k(e._h, 0, 4) and not lib.nvw_slot_set_top_p(e._h, 0, 0.5)          # outside slot mode
    assert lib.nvw_slot_top_k(e._h, 0) == -1 and lib.nvw_slot_top_p(e._h, 0) == -1.0
    assert np.array_equal(_run(e, case, dump=False)["y"], y_lock)
    e.close()
    # slot mode
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    assert not lib.nvw_set_top_k(e._h, vk.ctypes.data, s.B) and not lib.nvw_set_top_p(e._h, vp.ctypes.data, s.B)      # the lockstep calls, in slot mode
    for b in (1, 2, 3):
        r.start(_column_of(b, s.B), b)
        _set_all(e, _column_of(b, s.B), b, ks, ps, taus, temps)
    r.step(5)
    col = _column_of(3, s.B)
    for bad in bad_ks:
        assert not lib.nvw_slot_set_top_k(e._h, col, bad)
    for bad in CC.BAD_TOP_PS:
        assert not lib.nvw_slot_set_top_p(e._h, col, bad)
    assert not lib.nvw_slot_set_top_k(e._h, 5, 4) and not lib.nvw_slot_set_top_p(e._h, 5, 0.5)           # a column without an utterance
    assert not lib.nvw_slot_set_top_k(e._h, -1, 4) and not lib.nvw_slot_set_top_k(e._h, s.B, 4)
    assert not lib.nvw_slot_set_top_p(e._h, -1, 0.5) and not lib.nvw_slot_set_top_p(e._h, s.B, 0.5)
    assert lib.nvw_slot_top_k(e._h, 5) == -1 and lib.nvw_slot_top_k(e._h, s.B) == -1 and lib.nvw_slot_top_k(e._h, col) == 32
    assert lib.nvw_slot_top_p(e._h, 5) == -1.0 and lib.nvw_slot_top_p(e._h, col) == float(np.float32(0.9))
    _finish(r, 16)
    e.slotsEnd()
    assert lib.nvw_slot_top_k(e._h, col) == -1 and lib.nvw_slot_top_p(e._h, col) == -1.0
    e.close()
    r.check(y_lock, "slot mode after refusals")


@pytest.mark.parametrize("mode,cut", [("wg2", "k"), ("wg2", "p"), ("chain", "k"), ("chain", "p")])
def test_runs_that_cannot_honour_a_cut_return_0_and_run_again_without(mode, cut):
    """Packed conditioning on wavenet_wg, and a chain engine: with a cut in some column run() returns 0 and generates nothing; after
    the cut is taken back the same engine runs, and its samples are a fresh engine's."""
    case = cases.BY_NAME["C3_R64S256A256_L20_B16"]
    s = case.shape
    t = util.gen_o1(case, half=True)
    e = util.make_engine(case, t, precision=16, mode=mode)
    fresh = util.make_engine(case, t, precision=16, mode=mode)
    assert ("wavenet_chain" in e.kernelInfo()) == (mode == "chain"), e.kernelInfo()
    if cut == "k":
        e.setTopK([0] * (s.B - 1) + [5])
    else:
        e.setTopP([1.0] * (s.B - 1) + [0.9])
    y = np.full((s.B, s.N), -7, dtype=np.int32)
    assert not e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    assert (y == -7).all()
    e.setTopK(None) if cut == "k" else e.setTopP(None)
    assert e.run(s.N, s.B, y, 1, False)
    y_fresh = np.full((s.B, s.N), -1, dtype=np.int32)
    assert fresh.run(s.N, s.B, y_fresh, 1, False)
    e.synchronize()
    assert np.array_equal(y, y_fresh) and e.chainStatus() == 0
    e.close(), fresh.close()


def test_infer_features_takes_cuts_and_infer_refuses_them():
    """NVWaveNetEngine.infer_features(top_k=, top_p=): a list means column by column, a scalar every column; columns that are off are
    the plain run's; the engine the wrapper keeps goes back to off afterwards; infer(..., top_k= / top_p=) raises and points to
    infer_features."""
    from nv_wavenet_amd import nv_wavenet as NW
    import test_parity_gpu as TP
    s = TC.CASE.shape
    _, dev, cond = TP._wrapper_model(s.R, s.S, s.A, s.L, s.B, s.N)
    g = torch.Generator().manual_seed(23)
    n_cond = 80
    x = torch.randn(s.B, n_cond, s.N, generator=g).cuda()
    cw = ((torch.rand(2 * s.R * s.L, n_cond, 1, generator=g) - 0.5) * (3.46 * 0.5 / np.sqrt(n_cond))).cuda()
    cb = ((torch.rand(2 * s.R * s.L, generator=g) - 0.5) * 0.2).cuda()
    dev["conv_end_weight"] = dev["conv_end_weight"] * 40.0      # (logits of order one: the cuts must matter)
    ks, ps = CC.top_ks(s.B, s.A), CC.top_ps(s.B)
    wrapper = NW.NVWaveNetEngine(**dev, precision=32)
    run = lambda **kw: wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, **kw).cpu().numpy()
    plain = run()
    y = run(top_k=ks, top_p=ps)
    greedy = run(top_k=1)
    assert np.array_equal(run(top_k=np.int32(1)), greedy) and np.array_equal(run(top_k=torch.tensor(1)), greedy)      # scalars of any kind
    half = run(top_p=0.5)
    assert np.array_equal(run(top_p=np.float32(0.5)), half) and np.array_equal(run(top_p=torch.tensor(0.5)), half)
    assert np.array_equal(run(), plain)
    for kw in (dict(top_k=4), dict(top_p=0.9)):
        with pytest.raises(ValueError, match="infer_features"):
            wrapper.infer(cond.cuda(), NW.Impl.SINGLE_BLOCK, seed=5, **kw)
    assert wrapper.infer(cond.cuda(), NW.Impl.SINGLE_BLOCK, seed=5).shape == (s.B, s.N)      # the shared engine is back to off
    for kw in (dict(top_k=ks[:-1]), dict(top_k=[s.A + 1] * s.B), dict(top_k=-1), dict(top_k=1.5), dict(top_p=ps[:-1]), dict(top_p=[1.5] * s.B),
               dict(top_p=float("nan")), dict(top_p=0.0)):
        with pytest.raises(ValueError):
            run(**kw)
    assert np.array_equal(run(), plain)
    wrapper.close()
    off = [b for b in range(s.B) if ks[b] in (0, s.A) and ps[b] == 1.0]
    assert np.array_equal(y[off], plain[off]) and not np.array_equal(y[1], plain[1])
    assert not np.array_equal(greedy, plain) and not np.array_equal(half, plain)
    both = [b for b in range(s.B) if ks[b] == 1]
    assert np.array_equal(y[both], greedy[both])                 # top-k 1 is the argmax whatever top-p says
