"""GPU tests of the sampling temperature (`-m gpu`).  The softmax of wavenet_wg<.., RAW = 3> computes
exp2(x c - m c) with c = log2(e) / T per column.  Two exact properties carry the tests: T = 1 gives c = log2(e), so a run at
T = 1 is bit for bit the run without the feature; and for T a power of two c and m c are exact scalings, so column b of a run at
T_b equals, bit for bit, column b of the same engine with Wza / T_b and Bza / T_b handed to setOutWeights and no temperature (the
logits are Wza zs + Bza, scaled as a whole).  Other temperatures are held to the teacher-forced fp32 oracle given the scaled
weights, by the bars the features path is held to.  Shapes: tests/temperature_cases.py."""
import copy

import numpy as np
import pytest
import torch

import cases
import condgen
import temperature_cases as TC
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.slots import SlotState, SlotStream
from oracle import oracle as O
from test_features_gpu import _cond_inputs, _feature_engine, _run
from test_slots_gpu import SEED, _engine
from test_slots_mel_gpu import _mel_engine, _mel_inputs
from test_slots_state_gpu import Run, _finish

pytestmark = pytest.mark.gpu

RUNS = [(16, "wg"), (16, "wg2"), (16, "wg3"), (32, "wg"), (32, "wg2")]      # one to three tiles per workgroup (fp32: one and two)
WORD = 10                                                                    # of a blob's header: the bits of T, zero for T = 1
_cache = {}


def _bits(T):
    return int(np.array([T], dtype="<f4").view("<u4")[0])


def _scaled(t, T):
    """The model with Wza / T and Bza / T (fp32 division: exact for the powers of two)."""
    t2 = copy.copy(t)
    t2.Wza = (t.Wza / np.float32(T)).astype(np.float32)
    t2.Bza = (t.Bza / np.float32(T)).astype(np.float32)
    return t2


def _inputs(cc, precision):
    """(case, cond model, features x, cond weight w, Lh, network t) of a temperature case, once per (case, precision).  fp16: the
    nonzero |Wza| lie in [2^-10, 2^4] (smaller ones are zeroed), so that Wza / T is exact in half precision for every T of
    TC.POWERS -- asserted here, on the host."""
    key = ("inputs", cc.name, precision)
    if key not in _cache:
        half = precision == 16
        case, m, x, w, Lh = _cond_inputs(cc, half=half)
        t = util.gen_o1(case, half=half)
        if half:
            t.Wza[np.abs(t.Wza) < 2.0 ** -10] = 0
            nz = np.abs(t.Wza[t.Wza != 0])
            assert nz.min() >= 2.0 ** -10 and nz.max() <= 2.0 ** 4
            for T in TC.POWERS:
                sw = _scaled(t, T).Wza
                assert np.array_equal(sw.astype(np.float16).astype(np.float32), sw) and np.array_equal(sw * np.float32(T), t.Wza)
        t.sel = O.philox_selectors(SEED, case.shape.N, case.shape.B)
        t.Lh = Lh
        _cache[key] = (case, m, x, w, Lh, t)
    return _cache[key]


def _seeded(case, t, precision, mode, m, x, w):
    """The features-path engine of test_features_gpu with in-kernel selectors (the lockstep run slot mode reproduces)."""
    e = _feature_engine(case, t, precision, mode, m, x, w)
    e.setSelectorSeed(SEED)
    assert "RAW=3" in e.kernelInfo(), e.kernelInfo()
    return e


def _reference(cc, precision, mode, T):
    """y [B][N] and the dumped activations of the engine with Wza / T, Bza / T and no temperature, once per (case, precision, mode, T)."""
    key = ("ref", cc.name, precision, mode, T)
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(cc, precision)
        e = _seeded(case, _scaled(t, T), precision, mode, m, x, w)
        _cache[key] = _run(e, case)
        e.close()
    return _cache[key]


def _tempered(cc, precision, mode, temps):
    """The run under test: the unscaled model, column b at temps[b]; once per (case, precision, mode, temps)."""
    key = ("run", cc.name, precision, mode, tuple(temps))
    if key not in _cache:
        case, m, x, w, Lh, t = _inputs(cc, precision)
        e = _seeded(case, t, precision, mode, m, x, w)
        e.setTemperatures(temps)
        _cache[key] = _run(e, case)
        e.close()
    return _cache[key]


def _by_column(refs, temps, keys=("Xout", "skipOut", "Zs", "Za", "P", "y", "lo", "hi")):
    """One result whose column b is column b of refs[temps[b]] (Xout / skipOut: [L][B][..], the others [B][..])."""
    out = {}
    first = refs[temps[0]]
    for k in keys:
        if k not in first:
            continue
        a = np.array(first[k], copy=True)
        for b, T in enumerate(temps):
            if k in ("Xout", "skipOut"):
                a[:, b] = refs[T][k][:, b]
            else:
                a[b] = refs[T][k][b]
        out[k] = a
    return out


def _assert_columns_equal(got, temps, ref_of, what, keys=("y", "P")):
    for b, T in enumerate(temps):
        for k in keys:
            assert np.array_equal(got[k][b], ref_of(T)[k][b]), "%s: column %d at T = %g: %s differs from the engine with Wza / T, Bza / T" % (what, b, T, k)


# ---- 1. unit temperature is the identity -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", RUNS)
def test_unit_temperature_is_the_identity(precision, mode):
    """setTemperatures with all ones -- before any other value was set (no table exists, Params::softScale is NULL) and after one
    was (the table exists and holds log2(e) in every entry) -- gives the samples and the dumped P of the run without the call."""
    case, m, x, w, Lh, t = _inputs(TC.COND, precision)
    s = case.shape
    e = _seeded(case, t, precision, mode, m, x, w)
    plain = _run(e, case)
    for prepare in (lambda: None, lambda: e.setTemperatures([0.5] * s.B)):
        prepare()
        e.setTemperatures([1.0] * s.B)
        e.resetHistory()
        again = _run(e, case)
        assert np.array_equal(again["y"], plain["y"]) and np.array_equal(again["P"], plain["P"]) and np.array_equal(again["Za"], plain["Za"])
    e.close()
    _cache[("plain", precision, mode)] = plain["y"]


# ---- 2. powers of two are exact ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", RUNS)
def test_powers_of_two_equal_the_scaled_weights_bit_for_bit(precision, mode):
    """Column b at T_b = (1/4, 1/2, 1, 2, 4)[b mod 5]: samples over all 48 steps and the dumped P equal column b of the engine with
    Wza / T_b, Bza / T_b; Za stays the raw logits (the reference's times T_b, exactly).  fp32: also held to the oracle given the
    scaled weights, by the helper and bars of the features path (tests/test_features_gpu.py)."""
    cc = TC.COND
    case, m, x, w, Lh, t = _inputs(cc, precision)
    s = case.shape
    temps = TC.power_temperatures(s.B)
    got = _tempered(cc, precision, mode, temps)
    _assert_columns_equal(got, temps, lambda T: _reference(cc, precision, mode, T), "fp%d/%s" % (precision, mode))
    for b, T in enumerate(temps):
        assert np.array_equal(got["Za"][b], _reference(cc, precision, mode, T)["Za"][b] * np.float32(T)), "Za must stay the raw logits"
    assert len({got["y"][b].tobytes() for b in range(5)}) == 5 and not np.array_equal(got["y"], _reference(cc, precision, mode, 1.0)["y"])
    if precision == 32:
        key = ("oracle", cc.name, got["y"].tobytes())
        if key not in _cache:
            _cache[key] = _by_column({T: util.teacher_forced_oracle(case, _scaled(t, T), got["y"]) for T in TC.POWERS}, temps)
        ref = _cache[key]
        _, unexplained = util.explain_mismatches(ref["y"], got["y"], ref["lo"], ref["hi"], t.sel.T, 1e-5)
        assert not unexplained, "unexplained sample mismatches (b,t,ref,got,edge distance): %s" % unexplained[:5]
        assert (ref["y"] == got["y"]).mean() >= 0.999
        scaled = dict(got, Za=got["Za"] / np.array(temps, dtype=np.float32)[:, None])
        util.compare_activations(ref, scaled, atol_eps=32)


@pytest.mark.parametrize("cc", [TC.COND_A512, TC.COND_A1024], ids=lambda c: c.name)
def test_powers_of_two_in_the_other_softmax_lane_layouts(cc):
    """fp16, A = 512 and A = 1024 (B = 16): other numbers of lanes per utterance and rows per lane in softmax_pick."""
    case, m, x, w, Lh, t = _inputs(cc, 16)
    temps = TC.power_temperatures(case.shape.B)
    got = _tempered(cc, 16, "wg", temps)
    _assert_columns_equal(got, temps, lambda T: _reference(cc, 16, "wg", T), cc.name)


# ---- 3. other temperatures ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(32, "wg2"), (16, "wg3")])
def test_other_temperatures_are_held_to_the_oracle_with_the_scaled_weights(precision, mode):
    """T = 0.8 in the even columns, 1.3 in the odd ones: the dumped P, and Za times 1 / T, against the teacher-forced oracle given
    Wza / T, Bza / T -- fp32 by util.compare_activations(atol_eps=32) as smoke() does on these inputs, fp16 by util.fp16_bars."""
    cc = TC.COND
    case, m, x, w, Lh, t = _inputs(cc, precision)
    s = case.shape
    temps = [float(np.float32((0.8, 1.3)[b % 2])) for b in range(s.B)]
    got = _tempered(cc, precision, mode, temps)
    plain = _reference(cc, precision, mode, 1.0)
    assert not np.array_equal(got["y"][0], plain["y"][0]) and not np.array_equal(got["y"][1], plain["y"][1])
    ref = _by_column({T: util.teacher_forced_oracle(case, _scaled(t, T), got["y"]) for T in sorted(set(temps))}, temps)
    scaled = dict(got, Za=got["Za"] * (np.float32(1.0) / np.array(temps, dtype=np.float32))[:, None])
    if precision == 32:
        _, unexplained = util.explain_mismatches(ref["y"], got["y"], ref["lo"], ref["hi"], t.sel.T, 1e-5)
        assert not unexplained, unexplained[:5]
        util.compare_activations(ref, scaled, atol_eps=32)
    else:
        st = util.fp16_bars(ref, scaled, t.sel.T, "fp16 T = 0.8 / 1.3")
        print("fp16 temperatures 0.8 / 1.3: %s" % {k: round(v, 4) for k, v in st.items()})


# ---- 4. chunks ---------------------------------------------------------------------------------------------------------------------

K0 = 20


def _two_chunks(precision, mode):
    """y [B][N] and the last P of: samples [0, K0) at T_a, setTemperatures, [K0, N) at T_b -- the run under test, and per column the
    same two chunks on the engine that is handed Wza / T_a, then Wza / T_b, with the history carried over."""
    key = ("chunks", precision, mode)
    if key in _cache:
        return _cache[key]
    cc = TC.COND
    case, m, x, w, Lh, t = _inputs(cc, precision)
    s = case.shape
    ta, tb = TC.power_temperatures(s.B), TC.power_temperatures(s.B, 2)

    def chunks(e, between):
        y = np.full((s.B, s.N), -1, dtype=np.int32)
        assert e.run_partial_chunk(0, K0, s.N, s.B)
        between()
        assert e.run_partial(K0, s.N, s.B, y, 1, True)
        e.synchronize()
        return dict(y=y, P=e.getP())

    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(ta)
    got = chunks(e, lambda: e.setTemperatures(tb))
    e.close()
    refs = {}
    for a, b in sorted(set(zip(ta, tb))):
        r = _seeded(case, _scaled(t, a), precision, mode, m, x, w)
        tT = _scaled(t, b)
        refs[(a, b)] = chunks(r, lambda: r.setOutWeights(tT.Wzs, tT.Bzs, tT.Wza, tT.Bza))
        r.close()
    _cache[key] = (got, refs, ta, tb)
    return _cache[key]


@pytest.mark.parametrize("precision,mode", [(16, "wg2"), (32, "wg")])
def test_a_change_between_two_chunks_takes_effect_at_the_next_chunk(precision, mode):
    got, refs, ta, tb = _two_chunks(precision, mode)
    for b, pair in enumerate(zip(ta, tb)):
        assert np.array_equal(got["y"][b], refs[pair]["y"][b]), "column %d, T %g then %g: samples differ first at %d" % (
            (b,) + pair + (int(np.nonzero(got["y"][b] != refs[pair]["y"][b])[0][0]),))
        assert np.array_equal(got["P"][b], refs[pair]["P"][b]), (b, pair)
    # (the first chunk is the one-temperature run's, the rest is not)
    one = _tempered(TC.COND, precision, mode, ta)["y"]
    assert np.array_equal(got["y"][:, :K0], one[:, :K0]) and not np.array_equal(got["y"][:, K0:], one[:, K0:])


# ---- 5. slot mode ------------------------------------------------------------------------------------------------------------------

def _column_of(b, columns):
    return (7 * b + 3) % columns      # (a permutation of 40 columns without a fixed point)


def _slot_engine(precision, mode, columns=None):
    case, m, x, w, Lh, t = _inputs(TC.COND, precision)
    return _engine(case, t, precision, mode, w, m["cond_b"], columns or case.shape.B)


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2"), (16, "wg")])
def test_slot_utterances_reproduce_their_lockstep_columns_at_their_temperatures(precision, mode):
    """Utterance b (uid = b, T_b) joins at step b mod 4 in column 7 b + 3 mod 40, window = the largest dilation (16), steps of 5 and
    16 samples: every one crosses the window's wrap several times, and equals column b of the lockstep run of test 2."""
    case, m, x, w, Lh, t = _inputs(TC.COND, precision)
    s = case.shape
    temps = TC.power_temperatures(s.B)
    y_lock = _tempered(TC.COND, precision, mode, temps)["y"]
    e = _slot_engine(precision, mode)
    assert e.slotTemperature(0) == 0.0                       # outside slot mode
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    for step in range(64):
        for b in range(s.B):
            if b % 4 == step:
                col = _column_of(b, s.B)
                r.start(col, b)
                assert e.slotTemperature(col) == 1.0          # a start puts the column back to 1: start, then set
                e.slotSetTemperature(col, temps[b])
                assert e.slotTemperature(col) == temps[b]
        if not r.cols:
            break
        r.step((5, 16)[step % 2])
    e.close()
    assert len(r.got) == s.B and all(len(np.concatenate(v)) == s.N for v in r.got.values())
    r.check(y_lock, "fp%d/%s slot temperatures" % (precision, mode))


def test_mel_columns_reproduce_their_lockstep_columns_at_their_temperatures():
    """The same for mel utterances (frames upsampled in the steps), against nvw_set_mel + nvw_generate_stream with setTemperatures."""
    cc = TC.COND
    case, m, mel, up_w, w, t = _mel_inputs(cc, 16)
    s = case.shape
    temps = TC.power_temperatures(s.B)
    melg = torch.from_numpy(mel).cuda()
    lock = _mel_engine(case, t, 16, "wg2", w, m, up_w, cc.stride, s.B)
    lock.setMel(melg)
    lock.setTemperatures(temps)
    y_lock = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_lock)
    lock.setTemperatures(None)
    lock.setMel(melg)
    y_plain = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_plain)
    lock.close()
    assert np.array_equal(y_lock[2::5], y_plain[2::5]) and not np.array_equal(y_lock[0], y_plain[0])      # T = 1 columns are the plain run's
    e = _mel_engine(case, t, 16, "wg2", w, m, up_w, cc.stride, s.B)
    r = Run(e, None, s.maxD, melg=melg, stride=cc.stride)
    for step in range(64):
        for b in range(s.B):
            if b % 4 == step:
                r.start_mel(_column_of(b, s.B), b, s.N // cc.stride)
                e.slotSetTemperature(_column_of(b, s.B), temps[b])
        if not r.cols:
            break
        r.step((5, 16)[step % 2])
    e.close()
    assert len(r.got) == s.B
    r.check(y_lock, "mel slot temperatures")


@pytest.mark.parametrize("precision,mode", [(16, "wg2"), (32, "wg")])
def test_a_slot_temperature_set_between_two_steps_reproduces_the_chunked_run(precision, mode):
    """nvw_slot_set_temperature at local sample K0 = 20 (steps of 5), T_a before and T_b from there on: test 4's samples."""
    case, m, x, w, Lh, t = _inputs(TC.COND, precision)
    s = case.shape
    got, refs, ta, tb = _two_chunks(precision, mode)
    e = _slot_engine(precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    for b in range(s.B):
        r.start(_column_of(b, s.B), b)
        assert lib.nvw_slot_set_temperature(e._h, _column_of(b, s.B), ta[b])
    for _ in range(K0 // 5):
        r.step(5)
    for b in range(s.B):
        assert lib.nvw_slot_set_temperature(e._h, _column_of(b, s.B), tb[b])
    r.step(16)
    _finish(r, 5)
    e.close()
    r.check(got["y"], "fp%d/%s set at local sample %d" % (precision, mode, K0))


# ---- 6. moving and saving ----------------------------------------------------------------------------------------------------------

def _header(blob):
    return np.frombuffer(bytes(blob.cpu().numpy()[:64].tobytes()), dtype="<u4")


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2")])
def test_moves_saves_and_resumes_carry_the_temperature(precision, mode):
    """After some steps: slotMove across tiles, and slotSave + slotResume into another column of a second engine -- both continue bit
    for bit; header word 10 holds the bits of T, zero for the column at T = 1; nvw_slot_temperature says so on either side."""
    case, m, x, w, Lh, t = _inputs(TC.COND, precision)
    s = case.shape
    temps = TC.power_temperatures(s.B)
    y_lock = _tempered(TC.COND, precision, mode, temps)["y"]
    xg = torch.from_numpy(x).cuda()
    e = _slot_engine(precision, mode)
    r = Run(e, xg, s.maxD)
    for b in (0, 1, 2, 3, 4, 7, 21, 38):                     # T = 1/4, 1/2, 1, 2, 4, 1, 1/2, 2
        r.start(b + 1, b)
        e.slotSetTemperature(b + 1, temps[b])
    r.step(5)
    r.step(16)
    r.move(1, 30)                                             # uid 0 (T = 1/4) across tiles
    r.move(39, 0)                                             # uid 38 (T = 2) into the first tile
    assert (e.slotTemperature(30), e.slotTemperature(0), e.slotTemperature(1), e.slotTemperature(39)) == (0.25, 2.0, 0.0, 0.0)
    r.start(1, 5)                                             # the move's source takes a new utterance: back to 1 (uid 5: T = 1/4, not set)
    assert e.slotTemperature(1) == 1.0
    e.slotStop(1)
    del r.cols[1], r.got[len(r.got) - 1]
    r.step(5)
    # save uid 3 (T = 2), uid 2 (T = 1) and uid 1 (T = 1/2), resume them in a second engine in other columns at another counter
    e2 = _slot_engine(precision, mode, 24)
    r2 = Run(e2, xg, 2 * s.maxD, into=r)
    r2.start(3, 4)
    e2.slotSetTemperature(3, temps[4])
    r2.step(7)
    for col, uid, to in ((4, 3, 17), (3, 2, 0), (2, 1, 5)):
        blob, rec = r.suspend(col)
        h = _header(blob)
        assert h[WORD] == (_bits(temps[uid]) if temps[uid] != 1.0 else 0) and not h[11:].any() and (h[6], h[7]) == (26, uid)
        r2.resume(to, blob, rec)
        assert e2.slotTemperature(to) == temps[uid] and e.slotTemperature(col) == 0.0
    # a blob with a bad word 10 is refused and changes nothing
    blob, rec = r.suspend(8)                                  # uid 7, T = 1
    for word in (_bits(-2.0), _bits(float("nan")), _bits(4096.0), 7):
        bad = blob.clone()
        bad[4 * WORD:4 * WORD + 4] = torch.from_numpy(np.array([word], dtype="<u4").view(np.uint8).copy()).cuda()
        assert not lib.nvw_slot_resume(e2._h, 9, bad.data_ptr(), xg[7].data_ptr(), 32, xg[7].stride(0), xg[7].stride(1), s.N)
        assert e2.slotTemperature(9) == 0.0
    r2.resume(9, blob, rec)
    assert e2.slotTemperature(9) == 1.0
    _finish(r, 16)
    _finish(r2, 5)
    e.close(), e2.close()
    assert len(r.got) == 9
    r.check(y_lock, "fp%d/%s moved, saved and resumed" % (precision, mode))


def test_suspend_many_into_pinned_memory_and_resume_many_carry_the_temperature():
    """SlotStream: submit(temperature=), set_temperature, suspend_many(pinned=True) -- one list save, the device writes word 10 of
    every header --, to_bytes / from_bytes, resume_many in a stream on a second engine: every request's samples are its lockstep
    column's, and SlotState.temperature is the header's."""
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(TC.COND, precision)
    s = case.shape
    temps = TC.power_temperatures(s.B)
    y_lock = _tempered(TC.COND, precision, mode, temps)["y"]
    xg = torch.from_numpy(x).cuda()
    e, e2 = _slot_engine(precision, mode, 24), _slot_engine(precision, mode, 24)
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, s.maxD, pcm=False)
    uids = list(range(20))
    hs = {b: st.submit(xg[b], uid=b, temperature=temps[b] if b % 2 else 1.0) for b in uids}
    got = {b: [] for b in uids}

    def step(stream, handles, n):
        for h, (y, _) in stream.step(n).items():
            got[handles[h]].append(y)

    for b in uids[::2]:
        st.set_temperature(hs[b], temps[b])                   # waiting: applied at admission
    step(st, {h: b for b, h in hs.items()}, 5)
    step(st, {h: b for b, h in hs.items()}, 16)
    states = st.suspend_many([hs[b] for b in uids], pinned=True)
    torch.cuda.synchronize()
    for b, state in zip(uids, states):
        assert state.temperature == temps[b] and state.done == 21 and state.blob.is_pinned()
        assert _header(state.blob)[WORD] == (_bits(temps[b]) if temps[b] != 1.0 else 0), b
    back = [SlotState.from_bytes(state.to_bytes(), state.source) if b % 3 == 0 else state for b, state in zip(uids, states)]
    assert [sb.temperature for sb in back] == [temps[b] for b in uids]
    hs2 = dict(zip(st2.resume_many(back), uids))
    while st2.busy():
        step(st2, hs2, 5)
        st2.finished()
    st.close(), st2.close()
    e.close(), e2.close()
    for b in uids:
        y = np.concatenate(got[b])
        assert np.array_equal(y, y_lock[b]), "request %d (T = %g) differs from its lockstep column first at %d" % (
            b, temps[b], int(np.nonzero(y != y_lock[b, :len(y)])[0][0]) if len(y) == s.N else len(y))


# ---- 7. refusals change nothing ----------------------------------------------------------------------------------------------------

BAD = (float("nan"), 0.0, -1.0, float("inf"), 2.0 ** -11, 2.0 ** 10 + 1.0)


def test_refused_temperatures_change_nothing():
    precision, mode = 16, "wg2"
    case, m, x, w, Lh, t = _inputs(TC.COND, precision)
    s = case.shape
    temps = TC.power_temperatures(s.B)
    y_lock = _tempered(TC.COND, precision, mode, temps)["y"]
    # lockstep: a refused call leaves the values in force
    e = _seeded(case, t, precision, mode, m, x, w)
    e.setTemperatures(temps)
    for bad in BAD:
        v = np.array(temps[:-1] + [bad], dtype=np.float32)
        assert not lib.nvw_set_temperatures(e._h, v.ctypes.data, s.B)
    v = np.array(temps + [1.0], dtype=np.float32)
    assert not lib.nvw_set_temperatures(e._h, v.ctypes.data, s.B + 1) and not lib.nvw_set_temperatures(e._h, v.ctypes.data, 0)
    assert not lib.nvw_slot_set_temperature(e._h, 0, 2.0) and lib.nvw_slot_temperature(e._h, 0) == 0.0      # outside slot mode
    assert np.array_equal(_run(e, case, dump=False)["y"], y_lock)
    e.close()
    # slot mode
    e = _slot_engine(precision, mode)
    xg = torch.from_numpy(x).cuda()
    r = Run(e, xg, s.maxD)
    v = np.ones(s.B, dtype=np.float32)
    assert not lib.nvw_set_temperatures(e._h, v.ctypes.data, s.B)                                            # the lockstep call, in slot mode
    for b in (0, 1, 3):
        r.start(_column_of(b, s.B), b)
        e.slotSetTemperature(_column_of(b, s.B), temps[b])
    r.step(5)
    col = _column_of(3, s.B)
    for bad in BAD:
        assert not lib.nvw_slot_set_temperature(e._h, col, bad)
    assert not lib.nvw_slot_set_temperature(e._h, 5, 2.0)                                                    # an idle column
    assert not lib.nvw_slot_set_temperature(e._h, -1, 2.0) and not lib.nvw_slot_set_temperature(e._h, s.B, 2.0)
    assert lib.nvw_slot_temperature(e._h, 5) == 0.0 and lib.nvw_slot_temperature(e._h, s.B) == 0.0 and lib.nvw_slot_temperature(e._h, col) == temps[3]
    _finish(r, 16)
    e.slotsEnd()
    assert lib.nvw_slot_temperature(e._h, col) == 0.0
    e.close()
    r.check(y_lock, "slot mode after refusals")


@pytest.mark.parametrize("mode", ["wg2", "chain"])
def test_runs_that_cannot_honour_a_temperature_return_0_and_run_again_at_1(mode):
    """Packed conditioning on wavenet_wg, and a chain engine: with some T != 1 run() returns 0 and generates nothing; after
    setTemperatures(NULL) the same engine runs, and its samples are a fresh engine's."""
    case = cases.BY_NAME["C3_R64S256A256_L20_B16"]
    s = case.shape
    t = util.gen_o1(case, half=True)
    e = util.make_engine(case, t, precision=16, mode=mode)
    fresh = util.make_engine(case, t, precision=16, mode=mode)
    assert ("wavenet_chain" in e.kernelInfo()) == (mode == "chain"), e.kernelInfo()
    e.setTemperatures([1.0] * (s.B - 1) + [0.5])
    y = np.full((s.B, s.N), -7, dtype=np.int32)
    assert not e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    assert (y == -7).all()
    e.setTemperatures(None)
    assert e.run(s.N, s.B, y, 1, False)
    y_fresh = np.full((s.B, s.N), -1, dtype=np.int32)
    assert fresh.run(s.N, s.B, y_fresh, 1, False)
    e.synchronize()
    assert np.array_equal(y, y_fresh) and e.chainStatus() == 0
    e.close(), fresh.close()


# ---- 8. the Python wrapper ---------------------------------------------------------------------------------------------------------

def test_infer_features_takes_temperatures_and_infer_refuses_them():
    """NVWaveNetEngine.infer_features(temperature=[...]) has test 2's property: column b at T_b equals column b of the wrapper whose
    conv_end_weight is divided by T_b (the wrapper's output biases are zero), run without a temperature -- bit for bit, fp32,
    in-kernel selectors; a float means every column; the engine the wrapper keeps goes back to 1 afterwards;
    infer(..., temperature=...) raises and points to infer_features."""
    from nv_wavenet_amd import nv_wavenet as NW
    import test_parity_gpu as TP
    s = TC.CASE.shape
    _, dev, cond = TP._wrapper_model(s.R, s.S, s.A, s.L, s.B, s.N)
    g = torch.Generator().manual_seed(23)
    n_cond = 80
    x = torch.randn(s.B, n_cond, s.N, generator=g).cuda()
    cw = ((torch.rand(2 * s.R * s.L, n_cond, 1, generator=g) - 0.5) * (3.46 * 0.5 / np.sqrt(n_cond))).cuda()
    cb = ((torch.rand(2 * s.R * s.L, generator=g) - 0.5) * 0.2).cuda()
    dev["conv_end_weight"] = dev["conv_end_weight"] * 40.0      # (logits of order one: the temperature must matter)
    temps = TC.power_temperatures(s.B)
    wrapper = NW.NVWaveNetEngine(**dev, precision=32)
    plain = wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5).cpu().numpy()
    y = wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, temperature=temps).cpu().numpy()
    half = wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, temperature=0.5).cpu().numpy()
    assert np.array_equal(wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5).cpu().numpy(), plain)
    with pytest.raises(ValueError, match="infer_features"):
        wrapper.infer(cond.cuda(), NW.Impl.SINGLE_BLOCK, seed=5, temperature=0.5)
    assert wrapper.infer(cond.cuda(), NW.Impl.SINGLE_BLOCK, seed=5).shape == (s.B, s.N)      # the shared engine is back at 1
    for bad in (temps[:-1], [0.0] * s.B, float("nan")):
        with pytest.raises(ValueError):
            wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, temperature=bad)
    wrapper.close()
    assert not np.array_equal(y[0], plain[0]) and np.array_equal(y[2::5], plain[2::5])
    for T in sorted(set(temps)):
        ref = NW.NVWaveNetEngine(**dict(dev, conv_end_weight=dev["conv_end_weight"] / T), precision=32)
        y_ref = ref.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5).cpu().numpy()
        ref.close()
        for b in range(s.B):
            if temps[b] == T:
                assert np.array_equal(y[b], y_ref[b]), "column %d at T = %g" % (b, T)
        if T == 0.5:
            assert np.array_equal(half, y_ref)
