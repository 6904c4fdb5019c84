"""GPU tests of primed generation (`-m gpu`).  An utterance may carry a prime y[0 .. n): its local samples k < n are
y[k] -- delivered and fed back like drawn ones --, and from k = n on it draws as always.  What carries the tests: a prime made of an
unprimed run's own first n samples continues that run bit for bit (P1); a slot-mode utterance equals its lockstep column whatever
its placement (P3); behind a foreign prime the engine's picks are the teacher-forced oracle's, by the bars of the features path
(P4); and a column primed with the samples of an interrupted utterance saves the blob the uninterrupted one saved (P5).  Shapes and
primes: tests/prime_cases.py."""
import struct

import numpy as np
import pytest
import torch

import cases
import condgen
import prime_cases as PC
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.slots import SlotState, SlotStream
from test_features_gpu import _feature_engine, _run
from test_slots_gpu import SEED, _engine
from test_slots_mel_gpu import _mel_engine, _mel_inputs
from test_slots_state_gpu import Run, _finish

pytestmark = pytest.mark.gpu

assert SEED == PC.SEED
RUNS = [(16, "wg"), (16, "wg2"), (16, "wg3"), (32, "wg"), (32, "wg2")]      # one to three tiles per workgroup (fp32: one and two)
_cache = {}


def _lock_engine(cc, precision, mode):
    case, m, x, w, t = PC.inputs(cc, precision)
    e = _feature_engine(case, t, precision, mode, m, x, w)
    e.setSelectorSeed(SEED)
    assert "RAW=3" in e.kernelInfo(), e.kernelInfo()
    return e


def _again(e, case, **kw):
    e.resetHistory()
    return _run(e, case, **kw)


def _y0(cc, precision, mode):
    """the unprimed lockstep run (seed), once per (case, precision, mode)"""
    key = ("y0", cc.name, precision, mode)
    if key not in _cache:
        e = _lock_engine(cc, precision, mode)
        _cache[key] = _run(e, PC.inputs(cc, precision)[0])
        e.close()
    return _cache[key]


def _primes(cc, precision, mode, kind):
    """(primes [B][N], lengths) -- "own": the unprimed run's samples; "foreign": PC.foreign_primes against it"""
    y0 = _y0(cc, precision, mode)["y"]
    lengths = PC.prime_lengths(y0.shape[0])
    return (y0 if kind == "own" else PC.foreign_primes(PC.inputs(cc, precision)[0].shape.A, y0)), lengths


def _foreign(cc, precision, mode):
    """the lockstep run behind the foreign primes, in chunks of 20 with the last sample's activations; once per (case, precision, mode)"""
    key = ("foreign", cc.name, precision, mode)
    if key not in _cache:
        case = PC.inputs(cc, precision)[0]
        p, lengths = _primes(cc, precision, mode, "foreign")
        e = _lock_engine(cc, precision, mode)
        e.setPrime(p, lengths)
        _cache[key] = _run(e, case, chunk=case.chunk)
        e.close()
    return _cache[key]


def _dev(p, b, n):
    return torch.from_numpy(np.ascontiguousarray(p[b, :n])).cuda()


# ---- 1. continuation, lockstep (P1) ------------------------------------------------------------------------------------------------

def _ids(runs):
    return ["%s-fp%d-%s" % (cc.name, precision, mode) for cc, precision, mode in runs]


LOCKSTEP_RUNS = [(PC.COND, p, m) for p, m in RUNS] + [(PC.COND_A1024, 16, "wg")]
ORACLE_RUNS = [(PC.COND, 32, "wg2"), (PC.COND, 16, "wg3"), (PC.COND_A1024, 16, "wg")]


@pytest.mark.parametrize("cc,precision,mode", LOCKSTEP_RUNS, ids=_ids(LOCKSTEP_RUNS))
def test_a_prime_of_the_runs_own_samples_continues_it_bit_for_bit(cc, precision, mode):
    """Column b primed with the first n_b samples of the unprimed run (n_b cycling through 0, 1, 2, 15, 16, 17, 20, 31, 40, 47,
    48): in chunks of 20 and in one launch the samples are the unprimed run's everywhere, and so is the last sample's P.  The same
    with an uploaded selector table in place of the seed; the caller's table is not written: unprimed again, it gives y0."""
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    y0 = _y0(cc, precision, mode)
    p, lengths = _primes(cc, precision, mode, "own")
    e = _lock_engine(cc, precision, mode)
    e.setPrime(p[:, :max(lengths)], lengths)
    for chunk in (case.chunk, None):
        got = _again(e, case, chunk=chunk)
        assert np.array_equal(got["y"], y0["y"]), "seed, chunk %s: first difference at (b, t) = %s" % (chunk, np.argwhere(got["y"] != y0["y"])[:1])
        assert np.array_equal(got["P"], y0["P"]) and np.array_equal(got["Za"], y0["Za"])
    e.setPrime(torch.from_numpy(p).cuda(), lengths)                  # the values from device memory
    assert np.array_equal(_again(e, case, dump=False)["y"], y0["y"])
    e.setSelectors(t.sel, s.N)                                       # an uploaded table (the same draws)
    for chunk in (case.chunk, None):
        assert np.array_equal(_again(e, case, dump=False, chunk=chunk)["y"], y0["y"]), "table, chunk %s" % chunk
    e.setPrime(None)
    assert np.array_equal(_again(e, case, dump=False)["y"], y0["y"]), "the caller's table after the primed runs"
    e.close()


# ---- 2. a foreign prime against the oracle (P4) ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cc,precision,mode", ORACLE_RUNS, ids=_ids(ORACLE_RUNS))
def test_behind_a_foreign_prime_the_picks_are_the_teacher_forced_oracles(cc, precision, mode):
    """Primes that differ from the unprimed run everywhere (0 and A - 1 among them): the delivered samples below n_b are the prime;
    the fp32 oracle fed [prime ; the engine's samples] picks what the engine picked from n_b on -- fp32: exact up to a draw within
    1e-5 of a CDF edge, activations by compare_activations(atol_eps=32); fp16: util.fp16_bars --; and in at least 90 % of the
    columns with 0 < n_b < 48 the samples behind the prime leave the unprimed run (the prime is not ignored)."""
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    y0 = _y0(cc, precision, mode)["y"]
    p, lengths = _primes(cc, precision, mode, "foreign")
    got = _foreign(cc, precision, mode)
    forced = np.arange(s.N)[None, :] < np.array(lengths)[:, None]
    assert np.array_equal(got["y"][forced], p[forced]), "a forced sample was not delivered as given"
    inner = PC.inner_columns(lengths, s.N)
    differ = PC.differing_columns(got["y"], y0, lengths)
    print("%s fp%d/%s: %d of %d columns leave the unprimed run behind their prime" % (cc.name, precision, mode, len(differ), len(inner)))
    assert len(differ) >= 0.9 * len(inner), (len(differ), len(inner))
    ref = util.teacher_forced_oracle(case, t, got["y"])
    agree = (ref["y"] == got["y"])[~forced].mean()
    ref["y"] = np.where(forced, got["y"], ref["y"])                  # (a forced sample is nobody's pick)
    if precision == 32:
        _, unexplained = util.explain_mismatches(ref["y"], got["y"], ref["lo"], ref["hi"], t.sel.T, 1e-5)
        assert not unexplained, "unexplained sample mismatches (b,t,ref,got,edge distance): %s" % unexplained[:5]
        assert agree >= 0.999, agree
        util.compare_activations(ref, got, atol_eps=32)
    else:
        st = util.fp16_bars(ref, got, t.sel.T, "fp16 behind a foreign prime")
        assert agree >= util.FP16_MIN_AGREEMENT, agree
        print("fp16 behind a foreign prime: %s, agreement behind the primes %.4f" % ({k: round(v, 4) for k, v in st.items()}, agree))


# ---- 3. slot mode (P3) -------------------------------------------------------------------------------------------------------------

def _column_of(b, columns):
    return (7 * b + 3) % columns      # (a permutation of 40 columns without a fixed point)


def _slot_engine(cc, precision, mode, columns=None):
    case, m, x, w, t = PC.inputs(cc, precision)
    return _engine(case, t, precision, mode, w, m["cond_b"], columns or case.shape.B)


@pytest.mark.parametrize("precision,mode,window,kind", [(16, "wg3", 16, "foreign"), (32, "wg2", 32, "foreign"), (16, "wg", 32, "own"),
                                                        (16, "wg2", 16, "own")])
def test_slot_utterances_reproduce_their_primed_lockstep_columns(precision, mode, window, kind):
    """Utterance b (uid = b, its prime of test 1 / test 2) joins at step b mod 4 in column 7 b + 3 mod 40; steps of 1, 7 and 16
    samples, window 16 or 32: the rows wrap several times inside and past the primes, neighbours start and stop around every
    column.  Every utterance equals column b of the lockstep primed run."""
    cc = PC.COND
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    p, lengths = _primes(cc, precision, mode, kind)
    y_lock = (_y0 if kind == "own" else _foreign)(cc, precision, mode)["y"]
    e = _slot_engine(cc, precision, mode)
    assert e.slotPrimed(0) == 0                                      # outside slot mode
    r = Run(e, torch.from_numpy(x).cuda(), window)
    for step in range(64):
        for b in range(s.B):
            if b % 4 == step:
                col = _column_of(b, s.B)
                r.start(col, b)
                assert e.slotPrimed(col) == 0
                if lengths[b]:
                    e.slotPrime(col, _dev(p, b, lengths[b]))
                    assert e.slotPrimed(col) == lengths[b]
        if not r.cols:
            break
        r.step((1, 7, 16)[step % 3])
    assert all(e.slotPrimed(c) == 0 for c in range(s.B))
    e.close()
    assert len(r.got) == s.B and all(len(np.concatenate(v)) == s.N for v in r.got.values())
    r.check(y_lock, "fp%d/%s window %d, %s primes" % (precision, mode, window, kind))


def test_mel_requests_with_primes_reproduce_the_primed_lockstep_run():
    """SlotStream.submit_mel(prime=) at the smallest hop of tests/test_slots_mel_gpu.py's cases (2 samples per frame): the frames
    arrive a few at a time while the columns are still inside their primes (a step never outruns them), against nvw_set_mel +
    nvw_set_prime + nvw_generate_stream."""
    cc = condgen.COND_BY_NAME["cond_C3_B16"]
    assert cc.stride == 2
    case, m, mel, up_w, w, t = _mel_inputs(cc, 16)
    s = case.shape
    lengths = PC.prime_lengths(s.B)
    melg = torch.from_numpy(mel).cuda()
    lock = _mel_engine(case, t, 16, "wg", w, m, up_w, cc.stride, s.B)
    lock.setMel(melg)
    y_plain = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_plain)
    p = PC.foreign_primes(s.A, y_plain)
    p[1::2] = y_plain[1::2]                                          # odd columns continue their own run
    lock.setMel(melg)
    lock.setPrime(p[:, :max(lengths)], lengths)
    y_lock = np.full((s.B, s.N), -1, dtype=np.int32)
    assert lock.generate_stream(3 * cc.stride + 1, None, s.N, s.B, y_lock)
    lock.close()
    forced = np.arange(s.N)[None, :] < np.array(lengths)[:, None]
    assert np.array_equal(y_lock[forced], p[forced]) and np.array_equal(y_lock[1::2], y_plain[1::2])
    assert PC.differing_columns(y_lock[0::2], y_plain[0::2], lengths[0::2]), "no even column leaves the unprimed run: the primes were ignored"
    e = _mel_engine(case, t, 16, "wg", w, m, up_w, cc.stride, s.B)
    st = SlotStream(e, s.maxD, pcm=False)
    frames = s.N // cc.stride
    bufs = {b: torch.full_like(melg[b], float("nan")) for b in range(s.B)}      # frames not yet written: NaN, never to be read
    got, avail, hs = {b: [] for b in range(s.B)}, {}, {}
    for step in range(400):
        for b in range(s.B):
            if b % 4 == step:
                avail[b] = 3
                bufs[b][:, :3] = melg[b][:, :3]
                hs[b] = st.submit_mel(bufs[b], uid=b, frames=3, final=False, prime=torch.from_numpy(p[b, :lengths[b]].copy()) if lengths[b] else None)
        for b, h in hs.items():                                      # five more frames before every step, the last ones final
            if avail[b] < frames:
                new = min(frames, avail[b] + 5)
                bufs[b][:, avail[b]:new] = melg[b][:, avail[b]:new]
                st.extend_mel(h, new, final=new == frames)
                avail[b] = new
        if not st.busy():
            break
        by_handle = {h: b for b, h in hs.items()}
        for h, (y, _) in st.step((1, 7, 16)[step % 3]).items():
            got[by_handle[h]].append(y)
        st.finished()
    st.close()
    e.close()
    for b in range(s.B):
        y = np.concatenate(got[b])
        assert len(y) == s.N and np.array_equal(y, y_lock[b]), "mel request %d (n = %d) differs from its primed lockstep column" % (b, lengths[b])


# ---- 4. state mid-prime ------------------------------------------------------------------------------------------------------------

def test_a_column_suspended_or_moved_inside_its_prime_goes_on_unchanged():
    """n = 31 (utterances 7, 18, 29): suspended at done = 10, resumed in another column and primed again with the same y, n; moved at
    done = 10 (the move carries the prime); and one resumed WITHOUT its prime, which must then leave the primed run."""
    cc, precision, mode = PC.COND, 16, "wg2"
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    p, lengths = _primes(cc, precision, mode, "foreign")
    y_lock = _foreign(cc, precision, mode)["y"]
    assert [lengths[b] for b in (7, 18, 29)] == [31, 31, 31]
    e = _slot_engine(cc, precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    for col, b in ((2, 7), (20, 18), (33, 29), (5, 0)):
        r.start(col, b)
        if lengths[b]:
            e.slotPrime(col, _dev(p, b, lengths[b]))
    r.step(3)
    r.step(7)
    blob, rec = r.suspend(2)                                         # utterance 7 at done = 10
    assert e.slotPrimed(2) == 0
    r.resume(17, blob, rec)
    assert e.slotPrimed(17) == 0                                     # a resume puts the column back to "no prime": resume, then prime
    e.slotPrime(17, _dev(p, 7, 31))
    r.move(20, 1)                                                    # utterance 18 across tiles, inside its prime
    assert (e.slotPrimed(1), e.slotPrimed(20)) == (31, 0)
    blob29, rec29 = r.suspend(33)
    key29 = rec29[0]
    r.resume(34, blob29, rec29)                                      # utterance 29 goes on without its prime
    _finish(r, 16)
    e.close()
    assert len(r.got) == 4
    r.check(y_lock, "suspended / moved inside the prime", only=[k for k in r.got if k != key29])
    y29 = np.concatenate(r.got[key29])
    assert np.array_equal(y29[:10], y_lock[29, :10]) and not np.array_equal(y29[10:31], y_lock[29, 10:31])


def test_streams_keep_primes_through_drain_bytes_and_resume_many():
    """SlotStream: submit(prime=), 10 samples, drain(pinned=True) -- every state keeps its prime --, to_bytes / from_bytes for every
    third (the unconsumed part y[10 .. n) travels behind the blob), resume_many on a second engine: every request's samples are its
    primed lockstep column's.  The bytes of a state without a prime, or past it, are the documented record and the blob alone."""
    cc, precision, mode = PC.COND, 16, "wg2"
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    p, lengths = _primes(cc, precision, mode, "foreign")
    y_lock = _foreign(cc, precision, mode)["y"]
    xg = torch.from_numpy(x).cuda()
    e, e2 = _slot_engine(cc, precision, mode, 24), _slot_engine(cc, precision, mode, 24)
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, 2 * s.maxD, pcm=False)
    uids = list(range(22))
    hs = {b: st.submit(xg[b], uid=b, prime=torch.from_numpy(p[b, :lengths[b]].copy()) if lengths[b] else None) for b in uids}
    got = {b: [] for b in uids}

    def step(stream, handles, n):
        for h, (y, _) in stream.step(n).items():
            got[handles[h]].append(y)

    step(st, {h: b for b, h in hs.items()}, 3)
    step(st, {h: b for b, h in hs.items()}, 7)
    states = st.drain(pinned=True)
    torch.cuda.synchronize()
    assert not st.busy() and [state.uid for state in states] == uids
    back = []
    for b, state in zip(uids, states):
        assert state.done == 10 and (state.prime is None) == (lengths[b] == 0)
        data = state.to_bytes()
        record = b"NWSS" + struct.pack("<IIiiIiI", 1, 0, 0, 0, b, 10, state.blob.numel()) + state.blob.numpy().tobytes()
        if lengths[b] <= 10:
            assert data == record, "utterance %d (n = %d): a state without an unconsumed prime is the record and the blob" % (b, lengths[b])
        else:
            assert data == record + b"NWSP" + struct.pack("<II", 10, lengths[b] - 10) + p[b, 10:lengths[b]].astype("<i4").tobytes()
        back.append(SlotState.from_bytes(data, state.source) if b % 3 == 0 else state)
    hs2 = dict(zip(st2.resume_many(back), uids))
    while st2.busy():
        step(st2, hs2, 5)
        st2.finished()
    st.close(), st2.close()
    e.close(), e2.close()
    for b in uids:
        y = np.concatenate(got[b])
        assert len(y) == s.N and np.array_equal(y, y_lock[b]), "request %d (n = %d) differs from its primed lockstep column" % (b, lengths[b])


# ---- 5. a state rebuilt from the audio alone (P5) ----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(16, "wg2"), (32, "wg")])
def test_a_column_primed_with_the_delivered_samples_saves_the_same_blob(precision, mode):
    """An utterance runs unprimed for 30 samples and is saved and stopped; later, in another column and at another counter, it
    starts again with prime = those 30 samples.  After them its blob is byte for byte the first one, and its remaining 18 samples
    are the uninterrupted run's."""
    cc = PC.COND
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    y0 = _y0(cc, precision, mode)["y"]
    e = _slot_engine(cc, precision, mode)
    r = Run(e, torch.from_numpy(x).cuda(), s.maxD)
    r.start(4, 11)
    r.start(9, 2)                                                    # a neighbour in the same tile
    for c in (7, 16, 7):
        r.step(c)
    first = r.save(4).cpu().numpy().tobytes()
    delivered = np.concatenate(r.got[0])
    assert len(delivered) == 30 and np.array_equal(delivered, y0[11, :30])
    e.slotStop(4)
    del r.cols[4]
    r.step(5)
    key = r.start(22, 11)                                            # another tile, counter 35
    e.slotPrime(22, torch.from_numpy(delivered.copy()).cuda())
    for c in (16, 14):
        r.step(c)
    assert e.slotPrimed(22) == 0
    second = r.save(22).cpu().numpy().tobytes()
    assert len(first) == e.slotStateBytes() and first == second, "the blob rebuilt from the audio differs from the saved one at byte %d" % next(
        i for i in range(len(first)) if first[i] != second[i])
    _finish(r, 16)
    e.close()
    again = np.concatenate(r.got[key])
    assert np.array_equal(again[:30], delivered) and np.array_equal(again[30:], y0[11, 30:]) and len(again) == s.N


# ---- 6. with temperatures ----------------------------------------------------------------------------------------------------------

def test_primes_and_temperatures_together():
    """P1 with T = 0.5 on the even columns; and in slot mode a set_temperature issued while the column is inside its prime: T = 1
    up to local sample 20, 0.5 from there on, n = 31 -- the forced samples 20 .. 30 are not drawn, the drawn ones from 31 on are at
    0.5: the unprimed lockstep run with setTemperatures between its chunks."""
    cc, precision, mode = PC.COND, 16, "wg2"
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    lengths = PC.prime_lengths(s.B)
    temps = [0.5 if b % 2 == 0 else 1.0 for b in range(s.B)]
    e = _lock_engine(cc, precision, mode)
    e.setTemperatures(temps)
    yT = _again(e, case, dump=False)["y"]
    assert not np.array_equal(yT[0], _y0(cc, precision, mode)["y"][0])
    e.setPrime(yT, lengths)
    assert np.array_equal(_again(e, case, dump=False, chunk=case.chunk)["y"], yT)
    e.setPrime(None)
    e.setTemperatures(None)
    e.resetHistory()
    y2 = np.full((s.B, s.N), -1, dtype=np.int32)
    assert e.run_partial_chunk(0, 20, s.N, s.B)
    e.setTemperatures([0.5] * s.B)
    assert e.run_partial(20, s.N, s.B, y2, 1, False)
    e.synchronize()
    e.close()
    se = _slot_engine(cc, precision, mode)
    r = Run(se, torch.from_numpy(x).cuda(), s.maxD)
    for b in (7, 18, 3, 0):
        r.start(b, b)
        se.slotPrime(b, _dev(y2, b, 31))
    r.step(16)
    r.step(4)
    for b in (7, 18, 3, 0):
        se.slotSetTemperature(b, 0.5)                                # inside the prime: local sample 20 of 31
        assert se.slotPrimed(b) == 31
    _finish(r, 7)
    se.close()
    r.check(y2, "a temperature set inside the prime")


# ---- 7. the clamp ------------------------------------------------------------------------------------------------------------------

def test_device_primes_outside_the_alphabet_are_clamped():
    """-1 reads as 0 and A as A - 1, lockstep (values in device memory) and in slot mode: the samples of the clamped primes."""
    cc, precision, mode = PC.COND, 16, "wg"
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    lengths = PC.prime_lengths(s.B)
    rng = np.random.RandomState(5)
    edge = rng.choice([0, s.A - 1], size=(s.B, s.N)).astype(np.int32)
    wild = np.where(edge == 0, -1, s.A).astype(np.int32)
    wild[:, ::3] = np.where(edge[:, ::3] == 0, -2 ** 31, 2 ** 31 - 1)
    e = _lock_engine(cc, precision, mode)
    e.setPrime(edge, lengths)                                        # host values inside the alphabet
    y_edge = _again(e, case, dump=False)["y"]
    e.setPrime(torch.from_numpy(wild).cuda(), lengths)
    y_wild = _again(e, case, dump=False)["y"]
    e.close()
    forced = np.arange(s.N)[None, :] < np.array(lengths)[:, None]
    assert np.array_equal(y_edge[forced], edge[forced]) and np.array_equal(y_wild, y_edge)
    se = _slot_engine(cc, precision, mode)
    r = Run(se, torch.from_numpy(x).cuda(), s.maxD)
    for b in (3, 8, 10, 17):
        r.start(_column_of(b, s.B), b)
        se.slotPrime(_column_of(b, s.B), _dev(wild, b, lengths[b]))
    _finish(r, 7)
    se.close()
    r.check(y_edge, "clamped slot primes")


# ---- 8. refusals change nothing ----------------------------------------------------------------------------------------------------

def test_refused_primes_change_nothing():
    cc, precision, mode = PC.COND, 16, "wg2"
    case, m, x, w, t = PC.inputs(cc, precision)
    s = case.shape
    p, lengths = _primes(cc, precision, mode, "foreign")
    y_lock = _foreign(cc, precision, mode)["y"]
    n = np.array(lengths, dtype=np.int32)
    # lockstep: a refused call leaves the primes in force
    e = _lock_engine(cc, precision, mode)
    e.setPrime(p, lengths)
    big = np.ascontiguousarray(np.tile(p, (2, 1)))
    call = lambda y, nn, batch, max_n, stride: lib.nvw_set_prime(e._h, y.ctypes.data, nn.ctypes.data, batch, max_n, stride)
    assert not call(p, n, 0, s.N, s.N) and not call(big, np.tile(n, 2), s.B + 1, s.N, s.N)                  # batch outside 1 .. maxBatch
    for b, bad in ((0, -1), (5, s.N + 1), (s.B - 1, 21)):
        nn = n.copy()
        nn[b] = bad
        assert not call(p, nn, s.B, 20 if bad == 21 else s.N, s.N), (b, bad)                               # an n[b] outside 0 .. max_n
    assert not call(big.reshape(s.B, 2 * s.N), n, s.B, s.N + 1, 2 * s.N)                                    # max_n above the engine's samples
    assert not call(p, n, s.B, s.N, s.N - 1)                                                               # stride < max_n
    for bad in (-1, s.A):
        q = p.copy()
        q[10, 47] = bad
        assert not call(q, n, s.B, s.N, s.N)                                                               # a host value outside 0 .. A-1
    xg = torch.from_numpy(x).cuda()
    assert not lib.nvw_slot_prime(e._h, 0, _dev(p, 7, 31).data_ptr(), 31) and lib.nvw_slot_primed(e._h, 0) == 0      # outside slot mode
    assert np.array_equal(_again(e, case, dump=False)["y"], y_lock)
    e.close()
    # slot mode
    e = _slot_engine(cc, precision, mode)
    r = Run(e, xg, s.maxD)
    assert not lib.nvw_set_prime(e._h, p.ctypes.data, n.ctypes.data, s.B, s.N, s.N)                         # the lockstep call, in slot mode
    good = {b: _dev(p, b, lengths[b]) for b in (7, 3, 10)}
    spare = _dev(p, 6, 20)
    host = np.ascontiguousarray(p[7, :31])
    for b in (7, 3, 10):
        r.start(b, b)
        assert lib.nvw_slot_prime(e._h, b, good[b].data_ptr(), lengths[b])
    assert not lib.nvw_slot_prime(e._h, -1, spare.data_ptr(), 20) and not lib.nvw_slot_prime(e._h, s.B, spare.data_ptr(), 20)
    assert not lib.nvw_slot_prime(e._h, 5, spare.data_ptr(), 20)                                            # no pending start on the column
    assert not lib.nvw_slot_prime(e._h, 7, host.ctypes.data, 31)                                            # host memory
    assert not lib.nvw_slot_prime(e._h, 7, spare.data_ptr(), 0) and not lib.nvw_slot_prime(e._h, 7, None, 20)
    r.start(12, 6, 19)                                                                                      # an utterance of 19 samples
    assert not lib.nvw_slot_prime(e._h, 12, spare.data_ptr(), 20)                                           # n above its length
    assert lib.nvw_slot_primed(e._h, 12) == 0 and lib.nvw_slot_primed(e._h, 7) == 31
    r.step(5)
    assert not lib.nvw_slot_prime(e._h, 3, spare.data_ptr(), 15)                                            # running: no pending start any more
    assert lib.nvw_slot_primed(e._h, 3) == 15
    _finish(r, 16)
    e.slotsEnd()
    assert lib.nvw_slot_primed(e._h, 7) == 0
    e.close()
    only = [k for k, u in r.uid_of.items() if u != 6]
    r.check(y_lock, "slot mode after refusals", only=only)
    y6 = np.concatenate(r.got[[k for k, u in r.uid_of.items() if u == 6][0]])
    assert np.array_equal(y6, _y0(cc, precision, mode)["y"][6, :19])                                        # (its refused prime left it unprimed)


@pytest.mark.parametrize("mode", ["wg2", "inplace", "chain"])
def test_runs_that_cannot_honour_a_prime_return_0_and_run_again_after_a_clear(mode):
    """Packed conditioning on wavenet_wg, a conditioning tensor read in place, and a chain engine: while a column is primed run()
    returns 0 and generates nothing; after nvw_set_prime(e, NULL, ..) the same engine runs, and its samples are a fresh engine's."""
    case = cases.BY_NAME["C3_R64S256A256_L20_B16"]
    s = case.shape
    t = util.gen_o1(case, half=True)

    def make():
        e = util.make_engine(case, t, precision=16, mode="wg2" if mode == "inplace" else mode)
        if mode == "inplace":
            e.setConditioningDirect(torch.from_numpy(np.ascontiguousarray(t.Lh, dtype=np.float32)).cuda(), s.N)
        return e

    e, fresh = make(), make()
    assert ("wavenet_chain" in e.kernelInfo()) == (mode == "chain"), e.kernelInfo()
    e.setPrime(np.full((s.B, 4), 7, dtype=np.int32), [0] * (s.B - 1) + [4])
    y = np.full((s.B, s.N), -7, dtype=np.int32)
    assert not e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    assert (y == -7).all()
    e.setPrime(None)
    assert e.run(s.N, s.B, y, 1, False)
    y_fresh = np.full((s.B, s.N), -1, dtype=np.int32)
    assert fresh.run(s.N, s.B, y_fresh, 1, False)
    e.synchronize()
    assert np.array_equal(y, y_fresh) and e.chainStatus() == 0
    e.close(), fresh.close()


# ---- 9. the Python wrapper ---------------------------------------------------------------------------------------------------------

def test_infer_features_continues_its_own_audio_and_leaves_the_engine_unprimed():
    """NVWaveNetEngine.infer_features(prime=y[:, :n]) of a run y with the same features and seed returns y (P1 through the
    wrapper), with prime_lengths per utterance as well; afterwards the shared engine is unprimed: infer() on a conditioning tensor
    runs."""
    from nv_wavenet_amd import nv_wavenet as NW
    import test_parity_gpu as TP
    s = PC.CASE.shape
    _, dev, cond = TP._wrapper_model(s.R, s.S, s.A, s.L, s.B, s.N)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(s.B, 80, s.N, generator=g).cuda()
    cw = ((torch.rand(2 * s.R * s.L, 80, 1, generator=g) - 0.5) * (3.46 * 0.5 / np.sqrt(80))).cuda()
    cb = ((torch.rand(2 * s.R * s.L, generator=g) - 0.5) * 0.2).cuda()
    dev["conv_end_weight"] = dev["conv_end_weight"] * 40.0           # (logits of order one: the history must matter)
    wrapper = NW.NVWaveNetEngine(**dev, precision=32)
    y = wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5)
    lengths = PC.prime_lengths(s.B)
    assert torch.equal(wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, prime=y[:, :31].cpu().long()), y)
    assert torch.equal(wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, prime=y, prime_lengths=lengths), y)
    other = (y + 1) % s.A
    z = wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5, prime=other[:, :20])
    assert torch.equal(z[:, :20], other[:, :20]) and not torch.equal(z[:, 20:], y[:, 20:])
    assert wrapper.infer(cond.cuda(), NW.Impl.SINGLE_BLOCK, seed=5).shape == (s.B, s.N)
    assert torch.equal(wrapper.infer_features(x, cw, cb, NW.Impl.SINGLE_BLOCK, seed=5), y)
    wrapper.close()
