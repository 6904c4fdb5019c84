"""GPU tests of prefill (`-m gpu`): nvw_prefill_states makes, with one launch per layer over the last W samples of a
prime, the state blob that a column started from silence, primed and stepped to local sample n saves -- BYTE FOR BYTE, header and
payload, fp16 and fp32.  Equality is the contract, so every comparison here is one of bytes; what follows a resume is then held to
the primed lockstep column bit for bit, and through it to the teacher-forced oracle.  Shapes: tests/prefill_cases.py."""
import struct

import numpy as np
import pytest
import torch

import prefill_cases as PF
import prime_cases as PC
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import PREFILL_REQ, WavenetEngine
from nv_wavenet_amd.slots import SlotState, SlotStream
from test_prime_gpu import _foreign, _primes, _slot_engine
from test_slots_gpu import _engine
from test_slots_state_gpu import Run, _finish

pytestmark = pytest.mark.gpu

EQUALITY_RUNS = [(16, "wg2"), (32, "wg")]
LENGTHS = [n for n in PC.LENGTHS if n]
_cache = {}


def _first_difference(a, b):
    a, b = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    if len(a) != len(b):
        return "sizes %d and %d" % (len(a), len(b))
    bad = np.nonzero(a != b)[0]
    return None if bad.size == 0 else "first differing byte %d of %d (%d differ): %#04x against %#04x" % (bad[0], len(a), bad.size, a[bad[0]], b[bad[0]])


def _sequential_blobs(e, xg, jobs, window, lead=5):
    """The blobs that columns primed with y and stepped to local sample n save: jobs = [(column, uid, y CUDA int32 [n], T)].  The
    session first runs `lead` samples of another utterance (last column), so that the columns start at a counter other than 0."""
    e.slotsBegin(window)
    if lead:
        e.slotStart(e.maxBatch - 1, xg[0], 0)
        for at in range(0, lead, window):          # (a step is at most the window: 1 where every layer has d = 1)
            assert e.slotsStep(min(window, lead - at))
        e.slotStop(e.maxBatch - 1)
    for col, uid, y, T in jobs:
        e.slotStart(col, xg[uid], uid)
        if T != 1.0:
            e.slotSetTemperature(col, T)
        e.slotPrime(col, y)
    blobs, done = {}, 0
    for n in sorted({int(y.numel()) for _, _, y, _ in jobs}):
        while done < n:
            c = min(window, n - done)
            assert e.slotsStep(c)
            done += c
        for col, uid, y, T in jobs:
            if y.numel() == n:
                blob, got = e.slotSave(col)
                assert got == n, (got, n)
                blobs[col] = blob.cpu().numpy().tobytes()
    e.slotsEnd()
    return blobs


def _check_equal(e, xg, jobs, window, what):
    """every job's prefilled blob -- all jobs through ONE nvw_prefill_states call -- against its sequential blob"""
    pre = e.prefillStates([(y, xg[uid], uid, T) for _, uid, y, T in jobs])
    seq = _sequential_blobs(e, xg, jobs, window)
    pre_host = pre.cpu().numpy()
    for i, (col, uid, y, T) in enumerate(jobs):
        diff = _first_difference(seq[col], pre_host[i].tobytes())
        assert diff is None, "%s, utterance %d, n = %d: prefilled blob differs from the sequential one: %s" % (what, uid, y.numel(), diff)
    return pre


def _cond(precision, mode):
    """the equality case: (case, features on the GPU, foreign primes, utterances 1 .. 10 with the lengths 1 .. 48)"""
    case, m, x, w, t = PC.inputs(PC.COND, precision)
    p, lengths = _primes(PC.COND, precision, mode, "foreign")
    bs = list(range(1, 1 + len(LENGTHS)))
    assert [lengths[b] for b in bs] == LENGTHS
    return case, t, torch.from_numpy(x).cuda(), p, bs


def _dev(p, b, n):
    return torch.from_numpy(np.ascontiguousarray(p[b, :n])).cuda()


def _prefilled(precision, mode):
    """the prefilled blobs of the equality case (test 1 has held them to the sequential ones), kept for the resumes of test 4"""
    key = (precision, mode)
    if key not in _cache:
        case, t, xg, p, bs = _cond(precision, mode)
        assert p[10, :48].min() == 0 and p[10, :48].max() == case.shape.A - 1      # (0 and A - 1 among the forced samples)
        e = _slot_engine(PC.COND, precision, mode)
        assert e.prefillWindow() == PF.window(case.shape.L, case.shape.maxD) == 40
        jobs = [((7 * b + 3) % case.shape.B, b, _dev(p, b, n), 1.0) for b, n in zip(bs, LENGTHS)]
        pre = _check_equal(e, xg, jobs, case.shape.maxD, "fp%d/%s" % (precision, mode))
        _cache[key] = pre.cpu()
        e.close()
    return _cache[key]


# ---- 1. blob equality --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", EQUALITY_RUNS)
def test_prefilled_blobs_equal_the_sequentially_primed_columns_byte_for_byte(precision, mode):
    """R 64, 8 layers, dilations 1 .. 16 (W = 40), foreign primes with 0 and A - 1 among them, every length of prime_cases.LENGTHS
    but 0 in one nvw_prefill_states call: 1, 2, 15, 16, 17 leave ring slots unwritten and sit at the tile edge, 40 is W (t0 = 0), 47
    and 48 do not reach back to the start (the pass begins at a tile that the window rounds down to)."""
    pre = _prefilled(precision, mode)
    assert pre.shape[0] == len(LENGTHS)
    for i, n in enumerate(LENGTHS):
        words = np.frombuffer(pre[i].numpy().tobytes()[:PF.HEADER_BYTES], dtype="<i4")
        assert words[6] == n and words[7] == 1 + i and words[10] == 0 and not words[11:].any()


# ---- 2. the other R ----------------------------------------------------------------------------------------------------------------

def _shape_engine(shape, seed, precision, L=8, maxD=16, N=48, columns=3):
    case = PF.case_of(shape, seed, L, maxD, N, columns)
    s = case.shape
    t = util.gen_o1(case, half=precision == 16)
    x, w, b = PF.features(columns, N, s.R, L, half=precision == 16)
    e = _engine(case, t, precision, "wg", w, b, columns)
    return case, e, torch.from_numpy(x).cuda(), PF.primes(columns, N, s.A)


@pytest.mark.parametrize("R", sorted(PF.OTHER_R))
@pytest.mark.parametrize("precision", [16, 32])
def test_blob_equality_at_one_shape_per_other_R(R, precision):
    shape, seed = PF.OTHER_R[R]
    case, e, xg, p = _shape_engine(shape, seed, precision)
    assert e.prefillWindow() == 40
    jobs = [(b, b, _dev(p, b, n), 1.0) for b, n in enumerate(PF.OTHER_N)]
    _check_equal(e, xg, jobs, case.shape.maxD, "R %d fp%d" % (R, precision))
    e.close()


# ---- 3. a long window --------------------------------------------------------------------------------------------------------------

def _long_engine(precision):
    shape, seed, L, maxD, N = PF.LONG
    return _shape_engine(shape, seed, precision, L, maxD, N)


@pytest.mark.parametrize("precision", [16, 32])
def test_blob_equality_over_a_long_window(precision):
    """12 layers, maxDilation 128: W = 272.  n = 100 is 7 time tiles with taps of d >= 16 reading whole tiles back and most ring
    slots of the long layers unwritten; n = 300 starts at t0 = 16."""
    case, e, xg, p = _long_engine(precision)
    s = case.shape
    assert e.prefillWindow() == PF.window(s.L, s.maxD) == 272 and PF.first_tile_sample(300, s.L, s.maxD) == 16
    jobs = [(b, b, _dev(p, b, n), 1.0) for b, n in enumerate(PF.LONG_N)]
    _check_equal(e, xg, jobs, s.maxD, "long window fp%d" % precision)
    e.close()


def test_blob_equality_at_windows_that_start_past_sample_0():
    """The prime shape (R 64, 8 layers, dilations 1 .. 16, W = 40) at n = 56, 57 and 90: the pass starts at t0 = 16, 16 and 48, so
    the kernels index y and x from the window's first sample and the embedding reads its two history words from the prime itself,
    in front of the window.  Both precisions."""
    lengths = (56, 57, 90)
    assert [PF.first_tile_sample(n, 8, 16) for n in lengths] == [16, 16, 48]
    for precision in (16, 32):
        case, e, xg, p = _shape_engine((64, 256, 256), 915, precision, N=96)
        assert e.prefillWindow() == 40
        jobs = [(b, b, _dev(p, b, n), 1.0) for b, n in enumerate(lengths)]
        _check_equal(e, xg, jobs, case.shape.maxD, "windows past 0, fp%d" % precision)
        e.close()


# ---- 4. what follows a resume ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", EQUALITY_RUNS)
def test_resumed_prefilled_states_continue_as_the_primed_lockstep_columns(precision, mode):
    """Every blob of test 1 with samples left (n < 48), resumed in another column and at another counter of another engine: its
    samples n .. 47 are the primed lockstep column's bit for bit, and the fp32 oracle fed [prime ; those samples] picks them (fp32:
    exact up to a draw within 1e-5 of a CDF edge; fp16: the agreement bar of the features path)."""
    case, t, xg, p, bs = _cond(precision, mode)
    s = case.shape
    pre = _prefilled(precision, mode).cuda()
    y_lock = _foreign(PC.COND, precision, mode)["y"]
    e = _slot_engine(PC.COND, precision, mode)
    r = Run(e, xg, 2 * s.maxD)
    r.start(0, 0)
    r.step(3)
    keys = {}
    for i, (b, n) in enumerate(zip(bs, LENGTHS)):
        if n == s.N:
            continue
        keys[b] = key = len(r.got)
        r.got[key], r.uid_of[key] = [], b
        r.resume((7 * b + 3) % s.B, pre[i].contiguous(), [key, b, n, s.N, "x"])
    _finish(r, 7)
    e.close()
    y = y_lock.copy()
    for b, n in zip(bs, LENGTHS):
        if n == s.N:
            continue
        got = np.concatenate(r.got[keys[b]])
        bad = np.nonzero(got != y_lock[b, n:])[0]
        assert len(got) == s.N - n and bad.size == 0, "utterance %d resumed at %d leaves its primed lockstep column at sample %d" % (b, n, n + bad[0])
        y[b, n:] = got
    lengths = PC.prime_lengths(s.B)
    forced = np.arange(s.N)[None, :] < np.array(lengths)[:, None]
    ref = util.teacher_forced_oracle(case, t, y)
    agree = (ref["y"] == y)[~forced].mean()
    ref["y"] = np.where(forced, y, ref["y"])
    if precision == 32:
        _, unexplained = util.explain_mismatches(ref["y"], y, ref["lo"], ref["hi"], t.sel.T, 1e-5)
        assert not unexplained and agree >= 0.999, (unexplained[:5], agree)
    else:
        assert agree >= util.FP16_MIN_AGREEMENT, agree


# ---- 5. the window is the window ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,precision", [("cond", 16), ("cond", 32), ("long", 16)])
def test_only_the_last_W_samples_of_a_prime_reach_the_blob(which, precision):
    """Primes that differ at sample n - W - 1 alone, or everywhere before n - W, give identical blobs; one that differs at n - W --
    the oldest sample inside the window -- gives another payload (the control: the comparison sees something)."""
    if which == "cond":
        case, t, xg, p, bs = _cond(precision, "wg")
        e, n, x, base = _slot_engine(PC.COND, precision, "wg"), 48, xg[10], p[10, :48].copy()
    else:
        case, e, xg, p = _long_engine(precision)
        n, x, base = 300, xg[1], p[1, :300].copy()
    A, W = case.shape.A, e.prefillWindow()
    assert 0 < W < n
    one, older, inside = base.copy(), base.copy(), base.copy()
    one[n - W - 1] = (one[n - W - 1] + 97) % A
    older[:n - W] = (older[:n - W] + 31) % A
    inside[n - W] = (inside[n - W] + 97) % A
    ys = [torch.from_numpy(v).cuda() for v in (base, one, older, inside)]
    blobs = e.prefillStates([(y, x, 3, 1.0) for y in ys]).cpu().numpy()
    e.close()
    assert np.array_equal(blobs[0], blobs[1]), "a sample outside the window reached the blob: " + _first_difference(blobs[0].tobytes(), blobs[1].tobytes())
    assert np.array_equal(blobs[0], blobs[2]), "samples outside the window reached the blob: " + _first_difference(blobs[0].tobytes(), blobs[2].tobytes())
    assert np.array_equal(blobs[0][:PF.HEADER_BYTES], blobs[3][:PF.HEADER_BYTES])
    assert not np.array_equal(blobs[0][PF.HEADER_BYTES:], blobs[3][PF.HEADER_BYTES:]), "the oldest sample of the window does not reach the blob"


# ---- 6. the temperature word -------------------------------------------------------------------------------------------------------

def test_temperatures_land_in_header_word_10_and_a_resume_applies_them():
    case, t, xg, p, bs = _cond(16, "wg2")
    e = _slot_engine(PC.COND, 16, "wg2")
    temps = (0.5, 1.0, 1.75)
    jobs = [(4 + i, 7 + i, _dev(p, 7 + i, 20), T) for i, T in enumerate(temps)]
    pre = _check_equal(e, xg, jobs, case.shape.maxD, "with temperatures")
    for i, T in enumerate(temps):
        word = np.frombuffer(pre[i].cpu().numpy().tobytes()[40:44], dtype="<u4")[0]
        assert word == (0 if T == 1.0 else struct.unpack("<I", struct.pack("<f", T))[0])
    e.slotsBegin(case.shape.maxD)
    for i, T in enumerate(temps):
        e.slotResume(20 + i, pre[i].contiguous(), xg[7 + i])
        assert e.slotTemperature(20 + i) == T
    e.close()


# ---- 7. the clamp ------------------------------------------------------------------------------------------------------------------

def test_device_primes_outside_the_alphabet_are_clamped():
    """-1 reads as 0 and A as A - 1 (as slot_prime_kernel clamps them), in the embeddings and in the header's history words"""
    case, t, xg, p, bs = _cond(16, "wg")
    A = case.shape.A
    e = _slot_engine(PC.COND, 16, "wg")
    edge = np.random.RandomState(5).choice([0, A - 1], size=31).astype(np.int32)
    edge[-2:] = (0, A - 1)
    wild = np.where(edge == 0, -1, A).astype(np.int32)
    wild[::3] = np.where(edge[::3] == 0, -2 ** 31, 2 ** 31 - 1)
    blobs = e.prefillStates([(torch.from_numpy(v).cuda(), xg[7], 7, 1.0) for v in (edge, wild)]).cpu().numpy()
    e.close()
    assert np.array_equal(blobs[0], blobs[1])
    assert tuple(np.frombuffer(blobs[1].tobytes()[32:40], dtype="<i4")) == (0, A - 1)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_return_0_and_write_nothing():
    case, t, xg, p, bs = _cond(16, "wg")
    s = case.shape
    e = _slot_engine(PC.COND, 16, "wg")
    nbytes = e.slotStateBytes()
    y, x = _dev(p, 7, 31), xg[7]
    dst = torch.full((2, nbytes + 16), 0xAB, dtype=torch.uint8, device="cuda")
    host_y, host_x = np.ascontiguousarray(p[7, :31]), np.zeros((80, s.N), dtype=np.float32)

    def call(engine=e, count=1, dst_ptr=None, stride=nbytes + 16, **kw):
        req = dict(y=y.data_ptr(), n=31, x=x.data_ptr(), precision=32, c_stride=x.stride(0), t_stride=x.stride(1), uid=7, temperature=1.0)
        req.update(kw)
        reqs = np.zeros(2, dtype=PREFILL_REQ)
        for i in range(2):
            reqs[i] = tuple(req[k] for k in PREFILL_REQ.names)
        got = lib.nvw_prefill_states(engine._h, reqs.ctypes.data, count, dst.data_ptr() if dst_ptr is None else dst_ptr, stride, None)
        torch.cuda.synchronize()
        assert bool((dst == 0xAB).all()) or got, "a refused call wrote into dst"
        return got

    bare = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, 16, s.N, impl=1, tanhEmbed=True, precision=16, organisation=util.MODE_ORG["wg"])
    assert lib.nvw_prefill_window(bare._h) == 0 and call(engine=bare) == 0                                  # no conditioning weights
    bare.close()
    assert call(n=0) == 0 and call(n=-3) == 0                                                              # n < 1
    for T in (2.0 ** -11, 2.0 ** 11, float("nan"), 0.0, float("inf")):
        assert call(temperature=T) == 0, T                                                                 # a bad temperature
    assert call(precision=8) == 0 and call(precision=0) == 0                                               # a bad precision
    assert call(y=0) == 0 and call(x=0) == 0                                                               # NULL
    assert call(y=host_y.ctypes.data) == 0 and call(x=host_x.ctypes.data) == 0                             # host memory
    assert call(c_stride=0) == 0 and call(t_stride=-1) == 0                                                # strides
    assert call(dst_ptr=0) == 0 and call(dst_ptr=dst.data_ptr() + 8) == 0                                  # NULL, misaligned
    pageable = np.full(2 * (nbytes + 16), 0xAB, dtype=np.uint8)
    assert call(dst_ptr=pageable.ctypes.data) == 0 and (pageable == 0xAB).all()                            # pageable host memory
    assert call(stride=nbytes - 16) == 0 and call(stride=nbytes + 8) == 0                                  # too small, not a multiple of 16
    assert call(count=0) == 0 and call(count=-1) == 0                                                      # count < 1
    assert bool((dst == 0xAB).all())
    assert call(count=2) == 2                                                                              # ... and the call they all vary
    out = dst.cpu().numpy()
    assert (out[:, nbytes:] == 0xAB).all() and np.array_equal(out[0, :nbytes], out[1, :nbytes])
    pinned = torch.full((1, nbytes), 0xAB, dtype=torch.uint8).pin_memory()                                 # pinned memory is written in place
    assert call(dst_ptr=pinned.data_ptr(), stride=nbytes) == 1
    assert np.array_equal(pinned.numpy()[0], out[0, :nbytes])
    e.close()


# ---- 9. the scheduler --------------------------------------------------------------------------------------------------------------

def test_streams_deliver_from_sample_n_on_what_a_forced_prime_delivers():
    """SlotStream.submit(prime=, prefill=True) against prefill=False on a second engine: the samples from n on are equal, and the
    prefilled request delivers nothing below n; a state of SlotStream.prefill survives to_bytes / from_bytes and resumes."""
    precision, mode = 16, "wg2"
    case, t, xg, p, bs = _cond(precision, mode)
    s = case.shape
    y_lock = _foreign(PC.COND, precision, mode)["y"]
    e, e2 = _slot_engine(PC.COND, precision, mode, 16), _slot_engine(PC.COND, precision, mode, 16)
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, s.maxD, pcm=False)
    todo = [(b, n) for b, n in zip(bs, LENGTHS) if n < s.N]
    hs = {st.submit(xg[b], uid=b, prime=torch.from_numpy(p[b, :n].copy()), prefill=True): b for b, n in todo}
    hs2 = {st2.submit(xg[b], uid=b, prime=torch.from_numpy(p[b, :n].copy())): b for b, n in todo}
    with pytest.raises(ValueError):
        st.submit(xg[10], uid=10, prime=torch.from_numpy(p[10, :s.N].copy()), prefill=True)                 # nothing left to generate
    with pytest.raises(ValueError):
        st.submit_mel(xg[1], prime=torch.from_numpy(p[1, :4].copy()), prefill=True)
    state = st.prefill(xg[7], torch.from_numpy(p[7, :31].copy()), uid=7, temperature=1.0)      # (utterance 7 a second time)
    assert state.done == 31 and state.uid == 7 and state.prime is None
    back = SlotState.from_bytes(state.to_bytes(), xg[7])
    assert back.done == 31 and back.uid == 7 and np.array_equal(back.blob.numpy(), state.blob.cpu().numpy())
    hs[st.resume_many([back])[0]] = 7
    got, got2 = {h: [] for h in hs}, {h: [] for h in hs2}
    for stream, handles, sink in ((st, hs, got), (st2, hs2, got2)):
        while stream.busy():
            for h, (y, _) in stream.step(7).items():
                sink[h].append(y)
            stream.finished()
    st.close(), st2.close()
    e.close(), e2.close()
    by_b = {b: np.concatenate(got2[h]) for h, b in hs2.items()}
    for h, b in hs.items():
        n = dict(todo)[b]
        y = np.concatenate(got[h])
        assert len(y) == s.N - n and np.array_equal(y, y_lock[b, n:]), "prefilled request %d (n = %d) differs from its primed lockstep column" % (b, n)
        assert np.array_equal(by_b[b][:n], p[b, :n]) and np.array_equal(by_b[b][n:], y), "request %d: prefill=True and prefill=False deliver other samples" % b
