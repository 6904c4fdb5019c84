"""CPU tests of primed generation (no GPU): the three entry points within ABI 7, the two kernels in the shipped code
object, the Python-side argument checks, the prime record of SlotState.to_bytes / from_bytes, the SlotStream bookkeeping against a
stub engine that models nvw_slot_prime by the rules of wn::SlotSession, and the condition of the foreign-prime GPU test on the
oracle alone: behind a foreign prime the model goes another way than behind its own samples."""
import ctypes
import os

import numpy as np
import pytest
import torch

import prime_cases as PC
import util
from oracle import oracle as O
from test_code_objects_cpu import BUILD, kernel_table
from test_slots_state_cpu import StateFakeEngine
from test_temperature_cpu import _synthetic_blob

PRIME_SYMBOLS = ("nvw_set_prime", "nvw_slot_prime", "nvw_slot_primed")


# ---- ABI and code object ----------------------------------------------------------------------------------------------------------

def test_prime_entries_are_declared_exported_and_bound_within_abi_7():
    from nv_wavenet_amd import _lib, engine, slots
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(BUILD), "..", "..", "include", "nv_wavenet_c.h")).read()
    assert "#define NVW_ABI_VERSION 7" in header
    for name in PRIME_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert _lib.SIGNATURES["nvw_set_prime"][1][-1] is ctypes.c_longlong and len(_lib.SIGNATURES["nvw_set_prime"][1]) == 6
    assert len(_lib.SIGNATURES["nvw_slot_prime"][1]) == 4 and _lib.SIGNATURES["nvw_slot_primed"][0] is ctypes.c_int
    for name in ("setPrime", "slotPrime", "slotPrimed"):
        assert hasattr(engine.WavenetEngine, name), name
    import inspect
    assert "prime" in inspect.signature(slots.SlotStream.submit).parameters
    assert "prime" in inspect.signature(slots.SlotStream.submit_mel).parameters


def test_the_prime_kernels_are_in_the_shipped_code_object_and_use_no_scratch():
    obj = os.path.join(BUILD, "slots_prime.o")
    assert os.path.exists(obj), "no slots_prime.o: build the library first (__graft_entry__.build())"
    names = {r[0].replace(" ", "").split("(")[0]: r for r in kernel_table(obj)}
    for name in ("wn::slot_prime_kernel", "wn::prime_selectors_kernel"):
        assert name in names, (name, sorted(names))
        _, vgpr, agpr, sgpr, scratch, spill = names[name]
        assert scratch == 0 and spill == 0 and vgpr <= 32 and agpr == 0, names[name]


# ---- argument checks ---------------------------------------------------------------------------------------------------------------

def test_check_prime_takes_integer_vectors_within_the_length():
    from nv_wavenet_amd.slots import check_prime
    assert check_prime(None) is None
    p = check_prime(torch.arange(5, dtype=torch.int64), 5)
    assert p.dtype == torch.int32 and p.is_contiguous() and p.tolist() == [0, 1, 2, 3, 4]
    assert check_prime(torch.arange(10, dtype=torch.int32)[::2], 5).is_contiguous()
    assert check_prime(torch.arange(500), None).numel() == 500          # (a mel request that is not final: unbounded)
    for bad, length in ((torch.zeros(0, dtype=torch.int32), 5), (torch.zeros(6, dtype=torch.int32), 5), (torch.zeros(3), 5),
                        (torch.zeros(2, 2, dtype=torch.int32), 5), ([1, 2], 5), (torch.zeros(3, dtype=torch.bool), 5)):
        with pytest.raises(ValueError):
            check_prime(bad, length)


def _model(precision=32):
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    R, S, A, L = 64, 256, 256, 3
    mk = lambda *s: torch.zeros(*s)
    return NVWaveNetEngine(embedding_prev=mk(A, R), embedding_curr=mk(A, R), conv_out_weight=mk(A, S, 1), conv_end_weight=mk(A, A, 1),
                           dilate_weights=[mk(2 * R, R, 2) for _ in range(L)], dilate_biases=[mk(2 * R) for _ in range(L)], max_dilation=4,
                           res_weights=[mk(R, R, 1) for _ in range(L - 1)], res_biases=[mk(R) for _ in range(L - 1)],
                           skip_weights=[mk(S, R, 1) for _ in range(L)], skip_biases=[mk(S) for _ in range(L)], use_embed_tanh=False,
                           precision=precision)


def test_infer_points_to_infer_features_and_infer_features_checks_its_prime():
    m = _model()
    with pytest.raises(ValueError, match="infer_features"):
        m.infer(torch.zeros(128, 2, 3, 8), prime=torch.zeros(2, 4, dtype=torch.int32))
    x, w, b = torch.zeros(2, 80, 8), torch.zeros(3 * 128, 80), torch.zeros(3 * 128)
    ok = torch.zeros(2, 4, dtype=torch.int32)
    for prime, lengths in ((torch.zeros(3, 4, dtype=torch.int32), None),         # another batch
                           (torch.zeros(2, 9, dtype=torch.int32), None),         # longer than the utterance
                           (torch.zeros(2, 0, dtype=torch.int32), None),
                           (torch.zeros(2, 4), None),                            # not integers
                           (torch.zeros(8, dtype=torch.int32), None),
                           (torch.full((2, 4), 256, dtype=torch.int32), None),   # outside the alphabet
                           (torch.full((2, 4), -1, dtype=torch.int32), None),
                           (ok, [1]), (ok, [1, 5]), (ok, [-1, 2])):
        with pytest.raises(ValueError):
            m.infer_features(x, w, b, seed=1, prime=prime, prime_lengths=lengths)
    with pytest.raises(ValueError):
        m.infer_features(x, w, b, seed=1, prime_lengths=[1, 1])


# ---- SlotState ---------------------------------------------------------------------------------------------------------------------

def test_to_bytes_of_a_state_without_a_prime_is_the_documented_layout():
    """The bytes of a state that carries no prime, or has left it behind, are the record (magic "NWSS", version 1, kind, frames,
    final, uid, done, blob bytes -- little-endian, 32 bytes) and the blob, built here from that layout: nothing follows."""
    import struct
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    blob = _synthetic_blob(5, 8, 13, 4)
    literal = b"NWSS" + struct.pack("<IIiiIiI", 1, 0, 0, 0, 4, 13, blob.numel()) + blob.numpy().tobytes()
    assert SlotState(blob, src, 4, 13, "features").to_bytes() == literal
    passed = SlotState(blob, src, 4, 13, "features", prime=torch.arange(13, dtype=torch.int32))      # done >= n
    assert passed.to_bytes() == literal
    back = SlotState.from_bytes(literal, src)
    assert back.prime is None and back.done == 13
    mel = b"NWSS" + struct.pack("<IIiiIiI", 1, 1, 9, 0, 4, 13, blob.numel()) + blob.numpy().tobytes()
    assert SlotState(blob, src, 4, 13, "mel", 9, False).to_bytes() == mel
    assert SlotState(None, src, 7, 0, "features").to_bytes() == b"NWSS" + struct.pack("<IIiiIiI", 1, 0, 0, 0, 7, 0, 0)


def test_the_unconsumed_prime_survives_to_bytes_and_from_bytes():
    import struct
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    blob = _synthetic_blob(5, 8, 13, 4)
    y = torch.arange(100, 131, dtype=torch.int32)                     # n = 31, done = 13
    plain = SlotState(blob, src, 4, 13, "features").to_bytes()
    data = SlotState(blob, src, 4, 13, "features", prime=y).to_bytes()
    assert data[:len(plain)] == plain
    assert data[len(plain):] == b"NWSP" + struct.pack("<II", 13, 18) + y[13:].numpy().astype("<i4").tobytes()
    back = SlotState.from_bytes(data, src)
    assert back.done == 13 and back.prime.dtype == torch.int32 and back.prime.numel() == 31
    assert torch.equal(back.prime[13:], y[13:]) and torch.equal(back.blob, blob)
    assert back.to_bytes() == data
    # a request that had not started: no blob, the whole prime
    fresh = SlotState(None, src, 9, 0, "mel", 3, False, prime=y)
    back = SlotState.from_bytes(fresh.to_bytes(), src)
    assert back.blob is None and back.kind == "mel" and torch.equal(back.prime, y)
    # damaged tails are refused
    for bad in (data[:-1], data + b"\0\0\0\0", data[:len(plain)] + b"XXXX" + data[len(plain) + 4:],
                data[:len(plain) + 4] + struct.pack("<II", 12, 18) + data[len(plain) + 12:]):
        with pytest.raises(ValueError):
            SlotState.from_bytes(bad, src)


# ---- SlotStream against a fake engine ----------------------------------------------------------------------------------------------

class PrimeFakeEngine(StateFakeEngine):
    """StateFakeEngine with nvw_slot_prime by the rules of wn::SlotSession: only on a pending start or resume, a start / resume /
    stop drops the prime, a move carries it, it is gone once its last sample has been issued; local sample k < n of a primed
    column is y[k]."""

    def __init__(self, columns, window=64):
        super().__init__(columns, window)
        self.prime = {}

    def slotStart(self, col, x, uid, length=None):
        super().slotStart(col, x, uid, length)
        self.prime.pop(col, None)

    def slotStartMel(self, col, mel, uid, frames=None, final=True):
        super().slotStartMel(col, mel, uid, frames, final)
        self.prime.pop(col, None)

    def slotResume(self, col, blob, x, length=None):
        super().slotResume(col, blob, x, length)
        self.prime.pop(col, None)

    def slotStop(self, col):
        super().slotStop(col)
        self.prime.pop(col, None)

    def slotMove(self, src, dst):
        super().slotMove(src, dst)
        if src in self.prime:
            self.prime[dst] = self.prime.pop(src)

    def slotPrime(self, col, y):
        assert col in self.pending, "prime without a pending start or resume"
        assert y.dim() == 1 and y.dtype == torch.int32 and y.numel() >= 1
        self.calls.append(("prime", col, y.numel()))
        self.prime[col] = y

    def slotPrimed(self, col):
        return self.prime[col].numel() if col in self.prime else 0

    def slotsStep(self, count, y, pcm):
        t = self.t
        assert super().slotsStep(count, y, pcm)
        for col in list(self.prime):
            p, k0 = self.prime[col].numpy(), t - self.active[col][1]
            m = max(0, min(count, len(p) - k0))
            y[col, :m] = p[k0:k0 + m]
            if k0 + count >= len(p):
                del self.prime[col]
        return True


def test_the_stream_primes_after_the_start_and_keeps_the_prime_through_suspend_compact_and_resume():
    from nv_wavenet_amd.slots import SlotStream
    eng = PrimeFakeEngine(32)
    st = SlotStream(eng, 64, pcm=False)
    y = torch.arange(500, 531, dtype=torch.int32)
    h0 = st.submit(torch.zeros(80, 48), uid=3)
    h1 = st.submit(torch.zeros(80, 48), uid=5, prime=y)
    with pytest.raises(ValueError):
        st.submit(torch.zeros(80, 20), prime=y)                      # longer than the utterance
    out = st.step(10)
    assert eng.calls.index(("start", 1, 5)) < eng.calls.index(("prime", 1, 31))
    assert ("prime", 0, 31) not in eng.calls
    assert out[h1][0].tolist() == list(range(500, 510)) and out[h0][0].tolist() == list(range(3000, 3010))
    state = st.suspend(h1)                                            # done = 10 < 31: the state keeps the prime
    assert state.done == 10 and torch.equal(state.prime, y)
    st.submit(torch.zeros(80, 1000))
    h2 = st.resume(state)                                             # (at the front of the queue)
    out = st.step(7)
    col = st.running()[h2]
    last = lambda call: len(eng.calls) - 1 - eng.calls[::-1].index(call)
    assert ("resume", col, 5, 10) in eng.calls and last(("resume", col, 5, 10)) < last(("prime", col, 31))
    assert out[h2][0].tolist() == list(range(510, 517))
    out = st.step(20)                                                 # passes n = 31 at local sample 31
    assert out[h2][0].tolist() == list(range(517, 531)) + [5000 + k for k in range(31, 37)]
    assert eng.slotPrimed(col) == 0
    state = st.suspend(h2)                                            # done = 37 >= 31: resumed without a prime call
    n_prime = sum(1 for c in eng.calls if c[0] == "prime")
    h3 = st.resume(state)
    st.step(5)
    assert sum(1 for c in eng.calls if c[0] == "prime") == n_prime
    # a queued request keeps its prime through suspend / resume as well
    full = SlotStream(PrimeFakeEngine(1), 64, pcm=False)
    full.submit(torch.zeros(80, 100))
    hq = full.submit(torch.zeros(80, 48), prime=y)
    full.step(4)
    sq = full.suspend(hq)
    assert sq.blob is None and torch.equal(sq.prime, y)
    other = SlotStream(PrimeFakeEngine(4), 64, pcm=False)
    hr = other.resume(sq)
    assert other.step(31)[hr][0].tolist() == list(range(500, 531))


# ---- the oracle alone: behind a foreign prime the model goes another way -------------------------------------------------------------

@pytest.mark.parametrize("cc", [PC.COND, PC.COND_A1024], ids=lambda c: c.name)
def test_the_oracle_leaves_its_free_run_behind_a_foreign_prime(cc):
    """The condition of the foreign-prime GPU test, on the fp32 oracle: its free run y0 against its run behind the foreign primes
    of prime_cases.foreign_primes (PC.FOREIGN_SEED).  The oracle can only be forced over a whole run, so the run behind the primes
    is built pass by pass -- pass i feeds [prime ; the picks of pass i - 1] and makes the samples n .. n + i exact --; two passes
    already show at least 90 % of the columns with 0 < n < 48 leaving y0 within their first two samples behind the prime."""
    case, m, x, w, t = PC.inputs(cc, 32)
    s = case.shape
    o = O.Oracle(s.L, s.B, s.N, s.R, s.S, s.A, s.maxD)
    o.set_model(t)
    o.set_tanh_embed(True)
    o.set_inputs(t.Lh, t.sel)
    y0 = o.run(s.N)
    o.close()
    lengths = PC.prime_lengths(s.B)
    inner = PC.inner_columns(lengths, s.N)
    assert len(inner) == {40: 33, 16: 13}[s.B]
    p = PC.foreign_primes(s.A, y0)
    forced = y0.copy()
    for b, n in enumerate(lengths):
        forced[b, :n] = p[b, :n]
    passes = 2
    for i in range(passes):
        own = util.teacher_forced_oracle(case, t, forced)["y"]
        for b, n in enumerate(lengths):
            forced[b, n:] = own[b, n:]
    differ = [b for b in inner if not np.array_equal(forced[b, lengths[b]:lengths[b] + passes], y0[b, lengths[b]:lengths[b] + passes])]
    print("%s: %d of %d columns leave the free run within %d samples behind their prime" % (cc.name, len(differ), len(inner), passes))
    assert len(differ) >= 0.9 * len(inner), (len(differ), len(inner))
