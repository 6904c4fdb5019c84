"""CPU tests of the probability floor (min-p; no GPU): the three entry points within ABI 7; the word helpers, the
refusals and sizeof(Params) through the host compiler; the numpy mirror of the rule with four negative controls, each rejected by the
support and CDF checks the GPU tests use (tests/min_p_cases.py), on free runs of the float64 reference of tests/score_cases.py;
min_p_rows; the floor word of a state blob through SlotState.to_bytes / from_bytes; and the SlotStream bookkeeping against a stub
engine that models slotSetMinP by the engine's rules (a start puts the column back to 0, a move carries the value, a resume takes
the blob's)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import min_p_cases as MP
import score_cases as SC
from oracle import oracle as O
from test_slots_state_cpu import HEADER_BYTES
from test_temperature_cpu import TemperatureFakeEngine, _kinds, _synthetic_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nv_wavenet_amd", "csrc")
MIN_P_SYMBOLS = ("nvw_set_min_p", "nvw_slot_set_min_p", "nvw_slot_min_p")
WORD = 11                                    # of the blob's header: the floor as the bits of the float, zero for 0
PARAMS_BYTES = 1816                          # sizeof(wn::Params) before floors existed


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------

def test_min_p_entries_are_declared_exported_and_bound_within_abi_7():
    from nv_wavenet_amd import _lib, engine, slots
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    import inspect
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert "PROBABILITY FLOOR" in header
    for name in MIN_P_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert _lib.SIGNATURES["nvw_slot_min_p"][0] is ctypes.c_float
    assert _lib.SIGNATURES["nvw_slot_set_min_p"][1][-1] is ctypes.c_float
    for name in ("setMinP", "slotSetMinP", "slotMinP"):
        assert hasattr(engine.WavenetEngine, name), name
    for name in ("set_min_p", "min_p"):
        assert hasattr(slots.SlotStream, name), name
    assert slots.SlotState.MIN_P_WORD == WORD and callable(slots.min_p_rows)
    for fn in (slots.SlotStream.submit, slots.SlotStream.submit_mel):
        assert inspect.signature(fn).parameters["min_p"].default == 0.0
    for fn in (NVWaveNetEngine.infer, NVWaveNetEngine.infer_features):
        assert inspect.signature(fn).parameters["min_p"].default is None


# ---- the helpers of slots_sampler.hpp and sizeof(Params), through the host compiler ------------------------------------------------

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <cmath>
#include "wn_kernels.hpp"
#include "slots_sampler.hpp"
#include "slots_state.hpp"
static unsigned bits(float v) { unsigned w; memcpy(&w, &v, 4); return w; }
static float of_bits(unsigned w) { float v; memcpy(&v, &w, 4); return v; }
int main() {
    printf("sizeof_Params %zu\n", sizeof(wn::Params));
    printf("offsetof_floorOn %zu\n", offsetof(wn::Params, floorOn));
    printf("sizeof_SlotSave %zu\n", sizeof(wn::SlotSave));
    printf("offsetof_minp %zu\n", offsetof(wn::SlotSave, minp));
    printf("sizeof_SlotStateHeader %zu\n", sizeof(wn::SlotStateHeader));
    printf("offsetof_pad1 %zu\n", offsetof(wn::SlotStateHeader, pad) + 4);
    const float vals[] = {0.0f, -0.0f, 0.05f, 0.1f, 0.25f, 0.5f, 1e-30f, -0.1f, 0.6f, 0.50000006f, NAN, INFINITY, -INFINITY, 1.0f};
    for (float v : vals) {
        float back = -7.0f;
        const int w = wn::min_p_word(v);
        const bool okw = wn::min_p_of_word(w, back);
        printf("value %08x ok %d word %08x word_ok %d back %08x\n", bits(v), (int)wn::min_p_ok(v), (unsigned)w, (int)okw, bits(back));
    }
    const unsigned words[] = {0u, bits(0.25f), bits(-0.0f), bits(-0.1f), bits(0.6f), bits(NAN), bits(INFINITY), 1u, 7u, bits(1.0f)};
    for (unsigned w : words) {
        float back = -7.0f;
        const bool okw = wn::min_p_of_word((int)w, back);
        printf("word %08x word_ok %d back %08x\n", w, (int)okw, bits(back));
    }
    (void)of_bits;
    return 0;
}
"""


def _bits(v):
    return int(np.array([v], dtype="<f4").view("<u4")[0])


@pytest.fixture(scope="module")
def helper_report(tmp_path_factory):
    d = tmp_path_factory.mktemp("min_p_words")
    src, exe = d / "min_p_words.hip", d / "min_p_words"
    src.write_text(PROGRAM)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O1", "-std=c++17", "-Wno-unused-result", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()


def test_params_did_not_grow_and_the_floor_words_have_their_places(helper_report):
    got = dict(ln.split() for ln in helper_report if len(ln.split()) == 2)
    assert int(got["sizeof_Params"]) == PARAMS_BYTES and int(got["offsetof_floorOn"]) == PARAMS_BYTES - 4
    assert int(got["sizeof_SlotSave"]) == 32 and int(got["offsetof_minp"]) == 28
    assert int(got["sizeof_SlotStateHeader"]) == 64 and int(got["offsetof_pad1"]) == 4 * WORD
    src = open(os.path.join(CSRC, "wn_kernels.hpp")).read()
    assert "static_assert(sizeof(Params) == %d" % PARAMS_BYTES in src


def test_the_word_helpers_accept_the_floors_and_refuse_everything_else(helper_report):
    vals = {}
    for ln in helper_report:
        f = ln.split()
        if f[0] == "value":
            vals[int(f[1], 16)] = (int(f[3]), int(f[5], 16), int(f[7]), int(f[9], 16))
    for good in (0.0, 0.05, 0.1, 0.25, 0.5, 1e-30):
        ok, word, word_ok, back = vals[_bits(good)]
        assert ok == 1 and word == (_bits(good) if good != 0.0 else 0) and word_ok == 1 and back == _bits(good), good
    assert vals[_bits(-0.0)][:3] == (1, 0, 1)                                # -0 is 0: all-zero bits
    for bad in (-0.1, 0.6, 0.50000006, float("nan"), float("inf"), float("-inf"), 1.0):
        assert vals[_bits(bad)][0] == 0, bad
    words = {int(ln.split()[1], 16): (int(ln.split()[3]), int(ln.split()[5], 16)) for ln in helper_report if ln.startswith("word ")}
    assert words[0] == (1, _bits(0.0)) and words[_bits(0.25)] == (1, _bits(0.25))
    for bad in (_bits(-0.0), _bits(-0.1), _bits(0.6), _bits(float("nan")), _bits(float("inf")), _bits(1.0)):
        assert words[bad][0] == 0, hex(bad)
    assert words[1][0] == 1 and words[7][0] == 1                              # (a denormal is a small positive floor)


def test_check_min_p_is_the_engines_range():
    from nv_wavenet_amd.slots import check_min_p
    for good in (0, 0.0, -0.0, 0.05, 0.5, np.float32(0.25)):
        assert check_min_p(good) == float(np.float32(good))
    assert str(check_min_p(-0.0)) == "0.0"
    for bad in MP.BAD_FLOORS + (0.50001, "low", None):
        with pytest.raises(ValueError):
            check_min_p(bad)


# ---- the rule, mirrored in numpy, with negative controls ---------------------------------------------------------------------------

SEED = 5
COLUMNS = 5
_runs = {}


def _setup():
    if "setup" not in _runs:
        shape, seed, L, maxD, N = SC.PRIME_SHAPE
        case, t, x, w, b = SC.setup(shape, seed, 32, L, maxD, N, COLUMNS)
        Lh = [SC.lh_of(x[c], w, b, case.shape.R, L) for c in range(COLUMNS)]
        u = O.philox_selectors(SEED, N, COLUMNS).astype(np.float64)
        _runs["setup"] = (case, t, Lh, u)
    return _runs["setup"]


def _free_run(c, T, picker):
    """(y [N], rows [N][A]) of column c drawn sample by sample by `picker(rows_T [1][A], rows_1 [1][A], u [1]) -> y [1]` on the float64
    reference; rows = the log-probabilities at temperature T of every sample of the finished run"""
    case, t, Lh, u = _setup()
    s = case.shape
    y = np.zeros(s.N, dtype=np.int64)
    for k in range(s.N):
        Za, _ = SC.reference(t, s, y[:k + 1], Lh[c])
        y[k] = min(int(picker(SC.log_softmax(Za[k:k + 1], T), SC.log_softmax(Za[k:k + 1], 1.0), u[k:k + 1, c])[0]), s.A - 1)
    Za, _ = SC.reference(t, s, y, Lh[c])
    return y, SC.log_softmax(Za, T), float(np.abs(Za).max())


def _restricted(rows, keep, u):
    """the pick from the distribution exp(rows) restricted to `keep` and renormalised"""
    e = np.where(keep, np.exp(rows - rows.max(axis=1, keepdims=True)), 0.0)
    cum = np.cumsum(e, axis=1)
    first = (cum <= (u * cum[:, -1])[:, None]).sum(axis=1)
    return np.where(first < rows.shape[1], first, 128)


def _samplers(tau, neighbour):
    return {
        "the rule": lambda rT, r1, u: MP.pick_min_p(rT, u, tau),
        "floor ignored": lambda rT, r1, u: MP.pick_min_p(rT, u, 0.0),
        "floor on the untempered distribution": lambda rT, r1, u: _restricted(rT, MP.kept(r1, tau), u),
        "floor against the sum": lambda rT, r1, u: _restricted(rT, np.exp(rT) >= tau, u),
        "the neighbouring column's floor": lambda rT, r1, u: MP.pick_min_p(rT, u, neighbour),
    }


def _totals(name, T):
    """check_run's totals over the columns whose floor is not 0, each drawn by sampler `name` at temperature T"""
    from nv_wavenet_amd.slots import min_p_rows
    key = (name, T)
    if key not in _runs:
        case, t, Lh, u = _setup()
        taus = MP.floors(COLUMNS)
        tot = np.zeros(4, dtype=np.int64)
        for c in range(COLUMNS):
            if taus[c] == 0.0:
                continue
            y, rows, za_max = _free_run(c, T, _samplers(taus[c], taus[(c + 1) % COLUMNS])[name])
            eps = MP.epsilon(T, za_max, float(np.abs(rows[np.isfinite(rows)]).max()))
            assert 1e-6 < eps < 1e-4, eps
            tot += np.array(MP.check_column(rows, y, u[:, c], taus[c], eps, min_p_rows))
        _runs[key] = tuple(int(v) for v in tot)
    return _runs[key]


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_the_mirror_passes_the_checks_the_gpu_tests_use(T):
    tot = _totals("the rule", T)
    print("T = %g: support violations %d, CDF violations %d, left out %d of %d rows" % ((T,) + tot))
    assert MP.accepted(tot), tot


@pytest.mark.parametrize("control,T", [("floor ignored", 0.5), ("floor ignored", 1.0), ("floor ignored", 2.0),
                                       ("floor on the untempered distribution", 0.5), ("floor on the untempered distribution", 2.0),
                                       ("floor against the sum", 0.5), ("floor against the sum", 1.0), ("floor against the sum", 2.0),
                                       ("the neighbouring column's floor", 0.5), ("the neighbouring column's floor", 1.0),
                                       ("the neighbouring column's floor", 2.0)])
def test_every_negative_control_is_rejected_by_the_same_checks(control, T):
    tot = _totals(control, T)
    print("%s, T = %g: support violations %d, CDF violations %d, left out %d of %d rows" % ((control, T) + tot))
    assert not MP.accepted(tot), (control, T, tot)
    assert tot[0] + tot[1] >= 3, "a control that differs in fewer than three samples has no power: %s" % (tot,)


def test_draws_from_the_unfloored_distribution_leave_the_kept_set_often():
    """the power of the "floor ignored" control: the share of unfloored draws outside the kept set, per floor (T = 1)"""
    case, t, Lh, u = _setup()
    shares = {}
    for tau in MP.FLOORS[1:]:
        out = n = 0
        for c in range(COLUMNS):
            y, rows, _ = _free_run(c, 1.0, lambda rT, r1, uu: MP.pick_min_p(rT, uu, 0.0))
            out += int((~MP.kept(rows, tau)[np.arange(len(y)), y]).sum())
            n += len(y)
        shares[tau] = out / n
    print("unfloored draws outside the kept set: %s" % {k: round(v, 3) for k, v in shares.items()})
    # a higher floor keeps a subset; every floor leaves at least three of the 240 draws outside (below that the control has no
    # power, as in the test above); at 0.5 only bins within a factor two of the maximum stay: the majority of draws is outside
    assert all(shares[a] <= shares[b] for a, b in zip(MP.FLOORS[1:], MP.FLOORS[2:])) and shares[0.05] * n >= 3 and shares[0.5] >= 0.5, shares


def test_the_floor_zero_mirror_is_the_plain_inverse_cdf_pick():
    rng = np.random.default_rng(2)
    rows = SC.log_softmax(rng.standard_normal((64, 256)) * 3.0)
    u = rng.random(64)
    y = MP.pick_min_p(rows, u, 0.0)
    inside, _, _ = SC.cdf_check(rows, y, u)
    assert inside.all()
    assert (MP.pick_min_p(rows, u, 0.5) != y).any()


def test_min_p_rows_is_the_floored_renormalised_distribution():
    from nv_wavenet_amd.slots import min_p_rows
    rng = np.random.default_rng(4)
    rows = SC.log_softmax(rng.standard_normal((7, 256)) * 2.5).astype(np.float32)
    for tau in (0.0, 0.05, 0.5):
        out = min_p_rows(rows, tau)
        assert out.dtype == np.float32 and out.shape == rows.shape
        keep = MP.kept(rows, tau)
        assert np.array_equal(np.isfinite(out), keep) and (out[~keep] == -np.inf).all()
        assert np.abs(np.exp(out.astype(np.float64)).sum(axis=1) - 1.0).max() <= 256 * 4 * SC.EPS32
        p = np.exp(rows.astype(np.float64))
        ref = np.where(keep, p, 0.0) / np.where(keep, p, 0.0).sum(axis=1, keepdims=True)
        assert np.abs(np.exp(out.astype(np.float64)) - ref).max() <= 4 * SC.EPS32
        assert keep[np.arange(7), rows.argmax(axis=1)].all()                 # the most probable bin always stays
    per_row = min_p_rows(rows, [0.0, 0.05, 0.1, 0.25, 0.5, 0.0, 0.5])
    assert np.array_equal(per_row[4], min_p_rows(rows, 0.5)[4]) and np.array_equal(per_row[0], min_p_rows(rows, 0.0)[0])
    one = min_p_rows(rows[3], 0.25)
    assert one.shape == (256,) and np.array_equal(one, min_p_rows(rows, 0.25)[3])
    tt = min_p_rows(torch.from_numpy(rows), 0.25)
    assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), min_p_rows(rows, 0.25))
    for bad in (-0.1, 0.6, float("nan"), [0.1, 0.2]):
        with pytest.raises(ValueError):
            min_p_rows(rows, bad)


# ---- SlotState ---------------------------------------------------------------------------------------------------------------------

def _floored_blob(p, temperature=None, done=13, uid=4):
    blob = _synthetic_blob(5, 8, done, uid, temperature)
    blob.numpy().view("<u4")[WORD] = MP.bits(p)
    return blob


def test_the_floor_survives_to_bytes_and_from_bytes():
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    R = SlotState.RECORD_BYTES
    # word 11 zero reads as 0; a blob made at floor 0 keeps its bytes through the trip
    blob = _synthetic_blob(5, 8, 13, 4)
    s0 = SlotState(blob, src, 4, 13, "features")
    assert s0.min_p == 0.0 and s0.to_bytes()[R:] == blob.numpy().tobytes()
    assert SlotState.from_bytes(s0.to_bytes(), src).min_p == 0.0
    for p in (0.05, 0.1, 0.25, 0.5):
        p = float(np.float32(p))
        blob = _floored_blob(p, 0.5)
        data = SlotState(blob, src, 4, 13, "mel", 9, False, temperature=0.5, min_p=p).to_bytes()
        assert data[R:] == blob.numpy().tobytes()
        back = SlotState.from_bytes(data, src)
        assert (back.min_p, back.temperature, back.kind, back.frames, back.final, back.done) == (p, 0.5, "mel", 9, False, 13)
        assert back._blob_sampling.min_p == p and back.to_bytes() == data
    # a prefilled or scored state: the blob's word 11 is zero, the state's floor is not -- the bytes carry it
    st = SlotState(_synthetic_blob(5, 8, 13, 4), src, 4, 13, "features")
    st.min_p = 0.25
    assert st._blob_sampling.min_p == 0.0
    data = st.to_bytes()
    assert np.frombuffer(data, dtype="<u4", count=16, offset=R)[WORD] == MP.bits(0.25)
    back = SlotState.from_bytes(data, src)
    assert back.min_p == 0.25 and back._blob_sampling.min_p == 0.25
    # a request that had not started: the record alone at floor 0 (as before), the record and a bare header otherwise
    assert len(SlotState(None, src, 3, 0, "features").to_bytes()) == R
    data = SlotState(None, src, 3, 0, "features", min_p=0.1).to_bytes()
    assert len(data) == R + HEADER_BYTES
    words = np.frombuffer(data, dtype="<u4", count=16, offset=R)
    assert words[WORD] == MP.bits(float(np.float32(0.1))) and words[10] == 0
    back = SlotState.from_bytes(data, src)
    assert back.blob is None and back.min_p == float(np.float32(0.1)) and back.temperature == 1.0 and back.to_bytes() == data
    both = SlotState.from_bytes(SlotState(None, src, 3, 0, "mel", 2, False, temperature=0.5, min_p=0.5).to_bytes(), src)
    assert (both.blob, both.min_p, both.temperature) == (None, 0.5, 0.5)


@pytest.mark.parametrize("word", [_bits(-0.1), _bits(0.6), _bits(float("nan")), _bits(float("inf")), _bits(1.0)])
def test_from_bytes_refuses_a_bad_floor_word(word):
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    blob = _synthetic_blob(5, 8, 9, 2)
    blob.numpy().view("<u4")[WORD] = word
    data = SlotState.RECORD.pack(b"NWSS", 1, 0, 0, 0, 2, 9, blob.numel()) + blob.numpy().tobytes()
    with pytest.raises(ValueError):
        SlotState.from_bytes(data, src)


# ---- SlotStream against a stub engine ----------------------------------------------------------------------------------------------

class MinPFakeEngine(TemperatureFakeEngine):
    """TemperatureFakeEngine with the floor by the engine's rules: per column, 0 after a start, the blob's after a resume, carried by a
    move; slotSetMinP needs an utterance (or a pending start or resume) in the column.  Blobs are ("blob", uid, done, T, p).
    floors_at_step[i]: {uid: p} in force for step i."""

    def __init__(self, columns, window=64):
        super().__init__(columns, window)
        self.minp = {}
        self.floors_at_step = []

    def slotStart(self, col, x, uid, length=None):
        super().slotStart(col, x, uid, length)
        self.minp[col] = 0.0

    def slotStartMel(self, col, mel, uid, frames=None, final=True):
        super().slotStartMel(col, mel, uid, frames, final)
        self.minp[col] = 0.0

    def slotResume(self, col, blob, x, length=None):
        super().slotResume(col, blob, x, length)
        self.minp[col] = blob[4]

    def slotResumeMel(self, col, blob, mel, frames=None, final=True):
        super().slotResumeMel(col, blob, mel, frames, final)
        self.minp[col] = blob[4]

    def slotStop(self, col):
        super().slotStop(col)
        self.minp.pop(col)

    def slotMove(self, src, dst):
        super().slotMove(src, dst)
        self.minp[dst] = self.minp.pop(src)

    def slotSave(self, col, stream=None):
        blob, done = super().slotSave(col, stream)
        return blob + (self.minp[col],), done

    def slotSetMinP(self, col, p):
        assert col in self.active, "a floor for a column without an utterance"
        assert 0.0 <= p <= 0.5
        self.calls.append(("min_p", col, p))
        self.minp[col] = p

    def slotsStep(self, count, y, pcm):
        self.floors_at_step.append({self.active[c][0]: self.minp[c] for c in self.active})
        return super().slotsStep(count, y, pcm)


@pytest.mark.parametrize("bad", list(MP.BAD_FLOORS) + [0.50001, "low", None])
def test_bad_floors_raise_everywhere_and_change_nothing(bad):
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = MinPFakeEngine(4)
    st = SlotStream(eng, 64)
    x = torch.zeros(80, 30)
    with pytest.raises(ValueError):
        st.submit(x, min_p=bad)
    with pytest.raises(ValueError):
        st.submit_mel(torch.zeros(80, 5), min_p=bad)
    assert not st.busy() and st._next_handle == 0
    h = st.submit(x, min_p=0.25)
    with pytest.raises(ValueError):
        st.set_min_p(h, bad)                        # waiting
    st.step(4)
    with pytest.raises(ValueError):
        st.set_min_p(h, bad)                        # running
    assert st.min_p(h) == 0.25 and eng.minp[0] == 0.25
    assert [c for c in eng.calls if c[0] == "min_p"] == [("min_p", 0, 0.25)]
    with pytest.raises(ValueError):
        SlotState(None, x, 0, 0, "features", min_p=bad)
    with pytest.raises(KeyError):
        st.set_min_p(99, 0.1)
    with pytest.raises(KeyError):
        st.min_p(99)
    st.close()


def test_submit_with_a_floor_sets_it_after_the_start_and_before_the_step():
    from nv_wavenet_amd.slots import SlotStream
    eng = MinPFakeEngine(3)
    st = SlotStream(eng, 64)
    a = st.submit(torch.zeros(80, 12), min_p=0.5)
    b = st.submit(torch.zeros(80, 12))                                   # floor 0: no call at all
    c = st.submit_mel(torch.zeros(80, 3), temperature=2.0, min_p=0.25)
    d = st.submit(torch.zeros(80, 8), min_p=0.125)                       # waits for a column
    st.step(4)
    assert _kinds(eng) == ["begin", "start", "start", "start_mel", "temperature", "min_p", "min_p", "step"]
    assert [x for x in eng.calls if x[0] == "min_p"] == [("min_p", 0, 0.5), ("min_p", 2, 0.25)]
    assert eng.floors_at_step[0] == {0: 0.5, 1: 0.0, 2: 0.25} and eng.temps_at_step[0] == {0: 1.0, 1: 1.0, 2: 2.0}
    assert (st.min_p(a), st.min_p(b), st.min_p(c), st.min_p(d)) == (0.5, 0.0, 0.25, 0.125)
    st.set_min_p(b, 0.25)                                                # running: at once, in force from the next step
    assert eng.calls[-1] == ("min_p", 1, 0.25)
    st.step(4)
    assert eng.floors_at_step[1] == {0: 0.5, 1: 0.25, 2: 0.25}
    st.set_min_p(d, 0.5)                                                 # waiting: when it is admitted, after its start
    assert eng.calls[-1][0] == "step"
    st.step(4)
    before = len(eng.calls)
    st.step(4)
    assert _kinds(eng, before)[-3:] == ["start", "min_p", "step"] and eng.calls[-2] == ("min_p", 0, 0.5)
    assert eng.floors_at_step[3] == {3: 0.5}
    while st.busy():
        st.step(4)
    assert st._sampling == {}                                                # nothing is kept of a finished request
    st.close()


def test_compact_suspend_and_resume_keep_the_floor():
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = MinPFakeEngine(40)
    st = SlotStream(eng, 64)
    hs = [st.submit(torch.zeros(80, 4 if i < 38 else 40), min_p=0.0 if i < 38 else (0.5, 0.25)[i - 38]) for i in range(40)]
    st.step(4)
    assert st.compact() == 2                                             # 39 -> 0, 38 -> 1: the engine's move carries the value
    n_set = len([c for c in eng.calls if c[0] == "min_p"])
    st.step(4)
    assert eng.floors_at_step[-1] == {39: 0.25, 38: 0.5} and (eng.minp[0], eng.minp[1]) == (0.25, 0.5)
    assert len([c for c in eng.calls if c[0] == "min_p"]) == n_set, "a move needs no new call"
    # suspend: the state carries it; resume in another stream: the engine takes it from the blob, no call
    state = st.suspend(hs[39])
    assert state.min_p == 0.25 and state.blob[4] == 0.25 and state.done == 8
    other_eng = MinPFakeEngine(2)
    other = SlotStream(other_eng, 64)
    h2 = other.resume(state)
    assert other.min_p(h2) == 0.25
    other.step(4)
    assert other_eng.floors_at_step[0] == {39: 0.25} and "min_p" not in _kinds(other_eng)
    # ... unless it was changed on the state, or the blob's word is not the state's floor (a prefilled one): resume, then set
    state = other.suspend(h2)
    state.min_p = 0.5
    h3 = other.resume(state)
    other.step(4)
    assert _kinds(other_eng)[-3:] == ["resume", "min_p", "step"] and other_eng.floors_at_step[-1] == {39: 0.5}
    # a request suspended before it started keeps it too (through bytes as well)
    w3 = other.submit(torch.zeros(80, 6), min_p=0.1)
    waiting = other.suspend(w3)
    assert waiting.blob is None and waiting.min_p == float(np.float32(0.1))
    again = SlotState.from_bytes(waiting.to_bytes(), waiting.source)
    assert again.blob is None and again.min_p == waiting.min_p
    h4 = st.resume(again)
    st.step(4)
    assert eng.floors_at_step[-1][again.uid] == waiting.min_p and st.min_p(h4) == waiting.min_p
    assert other.suspend(h3).min_p == 0.5 and other._sampling == {}
    other.close()
    st.close()
