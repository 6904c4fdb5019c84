"""CPU tests of the tail cuts (top-k and top-p; no GPU): the six entry points within ABI 7; the word helpers, the
refusals and the sizes of Params, SlotSave and SlotStateHeader through the host compiler; the numpy mirror of the kernel's
bit-pattern bisection against the definition by a sort, on random and adversarial rows; the mirror of the rule with six negative
controls, each rejected by the candidate check the GPU tests use (tests/cut_cases.py), on free runs of the float64 reference of
tests/score_cases.py, where at most 5 % of the rows may have more than one candidate; cut_rows; words 12 and 13 of a state blob
through SlotState.to_bytes / from_bytes; and the SlotStream bookkeeping against a stub engine that models the cuts by the engine's
rules (a start puts the column back to off, a move carries the values, a resume takes the blob's)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import cut_cases as CC
import min_p_cases as MP
import score_cases as SC
from oracle import oracle as O
from test_min_p_cpu import MinPFakeEngine
from test_slots_state_cpu import HEADER_BYTES
from test_temperature_cpu import _kinds, _synthetic_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nv_wavenet_amd", "csrc")
CUT_SYMBOLS = ("nvw_set_top_k", "nvw_set_top_p", "nvw_slot_set_top_k", "nvw_slot_set_top_p", "nvw_slot_top_k", "nvw_slot_top_p",
               "nvw_sampler_mask")
K_WORD, P_WORD = 12, 13                      # of the blob's header: top-k as the integer, top-p as the bits of the float (zero: 1)
PARAMS_BYTES = 1816


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------

def test_cut_entries_are_declared_exported_and_bound_within_abi_7():
    from nv_wavenet_amd import _lib, engine, slots
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    import inspect
    assert _lib.ABI_VERSION == 7 and _lib.lib.nvw_abi_version() == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert "TAIL CUTS" in header
    for name in CUT_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert _lib.SIGNATURES["nvw_slot_top_p"][0] is ctypes.c_float and _lib.SIGNATURES["nvw_slot_top_k"][0] is ctypes.c_int
    assert _lib.SIGNATURES["nvw_slot_set_top_p"][1][-1] is ctypes.c_float and _lib.SIGNATURES["nvw_slot_set_top_k"][1][-1] is ctypes.c_int
    for name in ("setTopK", "setTopP", "slotSetTopK", "slotSetTopP", "slotTopK", "slotTopP", "samplerMask"):
        assert hasattr(engine.WavenetEngine, name), name
    for name in ("set_top_k", "set_top_p", "top_k", "top_p"):
        assert hasattr(slots.SlotStream, name), name
    assert (slots.SlotState.TOP_K_WORD, slots.SlotState.TOP_P_WORD) == (K_WORD, P_WORD) and callable(slots.cut_rows)
    for fn in (slots.SlotStream.submit, slots.SlotStream.submit_mel):
        assert inspect.signature(fn).parameters["top_k"].default == 0 and inspect.signature(fn).parameters["top_p"].default == 1.0
    for fn in (NVWaveNetEngine.infer, NVWaveNetEngine.infer_features):
        assert inspect.signature(fn).parameters["top_k"].default is None and inspect.signature(fn).parameters["top_p"].default is None


# ---- the helpers of slots_sampler.hpp and the sizes, through the host compiler -----------------------------------------------------

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <cmath>
#include "wn_kernels.hpp"
#include "slots_sampler.hpp"
#include "slots_state.hpp"
static unsigned bits(float v) { unsigned w; memcpy(&w, &v, 4); return w; }
int main() {
    printf("sizeof_Params %zu\n", sizeof(wn::Params));
    printf("offsetof_floorOn %zu\n", offsetof(wn::Params, floorOn));
    printf("sizeof_SlotSave %zu\n", sizeof(wn::SlotSave));
    printf("offsetof_minp %zu\n", offsetof(wn::SlotSave, minp));
    printf("sizeof_SlotSaveCut %zu\n", sizeof(wn::SlotSaveCut));
    printf("sizeof_SlotStateHeader %zu\n", sizeof(wn::SlotStateHeader));
    printf("offsetof_pad2 %zu\n", offsetof(wn::SlotStateHeader, pad) + 8);
    const float ps[] = {1.0f, 0.5f, 0.8f, 0.9f, 1e-30f, 0.99999994f, 0.0f, -0.0f, -0.5f, 1.0000001f, 1.5f, NAN, INFINITY, -INFINITY};
    for (float v : ps) {
        float back = -7.0f;
        const int w = wn::top_p_word(v);
        const bool okw = wn::top_p_of_word(w, back);
        printf("p %08x ok %d word %08x word_ok %d back %08x\n", bits(v), (int)wn::top_p_ok(v), (unsigned)w, (int)okw, bits(back));
    }
    const unsigned words[] = {0u, bits(0.5f), bits(1.0f), bits(-0.0f), bits(-0.5f), bits(1.5f), bits(NAN), bits(INFINITY), 1u};
    for (unsigned w : words) {
        float back = -7.0f;
        const bool okw = wn::top_p_of_word((int)w, back);
        printf("pword %08x word_ok %d back %08x\n", w, (int)okw, bits(back));
    }
    const int ks[] = {0, 1, 4, 32, 255, 256, 257, -1, 1024, 1025, -2147483647 - 1, 2147483647};
    for (int k : ks)
        for (int A : {256, 1024}) {
            int back = -7;
            const bool okw = wn::top_k_of_word(wn::top_k_word(k), A, back);
            int e = 0;
            const float f = wn::top_k_entry(k);
            memcpy(&e, &f, 4);
            printf("k %d A %d ok %d word %d word_ok %d back %d entry %d\n", k, A, (int)wn::top_k_ok(k, A), wn::top_k_word(k), (int)okw, back, e);
        }
    // the record helpers beside the per-kind ones: off, each field alone at a valid value, all four, each field alone at a bad one
    const wn::Sampling recs[] = {{}, {0.5f, 0.0f, 0, 1.0f}, {1.0f, 0.25f, 0, 1.0f}, {1.0f, 0.0f, 32, 1.0f}, {1.0f, 0.0f, 0, 0.9f},
                                 {2.0f, 0.1f, 4, 0.8f}, {4096.0f, 0.0f, 0, 1.0f}, {1.0f, 0.6f, 0, 1.0f}, {1.0f, 0.0f, 257, 1.0f},
                                 {1.0f, 0.0f, 0, 1.5f}};
    for (const wn::Sampling& s : recs) {
        const int A = 256;
        int w[4];
        wn::sampling_words(s, w);
        const int pw[4] = {wn::temperature_word(s.temperature), wn::min_p_word(s.minP), wn::top_k_word(s.topK), wn::top_p_word(s.topP)};
        wn::Sampling back{-7.0f, -7.0f, -7, -7.0f}, pb{-7.0f, -7.0f, -7, -7.0f};
        const bool okb = wn::sampling_of_words(w, A, back);
        const bool pokb[4] = {wn::temperature_of_word(pw[0], pb.temperature), wn::min_p_of_word(pw[1], pb.minP),
                              wn::top_k_of_word(pw[2], A, pb.topK), wn::top_p_of_word(pw[3], pb.topP)};
        float e[4];
        wn::sampling_entries(s, e);
        const float pe[4] = {wn::temperature_scale(s.temperature), s.minP, wn::top_k_entry(s.topK), s.topP};
        printf("rec %x %x %x %x %x", (int)wn::sampling_ok(s, A), (int)wn::temperature_ok(s.temperature), (int)wn::min_p_ok(s.minP),
               (int)wn::top_k_ok(s.topK, A), (int)wn::top_p_ok(s.topP));
        for (int i = 0; i < 4; i++) printf(" %x", (unsigned)w[i]);
        for (int i = 0; i < 4; i++) printf(" %x", (unsigned)pw[i]);
        printf(" %x %x %x %x %x", (int)okb, (int)pokb[0], (int)pokb[1], (int)pokb[2], (int)pokb[3]);
        printf(" %x %x %x %x", bits(back.temperature), bits(back.minP), (unsigned)back.topK, bits(back.topP));
        printf(" %x %x %x %x", bits(pb.temperature), bits(pb.minP), (unsigned)pb.topK, bits(pb.topP));
        for (int i = 0; i < 4; i++) printf(" %x", bits(e[i]));
        for (int i = 0; i < 4; i++) printf(" %x", bits(pe[i]));
        printf(" %x %x\n", (int)(s == wn::Sampling{}), (int)(back == s));
    }
    return 0;
}
"""


def _bits(v):
    return int(np.array([v], dtype="<f4").view("<u4")[0])


@pytest.fixture(scope="module")
def helper_report(tmp_path_factory):
    d = tmp_path_factory.mktemp("cut_words")
    src, exe = d / "cut_words.hip", d / "cut_words"
    src.write_text(PROGRAM)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O1", "-std=c++17", "-Wno-unused-result", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()


def test_params_slot_save_and_the_header_are_the_sizes_they_were(helper_report):
    got = dict(ln.split() for ln in helper_report if len(ln.split()) == 2)
    assert int(got["sizeof_Params"]) == PARAMS_BYTES and int(got["offsetof_floorOn"]) == PARAMS_BYTES - 4
    assert int(got["sizeof_SlotSave"]) == 32 and int(got["offsetof_minp"]) == 28 and int(got["sizeof_SlotSaveCut"]) == 8
    assert int(got["sizeof_SlotStateHeader"]) == 64 and int(got["offsetof_pad2"]) == 4 * K_WORD


def test_the_word_helpers_accept_the_cuts_and_refuse_everything_else(helper_report):
    vals = {}
    for ln in helper_report:
        f = ln.split()
        if f[0] == "p":
            vals[int(f[1], 16)] = (int(f[3]), int(f[5], 16), int(f[7]), int(f[9], 16))
    for good in (1.0, 0.5, 0.8, 0.9, 1e-30, 0.99999994):
        ok, word, word_ok, back = vals[_bits(good)]
        assert ok == 1 and word == (_bits(good) if good != 1.0 else 0) and word_ok == 1 and back == _bits(good), good
    for bad in (0.0, -0.0, -0.5, 1.0000001, 1.5, float("nan"), float("inf"), float("-inf")):
        assert vals[_bits(bad)][0] == 0, bad
    words = {int(ln.split()[1], 16): (int(ln.split()[3]), int(ln.split()[5], 16)) for ln in helper_report if ln.startswith("pword ")}
    assert words[0] == (1, _bits(1.0)) and words[_bits(0.5)] == (1, _bits(0.5)) and words[1][0] == 1
    for bad in (_bits(1.0), _bits(-0.0), _bits(-0.5), _bits(1.5), _bits(float("nan")), _bits(float("inf"))):
        assert words[bad][0] == 0, hex(bad)          # (the bits of 1.0 are not a valid word: 1 is all-zero bits)
    ks = {}
    for ln in helper_report:
        f = ln.split()
        if f[0] == "k":
            ks[(int(f[1]), int(f[3]))] = tuple(int(f[i]) for i in (5, 7, 9, 11, 13))
    for A in (256, 1024):
        for k in (0, 1, 4, 32, 255, 256, 257, -1, 1024, 1025, -2 ** 31, 2 ** 31 - 1):
            ok, word, word_ok, back, entry = ks[(k, A)]
            good = 0 <= k <= A
            assert (ok, word_ok) == (int(good), int(good)) and word == k and entry == k and back == (k if good else 0), (k, A)


def test_the_record_helpers_are_the_per_kind_helpers_field_by_field(helper_report):
    """wn::Sampling through sampling_ok, sampling_words, sampling_of_words and sampling_entries against temperature_*, min_p_*,
    top_k_* and top_p_* on the same values (A = 256): off, each field alone at a valid value, all four, each field alone at a bad one."""
    recs = [[int(x, 16) for x in ln.split()[1:]] for ln in helper_report if ln.startswith("rec ")]
    values = [(1.0, 0.0, 0, 1.0), (0.5, 0.0, 0, 1.0), (1.0, 0.25, 0, 1.0), (1.0, 0.0, 32, 1.0), (1.0, 0.0, 0, 0.9), (2.0, 0.1, 4, 0.8),
              (4096.0, 0.0, 0, 1.0), (1.0, 0.6, 0, 1.0), (1.0, 0.0, 257, 1.0), (1.0, 0.0, 0, 1.5)]
    assert len(recs) == len(values)
    for i, (f, v) in enumerate(zip(recs, values)):
        ok, ok_kinds, words, kind_words = f[0], f[1:5], f[5:9], f[9:13]
        back_ok, back_ok_kinds, back, kind_back = f[13], f[14:18], f[18:22], f[22:26]
        entries, kind_entries, is_off, round_trip = f[26:30], f[30:34], f[34], f[35]
        as_bits = [_bits(v[0]), _bits(v[1]), v[2], _bits(v[3])]
        for kind in range(4):
            assert words[kind] == kind_words[kind], (i, kind)
            assert back[kind] == kind_back[kind], (i, kind)
            assert entries[kind] == kind_entries[kind], (i, kind)
        assert ok == int(all(ok_kinds)) and back_ok == int(all(back_ok_kinds)), i
        assert is_off == int(i == 0)
        if i < 6:                                       # valid: the words are the values' bits, zero where off, and come back as they went
            assert ok == 1 and back_ok == 1 and round_trip == 1, i
            assert words == [0 if v[k] == values[0][k] else as_bits[k] for k in range(4)] and back == as_bits, i
        else:                                           # one bad field: that kind alone is refused, as a value and as a word
            assert ok == 0 and back_ok == 0 and ok_kinds == back_ok_kinds == [int(k != i - 6) for k in range(4)], i
    assert recs[0][5:9] == [0, 0, 0, 0]                 # off is four zero words: the blobs of before the values existed
    assert recs[5][26:30] == [_bits(np.float32(1.4426950408889634) * (np.float32(1.0) / np.float32(2.0))), _bits(0.1), 4, _bits(0.8)]


def test_check_top_k_and_check_top_p_are_the_engines_ranges():
    from nv_wavenet_amd.slots import check_top_k, check_top_p
    for good in (0, 1, 4, 256, np.int32(7), 3.0):
        assert check_top_k(good, 256) == int(good) and isinstance(check_top_k(good), int)
    for bad in (-1, 257, 2.5, "many", None, float("nan"), 2 ** 31):
        with pytest.raises(ValueError):
            check_top_k(bad, 256)
    assert check_top_k(1000) == 1000                                       # (without an alphabet only the sign is checked)
    for good in (1, 1.0, 0.5, 0.9, np.float32(0.8), 1e-30):
        assert check_top_p(good) == float(np.float32(good))
    for bad in CC.BAD_TOP_PS + ("most", None):
        with pytest.raises(ValueError):
            check_top_p(bad)


# ---- the kernel's bisection, mirrored in numpy, against the definition by a sort ---------------------------------------------------

def _rows_for_the_search():
    rng = np.random.default_rng(11)
    A = 256
    rows = {}
    for i in range(4):
        e = np.exp2(-rng.random(A) * (2.0, 8.0, 20.0, 60.0)[i]).astype(np.float32)
        e[rng.integers(A)] = np.float32(1.0)
        rows["random %d" % i] = e
    rows["all equal"] = np.full(A, 1.0, dtype=np.float32)
    tied = np.exp2(-rng.random(A) * 6.0).astype(np.float32)
    tied[np.argsort(-tied)[2:9]] = np.sort(tied)[::-1][3]                  # the 3rd to 9th largest tie: k = 4 and k = 5 keep all of them
    rows["ties at the boundary"] = tied
    dom = np.full(A, 2.0 ** -40, dtype=np.float32)
    dom[77] = 1.0
    rows["one dominant bin"] = dom
    under = np.exp2(-rng.random(A) * 140.0).astype(np.float32)            # (some e underflow to 0)
    under[5] = np.float32(1.1892071)                                       # (an e_max above 1: the rounding of m c)
    rows["zeros and a maximum above one"] = under
    return rows


@pytest.mark.parametrize("LPU", [4, 8, 16])
def test_the_bisection_over_bit_patterns_equals_the_definition_by_a_sort(LPU):
    for name, e in _rows_for_the_search().items():
        A = len(e)
        for k, p in ((0, 1.0), (1, 1.0), (A, 1.0), (4, 1.0), (5, 1.0), (32, 1.0), (0, 0.5), (0, 0.9), (0, 1e-6), (0, 0.99999994), (4, 0.8),
                     (32, 0.5), (1, 0.9), (A, 0.8)):
            got, want = CC.bisect_threshold(e, k, p, LPU), CC.sorted_threshold(e, k, p, LPU)
            assert got == want, (name, k, p, got, want)
            assert CC.search_from_the_top(e, k, p, LPU) == want, (name, k, p)          # (the dump kernels' form of the search)
            keep = e >= got
            assert keep[np.argmax(e)] and keep.sum() >= 1, (name, k, p)                # the most probable bin always survives
            if p >= 1.0 and k > 0:
                assert keep.sum() >= k and (e >= np.nextafter(got, np.float32(np.inf))).sum() < k, (name, k)
            if k == 0 and p >= 1.0:
                assert got == 0.0                                                      # off: a select, every bin stays
            if k == A and p >= 1.0:
                assert keep.all()
    e = _rows_for_the_search()["ties at the boundary"]
    assert (e >= CC.bisect_threshold(e, 4, 1.0, LPU)).sum() == 9 and (e >= CC.bisect_threshold(e, 2, 1.0, LPU)).sum() == 2
    assert (_rows_for_the_search()["all equal"] >= CC.bisect_threshold(np.full(256, 1.0, dtype=np.float32), 1, 0.5, LPU)).all()
    dom = _rows_for_the_search()["one dominant bin"]
    assert (dom >= CC.bisect_threshold(dom, 0, 0.9, LPU)).sum() == 1 and (dom >= CC.bisect_threshold(dom, 0, 1e-6, LPU)).sum() == 1


def test_the_search_covers_every_non_negative_float_and_a_bound_of_zero_ends_at_the_maximum():
    rng = np.random.default_rng(12)
    e = np.exp2(-rng.random(256) * 30.0).astype(np.float32)
    e[3] = np.float32(3.0e38)                                              # (far beyond what exp2 of a non-positive exponent gives)
    for k, p in ((1, 1.0), (7, 1.0), (0, 0.5), (256, 0.9)):
        assert CC.bisect_threshold(e, k, p, 16) == CC.search_from_the_top(e, k, p, 16) == CC.sorted_threshold(e, k, p, 16)
    # a p so small that p S(0) rounds to zero: the mass predicate would hold at every threshold; it counts only while some bin
    # passes, so the search ends at the largest e -- greedy -- and never above it
    e = np.exp2(-rng.random(256) * 8.0).astype(np.float32)
    e[9] = np.float32(1.0)
    got = CC.bisect_threshold(e, 0, 1e-46, 16)
    assert CC.search_from_the_top(e, 0, 1e-46, 16) == got
    assert np.float32(np.float32(1e-46) * CC.group_sum(e, 16)) == 0.0 and got == e.max() and (e >= got).sum() == 1


# ---- the rule, mirrored in numpy, with negative controls ---------------------------------------------------------------------------

SEED = 5
COLUMNS = 20                                 # every pair of TOP_KS and TOP_PS once
_runs = {}


def _setup():
    """the network and the features of tests/test_min_p_cpu.py's reference, 20 columns of them"""
    if "setup" not in _runs:
        shape, seed, L, maxD, N = SC.PRIME_SHAPE
        case, t, x, w, b = SC.setup(shape, seed, 32, L, maxD, N, COLUMNS)
        Lh = [SC.lh_of(x[c], w, b, case.shape.R, L) for c in range(COLUMNS)]
        _runs["setup"] = (case, t, Lh, O.philox_selectors(SEED, N, COLUMNS).astype(np.float64))
    return _runs["setup"]


def _free_run(c, T, picker):
    """(y [N], rows [N][A], max |Za|) of column c drawn sample by sample by `picker(rows_T [1][A], rows_1 [1][A], u [1]) -> y [1]` on
    the float64 reference; rows = the log-probabilities at temperature T of every sample of the finished run"""
    case, t, Lh, u = _setup()
    s = case.shape
    y = np.zeros(s.N, dtype=np.int64)
    for k in range(s.N):
        Za, _ = SC.reference(t, s, y[:k + 1], Lh[c])
        y[k] = min(int(picker(SC.log_softmax(Za[k:k + 1], T), SC.log_softmax(Za[k:k + 1], 1.0), u[k:k + 1, c])[0]), s.A - 1)
    Za, _ = SC.reference(t, s, y, Lh[c])
    return y, SC.log_softmax(Za, T), float(np.abs(Za).max())


def _values():
    A = _setup()[0].shape.A
    return CC.top_ks(COLUMNS, A), CC.top_ps(COLUMNS), CC.floors(COLUMNS)


def _sequential(rows, k, p, tau):
    """top-p of the renormalised top-k (the convention the rule is NOT), then the floor"""
    first = CC.kept(rows, k, 1.0, 0.0)
    inner = CC.rows_of_mask(rows, first)
    out = np.zeros_like(first)
    for t in range(len(rows)):
        r = np.where(first[t], inner[t], -800.0)[None, :]
        out[t] = CC.kept(r, 0, p, tau)[0] & first[t]
    return out


def _one_short(rows, k, p, tau):
    """top-p that stops one bin before the mass is reached"""
    full = CC.kept(rows, k, p, tau)
    only_p = CC.kept(rows, 0, p, 0.0)
    out = full.copy()
    for t in range(len(rows)):
        if p < 1.0 and only_p[t].sum() > 1 and np.array_equal(full[t], only_p[t]):      # (top-p is the binding cut)
            last = np.where(only_p[t], rows[t], np.inf).argmin()
            out[t, last] = False
    return out


def _samplers(c):
    ks, ps, taus = _values()
    k, p, tau = ks[c], ps[c], taus[c]
    n = (c + 1) % COLUMNS
    A = _setup()[0].shape.A
    return {
        "the rule": lambda rT, r1, u: CC.pick_cut(rT, u, k, p, tau),
        "cuts ignored": lambda rT, r1, u: CC.pick_cut(rT, u, 0, 1.0, tau),
        "top-k keeps k + 1": lambda rT, r1, u: CC.pick_cut(rT, u, min(k + 1, A) if k else 0, p, tau),
        "top-p stops one bin short": lambda rT, r1, u: CC.pick(rT, u, _one_short(rT, k, p, tau)),
        "cuts on the untempered distribution": lambda rT, r1, u: CC.pick(rT, u, CC.kept(r1, k, p, 0.0) & MP.kept(rT, tau)),
        "sequential, not the intersection": lambda rT, r1, u: CC.pick(rT, u, _sequential(rT, k, p, tau)),
        "the neighbouring column's values": lambda rT, r1, u: CC.pick_cut(rT, u, ks[n], ps[n], taus[n]),
    }


def _columns(name):
    """the columns a sampler is run on: all of them for the rule; for a control those whose values give it something to get wrong"""
    ks, ps, taus = _values()
    A = _setup()[0].shape.A
    on = {"top-k keeps k + 1": lambda c: 0 < ks[c] < A, "top-p stops one bin short": lambda c: ps[c] < 1.0,
          "sequential, not the intersection": lambda c: 1 < ks[c] < A and ps[c] < 1.0,
          "cuts ignored": lambda c: 0 < ks[c] < A or ps[c] < 1.0}.get(name, lambda c: True)
    return [c for c in range(COLUMNS) if on(c)]


def _totals(name, T):
    """check_run's totals over the columns of _columns(name), each drawn by sampler `name` at temperature T and held to its own values"""
    from nv_wavenet_amd.slots import cut_rows
    key = (name, T)
    if key not in _runs:
        case, t, Lh, u = _setup()
        ks, ps, taus = _values()
        tot = np.zeros(3, dtype=np.int64)
        for c in _columns(name):
            y, rows, za_max = _free_run(c, T, _samplers(c)[name])
            dlt = CC.delta(T, za_max, float(np.abs(rows[np.isfinite(rows)]).max()), case.shape.A)
            assert 2e-6 < dlt < 2e-4, dlt
            tot += np.array(CC.check_column(rows, y, u[:, c], ks[c], ps[c], taus[c], dlt, cut_rows))
        _runs[key] = tuple(int(v) for v in tot)
    return _runs[key]


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_the_mirror_passes_the_checks_the_gpu_tests_use(T):
    tot = _totals("the rule", T)
    print("T = %g: violations %d, rows with more than one candidate %d of %d" % ((T,) + tot))
    assert CC.accepted(tot, 0.05), tot


@pytest.mark.parametrize("control,T", [("cuts ignored", 0.5), ("cuts ignored", 1.0), ("cuts ignored", 2.0),
                                       ("top-k keeps k + 1", 0.5), ("top-k keeps k + 1", 1.0), ("top-k keeps k + 1", 2.0),
                                       ("top-p stops one bin short", 0.5), ("top-p stops one bin short", 1.0), ("top-p stops one bin short", 2.0),
                                       ("cuts on the untempered distribution", 0.5), ("cuts on the untempered distribution", 2.0),
                                       ("sequential, not the intersection", 0.5), ("sequential, not the intersection", 1.0),
                                       ("sequential, not the intersection", 2.0),
                                       ("the neighbouring column's values", 0.5), ("the neighbouring column's values", 1.0),
                                       ("the neighbouring column's values", 2.0)])
def test_every_negative_control_is_rejected_by_the_same_checks(control, T):
    tot = _totals(control, T)
    print("%s, T = %g: violations %d, rows with more than one candidate %d of %d" % ((control, T) + tot))
    assert not CC.accepted(tot), (control, T, tot)
    assert tot[0] >= 3, "a control that differs in fewer than three samples has no power: %s" % (tot,)


def test_a_row_clear_of_every_boundary_has_one_candidate_and_near_ones_have_their_neighbours():
    rows = SC.log_softmax(np.array([[5.0, 4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0]]))
    assert len(CC.candidates(rows[0], 3, 1.0, 0.0, 1e-4)) == 1 and CC.candidates(rows[0], 3, 1.0, 0.0, 1e-4)[0].sum() == 3
    near = rows.copy()
    near[0, 3] = near[0, 2] - 5e-5                                         # the 3rd and the 4th within delta: either, or both (a tie)
    sets = {tuple(np.nonzero(m)[0]) for m in CC.candidates(near[0], 3, 1.0, 0.0, 1e-4)}
    assert sets == {(0, 1, 2), (0, 1, 3), (0, 1, 2, 3)}
    q = np.exp(rows[0])
    F = np.cumsum(q) / q.sum()
    sets = {tuple(np.nonzero(m)[0]) for m in CC.candidates(rows[0], 0, F[1] + 2e-5, 0.0, 1e-4)}      # a prefix mass within delta of p
    assert sets == {(0, 1), (0, 1, 2)}
    sets = {tuple(np.nonzero(m)[0]) for m in CC.candidates(rows[0], 0, 1.0, float(np.exp(-2.0)) * (1 + 3e-5), 1e-4)}      # a bin within delta of the floor
    assert sets == {(0, 1), (0, 1, 2)}


# ---- cut_rows ----------------------------------------------------------------------------------------------------------------------

def test_cut_rows_is_the_cut_renormalised_distribution_and_min_p_rows_agrees():
    from nv_wavenet_amd.slots import cut_rows, min_p_rows
    rng = np.random.default_rng(4)
    rows = SC.log_softmax(rng.standard_normal((7, 256)) * 2.5).astype(np.float32)
    for k, p, tau in ((0, 1.0, 0.0), (1, 1.0, 0.0), (4, 1.0, 0.0), (0, 0.5, 0.0), (0, 0.9, 0.0), (32, 0.8, 0.1), (256, 1.0, 0.0), (4, 0.9, 0.5)):
        out = cut_rows(rows, k, p, tau)
        assert out.dtype == np.float32 and out.shape == rows.shape
        keep = CC.kept(rows, k, p, tau)
        assert np.array_equal(np.isfinite(out), keep) and (out[~keep] == -np.inf).all()
        assert np.abs(np.exp(out.astype(np.float64)).sum(axis=1) - 1.0).max() <= 256 * 4 * SC.EPS32
        pr = np.exp(rows.astype(np.float64))
        ref = np.where(keep, pr, 0.0) / np.where(keep, pr, 0.0).sum(axis=1, keepdims=True)
        assert np.abs(np.exp(out.astype(np.float64)) - ref).max() <= 4 * SC.EPS32
        assert keep[np.arange(7), rows.argmax(axis=1)].all()                 # the most probable bin always stays
        if k:
            assert (keep.sum(axis=1) <= k).all() or k == 256
        if p < 1.0 and k == 0 and tau == 0.0:                                # the smallest set of most probable bins that reaches p
            mass = np.where(keep, pr, 0.0).sum(axis=1)
            smallest_kept = np.where(keep, pr, np.inf).min(axis=1)
            assert (mass >= p * pr.sum(axis=1) - 1e-12).all() and (mass - smallest_kept < p * pr.sum(axis=1)).all()
    assert (np.isfinite(cut_rows(rows, 1)).sum(axis=1) == 1).all() and np.array_equal(cut_rows(rows, 1).argmax(axis=1), rows.argmax(axis=1))
    assert np.array_equal(cut_rows(rows), min_p_rows(rows, 0.0)) and np.array_equal(cut_rows(rows, 256), cut_rows(rows))
    for tau in (0.05, 0.25, 0.5):
        assert np.array_equal(cut_rows(rows, min_p=tau), min_p_rows(rows, tau))
    # ties at the boundary all stay
    tied = np.log(np.array([[0.3, 0.2, 0.2, 0.2, 0.1]]))
    assert np.isfinite(cut_rows(tied, 2)).sum() == 4 and np.isfinite(cut_rows(tied, 0, 0.45)).sum() == 4 and np.isfinite(cut_rows(tied, 0, 0.29)).sum() == 1
    # the intersection, not the sequential convention: the top 4 of these hold 0.72 of the mass, and 0.8 of THAT is reached by three
    # bins; 0.8 of the whole mass needs five bins, so the intersection is the top 4
    inter = np.log(np.array([[0.25, 0.2, 0.15, 0.12, 0.1, 0.09, 0.09]]))
    assert np.isfinite(cut_rows(inter, 4, 0.8)).sum() == 4 and np.isfinite(cut_rows(inter, 0, 0.8)).sum() == 5
    per_row = cut_rows(rows, [0, 1, 4, 32, 256, 0, 4], [1.0, 0.5, 0.8, 0.9, 1.0, 0.5, 0.8], [0.0, 0.05, 0.1, 0.25, 0.5, 0.0, 0.5])
    assert np.array_equal(per_row[2], cut_rows(rows, 4, 0.8, 0.1)[2]) and np.array_equal(per_row[0], cut_rows(rows)[0])
    one = cut_rows(rows[3], 4, 0.9)
    assert one.shape == (256,) and np.array_equal(one, cut_rows(rows, 4, 0.9)[3])
    tt = cut_rows(torch.from_numpy(rows), 4, 0.9)
    assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), cut_rows(rows, 4, 0.9))
    for bad in (dict(top_k=-1), dict(top_k=257), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
                dict(min_p=0.6), dict(top_k=[1, 2])):
        with pytest.raises(ValueError):
            cut_rows(rows, **bad)


# ---- SlotState ---------------------------------------------------------------------------------------------------------------------

def _cut_blob(k, p, done=13, uid=4):
    blob = _synthetic_blob(5, 8, done, uid)
    blob.numpy().view("<u4")[K_WORD] = k
    blob.numpy().view("<u4")[P_WORD] = CC.p_bits(p)
    return blob


def test_the_cuts_survive_to_bytes_and_from_bytes():
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    R = SlotState.RECORD_BYTES
    blob = _synthetic_blob(5, 8, 13, 4)
    s0 = SlotState(blob, src, 4, 13, "features")
    assert (s0.top_k, s0.top_p) == (0, 1.0) and s0.to_bytes()[R:] == blob.numpy().tobytes()      # no cut: the bytes they were
    back = SlotState.from_bytes(s0.to_bytes(), src)
    assert (back.top_k, back.top_p) == (0, 1.0)
    for k, p in ((1, 1.0), (0, 0.5), (32, 0.9), (256, 0.8)):
        p = float(np.float32(p))
        blob = _cut_blob(k, p)
        data = SlotState(blob, src, 4, 13, "mel", 9, False, top_k=k, top_p=p).to_bytes()
        assert data[R:] == blob.numpy().tobytes()
        back = SlotState.from_bytes(data, src)
        assert (back.top_k, back.top_p, back.min_p, back.temperature, back.kind, back.done) == (k, p, 0.0, 1.0, "mel", 13)
        assert back._blob_sampling[2:] == (k, p) and back.to_bytes() == data
    # a prefilled or scored state: the blob's words are zero, the state's cuts are not -- the bytes carry them
    st = SlotState(_synthetic_blob(5, 8, 13, 4), src, 4, 13, "features")
    st.top_k, st.top_p = 4, 0.5
    assert st._blob_sampling[2:] == (0, 1.0)
    words = np.frombuffer(st.to_bytes(), dtype="<u4", count=16, offset=R)
    assert (words[K_WORD], words[P_WORD], words[11]) == (4, CC.p_bits(0.5), 0)
    back = SlotState.from_bytes(st.to_bytes(), src)
    assert (back.top_k, back.top_p) == (4, 0.5) and back._blob_sampling[2:] == (4, 0.5)
    # a request that had not started: the record alone without a cut (as before), the record and a bare header otherwise
    assert len(SlotState(None, src, 3, 0, "features").to_bytes()) == R
    data = SlotState(None, src, 3, 0, "features", top_k=7).to_bytes()
    assert len(data) == R + HEADER_BYTES
    words = np.frombuffer(data, dtype="<u4", count=16, offset=R)
    assert (words[K_WORD], words[P_WORD], words[10], words[11]) == (7, 0, 0, 0)
    back = SlotState.from_bytes(data, src)
    assert back.blob is None and (back.top_k, back.top_p) == (7, 1.0) and back.to_bytes() == data
    both = SlotState.from_bytes(SlotState(None, src, 3, 0, "mel", 2, False, temperature=0.5, min_p=0.25, top_k=3, top_p=0.9).to_bytes(), src)
    assert (both.blob, both.min_p, both.temperature, both.top_k, both.top_p) == (None, 0.25, 0.5, 3, float(np.float32(0.9)))


@pytest.mark.parametrize("word,value", [(K_WORD, 0x80000000), (K_WORD, 0xFFFFFFFF), (P_WORD, _bits(1.0)), (P_WORD, _bits(1.5)),
                                        (P_WORD, _bits(-0.5)), (P_WORD, _bits(float("nan"))), (P_WORD, _bits(float("inf"))),
                                        (P_WORD, 0x80000000)])
def test_from_bytes_refuses_a_bad_cut_word(word, value):
    from nv_wavenet_amd.slots import SlotState
    src = torch.zeros(80, 40)
    blob = _synthetic_blob(5, 8, 9, 2)
    blob.numpy().view("<u4")[word] = value
    data = SlotState.RECORD.pack(b"NWSS", 1, 0, 0, 0, 2, 9, blob.numel()) + blob.numpy().tobytes()
    with pytest.raises(ValueError):
        SlotState.from_bytes(data, src)


# ---- SlotStream against a stub engine ----------------------------------------------------------------------------------------------

class CutFakeEngine(MinPFakeEngine):
    """MinPFakeEngine with the cuts by the engine's rules: per column, off after a start, the blob's after a resume, carried by a
    move; the setters need an utterance (or a pending start or resume) in the column.  Blobs are ("blob", uid, done, T, p, (k, q)).
    cuts_at_step[i]: {uid: (k, q)} in force for step i."""
    A = 256

    def __init__(self, columns, window=64):
        super().__init__(columns, window)
        self.cut = {}
        self.cuts_at_step = []

    def slotStart(self, col, x, uid, length=None):
        super().slotStart(col, x, uid, length)
        self.cut[col] = (0, 1.0)

    def slotStartMel(self, col, mel, uid, frames=None, final=True):
        super().slotStartMel(col, mel, uid, frames, final)
        self.cut[col] = (0, 1.0)

    def slotResume(self, col, blob, x, length=None):
        super().slotResume(col, blob, x, length)
        self.cut[col] = blob[5]

    def slotResumeMel(self, col, blob, mel, frames=None, final=True):
        super().slotResumeMel(col, blob, mel, frames, final)
        self.cut[col] = blob[5]

    def slotStop(self, col):
        super().slotStop(col)
        self.cut.pop(col)

    def slotMove(self, src, dst):
        super().slotMove(src, dst)
        self.cut[dst] = self.cut.pop(src)

    def slotSave(self, col, stream=None):
        blob, done = super().slotSave(col, stream)
        return blob + (self.cut[col],), done

    def slotSetTopK(self, col, k):
        assert col in self.active, "a cut for a column without an utterance"
        assert 0 <= k <= self.A
        self.calls.append(("top_k", col, k))
        self.cut[col] = (k, self.cut[col][1])

    def slotSetTopP(self, col, p):
        assert col in self.active, "a cut for a column without an utterance"
        assert 0.0 < p <= 1.0
        self.calls.append(("top_p", col, p))
        self.cut[col] = (self.cut[col][0], p)

    def slotsStep(self, count, y, pcm):
        self.cuts_at_step.append({self.active[c][0]: self.cut[c] for c in self.active})
        return super().slotsStep(count, y, pcm)


@pytest.mark.parametrize("bad", [dict(top_k=-1), dict(top_k=257), dict(top_k=2.5), dict(top_k="many"), dict(top_k=None)] +
                         [dict(top_p=p) for p in CC.BAD_TOP_PS] + [dict(top_p="most"), dict(top_p=None)])
def test_bad_cuts_raise_everywhere_and_change_nothing(bad):
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = CutFakeEngine(4)
    st = SlotStream(eng, 64)
    x = torch.zeros(80, 30)
    with pytest.raises(ValueError):
        st.submit(x, **bad)
    with pytest.raises(ValueError):
        st.submit_mel(torch.zeros(80, 5), **bad)
    assert not st.busy() and st._next_handle == 0
    h = st.submit(x, top_k=4, top_p=0.5)
    setter = st.set_top_k if "top_k" in bad else st.set_top_p
    with pytest.raises(ValueError):
        setter(h, list(bad.values())[0])             # waiting
    st.step(4)
    with pytest.raises(ValueError):
        setter(h, list(bad.values())[0])             # running
    assert (st.top_k(h), st.top_p(h)) == (4, 0.5) and eng.cut[0] == (4, 0.5)
    assert [c for c in eng.calls if c[0] in ("top_k", "top_p")] == [("top_k", 0, 4), ("top_p", 0, 0.5)]
    if bad != dict(top_k=257):                      # (a state does not know the alphabet: the engine refuses such a k at the resume)
        with pytest.raises(ValueError):
            SlotState(None, x, 0, 0, "features", **bad)
    for call in (lambda: st.set_top_k(99, 1), lambda: st.set_top_p(99, 0.5), lambda: st.top_k(99), lambda: st.top_p(99)):
        with pytest.raises(KeyError):
            call()
    st.close()


def test_submit_with_cuts_sets_them_after_the_start_and_before_the_step():
    from nv_wavenet_amd.slots import SlotStream
    eng = CutFakeEngine(3)
    st = SlotStream(eng, 64)
    a = st.submit(torch.zeros(80, 12), top_k=1)
    b = st.submit(torch.zeros(80, 12))                                   # no cut: no call at all
    c = st.submit_mel(torch.zeros(80, 3), temperature=2.0, min_p=0.25, top_k=32, top_p=0.9)
    d = st.submit(torch.zeros(80, 8), top_p=0.5)                         # waits for a column
    st.step(4)
    p9 = float(np.float32(0.9))
    assert _kinds(eng) == ["begin", "start", "start", "start_mel", "temperature", "min_p", "top_k", "top_k", "top_p", "step"]
    assert [x for x in eng.calls if x[0] in ("top_k", "top_p")] == [("top_k", 0, 1), ("top_k", 2, 32), ("top_p", 2, p9)]
    assert eng.cuts_at_step[0] == {0: (1, 1.0), 1: (0, 1.0), 2: (32, p9)} and eng.floors_at_step[0] == {0: 0.0, 1: 0.0, 2: 0.25}
    assert [(st.top_k(h), st.top_p(h)) for h in (a, b, c, d)] == [(1, 1.0), (0, 1.0), (32, p9), (0, 0.5)]
    st.set_top_p(b, 0.8)                                                 # running: at once, in force from the next step
    assert eng.calls[-1] == ("top_p", 1, float(np.float32(0.8)))
    st.set_top_k(a, 0)                                                   # ... and back to off
    st.step(4)
    assert eng.cuts_at_step[1] == {0: (0, 1.0), 1: (0, float(np.float32(0.8))), 2: (32, p9)}
    st.set_top_k(d, 4)                                                   # waiting: when it is admitted, after its start
    assert eng.calls[-1][0] == "step"
    st.step(4)
    before = len(eng.calls)
    st.step(4)
    assert _kinds(eng, before)[-4:] == ["start", "top_k", "top_p", "step"] and eng.cuts_at_step[3] == {3: (4, 0.5)}
    while st.busy():
        st.step(4)
    assert st._sampling == {}                                                 # nothing is kept of a finished request
    st.close()


def test_resume_refuses_a_top_k_beyond_the_engines_alphabet_before_anything_is_queued():
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = CutFakeEngine(2)
    st = SlotStream(eng, 64)
    state = SlotState(None, torch.zeros(80, 12), 5, 0, "features", top_k=CutFakeEngine.A + 1)      # (a state does not know the alphabet)
    with pytest.raises(ValueError):
        st.resume(state)
    assert not st.busy() and st._next_handle == 0 and st._sampling == {} and _kinds(eng) == ["begin"]
    state.top_k = CutFakeEngine.A
    h = st.resume(state)
    st.step(4)
    assert st.top_k(h) == CutFakeEngine.A and eng.cuts_at_step[0] == {5: (CutFakeEngine.A, 1.0)}
    st.close()


def test_compact_suspend_and_resume_keep_the_cuts():
    from nv_wavenet_amd.slots import SlotState, SlotStream
    eng = CutFakeEngine(40)
    st = SlotStream(eng, 64)
    cuts = {38: dict(top_k=4), 39: dict(top_k=32, top_p=0.5)}
    hs = [st.submit(torch.zeros(80, 4 if i < 38 else 40), **cuts.get(i, {})) for i in range(40)]
    st.step(4)
    assert st.compact() == 2                                             # 39 -> 0, 38 -> 1: the engine's move carries the values
    n_set = len([c for c in eng.calls if c[0] in ("top_k", "top_p")])
    st.step(4)
    assert eng.cuts_at_step[-1] == {39: (32, 0.5), 38: (4, 1.0)} and (eng.cut[0], eng.cut[1]) == ((32, 0.5), (4, 1.0))
    assert len([c for c in eng.calls if c[0] in ("top_k", "top_p")]) == n_set, "a move needs no new call"
    # suspend: the state carries them; resume in another stream: the engine takes them from the blob, no call
    state = st.suspend(hs[39])
    assert (state.top_k, state.top_p) == (32, 0.5) and state.blob[5] == (32, 0.5) and state.done == 8
    other_eng = CutFakeEngine(2)
    other = SlotStream(other_eng, 64)
    h2 = other.resume(state)
    assert (other.top_k(h2), other.top_p(h2)) == (32, 0.5)
    other.step(4)
    assert other_eng.cuts_at_step[0] == {39: (32, 0.5)} and "top_k" not in _kinds(other_eng) and "top_p" not in _kinds(other_eng)
    # ... unless one was changed on the state: resume, then set that one
    state = other.suspend(h2)
    state.top_p = 0.9
    h3 = other.resume(state)
    other.step(4)
    assert _kinds(other_eng)[-3:] == ["resume", "top_p", "step"] and other_eng.cuts_at_step[-1] == {39: (32, float(np.float32(0.9)))}
    # a request suspended before it started keeps them too (through bytes as well)
    w3 = other.submit(torch.zeros(80, 6), top_k=1, top_p=0.8)
    waiting = other.suspend(w3)
    assert waiting.blob is None and (waiting.top_k, waiting.top_p) == (1, float(np.float32(0.8)))
    again = SlotState.from_bytes(waiting.to_bytes(), waiting.source)
    assert again.blob is None and (again.top_k, again.top_p) == (waiting.top_k, waiting.top_p)
    h4 = st.resume(again)
    st.step(4)
    assert eng.cuts_at_step[-1][again.uid] == (1, float(np.float32(0.8))) and st.top_k(h4) == 1
    assert other.suspend(h3).top_p == float(np.float32(0.9)) and other._sampling == {}
    other.close()
    st.close()


def test_an_admission_sets_the_values_in_one_order_and_a_resume_only_those_that_differ_from_the_blob():
    """Two requests that differ from what their start leaves in all four values, one of them primed, admitted by one step: the whole
    call list -- the starts, every temperature, every floor, then top-k and top-p column by column, then the prime.  A suspended one
    resumed elsewhere takes its values from the blob: only those changed on the state since are set again."""
    from nv_wavenet_amd.slots import SlotStream

    class PrimedCutFakeEngine(CutFakeEngine):
        def slotPrime(self, col, y):
            assert col in self.pending, "prime without a pending start or resume"
            self.calls.append(("prime", col, y.numel()))

    eng = PrimedCutFakeEngine(4)
    st = SlotStream(eng, 64)
    p9, p8 = float(np.float32(0.9)), float(np.float32(0.8))
    a = st.submit(torch.zeros(80, 40), temperature=0.5, min_p=0.25, top_k=32, top_p=0.9, prime=torch.tensor([3, 1, 2]))
    st.submit_mel(torch.zeros(80, 10), temperature=2.0, min_p=0.125, top_k=4, top_p=0.8)
    st.step(4)
    assert eng.calls == [("begin", 64), ("start", 0, 0), ("start_mel", 1, 1, 10, True),
                         ("temperature", 0, 0.5), ("temperature", 1, 2.0), ("min_p", 0, 0.25), ("min_p", 1, 0.125),
                         ("top_k", 0, 32), ("top_p", 0, p9), ("top_k", 1, 4), ("top_p", 1, p8), ("prime", 0, 3), ("step", 4, 1)]
    state = st.suspend(a)
    assert eng.calls[-2:] == [("save", 0, 4), ("stop", 0)] and state.blob == ("blob", 0, 4, 0.5, 0.25, (32, p9))
    other_eng = PrimedCutFakeEngine(2)
    other = SlotStream(other_eng, 64)
    h = other.resume(state)                                              # as saved: the engine reads all four from the blob
    other.step(4)
    assert other_eng.calls == [("begin", 64), ("resume", 0, 0, 4), ("step", 4, 1)]
    state = other.suspend(h)
    state.min_p, state.top_k = 0.5, 1                                    # two of the four changed on the state
    h = other.resume(state)
    other.step(4)
    assert other_eng.calls[3:] == [("save", 0, 8), ("stop", 0), ("resume", 0, 0, 8), ("min_p", 0, 0.5), ("top_k", 0, 1), ("step", 4, 1)]
    assert (other.temperature(h), other.min_p(h), other.top_k(h), other.top_p(h)) == (0.5, 0.5, 1, p9)
    assert (other_eng.temp[0], other_eng.minp[0], other_eng.cut[0]) == (0.5, 0.5, (1, p9))
    other.close()
    st.close()
