"""softmax_pick's floored and cutting forms, cut_threshold and cut_threshold_dump in isolation (GPU), through the test-only entries
wnp_softmax_pick_form and wnp_cut_threshold of tests/cpp/wn_primitives.hip (one workgroup, 16 utterances, every argument per
utterance), on the crafted and the random rows of tests/sampler_cases.py, at every softmax lane layout a generation kernel has and
at the selectors 0, 2^-24, 0.37, 1 - 2^-22, 1 - 2^-23 and 1 - 2^-24:

  * the forms agree with the plain form, bit for bit, when nothing is in force, and the two cutting forms with each other always;
  * both searches return the threshold of the definition (cut_cases.sorted_threshold on the plain form's e), the cut e is the plain
    e floored at it, and total and pick are those of the scan's float32 mirror (sampler_cases.scan_pick) -- all exactly;
  * on the crafted rows, none left out, the kept set is the one a sort in float64 gives, e / total the renormalised float64
    distribution and the pick its inverse-CDF pick;
  * the pick is a kept bin, for every row, form and selector.

tests/test_sampler_primitives_cpu.py shows that the crafted rows are clear of rounding and that each of six wrong rules would fail
these equalities."""
import ctypes as C
import os

import numpy as np
import pytest

import cut_cases as CC
import sampler_cases as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
MID = tuple(0.05 + 0.057 * u for u in range(16))          # one more launch, a selector per utterance, for the float64 pick


@pytest.fixture(scope="module")
def prim():
    import torch  # noqa: F401  (one HIP runtime per process: torch's, see nv_wavenet_amd/_lib.py)
    path = os.path.join(HERE, "cpp", "libwn_primitives.so")
    assert os.path.exists(path), "build it with python -c 'import __graft_entry__ as g; g.build()'"
    return bind(C.CDLL(path))


def bind(lib):
    lib.wnp_softmax_pick_form.argtypes = [C.c_int] * 3 + [_fp] * 4 + [_ip, _fp, _ip, _fp, _fp]
    lib.wnp_cut_threshold.argtypes = [C.c_int] * 3 + [_fp, _fp, _ip, _fp, _fp]
    return lib


def _f(a):
    assert a.dtype == F32 and a.flags.c_contiguous
    return a.ctypes.data_as(_fp)


def _i(a):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(_ip)


def run_form(lib, A, nw, form, logits, sel, T, tau, k, p):
    """(pick [16], e [16][A], total [16]) of softmax_pick's form `form` on 16 utterances"""
    sel = np.ascontiguousarray(np.broadcast_to(np.asarray(sel, dtype=F32), (16,)))
    picks, e, total = np.full(16, -7, dtype=np.int32), np.full((16, A), np.nan, dtype=F32), np.full(16, np.nan, dtype=F32)
    k = np.ascontiguousarray(k, dtype=np.int32)
    args = [np.ascontiguousarray(a, dtype=F32) for a in (logits, sel, S.scale_of(T), tau)]
    assert args[0].shape == (16, A) and all(a.shape == (16,) for a in args[1:]) and k.shape == (16,)
    p = np.ascontiguousarray(p, dtype=F32)
    assert lib.wnp_softmax_pick_form(A, nw, form, *[_f(a) for a in args], _i(k), _f(p), _i(picks), _f(e), _f(total)) == 0
    return picks.astype(np.int64), e, total


def run_threshold(lib, A, nw, dump, logits, T, k, p):
    thr = np.full(16, np.nan, dtype=F32)
    logits, p, k = np.ascontiguousarray(logits, dtype=F32), np.ascontiguousarray(p, dtype=F32), np.ascontiguousarray(k, dtype=np.int32)
    assert lib.wnp_cut_threshold(A, nw, dump, _f(logits), _f(S.scale_of(T)), _i(k), _f(p), _f(thr)) == 0
    return thr


_runs = {}


def _device(lib, A, nw):
    """Everything the device computes for one lane layout, once: per launch of 16 rows (the crafted ones first) the plain form, the
    three other forms with the rows' settings (form 1: the floor alone) and with everything off, at every selector, and the two
    searches; beside it the mirrors' threshold and cut e of every row."""
    if (A, nw) not in _runs:
        LPU = 4 * nw
        rows = S.crafted(A, LPU)
        n_crafted = len(rows) // 16
        out = []
        for li, (logits, k, p, tau, T, group) in enumerate(S.launches(rows + S.random_rows(A))):
            off_k = np.where(np.arange(16) % 2, A, 0).astype(np.int32)
            zero, one = np.zeros(16, dtype=F32), np.ones(16, dtype=F32)
            d = dict(rows=group, crafted=li < n_crafted, k=k, p=p, tau=tau, T=T, logits=logits, plain={}, form={1: {}, 2: {}, 3: {}},
                     off={1: {}, 2: {}, 3: {}})
            for sel in S.SELECTORS + (1.5,) + ((MID,) if d["crafted"] else ()):
                d["plain"][sel] = run_form(lib, A, nw, 0, logits, sel, T, zero, off_k, one)
                for form in (1, 2, 3):
                    d["form"][form][sel] = run_form(lib, A, nw, form, logits, sel, T, tau, k, p)
                    if sel in S.SELECTORS:
                        d["off"][form][sel] = run_form(lib, A, nw, form, logits, sel, T, zero, off_k, one)
            d["thr"] = [run_threshold(lib, A, nw, dump, logits, T, k, p) for dump in (0, 1)]
            e0 = d["plain"][0.0][1]
            d["e0"] = e0
            d["want_thr"] = np.array([CC.sorted_threshold(e0[u], int(k[u]), float(p[u]), LPU) for u in range(16)], dtype=F32)
            d["want_e"] = {1: np.where(e0 >= tau[:, None], e0, F32(0)),
                           2: np.where(e0 >= np.maximum(d["want_thr"], tau)[:, None], e0, F32(0))}
            d["want_e"][3] = d["want_e"][2]
            out.append(d)
        _runs[(A, nw)] = out
    return _runs[(A, nw)]


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("A,nw", S.PAIRS)
def test_the_forms_agree_when_nothing_is_in_force_and_the_cutting_forms_always(prim, A, nw):
    """Form 1 at floor 0 and forms 2 and 3 at k of 0 and A, p = 1 and floor 0 hand back the plain form's e and total bit for bit, and
    its pick -- but where the plain form's scan falls off the end (its 128) or stops on a bin whose e is 0: there these forms
    answer the kept bin below, which the mirror-equality test holds them to.  Forms 2 and 3 agree bit for bit at every setting."""
    LPU = 4 * nw
    apart = 0
    for d in _device(prim, A, nw):
        for sel in S.SELECTORS:
            pick0, e0, total0 = d["plain"][sel]
            assert _same(e0, d["e0"])
            stray = S.falls_off(e0, sel, LPU) | S.stops_on_a_dropped_bin(e0, sel, LPU)
            for form in (1, 2, 3):
                pick, e, total = d["off"][form][sel]
                assert _same(e, e0) and _same(total, total0), (form, sel)
                assert np.array_equal(pick[~stray], pick0[~stray]), (form, sel, pick, pick0)
                assert (e0[np.arange(16), pick] > 0).all(), (form, sel)
                apart += int((pick != pick0).sum())
        for sel in d["form"][2]:
            (pick2, e2, total2), (pick3, e3, total3) = d["form"][2][sel], d["form"][3][sel]
            assert np.array_equal(pick2, pick3) and _same(e2, e3) and _same(total2, total3), sel
    print("A %d nw %d: with everything off, %d picks differ from the plain form's (its scan fell off or stopped on e = 0)" % (A, nw, apart))


@pytest.mark.parametrize("A,nw", S.PAIRS)
def test_the_threshold_is_the_definition_and_the_scan_is_its_mirror(prim, A, nw):
    """Exact: both searches against cut_cases.sorted_threshold on the plain form's e; the cut e against the plain e floored at
    max(threshold, floor); total and pick of every form against sampler_cases.scan_pick on the e the form handed back."""
    LPU = 4 * nw
    for d in _device(prim, A, nw):
        names = [r.name for r in d["rows"]]
        for dump in (0, 1):
            bad = np.nonzero(d["thr"][dump].view(np.uint32) != d["want_thr"].view(np.uint32))[0]
            assert not len(bad), (dump, [(names[u], d["thr"][dump][u], d["want_thr"][u]) for u in bad[:3]])
        for form in (0, 1, 2, 3):
            for sel, (pick, e, total) in (d["form"][form] if form else d["plain"]).items():
                if form:
                    bad = np.nonzero((e.view(np.uint32) != d["want_e"][form].view(np.uint32)).any(axis=1))[0]
                    assert not len(bad), (form, sel, [names[u] for u in bad[:3]])
                want_pick, want_total = S.scan_pick(e, sel, LPU, floored=form >= 1)
                assert _same(total, want_total), (form, sel, total, want_total)
                bad = np.nonzero(pick != want_pick)[0]
                assert not len(bad), (form, sel, [(names[u], int(pick[u]), int(want_pick[u])) for u in bad[:3]])


def _float64_pick(q, sel):
    """the rule of test_primitives_gpu._expected_pick on an un-normalised distribution q: (index, within 1e-6 of a CDF edge)"""
    c = np.cumsum(q) / q.sum()
    return int(np.searchsorted(c, sel, side="right")), bool(np.abs(c - sel).min() < 1e-6)


@pytest.mark.parametrize("A,nw", S.PAIRS)
def test_the_crafted_rows_against_a_sort_in_float64(prim, A, nw):
    """Independent of the mirrors, on every crafted row: the kept set is the one sampler_cases.kept64 finds by sorting in float64
    (over the bins whose e is not 0 in float32 already: those have less than 2^-126 of the maximum's mass and nothing to keep);
    e / total is within 4 A eps32 of the float64 distribution renormalised over the kept set; the pick is that distribution's
    inverse-CDF pick wherever the selector is further than 1e-6 from an edge of its CDF."""
    checked = 0
    for d in _device(prim, A, nw):
        if not d["crafted"]:
            continue
        for u, r in enumerate(d["rows"]):
            x = r.logits.astype(np.float64) / r.T
            q = np.exp(x - x.max())
            assert (q[d["e0"][u] == 0] < 2.0 ** -126).all() and (d["e0"][u][q >= 2.0 ** -120] > 0).all(), r.name
            for form in (1, 2, 3):
                k, p = (r.k, r.p) if form >= 2 else (0, 1.0)
                keep = S.kept64(r.logits, k, p, r.tau, r.T) & (d["e0"][u] > 0)
                if form >= 2:
                    assert np.array_equal(np.nonzero(keep)[0], r.keep), r.name
                qk = np.where(keep, q, 0.0)
                for sel, (pick, e, total) in d["form"][form].items():
                    assert np.array_equal(e[u] > 0, keep), (r.name, form, np.nonzero((e[u] > 0) != keep)[0][:5])
                    err = np.abs(e[u].astype(np.float64) / np.float64(total[u]) - qk / qk.sum()).max()
                    assert err <= 4 * A * CC.EPS32, (r.name, form, err)
                    s = float(F32(MID[u] if sel is MID else sel))
                    idx, near = _float64_pick(qk, s)
                    if not near and s < 1.0:
                        assert int(pick[u]) == idx, (r.name, form, s, int(pick[u]), idx)
                        checked += 1
    assert checked >= 3 * 32                               # (0.37 and the launch of its own: about two per row and form)
    print("A %d nw %d: %d picks held to the float64 inverse CDF" % (A, nw, checked))


@pytest.mark.parametrize("A,nw", S.PAIRS)
def test_the_pick_is_a_kept_bin(prim, A, nw):
    """Every crafted and random row, every form with something in force, every selector of the sweep: e[pick] > 0.  A selector
    beyond the total makes every scan fall off: the plain form keeps its documented 128, the others answer the last kept bin."""
    draws = outside = 0
    for d in _device(prim, A, nw):
        for form in (1, 2, 3):
            on = np.array([S.in_force(r, form, A) for r in d["rows"]])
            for sel in S.SELECTORS:
                pick, e, _ = d["form"][form][sel]
                assert ((0 <= pick) & (pick < A)).all(), (form, sel, pick)
                miss = on & ~(e[np.arange(16), pick] > 0)
                draws += int(on.sum())
                outside += int(miss.sum())
                assert not miss.any(), (form, sel, [(d["rows"][u].name, int(pick[u])) for u in np.nonzero(miss)[0][:3]])
            pick, e, _ = d["form"][form][1.5]
            assert np.array_equal(pick, A - 1 - np.argmax((e > 0)[:, ::-1], axis=1)), form
        assert (d["plain"][1.5][0] == 128).all()
    print("A %d nw %d: %d draws under a floor or a cut, %d outside the kept set" % (A, nw, draws, outside))
