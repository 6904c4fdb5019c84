"""GPU tests of the layer / dilation schedule at its edges (`-m gpu`; the schedules and why: tests/schedule_edges.py): two layers,
maxDilation 1, a maxDilation that is no power of two or is never reached, a dilation beyond what the ring in LDS takes, and as many
layers as the library accepts.  The schedule is restated in the host's fillSchedule / placeLdsRing / ring size, the kernel's
travelling entries (dil_next), the chain's own entries and slot mode's largest dilation, rotation and blob order: every one of them
is held here to the CPU oracle (fp32: exact samples; fp16: util.fp16_bars) or, bit for bit, to a run that is.
tests/test_schedule_edges_cpu.py shows on the oracle alone that these inputs tell the schedules apart."""
import numpy as np
import pytest
import torch

import schedule_edges as E
import test_parity_gpu as P
import test_slots_gpu as TS
import util
from nv_wavenet_amd._lib import lib
from oracle import oracle as O
from test_slots_state_cpu import HEADER_BYTES
from test_slots_state_gpu import Run

pytestmark = pytest.mark.gpu

WG_MODES = ("wg", "wg2", "wg3", "wg4")           # organisations of wn::wavenet_wg: none of them may refuse a schedule here
_lmax = {}


def lmax(precision):
    """The most layers nvw_create_ex accepts at R32 in organisation "wg": kMaxLayers = 128 if that is accepted, else found by
    bisecting the create call (a refusal is a NULL and a message: the bias table of the model lives in LDS)."""
    if precision not in _lmax:
        def ok(L):
            h = lib.nvw_create_ex(32, 128, 256, precision, L, 2, 5, 24, 1, 1, util.MODE_ORG["wg"])
            if h:
                lib.nvw_destroy(h)
            return bool(h)
        lo, hi = 2, E.L_MAX + 1                   # accepted, refused (kMaxLayers + 1: test_schedule_edges_cpu)
        if ok(E.L_MAX):
            lo = E.L_MAX
        else:
            assert ok(lo)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        _lmax[precision] = lo
        print("EDGE Lmax fp%d = %d" % (precision, lo))
    return _lmax[precision]


def _case(run, precision):
    shape, L, maxD = run
    return E.case_of(shape, L, maxD, lmax(precision) if L == "Lmax" else None)


def _create(case, t, precision, mode):
    """The engine in organisation `mode`, or None when nvw_create_ex refuses it (a chain organisation only: recorded in the output)."""
    try:
        e = P._engine_o1(case, t, precision, mode)
    except RuntimeError:
        assert mode not in WG_MODES, "wavenet_wg organisation %s refused %s" % (mode, case.name)
        print("EDGE refused %s fp%d %s: nvw_create_ex returned NULL" % (case.name, precision, mode))
        return None
    info = e.kernelInfo(case.shape.B, True)
    print("EDGE launches %s fp%d %s: %s" % (case.name, precision, mode, info))
    if mode in WG_MODES:
        assert "wavenet_wg<" in info, info
    return e


def _chain_clean(e):
    if "wavenet_chain<" in e.kernelInfo():
        assert e.chainStatus() == 0 and e.chainFallbacks() == 0


def _fp32_bars(ref, got, sel_bn, B):
    """The caps of test_fp32_engine_o1_exact_samples_and_reference_bars."""
    diverged, unexplained = util.explain_mismatches(ref["y"], got["y"], ref["lo"], ref["hi"], sel_bn, 1e-5)
    assert not unexplained, "unexplained sample mismatches (b,t,ref,got,edge distance): %s" % unexplained[:5]
    assert diverged <= max(1, B // 8), "%d utterances diverged" % diverged
    util.compare_activations(ref, got, atol_eps=32)


def _free_run(e, case, chunk=None):
    s = case.shape
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    if chunk:
        assert e.run_chunks(chunk, None, s.N, s.B, y, 1)
    else:
        assert e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    return y


def test_the_most_layers_the_library_accepts():
    """Lmax per precision (printed; LABNOTES.md has the values of one MI355X): accepted, and -- below kMaxLayers -- one more refused
    with a NULL."""
    for precision in (32, 16):
        L = lmax(precision)
        assert 2 <= L <= E.L_MAX
        h = lib.nvw_create_ex(32, 128, 256, precision, L + 1, 2, 5, 24, 1, 1, util.MODE_ORG["wg"])
        assert not h, "fp%d: %d layers accepted beyond Lmax = %d" % (precision, L + 1, L)


# ---- a, c: fp32 against the oracle -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["wg", "wg2", "chain"])
@pytest.mark.parametrize("run", E.RUNS, ids=E.run_id)
def test_fp32_exact_samples_at_the_edge_schedules(run, mode):
    """Exact sample indices (a divergence only within 1e-5 of a CDF edge, at most max(1, B // 8) utterances), last-sample
    activations within the reference harness's bars."""
    case = _case(run, 32)
    t = util.gen_o1(case, half=False)
    e = _create(case, t, 32, mode)
    if e is None:
        return
    got = P._run_dumped(e, case)
    ref = P._teacher_forced_ref(case, t, got["y"])
    _fp32_bars(ref, got, t.sel.T, case.shape.B)
    _chain_clean(e)
    e.close()


# ---- b, c: fp16 against the oracle -------------------------------------------------------------------------------------------------

_fp16_y = {}


def _fp16_modes():
    return [(run, mode) for run in E.RUNS for mode in ("wg", "wg2", "wg3", "chain") + (("wg4",) if run[0] == "R64" else ())]


@pytest.mark.parametrize("run,mode", _fp16_modes(), ids=lambda v: E.run_id(v) if isinstance(v, tuple) else v)
def test_fp16_bars_at_the_edge_schedules(run, mode):
    """util.fp16_bars (FP16_K = 8 units of 2^-11 max|tensor|, >= 98 % of the picks the oracle's) against the teacher-forced fp32
    oracle fed the fp16-rounded parameters; the dump-free kernel and every organisation generate the same samples, bit for bit."""
    case = _case(run, 16)
    s = case.shape
    t = util.gen_o1(case, half=True)
    e = _create(case, t, 16, mode)
    if e is None:
        return
    got = P._run_dumped(e, case)
    ref = P._teacher_forced_ref(case, t, got["y"])
    st = util.fp16_bars(ref, got, t.sel.T, "%s/%s" % (case.name, mode))
    worst = max(st[k] for k in ("Xout_units", "skipOut_units", "Zs_units", "Za_units")) / util.FP16_K
    print("EDGE fp16 %s %s: worst activation error %.3f of the bar, agreement %.4f (%d misses)" % (case.name, mode, worst, st["agreement"], st["misses"]))
    e.setInputs(t.Lh, t.sel)
    print("EDGE launches %s fp16 %s (no dump): %s" % (case.name, mode, e.kernelInfo(s.B, False)))
    y2 = _free_run(e, case)
    assert np.array_equal(y2, got["y"]), "dump and no-dump kernel variants disagree"
    _chain_clean(e)
    e.close()
    first_mode, first = _fp16_y.setdefault(run, (mode, got["y"]))
    assert np.array_equal(first, got["y"]), "%s and %s disagree in fp16" % (first_mode, mode)


# ---- d: the ring in LDS --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [(16, "wg"), (16, "wg2"), (16, "wg3"), (32, "wg")])
@pytest.mark.parametrize("run", E.RUNS, ids=E.run_id)
def test_ring_in_lds_at_the_edge_schedules(run, precision, mode):
    """setRingInLds(0) (as many short-dilation layers' slots in LDS as fit) against setRingInLds(-1) (none): the same samples, whole, in
    chunks of 1 and of 7 (the state crosses launches through the HBM ring), and with the mode switched at N // 2 in both
    directions.  (20, 1): twenty one-slot layers against the three in-place slots -- whether they are held or not (printed) the
    samples agree; (11, 1024): the dilation on chip never exceeds WN_LDS_RING_MAXD = 512."""
    case = _case(run, precision)
    s = case.shape
    t = util.gen_o1(case, half=(precision == 16))
    e0 = P._engine_o1(case, t, precision, mode)
    e0.setRingInLds(-1)
    assert "LR" not in e0.kernelInfo(s.B, False)
    y0 = _free_run(e0, case)
    e0.close()
    e = P._engine_o1(case, t, precision, mode)
    e.setRingInLds(0)
    info = e.kernelInfo(s.B, False)
    held = int(info.split("ring_in_lds=d<=")[1].split()[0]) if "ring_in_lds=d<=" in info else 0
    assert ("LR=1" in info) == (held > 0), info
    print("EDGE ring %s fp%d %s: ring_in_lds d <= %d (%d of %d layers)" % (case.name, precision, mode, held,
                                                                           sum(d <= held for d in E.dilations(s.L, s.maxD)), s.L))
    assert held <= 512, info
    for chunk in (None, 1, 7):
        e.setInputs(t.Lh, t.sel)
        y = _free_run(e, case, chunk)
        assert np.array_equal(y, y0), "ring in LDS (d <= %d), chunk %s: samples differ" % (held, chunk)
    half = s.N // 2
    for first_mode, second_mode in ((0, -1), (-1, 0)):
        e.setInputs(t.Lh, t.sel)
        e.setRingInLds(first_mode)
        assert e.run_partial_chunk(0, half, s.N, s.B)
        e.setRingInLds(second_mode)
        assert e.run_partial_chunk(half, s.N - half, s.N, s.B)
        y = np.full((s.B, s.N), -1, dtype=np.int32)
        e.getYOut(y, 0, s.N)
        e.synchronize()
        assert np.array_equal(y, y0), "ring %s then %s: samples differ" % (first_mode, second_mode)
    e.close()


# ---- e: a maxDilation the schedule never reaches -------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("shape", ["R32", "R64"])
def test_maxdilation_512_over_four_layers_is_maxdilation_8(shape, precision):
    """(L = 4, maxDilation 512) is the schedule 1, 2, 4, 8: an engine built with 512 generates exactly the samples of one built
    with 8 (which the oracle holds: test_schedule_edges_cpu shows the two oracles equal), and a column's state is as large."""
    case = E.case_of(shape, 4, 512)
    s = case.shape
    small = case._replace(name=case.name.replace("maxD512", "maxD8"), shape=s._replace(maxD=8))
    t = util.gen_o1(case, half=(precision == 16))
    for mode in ("wg", "wg2", "chain"):
        ys, bytes_ = [], []
        for c in (case, small):
            e = _create(c, t, precision, mode)
            assert e is not None
            ys.append(_free_run(e, c, c.chunk))
            bytes_.append(e.slotStateBytes())
            _chain_clean(e)
            e.close()
        assert np.array_equal(ys[0], ys[1]), "fp%d %s: maxDilation 512 and 8 generate different samples over four layers" % (precision, mode)
        assert bytes_[0] == bytes_[1] == HEADER_BYTES + 15 * s.R * (2 if precision == 16 else 4), bytes_


# ---- f: slot mode ----------------------------------------------------------------------------------------------------------------------

def _feature_engine(case, t, precision, mode, w, b, columns, xg=None):
    e = TS._engine(case, t, precision, mode, w, b, columns)
    if xg is not None:
        e.setFeatures(xg)
        assert "RAW=3" in e.kernelInfo(columns, True), e.kernelInfo(columns, True)
    return e


def _slot_session(e, xg, y_lock, D, W, big, what):
    """Joins at counters 0, 1 and D + 1 in both tiles; steps of 1 and of `big` (the window; 300 at window 1024); one utterance
    saved from two columns that joined at counters 0 and 1, at the same `done`: the same bytes; one suspended mid-utterance and
    resumed in a column of the other tile at another counter.  Every utterance equals its lockstep column."""
    B, cols = y_lock.shape[0], e.maxBatch
    u = lambda i: i % B
    r = Run(e, xg, W)
    r.start(0, u(0))
    r.start(cols - 2, u(1))
    r.start(3, u(4))
    r.step(1)                                  # counter 1
    r.start(5, u(2))
    r.start(cols - 3, u(4))
    left = D
    while left:                                # counter D + 1
        c = min(big, left)
        r.step(c)
        left -= c
    a = r.save(3)                              # done = D + 1, joined at counter 0
    r.start(cols - 1, u(3))
    r.step(1)
    b = r.save(cols - 3)                       # done = D + 1, joined at counter 1: another rotation of every ring with d > 1
    torch.cuda.synchronize()
    assert torch.equal(a, b), "%s: the blob depends on the column or the join step" % what
    assert a.cpu().numpy()[HEADER_BYTES:].any()
    blob, rec = r.suspend(cols - 2)            # done = D + 2
    assert 0 < rec[2] < rec[3]
    r.step(1)
    r.resume(2, blob, rec)                     # the other tile, three samples on
    sizes = (big, 1) if W > 1 else (1,)
    k = 0
    while r.cols:
        r.step(sizes[k % len(sizes)])
        k += 1
    e.slotsEnd()
    r.check(y_lock, what)
    assert len(r.got) == 6 and all(len(np.concatenate(v)) == y_lock.shape[1] for v in r.got.values())


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("run", E.RUNS, ids=E.run_id)
def test_slot_mode_at_the_edge_schedules(run, precision):
    """The features path (RAW = 3; five feature channels handed over directly).  Lockstep setFeatures + setSelectorSeed against the
    oracle fed Lh = Wcond x + bcond (float64) and philox_selectors(seed): fp32 by the bars of the fp32 test above, fp16 by
    util.fp16_bars, the organisations bit-identical.  Then slot sessions on the smallest legal window, the schedule's largest
    dilation (1 for maxDilation 1; 8 for (4, 512), whatever maxDilation says): _slot_session.  A window that is no multiple of
    the largest dilation is refused."""
    case = _case(run, precision)
    s = case.shape
    half = precision == 16
    D = max(E.dilations(s.L, s.maxD))
    W, big = D, (300 if D == 1024 else D)
    x, w, b = E.feature_model(case, half)
    xg = torch.from_numpy(x).cuda()
    t = util.gen_o1(case, half=half)
    t.Lh = E.feature_lh(case, x, w, b)
    t.sel = O.philox_selectors(TS.SEED, s.N, s.B)
    y_lock = {}
    for mode in (("wg", "wg2", "wg3") if half else ("wg", "wg2")):
        e = _feature_engine(case, t, precision, mode, w, b, s.B, xg)
        y = np.full((s.B, s.N), -1, dtype=np.int32)
        assert e.run_chunks(case.chunk, None, s.N, s.B, y, 1, True)
        e.synchronize()
        got = util.engine_getters(e, s.L)
        got["y"] = y
        ref = P._teacher_forced_ref(case, t, y)
        if half:
            st = util.fp16_bars(ref, got, t.sel.T, "features %s/%s" % (case.name, mode))
            worst = max(st[k] for k in ("Xout_units", "skipOut_units", "Zs_units", "Za_units")) / util.FP16_K
            print("EDGE fp16 features %s %s: worst activation error %.3f of the bar, agreement %.4f" % (case.name, mode, worst, st["agreement"]))
            e.setFeatures(xg)
            y2 = np.full((s.B, s.N), -1, dtype=np.int32)
            assert e.run(s.N, s.B, y2, 1, False)
            e.synchronize()
            assert np.array_equal(y2, y), "dump and no-dump kernel variants disagree"
            assert np.array_equal(y, y_lock.get("wg", y)), "wg and %s disagree in fp16" % mode
        else:
            _fp32_bars(ref, got, t.sel.T, s.B)
        y_lock[mode] = y
        e.close()
    columns = 19
    for mode in (("wg", "wg3") if half else ("wg", "wg2")):
        e = _feature_engine(case, t, precision, mode, w, b, columns)
        bad = [0, -D] + ([D + 1, D // 2, 3 * D // 2] if D > 1 else [])
        assert [lib.nvw_slots_begin(e._h, v) for v in bad] == [0] * len(bad), bad
        if D < s.maxD:
            assert lib.nvw_slots_begin(e._h, 5 * D) == 1                 # (a multiple of the largest dilation, not of maxDilation)
        assert e.slotStateBytes() == HEADER_BYTES + sum(E.dilations(s.L, s.maxD)) * s.R * (2 if half else 4)
        _slot_session(e, xg, y_lock[mode], D, W, big, "%s fp%d %s" % (case.name, precision, mode))
        e.close()
