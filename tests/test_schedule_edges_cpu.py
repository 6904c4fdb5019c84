"""CPU half of the schedule-edge tests (no GPU): what nvw_create_ex refuses, and -- oracle against oracle -- that the seeded inputs
of tests/test_schedule_edges_gpu.py make the schedule matter, so that "the engine's samples are the oracle's" says something about
the schedule the engine ran."""
import numpy as np
import pytest

import schedule_edges as E
import util


@pytest.mark.parametrize("what,args", [
    ("one layer", dict(L=1)), ("no layer", dict(L=0)), ("a negative layer count", dict(L=-1)), ("kMaxLayers + 1", dict(L=E.L_MAX + 1)),
    ("maxDilation 0", dict(maxD=0)), ("batch 0", dict(B=0)), ("no samples", dict(N=0))])
@pytest.mark.parametrize("precision", [32, 16])
def test_create_refuses_what_the_class_asserts(what, args, precision):
    """include/nv_wavenet_c.h, "Errors": NULL and a line on stderr, before any HIP call (so it runs here, like
    test_unsupported_config_is_rejected_loudly) -- not the constructor's assert, which takes the host process with it."""
    from nv_wavenet_amd._lib import lib
    a = dict(L=4, maxD=8, B=3, N=8)
    a.update(args)
    for org in (util.MODE_ORG["auto"], util.MODE_ORG["wg"], util.MODE_ORG["chain"]):
        assert not lib.nvw_create_ex(32, 128, 256, precision, a["L"], a["maxD"], a["B"], a["N"], 1, 1, org), what
    assert not lib.nvw_create(64, 256, 256, precision, a["L"], a["maxD"], a["B"], a["N"], 0, 1), what


def test_the_python_engine_reports_the_refusal():
    from nv_wavenet_amd import WavenetEngine
    with pytest.raises(RuntimeError):
        WavenetEngine(32, 128, 256, 1, 8, 3, 8)
    with pytest.raises(RuntimeError):
        WavenetEngine(32, 128, 256, E.L_MAX + 1, 8, 3, 8, precision=16)


def test_dilations_of_the_edge_schedules():
    assert E.dilations(5, 3) == [1, 2, 1, 2, 1] and E.dilations(7, 6) == [1, 2, 4, 1, 2, 4, 1]
    assert E.dilations(4, 512) == E.dilations(4, 8) == [1, 2, 4, 8] and max(E.dilations(11, 1024)) == 1024
    assert E.dilations(20, 1) == [1] * 20 and E.dilations(3, 4) == [1, 2, 4]


@pytest.mark.parametrize("L,maxD,other", [(5, 3, 4), (7, 6, 8)])
def test_a_maxdilation_that_is_no_power_of_two_is_its_own_schedule(L, maxD, other):
    """The samples under `d > maxDilation -> 1` with maxDilation 3 (6) differ from those with 4 (8): an engine that rounded the
    value to a power of two would not produce the oracle's samples."""
    case = E.case_of("R32", L, maxD)
    t = util.gen_o1(case, half=False)
    y, _ = E.oracle_free_run(case, t)
    y2, _ = E.oracle_free_run(case, t, maxD=other)
    d = max(E.dilations(L, other))
    assert np.array_equal(y[:, :1], y2[:, :1])                       # (the first sample sees silence behind every tap)
    differ = (y != y2).any(axis=1)
    assert differ.mean() >= 0.9, "only %d of %d utterances tell maxDilation %d from %d" % (differ.sum(), len(differ), maxD, other)
    assert d > maxD


def test_a_schedule_that_never_reaches_maxdilation_is_the_schedule_of_its_largest_dilation():
    """(L = 4, maxDilation 512) is 1, 2, 4, 8: the oracle's samples are those of maxDilation 8 -- the identity the engine is held to."""
    case = E.case_of("R32", 4, 512)
    t = util.gen_o1(case, half=False)
    y, a = E.oracle_free_run(case, t)
    y2, a2 = E.oracle_free_run(case, t, maxD=8)
    assert np.array_equal(y, y2)
    for k in a:
        assert np.array_equal(a[k], a2[k]), k


def test_the_1024_tap_counts_at_the_last_sample():
    """(11, 1024) over 1100 samples: the conditioning of layer 0 at sample N - 1 - 1024 is perturbed, the samples held fixed
    (teacher-forced).  Layers 0 .. 9 (d = 1 .. 512) reach back 1023 samples, so at the last sample they are unchanged, bit for bit;
    layer 10 reads x[t - 1024] and changes: the horizon is long enough for that tap to count, and nothing else carries it."""
    case = E.case_of("R32", 11, 1024)
    s = case.shape
    t = util.gen_o1(case, half=False)
    y, a = E.oracle_free_run(case, t)
    Lh = t.Lh.copy()
    t0 = s.N - 1 - 1024
    assert t0 >= 0
    Lh[t0, 0] += np.float32(0.5)
    y2, a2 = E.oracle_free_run(case, t, Lh=Lh, forced=y)
    for l in range(10):
        assert np.array_equal(a["Xout"][l], a2["Xout"][l]), "layer %d sees sample %d at the last sample" % (l, t0)
    scale = np.abs(a["Xout"][10]).max()
    moved = np.abs(a["Xout"][10] - a2["Xout"][10]).max(axis=1)
    assert (moved > 1e-4 * scale).all(), "x[t - 1024] does not reach layer 10 of the last sample: %s" % moved
    # ... and the control of the control: two samples later (layer 0's output reaches layer 9 over 2 + 4 + ... + 512 = 1022
    # samples) the perturbation is inside the reach of layer 9
    Lh = t.Lh.copy()
    Lh[t0 + 2, 0] += np.float32(0.5)
    _, a3 = E.oracle_free_run(case, t, Lh=Lh, forced=y)
    assert not np.array_equal(a["Xout"][9], a3["Xout"][9])
