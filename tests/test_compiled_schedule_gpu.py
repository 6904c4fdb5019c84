"""GPU tests of the kernels with the dilation schedule compiled in (wn::wavenet_wg_cs: ten-layer cycles unrolled, every layer's
dilation, slot placement and register-set parity constants; `-m gpu`).  GPU against GPU: the same engine with setCompiledSchedule(0)
and setCompiledSchedule(-1) must generate the same samples, element for element, whole, in chunks and with the two kinds of launch
mixed inside an utterance (the ring state handed over is the same either way).  R 64 / S 256 / A 256, maxDilation 512, fp16, three
tiles per workgroup, 48 utterances (every tile real), O(1) inputs."""
import numpy as np
import pytest

import cases
import util
import test_parity_gpu as T

pytestmark = pytest.mark.gpu

TOKEN = "sched=cycle10"
FIRST = "wn::wavenet_wg<fp16,64,256,256,BT=3,EMBLDS=1,DUMP=0,RAW=0,LR=1>"
B = 48
_inputs = {}


def _case(L, N):
    """(case, O(1) inputs), generated once per (layers, samples) and left unchanged."""
    if (L, N) not in _inputs:
        case = cases.Case("C3_compiled_schedule_L%d_N%d" % (L, N), 30, [], cases.Shape(64, 256, 256, L, B, N, 512), 3, 1, N)
        _inputs[(L, N)] = (case, util.gen_o1(case, half=True))
    return _inputs[(L, N)]


def _info(e, compiled, first=None):
    """kernelInfo of the launch: the first token as ever (`first`), the schedule token behind the others or absent."""
    info = e.kernelInfo(B, False)
    assert first is None or info.split(" ")[0] == first, info
    assert (TOKEN in info.split()) == compiled, info
    if compiled:
        assert info.split()[-1] == TOKEN, info
    return info


def _free_run(e, s, chunk=None):
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    if chunk:
        assert e.run_chunks(chunk, None, s.N, s.B, y, 1)
    else:
        assert e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    return y


def _both(L, N, expect_d=None):
    """(engine, samples of the run-time schedule): the compiled schedule is what the launch takes by default, and one whole launch of
    it generates the same samples."""
    case, t = _case(L, N)
    s = case.shape
    e = T._engine_o1(case, t, 16, "wg3")
    e.setCompiledSchedule(-1)
    first = _info(e, False, FIRST if L == 20 else None).split(" ")[0]
    assert first.startswith("wn::wavenet_wg<fp16,64,256,256,BT=3,") and first.endswith(",DUMP=0,RAW=0,LR=1>"), first
    y0 = _free_run(e, s)
    assert len(np.unique(y0)) > 8, "degenerate samples"
    e.setCompiledSchedule(0)
    info = _info(e, True, first)
    if expect_d is not None:
        assert "ring_in_lds=d<=%d" % expect_d in info.split(), info
    e.setInputs(t.Lh, t.sel)
    assert np.array_equal(_free_run(e, s), y0), "%s: samples differ from the run-time schedule's" % info
    return e, case, t, y0


def test_two_cycles_whole_in_chunks_and_mixed_with_the_run_time_schedule():
    """L = 20, 40 samples: one launch, chunks of 3 (the launch boundary falls on both phases of the d = 2 slots), and
    compiled-then-run-time and run-time-then-compiled halves."""
    e, case, t, y0 = _both(20, 40, expect_d=2)
    s = case.shape
    e.setInputs(t.Lh, t.sel)
    assert np.array_equal(_free_run(e, s, 3), y0), "chunks of 3: samples differ"
    half = s.N // 2
    for first_mode, second_mode in ((0, -1), (-1, 0)):
        e.setInputs(t.Lh, t.sel)
        e.setCompiledSchedule(first_mode)
        _info(e, first_mode == 0, FIRST)
        assert e.run_partial_chunk(0, half, s.N, s.B)
        e.setCompiledSchedule(second_mode)
        _info(e, second_mode == 0, FIRST)
        assert e.run_partial_chunk(half, s.N - half, s.N, s.B)
        y = np.full((s.B, s.N), -1, dtype=np.int32)
        e.getYOut(y, 0, s.N)
        e.synchronize()
        assert np.array_equal(y, y0), "schedule %s then %s: samples differ" % (first_mode, second_mode)
    e.close()


def test_the_longest_taps_live_and_their_slots_wrapped():
    """L = 20, 1 100 samples, in-kernel Philox selectors: behind sample 512 the d = 512 taps are live, behind 1 024 their slots have
    wrapped.  The conditioning is one 64-sample block packed again and again (the benchmark's way: no 1 100-sample tensor)."""
    import torch
    from nv_wavenet_amd import WavenetEngine
    N, blockN, cap = 1100, 64, 1152
    case, t = _case(20, blockN)
    s = case.shape
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, B, cap, impl=case.impl, tanhEmbed=True, precision=16, organisation=util.MODE_ORG["wg3"])
    e.setEmbeddings(t.embP, t.embC)
    for l in range(s.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    blk = torch.from_numpy(np.ascontiguousarray(t.Lh)).cuda()
    ys = []
    for mode in (-1, 0):
        e.setCompiledSchedule(mode)
        _info(e, mode == 0, FIRST)
        e.setSelectorSeed(77)
        e.resetHistory()
        for first in range(0, cap, blockN):
            e.packConditioning(blk, first, blockN)
        assert e.run_partial_chunk(0, N, cap, B)
        y = np.full((B, cap), -1, dtype=np.int32)
        e.getYOut(y, 0, N)
        e.synchronize()
        ys.append(y[:, :N].copy())
    e.close()
    assert len(np.unique(ys[0][:, 1024:])) > 8, "degenerate samples"
    assert np.array_equal(ys[0], ys[1]), "1 100 samples: the compiled schedule differs from the run-time one (first at sample %d)" % \
        int(np.argmax((ys[0] != ys[1]).any(axis=0)))


def test_one_cycle_that_is_first_and_last():
    e, _, _, _ = _both(10, 24)
    e.close()


def test_three_cycles_hold_d1_in_lds():
    """L = 30: a middle cycle.  The larger bias table leaves room for the slots of d <= 1 only: the LD = 1 kernel."""
    e, _, _, _ = _both(30, 24, expect_d=1)
    e.close()


def test_launches_that_are_not_eligible_run_the_run_time_schedule():
    """Ring slots not in LDS (setRingInLds(-1)), and a layer count that is no whole number of cycles: no token, same samples with
    the switch either way."""
    case, t = _case(20, 24)
    s = case.shape
    e = T._engine_o1(case, t, 16, "wg3")
    e.setRingInLds(-1)
    ys = []
    for mode in (-1, 0):
        e.setCompiledSchedule(mode)
        _info(e, False, FIRST.replace(",LR=1", ""))
        e.setInputs(t.Lh, t.sel)
        ys.append(_free_run(e, s))
    e.close()
    assert np.array_equal(ys[0], ys[1])
    case, t = _case(12, 24)
    s = case.shape
    e = T._engine_o1(case, t, 16, "wg3")
    ys = []
    for mode in (-1, 0):
        e.setCompiledSchedule(mode)
        info = e.kernelInfo(B, False)
        assert TOKEN not in info and "BT=3" in info, info
        e.setInputs(t.Lh, t.sel)
        ys.append(_free_run(e, s))
    e.close()
    assert np.array_equal(ys[0], ys[1])
