"""GPU tests of the straight-line kernel (wn::wavenet_wg_sl: the L = 20 layers of a sample one behind the other, no control-flow join
with loads in flight; `-m gpu`).  GPU against GPU, as in test_compiled_schedule_gpu.py, whose helpers and inputs these tests share:
the launch the engine takes by default must generate the samples of the run-time schedule (setCompiledSchedule(-1)), element for
element -- whole, in chunks whose boundaries fall on every phase of the d = 2 and d = 4 slots, and with the two kinds of launch
alternating inside one utterance (each launch then runs on the ring and the history the other kind left: equal samples show that what
is handed over is the same).  Models of one and of three cycles keep the cycle-loop kernel.
R 64 / S 256 / A 256, maxDilation 512, fp16, three tiles per workgroup, 48 utterances, O(1) inputs.
LD = 1 of the straight-line kernel: setRingInLds switches the ring in LDS on or off, it does not choose how much of it, and at this
shape and L = 20 the plan holds d <= 2 -- the engine offers no launch of that instantiation here; tests/test_sample_loop_waits_cpu.py
holds its code to the same static properties."""
import numpy as np
import pytest

import test_compiled_schedule_gpu as CS

pytestmark = pytest.mark.gpu

STRAIGHT = "cycles=2"


def _straight(e, yes):
    info = CS._info(e, True)
    assert (STRAIGHT in info.split()) == yes, info
    return info


def test_twenty_layers_whole_and_in_chunks_of_3_and_7():
    """40 samples.  Chunks of 3: launches begin at t = 3, 6, 9, 12 .. (t & 3 = 3, 2, 1, 0: every phase of d = 4, both of d = 2); of 7:
    t = 7, 14, 21, 28, 35 (3, 2, 1, 0, 3)."""
    e, case, t, y0 = CS._both(20, 40, expect_d=2)
    _straight(e, True)
    s = case.shape
    for chunk in (3, 7):
        e.setInputs(t.Lh, t.sel)
        assert np.array_equal(CS._free_run(e, s, chunk), y0), "chunks of %d: samples differ" % chunk
    e.close()


def test_the_two_kinds_of_launch_alternating_inside_one_utterance():
    """Launches of 5 samples, straight-line and run-time schedule in turn (and the other way round): the boundaries fall on
    t & 3 = 1, 2, 3, 0, and every launch but the first continues from the ring slots (HBM and, spilled back, LDS) and the sample
    history that a launch of the other kind wrote."""
    e, case, t, y0 = CS._both(20, 40, expect_d=2)
    s = case.shape
    for first_mode in (0, -1):
        e.setInputs(t.Lh, t.sel)
        mode = first_mode
        for at in range(0, s.N, 5):
            e.setCompiledSchedule(mode)
            if mode == 0:
                _straight(e, True)
            else:
                CS._info(e, False, CS.FIRST)
            assert e.run_partial_chunk(at, 5, s.N, s.B)
            mode = -1 - mode
        y = np.full((s.B, s.N), -1, dtype=np.int32)
        e.getYOut(y, 0, s.N)
        e.synchronize()
        assert np.array_equal(y, y0), "alternating launches, first %d: samples differ (first at sample %d)" % \
            (first_mode, int(np.argmax((y != y0).any(axis=0))))
    e.close()


@pytest.mark.parametrize("L,expect_d", [(10, None), (30, 1)])
def test_other_whole_numbers_of_cycles_keep_the_cycle_loop(L, expect_d):
    e, _, _, _ = CS._both(L, 24, expect_d=expect_d)
    _straight(e, False)
    e.close()
