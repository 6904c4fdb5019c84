"""GPU tests of the LDS layout in which the layers' exchange images (x, h, dilated tap) lie on the head's zs / logits image and the
three places they left hold ring slots (Cfg::OVERLAY, Cfg::ringSlotOffset; `-m gpu`).  C3 at its full dilation range (R 64, S 256,
A 256, 20 layers, maxDilation 512) on the O(1) inputs: every tile of a workgroup real, so that every aliased image is written in
full; 40 samples cover both phases of the d = 2 slots, several wraps and many heads."""
import numpy as np
import pytest

import cases
import util
import test_parity_gpu as T

pytestmark = pytest.mark.gpu

_SHAPE = lambda B, N: cases.Shape(64, 256, 256, 20, B, N, 512)
_inputs = {}


def _case(B, N, half=True):
    """(case, O(1) inputs), generated once per shape and left unchanged."""
    key = (B, N, half)
    if key not in _inputs:
        case = cases.Case("C3_full_overlay_B%d_N%d" % (B, N), 30, [], _SHAPE(B, N), 3, 1, N)
        _inputs[key] = (case, util.gen_o1(case, half=half))
    return _inputs[key]


def _free_run(e, s, chunk=None):
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    if chunk:
        assert e.run_chunks(chunk, None, s.N, s.B, y, 1)
    else:
        assert e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    return y


def _ring_parity(mode, precision, B, N, expect_d=None):
    """Samples with as many ring slots in LDS as fit == samples of the same engine with the ring in HBM: one launch, chunks of 3
    (the launch boundary falls on both phases of the d = 2 slots), LDS-then-HBM and HBM-then-LDS halves."""
    case, t = _case(B, N, half=(precision == 16))
    s = case.shape
    e = T._engine_o1(case, t, precision, mode)
    e.setRingInLds(-1)
    assert "LR" not in e.kernelInfo(s.B, False), e.kernelInfo(s.B, False)
    y0 = _free_run(e, s)
    e.setRingInLds(0)
    info = e.kernelInfo(s.B, False)
    assert "LR=1" in info and "ring_in_lds=d<=" in info, info
    if expect_d is not None:
        assert "ring_in_lds=d<=%d" % expect_d in info.split(), info
    for chunk in (None, 3):
        e.setInputs(t.Lh, t.sel)
        y = _free_run(e, s, chunk)
        assert np.array_equal(y, y0), "%s: ring in LDS, chunk %s: samples differ" % (info, chunk)
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
    return info


def test_three_tiles_hold_d2_in_lds_and_generate_the_same_samples():
    """The headline launch shape: with the three in-place slots the three-tile kernel keeps the layers with d <= 2 on chip."""
    info = _ring_parity("wg3", 16, 48, 40, expect_d=2)
    assert "BT=3" in info and "EMBLDS=1" in info, info


@pytest.mark.parametrize("mode,precision,bt,expect_d", [("wg", 16, 1, 4), ("wg2", 16, 2, 2), ("wg4", 16, 4, 1), ("wg", 32, 1, None)])
def test_other_tile_counts_and_fp32_generate_the_same_samples(mode, precision, bt, expect_d):
    """The overlay is in every Cfg: one, two and four tiles per workgroup and the fp32 engine, 16 utterances per tile.  The fp16
    placements are those tests/test_lds_layout_cpu.py derives from the Cfg constants."""
    info = _ring_parity(mode, precision, 16 * bt, 40, expect_d=expect_d)
    assert "BT=%d" % bt in info, info


def test_dumping_launch_on_the_overlaid_layout_against_the_oracle():
    """One dumping launch (three tiles, 48 utterances, 6 samples): xtOut, skipOut, zs, za and p of the last sample against the fp32
    oracle fed the engine's samples, within the fp16 bars of tests/util.py -- the way test_parity_gpu holds every dump."""
    case, t = _case(48, 6)
    s = case.shape
    e = T._engine_o1(case, t, 16, "wg3")
    assert "BT=3" in e.kernelInfo(s.B, True) and "DUMP=1" in e.kernelInfo(s.B, True), e.kernelInfo(s.B, True)
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, s.B, y, 1, True)
    e.synchronize()
    got = util.engine_getters(e, s.L)
    got["y"] = y
    e.close()
    ref = util.teacher_forced_oracle(case, t, y)
    st = util.fp16_bars(ref, got, t.sel.T, "overlay dump wg3")
    print("overlay dump: %s" % {k: round(v, 4) for k, v in st.items()})


def test_in_place_conditioning_with_the_ring_in_lds_equals_the_packed_run():
    """RAW = 2 (the fp16 conditioning tensor read in place) at three tiles, ring slots in LDS: the packed run's samples."""
    import torch
    case, t = _case(48, 24)
    s = case.shape
    e = T._engine_o1(case, t, 16, "wg3")
    assert "RAW=0" in e.kernelInfo(s.B, False) and "ring_in_lds=d<=2" in e.kernelInfo(s.B, False), e.kernelInfo(s.B, False)
    y_packed = _free_run(e, s)
    Lh16 = torch.from_numpy(t.Lh).cuda().half()
    e.setInputs(t.Lh, t.sel)
    e.setConditioningDirect(Lh16)
    info = e.kernelInfo(s.B, False)
    assert "RAW=2" in info and "BT=3" in info and "LR=1" in info, info
    y = _free_run(e, s)
    assert np.array_equal(y, y_packed), "in-place conditioning with the ring in LDS differs from the packed run"
    e.close()


def test_feature_conditioning_with_the_ring_in_lds_equals_the_ring_in_hbm():
    """RAW = 3 (the conditioning computed in the kernel from upsampled features) at three tiles: ring slots in LDS against the same
    engine with the ring in HBM."""
    import torch
    from nv_wavenet_amd import WavenetEngine
    case, t = _case(48, 24)
    s = case.shape
    n_cond = 80
    rng = np.random.RandomState(5)
    half = lambda a: a.astype(np.float16).astype(np.float32)
    x = half(rng.uniform(-1, 1, (s.B, n_cond, s.N)).astype(np.float32))
    w = half((rng.uniform(-1, 1, (s.L * 2 * s.R, n_cond)) / np.sqrt(n_cond)).astype(np.float32))
    b = rng.uniform(-0.1, 0.1, s.L * 2 * s.R).astype(np.float32)
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, s.B, s.N, impl=1, tanhEmbed=True, precision=16, organisation=util.MODE_ORG["wg3"])
    e.setEmbeddings(t.embP, t.embC)
    for l in range(s.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    e.setConditioningWeights(np.ascontiguousarray(w), b)
    e.setSelectors(t.sel, s.N)
    ys = []
    for ring_mode in (-1, 0):
        e.setRingInLds(ring_mode)
        e.setFeatures(torch.from_numpy(x).cuda())
        info = e.kernelInfo()
        assert "RAW=3" in info and "BT=3" in info and ("LR=1" in info) == (ring_mode == 0), info
        ys.append(_free_run(e, s))
    e.close()
    assert len(np.unique(ys[0])) > 8, "degenerate samples"
    assert np.array_equal(ys[0], ys[1]), "conditioning from features: ring in LDS differs from ring in HBM"
