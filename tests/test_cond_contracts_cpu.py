"""CPU controls of the conditioning-contract tests (no GPU): the shallow models of tests/cond_contract_cases.py can see a
conditioning row bound to the wrong layer, utterance, tile, gate half, sample or wave, and a tensor strided by the batch instead of
the capacity.

The "engine" is the oracle itself fed mutated conditioning (the style of tests/test_parity_bars_cpu.py): the true oracle is fed the
engine's samples and the very bar functions tests/test_cond_contracts_gpu.py calls must RAISE -- cond_contract_cases.fp32_picks on the
fp32 inputs, util.fp16_bars on the fp16-rounded ones with tests/fp16_model.py (the fp16 engine's rounding points) as the engine.  The
unmutated models pass both.  The fused producer's derived error bar is checked against an fp32-accumulating model of its kernel."""
import time

import numpy as np
import pytest

import cond_contract_cases as K
import fp16_model
import util


def _free_run(case, t):
    o = util.make_oracle(case, t)
    y = o.run(case.shape.N)
    o.close()
    return y


_seconds = {}


def _teacher_forced(name, t, y):
    t0 = time.time()
    ref = util.teacher_forced_oracle(K.case_of(name), t, y)
    _seconds.setdefault(name, time.time() - t0)
    return ref


def _engine_fp32(name, Lh):
    """A stand-in fp32 engine that reads the conditioning Lh: (samples, teacher-forced true oracle)."""
    t = K.inputs(name, False)
    y = _free_run(K.case_of(name), K.with_inputs(t, Lh=Lh))
    return dict(y=y), _teacher_forced(name, t, y)


def _engine_fp16(name, Lh):
    """A stand-in fp16 engine (fp16_model on the free run's history) that reads Lh: (picks + dump, teacher-forced true oracle)."""
    t = K.inputs(name, True)
    tm = K.with_inputs(t, Lh=Lh)
    case = K.case_of(name)
    y = _free_run(case, tm)
    return fp16_model.run(tm, case.shape, y), _teacher_forced(name, t, y)


@pytest.mark.parametrize("name", K.NAMES)
def test_the_unmutated_models_pass_and_use_the_bins(name):
    t32, t16 = K.inputs(name, False), K.inputs(name, True)
    got, ref = _engine_fp32(name, t32.Lh)
    assert K.fp32_picks(ref, got, t32.sel.T, name) == 0
    distinct = len(np.unique(got["y"]))
    print("COND %s: %d distinct picks over %d x %d samples, %.2f GMAC per oracle run" % (name, distinct, K.B, K.N, K.oracle_macs(name) / 1e9))
    assert distinct >= K.MIN_DISTINCT_PICKS
    got, ref = _engine_fp16(name, t16.Lh)
    st = util.fp16_bars(ref, got, t16.sel.T, "fp16 model " + name)
    print("COND %s fp16 rounding model vs fp32 oracle: %s" % (name, {k: round(v, 4) for k, v in st.items()}))
    for k in ("Xout_units", "skipOut_units", "Zs_units", "Za_units"):
        assert st[k] < 2.0, (k, st[k])
    assert len(np.unique(got["y"])) >= K.MIN_DISTINCT_PICKS


@pytest.mark.parametrize("mutation", sorted(K.MUTATIONS))
@pytest.mark.parametrize("name", K.NAMES)
def test_a_misbound_conditioning_row_is_rejected(name, mutation):
    R = K.SHAPES[name][0][0]
    for half in (False, True):
        Lh = K.inputs(name, half).Lh
        Lm = K.MUTATIONS[mutation](Lh, R)
        assert Lm.shape == Lh.shape and Lm.dtype == np.float32 and not np.array_equal(Lm, Lh)
    t32, t16 = K.inputs(name, False), K.inputs(name, True)
    got, ref = _engine_fp32(name, K.MUTATIONS[mutation](t32.Lh, R))
    with pytest.raises(AssertionError):
        K.fp32_picks(ref, got, t32.sel.T, mutation)
    got, ref = _engine_fp16(name, K.MUTATIONS[mutation](t16.Lh, R))
    print("COND %s %s: fp16 teacher-forced agreement %.3f" % (name, mutation, (got["y"] == ref["y"]).mean()))
    with pytest.raises(AssertionError):
        util.fp16_bars(ref, got, t16.sel.T, mutation)


def test_the_mutations_are_what_they_say():
    Lh = K.inputs("C3", False).Lh
    R = 64
    m = K.MUTATIONS["batch_stride_21_in_a_tensor_of_37"](Lh, R)
    cap = K.capacity_tensor(Lh, "other")
    assert cap.shape == (K.N, K.L, K.CAP, 2 * R) and np.array_equal(cap[:, :, :K.B], Lh)
    assert np.array_equal(m[0, 0], Lh[0, 0])                                   # the first row is still the right one
    assert np.array_equal(m[0, 1, :K.CAP - K.B], cap[0, 0, K.B:])              # the second starts in the first row's dead columns
    m = K.MUTATIONS["layer_taken_from_the_next_layer"](Lh, R)
    assert np.array_equal(m[2, 1], Lh[2, 2]) and np.array_equal(m[2, K.L - 1], Lh[3, 0]) and not m[K.N - 1, K.L - 1].any()
    m = K.MUTATIONS["sample_taken_from_the_next_sample"](Lh, R)
    assert np.array_equal(m[2], Lh[3]) and not m[K.N - 1].any()
    m = K.MUTATIONS["tanh_and_sigmoid_halves_swapped"](Lh, R)
    assert np.array_equal(m[..., :R], Lh[..., R:]) and np.array_equal(m[..., R:], Lh[..., :R])
    m = K.MUTATIONS["tile_0_row_used_for_tile_1"](Lh, R)
    assert np.array_equal(m[:, :, 16:], Lh[:, :, :5]) and np.array_equal(m[:, :, :16], Lh[:, :, :16])
    m = K.MUTATIONS["two_utterances_swapped_within_a_tile"](Lh, R)
    assert np.array_equal(m[:, :, 3], Lh[:, :, 4]) and np.array_equal(m[:, :, 4], Lh[:, :, 3]) and (m != Lh).any(axis=(0, 1, 3)).sum() == 2
    m = K.MUTATIONS["one_wave_slice_zeroed"](Lh, R)
    assert not m[..., 16:32].any() and np.array_equal(m[..., 32:], Lh[..., 32:]) and np.array_equal(m[..., :16], Lh[..., :16])


def test_the_oracle_work_stays_small():
    """One teacher-forced oracle run of every shape: the whole table inside the budget; the stated multiply-add counts."""
    for name in K.NAMES:
        if name not in _seconds:
            t = K.inputs(name, False)
            _teacher_forced(name, t, _free_run(K.case_of(name), t))
    total = sum(_seconds[name] for name in K.NAMES)
    print("COND oracle seconds per shape: %s, total %.2f" % ({k: round(v, 2) for k, v in _seconds.items()}, total))
    assert total < K.ORACLE_BUDGET_SECONDS
    assert sum(K.oracle_macs(n) for n in K.NAMES) < 2.0e9 and K.oracle_macs("R256") == 21 * 14 * (5 * 6 * 65536 + 2 * 65536)


@pytest.mark.parametrize("p", K.PRODUCER_CASES, ids=K.producer_id)
def test_the_producers_bar_holds_for_an_fp32_accumulating_model(p):
    """The operands nv_wavenet.py:cond_producer_weights arranges are, row for row, fp16(w[perm] * scale) and fp32(b[perm] * scale)
    of cond_fragment_order; an fp32-accumulating model of the kernel on them stays inside the derived bar of the float64 sums, and
    a product dropped, or a second rounding, does not."""
    import torch
    from nv_wavenet_amd.nv_wavenet import cond_producer_weights
    w, b, x = K.producer_operands(p)
    wfrag, bias, KF, NWF = cond_producer_weights(torch.from_numpy(w).half()[:, :, None], torch.from_numpy(b).half(), K.L, 16)
    assert (KF, NWF) == ((p.n_cond + 31) // 32, 2 * p.R // 32) and wfrag.dtype == torch.float16 and bias.dtype == torch.float32
    wpos, bpos = K.producer_position_operands(w, b, p.R)
    assert np.array_equal(K.producer_wfrag_rows(wfrag.float().numpy())[:, :, :p.n_cond], wpos)
    assert not K.producer_wfrag_rows(wfrag.float().numpy())[:, :, p.n_cond:].any()
    assert np.array_equal(bias.numpy(), bpos)
    want, bar = K.producer_want(wpos, bpos, x)
    got = K.producer_fp32_model(wpos, bpos, x)
    units = np.abs(got - want) / bar
    print("COND producer model nwf %d KF %d N %d tiles %d: max error %.3f of the bar; conditioning std %.3f" %
          (NWF, KF, p.samples, p.tiles, units.max(), want.std()))
    assert units.max() <= 1.0
    assert 0.2 < want.std() < 3.0
    # what the bar must not let through: the last product missing; the sum rounded to fp16 before the bias is added
    k = p.n_cond - 1
    dropped = want - wpos[None, :, None, :, k].astype(np.float64) * x.transpose(1, 0, 2)[:, None, :, None, k]
    assert (np.abs(dropped.astype(np.float16).astype(np.float64) - want) > bar).mean() > 0.5
    f16 = lambda a: a.astype(np.float16).astype(np.float64)
    twice = f16(f16(want - bpos[None, :, None, :]) + bpos[None, :, None, :])
    assert (np.abs(twice - want) > bar).any()
    # fragment order and back
    fr = K.fragments_of_positions(got, p.tiles)
    assert fr.shape == (p.samples, K.L, p.tiles, NWF, 4, 16, 8) and np.array_equal(K.positions_of_fragments(fr), got)
