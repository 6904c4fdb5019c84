"""CPU controls of the multi-tile tests (no GPU): the inputs of tests/tile_cases.py can reveal a mix-up between the tiles of a
workgroup, and the bars that tests/test_tiles_gpu.py holds the fp16 kernels to are sized for these inputs.

  1. every one of the 85 columns generates samples of its own: no two columns agree, and in particular no column of an upper tile
     repeats the column of tile 0 it would be confused with (b mod 16);
  2. handing tile 2's conditioning to tile 0 and the other way round changes the samples of nearly every column of both;
  3. tests/fp16_model.py -- the oracle's arithmetic with the fp16 engine's rounding points -- passes util.fp16_bars on these inputs
     with room to spare, so a GPU run that misses the bars differs by more than rounding."""
import numpy as np
import pytest

import fp16_model
import tile_cases as TC
import util


def _free_run(name, t):
    case = TC.case_of(name)
    o = util.make_oracle(case, t)
    y = o.run(case.shape.N)
    o.close()
    return y


_free = {}


def _free_run_of(name, half):
    if (name, half) not in _free:
        _free[(name, half)] = _free_run(name, TC.inputs(name, half))
    return _free[(name, half)]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", TC.NAMES)
def test_every_column_is_an_utterance_of_its_own(name, half):
    y = _free_run_of(name, half)
    assert y.shape == (TC.COLUMNS, TC.N)
    distinct = len({row.tobytes() for row in y})
    repeats = sum(int(np.array_equal(y[b], y[b % 16])) for b in range(16, TC.COLUMNS))
    values = len(np.unique(y))
    print("%s %s: %d distinct columns of %d, %d equal to column b %% 16, %d distinct sample values" % (
        name, "fp16" if half else "fp32", distinct, TC.COLUMNS, repeats, values))
    assert distinct == TC.COLUMNS, "two columns generate the same samples"
    assert repeats == 0, "a column of an upper tile repeats its column of tile 0"
    # (the samples use the bins: 2 040 draws from 256 / 512 bins of an order-one distribution)
    assert values >= TC.SHAPES[name][0][2] // 2


@pytest.mark.parametrize("name", TC.NAMES)
def test_exchanging_two_tiles_conditioning_changes_their_samples(name):
    t = TC.inputs(name, True)
    y = _free_run_of(name, True)
    Lh = t.Lh.copy()
    Lh[:, :, 0:16], Lh[:, :, 32:48] = t.Lh[:, :, 32:48], t.Lh[:, :, 0:16]
    y2 = _free_run(name, TC.with_inputs(t, Lh=Lh))
    changed = (y != y2).any(axis=1)
    print("%s: columns changed in tile 0: %d, tile 2: %d, elsewhere: %d" % (name, changed[0:16].sum(), changed[32:48].sum(),
                                                                           changed[16:32].sum() + changed[48:].sum()))
    assert changed[0:16].mean() >= 0.9 and changed[32:48].mean() >= 0.9
    assert not changed[16:32].any() and not changed[48:].any(), "columns are independent"


@pytest.mark.parametrize("name", TC.NAMES)
def test_the_fp16_rounding_model_stays_inside_the_bars(name):
    case = TC.case_of(name)
    t = TC.inputs(name, True)
    y = _free_run_of(name, True)
    got = fp16_model.run(t, case.shape, y)
    ref = util.teacher_forced_oracle(case, t, y)
    assert np.array_equal(ref["y"], y)
    st = util.fp16_bars(ref, got, t.sel.T, "fp16 model " + name)
    print("fp16 rounding model vs fp32 oracle (%s): %s" % (name, {k: round(v, 4) for k, v in st.items()}))
    # the rounding model alone uses a fraction of the bar (test_parity_bars_cpu.py: below 2 of the FP16_K = 8 units at 20-30 layers)
    for k in ("Xout_units", "skipOut_units", "Zs_units", "Za_units"):
        assert st[k] < 2.0, (k, st[k])
    assert st["agreement"] >= 0.99
