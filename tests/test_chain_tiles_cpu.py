"""CPU controls of the multi-tile chain tests (no GPU): the inputs of tests/chain_cases.py can reveal a mix-up between the tiles of a
chain, its mirror of the launch plan says what the engine is known to say, and the bars that tests/test_chain_tiles_gpu.py holds
the fp16 kernels to are sized for these inputs.

  1. the gather map keeps every two tiles of every case's batch apart, at 32 to 304 CUs;
  2. the mirror of the plan reproduces what tests/test_parity_gpu.py asserts of the engine (C3 fp16: 5 stages, 51 chains at 256 CUs;
     C4: HOIST exactly beyond four tiles per chain);
  3. every one of a shape's K columns generates samples of its own;
  4. handing one tile's conditioning to another tile of a gathered batch and the other way round changes the samples of nearly
     every lane in which the two differ, and of no other column: a chain that read tile q''s conditioning row, in-place offset,
     ring, mailbox or history for tile q cannot generate the reference's samples;
  5. tests/fp16_model.py -- the oracle's arithmetic with the fp16 engine's rounding points -- passes util.fp16_bars on these inputs,
     30 layers deep, with room to spare;
  6. the comparison the GPU tests make trips on what a mis-addressed chain would deliver (a tile generating another tile's
     utterances, two tiles exchanged, the in-place conditioning strided by the batch) and names the tile, its q and its chain."""
import time

import numpy as np
import pytest

import chain_cases as CC
import fp16_model
import tile_cases as TC
import util


def _free_run(case, t):
    o = util.make_oracle(case, t)
    y = o.run(case.shape.N)
    o.close()
    return y


_free = {}


def _free_run_of(name, half):
    if (name, half) not in _free:
        t0 = time.time()
        _free[(name, half)] = _free_run(CC.case_of(name), CC.inputs(name, half))
        print("CHAIN %s: oracle free run of %d columns, %.2f GMAC: %.2f s" % (name, CC.MODELS[name].K, CC.oracle_macs(name) / 1e9,
                                                                            time.time() - t0))
    return _free[(name, half)]


@pytest.mark.parametrize("ncu", CC.CU_COUNTS)
def test_the_gather_map_keeps_every_two_tiles_apart(ncu):
    for name, precision, org, tpc in CC.CASES:
        pl = CC.plan(name, precision, org, ncu, tpc)
        for B in (pl.batch, pl.max_batch, 16 * (pl.chains + pl.chains // 2) - 5, 16 * pl.chains - 3):
            idx = CC.map_of(name, B)
            assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < CC.MODELS[name].K
            differ, live = CC.tile_distances(idx)
            off = ~np.eye(len(differ), dtype=bool)
            assert (2 * differ >= live)[off].all()
            if B % 16 == 0 and len(differ) > 1:
                assert differ[off].min() >= 8
    # ... and the condition is one that a replicated batch (idx = b % 16, what the older chain tests feed) fails
    with pytest.raises(AssertionError):
        CC.check_map(np.arange(64) % 16)
    with pytest.raises(AssertionError):
        CC.check_map(np.concatenate([np.arange(16), np.arange(16, 32), np.r_[np.arange(9), np.arange(40, 47)]]))


def test_the_mirror_of_the_plan():
    # what test_chain_fills_the_gpu_by_replication / test_chain_with_several_tiles_per_chain assert of the engine at 256 CUs
    pl = CC.plan("C3", 16, "chain", 256, 2)
    assert (pl.stages, pl.lpc, pl.chains) == (5, 5, 51)
    assert pl.batch == 16 * (51 * 2 - 25) - 5 and pl.max_batch == 16 * 51 * 2
    for tpc in range(1, CC.TPC_MAX + 1):
        pl = CC.plan("C4", 16, "chain", 256, tpc)
        assert (pl.stages, pl.lpc, pl.chains) == (16, 2, 16)
        for dump in (False, True):
            fields, hoist = CC.expected_info(pl, pl.batch, pl.batch, dump)
            assert hoist == (tpc > 4 and not dump) and ("HOIST=1" in fields) == hoist
        assert not CC.expected_info(CC.plan("C3", 16, "chain", 256, tpc), 16 * 51 * tpc, 16 * 51 * tpc, False)[1]
    assert not CC.hoist_built("C4", 32) and not CC.hoist_built("A1024", 16) and not CC.hoist_built("C3", 16)
    # the stage and chain counts of the case table
    want = {("C4", 16, "chain"): (16, 2, 16), ("C4", 32, "chain"): (31, 1, 8), ("C3", 16, "chain"): (5, 5, 51),
            ("C3", 16, "chain1"): (21, 1, 12), ("C3", 32, "chain1"): (21, 1, 12), ("R32", 16, "chain1"): (25, 1, 10),
            ("R32", 32, "chain1"): (25, 1, 10), ("A512", 16, "chain1"): (17, 1, 15), ("A1024", 16, "chain"): (7, 2, 36)}
    assert set(want) == set(CC.ORGS)
    for (name, precision, org), v in want.items():
        pl = CC.plan(name, precision, org, 256, 2)
        assert (pl.stages, pl.lpc, pl.chains) == v, (name, precision, org, pl)
    # a capacity beyond the batch: the layout is the capacity's, the chains are the batch's
    pl = CC.plan("R32", 32, "chain1", 256, 3)
    assert CC.expected_info(pl, pl.max_batch, 16 * pl.chains - 3, False)[0] == "DUMP=0> stages=25 layers/stage=1 chains=10 tiles/chain=3 wgs=250 "
    assert CC.expected_info(pl, pl.max_batch, 16 * 4, True)[0] == "DUMP=1> stages=25 layers/stage=1 chains=4 tiles/chain=3 wgs=100 "
    # the balanced split: 20 layers on CUs that hold 8 take 3 stages of 7, 7 and 6 layers
    assert CC.chain_lpc_max(20, 8) == 7 and CC.chain_stages_for(20, 7) == 4 and CC.chain_lpc_max(20, 0) == 0
    assert CC.chain_tpc(1000, 256, 16) == CC.TPC_MAX and CC.chain_tpc(1, 256, 16) == 1 and CC.chain_tpc(17, 256, 16) == 2


def test_the_reference_work_stays_small():
    """At most about 2 GMAC of oracle arithmetic per (shape, precision), and K never below 21."""
    for name in CC.NAMES:
        assert CC.oracle_macs(name) <= 2.0e9 and CC.MODELS[name].K >= 21 and CC.MODELS[name].K % 16 != 0


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", CC.NAMES)
def test_every_column_is_an_utterance_of_its_own(name, half):
    m = CC.MODELS[name]
    y = _free_run_of(name, half)
    assert y.shape == (m.K, m.N)
    distinct = len({row.tobytes() for row in y})
    values = len(np.unique(y))
    print("%s %s: %d distinct columns of %d, %d distinct sample values" % (name, "fp16" if half else "fp32", distinct, m.K, values))
    assert distinct == m.K, "two columns generate the same samples"
    # (the samples use the bins: K N draws from A bins of an order-one distribution)
    assert values >= min(m.rsa[2] // 2, m.K * m.N // 4)


@pytest.mark.parametrize("name", CC.NAMES)
def test_exchanging_two_tiles_conditioning_changes_their_samples(name):
    """A gathered batch of 43 columns = the three tiles of one chain, the last one ragged; tiles 0 and 1 exchange their conditioning.
    The comparand is what the GPU tests compare with: the samples of the K source columns, gathered."""
    B = 43
    idx = CC.map_of(name, B)
    t = CC.gathered(CC.inputs(name, True), idx)
    y = _free_run_of(name, True)[idx]
    Lh = t.Lh.copy()
    Lh[:, :, 0:16], Lh[:, :, 16:32] = t.Lh[:, :, 16:32], t.Lh[:, :, 0:16]
    y2 = _free_run(CC.case_of(name, B), TC.with_inputs(t, Lh=Lh))
    changed = (y != y2).any(axis=1)
    differ = idx[0:16] != idx[16:32]
    assert differ.sum() >= 8
    hit = (changed[0:16][differ].sum() + changed[16:32][differ].sum()) / (2.0 * differ.sum())
    print("%s: lanes in which tiles 0 and 1 differ: %d, columns of them changed: %.3f" % (name, differ.sum(), hit))
    assert changed[0:16][differ].mean() >= 0.9 and changed[16:32][differ].mean() >= 0.9
    other = np.ones(B, dtype=bool)
    other[0:16][differ] = False
    other[16:32][differ] = False
    assert not changed[other].any(), "a gathered column generates the samples of its source column: columns are independent"


def test_the_comparison_names_a_tile_that_took_anothers_place():
    """What a mis-addressed chain would deliver, made on the host from the oracle's samples: tile q = 2 of chain 3 generating tile
    q = 1's utterances (a wrong `q` in a conditioning row, mailbox or history slot), two tiles' outputs exchanged, the in-place
    conditioning strided by the batch instead of the capacity.  The comparison of the GPU tests trips on each and names the place."""
    name, chains, tpc = "R32", 10, 3
    y_ref = _free_run_of(name, True)
    B = 16 * (chains * tpc - chains // 2) - 5
    idx = CC.map_of(name, B)
    good = y_ref[idx]
    CC.assert_same_as_reference(good, y_ref, idx, chains, "as it should be")
    CC.assert_same_as_reference(good[:16 * chains - 3], y_ref, idx, chains, "a prefix of the batch")
    wrong_q = good.copy()
    wrong_q[16 * 23:16 * 24] = good[16 * 13:16 * 14]
    with pytest.raises(AssertionError, match=r"column 368 \(tile 23 = tile q = 2 of chain 3, lane 0; utterance %d\)" % idx[368]):
        CC.assert_same_as_reference(wrong_q, y_ref, idx, chains, "wrong q")
    swapped = good.copy()
    swapped[0:16], swapped[160:176] = good[160:176], good[0:16]
    with pytest.raises(AssertionError, match=r"column 0 \(tile 0 = tile q = 0 of chain 0.*utterances \[%d\]" % idx[160]):
        CC.assert_same_as_reference(swapped, y_ref, idx, chains, "exchanged")
    # [..][maxBatch][2R] read with the running batch as its stride: from the second (sample, layer) row on every column reads
    # another column's conditioning -- at sample 0, layer 1 column b reads what belongs to column (b + B) % cap of layer 0
    cap = 16 * chains * tpc
    idx_cap = CC.map_of(name, cap)
    assert np.array_equal(idx_cap[:B], idx)
    strided = y_ref[idx_cap[(np.arange(B) + B) % cap]]
    with pytest.raises(AssertionError, match="differs from the one-tile run"):
        CC.assert_same_as_reference(strided, y_ref, idx_cap, chains, "batch stride")
    unwritten = good.copy()
    unwritten[B - 1] = -1
    with pytest.raises(AssertionError, match=r"column %d \(tile %d = tile q = 2 of chain 4, lane 10" % (B - 1, (B - 1) // 16)):
        CC.assert_same_as_reference(unwritten, y_ref, idx, chains, "last live lane of the ragged tile")


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_fp16_rounding_model_stays_inside_the_bars(name):
    case = CC.case_of(name)
    t = CC.inputs(name, True)
    y = _free_run_of(name, True)
    got = fp16_model.run(t, case.shape, y)
    t0 = time.time()
    ref = util.teacher_forced_oracle(case, t, y)
    print("CHAIN %s: teacher-forced oracle of %d columns: %.2f s" % (name, CC.MODELS[name].K, time.time() - t0))
    assert np.array_equal(ref["y"], y)
    st = util.fp16_bars(ref, got, t.sel.T, "fp16 model " + name)
    print("fp16 rounding model vs fp32 oracle (%s): %s" % (name, {k: round(v, 4) for k, v in st.items()}))
    # the rounding model alone uses a fraction of the bar (test_parity_bars_cpu.py: below 2 of the FP16_K = 8 units at 20-30 layers)
    for k in ("Xout_units", "skipOut_units", "Zs_units", "Za_units"):
        assert st[k] < 2.0, (k, st[k])
    assert st["agreement"] >= 0.99
