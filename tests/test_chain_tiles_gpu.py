"""GPU tests of wavenet_chain with two to eight tiles of 16 utterances per chain (`-m gpu`), EVERY tile holding utterances of its
own (tests/chain_cases.py: K distinct columns per shape, a launch of B columns takes column idx[b] of them by a map that keeps every
two tiles of the launch apart; tests/test_chain_tiles_cpu.py shows that these inputs tell the tiles apart).  The batches derive from
the GPU's CU count: as many chains as it holds, the upper half of them with one tile fewer, the last tile ragged.

The reference is the one-tile wavenet_wg on the K columns, held to the oracle first (fp32: exact samples and the reference harness's
activation bars; fp16: util.fp16_bars).  Every chain launch must then say what the mirror of the plan says (stages, layers per
stage, chains, tiles per chain, HOIST), complete without giving up or falling back, and generate in column b, bit for bit in fp16
and in fp32, the samples of reference column idx[b]: a stage that took tile q''s conditioning row, in-place offset, ring, mailbox,
sample history or utterance number for tile q generates another utterance's samples there."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import tile_cases as TC
import util
from nv_wavenet_amd import WavenetEngine
from test_tiles_gpu import _fp32_checks

pytestmark = pytest.mark.gpu


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(name, precision, org, capacity):
    m = CC.MODELS[name]
    t = CC.inputs(name, precision == 16)
    R, S, A = m.rsa
    e = WavenetEngine(R, S, A, m.L, m.maxD, capacity, m.N, impl=3, tanhEmbed=True, precision=precision, organisation=util.MODE_ORG[org])
    e.setEmbeddings(t.embP, t.embC)
    for l in range(m.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    return e


_device = {}


def _gathered(name, precision, idx):
    """(Lh [N][L][B][2R], sel [N][B]) of the launch on the device: columns idx of the shape's K, gathered there."""
    key = (name, precision)
    if key not in _device:
        t = CC.inputs(name, precision == 16)
        _device[key] = (torch.from_numpy(t.Lh).cuda(), torch.from_numpy(t.sel).cuda())
    Lh, sel = _device[key]
    gi = torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
    return Lh.index_select(2, gi).contiguous(), sel.index_select(1, gi).contiguous()


def _condition(e, name, precision, idx, cond="packed", seed=None):
    """Hands the engine the gathered conditioning of kind `cond` (packed / raw32 / raw16: read in place) and the gathered selector
    table, or the seed of the in-kernel selectors; every kind resets the history."""
    Lh, sel = _gathered(name, precision, idx)
    e.setInputs(Lh, sel)
    if cond != "packed":
        e.setConditioningDirect(Lh.half() if cond == "raw16" else Lh)
    if seed is not None:
        e.setSelectorSeed(seed)


def _check_info(e, pl, B, dump, what):
    info = e.kernelInfo(B, dump)
    fields, hoist = CC.expected_info(pl, e.maxBatch, B, dump)
    assert ("wavenet_chain<fp%d,%d,%d,%d," % ((pl.precision,) + CC.MODELS[pl.name].rsa)) in info, (what, info)
    assert fields in info and ("HOIST=1" in info) == hoist, (what, info, fields)
    return info


def _done(e, what):
    """The launches so far ran on the chain: none gave up, none was re-run on wavenet_wg (which would prove nothing about the chain)."""
    e.synchronize()
    status, fallbacks = e.chainStatus(), e.chainFallbacks()
    assert status == 0 and fallbacks == 0, "%s: chainStatus %#x, %d launches re-run on wavenet_wg, last give-up code %#x" % (
        what, status, fallbacks, e.chainLastTimeout())


def _launch(e, B, chunk=None, dump=False, what=""):
    """One launch of B columns, or run_chunks(chunk) (its launches after the first start at init_sample != 0: the tags restart and
    the head reloads its per-tile history); the samples [B][N]."""
    y = np.full((e.maxBatch, e.maxSamples), -1, dtype=np.int32)
    if chunk is None:
        assert e.run(e.maxSamples, B, y, 1, dump), what
    else:
        assert e.run_chunks(chunk, None, e.maxSamples, B, y, 1, dump), what
    _done(e, what)
    return y[:B]


_same_as_reference = CC.assert_same_as_reference      # (y, y_ref, idx, chains, what): column b holds reference column idx[b]


# ---- the reference: one tile per workgroup on the K columns, held to the oracle ---------------------------------------------------
_refs = {}


def _reference(name, precision):
    """Memoised: the one-tile kernel's chunked dumping run `got`, its dump-free launch `y_single`, the oracle teacher-forced on its
    samples `ref`, the inputs `t`."""
    key = (name, precision)
    if key not in _refs:
        m = CC.MODELS[name]
        t = CC.inputs(name, precision == 16)
        e = _engine(name, precision, "wg", m.K)
        e.setInputs(t.Lh, t.sel)
        info = e.kernelInfo(m.K, False)
        assert "wavenet_wg<" in info and "BT=1," in info and "RAW=0" in info, info
        y_single = _launch(e, m.K)
        e.setInputs(t.Lh, t.sel)
        y = _launch(e, m.K, chunk=m.chunk, dump=True)
        got = util.engine_getters(e, m.L)
        got["y"] = y
        e.close()
        _refs[key] = dict(got=got, y_single=y_single, t=t, ref=util.teacher_forced_oracle(CC.case_of(name), t, y), held=False)
    return _refs[key]


def _hold_reference(name, precision):
    """The memoised one-tile run against the oracle (as tests/test_tiles_gpu.py holds its own); returns its samples [K][N]."""
    r = _reference(name, precision)
    if not r["held"]:
        what = "%s fp%d one tile" % (name, precision)
        assert np.array_equal(r["y_single"], r["got"]["y"]), what + ": dump-free and dumping launches disagree"
        if precision == 32:
            n = _fp32_checks(r["ref"], r["got"], r["t"].sel.T, what)
            print("CHAIN %s: %d picks on a CDF edge" % (what, n))
        else:
            st = util.fp16_bars(r["ref"], r["got"], r["t"].sel.T, what)
            print("CHAIN %s: %s" % (what, {k: round(v, 4) for k, v in st.items()}))
        r["held"] = True
    return r["got"]["y"]


def _hold_dump(name, precision, got, idx, what):
    """A chain's dumped activations of all its columns (whose samples are the reference's, column idx[b]) against the teacher-forced
    oracle record of the reference, gathered."""
    r = _reference(name, precision)
    ref = CC.gather_columns(r["ref"], idx)
    sel_bn = r["t"].sel.T[idx]
    if precision == 16:
        st = util.fp16_bars(ref, got, sel_bn, what)
        print("CHAIN %s: %s" % (what, {k: round(v, 4) for k, v in st.items()}))
    else:
        print("CHAIN %s: %d picks on a CDF edge" % (what, _fp32_checks(ref, got, sel_bn, what)))


def _getters(e, B, y):
    got = {k: (v[:, :B] if k in ("Xout", "skipOut") else v[:B]) for k, v in util.engine_getters(e, e.numLayers).items()}
    got["y"] = y
    return got


# ---- tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", sorted({(n, p) for n, p, _ in CC.ORGS}), ids=lambda v: str(v))
def test_one_tile_reference_against_the_oracle(name, precision):
    _hold_reference(name, precision)


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_packed_conditioning_every_tile_distinct(case):
    """One dump-free launch, then run_chunks from reset history: both the reference's samples."""
    name, precision, org, tpc = case
    what = CC.case_id(case)
    y_ref = _hold_reference(name, precision)
    pl = CC.plan(name, precision, org, _ncu(), tpc)
    B = pl.batch
    idx = CC.map_of(name, B)
    e = _engine(name, precision, org, B)
    _condition(e, name, precision, idx)
    print("CHAIN %s: B = %d, %s" % (what, B, _check_info(e, pl, B, False, what)))
    y = _launch(e, B, what=what)
    _same_as_reference(y, y_ref, idx, pl.chains, what + ", one launch")
    e.resetHistory()
    y2 = _launch(e, B, chunk=CC.MODELS[name].chunk, what=what)
    e.close()
    _same_as_reference(y2, y_ref, idx, pl.chains, what + ", chunked")


@pytest.mark.parametrize("case", [("C4", 16, "chain", 5), ("C3", 16, "chain", 2), ("R32", 32, "chain1", 3), ("A1024", 16, "chain", 2)],
                         ids=CC.case_id)
def test_dumping_launch_with_several_tiles_per_chain(case):
    """DUMP=1 (never the hoisting instantiation): chunked, the last launch dumps the activations of all B columns."""
    name, precision, org, tpc = case
    what = CC.case_id(case) + " dumping"
    y_ref = _hold_reference(name, precision)
    pl = CC.plan(name, precision, org, _ncu(), tpc)
    B = pl.batch
    idx = CC.map_of(name, B)
    e = _engine(name, precision, org, B)
    _condition(e, name, precision, idx)
    info = _check_info(e, pl, B, True, what)
    assert "DUMP=1" in info and "HOIST" not in info, info
    y = _launch(e, B, chunk=CC.MODELS[name].chunk, dump=True, what=what)
    got = _getters(e, B, y)
    e.close()
    _same_as_reference(y, y_ref, idx, pl.chains, what)
    _hold_dump(name, precision, got, idx, what)


@pytest.mark.parametrize("case", [("C4", 16, "chain", 2), ("C4", 16, "chain", 5), ("R32", 16, "chain1", 3), ("R32", 32, "chain1", 2)],
                         ids=CC.case_id)
def test_conditioning_in_place_every_tile_distinct(case):
    """setConditioningDirect: an fp32 tensor, and -- fp16 engines -- an fp16 one; at five tiles per chain the HOIST=1 kernel runs with
    condRawKind != 0.  The samples are those of the packed run of the same launch."""
    name, precision, org, tpc = case
    y_ref = _hold_reference(name, precision)
    pl = CC.plan(name, precision, org, _ncu(), tpc)
    B = pl.batch
    idx = CC.map_of(name, B)
    e = _engine(name, precision, org, B)
    _condition(e, name, precision, idx)
    y_packed = _launch(e, B, what=CC.case_id(case) + " packed")
    _same_as_reference(y_packed, y_ref, idx, pl.chains, CC.case_id(case) + " packed")
    for cond in (("raw32", "raw16") if precision == 16 else ("raw32",)):
        what = "%s %s" % (CC.case_id(case), cond)
        _condition(e, name, precision, idx, cond)
        info = _check_info(e, pl, B, False, what)
        assert ("HOIST=1" in info) == (name == "C4" and tpc == 5), info
        y = _launch(e, B, what=what)
        _same_as_reference(y, y_ref, idx, pl.chains, what + ", one launch")
        assert np.array_equal(y, y_packed)
        e.resetHistory()
        y2 = _launch(e, B, chunk=CC.MODELS[name].chunk, what=what)
        _same_as_reference(y2, y_ref, idx, pl.chains, what + ", chunked")
    e.close()


@pytest.mark.parametrize("case", [("C4", 16, "chain", 4), ("R32", 16, "chain1", 8)], ids=CC.case_id)
def test_in_kernel_selectors_every_tile_distinct(case):
    """setSelectorSeed: the Philox draws depend on the utterance NUMBER, so the reference is the one-tile wavenet_wg on the same
    gathered B columns; chain and wavenet_wg agree on every column, and 32 columns taken evenly from every q level are held to the
    oracle fed philox_selectors(seed, N, B)[:, columns], teacher-forced."""
    name, precision, org, tpc = case
    what = CC.case_id(case) + " philox"
    m = CC.MODELS[name]
    pl = CC.plan(name, precision, org, _ncu(), tpc)
    B = pl.batch
    idx = CC.map_of(name, B)
    e = _engine(name, precision, org, B)
    _condition(e, name, precision, idx, seed=CC.SEED)
    _check_info(e, pl, B, False, what)
    y = _launch(e, B, what=what)
    _condition(e, name, precision, idx, seed=CC.SEED)
    y_dump = _launch(e, B, chunk=m.chunk, dump=True, what=what)
    got = _getters(e, B, y_dump)
    e.close()
    assert np.array_equal(y, y_dump), what + ": dump-free and dumping launches disagree"
    w = _engine(name, precision, "wg", B)
    _condition(w, name, precision, idx, seed=CC.SEED)
    info = w.kernelInfo(B, False)
    assert "wavenet_wg<" in info and "BT=1," in info, info
    y_wg = _launch(w, B, what=what + " one tile")
    w.close()
    _same_as_reference(y, y_wg, np.arange(B), pl.chains, what)
    # the columns held to the oracle: 32 / tpc of every level q
    level = (np.arange(B) // 16) // pl.chains
    assert level.max() == tpc - 1
    cols = np.concatenate([np.flatnonzero(level == q)[np.linspace(0, (level == q).sum() - 1, 32 // tpc).astype(int)] for q in range(tpc)])
    assert len(np.unique(cols)) == 32
    sel = util.O.philox_selectors(CC.SEED, m.N, B)[:, cols]
    t = TC.with_inputs(CC.inputs(name, precision == 16), Lh=CC.inputs(name, precision == 16).Lh[:, :, idx[cols], :], sel=sel)
    sub = {k: (v[:, cols] if k in ("Xout", "skipOut") else v[cols]) for k, v in got.items()}
    ref = util.teacher_forced_oracle(CC.case_of(name, len(cols)), t, sub["y"])
    st = util.fp16_bars(ref, sub, sel.T, what)
    print("CHAIN %s: %s" % (what, {k: round(v, 4) for k, v in st.items()}))


@pytest.mark.parametrize("name,precision,org", [("C4", 16, "chain"), ("R32", 32, "chain1")], ids=lambda v: str(v))
def test_capacity_larger_than_the_batch(name, precision, org):
    """An engine with the capacity (and so the mailbox layout) of three tiles per chain runs 16 (chains + chains // 2) - 5 columns
    (q = 0 full, q = 1 half, q = 2 empty), packed and -- its tensor of the capacity's width, the maxBatch stride -- in place; after
    resetHistory 16 chains - 3 (one tile per chain); then its full capacity."""
    y_ref = _hold_reference(name, precision)
    pl = CC.plan(name, precision, org, _ncu(), 3)
    cap = pl.max_batch
    idx = CC.map_of(name, cap)
    e = _engine(name, precision, org, cap)
    B1, B2 = 16 * (pl.chains + pl.chains // 2) - 5, 16 * pl.chains - 3
    CC.check_map(idx[:B1]), CC.check_map(idx[:B2])
    for cond in ("packed", "raw32"):
        what = "%s fp%d %s capacity %d, %d columns %s" % (name, precision, org, cap, B1, cond)
        _condition(e, name, precision, idx, cond)
        _check_info(e, pl, B1, False, what)
        _same_as_reference(_launch(e, B1, what=what), y_ref, idx, pl.chains, what)
    for B in (B2, cap):
        what = "%s fp%d %s capacity %d, then %d columns in place" % (name, precision, org, cap, B)
        e.resetHistory()
        _check_info(e, pl, B, False, what)
        _same_as_reference(_launch(e, B, what=what), y_ref, idx, pl.chains, what)
    what = "%s fp%d %s capacity %d, all columns packed, chunked" % (name, precision, org, cap)
    _condition(e, name, precision, idx)
    _same_as_reference(_launch(e, cap, chunk=CC.MODELS[name].chunk, what=what), y_ref, idx, pl.chains, what)
    e.close()


def test_a_smaller_batch_then_the_full_one():
    """A512 fp16, five tiles per chain: one engine runs two levels and three tiles of the third, the last one ragged, then -- after
    resetHistory -- its full batch: the rings and padding lanes the first run touched do not leak into the second."""
    name, precision, org, tpc = "A512", 16, "chain1", 5
    y_ref = _hold_reference(name, precision)
    pl = CC.plan(name, precision, org, _ncu(), tpc)
    B = pl.batch
    idx = CC.map_of(name, B)
    B0 = 16 * (2 * pl.chains + min(3, pl.chains)) - 7
    CC.check_map(idx[:B0])
    e = _engine(name, precision, org, B)
    _condition(e, name, precision, idx)
    what = "A512 fp16 chain1 capacity %d, %d columns" % (B, B0)
    _check_info(e, pl, B0, False, what)
    _same_as_reference(_launch(e, B0, what=what), y_ref, idx, pl.chains, what)
    e.resetHistory()
    what = "A512 fp16 chain1, %d columns after %d" % (B, B0)
    _check_info(e, pl, B, False, what)
    _same_as_reference(_launch(e, B, what=what), y_ref, idx, pl.chains, what)
    e.close()
