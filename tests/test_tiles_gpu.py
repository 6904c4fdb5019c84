"""GPU tests of wavenet_wg with two, three and four tiles of 16 utterances per workgroup (`-m gpu`), at every instantiation that
builds such kernels, with EVERY tile holding utterances of its own (tests/tile_cases.py: 85 distinct columns per shape, batches of
16 (BT + 1) + 5; tests/test_tiles_cpu.py shows that these inputs tell the tiles apart).

The one-tile kernel on all 85 columns is held to the oracle first (fp32: exact samples and the reference harness's activation bars;
fp16: util.fp16_bars).  Every multi-tile launch -- packed conditioning, conditioning read in place, conditioning computed from
features, a batch that grows, slot mode, the planner's own choice at a full-chip batch -- must then generate, column by column, the
samples of that run (fp16: bit for bit) and is held to the oracle by its own dumped activations of all its columns."""
import numpy as np
import pytest
import torch

import tile_cases as TC
import util
from nv_wavenet_amd import WavenetEngine
from test_slots_gpu import _check_prefixes, _plan, _slot_run

pytestmark = pytest.mark.gpu

N, CHUNK = TC.N, TC.CHUNK
RAW_OF = {"packed": 0, "raw32": 1, "raw16": 2, "feat": 3}


def _engine(name, precision, mode, B, samples=N, impl=None, feat=False):
    """An engine of batch B with the shape's model; feat: with the conditioning weights of the features path.  (The organisation is
    forced, so the Implementation value only has to be one that accepts the shape: SINGLE_BLOCK refuses S > 4R as the reference's does.)"""
    t = TC.inputs(name, precision == 16)
    s = TC.case_of(name).shape
    if impl is None:
        impl = 1 if s.S <= 4 * s.R else 3
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, B, samples, impl=impl, tanhEmbed=True, precision=precision,
                      organisation=util.MODE_ORG[mode])
    e.setEmbeddings(t.embP, t.embC)
    for l in range(s.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    if feat:
        m, x, w, _ = TC.features(name, precision == 16)
        e.setConditioningWeights(w, m["cond_b"])
    return e


def _condition(e, name, precision, B, cond, selectors):
    """Hands the engine the first B columns' conditioning of kind `cond` (packed / raw32 / raw16: in place / feat) and the selector
    table or the seed of the in-kernel selectors; every kind resets the history."""
    t = TC.inputs(name, precision == 16)
    Lh, sel = TC.first_columns(t, B)
    if cond == "feat":
        x = TC.features(name, precision == 16)[1]
        e.setSelectors(sel)
        e.setFeatures(torch.from_numpy(np.ascontiguousarray(x[:B])).cuda())
    else:
        e.setInputs(Lh, sel)
        if cond != "packed":
            g = torch.from_numpy(Lh).cuda()
            e.setConditioningDirect(g.half() if cond == "raw16" else g)
    if selectors == "philox":
        e.setSelectorSeed(TC.SEED)


def _oracle_inputs(name, precision, cond, selectors, B=TC.COLUMNS):
    """What the oracle is fed for an engine run of the first B columns."""
    t = TC.inputs(name, precision == 16)
    Lh = TC.features(name, precision == 16)[3] if cond == "feat" else t.Lh
    sel = TC.philox_sel() if selectors == "philox" else t.sel
    return TC.with_inputs(t, Lh=Lh[:, :, :B, :], sel=sel[:, :B])


def _single(e, B, samples=N, batch=None):
    """One dump-free launch (the production kernels)."""
    y = np.full((B, samples), -1, dtype=np.int32)
    assert e.run(samples, B if batch is None else batch, y, 1, False)
    e.synchronize()
    assert e.chainStatus() == 0
    return y


def _chunked_dump(e, name, B):
    """run_chunks(7) with the dump on: several launches, the last one dumps the activations of every column."""
    y = np.full((B, N), -1, dtype=np.int32)
    assert e.run_chunks(CHUNK, None, N, B, y, 1, True)
    e.synchronize()
    assert e.chainStatus() == 0
    got = util.engine_getters(e, TC.L)
    got["y"] = y
    return got


def _fp32_checks(ref, got, sel_bn, what):
    """fp32: the samples are the oracle's (a differing pick only with the draw within 1e-5 of a CDF edge of the oracle's pick,
    checked at every teacher-forced position) and the reference harness's activation bars.  Returns the number of such picks."""
    _, unexplained = util.explain_mismatches(ref["y"], got["y"], ref["lo"], ref["hi"], sel_bn, 1e-5)
    assert not unexplained, "%s: unexplained sample mismatches (b,t,ref,got,edge distance): %s" % (what, unexplained[:5])
    misses = np.argwhere(ref["y"] != got["y"])
    for b, n in misses:
        near = min(abs(float(sel_bn[b, n]) - float(ref["lo"][b, n])), abs(float(sel_bn[b, n]) - float(ref["hi"][b, n])))
        assert near <= 1e-5 and abs(int(ref["y"][b, n]) - int(got["y"][b, n])) <= 1, (what, int(b), int(n), near)
    util.compare_activations(ref, got, atol_eps=32)
    return len(misses)


_refs = {}


def _reference(name, precision, cond, selectors):
    """The one-tile kernel (organisation wg) on all 85 columns, memoised: its chunked dumping run `got`, its dump-free launch
    `y_single`, the inputs `t` the oracle is fed and the oracle teacher-forced on its samples, `ref`."""
    key = (name, precision, cond, selectors)
    if key not in _refs:
        B = TC.COLUMNS
        e = _engine(name, precision, "wg", B, feat=cond == "feat")
        _condition(e, name, precision, B, cond, selectors)
        info = e.kernelInfo(B, False)
        assert "wavenet_wg<" in info and "BT=1," in info and "RAW=%d" % RAW_OF[cond] in info, info
        y_single = _single(e, B)
        _condition(e, name, precision, B, cond, selectors)
        got = _chunked_dump(e, name, B)
        e.close()
        t = _oracle_inputs(name, precision, cond, selectors)
        _refs[key] = dict(got=got, y_single=y_single, t=t, ref=util.teacher_forced_oracle(TC.case_of(name), t, got["y"]))
    return _refs[key]


def _hold_reference(name, precision, cond, selectors):
    """The memoised one-tile run against the oracle."""
    r = _reference(name, precision, cond, selectors)
    what = "%s fp%d one tile, %s, %s selectors" % (name, precision, cond, selectors)
    assert np.array_equal(r["y_single"], r["got"]["y"]), what + ": dump-free and dumping launches disagree"
    if precision == 32:
        n = _fp32_checks(r["ref"], r["got"], r["t"].sel.T, what)
        print("TILES %s: %d picks on a CDF edge" % (what, n))
    else:
        st = util.fp16_bars(r["ref"], r["got"], r["t"].sel.T, what)
        print("TILES %s: %s" % (what, {k: round(v, 4) for k, v in st.items()}))
    return r


def _same_columns(y, y_ref, what):
    bad = np.argwhere((y != y_ref[:y.shape[0], :y.shape[1]]).any(axis=1))
    assert bad.size == 0, "%s: column %d (tile %d) differs from the one-tile run" % (what, int(bad[0, 0]), int(bad[0, 0]) // 16)


def _hold(e, name, precision, mode, B, cond, selectors):
    """The engine's dump-free launch and its chunked dumping run of the first B columns: tiles per workgroup and conditioning kind as
    expected, both runs the same samples; fp16: bit-identical to the one-tile run's columns and the dump of all B columns inside
    util.fp16_bars; fp32: held to the oracle as the one-tile run is.  Returns the samples."""
    what = "%s fp%d %s B=%d, %s, %s selectors" % (name, precision, mode, B, cond, selectors)
    raw = RAW_OF[cond]
    base = _reference(name, precision, "feat" if cond == "feat" else "packed", selectors)
    _condition(e, name, precision, B, cond, selectors)
    for dump in (False, True):
        info = e.kernelInfo(B, dump)
        assert "wavenet_wg<" in info and "BT=%d," % TC.launched_bt(name, mode, dump, raw) in info and "RAW=%d" % raw in info, (what, info)
    y1 = _single(e, B)
    _condition(e, name, precision, B, cond, selectors)
    got = _chunked_dump(e, name, B)
    assert np.array_equal(y1, got["y"]), what + ": dump-free and dumping launches disagree"
    sel_bn = base["t"].sel.T[:B]
    if precision == 16:
        _same_columns(got["y"], base["got"]["y"], what)
        st = util.fp16_bars(TC.columns_of(base["ref"], B), got, sel_bn, what)
        print("TILES %s: %s" % (what, {k: round(v, 4) for k, v in st.items()}))
    else:
        if np.array_equal(got["y"], base["got"]["y"][:B]):
            ref = TC.columns_of(base["ref"], B)
        else:      # (a pick on a CDF edge went the other way than in the one-tile run: the oracle is fed THESE samples)
            ref = util.teacher_forced_oracle(TC.case_of(name, B), _oracle_inputs(name, precision, cond, selectors, B), got["y"])
        n = _fp32_checks(ref, got, sel_bn, what)
        print("TILES %s: %d picks on a CDF edge, identical to the one-tile run: %s" % (what, n, np.array_equal(got["y"], base["got"]["y"][:B])))
    return y1


MULTI = [(16, "wg2"), (16, "wg3"), (16, "wg4"), (32, "wg2")]
_id = lambda v: str(v)


@pytest.mark.parametrize("precision", [32, 16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", TC.NAMES)
def test_one_tile_reference_against_the_oracle(name, precision):
    """Organisation wg, B = 85, with the selector table and with in-kernel selectors (the oracle fed philox_selectors)."""
    _hold_reference(name, precision, "packed", "table")
    _hold_reference(name, precision, "packed", "philox")


@pytest.mark.parametrize("precision,mode", MULTI, ids=_id)
@pytest.mark.parametrize("name", TC.NAMES)
def test_packed_conditioning_every_tile_live(name, precision, mode):
    """RAW 0: fp16 with two, three and four tiles per workgroup, fp32 with two; the engine launches three where four do not fit
    (A = 512) and says so.  Table and in-kernel selectors; the ring in LDS (the default) and in HBM give the same samples."""
    B = TC.batch_of(TC.BT_OF[mode])
    e = _engine(name, precision, mode, B)
    y = _hold(e, name, precision, mode, B, "packed", "table")
    _hold(e, name, precision, mode, B, "packed", "philox")
    e.setRingInLds(-1)
    _condition(e, name, precision, B, "packed", "table")
    assert "LR" not in e.kernelInfo(B, False)
    assert np.array_equal(_single(e, B), y), "ring in HBM: samples differ from the default placement"
    e.close()


@pytest.mark.parametrize("precision,mode", MULTI, ids=_id)
@pytest.mark.parametrize("name", TC.NAMES)
def test_conditioning_in_place_every_tile_live(name, precision, mode):
    """setConditioningDirect with an fp32 tensor (RAW 1) and -- fp16 engines -- an fp16 one (RAW 2), two and three tiles per
    workgroup; a request for four runs three (asserted through kernelInfo in _hold)."""
    B = TC.batch_of(TC.BT_OF[mode])
    e = _engine(name, precision, mode, B)
    for cond in (("raw32", "raw16") if precision == 16 else ("raw32",)):
        for selectors in ("table", "philox"):
            _hold(e, name, precision, mode, B, cond, selectors)
    e.close()


@pytest.mark.parametrize("precision,mode", [(16, "wg2"), (16, "wg3"), (32, "wg2")], ids=_id)
@pytest.mark.parametrize("name", TC.NAMES)
def test_conditioning_from_features_every_tile_live(name, precision, mode):
    """RAW 3: setConditioningWeights + setFeatures, in-kernel selectors, against the oracle fed Lh = Wcond x + bcond (float64)."""
    B = TC.batch_of(TC.BT_OF[mode])
    _hold_reference(name, precision, "feat", "philox")
    e = _engine(name, precision, mode, B, feat=True)
    _hold(e, name, precision, mode, B, "feat", "philox")
    e.close()


@pytest.mark.parametrize("name,mode", [("A512", "wg3"), ("R32S128", "wg4")])
def test_a_smaller_batch_then_the_full_one(name, mode):
    """One engine runs 37 columns (three tiles, the last ragged), then -- after resetHistory -- its full batch: the padding tiles and
    the rings the first run touched do not leak into the second."""
    B = TC.batch_of(TC.BT_OF[mode])
    base = _hold_reference(name, 16, "packed", "table")["got"]["y"]
    e = _engine(name, 16, mode, B)
    _condition(e, name, 16, B, "packed", "table")
    y0 = _single(e, B, batch=37)
    _same_columns(y0[:37], base, "%s %s, 37 columns" % (name, mode))
    e.resetHistory()
    e.synchronize()
    y = _single(e, B)
    assert "BT=%d," % TC.launched_bt(name, mode) in e.kernelInfo(B, False)
    _same_columns(y, base, "%s %s, %d columns after 37" % (name, mode, B))
    e.close()


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (32, "wg2")], ids=_id)
@pytest.mark.parametrize("name", ["R32S128", "S8R", "A512"])
def test_slot_mode_with_live_upper_tiles(name, precision, mode):
    """69 columns in slot mode, 85 utterances joining at staggered steps into random free columns of all five tiles, on a window of
    16 samples that the schedule wraps many times: each utterance equals its column of the one-tile lockstep features run with
    in-kernel selectors (uid = column), which the oracle holds."""
    columns, window = 69, 16
    base = _hold_reference(name, precision, "feat", "philox")["got"]["y"]
    plan, counts = _plan(TC.COLUMNS, columns, N, TC.SHAPES[name][1], sizes=(1, 2, 1, 3))
    assert sum(counts) > 3 * window and max(counts) <= window
    assert {p[1] // 16 for p in plan} == set(range(5)), "the plan must put utterances into every tile"
    e = _engine(name, precision, mode, columns, feat=True)
    e.setSelectorSeed(TC.SEED)
    e.slotsBegin(window)
    info = e.kernelInfo()
    assert "RAW=3" in info and "BT=%d," % TC.BT_OF[mode] in info, info
    x = TC.features(name, precision == 16)[1]
    got, _ = _slot_run(e, torch.from_numpy(x).cuda(), plan, counts, window, begin=False)
    e.close()
    _check_prefixes(got, base, plan, "%s fp%d %s slots" % (name, precision, mode))


def test_the_planners_own_choice_at_a512():
    """Implementation AUTO at A = 512, fp16, beyond two tiles per CU: three tiles per workgroup.  The columns repeat the 85 with a
    period that is no multiple of 16, so the tiles of a workgroup still differ.  Beyond three tiles per CU the planner would take
    four, which do not fit the LDS: still three (asked of kernelInfo only)."""
    name, samples = "A512", 12
    base = _hold_reference(name, 16, "packed", "table")["got"]["y"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * (2 * cus + 1) + 5
    idx = np.arange(B) % TC.COLUMNS
    t = TC.inputs(name, True)
    gi = torch.from_numpy(idx).cuda()
    Lh = torch.from_numpy(t.Lh[:samples]).cuda().index_select(2, gi).contiguous()
    sel = torch.from_numpy(t.sel[:samples]).cuda().index_select(1, gi).contiguous()
    e = _engine(name, 16, "auto", B, samples=samples, impl=0)
    e.setInputs(Lh, sel)
    info = e.kernelInfo(B, False)
    assert "wavenet_wg<" in info and "BT=3," in info and "RAW=0" in info, info
    y = _single(e, B, samples=samples)
    e.close()
    bad = np.argwhere((y != base[idx, :samples]).any(axis=1))
    assert bad.size == 0, "column %d (utterance %d) differs from the one-tile run" % (int(bad[0, 0]), int(idx[bad[0, 0]]))
    e2 = _engine(name, 16, "auto", 16 * (3 * cus + 1), samples=samples, impl=0)
    info = e2.kernelInfo(16 * (3 * cus + 1), False)
    e2.close()
    assert "wavenet_wg<" in info and "BT=3," in info, info
