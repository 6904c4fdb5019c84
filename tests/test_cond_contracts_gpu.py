"""GPU tests of every way an engine takes its conditioning (`-m gpu`), at every (R, S, A) the library builds and in both precisions
(tests/cond_contract_cases.py: 5 layers, 14 samples in chunks of 5, 21 columns; tests/test_cond_contracts_cpu.py shows that the bars
used here reject a conditioning row bound to the wrong layer, utterance, tile, gate half, sample or wave at each of these shapes):

  a. the one-tile kernel with conditioning packed by setInputs, the caller's fragment-order buffer, an fp32 / fp16 tensor read in
     place, and features plus cond_layers weights: the launched kernel is the expected one, the chunked dumping run is held to the
     oracle, the dump-free launch gives the same samples, every tensor contract the packed run's samples bit for bit, the caller's
     memory is what is read and is left alone;
  b. a tensor laid out for a capacity of 37 columns, run with 21: [N][L][37][2R] is the layout, the other columns hold NaN;
  c. the multi-CU chain, wherever it exists, on the in-place tensors and the caller's fragments: the one-tile run's samples;
  d. the fused producer at every fragment count, feature count, block remainder and tile count, held to a float64 evaluation of
     the same fp16 operands by a derived bar, its output consumed by the generation kernel and held to the oracle."""
import numpy as np
import pytest
import torch

import chain_cases
import cond_contract_cases as K
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.nv_wavenet import cond_fragment_order, cond_producer_weights, pack_cond_input, produce_cond_packed
from test_parity_gpu import _check_mode, _engine_o1, _run_dumped, _teacher_forced_ref

pytestmark = pytest.mark.gpu

N, L = K.N, K.L
_prec_id = lambda p: "fp%d" % p if isinstance(p, int) else str(p)


def _engine(name, precision, mode, columns=K.B, feat=False):
    """An engine of `columns` columns with the shape's model (its conditioning and selectors are handed over by _condition)."""
    t = K.inputs(name, precision == 16)
    e = _engine_o1(K.case_of(name), t, precision, mode, B=columns, Lh=_padded(t.Lh, 2, columns, 0.0), sel=_padded(t.sel, 1, columns, 0.5))
    if feat:
        m, _, w, _ = K.features(name, precision == 16)
        e.setConditioningWeights(w, m["cond_b"])
    return e


def _padded(a, axis, columns, fill):
    """The 21 columns of `a` along `axis` as the prefix of `columns` columns holding `fill`."""
    if a.shape[axis] == columns:
        return np.ascontiguousarray(a)
    shape = list(a.shape)
    shape[axis] = columns
    out = np.full(shape, fill, dtype=a.dtype)
    out[(slice(None),) * axis + (slice(0, a.shape[axis]),)] = a
    return out


def _given(e, name, precision, contract, columns=K.B, dead=0.0):
    """The caller's device memory of a contract: the in-place tensor [N][L][columns][2R] (columns beyond the 21 hold `dead`), the
    fragment-order buffer built by pack_cond_input, the features [columns][n_cond][N]; packed: None."""
    t = K.inputs(name, precision == 16)
    if contract == "packed":
        return None
    if contract == "feat":
        return torch.from_numpy(_padded(K.features(name, precision == 16)[1], 0, columns, 0.0)).cuda()
    g = torch.from_numpy(_padded(t.Lh, 2, columns, dead)).cuda()
    if contract == "frags":
        return pack_cond_input(g, precision, e.condTiles())
    return g.half() if contract == "raw16" else g


def _condition(e, name, precision, contract, given, columns=K.B):
    """Hands the engine the conditioning of `contract` and the selector table; every kind starts a new utterance."""
    t = K.inputs(name, precision == 16)
    sel = _padded(t.sel, 1, columns, 0.5)
    if contract == "feat":
        e.setSelectors(sel)
        e.setFeatures(given)
    elif contract == "frags":
        e.setConditioningPacked(given)
        e.setSelectors(sel)
    else:
        e.setInputs(_padded(t.Lh, 2, columns, 0.0), sel)      # (packed; in place: the packed copy it leaves behind must NOT be used)
        if contract != "packed":
            e.setConditioningDirect(given)


def _single(e, columns=K.B, batch=K.B):
    """One dump-free launch (the production kernels) of the first `batch` columns."""
    y = np.full((columns, N), -1, dtype=np.int32)
    assert e.run(N, batch, y, 1, False)
    e.synchronize()
    assert e.chainStatus() == 0
    return y


def _chunked_dump(e, name, columns=K.B, batch=K.B):
    """run_chunks(5) with the dump on: launches of 5 + 5 + 4 samples, the last one dumps; the first `batch` columns."""
    if columns == batch:
        return _run_dumped(e, K.case_of(name), columns, K.CHUNK)
    y = np.full((columns, N), -1, dtype=np.int32)
    assert e.run_chunks(K.CHUNK, None, N, batch, y, 1, True)
    e.synchronize()
    assert e.chainStatus() == 0
    got = util.engine_getters(e, L)
    got["y"] = y
    return K.columns_of(got, batch)


def _oracle_inputs(name, precision, contract):
    t = K.inputs(name, precision == 16)
    return K.with_inputs(t, Lh=K.features(name, precision == 16)[3]) if contract == "feat" else t


def _hold_to_oracle(name, precision, contract, got, what, record=None, t=None):
    """The dumping run `got` of the 21 columns against the oracle fed its samples (memoised per inputs and samples, as _ref_cache
    does): fp32 exact picks and the reference harness's activation bars, fp16 util.fp16_bars.  Returns the oracle's record."""
    t = _oracle_inputs(name, precision, contract) if t is None else t
    ref = _teacher_forced_ref(K.case_of(name), t, got["y"])
    if precision == 32:
        n = K.fp32_bars(ref, got, t.sel.T, what)
        print("CONDGPU %s: %d picks on a CDF edge" % (what, n))
    else:
        st = util.fp16_bars(ref, got, t.sel.T, what)
        print("CONDGPU %s: %s" % (what, {k: round(v, 4) for k, v in st.items()}))
        if record:
            for k, v in st.items():
                record("fp16_" + k, v)
    return ref


def _info(e, contract, columns, what, record=None):
    for dump in (False, True):
        info = e.kernelInfo(columns, dump)
        assert "wavenet_wg<" in info and "BT=1," in info and "RAW=%d" % K.RAW_OF[contract] in info, (what, info)
    print("CONDGPU %s: %s" % (what, e.kernelInfo(columns, False).split(" ")[0]))
    if record:
        record("kernel", e.kernelInfo(columns, False).split(" ")[0])


_packed = {}


def _packed_run(name, precision):
    """The one-tile kernel on conditioning packed by setInputs, memoised: its chunked dumping run and its dump-free launch."""
    key = (name, precision)
    if key not in _packed:
        e = _engine(name, precision, "wg")
        _condition(e, name, precision, "packed", None)
        got = _chunked_dump(e, name)
        _condition(e, name, precision, "packed", None)
        _packed[key] = dict(got=got, y_single=_single(e))
        e.close()
    return _packed[key]


def _same_bits(a, b):
    """torch.equal of the bit patterns (a tensor that holds NaN is not torch.equal to its own clone)."""
    view = torch.int16 if a.dtype == torch.float16 else torch.int32
    return torch.equal(a.view(view), b.view(view))


# ---- a: one tile, every contract -------------------------------------------------------------------------------------------------------
PART_A = [(n, p, c) for n in K.NAMES for p in (32, 16) for c in K.contracts_of(p)]


@pytest.mark.parametrize("name,precision,contract", PART_A, ids=_prec_id)
def test_one_tile_kernel_every_contract(name, precision, contract, record_property):
    what = "%s fp%d one tile %s" % (name, precision, contract)
    e = _engine(name, precision, "wg", feat=contract == "feat")
    _check_mode(e, "wg", K.case_of(name).shape, precision)
    given = _given(e, name, precision, contract)
    before = None if given is None else given.clone()
    _condition(e, name, precision, contract, given)
    _info(e, contract, K.B, what, record_property)
    # 1. the chunked dumping run against the oracle (feat: fed Lh = Wcond x + bcond in float64)
    got = _chunked_dump(e, name)
    _hold_to_oracle(name, precision, contract, got, what, record_property)
    # 2. the dump-free launch
    _condition(e, name, precision, contract, given)
    y = _single(e)
    assert np.array_equal(y, got["y"]), what + ": dump-free and dumping launches disagree"
    if contract in ("raw32", "raw16", "frags"):
        # 3., 4. the packed run's samples, bit for bit (fp16 engines: gen_o1(half=True) makes Lh fp16-representable)
        base = _packed_run(name, precision)
        assert np.array_equal(got["y"], base["got"]["y"]) and np.array_equal(y, base["y_single"]), what + ": differs from the packed run"
        # 5. the caller's memory is left alone
        assert torch.equal(given, before), what + ": the caller's memory was modified"
        # 6. ... and is what is read: no stale packed copy
        neg = (-given).contiguous()
        _condition(e, name, precision, contract, neg)
        y2 = _single(e)
        assert (y2 != y).mean() > 0.5, "%s: negated conditioning changed only %.3f of the picks" % (what, (y2 != y).mean())
    elif contract == "packed":
        base = _packed_run(name, precision)
        assert np.array_equal(got["y"], base["got"]["y"]) and np.array_equal(y, base["y_single"])
    else:
        assert torch.equal(given, before)
    if precision == 32 and contract == "packed":
        with pytest.raises(TypeError):
            e.setConditioningDirect(torch.zeros(N, L, K.B, 2 * e.R, dtype=torch.float16, device="cuda"))
    e.close()


# ---- b: capacity larger than the batch -----------------------------------------------------------------------------------------------------
PART_B = [(n, p, c) for n in K.NAMES for p in (32, 16) for c in (("raw32", "raw16") if p == 16 else ("raw32",))]


@pytest.mark.parametrize("name,precision,contract", PART_B, ids=_prec_id)
def test_in_place_tensor_is_laid_out_for_the_capacity(name, precision, contract):
    """An engine of 37 columns runs 21: the tensor read in place is [N][L][37][2R] -- the batch axis is the engine's, as it is for
    setInputs and the selectors (include/nv_wavenet_c.h) -- whatever the batch of the launch.  Columns 21 .. 36 hold NaN."""
    what = "%s fp%d capacity %d, batch %d, %s" % (name, precision, K.CAP, K.B, contract)
    A = K.SHAPES[name][0][2]
    base = _packed_run(name, precision)
    e = _engine(name, precision, "wg", columns=K.CAP)
    given = _given(e, name, precision, contract, columns=K.CAP, dead=np.nan)
    assert tuple(given.shape) == (N, L, K.CAP, 2 * e.R) and bool(torch.isnan(given[:, :, K.B:]).all()) and not bool(torch.isnan(given[:, :, :K.B]).any())
    before = given.clone()
    _condition(e, name, precision, contract, given, columns=K.CAP)
    _info(e, contract, K.B, what)
    y = _single(e, columns=K.CAP)
    assert (y[:K.B] >= 0).all() and (y[:K.B] < A).all(), what + ": samples outside [0, A)"
    assert np.array_equal(y[:K.B], base["y_single"]), what + ": differs from the run of an engine of 21 columns"
    _condition(e, name, precision, contract, given, columns=K.CAP)
    got = _chunked_dump(e, name, columns=K.CAP)
    for k, v in got.items():
        assert np.all(np.isfinite(v)), "%s: %s of a live column is not finite" % (what, k)
    assert np.array_equal(got["y"], base["got"]["y"]), what + " (chunked): differs from the run of an engine of 21 columns"
    _hold_to_oracle(name, precision, contract, got, what)
    assert _same_bits(given, before), what + ": the caller's tensor was modified"
    e.close()


# ---- c: the chain ------------------------------------------------------------------------------------------------------------------------
PART_C = [(n, p) for n in K.NAMES for p in (32, 16) if chain_cases.LPC[p][K.SHAPES[n][0]] > 0]


def test_the_chain_exists_everywhere_but_at_r256():
    assert [n for n in K.NAMES if (n, 16) not in PART_C or (n, 32) not in PART_C] == ["R256"]


@pytest.mark.parametrize("name,precision", PART_C, ids=_prec_id)
def test_chain_on_in_place_tensors_and_the_callers_fragments(name, precision):
    base = _packed_run(name, precision)
    e = _engine(name, precision, "chain")
    for contract in ("raw32", "raw16", "frags"):
        if contract == "raw16" and precision == 32:
            continue
        what = "%s fp%d chain %s" % (name, precision, contract)
        given = _given(e, name, precision, contract)
        before = given.clone()
        _condition(e, name, precision, contract, given)
        for dump in (False, True):
            assert "wavenet_chain<" in e.kernelInfo(K.B, dump), (what, e.kernelInfo(K.B, dump))
        print("CONDGPU %s: %s" % (what, e.kernelInfo(K.B, False)))
        y = _single(e)
        assert e.chainStatus() == 0 and e.chainFallbacks() == 0, what + ": the launch fell back to wavenet_wg"
        assert np.array_equal(y, base["y_single"]), what + ": differs from the one-tile run"
        _condition(e, name, precision, contract, given)
        got = _chunked_dump(e, name)
        assert e.chainStatus() == 0 and e.chainFallbacks() == 0, what + " (chunked): a launch fell back to wavenet_wg"
        assert np.array_equal(got["y"], base["got"]["y"]), what + " (chunked): differs from the one-tile run"
        _hold_to_oracle(name, precision, contract, got, what)
        assert torch.equal(given, before), what + ": the caller's memory was modified"
        _condition(e, name, precision, contract, (-given).contiguous())
        y2 = _single(e)
        assert e.chainFallbacks() == 0
        assert (y2 != y).mean() > 0.5, "%s: negated conditioning changed only %.3f of the picks" % (what, (y2 != y).mean())
    e.close()


# ---- d: the fused producer ---------------------------------------------------------------------------------------------------------------
NAME_OF_R = {32: "R32S128", 64: "C3", 128: "C4", 256: "R256"}


def _produce(p, samples_allocated):
    """Runs the producer on the case's operands into the first p.samples samples of a buffer of `samples_allocated` pre-filled with
    7.0.  Returns (buffer, wpos, bpos, x, KF, NWF)."""
    w, b, x = K.producer_operands(p)
    wfrag, bias, KF, NWF = cond_producer_weights(torch.from_numpy(w).half().cuda()[:, :, None], torch.from_numpy(b).half().cuda(), L, 16)
    assert (KF, NWF) == ((p.n_cond + 31) // 32, 2 * p.R // 32)
    buf = torch.full((samples_allocated, L, p.tiles, NWF, 4, 16, 8), 7.0, dtype=torch.float16, device="cuda")
    xg = torch.from_numpy(x).half().cuda()
    assert tuple(xg.shape) == (p.tiles * 16, p.samples, 32 * KF) and not bool(xg[:, :, p.n_cond:].any())
    out = produce_cond_packed(xg, wfrag, bias, buf[:p.samples], p.tiles)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    wpos, bpos = K.producer_position_operands(w, b, p.R)
    assert np.array_equal(K.producer_wfrag_rows(wfrag.float().cpu().numpy())[:, :, :p.n_cond], wpos) and np.array_equal(bias.cpu().numpy(), bpos)
    return buf, wpos, bpos, x, KF, NWF


def _hold_producer(p, buf, wpos, bpos, x, KF, NWF, record=None):
    """Every produced value within the derived bar of the float64 sums of the same operands; nothing written past the samples."""
    assert bool((buf[p.samples:] == 7.0).all()), "the producer wrote beyond the samples it was given"
    got = K.positions_of_fragments(buf[:p.samples].float().cpu().numpy())
    want, bar = K.producer_want(wpos, bpos, x)
    assert np.all(np.isfinite(got))
    units = np.abs(got - want) / bar
    k = np.unravel_index(int(units.argmax()), units.shape)
    print("CONDGPU producer nwf %d KF %d N %d tiles %d: max error %.3f of the derived bar" % (NWF, KF, p.samples, p.tiles, units.max()))
    if record:
        record("producer_error_in_bars", float(units.max()))
    assert units.max() <= 1.0, "(sample, layer, column, position) %s: produced %.6f, float64 %.6f, bar %.3g" % (k, got[k], want[k], bar[k])
    assert len(np.unique(got)) > 1000
    return got


@pytest.mark.parametrize("p", K.PRODUCER_CASES[len(K.PRODUCER_ENGINE_CASES):], ids=K.producer_id)
def test_fused_producer_against_float64(p, record_property):
    """KF = 1 .. 4 at R = 64; 5, 8 and 14 samples (blocks of 8) in one tile and three; three samples allocated past the produced."""
    _hold_producer(p, *_produce(p, p.samples + 3), record=record_property)


@pytest.mark.parametrize("p", K.PRODUCER_ENGINE_CASES, ids=K.producer_id)
def test_fused_producer_consumed_by_the_generation_kernel(p, record_property):
    """nwf = 2, 4, 8, 16: the produced buffer against float64, then -- its padding sample zeroed -- handed to setConditioningPacked
    of an fp16 engine of 21 columns, whose chunked dumping run is held to the oracle fed exactly what the buffer holds (fragment
    value / pre-scale, back in channel order)."""
    name = NAME_OF_R[p.R]
    what = "%s fp16 one tile, produced fragments" % name
    e = _engine(name, 16, "wg")
    assert e.condTiles() == p.tiles
    buf, wpos, bpos, x, KF, NWF = _produce(p, N + 1)
    got_pos = _hold_producer(p, buf, wpos, bpos, x, KF, NWF, record_property)
    buf[N].zero_()
    before = buf.clone()
    t = K.inputs(name, True)
    e.setConditioningPacked(buf)
    e.setSelectors(t.sel)
    _info(e, "frags", K.B, what)
    got = _chunked_dump(e, name)
    perm, scale = cond_fragment_order(p.R, 16)
    Lh_eff = np.empty((N, L, K.B, 2 * p.R), dtype=np.float32)
    Lh_eff[..., np.asarray(perm)] = got_pos[:, :, :K.B, :] / np.asarray(scale, dtype=np.float32)
    assert 0.2 < Lh_eff.std() < 1.0
    _hold_to_oracle(name, 16, "frags", got, what, record_property, t=K.with_inputs(t, Lh=Lh_eff))
    e.setConditioningPacked(buf)
    e.setSelectors(t.sel)
    assert np.array_equal(_single(e), got["y"]), what + ": dump-free and dumping launches disagree"
    assert torch.equal(buf, before)
    e.close()


def test_fused_producer_refuses_what_it_cannot_do():
    """kfrags outside 1 .. 4 and tiles, num_samples, num_layers or nwf <= 0: 0 is returned and nothing is written."""
    p = K.PRODUCER_CASES[len(K.PRODUCER_ENGINE_CASES)]
    w, b, x = K.producer_operands(p)
    wfrag, bias, KF, NWF = cond_producer_weights(torch.from_numpy(w).half().cuda()[:, :, None], torch.from_numpy(b).half().cuda(), L, 16)
    xg = torch.from_numpy(x).half().cuda()
    buf = torch.full((p.samples, L, p.tiles, NWF, 4, 16, 8), 7.0, dtype=torch.float16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = (p.tiles, p.samples, L, KF, NWF)
    for at, values in ((3, (0, 5)), (0, (0, -1)), (1, (0, -1)), (2, (0, -1)), (4, (0, -1))):
        for v in values:
            args = list(good)
            args[at] = v
            assert lib.nvw_produce_conditioning_f16(xg.data_ptr(), wfrag.data_ptr(), bias.data_ptr(), buf.data_ptr(), *args, st) == 0, args
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    assert lib.nvw_produce_conditioning_f16(xg.data_ptr(), wfrag.data_ptr(), bias.data_ptr(), buf.data_ptr(), *good, st) == 1
    torch.cuda.synchronize()
    assert not bool((buf == 7.0).all())
