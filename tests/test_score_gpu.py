"""GPU tests of scoring (`-m gpu`): nvw_score_samples gives, from one time-parallel pass, logp[t] = log softmax(Za_t /
T)[y[t]] of known samples.  The reference is the float64 model of tests/score_cases.py (held to the oracle by
tests/test_score_cpu.py); the bar is the project's logit bar carried through the log-softmax, |d logp| <= 2 delta / T
(score_cases.bar).  Everything that is not a comparison with the reference is one of bytes."""
import numpy as np
import pytest
import torch

import prefill_cases as PF
import score_cases as SC
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import SCORE_REQ, WavenetEngine
from nv_wavenet_amd.slots import SlotStream
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x5C02E0000000011
_nets, _refs = {}, {}


def _engine(case, t, precision, w, b, columns=16, weights=True, tanh_embed=True):
    s = case.shape
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, columns, max(s.N, 64), impl=1 if s.S <= 4 * s.R else 3, tanhEmbed=tanh_embed,
                      precision=precision, organisation=util.MODE_ORG["wg"])
    e.setEmbeddings(t.embP, t.embC)
    for l in range(s.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    if weights:
        e.setConditioningWeights(np.ascontiguousarray(w), b)
    e.setSelectorSeed(SEED)
    return e


class Net:
    """one network with its features, samples to score and (lazily) its references"""

    def __init__(self, shape, seed, precision, L=8, maxD=16, N=48, columns=3):
        self.key = (shape, seed, precision, L, maxD, N)
        self.precision = precision
        self.case, self.t, self.x, self.w, self.b = SC.setup(shape, seed, precision, L, maxD, N, columns)
        self.s = self.case.shape
        self.y = PF.primes(columns, N, shape[2])
        self.xg = torch.from_numpy(self.x).cuda()
        self.yg = torch.from_numpy(self.y).cuda()

    def engine(self, **kw):
        return _engine(self.case, self.t, self.precision, self.w, self.b, **kw)

    def reference(self, c, n, T=1.0):
        """(Za [n][A], logp [n]) of column c's first n samples, computed once"""
        key = self.key + (c, n, float(T))
        if key not in _refs:
            _refs[key] = SC.reference(self.t, self.s, self.y[c, :n], SC.lh_of(self.x[c], self.w, self.b, self.s.R, self.s.L), T)
        return _refs[key]

    def req(self, c, n, T=1.0):
        return (self.yg[c, :n].contiguous(), self.xg[c], T)


def _net(shape, seed, precision, L=8, maxD=16, N=48):
    key = (shape, seed, precision, L, maxD, N)
    if key not in _nets:
        _nets[key] = Net(shape, seed, precision, L, maxD, N)
    return _nets[key]


def _prime_net(precision):
    return _net(*SC.PRIME_SHAPE[:2], precision, *SC.PRIME_SHAPE[2:])


def _hold(net, c, n, T, logp, rows=None, what=""):
    """logp (and rows) of an engine against the reference; returns the largest error in units of the bar"""
    Za, ref = net.reference(c, n, T)
    bar = SC.bar(Za, T, net.precision)
    got = logp.cpu().numpy().astype(np.float64)
    assert got.shape == (n,) and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    worst = float(err.max() / bar)
    at = SC.positions(n, long=n > 272)
    print("%s fp%d n = %d T = %g: max |d logp| = %.3g = %.3f bars (at the listed positions %.3f)" %
          (what, net.precision, n, T, err.max(), worst, err[at].max() / bar))
    assert (err <= bar).all(), "%s: sample %d off by %.3g, bar %.3g" % (what, int(err.argmax()), err.max(), bar)
    if rows is not None:
        full = SC.log_softmax(Za, T)
        rerr = np.abs(rows.cpu().numpy().astype(np.float64) - full)
        print("%s rows: max |d| = %.3f bars" % (what, rerr.max() / bar))
        assert (rerr <= bar).all(), "%s rows: off by %.3g, bar %.3g" % (what, rerr.max(), bar)
        worst = max(worst, float(rerr.max() / bar))
    return worst


# ---- 6. against the reference ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
def test_every_length_around_the_tile_edge(precision):
    """R 64, 8 layers, dilations 1 .. 16: n = 1, 2 (taps before the start everywhere), 15, 16, 17 (the tile edge), 47, 48."""
    net = _prime_net(precision)
    e = net.engine()
    assert e.scoreMaxSamples() > 0 and e.scoreMaxSamples() % 16 == 0
    for i, n in enumerate(SC.LENGTHS):
        c = i % 3
        _hold(net, c, n, 1.0, e.scoreSamples([net.req(c, n)])[0], what="prime shape")
    e.close()


@pytest.mark.parametrize("shape", sorted(SC.BUILT))
@pytest.mark.parametrize("precision", [16, 32])
def test_every_built_shape(shape, precision):
    net = _net(shape, SC.BUILT[shape], precision)
    e = net.engine()
    _hold(net, 1, 47, 1.0, e.scoreSamples([net.req(1, 47)])[0], what="R %d S %d A %d" % shape)
    e.close()


@pytest.mark.parametrize("precision", [16, 32])
def test_a_long_schedule(precision):
    """12 layers, maxDilation 128, n = 300: 19 time tiles, taps a whole tile and more back, the dilation restart."""
    shape, seed, L, maxD, N = SC.LONG
    net = _net(shape, seed, precision, L, maxD, N)
    e = net.engine()
    _hold(net, 0, SC.LONG_N, 1.0, e.scoreSamples([net.req(0, SC.LONG_N)])[0], what="long schedule")
    e.close()


@pytest.mark.parametrize("depth", range(len(SC.DEPTHS)))
@pytest.mark.parametrize("precision", [16, 32])
def test_odd_and_minimal_depth(depth, precision):
    """L = 7 with maxDilation 4, and L = 2: the stream positions of layers 0 and L - 1 are special cases of Cfg::streamPos."""
    shape, seed, L, maxD, N = SC.DEPTHS[depth]
    net = _net(shape, seed, precision, L, maxD, N)
    e = net.engine()
    _hold(net, 2, 47, 1.0, e.scoreSamples([net.req(2, 47)])[0], what="L = %d" % L)
    e.close()


# ---- 7. rows -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(64, 256, 256), (64, 128, 512), (128, 256, 1024)])
@pytest.mark.parametrize("precision", [16, 32])
def test_rows_are_the_whole_log_distribution(shape, precision):
    net = _net(shape, SC.BUILT[shape], precision)
    A, n = shape[2], 47
    e = net.engine()
    logp, rows = e.scoreSamples([net.req(0, n)], rows=True)[0]
    alone = e.scoreSamples([net.req(0, n)])[0]
    e.close()
    _hold(net, 0, n, 1.0, logp, rows, what="A = %d" % A)
    y = net.yg[0, :n].long()
    assert torch.equal(rows[torch.arange(n, device="cuda"), y].view(torch.int32), logp.view(torch.int32)), "rows[t][y[t]] is not logp[t] bit for bit"
    total = torch.exp(rows.double()).sum(dim=1).cpu().numpy()
    assert np.abs(total - 1.0).max() <= A * SC.EPS32 * 4, np.abs(total - 1.0).max()
    assert torch.equal(alone.view(torch.int32), logp.view(torch.int32)), "asking for rows changes logp"


# ---- 8. temperature ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
def test_temperatures(precision):
    net = _prime_net(precision)
    e = net.engine()
    got = {}
    for T in (0.5, 1.0, 2.0, 0.7):
        logp, rows = e.scoreSamples([net.req(1, 48, T)], rows=True)[0]
        _hold(net, 1, 48, T, logp, rows, what="temperature")
        got[T] = logp
    assert not torch.equal(got[0.5], got[1.0])
    st = SlotStream(e, net.s.maxD, pcm=False)
    default = st.score(net.xg[1], net.yg[1, :48])                      # (the temperature left at its default)
    assert torch.equal(default.view(torch.int32), got[1.0].view(torch.int32))
    st.close()
    e.close()


# ---- 9. features as the caller has them --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
def test_feature_tensors_of_either_type_and_any_strides(precision):
    """The same fp16-representable values as an fp32 and an fp16 tensor, channel-major, time-major and as a view with gaps in both
    dimensions: the same bytes, held to the reference once."""
    net = _prime_net(precision)
    x16 = PF.features(3, 48, net.s.R, net.s.L, half=True)[0][2]                                 # [n_cond][48]
    n = 47
    y = net.yg[2, :n].contiguous()
    base = torch.from_numpy(x16).cuda()
    padded = torch.full((2 * base.size(0), 3 + 2 * base.size(1)), 1e4, device="cuda")
    padded[::2, 3::2] = base
    variants = {"fp32 channel-major": base, "fp16 channel-major": base.half(), "fp32 time-major": base.t().contiguous().t(),
                "fp16 time-major": base.half().t().contiguous().t(), "fp32 view with gaps": padded[::2, 3::2], "fp16 view with gaps": padded.half()[::2, 3::2]}
    assert variants["fp32 time-major"].stride() == (1, base.size(0)) and variants["fp32 view with gaps"].stride() == (2 * padded.size(1), 2)
    e = net.engine()
    got = {k: e.scoreSamples([(y, v, 1.0)])[0] for k, v in variants.items()}
    e.close()
    for k, v in got.items():
        assert torch.equal(v.view(torch.int32), got["fp32 channel-major"].view(torch.int32)), k
    Za, ref = SC.reference(net.t, net.s, net.y[2, :n], SC.lh_of(x16, net.w, net.b, net.s.R, net.s.L))
    err = np.abs(got["fp32 channel-major"].cpu().numpy() - ref).max()
    print("features fp%d: %.3f bars" % (precision, err / SC.bar(Za, 1.0, precision)))
    assert err <= SC.bar(Za, 1.0, precision)


# ---- 10. several requests in one call ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
def test_requests_of_one_call_do_not_depend_on_each_other(precision):
    net = _prime_net(precision)
    e = net.engine()
    jobs = [(0, 5, 1.0), (1, 33, 0.7), (2, 48, 1.0)]
    together = e.scoreSamples([net.req(*j) for j in jobs], rows=True)
    again = e.scoreSamples([net.req(*j) for j in jobs], rows=True)
    for (c, n, T), (logp, rows), (logp2, rows2) in zip(jobs, together, again):
        alone, rows_alone = e.scoreSamples([net.req(c, n, T)], rows=True)[0]
        assert torch.equal(logp.view(torch.int32), alone.view(torch.int32)) and torch.equal(rows.view(torch.int32), rows_alone.view(torch.int32)), (c, n)
        assert torch.equal(logp.view(torch.int32), logp2.view(torch.int32)) and torch.equal(rows.view(torch.int32), rows2.view(torch.int32)), (c, n)
        _hold(net, c, n, T, logp, rows, what="three requests")
    e.close()


# ---- 11. nothing past the end ------------------------------------------------------------------------------------------------------

GUARD = 0x7FC0FFEE          # (a NaN pattern no result takes)


def _raw(e, req):
    reqs = np.zeros(1, dtype=SCORE_REQ)
    reqs[0] = tuple(req[k] for k in SCORE_REQ.names)
    got = lib.nvw_score_samples(e._h, reqs.ctypes.data, 1, None)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("precision", [16, 32])
def test_nothing_is_written_before_the_start_or_from_n_on(precision):
    net = _prime_net(precision)
    A = net.s.A
    e = net.engine()
    for n in (1, 17, 47):
        y, x = net.yg[0, :n].contiguous(), net.xg[0]
        ref_logp, ref_rows = e.scoreSamples([net.req(0, n)], rows=True)[0]
        for pinned in ((False, True) if n == 17 else (False,)):
            lbuf = torch.full((n + 64,), GUARD, dtype=torch.int32)
            lbuf = lbuf.pin_memory() if pinned else lbuf.cuda()
            rbuf = torch.full(((n + 2) * A,), GUARD, dtype=torch.int32, device="cuda")
            req = dict(y=y.data_ptr(), n=n, x=x.data_ptr(), precision=32, c_stride=x.stride(0), t_stride=x.stride(1), temperature=1.0,
                       logp=lbuf.data_ptr() + 4 * 29, rows=rbuf.data_ptr() + 4 * A)
            assert _raw(e, req) == 1
            lb, rb = lbuf.cpu().numpy(), rbuf.cpu().numpy()
            assert (lb[:29] == GUARD).all() and (lb[29 + n:] == GUARD).all(), "logp: written outside [0, n), n = %d" % n
            assert (rb[:A] == GUARD).all() and (rb[(n + 1) * A:] == GUARD).all(), "rows: written outside [0, n), n = %d" % n
            assert np.array_equal(lb[29:29 + n], ref_logp.view(torch.int32).cpu().numpy())
            assert np.array_equal(rb[A:(n + 1) * A], ref_rows.view(torch.int32).cpu().numpy().ravel())
    e.close()


# ---- 12. sampler consistency on the engine -----------------------------------------------------------------------------------------

def _wrapper(precision):
    """NVWaveNetEngine over the prime shape's network with zero output biases (the wrapper's), 16 utterances x 48 samples"""
    from nv_wavenet_amd import nv_wavenet as NW
    shape, seed, L, maxD, N = SC.PRIME_SHAPE
    case, t, x, w, b = SC.setup(shape, seed + 7, precision, L, maxD, N, 16)
    t.Bzs[:] = 0
    t.Bza[:] = 0
    kw = SC.wrapper_weights(t, case.shape)
    dev = {k: ([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in v] if isinstance(v, list) else
               torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    wrapper = NW.NVWaveNetEngine(**dev, precision=precision)
    return NW, wrapper, case, t, x, w, b, torch.from_numpy(x).cuda(), torch.from_numpy(w[:, :, None].copy()).cuda(), torch.from_numpy(b).cuda()


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize("T", [1.0, 0.5])
def test_the_scored_distribution_contains_the_engines_draws(precision, T):
    """Free runs of infer_features(seed=) scored with rows: the draw u of every sample (oracle.philox_selectors) lies in the picked
    bin of the CDF built from exp(rows).  fp32: every sample, or u within 1e-5 of the violated edge and y the adjacent bin (the bar
    of tests/test_prime_gpu.py); fp16: at least util.FP16_MIN_AGREEMENT strictly inside, every miss within two bins."""
    NW, wrapper, case, t, x, w, b, xg, cw, cb = _wrapper(precision)
    s = case.shape
    seed = 5
    temp = None if T == 1.0 else T
    y = wrapper.infer_features(xg, cw, cb, NW.Impl.SINGLE_BLOCK, seed=seed, temperature=temp)
    logp, rows = wrapper.score(xg, cw, cb, y, temperature=temp, return_rows=True)
    wrapper.close()
    assert logp.shape == (s.B, s.N) and rows.shape == (s.B, s.N, s.A)
    u = O.philox_selectors(seed, s.N, s.B)
    yh, rh = y.cpu().numpy().astype(np.int64), rows.cpu().numpy()
    inside = 0
    for c in range(s.B):
        ok, bins, edge = SC.cdf_check(rh[c], yh[c], u[:s.N, c].astype(np.float64))
        inside += int(ok.sum())
        if precision == 32:
            assert ((bins[~ok] <= 1) & (edge[~ok] <= 1e-5)).all(), (c, np.nonzero(~ok)[0], bins[~ok], edge[~ok])
        else:
            assert (bins[~ok] <= 2).all(), (c, np.nonzero(~ok)[0], bins[~ok])
    print("fp%d T = %g: %d of %d draws strictly inside the picked bin" % (precision, T, inside, s.B * s.N))
    if precision == 16:
        assert inside >= util.FP16_MIN_AGREEMENT * s.B * s.N


# ---- 13. the engine is undisturbed -------------------------------------------------------------------------------------------------

def test_generation_is_the_same_with_a_score_call_in_between():
    NW, wrapper, case, t, x, w, b, xg, cw, cb = _wrapper(16)
    y1 = wrapper.infer_features(xg, cw, cb, NW.Impl.SINGLE_BLOCK, seed=9)
    logp = wrapper.score(xg, cw, cb, y1, lengths=[48, 0, 17] + [48] * 13)
    assert len(wrapper._engines) == 1, "score() made an engine of its own"
    y2 = wrapper.infer_features(xg, cw, cb, NW.Impl.SINGLE_BLOCK, seed=9)
    wrapper.close()
    assert torch.equal(y1, y2)
    lp = logp.cpu().numpy()
    assert (lp[1] == 0).all() and (lp[2, 17:] == 0).all() and (lp[2, :17] < 0).all() and (lp[0] < 0).all()


def test_slot_streams_and_prefill_are_the_same_with_score_calls_in_between():
    net = _prime_net(16)
    s = net.s
    e, e2 = net.engine(), net.engine()
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, s.maxD, pcm=False)
    blob = e.prefillStates([(net.yg[0, :31].contiguous(), net.xg[0], 3, 1.0)]).cpu()
    hs = [st.submit(net.xg[c], uid=c) for c in range(3)]
    hs2 = [st2.submit(net.xg[c], uid=c) for c in range(3)]
    got, got2 = {h: [] for h in hs}, {h: [] for h in hs2}
    scored = []
    while st.busy():
        for h, (y, _) in st.step(7).items():
            got[h].append(np.array(y))
        st.finished()
        scored.append(st.score(net.xg[1], net.yg[1, :33]))
    while st2.busy():
        for h, (y, _) in st2.step(7).items():
            got2[h].append(np.array(y))
        st2.finished()
    for h, h2 in zip(hs, hs2):
        a, b = np.concatenate(got[h]), np.concatenate(got2[h2])
        assert len(a) == s.N and np.array_equal(a, b), "a scoring stream delivers other samples"
    assert all(torch.equal(v.view(torch.int32), scored[0].view(torch.int32)) for v in scored)
    _hold(net, 1, 33, 1.0, scored[-1], what="SlotStream.score")
    assert torch.equal(e.prefillStates([(net.yg[0, :31].contiguous(), net.xg[0], 3, 1.0)]).cpu(), blob), "a prefill after a score gives another blob"
    st.close(), st2.close()
    e.close(), e2.close()


# ---- 14. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_return_0_write_nothing_and_raise_in_python():
    net = _prime_net(16)
    s = net.s
    A, n = s.A, 31
    e = net.engine()
    y, x = net.yg[0, :n].contiguous(), net.xg[0]
    lbuf = torch.full((n + 8,), GUARD, dtype=torch.int32, device="cuda")
    rbuf = torch.full((n * A + 8,), GUARD, dtype=torch.int32, device="cuda")
    host_y, host_x = np.ascontiguousarray(net.y[0, :n]), np.zeros((80, s.N), dtype=np.float32)

    def call(engine=e, count=1, **kw):
        req = dict(y=y.data_ptr(), n=n, x=x.data_ptr(), precision=32, c_stride=x.stride(0), t_stride=x.stride(1), temperature=1.0,
                   logp=lbuf.data_ptr(), rows=rbuf.data_ptr())
        req.update(kw)
        reqs = np.zeros(2, dtype=SCORE_REQ)
        for i in range(2):
            reqs[i] = tuple(req[k] for k in SCORE_REQ.names)
        got = lib.nvw_score_samples(engine._h, reqs.ctypes.data, count, None)
        torch.cuda.synchronize()
        assert got or (bool((lbuf == GUARD).all()) and bool((rbuf == GUARD).all())), "a refused call wrote into its outputs"
        return got

    bare = net.engine(weights=False)
    assert bare.scoreMaxSamples() == 0 and call(engine=bare) == 0                                          # no conditioning weights
    with pytest.raises(ValueError):
        bare.scoreSamples([net.req(0, n)])
    bare.close()
    assert call(count=0) == 0 and call(count=-1) == 0 and call(count=65536) == 0                           # count outside 1 .. 65535
    assert call(n=0) == 0 and call(n=-3) == 0                                                              # n < 1
    for T in (2.0 ** -11, 2.0 ** 11, float("nan"), 0.0, float("inf")):
        assert call(temperature=T) == 0, T                                                                 # a bad temperature
    assert call(precision=8) == 0 and call(precision=0) == 0                                               # a bad precision
    assert call(c_stride=0) == 0 and call(t_stride=-1) == 0                                                # strides
    assert call(y=0) == 0 and call(x=0) == 0                                                               # NULL
    assert call(y=host_y.ctypes.data) == 0 and call(x=host_x.ctypes.data) == 0                             # host memory
    assert call(logp=0) == 0 and call(logp=lbuf.data_ptr() + 2) == 0                                       # NULL, misaligned
    pageable = np.full(n + 8, GUARD, dtype=np.int32)
    assert call(logp=pageable.ctypes.data) == 0 and (pageable == GUARD).all()                              # pageable host memory
    assert call(rows=rbuf.data_ptr() + 4) == 0                                                             # misaligned rows
    pinned_rows = torch.full((n * A,), GUARD, dtype=torch.int32).pin_memory()
    assert call(rows=pinned_rows.data_ptr()) == 0 and bool((pinned_rows == GUARD).all())                    # rows outside device memory
    # a total over the cap: every buffer is as large as the request says, so that nothing depends on the refusal
    cap = e.scoreMaxSamples()
    assert cap == ((1 << 30) // (s.R * 4 + 2 * s.R * 2 + s.S * 4)) // 16 * 16
    big = cap + 16
    by, bx, bl = torch.zeros(big, dtype=torch.int32, device="cuda"), torch.zeros((80, big), dtype=torch.float16, device="cuda"), \
        torch.full((big,), GUARD, dtype=torch.int32, device="cuda")
    over = dict(y=by.data_ptr(), n=big, x=bx.data_ptr(), precision=16, c_stride=bx.stride(0), t_stride=bx.stride(1), logp=bl.data_ptr(), rows=0)
    assert call(**over) == 0 and bool((bl == GUARD).all())
    assert call(count=2, **dict(over, n=cap // 2 + 16)) == 0 and bool((bl == GUARD).all())                  # ... the SUM of the padded n
    del by, bx, bl
    assert bool((lbuf == GUARD).all()) and bool((rbuf == GUARD).all())
    assert call() == 1                                                                                     # ... and the call they all vary
    assert bool((lbuf[:n] != GUARD).all()) and bool((lbuf[n:] == GUARD).all()) and bool((rbuf[n * A:] == GUARD).all())
    with pytest.raises(ValueError):
        e.scoreSamples([])
    with pytest.raises(ValueError):
        e.scoreSamples([(y, x, 0.0)])
    with pytest.raises(ValueError):
        e.scoreSamples([(y.cpu(), x, 1.0)])
    e.close()


def test_a_batch_over_the_cap_is_split_and_equals_the_reference():
    """NVWaveNetEngine.score splits a batch whose padded lengths exceed scoreMaxSamples() into several engine calls.  The real cap is
    hundreds of thousands of samples; the engine's answer is replaced by 64 here, so that 16 utterances of 48 take 16 calls."""
    NW, wrapper, case, t, x, w, b, xg, cw, cb = _wrapper(32)
    s = case.shape
    y = torch.from_numpy(PF.primes(s.B, s.N, s.A, seed=8)).cuda()
    whole = wrapper.score(xg, cw, cb, y)
    e = next(iter(wrapper._engines.values()))
    calls = []
    real = e.scoreSamples
    e.scoreMaxSamples = lambda: 64
    e.scoreSamples = lambda reqs, **kw: (calls.append(len(reqs)), real(reqs, **kw))[1]
    split = wrapper.score(xg, cw, cb, y)
    assert calls == [1] * s.B, calls
    e.scoreMaxSamples = lambda: 32
    with pytest.raises(ValueError):
        wrapper.score(xg, cw, cb, y)                                       # one utterance does not fit: not offered
    with pytest.raises(ValueError):
        wrapper.score(xg, cw, cb, y, temperature=0.0)
    with pytest.raises(ValueError):
        wrapper.score(xg, cw, cb, y[:, :0])
    wrapper.close()
    assert torch.equal(split.view(torch.int32), whole.view(torch.int32))
    for c in (0, 7, 15):
        Za, ref = SC.reference(t, s, y[c].cpu().numpy(), SC.lh_of(x[c], w, b, s.R, s.L))
        err = np.abs(split[c].cpu().numpy() - ref).max()
        assert err <= SC.bar(Za, 1.0, 32), (c, err)
