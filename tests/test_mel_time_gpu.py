"""GPU tests of the time-parallel upsampling pass and of prefill and scoring from mel frames (`-m gpu`):
nvw_upsample_requests writes, by request and sample range, the rows the lockstep upsampling computes -- BIT FOR BIT --, and
nvw_prefill_states_mel / nvw_score_samples_mel are the feature passes fed from such rows.  Equality is the contract: rows against
setMel + upsampleFeatures + getFeatures, blobs against sequentially mel-primed columns, log-likelihoods against scoreSamples fed
the lockstep features; the float64 references (the transposed convolution, the teacher-forced network) hold what the equalities
rest on.  Shapes: tests/mel_time_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import condgen
import mel_time_cases as MT
import prefill_cases as PF
import score_cases as SC
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import PREFILL_MEL_REQ, SCORE_MEL_REQ, UPSAMPLE_REQ
from nv_wavenet_amd.slots import SlotState, SlotStream
from oracle import oracle as O
from test_prefill_gpu import _first_difference
from test_slots_gpu import SEED, _engine
from test_slots_mel_gpu import _half, _mel_engine, _mel_inputs, _mel_lockstep
from test_upsampling_hops_gpu import B as HOP_B, C1, HOP, NAMES as HOP_NAMES, _net as _hop_net, _ulp16

pytestmark = pytest.mark.gpu


def _rows_of(fr, tiles):
    """[n][tiles][kf][4][16][EPL] fragments of getFeatures -> [tiles * 16][n][channels] (channel (kf TPF + tk) 16 + 4 g + r)"""
    n, tpf = fr.shape[0], fr.shape[-1] // 4
    a = fr.reshape(n, tiles, -1, 4, 16, tpf, 4)                    # [n][tile][kf][g][j][tk][r]
    return a.permute(1, 4, 0, 2, 5, 3, 6).reshape(tiles * 16, n, -1)


def _bits(a):
    """a tensor as integers: equality of these is equality bit for bit"""
    return a.contiguous().view(torch.int16 if a.dtype == torch.float16 else torch.int32)


def _views(melg, u, k):
    """utterance u's frames as view k mod 4: fp32, fp16, channels-last fp32, channels-last fp16 (the values are exact in fp16)"""
    return (melg[u], melg[u].half(), melg[u].t().contiguous().t(), melg[u].half().t().contiguous().t())[k % 4]


def _lock_rows(e, melg, N):
    """the lockstep rows of every utterance: setMel + upsampleFeatures(0, N) + getFeatures, unpacked; [B][N][channels], T_data"""
    e.setMel(melg)
    e.upsampleFeatures(0, N)
    return _rows_of(e.getFeatures(0, N), e.condTiles())


def _calls(N, stride, B):
    """The calls of the row tests, {name: [(utterance, first_sample, count)]}, and what the host launches for each:
    cuts         the six ranges of mel_time_cases.ranges, of different utterances: a few columns;
    four_groups  whole utterances, 49 .. 64 columns: the most the L2 variant takes -- at stride 1100 its waves go round the phase loop twice;
    many         the six ranges and at least 65 columns more of whole utterances: the LDS variant -- at stride 1100 every workgroup
                 stages a second phase."""
    frames = N // stride
    rg = MT.ranges(N, stride)
    assert len(rg) == 6 and rg[3] == (stride + 1, 2 * stride + 3) and rg[3][0] + rg[3][1] <= N
    cuts = [((3 * i) % B, a, c) for i, (a, c) in enumerate(rg)]
    four, cols = [], 0
    while cols < 49:          # whole utterances, the last one cut where 64 columns are full
        c = min(N, (64 - cols) * stride)
        four.append((len(four) % B, 0, c))
        cols += -(-c // stride)
    many = cuts + [(i % B, 0, N) for i in range(max(B, -(-65 // frames)))]
    calls = dict(cuts=cuts, four_groups=four, many=many)
    assert 48 < MT.columns([r[1:] for r in four], stride) <= 64 and MT.columns([r[1:] for r in many], stride) > 64 + MT.columns(rg, stride) - 1
    assert MT.plan([r[1:] for r in four], stride)[0] == "l2" and MT.plan([r[1:] for r in many], stride)[0] == "lds"
    return calls


def _check_call(e, melg, lock, reqs, n_cond, what):
    """one upsampleRequests call -- request i through view i mod 4 of its utterance's frames -- against the lockstep rows, bit for bit"""
    row = e.upsampleRowElems()
    assert row == 16 * -(-n_cond // 16)
    got = e.upsampleRequests([(_views(melg, u, i), a, c) for i, (u, a, c) in enumerate(reqs)])
    for i, ((u, a, c), rows) in enumerate(zip(reqs, got)):
        assert rows.shape == (c, row) and rows.dtype == lock.dtype
        assert not rows[:, n_cond:].any(), "%s: channels >= n_cond of request %d are not zero" % (what, i)
        bad = (_bits(rows) != _bits(lock[u, a:a + c, :row].to(rows.device))).any(1).nonzero().flatten()
        assert bad.numel() == 0, "%s: request %d (utterance %d, samples [%d, %d)) differs from the lockstep rows first at sample %d" % (
            what, i, u, a, a + c, a + int(bad[0]))
    return got


# ---- 1. rows equal the lockstep upsampling --------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("name", MT.ROW_CASES)
def test_rows_equal_the_lockstep_upsampling_bit_for_bit(name, precision):
    """The conditioning cases (8 / 2; 12 / 4 with 37 channels; 10 / 5; 16 / 8 with one utterance), the three calls of _calls each:
    requests of different utterances -- fp32 and fp16 frames, [n_cond][frames] and channels-last views, whatever the engine's
    precision -- over (0, N), (1, 1), (stride - 1, 2), (stride + 1, 2 stride + 3), a start that is a multiple of 16 (and not of the
    stride where the stride allows it) and the last sample alone; through the L2 variant and through the LDS variant."""
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, precision)
    s = case.shape
    mel = _half(mel)          # (exact in fp16 views too)
    e = _mel_engine(case, t, precision, "wg", w, m, up_w, cc.stride, s.B)
    melg = torch.from_numpy(mel).cuda()
    lock = _lock_rows(e, melg, s.N)
    assert not lock[:s.B, :, e.upsampleRowElems():].any()
    for call, reqs in _calls(s.N, cc.stride, s.B).items():
        _check_call(e, melg, lock, reqs, cc.n_cond, "%s fp%d %s" % (name, precision, call))
    e.close()


_hop_cache = {}


def _hop(name, precision):
    """Per real hop and precision, computed once: the C1 network with HOP_B utterances of mel_time_cases.HOP_FRAMES frames (exact in
    fp16), the lockstep rows of all of them (CPU tensor [B][N][channels], T_data), and for utterance 0 the float64 transposed
    convolution and S = |b| + sum |w x| (test_upsampling_hops_gpu's bars)."""
    key = (name, precision)
    if key not in _hop_cache:
        if len(_hop_cache) >= 2:          # (the rows of the long hops take tens of MiB)
            _hop_cache.pop(next(iter(_hop_cache)))
        cc = HOP[name].cc
        case = C1._replace(shape=C1.shape._replace(B=HOP_B, N=MT.HOP_FRAMES * cc.stride))
        m = condgen.make_cond_model(cc, case.shape)
        rnd = _half if precision == 16 else (lambda a: a)
        mel, up_w, w = _half(m["features"]), rnd(m["up_w"]), rnd(m["cond_w"][:, :, 0])
        e = _mel_engine(case, _hop_net(precision), precision, "wg", w, m, up_w, cc.stride, HOP_B)
        lock = _lock_rows(e, torch.from_numpy(mel).cuda(), case.shape.N).cpu()
        e.close()
        md, wd, bd = torch.from_numpy(mel[:1]).double(), torch.from_numpy(up_w).double(), torch.from_numpy(m["up_b"]).double()
        want = F.conv_transpose1d(md, wd, bd, stride=cc.stride)[0, :, :case.shape.N].numpy()
        S = F.conv_transpose1d(md.abs(), wd.abs(), bd.abs(), stride=cc.stride)[0, :, :case.shape.N].numpy()
        _hop_cache[key] = dict(cc=cc, case=case, m=m, mel=mel, up_w=up_w, w=w, lock=lock, want=want, S=S)
    return _hop_cache[key]


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("name", HOP_NAMES)
def test_rows_at_real_hops_equal_the_lockstep_rows_and_the_float64_convolution(name, precision):
    """1024 / 256, 800 / 200 (37 channels), 1375 / 275 (five taps: 125 KiB of operand in fp32) and 1100 / 1100 (more phases than the
    grid), 21 utterances of five frames, the three calls of _calls each: the six ranges that cut frames through the L2 variant;
    four column groups through it, which at stride 1100 is more (phase, group) work than its grid, so that its loop goes round
    twice; and the ranges among 21 whole utterances through the LDS variant, which stages the whole operand and at stride 1100 a
    second phase per workgroup.  Every row equals the lockstep row bit for bit, and the whole range of utterance 0 from either
    variant is within the bars test_upsampling_hops_gpu derives of the float64 transposed convolution (2 K 2^-24 S; fp16: one unit
    in the last place more)."""
    H = _hop(name, precision)
    cc, N, half = H["cc"], H["case"].shape.N, precision == 16
    calls = _calls(N, cc.stride, HOP_B)
    if cc.stride > MT.GRID:
        assert MT.plan([r[1:] for r in calls["four_groups"]], cc.stride) == ("l2", 2) and MT.plan([r[1:] for r in calls["many"]], cc.stride) == ("lds", 2)
    e = _mel_engine(H["case"], _hop_net(precision), precision, "wg", H["w"], H["m"], H["up_w"], cc.stride, HOP_B)
    melg = torch.from_numpy(H["mel"]).cuda()
    K = (cc.window // cc.stride) * cc.n_cond
    for call, reqs in calls.items():
        got = _check_call(e, melg, H["lock"], reqs, cc.n_cond, "%s fp%d %s" % (name, precision, call))
        assert reqs[0] == (0, 0, N)
        xe = got[0][:, :cc.n_cond].t().double().cpu().numpy()          # utterance 0: [n_cond][N]
        want, bar = H["want"], 2.0 * K * 2.0 ** -24 * H["S"]
        if half:
            bar = bar + _ulp16(want)
            want = want.astype(np.float16).astype(np.float64)
        d = np.abs(xe - want)
        print("rows %s fp%d %s: largest error %.4f of the bar" % (name, precision, call, float((d / bar).max())))
        assert np.isfinite(xe).all() and (d <= bar).all()
    e.close()


# ---- 2. nothing else is read or written -----------------------------------------------------------------------------------------

def _raw_upsample(e, reqs):
    """nvw_upsample_requests itself: reqs = [(mel tensor, frames, first, count, dst address)]"""
    r = np.zeros(max(len(reqs), 1), dtype=UPSAMPLE_REQ)
    for i, (mel, frames, first, count, dst) in enumerate(reqs):
        r[i] = (mel.data_ptr(), 16 if mel.dtype == torch.float16 else 32, mel.stride(0), mel.stride(1), frames, first, count, dst)
    return lib.nvw_upsample_requests(e._h, r.ctypes.data, len(reqs), None)


@pytest.mark.parametrize("call", ["cuts", "many"])
@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("name", ["cond_C3_B21_n37", "hop256"])
def test_only_the_frames_of_the_rule_are_read_and_only_the_rows_are_written(name, precision, call):
    """NaN in every frame outside frames_read(a, b) and in the frames >= `frames` of a longer tensor, a sentinel pattern before
    and after each destination: the rows are those of the clean call, the sentinels intact -- through the L2 variant (cuts) and
    through the LDS variant (many)."""
    if name in HOP:
        H = _hop(name, precision)
        cc, case, m, mel, up_w, w, t, batch = H["cc"], H["case"], H["m"], H["mel"], H["up_w"], H["w"], _hop_net(precision), HOP_B
    else:
        cc = condgen.COND_BY_NAME[name]
        case, m, mel, up_w, w, t = _mel_inputs(cc, precision)
        batch = case.shape.B
    N, stride = case.shape.N, cc.stride
    frames = N // stride
    e = _mel_engine(case, t, precision, "wg", w, m, up_w, stride, batch)
    melg = torch.from_numpy(mel).cuda()
    row, esz = e.upsampleRowElems(), 2 if precision == 16 else 4
    todo = _calls(N, stride, batch)[call]
    clean = e.upsampleRequests([(melg[u], a, c) for u, a, c in todo])
    pad = 256
    bufs, reqs, keep = [], [], []
    for u, a, c in todo:
        lo, hi = MT.frames_read(a, a + c, cc.window, stride)
        written = max(hi + 1, -(-(a + c) // stride))                       # frames * stride >= a + c
        dirty = torch.full((cc.n_cond, frames + 2), float("nan"), device="cuda")
        dirty[:, lo:hi + 1] = melg[u][:, lo:hi + 1]
        buf = torch.full((pad + c * row * esz + pad,), 0xAB, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        keep.append(dirty)
        bufs.append(buf)
        reqs.append((dirty, written, a, c, buf.data_ptr() + pad))
    assert _raw_upsample(e, reqs) == len(reqs)
    torch.cuda.synchronize()
    for i, ((u, a, c), buf) in enumerate(zip(todo, bufs)):
        assert bool((buf[:pad] == 0xAB).all()) and bool((buf[pad + c * row * esz:] == 0xAB).all()), "request %d: written outside its rows" % i
        got = buf[pad:pad + c * row * esz].view(clean[i].dtype).reshape(c, row)
        assert torch.equal(_bits(got), _bits(clean[i])), "request %d ([%d, %d)): a frame outside frames_read reached the rows" % (i, a, a + c)
    e.close()


# ---- 3. prefilled blobs ---------------------------------------------------------------------------------------------------------

class MelSetup:
    """a network (score_cases.setup: the O(1) recipe, prefill_cases' conditioning weights) with an upsampling and mel frames"""

    def __init__(self, shape, seed, precision, hop, L=8, maxD=16, N=48, columns=3):
        self.precision, self.window, self.stride, self.columns = precision, hop[0], hop[1], columns
        self.case, self.t, _, self.w, self.b = SC.setup(shape, seed, precision, L, maxD, N, columns)
        self.s = self.case.shape
        assert N % self.stride == 0
        rng = np.random.RandomState(seed + hop[0])
        taps = hop[0] // hop[1]
        self.up_w = ((rng.rand(PF.N_COND, PF.N_COND, hop[0]) - 0.5) * (3.46 / np.sqrt(taps * PF.N_COND))).astype(np.float32)
        self.up_b = ((rng.rand(PF.N_COND) - 0.5) * 0.2).astype(np.float32)
        self.mel = _half(rng.standard_normal((columns, PF.N_COND, N // self.stride)).astype(np.float32))
        self.melg = torch.from_numpy(self.mel).cuda()
        self.y = PF.primes(columns, N, self.s.A)
        self.yg = torch.from_numpy(self.y).cuda()

    def engine(self, columns=None):
        e = _engine(self.case, self.t, self.precision, "wg", self.w, self.b, columns or self.columns)
        e.setUpsampling(self.up_w, self.up_b, self.stride)
        return e

    def lock(self):
        """the lockstep-upsampled features of every utterance, [columns][n_cond][N] in T_data (a view of the rows)"""
        e = self.engine()
        rows = _lock_rows(e, self.melg, self.s.N)[:self.columns, :, :PF.N_COND].clone()
        e.close()
        return rows.transpose(1, 2)


def _sequential_mel_blobs(e, melg, jobs, window, lead=5):
    """test_prefill_gpu._sequential_blobs with mel columns: jobs = [(column, uid, y CUDA int32 [n], T)]"""
    e.slotsBegin(window)
    if lead:
        e.slotStartMel(e.maxBatch - 1, melg[0], 0)
        assert e.slotsStep(lead)
        e.slotStop(e.maxBatch - 1)
    for col, uid, y, T in jobs:
        e.slotStartMel(col, melg[uid], uid)
        if T != 1.0:
            e.slotSetTemperature(col, T)
        e.slotPrime(col, y)
    blobs, done = {}, 0
    for n in sorted({int(y.numel()) for _, _, y, _ in jobs}):
        while done < n:
            c = min(window, n - done)
            assert e.slotsStep(c)
            done += c
        for col, uid, y, T in jobs:
            if y.numel() == n:
                blob, got = e.slotSave(col)
                assert got == n, (got, n)
                blobs[col] = blob.cpu().numpy().tobytes()
    e.slotsEnd()
    return blobs


def _check_blobs(ms, lengths, what, temperature=1.0):
    """every length's blob -- all through ONE prefillStatesMel call -- against the sequentially mel-primed column's, against
    prefillStates fed the rows of upsampleRequests, and (negative control) against the same call on frames shifted by one"""
    cols = ms.columns
    e = ms.engine(len(lengths) + 1)
    jobs = [(i, i % cols, ms.yg[i % cols, :n].contiguous(), temperature if i % 2 else 1.0) for i, n in enumerate(lengths)]
    pre = e.prefillStatesMel([(y, ms.melg[uid], uid, T) for _, uid, y, T in jobs])
    W = e.prefillWindow()
    rows = e.upsampleRequests([(ms.melg[uid], PF.first_tile_sample(y.numel(), ms.s.L, ms.s.maxD), y.numel() - PF.first_tile_sample(y.numel(), ms.s.L, ms.s.maxD))
                               for _, uid, y, _ in jobs])
    feats = []
    for (_, uid, y, _), r in zip(jobs, rows):          # rows.t()[:n_cond] placed so that column t0 is the first row
        t0 = PF.first_tile_sample(y.numel(), ms.s.L, ms.s.maxD)
        full = torch.zeros((y.numel(), r.size(1)), dtype=r.dtype, device="cuda")
        full[t0:] = r
        feats.append(full.t()[:PF.N_COND])
    via = e.prefillStates([(y, x, uid, T) for (_, uid, y, T), x in zip(jobs, feats)])
    assert torch.equal(pre, via), "%s: prefillStatesMel differs from prefillStates fed the rows of upsampleRequests" % what
    shifted = torch.roll(ms.melg, 1, dims=2).contiguous()
    other = e.prefillStatesMel([(y, shifted[uid], uid, T) for _, uid, y, T in jobs])
    seq = _sequential_mel_blobs(e, ms.melg, jobs, ms.s.maxD)
    pre_host, other_host = pre.cpu().numpy(), other.cpu().numpy()
    for i, (col, uid, y, T) in enumerate(jobs):
        diff = _first_difference(seq[col], pre_host[i].tobytes())
        assert diff is None, "%s, utterance %d, n = %d: prefilled blob differs from the sequential one: %s" % (what, uid, y.numel(), diff)
        assert np.array_equal(pre_host[i, :PF.HEADER_BYTES], other_host[i, :PF.HEADER_BYTES])
        assert not np.array_equal(pre_host[i, PF.HEADER_BYTES:], other_host[i, PF.HEADER_BYTES:]), "%s: shifted frames give the same payload" % what
    assert W == PF.window(ms.s.L, ms.s.maxD)
    e.close()


PRIME_SHAPE = (64, 128, 256)


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize("hop", MT.PRIME_HOPS, ids=lambda h: "%d_%d" % h)
def test_prefilled_mel_blobs_equal_the_sequentially_primed_columns_byte_for_byte(hop, precision):
    """R 64, 8 layers, dilations 1 .. 16, 48 samples at 8 / 2, 12 / 4, 16 / 8 and 48 / 16 (one frame per time tile); the lengths 1,
    2, 15, 16, 17, 40, 47 in one call, every other request at temperature 0.5."""
    ms = MelSetup(PRIME_SHAPE, 961, precision, hop)
    _check_blobs(ms, MT.PRIME_LENGTHS, "prime shape %d / %d fp%d" % (hop + (precision,)), temperature=0.5)


@pytest.mark.parametrize("precision", [16, 32])
def test_prefilled_mel_blobs_over_a_long_window(precision):
    """12 layers, W = 272, 304 samples at 16 / 8, n = 100 and 300: the window of n = 300 starts at 16, inside a frame."""
    shape, seed, L, maxD, N = PF.LONG
    ms = MelSetup(shape, seed, precision, MT.LONG_HOP, L, maxD, N)
    assert PF.first_tile_sample(300, L, maxD) == 16 and 16 % MT.LONG_HOP[0] == 0
    _check_blobs(ms, MT.LONG_LENGTHS, "long window fp%d" % precision)


@pytest.mark.parametrize("precision", [16, 32])
def test_prefilled_mel_blobs_at_hop_256(precision):
    """the C1 network at 1024 / 256, three frames: n = 255, 256, 257 around the first frame edge, and 600"""
    ms = MelSetup((32, 128, 256), 962, precision, (1024, 256), N=768)
    _check_blobs(ms, MT.C1_HOP256_LENGTHS, "hop 256 fp%d" % precision)


@pytest.mark.parametrize("R", sorted(PF.OTHER_R))
@pytest.mark.parametrize("precision", [16, 32])
def test_prefilled_mel_blobs_at_one_shape_per_other_R(R, precision):
    shape, seed = PF.OTHER_R[R]
    ms = MelSetup(shape, seed, precision, MT.OTHER_R_HOP)
    _check_blobs(ms, MT.OTHER_R_LENGTHS, "R %d fp%d" % (R, precision))


# ---- 4. resumed states ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
def test_resumed_mel_states_continue_as_the_lockstep_mel_run(precision):
    """A state from prefillStatesMel of a lockstep run's own first n samples, resumed with slotResumeMel in another column at
    another counter, delivers from n on the samples of column uid of setMel + generate_stream.  fp32: that run is held to the
    oracle as test_slots_mel_gpu holds it."""
    name, mode = "cond_C3_B16", "wg2"
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, precision)
    s = case.shape
    y_lock = _mel_lockstep(case, t, precision, mode, mel, w, m, up_w, cc.stride)
    if precision == 32:
        e = _mel_engine(case, t, 32, mode, w, m, up_w, cc.stride, s.B)
        x = _lock_rows(e, torch.from_numpy(mel).cuda(), s.N)[:s.B, :, :cc.n_cond].cpu().numpy().transpose(0, 2, 1)      # [B][n_cond][N]
        e.close()
        lh = np.einsum("oc,bct->bot", w.astype(np.float64), x.astype(np.float64)) + m["cond_b"].astype(np.float64)[None, :, None]
        t.Lh = np.ascontiguousarray(lh.reshape(s.B, s.L, 2 * s.R, s.N).transpose(3, 1, 0, 2).astype(np.float32))
        t.sel = O.philox_selectors(SEED, s.N, s.B)
        ref = util.teacher_forced_oracle(case, t, y_lock)
        _, unexplained = util.explain_mismatches(ref["y"], y_lock, ref["lo"], ref["hi"], t.sel.T, 1e-5)
        assert not unexplained and (ref["y"] == y_lock).mean() >= 0.999
    melg = torch.from_numpy(mel).cuda()
    todo = [(u, n) for u, n in zip(range(1, s.B), (1, 2, 15, 16, 17, 40, 47, s.N // 2 + 1, s.N - 1))]
    e = _mel_engine(case, t, precision, mode, w, m, up_w, cc.stride, s.B)
    primes = [torch.from_numpy(np.ascontiguousarray(y_lock[u, :n])).cuda() for u, n in todo]
    blobs = e.prefillStatesMel([(y, melg[u], u, 1.0) for (u, n), y in zip(todo, primes)])
    W = 2 * max(32, s.maxD)
    e.slotsBegin(W)
    e.slotStartMel(0, melg[0], 0)
    assert e.slotsStep(3)
    e.slotStop(0)
    for i, (u, n) in enumerate(todo):
        e.slotResumeMel(1 + i, blobs[i].contiguous(), melg[u])
    got = {u: [] for u, _ in todo}
    left = {u: s.N - n for u, n in todo}
    while any(left.values()):
        c = min(7, max(left.values()))
        y = np.full((s.B, c), -1, dtype=np.int32)
        assert e.slotsStep(c, y)
        for i, (u, n) in enumerate(todo):
            k = min(c, left[u])
            got[u].append(y[1 + i, :k])
            left[u] -= k
            if k and left[u] == 0:
                e.slotStop(1 + i)
    e.slotsEnd()
    e.close()
    for u, n in todo:
        g = np.concatenate(got[u])
        bad = np.nonzero(g != y_lock[u, n:])[0]
        assert len(g) == s.N - n and bad.size == 0, "utterance %d resumed at %d leaves its lockstep column at sample %d" % (u, n, n + (bad[0] if bad.size else -1))


# ---- 5. scoring -----------------------------------------------------------------------------------------------------------------

def _score_setup(precision, long):
    if long:
        shape, seed, L, maxD, N = SC.LONG
        return MelSetup(shape, seed, precision, MT.LONG_HOP, L, maxD, N)
    shape, seed, L, maxD, N = SC.PRIME_SHAPE
    return MelSetup(shape, seed, precision, (12, 4), L, maxD, N)


@pytest.mark.parametrize("long", [False, True], ids=["prime_shape", "long_schedule"])
@pytest.mark.parametrize("precision", [16, 32])
def test_scores_from_mel_equal_the_scores_of_the_lockstep_features(precision, long):
    """scoreSamplesMel against scoreSamples fed the lockstep-upsampled features as a T_data tensor: logp and rows bit for bit, at
    T = 1 and 0.5, n = 1, 16, 17, 47 (300 on the long schedule), alone and among other requests; and within 2 delta / T
    (score_cases.bar) of the float64 teacher-forced reference fed those same features."""
    ms = _score_setup(precision, long)
    x = ms.lock()                                              # [columns][n_cond][N], T_data
    e = ms.engine()
    lengths = (SC.LONG_N,) if long else MT.SCORE_LENGTHS
    worst = 0.0
    for T in (1.0, 0.5):
        reqs = [(ms.yg[i % ms.columns, :n].contiguous(), i % ms.columns, T) for i, n in enumerate(lengths)]
        together = e.scoreSamplesMel([(y, ms.melg[c], T) for y, c, T in reqs], rows=True)
        want = e.scoreSamples([(y, x[c], T) for y, c, T in reqs], rows=True)
        for (y, c, _), (lp, rw), (wlp, wrw) in zip(reqs, together, want):
            n = y.numel()
            assert torch.equal(_bits(lp), _bits(wlp)) and torch.equal(_bits(rw), _bits(wrw)), "n = %d, T = %g: differs from scoreSamples" % (n, T)
            alone = e.scoreSamplesMel([(y, ms.melg[c], T)])[0]
            assert torch.equal(_bits(alone), _bits(lp)), "n = %d, T = %g: alone differs from among others" % (n, T)
            Za, ref = SC.reference(ms.t, ms.s, ms.y[c, :n], SC.lh_of(x[c].double().cpu().numpy(), ms.w, ms.b, ms.s.R, ms.s.L), T)
            bar = SC.bar(Za, T, precision)
            err = np.abs(lp.cpu().numpy().astype(np.float64) - ref)
            rerr = np.abs(rw.cpu().numpy().astype(np.float64) - SC.log_softmax(Za, T))
            worst = max(worst, float(err.max() / bar), float(rerr.max() / bar))
            assert (err <= bar).all() and (rerr <= bar).all(), "n = %d, T = %g: %.3g against a bar of %.3g" % (n, T, max(err.max(), rerr.max()), bar)
    print("scores from mel fp%d %s: at most %.3f of the bar" % (precision, "long" if long else "prime shape", worst))
    e.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_return_0_and_write_nothing():
    ms = MelSetup(PRIME_SHAPE, 961, 16, (12, 4))
    e = ms.engine()
    row, N, stride = e.upsampleRowElems(), ms.s.N, ms.stride
    frames = N // stride
    mel, host_mel = ms.melg[0], ms.melg[0].cpu()
    dst = torch.full((4096,), 0xAB, dtype=torch.uint8, device="cuda")
    host_dst = torch.full((4096,), 0xAB, dtype=torch.uint8).pin_memory()

    def up(mel=mel, bits=16 if mel.dtype == torch.float16 else 32, sc=None, sf=None, frames=frames, first=0, count=8, dst_ptr=None, n=1, eng=e):
        r = np.zeros(2, dtype=UPSAMPLE_REQ)
        r[:] = (mel.data_ptr(), bits, mel.stride(0) if sc is None else sc, mel.stride(1) if sf is None else sf, frames, first, count,
                dst.data_ptr() if dst_ptr is None else dst_ptr)
        r[1]["dst"] += 2048
        return lib.nvw_upsample_requests(eng._h, r.ctypes.data, n, None)

    bare = _engine(ms.case, ms.t, 16, "wg", ms.w, ms.b, 3)                        # no setUpsampling
    assert bare.upsampleRowElems() == 0 and up(eng=bare) == 0
    assert up(mel=host_mel) == 0                                                   # mel not in device memory
    assert up(bits=8) == 0 and up(sc=0) == 0 and up(sf=-1) == 0                    # precision, strides
    assert up(frames=1, first=0, count=stride + 1) == 0                            # frames * stride short of the range
    assert up(first=N - 4, count=8) == 0 and up(first=-1) == 0 and up(count=0) == 0
    assert up(dst_ptr=dst.data_ptr() + 8) == 0 and up(dst_ptr=host_dst.data_ptr()) == 0 and up(dst_ptr=0) == 0
    assert up(n=0) == 0 and up(n=-1) == 0
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all()) and bool((host_dst == 0xAB).all())
    assert up(n=2) == 2                                                            # ... and the call they all vary
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[8 * row * 2:2048] == 0xAB).all() and np.array_equal(out[:8 * row * 2], out[2048:2048 + 8 * row * 2])

    # the two passes: everything above that reaches them, and what the feature entries refuse
    y = ms.yg[0, :17].contiguous()
    nbytes = e.slotStateBytes()
    blob = torch.full((2, nbytes + 16), 0xAB, dtype=torch.uint8, device="cuda")
    logp = torch.full((32,), float("nan"), device="cuda")

    def pre(mel=mel, y=y, n=17, bits=16 if mel.dtype == torch.float16 else 32, sf=None, frames=frames, T=1.0, dst_ptr=None, eng=e, count=1):
        r = np.zeros(1, dtype=PREFILL_MEL_REQ)
        r[0] = (y.data_ptr(), n, mel.data_ptr(), bits, mel.stride(0), mel.stride(1) if sf is None else sf, frames, 5, T)
        return lib.nvw_prefill_states_mel(eng._h, r.ctypes.data, count, blob.data_ptr() if dst_ptr is None else dst_ptr, blob.stride(0), None)

    def score(mel=mel, y=y, n=17, bits=16 if mel.dtype == torch.float16 else 32, sf=None, frames=frames, T=1.0, lp=None, eng=e, count=1):
        r = np.zeros(1, dtype=SCORE_MEL_REQ)
        r[0] = (y.data_ptr(), n, mel.data_ptr(), bits, mel.stride(0), mel.stride(1) if sf is None else sf, frames, T, logp.data_ptr() if lp is None else lp, 0)
        return lib.nvw_score_samples_mel(eng._h, r.ctypes.data, count, None)

    for call in (pre, score):
        assert call(eng=bare) == 0 and call(mel=host_mel) == 0 and call(bits=8) == 0 and call(sf=0) == 0
        assert call(frames=4, n=17) == 0                                           # 4 frames x 4 < 17
        assert call(n=0) == 0 and call(T=0.0) == 0 and call(T=float("nan")) == 0 and call(y=ms.yg[0, :17].cpu()) == 0
        assert call(count=0) == 0
    assert pre(dst_ptr=blob.data_ptr() + 8) == 0 and score(lp=0) == 0
    torch.cuda.synchronize()
    assert bool((blob == 0xAB).all()) and bool(torch.isnan(logp).all())
    assert pre() == 1 and score() == 1
    torch.cuda.synchronize()
    assert not bool((blob[0, :nbytes] == 0xAB).all()) and bool((blob[0, nbytes:] == 0xAB).all()) and bool((blob[1] == 0xAB).all())
    assert bool(torch.isfinite(logp[:17]).all()) and bool(torch.isnan(logp[17:]).all())
    with pytest.raises(ValueError):
        e.prefillStatesMel([(y, mel, 5, 1.0, 4)])
    with pytest.raises(ValueError):
        e.scoreSamplesMel([(y, mel, 1.0, 4)])
    with pytest.raises(ValueError):
        bare.upsampleRequests([(mel, 0, 8)])
    bare.close()
    e.close()


# ---- 7. the scheduler -----------------------------------------------------------------------------------------------------------

def test_streams_deliver_from_sample_n_on_what_a_forced_mel_prime_delivers():
    """SlotStream.submit_mel(prime=, prefill=True) against prefill=False on a second engine: delivery starts at n and the samples
    from n on are equal; one request is streamed with extend_mel after submission; a prefill_mel state survives to_bytes /
    from_bytes and resumes; the three ValueError cases leave waiting() and the uid counter as they were."""
    ms = MelSetup(PRIME_SHAPE, 961, 16, (12, 4), columns=8)
    N, stride = ms.s.N, ms.stride
    frames = N // stride
    e, e2 = ms.engine(), ms.engine()
    st, st2 = SlotStream(e, ms.s.maxD, pcm=False), SlotStream(e2, ms.s.maxD, pcm=False)
    todo = list(zip(range(1, 7), (1, 2, 16, 17, 40, 47)))
    prime = lambda u, n: torch.from_numpy(ms.y[u, :n].copy())
    streamed = todo[3]
    hs = {st.submit_mel(ms.melg[u], uid=u, prime=prime(u, n), prefill=True): (u, n) for u, n in todo if (u, n) != streamed}
    hs2 = {st2.submit_mel(ms.melg[u], uid=u, prime=prime(u, n)): (u, n) for u, n in todo}
    u, n = streamed                                                               # streamed: the frames that cover the prime, the rest later
    part = -(-n // stride)
    assert part < frames
    late = st.submit_mel(ms.melg[u], uid=u, frames=part, final=False, prime=prime(u, n), prefill=True)
    hs[late] = (u, n)
    waiting, next_uid = st.waiting(), st._next_uid
    with pytest.raises(ValueError):
        st.submit_mel(ms.melg[7], uid=70, frames=1, final=False, prime=prime(7, stride + 1), prefill=True)      # frames do not cover the prime
    with pytest.raises(ValueError):
        st.submit_mel(ms.melg[7], uid=71, prime=prime(7, N), prefill=True)                                      # nothing left to generate
    bare = _engine(ms.case, ms.t, 16, "wg", ms.w, ms.b, 2)
    stb = SlotStream(bare, ms.s.maxD, pcm=False)
    with pytest.raises(ValueError):
        stb.submit_mel(ms.melg[7], uid=72, prime=prime(7, 4), prefill=True)                                     # no upsampling table
    assert stb.waiting() == 0 and stb._next_uid == 0
    stb.close()
    bare.close()
    assert st.waiting() == waiting and st._next_uid == next_uid
    state = st.prefill_mel(ms.melg[7], prime(7, 31), uid=7)
    assert state.kind == "mel" and state.done == 31 and state.uid == 7 and state.frames == frames and state.final is True
    back = SlotState.from_bytes(state.to_bytes(), ms.melg[7])
    assert back.kind == "mel" and back.done == 31 and back.frames == frames and back.final and np.array_equal(back.blob.numpy(), state.blob.cpu().numpy())
    hs[st.resume_many([back])[0]] = (7, 31)
    hs2[st2.submit_mel(ms.melg[7], uid=7, prime=prime(7, 31))] = (7, 31)
    got, got2 = {h: [] for h in hs}, {h: [] for h in hs2}
    steps = 0
    for stream, sink in ((st, got), (st2, got2)):
        while stream.busy():
            for h, (y, _) in stream.step(7).items():
                sink[h].append(y)
            stream.finished()
            steps += 1
            if stream is st and steps == 2:
                st.extend_mel(late, frames, final=True)
            assert steps < 200
    by_uid2 = {hs2[h][0]: np.concatenate(got2[h]) for h in hs2}
    for h, (u, n) in hs.items():
        g = np.concatenate(got[h]) if got[h] else np.zeros(0, dtype=np.int32)
        full = by_uid2[u]
        assert len(full) == N and np.array_equal(full[:n], ms.y[u, :n])
        assert len(g) == N - n, "utterance %d: %d samples delivered, %d follow its prime" % (u, len(g), N - n)
        assert np.array_equal(g, full[n:]), "utterance %d: the samples from %d on differ from the forced prime's" % (u, n)
    st.close()
    st2.close()
    e.close()
    e2.close()
