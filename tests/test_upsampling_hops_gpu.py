"""GPU tests of the mel upsampling at the hop sizes that ship (`-m gpu`): window 1024 / stride 256 (bench.py's
end-to-end configuration), the reference model's 800 / 200, an odd stride at the largest tap count (1375 / 275) and a stride
above the phase grid (1100 / 1100).  At these sizes a slot step lies inside one frame or straddles one edge, a lockstep range
cuts frames, the phase grid takes its shipped shape and -- at 1100 -- makes a second pass.

(1) upsample_features_kernel against a float64 transposed convolution of the same tensors, under bars derived from the number
formats; (2) ranges that cut frames, and generate_stream over them, bit for bit against the single call; (3) the slot-mode feed
(slot_mel_stage / upsample / place kernels), row by row, against the lockstep rows; (4) frames streamed one at a time, the
headroom held to the frames delivered; (5) staggered joins against the lockstep samples.  The network is the smallest there is
(the C1 shape of tests/cases.py): the upsampling does not depend on it."""
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import condgen
import util
from nv_wavenet_amd._lib import lib
from oracle import oracle as O
from test_slots_gpu import _check_prefixes
from test_slots_mel_gpu import _frag_cols, _half, _mel_engine, _mel_plan, _mel_run

pytestmark = pytest.mark.gpu

C1 = cases.BY_NAME["C1_R32S128A256_L8_B1"]
Hop = namedtuple("Hop", "cc frames")
HOPS = [Hop(condgen.CondCase("hop256", 541, C1.name, 80, 1024, 256), 3),          # the shipped end-to-end configuration
        Hop(condgen.CondCase("hop200", 542, C1.name, 37, 800, 200), 3),           # the reference's model; fewer channels than 80
        Hop(condgen.CondCase("hop275_m5", 543, C1.name, 80, 1375, 275), 3),       # odd stride, five taps: the largest LDS operand
        Hop(condgen.CondCase("hop1100_m1", 544, C1.name, 80, 1100, 1100), 2)]     # more phases than the grid; one tap
HOP = {h.cc.name: h for h in HOPS}
NAMES = [h.cc.name for h in HOPS]
B = 21          # a full tile and a ragged one


def _inputs(name, precision, batch):
    """(case, model tensors, mel [batch][n_cond][frames], upsample weight, cond weight) as an engine of `precision` holds them
    (condgen.make_cond_model from the case's seed; fp16: rounded through fp16); the C1 network with `batch` utterances."""
    hop = HOP[name]
    case = C1._replace(shape=C1.shape._replace(B=batch, N=hop.frames * hop.cc.stride))
    m = condgen.make_cond_model(hop.cc, case.shape)
    rnd = _half if precision == 16 else (lambda a: a)
    return case, m, rnd(m["features"]), rnd(m["up_w"]), rnd(m["cond_w"][:, :, 0])


_nets = {}


def _net(precision):
    """The O(1) network of the C1 case (weights only are used: they do not depend on the batch or the length)."""
    if precision not in _nets:
        _nets[precision] = util.gen_o1(C1, half=precision == 16)
    return _nets[precision]


def _bits(a):
    """A feature fragment tensor as integers: equality of these is equality bit for bit."""
    return a.contiguous().view(torch.int16 if a.dtype == torch.float16 else torch.int32)


_lockstep_cache = {}


def _lockstep_features(name, precision):
    """What tests 1 and 2 share per hop case and precision, computed once: the fragments of ONE upsampleFeatures(0, N) call on a
    fresh engine (CPU tensor [N][tiles][KFC][4][16][EPL] of the engine's type), the float64 transposed convolution of the same
    tensors cut to frames x stride samples, and S = |b| + sum |w x| from one more convolution of the absolute values."""
    key = (name, precision)
    if key not in _lockstep_cache:
        cc = HOP[name].cc
        case, m, mel, up_w, w = _inputs(name, precision, B)
        N = case.shape.N
        e = _mel_engine(case, _net(precision), precision, "wg", w, m, up_w, cc.stride, B)
        e.setMel(torch.from_numpy(mel).cuda())
        e.upsampleFeatures(0, N)
        frags = e.getFeatures(0, N).cpu()
        tiles = e.condTiles()
        e.close()
        md, wd, bd = torch.from_numpy(mel).double(), torch.from_numpy(up_w).double(), torch.from_numpy(m["up_b"]).double()
        want = F.conv_transpose1d(md, wd, bd, stride=cc.stride)[..., :N].numpy()
        S = F.conv_transpose1d(md.abs(), wd.abs(), bd.abs(), stride=cc.stride)[..., :N].numpy()
        _lockstep_cache[key] = dict(case=case, m=m, mel=mel, up_w=up_w, w=w, frags=frags, tiles=tiles, want=want, S=S)
    return _lockstep_cache[key]


def _ulp16(x):
    """Spacing of fp16 in the binade of |x| (float64 in, float64 out); 2^-24 below the smallest normal."""
    e = np.frexp(np.maximum(np.abs(x), 2.0 ** -14))[1] - 1
    return 2.0 ** (e - 10).astype(np.float64)


# ---- 1. the lockstep kernel against the float64 convolution -----------------------------------------------------------------

@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("name", NAMES)
def test_lockstep_upsampling_against_the_float64_transposed_convolution(name, precision):
    """setUpsampling + setMel + upsampleFeatures(0, N) + getFeatures, unpacked to [b][c][n] as test_features_in_samples_out does,
    against F.conv_transpose1d in float64.  Channels >= n_cond are exactly zero.  Bars per element, from the formats: a K-term fp32
    sum (K = taps x n_cond) of terms whose absolute values sum to S errs by at most K 2^-24 S; twice that, because the order of
    the MFMA's internal summation is not specified.  fp16: that sum is rounded once more, to fp16, which can land on the
    neighbour of fp16(want): one more unit in the last place of want.  Four taps, fp16: 98 % of the values are fp16(want)
    exactly, the bar test_features_in_samples_out holds at the same K = 320 and the same magnitudes."""
    L = _lockstep_features(name, precision)
    cc, N, half = HOP[name].cc, L["case"].shape.N, precision == 16
    taps = cc.window // cc.stride
    TPF = 2 if half else 1
    fr = L["frags"].float().numpy().reshape(N, L["tiles"], -1, 4, 16, TPF, 4)                     # [n][tile][kf][g][j][tk][r]
    xall = fr.transpose(1, 4, 2, 5, 3, 6, 0).reshape(L["tiles"] * 16, -1, N)                     # [b][c][n]
    assert xall.shape[1] >= 80
    assert not xall[:, cc.n_cond:].any(), "channels beyond n_cond must be zero"
    xe = xall[:B, :cc.n_cond].astype(np.float64)          # (utterances beyond the batch hold the bias: never read)
    want, S = L["want"], L["S"]
    assert want.shape == xe.shape == S.shape
    K = taps * cc.n_cond
    bar = 2.0 * K * 2.0 ** -24 * S
    if half:
        bar = bar + _ulp16(want)
        want = want.astype(np.float16).astype(np.float64)
    d = np.abs(xe - want)
    worst = float((d / bar).max())
    exact = float((d == 0).mean())
    print("upsampling %s fp%d: largest error %.4f of the bar (K = %d, %d values, %.4f of them exact)" % (name, precision, worst, K, d.size, exact))
    assert np.isfinite(xe).all()
    assert (d <= bar).all(), "%s fp%d: %d values beyond the bar, the worst at %.3f of it" % (name, precision, int((d > bar).sum()), worst)
    if half and taps == 4:
        assert exact >= 0.98, exact


# ---- 2. ranges that cut frames ----------------------------------------------------------------------------------------------

EDGES = {"hop256": (0, 1, 255, 257, 600), "hop200": (0, 1, 199, 201, 470)}


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_ranges_that_cut_frames_write_their_rows_and_no_others(name, precision):
    """upsampleFeatures in pieces whose edges are no multiples of the stride (one sample; up to one before a frame edge; across
    it; the rest), on a fresh engine whose feature buffer starts zeroed: after every piece the rows written so far are those of
    the single upsampleFeatures(0, N) call, bit for bit, and every row from the piece's end on is still zero."""
    L = _lockstep_features(name, precision)
    cc, N = HOP[name].cc, L["case"].shape.N
    full = _bits(L["frags"])
    e = _mel_engine(L["case"], _net(precision), precision, "wg", L["w"], L["m"], L["up_w"], cc.stride, B)
    e.setMel(torch.from_numpy(L["mel"]).cuda())
    edges = EDGES[name] + (N,)
    assert all(a % cc.stride for a in edges[1:-1]) and edges[2] == cc.stride - 1 and edges[3] == cc.stride + 1
    for a, b in zip(edges[:-1], edges[1:]):
        e.upsampleFeatures(a, b - a)
        got = _bits(e.getFeatures(0, N).cpu())
        bad = (got[:b] != full[:b]).flatten(1).any(1).nonzero().flatten()
        assert bad.numel() == 0, "after [%d, %d): rows %s... differ from the single call's" % (a, b, bad[:5].tolist())
        late = (got[b:] != 0).flatten(1).any(1).nonzero().flatten()
        assert late.numel() == 0, "after [%d, %d): rows %s... beyond the piece were written" % (a, b, (late[:5] + b).tolist())
    e.close()


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_streamed_chunks_that_cut_frames_give_the_samples_of_one_launch(name, precision):
    """generate_stream with a chunk that is neither a divisor nor a multiple of the stride leaves the fragments of the single
    upsampleFeatures call in the engine's buffer and gives, bit for bit, the samples of one launch over those very fragments
    handed back with setConditioningFeatures (test 1 holds the fragments; such a launch is held to the oracle, at small
    strides, by test_features_in_samples_out)."""
    L = _lockstep_features(name, precision)
    cc, s = HOP[name].cc, L["case"].shape
    chunk = 333
    assert chunk % cc.stride and cc.stride % chunk and s.N % chunk
    e = _mel_engine(L["case"], _net(precision), precision, "wg", L["w"], L["m"], L["up_w"], cc.stride, B)
    e.setMel(torch.from_numpy(L["mel"]).cuda())
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    seen = []
    assert e.generate_stream(chunk, lambda yo, first, count: seen.append((first, count)), s.N, s.B, y)
    e.synchronize()
    assert seen == [(f, min(chunk, s.N - f)) for f in range(0, s.N, chunk)]
    assert torch.equal(_bits(e.getFeatures(0, s.N).cpu()), _bits(L["frags"])), "chunked upsampling differs from the single call"
    frags = L["frags"].cuda()
    e.setConditioningFeatures(frags)
    y1 = np.full((s.B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, s.B, y1, 1, False)
    e.synchronize()
    assert y1.min() >= 0 and len(np.unique(y1)) > 16          # (a generation, not a constant)
    assert np.array_equal(y, y1), "streamed samples differ from one launch over the same features"
    e.close()


# ---- 3. the slot-mode feed, row by row ----------------------------------------------------------------------------------------

_feed_cache = {}
N_REF = 24          # utterances of the lockstep engine the rows come from


def _feed_reference(name, precision):
    """Per hop case and precision, computed once: mel frames (exact in fp16, so that fp16 views hold the same values) and
    upsampled features of N_REF utterances, and the lockstep engine's rows of both per utterance ([32][N][lane bytes])."""
    key = (name, precision)
    if key not in _feed_cache:
        if len(_feed_cache) >= 2:          # (the rows of the long hops take tens of MiB)
            _feed_cache.pop(next(iter(_feed_cache)))
        hop = HOP[name]
        cc = hop.cc
        case, m, _, up_w, w = _inputs(name, precision, N_REF)
        s = case.shape
        rng = np.random.default_rng(cc.seed)
        rnd = _half if precision == 16 else (lambda a: a)
        mel = _half(rng.standard_normal((s.B, cc.n_cond, hop.frames)).astype(np.float32))
        feat = rnd(rng.standard_normal((s.B, cc.n_cond, s.N)).astype(np.float32))
        ref = _mel_engine(case, _net(precision), precision, "wg", w, m, up_w, cc.stride, s.B)
        ref.setMel(torch.from_numpy(mel).cuda())
        ref.upsampleFeatures(0, s.N)
        want_mel = _frag_cols(ref.getFeatures(0, s.N), ref.condTiles())
        ref.setFeatures(torch.from_numpy(feat).cuda())
        want_feat = _frag_cols(ref.getFeatures(0, s.N), ref.condTiles())
        ref.close()
        assert np.abs(want_mel[:s.B]).max() > 0.5
        _feed_cache[key] = dict(case=case, m=m, up_w=up_w, w=w, mel=mel, feat=feat, want_mel=want_mel, want_feat=want_feat)
    return _feed_cache[key]


def _feed_steps(stride, N, cycle, joins):
    """The steps of the feed test: [(samples, index of the join that follows it or None)].  Step sizes cycle through `cycle`; a
    step that would pass the next join's counter -- the first one >= its earliest counter with its residue of the stride -- ends
    there instead.  Runs until every column that joined last has passed its utterance's end."""
    out, counter, k, last = [], 0, 0, None
    while k < len(joins) or counter < last + N + 1:
        c, target = cycle[len(out) % len(cycle)], None
        if k < len(joins):
            res, lo = joins[k]
            first = max(lo, counter + 1)
            target = first + (res - first) % stride
            c = min(c, target - counter)
        counter += c
        out.append((c, k if counter == target else None))
        if counter == target:
            k, last = k + 1, counter
    return out


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("window", ["W64", "W2hops"])
@pytest.mark.parametrize("name", NAMES)
def test_slot_feed_rows_equal_the_lockstep_rows_at_real_hops(name, window, precision):
    """40 columns, 30 started at once and more joining at counters = 1, stride - 1 and another residue of the stride (one into
    a column stopped before); fp32 and fp16 mel, [n_cond][frames] and channels-last views, every third column a feature column.
    After every step the window's rows of every owned column equal, bit for bit, the lockstep rows of its uid; the rows past a
    mel utterance's end (it ends inside a step) hold the zeros the feed writes into an idle lane.
    W64: a window smaller than a frame, steps of 1, 7, 63 and 64 -- every step inside one frame or across one edge.
    W2hops: the smallest window >= 2 stride + 2, steps of 1, stride - 1, stride, stride + 1, 2 stride + 1 (three frames), 3 and
    stride - 2, so that steps start and end at every alignment to a frame edge."""
    R = _feed_reference(name, precision)
    cc, case = HOP[name].cc, R["case"]
    s, stride = case.shape, HOP[name].cc.stride
    want_mel, want_feat = R["want_mel"], R["want_feat"]
    if window == "W64":
        W, cycle, earliest = 2 * max(32, s.maxD), (1, 7, 64, 63, 1, 64), (0, stride // 2, stride + stride // 4)
        assert W < stride
    else:
        W = -(-(2 * stride + 2) // s.maxD) * s.maxD
        cycle, earliest = (1, stride - 1, stride, stride + 1, 2 * stride + 1, 3, stride - 2), (0, 2 * stride, 5 * stride + 1)
        assert max(cycle) <= W
    columns = 40
    rng = np.random.default_rng(cc.seed + precision)
    e = _mel_engine(case, _net(precision), precision, "wg", R["w"], R["m"], R["up_w"], stride, columns)
    e.slotsBegin(W)
    melg = torch.from_numpy(R["mel"]).cuda()
    views = [melg[u] if u % 4 == 0 else melg[u].half() if u % 4 == 1 else melg[u].t().contiguous().t() if u % 4 == 2
             else melg[u].half().t().contiguous().t() for u in range(s.B)]
    assert views[2].stride(0) == 1 and views[3].dtype == torch.float16
    featg = torch.from_numpy(R["feat"]).cuda()
    owner = {}                  # column -> (kind, uid, counter at its local sample 0)
    order = [int(c) for c in rng.permutation(columns)]
    for i, col in enumerate(order[:30]):
        u = i % s.B
        if i % 3 == 2:
            e.slotStart(col, featg[u], u)
            owner[col] = ("feat", u, 0)
        else:
            e.slotStartMel(col, views[u], u)
            owner[col] = ("mel", u, 0)
    assert owner[order[0]][0] == "mel"
    # joins: (residue of the counter, earliest counter, columns, column to stop); the last one goes into the stopped column
    joins = [(1, earliest[0], order[30:32], order[0]), (stride - 1, earliest[1], order[32:35], None),
             (stride // 2 + 3, earliest[2], [order[0], order[35]], None)]
    counter, ended_inside, joined = 0, 0, 0
    steps = _feed_steps(stride, s.N, cycle, [(j[0], j[1]) for j in joins])
    for step, (c, join) in enumerate(steps):
        assert e.slotsStep(c)
        got = _frag_cols(e.slotsGetFeatures(counter, c), e.condTiles())
        for col, (kind, u, s0) in owner.items():
            k0 = counter - s0
            want = (want_mel if kind == "mel" else want_feat)[u, k0:k0 + c]
            n = want.shape[0]
            assert np.array_equal(got[col, :n], want), "%s column %d (uid %d), step %d of %d samples at counter %d: rows differ from the lockstep %s" % (
                kind, col, u, step, c, counter, "upsampling" if kind == "mel" else "packing")
            if kind == "mel" and n < c:
                assert not got[col, n:].any(), "mel column %d (uid %d), step %d: rows past its end were written" % (col, u, step)
                ended_inside += n > 0
        counter += c
        if join is not None:
            res, _, cols, stop = joins[join]
            assert counter % stride == res and res % stride != 0
            if stop is not None:
                e.slotStop(stop)
                owner.pop(stop)
            for i, col in enumerate(cols):
                u = (5 * (i + joined) + 3) % s.B
                assert col not in owner
                e.slotStartMel(col, views[u], u)
                owner[col] = ("mel", u, counter)
            joined += len(cols)
    longest = max(c for c, _ in steps)
    assert ended_inside >= 3, "no mel utterance ended inside a step"
    assert counter > 2 * W and counter > 2 * stride
    assert longest == (2 * stride + 1 if window == "W2hops" else 64)
    with pytest.raises(ValueError):
        e.slotsGetFeatures(counter - W - 1, 2)          # (older than the window)
    e.slotsEnd()
    e.close()


# ---- 4. streamed frames, 5. staggered joins: against the lockstep samples -------------------------------------------------------

def _lockstep_samples(name, precision, mode, batch, chunk=333):
    """(inputs, y [batch][N], pcm [batch][N]) of the lockstep mel path: setMel + generate_stream, in-kernel selectors."""
    cc = HOP[name].cc
    case, m, mel, up_w, w = _inputs(name, precision, batch)
    s = case.shape
    e = _mel_engine(case, _net(precision), precision, mode, w, m, up_w, cc.stride, s.B)
    e.setMel(torch.from_numpy(mel).cuda())
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    pcm = torch.zeros(s.B, s.N, dtype=torch.int16, device="cuda")
    e.setAudioOut(pcm)
    assert e.generate_stream(chunk, None, s.N, s.B, y)
    e.synchronize()
    e.setAudioOut(None)
    e.close()
    pcm = pcm.cpu().numpy()
    assert np.array_equal(pcm, O.mulaw_pcm_table(s.A)[y])
    return (case, m, mel, up_w, w), y, pcm


@pytest.mark.parametrize("precision", [16, 32])
def test_frames_streamed_one_at_a_time_at_hop256(precision):
    """Ten utterances of three frames whose frames arrive one at a time -- sometimes none, sometimes two -- between steps, `final`
    late, NaN in the frames not yet delivered.  Before every step the headroom is what the frames delivered give: the least,
    over the columns that are not final, of frames x stride - local position (the window otherwise); a step of one more is
    refused and changes nothing.  No NaN reaches a feature row, and every utterance's samples are its lockstep column's."""
    name, n_utt, W = "hop256", 10, 512
    stride, frames = HOP[name].cc.stride, HOP[name].frames
    (case, m, mel, up_w, w), y_lock, _ = _lockstep_samples(name, precision, "wg", n_utt)
    N = case.shape.N
    e = _mel_engine(case, _net(precision), precision, "wg", w, m, up_w, stride, n_utt)
    e.slotsBegin(W)
    melg = torch.from_numpy(mel).cuda()
    rng = np.random.default_rng(9 + precision)
    later = [(1, 7), (100, 8), (300, 9)]          # (earliest counter, column = uid) of those that join a running session
    sizes = (1, 7, 64, 200, 255, 3, 300, 64)
    bufs, have, final, pos, ys = {}, {}, {}, {}, {u: [] for u in range(n_utt)}
    counter, step, refused, short, done, join_counters = 0, 0, 0, 0, set(), []
    while len(done) < n_utt:
        joining = list(range(7)) if step == 0 else []
        if later and counter >= later[0][0] and counter % stride not in [j % stride for j in join_counters]:
            joining.append(later.pop(0)[1])          # (at a counter that is no multiple of the stride, each at another residue)
        for col in joining:
            a0 = int(rng.integers(0, 3))
            bufs[col] = torch.full_like(melg[col], float("nan"))          # frames not yet delivered: NaN, never to be read
            bufs[col][:, :a0] = melg[col][:, :a0]
            e.slotStartMel(col, bufs[col], col, frames=a0, final=False)
            have[col], final[col], pos[col] = a0, False, 0
            join_counters.append(counter)
        want_h = min([W] + [have[c] * stride - pos[c] for c in pos if not final[c]])
        h = e.slotsHeadroom()
        assert h == want_h, "step %d: headroom %d, the frames delivered give %d" % (step, h, want_h)
        if h < W:
            y0 = np.full((n_utt, h + 1), -7, dtype=np.int32)
            assert not lib.nvw_slots_step(e._h, h + 1, y0.ctypes.data, None, None), "a step above the headroom"
            assert (y0 == -7).all() and e.slotsHeadroom() == h
            refused += 1
        c = sizes[step % len(sizes)]
        k = min(c, h)
        short += k < c
        if k > 0:
            y = np.full((n_utt, k), -1, dtype=np.int32)
            assert e.slotsStep(k, y)
            assert not torch.isnan(e.slotsGetFeatures(counter, k)).any(), "step %d: NaN in a feature row" % step
            counter += k
            for col in list(pos):
                kk = min(k, N - pos[col])
                ys[col].append(y[col, :kk])
                pos[col] += kk
                if pos[col] == N:
                    e.slotStop(col)
                    done.add(col)
                    del pos[col]
        for col in pos:          # the producer: 0, 1 or 2 frames more; `final` with the last frame or later
            if final[col]:
                continue
            new = min(frames, have[col] + int(rng.choice([0, 1, 1, 2])))
            bufs[col][:, have[col]:new] = melg[col][:, have[col]:new]
            have[col] = new
            final[col] = bool(new == frames and rng.random() < 0.5)
            e.slotMelFrames(col, new, final[col])
        step += 1
        assert step < 2000
    assert refused > 0 and short > 0 and len({c % stride for c in join_counters}) == 4
    e.slotsEnd()
    e.close()
    for u in range(n_utt):
        got = np.concatenate(ys[u])
        assert got.shape == (N,)
        bad = np.nonzero(got != y_lock[u])[0]
        assert bad.size == 0, "utterance %d differs from its lockstep run first at sample %d" % (u, bad[0])


@pytest.mark.parametrize("name,precision,mode", [("hop256", 16, "wg"), ("hop256", 16, "wg3"), ("hop200", 32, "wg")])
def test_staggered_mel_joins_at_real_hops_give_the_lockstep_samples(name, precision, mode):
    """30 utterances of two and three frames through 24 columns with a window of 512 samples, joining at counters that are no
    multiples of the stride, in steps from 1 to 300 samples: every utterance's samples and PCM are the prefix of its lockstep
    column's (setMel + generate_stream of the same seed)."""
    n_utt, columns, W = 30, 24, 512
    stride = HOP[name].cc.stride
    (case, m, mel, up_w, w), y_lock, pcm_lock = _lockstep_samples(name, precision, mode, n_utt)
    s = case.shape
    plan, counts = _mel_plan(n_utt, columns, s.N, stride, 25, sizes=(7, 1, 64, 255, 300, 1, 257, 64))
    at = np.concatenate([[0], np.cumsum(counts)])
    assert sum(at[p[0]] % stride != 0 for p in plan) >= 10 and {p[3] for p in plan} == {2 * stride, 3 * stride}
    assert 16 <= len({p[1] for p in plan}) < len(plan) == n_utt and sum(counts) > 3 * W          # (columns are reused)
    e = _mel_engine(case, _net(precision), precision, mode, w, m, up_w, stride, columns)
    if mode == "wg3":
        assert "BT=3" in e.kernelInfo(), e.kernelInfo()
    got, pcm = _mel_run(e, torch.from_numpy(mel).cuda(), plan, counts, W, stride)
    e.close()
    _check_prefixes(got, y_lock, plan, "%s fp%d %s" % (name, precision, mode))
    _check_prefixes(pcm, pcm_lock, plan, "PCM %s fp%d %s" % (name, precision, mode))
