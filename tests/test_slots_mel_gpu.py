"""GPU tests of slot mode from mel frames (`-m gpu`): a column holds an utterance as frames before upsampling, handed
over whole or piece by piece while it runs, and its samples are bit for bit those of its column uid of a lockstep nvw_set_mel +
nvw_generate_stream run with the same seed -- whatever the column, the join step, the step sizes, the window wraps, the neighbours
(feature or mel columns) and however its frames arrived.  The feed is also checked alone, row by row, against the lockstep
upsampling of the same frames."""
import numpy as np
import pytest
import torch

import cases
import condgen
import util
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.slots import SlotStream
from oracle import oracle as O
from test_features_gpu import _cond_inputs
from test_slots_gpu import SEED, WINDOW, _check_prefixes, _engine, _lockstep

pytestmark = pytest.mark.gpu

COUNTS = (7, 1, 64, 7, 1, 7, 64, 1, 7)


def _half(a):
    return a.astype(np.float16).astype(np.float32)


def _mel_inputs(cc, precision):
    """(case, model tensors, mel [B][n_cond][frames], upsample weight, cond weight, O(1) network) as an engine of `precision` holds
    them (fp16: rounded through fp16)."""
    case = cases.BY_NAME[cc.case_name]
    m = condgen.make_cond_model(cc, case.shape)
    rnd = _half if precision == 16 else (lambda a: a)
    return case, m, rnd(m["features"]), rnd(m["up_w"]), rnd(m["cond_w"][:, :, 0]), util.gen_o1(case, half=precision == 16)


def _mel_engine(case, t, precision, mode, w, m, up_w, stride, columns):
    e = _engine(case, t, precision, mode, w, m["cond_b"], columns)
    e.setUpsampling(up_w, m["up_b"], stride)
    return e


def _mel_lockstep(case, t, precision, mode, mel, w, m, up_w, stride, chunk=None):
    """y [B][N] of the lockstep mel path: nvw_set_mel + nvw_generate_stream with in-kernel selectors of SEED."""
    s = case.shape
    e = _mel_engine(case, t, precision, mode, w, m, up_w, stride, s.B)
    e.setMel(torch.from_numpy(mel).cuda())
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    assert e.generate_stream(chunk or 3 * stride + 1, None, s.N, s.B, y)
    e.synchronize()
    e.close()
    return y


def _mel_plan(n_utt, columns, N, stride, seed, sizes=COUNTS):
    """_plan of test_slots_gpu with lengths that are multiples of the stride (a mel utterance is frames x stride samples long)."""
    rng = np.random.default_rng(seed)
    lengths = [N if i % 3 == 0 else stride * int(rng.integers(2, N // stride)) for i in range(n_utt)]
    queue = [int(u) for u in rng.permutation(n_utt)]
    free, running, plan, counts, step = list(range(columns)), {}, [], [], 0
    while queue or running:
        if queue and free and (not running or rng.random() < 0.6):
            col = free.pop(int(rng.integers(len(free))))
            uid = queue.pop(0)
            plan.append((step, col, uid, lengths[uid]))
            running[col] = lengths[uid]
        c = sizes[step % len(sizes)]
        counts.append(c)
        for col in list(running):
            running[col] -= min(c, running[col])
            if running[col] == 0:
                del running[col]
                free.append(col)
        step += 1
    return plan, counts


def _mel_run(e, melg, plan, counts, window, stride, feats=None, stream_rng=None, refusals=False):
    """Drives the engine through the schedule; returns {uid: samples}, {uid: pcm}.  melg[uid]: the utterance's mel [n_cond][frames];
    feats: {uid: features} of utterances that run as feature columns instead.  stream_rng: the frames are handed over in irregular
    pieces (0, 1, fewer than the taps, several) between steps and `final` comes late; a planned step then covers min(count,
    headroom) samples, and the plan's next step waits until it has run in full.  refusals: a step above the headroom and refused
    nvw_slot_mel_frames calls along the way, which must change nothing."""
    e.slotsBegin(window)
    ys, pcms, running, fed = {}, {}, {}, {}
    feats = feats or {}
    refused = 0

    bufs = {}

    def feed_more(col):
        uid, avail, final = running[col][0], fed[col][0], fed[col][1]
        total = bufs[col].size(1)
        if final:
            return
        piece = int(stream_rng.choice([0, 1, 2, 5, 9]))
        new = min(total, avail + piece)
        bufs[col][:, avail:new] = melg[uid][:, avail:new]      # (written on the stream the steps run on, before the next one)
        final = new == total and stream_rng.random() < 0.5
        e.slotMelFrames(col, new, final)
        fed[col] = [new, final]

    for step, c in enumerate(counts):
        for (s0, col, uid, n) in plan:
            if s0 == step:
                assert col not in running
                if uid in feats:
                    e.slotStart(col, feats[uid], uid, n)
                else:
                    mel = melg[uid][:, :n // stride]
                    if stream_rng is None:
                        e.slotStartMel(col, mel, uid)
                        fed[col] = [mel.size(1), True]
                    else:
                        a0 = min(int(stream_rng.choice([0, 1, 2, 3])), mel.size(1))
                        bufs[col] = torch.full_like(mel, float("nan"))          # frames not yet written: NaN, never to be read
                        bufs[col][:, :a0] = mel[:, :a0]
                        e.slotStartMel(col, bufs[col], uid, frames=a0, final=False)
                        fed[col] = [a0, False]
                running[col] = [uid, n]
                ys[uid], pcms[uid] = [], []
        done = 0
        while done < c:
            h = e.slotsHeadroom()
            if refusals and step % 3 == 1 and h < e.slotWindow:
                y0 = np.full((e.maxBatch, h + 1), -7, dtype=np.int32)
                assert not lib.nvw_slots_step(e._h, h + 1, y0.ctypes.data, None, None), "a step above the headroom"
                assert (y0 == -7).all() and e.slotsHeadroom() == h
                refused += 1
            k = min(c - done, h)
            if k == 0:
                for col in running:
                    if col in fed:
                        feed_more(col)
                continue
            y = np.full((e.maxBatch, k), -1, dtype=np.int32)
            pcm = np.zeros((e.maxBatch, k), dtype=np.int16)
            assert e.slotsStep(k, y, pcm)
            done += k
            for col in list(running):
                uid, left = running[col]
                kk = min(k, left)
                ys[uid].append(y[col, :kk])
                pcms[uid].append(pcm[col, :kk])
                running[col][1] -= kk
                if running[col][1] == 0:
                    del running[col]
                    fed.pop(col, None)
                    e.slotStop(col)
            if stream_rng is not None:
                for col in list(running):
                    if col in fed:
                        feed_more(col)
                        if refusals and fed[col][1] is False and stream_rng.random() < 0.3:
                            with pytest.raises(ValueError):
                                e.slotMelFrames(col, fed[col][0] - 1)          # fewer frames than before
            if refusals:
                assert not lib.nvw_slot_mel_frames(e._h, e.maxBatch, 1, 0)     # outside the batch
                idle = [b for b in range(e.maxBatch) if b not in running]
                if idle:
                    assert not lib.nvw_slot_mel_frames(e._h, idle[0], 10 ** 6, 0)      # not a mel column
                for col in running:
                    if col in fed and fed[col][1]:
                        assert not lib.nvw_slot_mel_frames(e._h, col, fed[col][0] + 1, 0)      # already final
                        break
                for col in running:
                    if col not in fed:
                        assert not lib.nvw_slot_mel_frames(e._h, col, 5, 0)      # a feature column
                        break
    assert not running
    if refusals:
        assert refused > 0
    e.slotsEnd()
    return {u: np.concatenate(v) for u, v in ys.items()}, {u: np.concatenate(v) for u, v in pcms.items()}


# ---- 1. the feed alone ---------------------------------------------------------------------------------------------------------

FEED_CASES = [condgen.COND_BY_NAME["cond_C3_B16"], condgen.COND_BY_NAME["cond_C3_B21_n37"], condgen.COND_BY_NAME["cond_C1_B1"],
              condgen.CondCase("taps1_C3", 531, "C3_R64S256A256_L20_B16", 80, 4, 4),
              condgen.CondCase("taps5_C3", 532, "C3_R64S256A256_L20_B16", 80, 10, 2)]


def _frag_cols(fr, tiles):
    """[n][tiles][kf][4][16][EPL] fragments -> [tiles*16][n][kf*4*EPL] per column (the column's lane bytes)."""
    a = fr.float().cpu().numpy()
    n = a.shape[0]
    return a.transpose(1, 4, 0, 2, 3, 5).reshape(tiles * 16, n, -1)


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("cc", FEED_CASES, ids=lambda c: c.name)
def test_mel_feed_rows_equal_the_lockstep_upsampling(cc, precision):
    """After mel-column steps of 1, 7 and 64 samples that wrap the window, the window's feature rows of the mel columns equal, bit
    for bit, nvw_get_features of a lockstep setMel + upsampleFeatures of the same frames; fp32 and fp16 sources, [n_cond][frames]
    and channels-last views; the feature columns that share their tiles keep their own features."""
    case = cases.BY_NAME[cc.case_name]
    s = case.shape._replace(B=24, N=192 - 192 % cc.stride)
    case = case._replace(shape=s)
    rng = np.random.default_rng(cc.seed)
    m = condgen.make_cond_model(cc, s)
    rnd = _half if precision == 16 else (lambda a: a)
    up_w, w = rnd(m["up_w"]), rnd(m["cond_w"][:, :, 0])
    frames = s.N // cc.stride
    mel = _half(rng.standard_normal((s.B, cc.n_cond, frames)).astype(np.float32))      # (exact in fp16 sources too)
    feat = rnd(rng.standard_normal((s.B, cc.n_cond, s.N)).astype(np.float32))
    t = util.gen_o1(case, half=precision == 16)
    W = 2 * max(32, s.maxD)
    ref = _mel_engine(case, t, precision, "wg", w, m, up_w, cc.stride, s.B)
    ref.setMel(torch.from_numpy(mel).cuda())
    ref.upsampleFeatures(0, s.N)
    want_mel = _frag_cols(ref.getFeatures(0, s.N), ref.condTiles())
    ref.setFeatures(torch.from_numpy(feat).cuda())
    want_feat = _frag_cols(ref.getFeatures(0, s.N), ref.condTiles())
    ref.close()
    columns = 40
    e = _mel_engine(case, t, precision, "wg", w, m, up_w, cc.stride, columns)
    e.slotsBegin(W)
    melg = torch.from_numpy(mel).cuda()
    views = [melg[u] if u % 4 == 0 else melg[u].half() if u % 4 == 1 else melg[u].t().contiguous().t() if u % 4 == 2
             else melg[u].half().t().contiguous().t() for u in range(s.B)]
    assert views[2].stride(0) == 1 and views[3].dtype == torch.float16
    featg = torch.from_numpy(feat).cuda()
    owner = {}                  # column -> (kind, uid, start counter)
    order = rng.permutation(columns)
    for i, col in enumerate(order[:30]):
        u = i % s.B
        if i % 3 == 2:
            e.slotStart(int(col), featg[u], u)
            owner[int(col)] = ("feat", u, 0)
        else:
            e.slotStartMel(int(col), views[u], u)
            owner[int(col)] = ("mel", u, 0)
    counter = 0
    for step, c in enumerate((1, 7, 64, 7, 1, 64, 64, 7)):
        if step == 3:           # joins at an odd counter, into free columns and over a stopped one
            for i, col in enumerate(order[30:36]):
                u = (5 * i + 3) % s.B
                e.slotStartMel(int(col), views[u], u)
                owner[int(col)] = ("mel", u, counter)
            e.slotStop(int(order[0]))
            owner.pop(int(order[0]))
        assert e.slotsStep(c)
        got = _frag_cols(e.slotsGetFeatures(counter, c), e.condTiles())
        for col, (kind, u, s0) in owner.items():
            k0 = counter - s0
            want = (want_mel if kind == "mel" else want_feat)[u, k0:k0 + c]
            n = want.shape[0]
            assert np.array_equal(got[col, :n], want), "%s column %d (uid %d), step %d: rows differ from the lockstep %s" % (
                kind, col, u, step, "upsampling" if kind == "mel" else "packing")
        counter += c
    assert counter > 2 * W
    with pytest.raises(ValueError):
        e.slotsGetFeatures(counter - W - 1, 2)          # (older than the window)
    e.slotsEnd()
    e.close()


# ---- 2. staggered joins ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mode", [(n, md) for n in ("cond_C3_B16", "cond_C3_B21_n37") for md in ("wg", "wg2", "wg3")])
def test_fp16_mel_staggered_joins_bit_identical_to_lockstep(name, mode):
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, 16)
    s = case.shape
    y_lock = _mel_lockstep(case, t, 16, mode, mel, w, m, up_w, cc.stride)
    columns = s.B - 4
    plan, counts = _mel_plan(s.B, columns, s.N, cc.stride, 21)
    assert sum(counts) >= 3 * WINDOW[name] and any(p[0] % 2 for p in plan)
    e = _mel_engine(case, t, 16, mode, w, m, up_w, cc.stride, columns)
    if mode == "wg3":
        assert "BT=3" in e.kernelInfo(), e.kernelInfo()
    melg = torch.from_numpy(mel).cuda()
    got, pcm = _mel_run(e, melg, plan, counts, WINDOW[name], cc.stride)
    e.close()
    _check_prefixes(got, y_lock, plan, "fp16 mel %s/%s" % (name, mode))
    table = O.mulaw_pcm_table(s.A)
    for uid in got:
        assert np.array_equal(pcm[uid], table[got[uid]]), "PCM of utterance %d" % uid


def test_fp32_mel_staggered_joins_equal_the_oracle():
    name, mode = "cond_C3_B16", "wg2"
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, 32)
    s = case.shape
    y_lock = _mel_lockstep(case, t, 32, mode, mel, w, m, up_w, cc.stride)
    # the lockstep run against the oracle fed Lh = Wcond x + bcond of the engine's own upsampled features, philox_selectors(seed)
    e = _mel_engine(case, t, 32, mode, w, m, up_w, cc.stride, s.B)
    e.setMel(torch.from_numpy(mel).cuda())
    e.upsampleFeatures(0, s.N)
    x = _frag_cols(e.getFeatures(0, s.N), e.condTiles())[:s.B, :, :cc.n_cond].transpose(0, 2, 1)      # [B][n_cond][N]
    e.close()
    lh = np.einsum("oc,bct->bot", w.astype(np.float64), x.astype(np.float64)) + m["cond_b"].astype(np.float64)[None, :, None]
    t.Lh = np.ascontiguousarray(lh.reshape(s.B, s.L, 2 * s.R, s.N).transpose(3, 1, 0, 2).astype(np.float32))
    t.sel = O.philox_selectors(SEED, s.N, s.B)
    ref = util.teacher_forced_oracle(case, t, y_lock)
    _, unexplained = util.explain_mismatches(ref["y"], y_lock, ref["lo"], ref["hi"], t.sel.T, 1e-5)
    assert not unexplained, unexplained[:5]
    assert (ref["y"] == y_lock).mean() >= 0.999
    columns = s.B - 4
    plan, counts = _mel_plan(s.B, columns, s.N, cc.stride, 22)
    e = _mel_engine(case, t, 32, mode, w, m, up_w, cc.stride, columns)
    got, _ = _mel_run(e, torch.from_numpy(mel).cuda(), plan, counts, WINDOW[name], cc.stride)
    e.close()
    _check_prefixes(got, y_lock, plan, "fp32 mel %s" % name)
    for (_, col, uid, n) in plan:
        if np.array_equal(y_lock[uid], ref["y"][uid]):
            assert np.array_equal(got[uid], ref["y"][uid, :n]), uid


# ---- 3. mixed sessions, 4. streaming -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
def test_mixed_feature_and_mel_columns_share_tiles(precision):
    """Feature and mel utterances interleave in the same tiles, and columns pass from one kind to the other; each utterance equals
    its own lockstep run (features: nvw_set_features; mel: nvw_set_mel + nvw_generate_stream)."""
    name = "cond_C3_B16"
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, precision)
    _, _, x, wx, _ = _cond_inputs(cc, half=precision == 16)
    assert np.array_equal(w, wx)
    s = case.shape
    y_mel = _mel_lockstep(case, t, precision, "wg", mel, w, m, up_w, cc.stride)
    y_feat = _lockstep(case, t, precision, "wg", x, w, m["cond_b"])
    columns = s.B - 4
    plan, counts = _mel_plan(2 * s.B, columns, s.N, cc.stride, 23)
    # utterances 0..B-1 run from mel, B..2B-1 from the features of utterance u - B (uid u - B)
    xg = torch.from_numpy(x).cuda()
    melg = torch.from_numpy(mel).cuda()
    feats = {u: xg[u - s.B] for u in range(s.B, 2 * s.B)}
    mels = {u: melg[u] for u in range(s.B)}
    kinds = {}
    for (_, col, uid, _) in plan:
        kinds.setdefault(col, set()).add(uid >= s.B)
    assert any(len(k) == 2 for k in kinds.values()), "some column must be reused across both kinds"
    e = _mel_engine(case, t, precision, "wg", w, m, up_w, cc.stride, columns)
    # (the driver starts utterance uid with Philox uid `uid`: map the feature ones back to uid - B)
    got, _ = _mel_run(_UidShift(e, s.B), mels, plan, counts, WINDOW[name], cc.stride, feats=feats)
    e.close()
    for (_, col, uid, n) in plan:
        ref = y_mel[uid] if uid < s.B else y_feat[uid - s.B]
        assert np.array_equal(got[uid], ref[:n]), "utterance %d (%s, column %d)" % (uid, "mel" if uid < s.B else "features", col)


class _UidShift:
    """The engine, with the Philox uid of feature utterances u >= shift taken as u - shift."""

    def __init__(self, e, shift):
        self._e, self._shift = e, shift

    def __getattr__(self, k):
        return getattr(self._e, k)

    def slotStart(self, col, x, uid, length=None):
        return self._e.slotStart(col, x, uid - self._shift if uid >= self._shift else uid, length)


@pytest.mark.parametrize("precision", [16, 32])
def test_streamed_frames_give_the_samples_of_the_whole_mel(precision):
    """Frames appended between steps in irregular pieces (0, 1, fewer than the taps, several) with `final` arriving late: every
    utterance equals its lockstep run.  Along the way steps above the headroom and bad nvw_slot_mel_frames calls are refused and
    change nothing."""
    name = "cond_C3_B16"
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, precision)
    s = case.shape
    y_lock = _mel_lockstep(case, t, precision, "wg2", mel, w, m, up_w, cc.stride)
    columns = s.B - 4
    plan, counts = _mel_plan(s.B, columns, s.N, cc.stride, 24)
    e = _mel_engine(case, t, precision, "wg2", w, m, up_w, cc.stride, columns)
    melg = torch.from_numpy(mel).cuda()
    got, _ = _mel_run(e, melg, plan, counts, WINDOW[name], cc.stride, stream_rng=np.random.default_rng(5), refusals=True)
    _check_prefixes(got, y_lock, plan, "streamed fp%d" % precision)
    # the entry points refuse what they cannot do
    e.slotsBegin(WINDOW[name])
    bits = 32
    assert not lib.nvw_slot_start_mel(e._h, 0, melg[0].cpu().data_ptr(), bits, melg.stride(1), 1, 4, 1, 0)      # host memory
    assert not lib.nvw_slot_start_mel(e._h, 0, melg[0].data_ptr(), 8, melg.stride(1), 1, 4, 1, 0)               # precision
    assert not lib.nvw_slot_start_mel(e._h, 0, melg[0].data_ptr(), bits, 0, 1, 4, 1, 0)                         # stride
    assert not lib.nvw_slot_start_mel(e._h, 0, melg[0].data_ptr(), bits, melg.stride(1), 1, -1, 0, 0)           # frames < 0
    assert not lib.nvw_slot_start_mel(e._h, 0, melg[0].data_ptr(), bits, melg.stride(1), 1, 0, 1, 0)            # 0 frames, final
    assert not lib.nvw_slot_start_mel(e._h, columns, melg[0].data_ptr(), bits, melg.stride(1), 1, 4, 1, 0)      # slot
    assert lib.nvw_slot_start_mel(e._h, 0, melg[0].data_ptr(), bits, melg.stride(1), 1, 0, 0, 0)                # 0 frames, not final
    assert e.slotsHeadroom() == 0
    assert not lib.nvw_slots_step(e._h, 1, None, None, None)
    e.slotsEnd()
    e.close()


# ---- 5. full chip -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("organisation", ["auto", "chain"])
def test_full_chip_distinct_mel_columns_reproduce_a_small_lockstep_run(organisation):
    """12 304 columns under AUTO, each with a mel tensor of its own (a copy of one of 16 utterances, in one allocation per column
    slice: no two columns read the same frames); selected columns reproduce the lockstep mel run of the 16, also after a few
    hundred restart at an odd counter.  A chain-organisation engine (64 columns) gives the same samples."""
    name = "cond_C3_B16"
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, 16)
    s = case.shape
    y_lock = _mel_lockstep(case, t, 16, "auto", mel, w, m, up_w, cc.stride)
    columns = 12304 if organisation == "auto" else 64
    e = _mel_engine(case, t, 16, organisation, w, m, up_w, cc.stride, columns)
    melg = torch.from_numpy(mel).cuda()
    rng = np.random.default_rng(7)
    uid = rng.integers(s.B, size=columns)
    store = melg[torch.from_numpy(uid).cuda()].contiguous()          # [columns][n_cond][frames]: distinct frames per column
    W = 64
    e.slotsBegin(W)
    for b in range(columns):
        e.slotStartMel(b, store[b], int(uid[b]))
    pos, counter = np.zeros(columns, dtype=np.int64), 0
    check = np.unique(np.concatenate([np.arange(16), rng.choice(columns, min(200, columns), replace=False), np.arange(columns - 16, columns)]))
    for step, c in enumerate((33, 64, 1, 64)):
        if step == 2:          # a few hundred columns restart at an odd counter
            restart = rng.choice(columns, min(300, columns // 2), replace=False)
            for b in restart:
                e.slotStartMel(int(b), store[int(b)], int(uid[b]))
                pos[b] = 0
        y = np.full((columns, c), -1, dtype=np.int32)
        assert e.slotsStep(c, y)
        for b in check:
            p0 = pos[b]
            want = y_lock[uid[b], p0:p0 + c]
            assert np.array_equal(y[b, :len(want)], want), "column %d (uid %d), step %d" % (b, uid[b], step)
        pos += c
        counter += c
    e.slotsEnd()
    e.close()


# ---- 6. Python ----------------------------------------------------------------------------------------------------------------------

def test_slot_stream_with_a_late_producer():
    """SlotStream: mel requests whose frames a simulated producer writes late (steps clamped by the headroom, steps of none) equal
    their lockstep runs."""
    name = "cond_C3_B16"
    cc = condgen.COND_BY_NAME[name]
    case, m, mel, up_w, w, t = _mel_inputs(cc, 16)
    s = case.shape
    y_lock = _mel_lockstep(case, t, 16, "wg", mel, w, m, up_w, cc.stride)
    frames = s.N // cc.stride
    e = _mel_engine(case, t, 16, "wg", w, m, up_w, cc.stride, 6)
    st = SlotStream(e, WINDOW[name])
    melg = torch.from_numpy(mel).cuda()
    bufs = [torch.zeros_like(melg[u]) for u in range(s.B)]
    written = [0] * s.B
    handles = {}
    for u in range(s.B):
        n0 = 0 if u % 2 else 4
        bufs[u][:, :n0] = melg[u][:, :n0]
        written[u] = n0
        handles[st.submit_mel(bufs[u], uid=u, frames=n0, final=False)] = u
    rng = np.random.default_rng(3)
    got = {h: [] for h in handles}
    finished, clamped, idle = [], 0, 0
    for it in range(2000):
        if not st.busy():
            break
        out = st.step(16)
        idle += not out
        clamped += any(0 < len(v[0]) < 16 for v in out.values())
        for h, (y, _) in out.items():
            got[h].append(y)
        finished += st.finished()
        for h, u in handles.items():
            if written[u] < frames and rng.random() < 0.5:
                n = min(frames, written[u] + int(rng.integers(1, 7)))
                bufs[u][:, written[u]:n] = melg[u][:, written[u]:n]
                written[u] = n
                st.extend_mel(h, n, final=n == frames)
    assert not st.busy() and idle > 0 and clamped > 0
    assert sorted(finished) == sorted(handles)
    for h, u in handles.items():
        assert np.array_equal(np.concatenate(got[h]), y_lock[u]), "request of utterance %d" % u
    st.close()
    e.close()


def test_model_slot_stream_takes_mel_requests():
    """NVWaveNetEngine.slot_stream given the model's upsampling: mel requests equal the lockstep mel run of an engine of the same
    wrapper."""
    from nv_wavenet_amd import nv_wavenet as NW
    import test_parity_gpu as T
    R, S, A, L, B, N = 64, 256, 256, 6, 8, 64
    _, dev, _ = T._wrapper_model(R, S, A, L, B, N)
    wrapper = NW.NVWaveNetEngine(**dev, precision=16)
    g = torch.Generator().manual_seed(12)
    n_cond, stride, window = 80, 4, 8
    mel = torch.randn(B, n_cond, N // stride, generator=g).cuda()
    up_w = (torch.rand(n_cond, n_cond, window, generator=g) - 0.5).cuda() * (3.46 / np.sqrt(2 * n_cond))
    up_b = ((torch.rand(n_cond, generator=g) - 0.5) * 0.2).cuda()
    cw = ((torch.rand(2 * R * L, n_cond, 1, generator=g) - 0.5) * (3.46 * 0.5 / np.sqrt(n_cond))).cuda()
    cb = ((torch.rand(2 * R * L, generator=g) - 0.5) * 0.2).cuda()
    e = wrapper._new_engine(B, N, NW.Impl.AUTO)
    e.setConditioningWeights(cw.float().contiguous(), cb.float().contiguous())
    e.setUpsampling(up_w.float().contiguous(), up_b.float().contiguous(), stride)
    e.setSelectorSeed(SEED)
    e.setMel(mel)
    y_lock = np.full((B, N), -1, dtype=np.int32)
    assert e.generate_stream(16, None, N, B, y_lock)
    e.synchronize()
    e.close()
    st = wrapper.slot_stream(3, 32, cw, cb, seed=SEED, upsample_weight=up_w, upsample_bias=up_b, upsample_stride=stride)
    handles = {st.submit_mel(mel[u], uid=u): u for u in range(B)}
    got = {h: [] for h in handles}
    while st.busy():
        for h, (y, _) in st.step(24).items():
            got[h].append(y)
    for h, u in handles.items():
        assert np.array_equal(np.concatenate(got[h]), y_lock[u]), u
    st.close()
    wrapper.close()
