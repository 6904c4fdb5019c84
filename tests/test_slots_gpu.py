"""GPU tests of slot mode (continuous batching, `-m gpu`): utterances join and leave a running generation at any step, in any
column, with chunks of any size, and each one's samples are those of its own lockstep run -- column uid of nvw_set_features +
nvw_set_selector_seed -- and, fp32, of the oracle fed the same conditioning and philox_selectors(seed).

The schedules run more utterances than the engine has columns (columns are reused), start them at odd sample offsets in permuted
columns, and step in chunks of 1, 7 and 64 samples over several wraps of the window (cond_C3_B16: maxD 32, window 64;
cond_C3_B21_n37: maxD 16, window 80)."""
import numpy as np
import pytest
import torch

import condgen
import util
from nv_wavenet_amd import WavenetEngine
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.slots import SlotStream
from oracle import oracle as O
from test_features_gpu import _cond_inputs

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000000071
COUNTS = (7, 1, 64, 7, 1, 7, 64, 1, 7)
WINDOW = {"cond_C3_B16": 64, "cond_C3_B21_n37": 80}      # 2 x / 5 x the largest dilation (32 / 16): a wrap that is not a power of two


def _plan(n_utt, columns, N, seed):
    """A staggered schedule: (step, column, uid, length) of every utterance and the sample count of every step.  At most one join
    per step, at random steps (odd sample offsets included), into a random free column; a column is reused after its utterance ends."""
    rng = np.random.default_rng(seed)
    lengths = [N if i % 3 == 0 else int(rng.integers(5, N)) for i in range(n_utt)]
    queue = [int(u) for u in rng.permutation(n_utt)]
    free, running, plan, counts, step = list(range(columns)), {}, [], [], 0
    while queue or running:
        if queue and free and (not running or rng.random() < 0.6):
            col = free.pop(int(rng.integers(len(free))))
            uid = queue.pop(0)
            plan.append((step, col, uid, lengths[uid]))
            running[col] = lengths[uid]
        c = COUNTS[step % len(COUNTS)]
        counts.append(c)
        for col in list(running):
            running[col] -= min(c, running[col])
            if running[col] == 0:
                del running[col]
                free.append(col)
        step += 1
    return plan, counts


def _engine(case, t, precision, mode, w, cond_b, columns):
    s = case.shape
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, columns, s.N, impl=1, tanhEmbed=True, precision=precision,
                      organisation=util.MODE_ORG[mode])
    e.setEmbeddings(t.embP, t.embC)
    for l in range(s.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    e.setConditioningWeights(np.ascontiguousarray(w), cond_b)
    e.setSelectorSeed(SEED)
    return e


def _lockstep(case, t, precision, mode, x, w, cond_b):
    """y [B][N] of the lockstep features path with in-kernel selectors (utterance b in column b)."""
    s = case.shape
    e = _engine(case, t, precision, mode, w, cond_b, s.B)
    e.setFeatures(torch.from_numpy(x).cuda())
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    e.close()
    return y


def _slot_run(e, xg, plan, counts, window, extra=()):
    """Drives the engine through the schedule; returns {uid: samples}, {uid: pcm}.  extra: (start step, stop step, column, uid, x)
    of utterances started and stopped mid-run whose samples are not collected."""
    e.slotsBegin(window)
    ys, pcms, running = {}, {}, {}
    for step, c in enumerate(counts):
        for (s0, col, uid, n) in plan:
            if s0 == step:
                assert col not in running
                e.slotStart(col, xg[uid], uid, n)
                running[col] = [uid, n]
                ys[uid], pcms[uid] = [], []
        for (s0, s1, col, uid, xx) in extra:
            if s0 == step:
                e.slotStart(col, xx, uid)
            if s1 == step:
                e.slotStop(col)
        y = np.full((e.maxBatch, c), -1, dtype=np.int32)
        pcm = np.zeros((e.maxBatch, c), dtype=np.int16)
        assert e.slotsStep(c, y, pcm)
        for col in list(running):
            uid, left = running[col]
            k = min(c, left)
            ys[uid].append(y[col, :k])
            pcms[uid].append(pcm[col, :k])
            running[col][1] -= k
            if running[col][1] == 0:
                del running[col]
                e.slotStop(col)
    assert not running
    e.slotsEnd()
    return {u: np.concatenate(v) for u, v in ys.items()}, {u: np.concatenate(v) for u, v in pcms.items()}


def _setup(name, precision):
    cc = condgen.COND_BY_NAME[name]
    case, m, x, w, Lh = _cond_inputs(cc, half=precision == 16)
    t = util.gen_o1(case, half=precision == 16)
    return case, m, x, w, Lh, t


def _check_prefixes(got, y_ref, plan, what):
    for (_, col, uid, n) in plan:
        assert got[uid].shape == (n,), (what, uid, got[uid].shape)
        bad = np.nonzero(got[uid] != y_ref[uid, :n])[0]
        assert bad.size == 0, "%s: utterance %d (column %d, %d samples) differs from its lockstep run first at sample %d" % (
            what, uid, col, n, bad[0])


@pytest.mark.parametrize("name,mode", [("cond_C3_B16", "wg"), ("cond_C3_B21_n37", "wg2")])
def test_fp32_staggered_joins_equal_the_oracle(name, mode):
    case, m, x, w, Lh, t = _setup(name, 32)
    s = case.shape
    y_lock = _lockstep(case, t, 32, mode, x, w, m["cond_b"])
    # the lockstep run against the oracle fed Lh = Wcond x + bcond and philox_selectors(seed), the bar of test_features_gpu
    t.Lh = Lh
    t.sel = O.philox_selectors(SEED, s.N, s.B)
    ref = util.teacher_forced_oracle(case, t, y_lock)
    _, unexplained = util.explain_mismatches(ref["y"], y_lock, ref["lo"], ref["hi"], t.sel.T, 1e-5)
    assert not unexplained, unexplained[:5]
    assert (ref["y"] == y_lock).mean() >= 0.999
    # slot mode: the same samples, utterance by utterance, whatever the column, start step and chunking
    columns = s.B - 4
    plan, counts = _plan(s.B, columns, s.N, 11)
    assert sum(counts) >= 3 * WINDOW[name] and any(p[0] % 2 for p in plan)
    e = _engine(case, t, 32, mode, w, m["cond_b"], columns)
    got, _ = _slot_run(e, torch.from_numpy(x).cuda(), plan, counts, WINDOW[name])
    e.close()
    _check_prefixes(got, y_lock, plan, "fp32 %s" % name)
    # (so every utterance whose lockstep column is the oracle's column uid -- all of them but a CDF-edge divergence -- equals it too)
    for (_, col, uid, n) in plan:
        if np.array_equal(y_lock[uid], ref["y"][uid]):
            assert np.array_equal(got[uid], ref["y"][uid, :n]), uid


@pytest.mark.parametrize("name,mode", [(n, md) for n in ("cond_C3_B16", "cond_C3_B21_n37") for md in ("wg", "wg2", "wg3")])
def test_fp16_staggered_joins_bit_identical_to_lockstep(name, mode):
    """fp16: one, two and three tiles per workgroup; every utterance bit-identical to its column of the lockstep run; the per-slot
    PCM is the mu-law table of the samples."""
    case, m, x, w, Lh, t = _setup(name, 16)
    s = case.shape
    y_lock = _lockstep(case, t, 16, mode, x, w, m["cond_b"])
    columns = s.B - 4
    plan, counts = _plan(s.B, columns, s.N, 12)
    assert sum(counts) >= 3 * WINDOW[name]
    e = _engine(case, t, 16, mode, w, m["cond_b"], columns)
    if mode == "wg3":
        assert "BT=3" in e.kernelInfo(), e.kernelInfo()
    got, pcm = _slot_run(e, torch.from_numpy(x).cuda(), plan, counts, WINDOW[name])
    e.close()
    _check_prefixes(got, y_lock, plan, "fp16 %s/%s" % (name, mode))
    table = O.mulaw_pcm_table(s.A)
    for uid in got:
        assert np.array_equal(pcm[uid], table[got[uid]]), "PCM of utterance %d" % uid


@pytest.mark.parametrize("precision", [32, 16])
def test_starting_and_stopping_a_column_leaves_the_others_unchanged(precision):
    name = "cond_C3_B16"
    case, m, x, w, Lh, t = _setup(name, precision)
    s = case.shape
    columns = s.B - 4
    plan, counts = _plan(s.B, columns, s.N, 13)
    xg = torch.from_numpy(x).cuda()
    e = _engine(case, t, precision, "wg", w, m["cond_b"], columns + 1)      # column `columns` is the plan's spare
    base, _ = _slot_run(e, xg, plan, counts, WINDOW[name])
    intruder = [(3, 6, columns, 1000, xg[2].half() if precision == 16 else xg[2].clone()), (8, 9, columns, 1001, xg[5])]
    disturbed, _ = _slot_run(e, xg, plan, counts, WINDOW[name], extra=intruder)
    e.close()
    for uid in base:
        assert np.array_equal(base[uid], disturbed[uid]), "utterance %d changed when another column started and stopped" % uid


def _raw_start(e, slot, x, precision=None, cs=None, ts=None, length=None, uid=0):
    return lib.nvw_slot_start(e._h, slot, x.data_ptr() if hasattr(x, "data_ptr") else x, precision or 32,
                              x.stride(0) if cs is None else cs, x.stride(1) if ts is None else ts,
                              x.size(1) if length is None else length, uid)


def test_refusals_change_nothing_and_a_chain_engine_gives_the_same_samples():
    name = "cond_C3_B16"
    case, m, x, w, Lh, t = _setup(name, 16)
    s = case.shape
    columns = s.B - 4
    plan, counts = _plan(s.B, columns, s.N, 14)
    xg = torch.from_numpy(x).cuda()
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, columns, s.N, impl=1, precision=16, organisation=util.MODE_ORG["wg"])
    assert lib.nvw_slots_begin(e._h, 64) == 0                       # no conditioning weights yet
    e.close()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], columns)
    x0 = xg[0]
    assert _raw_start(e, 0, x0) == 0                                # not in slot mode
    assert lib.nvw_slots_step(e._h, 8, None, None, None) == 0
    assert lib.nvw_slot_stop(e._h, 0) == 0
    for bad in (0, -64, 48, 16):                                    # not a positive multiple of the largest dilation (32)
        assert lib.nvw_slots_begin(e._h, bad) == 0
    e.slotsBegin(64)
    host = np.zeros((s.N, 80), dtype=np.float32)
    refused = [_raw_start(e, -1, x0), _raw_start(e, columns, x0), _raw_start(e, 0, x0, precision=8), _raw_start(e, 0, x0, cs=0),
               _raw_start(e, 0, x0, ts=-1), _raw_start(e, 0, x0, length=0), _raw_start(e, 0, host.ctypes.data, cs=1, ts=80, length=s.N),
               lib.nvw_slot_stop(e._h, -1), lib.nvw_slot_stop(e._h, columns), lib.nvw_slots_step(e._h, 0, None, None, None),
               lib.nvw_slots_step(e._h, 65, None, None, None)]
    assert refused == [0] * len(refused), refused
    got, _ = _slot_run(e, xg, plan, counts, 64)
    e.close()
    clean = _engine(case, t, 16, "wg", w, m["cond_b"], columns)
    want, _ = _slot_run(clean, xg, plan, counts, 64)
    clean.close()
    for uid in want:
        assert np.array_equal(got[uid], want[uid]), uid
    # a chain-organisation engine runs wavenet_wg in slot mode, as it does for the features path: the same samples
    ch = _engine(case, t, 16, "chain", w, m["cond_b"], columns)
    assert "wavenet_chain" in ch.kernelInfo(), ch.kernelInfo()
    chain, _ = _slot_run(ch, xg, plan, counts, 64)
    ch.close()
    for uid in want:
        assert np.array_equal(chain[uid], want[uid]), uid


def test_slot_stream_more_requests_than_columns():
    """SlotStream end to end: 16 requests on 5 columns (a FIFO), fp16 and fp32 sources; every request completes exactly once, its
    samples are its solo run (column uid of the lockstep run) and its PCM their mu-law values; a device-memory step gives the same."""
    name = "cond_C3_B16"
    case, m, x, w, Lh, t = _setup(name, 16)
    s = case.shape
    y_lock = _lockstep(case, t, 16, "wg", x, w, m["cond_b"])
    xg = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(15)
    lengths = [int(rng.integers(3, s.N + 1)) for _ in range(s.B)]
    e = _engine(case, t, 16, "wg", w, m["cond_b"], 5)
    st = SlotStream(e, 64)
    handles = {}
    for uid in range(s.B):
        src = xg[uid, :, :lengths[uid]]
        handles[st.submit(src.half() if uid % 2 else src, uid=uid)] = uid
    assert st.waiting() == s.B
    out = {h: [] for h in handles}
    pcm = {h: [] for h in handles}
    done = []
    steps = 0
    while st.busy():
        for h, (yy, pp) in st.step(COUNTS[steps % len(COUNTS)]).items():
            out[h].append(yy)
            pcm[h].append(pp)
        assert max(st.running().values(), default=0) < 5
        done += st.finished()
        steps += 1
        assert steps < 1000
    assert sorted(done) == sorted(handles) and st.finished() == []
    table = O.mulaw_pcm_table(s.A)
    for h, uid in handles.items():
        y = np.concatenate(out[h])
        assert np.array_equal(y, y_lock[uid, :lengths[uid]]), "request %d" % uid
        assert np.array_equal(np.concatenate(pcm[h]), table[y])
    st.close()
    e.close()
    # device-resident outputs: the same samples
    e = _engine(case, t, 16, "wg", w, m["cond_b"], 5)
    e.slotsBegin(64)
    e.slotStart(3, xg[7], 7)
    yd = torch.full((5, 40), -1, dtype=torch.int32, device="cuda")
    assert e.slotsStep(40, yd)
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy()[3], y_lock[7, :40])
    e.close()
