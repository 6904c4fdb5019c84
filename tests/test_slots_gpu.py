"""GPU tests of slot mode (continuous batching, `-m gpu`): utterances join and leave a running generation at any step, in any
column, with chunks of any size, and each one's samples are those of its own lockstep run -- column uid of nvw_set_features +
nvw_set_selector_seed -- and, fp32, of the oracle fed the same conditioning and philox_selectors(seed).

The schedules run more utterances than the engine has columns (columns are reused), start them at odd sample offsets in permuted
columns, and step in chunks of 1, 7 and 64 samples over several wraps of the window (cond_C3_B16: maxD 32, window 64;
cond_C3_B21_n37: maxD 16, window 80)."""
import numpy as np
import pytest
import torch

import cases
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


def _plan(n_utt, columns, N, seed, sizes=COUNTS, lo=5):
    """A staggered schedule: (step, column, uid, length) of every utterance and the sample count of every step.  At most one join
    per step, at random steps (odd sample offsets included), into a random free column; a column is reused after its utterance ends.
    Step sizes cycle through `sizes`; lengths are N or drawn from [lo, N)."""
    rng = np.random.default_rng(seed)
    lengths = [N if i % 3 == 0 else int(rng.integers(lo, N)) for i in range(n_utt)]
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


def _engine(case, t, precision, mode, w, cond_b, columns, tanh_embed=True):
    s = case.shape
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, columns, s.N, impl=1 if s.S <= 4 * s.R else 3, tanhEmbed=tanh_embed, precision=precision,
                      organisation=util.MODE_ORG[mode])
    e.setEmbeddings(t.embP, t.embC)
    for l in range(s.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    e.setConditioningWeights(np.ascontiguousarray(w), cond_b)
    e.setSelectorSeed(SEED)
    return e


def _lockstep(case, t, precision, mode, x, w, cond_b, info_batch=None):
    """y [B][N] of the lockstep features path with in-kernel selectors (utterance b in column b); info_batch: also what the
    engine reports it launches for that batch (y, kernelInfo)."""
    s = case.shape
    e = _engine(case, t, precision, mode, w, cond_b, s.B)
    e.setFeatures(torch.from_numpy(x).cuda())
    y = np.full((s.B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, s.B, y, 1, False)
    e.synchronize()
    info = e.kernelInfo(info_batch) if info_batch else None
    e.close()
    return (y, info) if info_batch else y


def _slot_run(e, xg, plan, counts, window, extra=(), begin=True, end=True, uids=None):
    """Drives the engine through the schedule; returns {uid: samples}, {uid: pcm}.  extra: (start step, stop step, column, uid, x)
    of utterances started and stopped mid-run whose samples are not collected.  xg[uid]: the utterance's features (any view);
    uids[uid]: the Philox uid it runs with (default: uid)."""
    if begin:
        e.slotsBegin(window)
    ys, pcms, running = {}, {}, {}
    for step, c in enumerate(counts):
        for (s0, col, uid, n) in plan:
            if s0 == step:
                assert col not in running
                e.slotStart(col, xg[uid], uid if uids is None else uids[uid], n)
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
    if end:
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


# ---- every shape family ------------------------------------------------------------------------------------------------------------

def _synth(name, shape, precision, seed, n_cond=80, stride=4, window=8):
    """_setup for a shape without a tests/golden/cond_* record: a cond_layers + upsample pair and features from `seed`
    (condgen.make_cond_model), upsampled on the CPU.  Returns (case, m, x [B][n_cond][N], w, Lh [N][L][B][2R] for the oracle, t)."""
    import torch.nn.functional as F
    s = shape
    case = cases.Case(name, seed, [], s, 1, 1, 64)
    cc = condgen.CondCase(name, seed, name, n_cond, window, stride)
    m = condgen.make_cond_model(cc, s)
    x = F.conv_transpose1d(torch.from_numpy(m["features"]), torch.from_numpy(m["up_w"]), torch.from_numpy(m["up_b"]), stride=stride)
    x = x[:, :, :-(window - stride)].contiguous().numpy()
    w = m["cond_w"][:, :, 0]
    if precision == 16:
        x, w = x.astype(np.float16).astype(np.float32), w.astype(np.float16).astype(np.float32)
    t = util.gen_o1(case, half=precision == 16)
    return case, m, x, w, _lh(s, x, w, m["cond_b"]), t


def _lh(s, x, w, b):
    """Lh [N][L][B][2R] = Wcond x + bcond in float64, for the oracle."""
    lh = np.einsum("oc,bct->bot", w.astype(np.float64), x.astype(np.float64)) + b.astype(np.float64)[None, :, None]
    return np.ascontiguousarray(lh.reshape(s.B, s.L, 2 * s.R, s.N).transpose(3, 1, 0, 2).astype(np.float32))


Shape = cases.Shape      # R S A L B N maxD
FAMILIES = {              # shape, window (a multiple of the largest dilation), seed
    "C1_R32": (Shape(32, 128, 256, 8, 8, 64, 8), 16, 601),
    "C2_maxD512_W512": (Shape(64, 128, 256, 20, 6, 1100, 512), 512, 602),
    "C2_maxD512_W1024": (Shape(64, 128, 256, 20, 6, 1100, 512), 1024, 602),
    "C4_R128_L30": (Shape(128, 256, 256, 30, 8, 48, 16), 48, 603),
    "oddL7": (Shape(64, 128, 256, 7, 10, 40, 4), 12, 604),
    "A512": (Shape(64, 128, 512, 20, 8, 48, 8), 24, 605),
    "A1024_L12": (Shape(128, 256, 1024, 12, 8, 48, 8), 16, 606),
    "R256": (Shape(256, 256, 256, 6, 6, 40, 8), 24, 607),
    "S8R": (Shape(32, 256, 256, 6, 6, 40, 8), 24, 608),
}
# tiles per workgroup a slot step launches by requested organisation: the four-tile kernels exist for the packed conditioning only,
# so wg4 launches the three-tile wavenet_wg<.., RAW=3> in slot mode, as it does for the lockstep features path
SLOT_BT = {"wg": 1, "wg2": 2, "wg3": 3, "wg4": 3}


def _family_runs():
    runs = []
    for name, (s, _, _) in FAMILIES.items():
        runs += [(name, 16, md) for md in (("wg", "wg2", "wg3", "wg4") if s.R <= 64 else ("wg",))]
        runs += [(name, 32, md) for md in (("wg", "wg2") if s.R < 128 else ("wg",))]
    return runs


ORACLE_TIED = {"C1_R32", "C4_R128_L30", "C2_maxD512_W512"}


@pytest.mark.parametrize("name,precision,mode", _family_runs())
def test_staggered_joins_at_every_shape_family(name, precision, mode):
    """Each utterance of a staggered schedule equals its column uid of the lockstep setFeatures + setSelectorSeed run, bit for
    bit, at every shape family the library builds: R = 32 (two waves), maxD 512 with windows 512 and 1 024, R = 128 with 30
    layers, an odd layer count, A = 512 and 1 024, R = 256, S = 8R.  fp16 with one to three tiles per workgroup, fp32 with one and
    two; fp32 lockstep runs of R32, R128 and maxD 512 are held to the oracle as in test_fp32_staggered_joins_equal_the_oracle."""
    s, window, seed = FAMILIES[name]
    case, m, x, w, Lh, t = _synth(name, s, precision, seed)
    counts = tuple(min(c, window) for c in (COUNTS if window >= 64 else (7, 1, window, 3, window - 1)))
    columns = s.B - 2
    y_lock, lock_info = _lockstep(case, t, precision, mode, x, w, m["cond_b"], info_batch=columns)
    if precision == 32 and mode == "wg" and name in ORACLE_TIED:
        t.Lh = Lh
        t.sel = O.philox_selectors(SEED, s.N, s.B)
        ref = util.teacher_forced_oracle(case, t, y_lock)
        _, unexplained = util.explain_mismatches(ref["y"], y_lock, ref["lo"], ref["hi"], t.sel.T, 1e-5)
        assert not unexplained, unexplained[:5]
        assert (ref["y"] == y_lock).mean() >= 0.999
    plan, steps = _plan(s.B, columns, s.N, seed, sizes=counts)
    assert sum(steps) > window, "the schedule must wrap the window"
    e = _engine(case, t, precision, mode, w, m["cond_b"], columns)
    e.slotsBegin(window)
    info = e.kernelInfo()
    assert "RAW=3" in info and "BT=%d," % SLOT_BT[mode] in info and info == lock_info, (info, lock_info)
    got, pcm = _slot_run(e, torch.from_numpy(x).cuda(), plan, steps, window, begin=False)
    e.close()
    _check_prefixes(got, y_lock, plan, "fp%d %s/%s" % (precision, name, mode))
    table = O.mulaw_pcm_table(s.A)
    for uid in got:
        assert np.array_equal(pcm[uid], table[got[uid]]), "PCM of utterance %d" % uid


# ---- full-chip column counts ---------------------------------------------------------------------------------------------------

C3 = Shape(64, 256, 256, 20, 24, 2048, 32)


@pytest.mark.parametrize("columns", [4112, 8208, 12304])
def test_full_chip_columns_reproduce_a_small_lockstep_run(columns):
    """Column b runs utterance u = perm(b) mod 24 of a small C3 case with uid u, so it must reproduce column u of one fp16
    lockstep run of 24 utterances.  Every column starts in the first step (more than 1 024 restarted columns: the reset kernel's
    blockIdx.y loop); a few hundred restart later in scattered tiles; the highest columns stop (the launch shrinks) and start
    again (it grows).  Steps of 1 024 samples on a window of 1 024 (the feed's second grid-stride pass) and odd steps that wrap.
    AUTO's tiles per workgroup follow from the CU count: 2 beyond one tile per CU, 3 beyond two (four-tile kernels are not built
    for slot mode)."""
    case, m, x, w, Lh, t = _synth("full_chip_C3", C3, 16, 611)
    B0, W = C3.B, 1024
    y_lock = _lockstep(case, t, 16, "auto", x, w, m["cond_b"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(columns)
    lengths = [int(v) for v in rng.integers(1100, C3.N + 1, size=B0)]
    xg = torch.from_numpy(x).cuda()
    s = case.shape
    e = WavenetEngine(s.R, s.S, s.A, s.L, s.maxD, columns, 64, impl=1, tanhEmbed=True, precision=16, organisation=0)
    e.setEmbeddings(t.embP, t.embC)
    for l in range(s.L):
        e.setLayerWeights(l, t.Wprev[l], t.Wcur[l], t.Bh[l], t.Wres[l], t.Bres[l], t.Wskip[l], t.Bskip[l])
    e.setOutWeights(t.Wzs, t.Bzs, t.Wza, t.Bza)
    e.setConditioningWeights(np.ascontiguousarray(w), m["cond_b"])
    e.setSelectorSeed(SEED)
    e.slotsBegin(W)
    utt = np.full(columns, -1)        # utterance of the column (-1 idle), its next local sample
    pos = np.zeros(columns, dtype=np.int64)

    def start(cols):
        for b in cols:
            u = int(rng.integers(B0))
            e.slotStart(int(b), xg[u], u, lengths[u])
            utt[b], pos[b] = u, 0

    perm = rng.permutation(columns)
    for b in range(columns):
        u = int(perm[b] % B0)
        e.slotStart(b, xg[u], u, lengths[u])
        utt[b] = u
    counts = [700, W, 333, W, W]
    top = columns - 40
    for step, c in enumerate(counts):
        if step == 2:
            start(rng.choice(top, size=300, replace=False))               # scattered restarts
            for b in range(top, columns):                                  # the highest columns stop: the launch shrinks
                e.slotStop(b)
                utt[b] = -1
        if step == 3:
            start(range(top, columns))                                     # ... and grows again
        live = np.nonzero(utt >= 0)[0]
        tiles = int(live.max()) // 16 + 1
        bt = 3 if tiles > 2 * cus else 2 if tiles > cus else 1
        info = e.kernelInfo(int(live.max()) + 1)
        assert "BT=%d," % bt in info and "RAW=3" in info, (columns, cus, info)
        y = np.full((columns, c), -1, dtype=np.int32)
        assert e.slotsStep(c, y)
        for b in live:
            u, p0 = utt[b], pos[b]
            k = min(c, lengths[u] - p0)
            if not np.array_equal(y[b, :k], y_lock[u, p0:p0 + k]):
                bad = int(np.nonzero(y[b, :k] != y_lock[u, p0:p0 + k])[0][0])
                raise AssertionError("%d columns, step %d: column %d (utterance %d) differs at local sample %d" % (
                    columns, step, b, u, p0 + bad))
            pos[b] += k
            if pos[b] == lengths[u]:
                e.slotStop(int(b))
                utt[b] = -1
    e.slotsEnd()
    e.close()


# ---- lifetime and interface edges ------------------------------------------------------------------------------------------------

EDGE = Shape(64, 256, 256, 20, 8, 96, 32)


def _edge(precision, N=96, B=8, seed=621):
    s = EDGE._replace(N=N, B=B)
    return _synth("edge_C3_N%d" % N, s, precision, seed)


def test_utterances_longer_than_the_engine():
    """A slot engine built for N = 8 samples runs utterances of 300 to 1 500 samples: each equals its column of a lockstep engine
    whose N covers it."""
    case, m, x, w, Lh, t = _edge(16, N=1500, B=6)
    s = case.shape
    y_lock = _lockstep(case, t, 16, "wg", x, w, m["cond_b"])
    plan, counts = _plan(s.B, 3, s.N, 31, lo=300)
    assert min(p[3] for p in plan) >= 300 and max(p[3] for p in plan) == 1500
    short = case._replace(shape=s._replace(N=8))
    e = _engine(short, t, 16, "wg", w, m["cond_b"], 3)
    assert e.maxSamples == 8
    got, _ = _slot_run(e, torch.from_numpy(x).cuda(), plan, counts, 64)
    e.close()
    _check_prefixes(got, y_lock, plan, "N = 8 engine")


@pytest.mark.parametrize("mode", ["wg", "wg2"])
def test_smallest_window_equals_the_largest_dilation(mode):
    """W = maxD = 32, steps of 1, W - 1 and W samples."""
    case, m, x, w, Lh, t = _edge(16)
    s = case.shape
    y_lock = _lockstep(case, t, 16, mode, x, w, m["cond_b"])
    plan, counts = _plan(s.B, s.B - 3, s.N, 32, sizes=(1, 31, 32))
    e = _engine(case, t, 16, mode, w, m["cond_b"], s.B - 3)
    got, _ = _slot_run(e, torch.from_numpy(x).cuda(), plan, counts, 32)
    e.close()
    _check_prefixes(got, y_lock, plan, "W = 32")


def test_idle_steps_and_a_second_session():
    """Steps with no active column in the middle of a session, then new joins: their samples are unchanged.  slotsBegin called
    again without slotsEnd (ending a session with utterances still running): the second session equals a fresh engine's."""
    case, m, x, w, Lh, t = _edge(16)
    s = case.shape
    y_lock = _lockstep(case, t, 16, "wg", x, w, m["cond_b"])
    xg = torch.from_numpy(x).cuda()
    half = s.B // 2
    pa, ca = _plan(half, 3, s.N, 33)
    pb, cb = _plan(s.B - half, 3, s.N, 34)
    gap = [5, 64, 1]
    shift = len(ca) + len(gap)
    plan = pa + [(st + shift, col, uid + half, n) for (st, col, uid, n) in pb]
    counts = list(ca) + gap + list(cb)
    e = _engine(case, t, 16, "wg", w, m["cond_b"], 3)
    got, _ = _slot_run(e, xg, plan, counts, 64)
    _check_prefixes(got, y_lock, plan, "idle gap")
    # an unfinished session: three utterances running, two steps; then a new session on the same engine
    e.slotsBegin(64)
    for col in range(3):
        e.slotStart(col, xg[col + 1], 77 + col)
    assert e.slotsStep(7) and e.slotsStep(40)
    again, _ = _slot_run(e, xg, plan, counts, 64)
    e.close()
    fresh = _engine(case, t, 16, "wg", w, m["cond_b"], 3)
    want, _ = _slot_run(fresh, xg, plan, counts, 64)
    fresh.close()
    for uid in want:
        assert np.array_equal(again[uid], want[uid]), "second session, utterance %d" % uid


@pytest.mark.parametrize("precision,mode", [(16, "wg3"), (16, "wg4"), (32, "wg2")])
def test_lockstep_after_slot_end_starts_from_clean_rings(precision, mode):
    """maxBatch 200: a lockstep batch of 16, a slot session whose highest column is 199, slotsEnd, then a lockstep batch of 200:
    equal to a fresh engine's bit for bit.  The slot launches write rings of tiles the first lockstep run never touched, so the
    run after them is only clean if the steps raised the dirty-tile count that the next run's clear covers."""
    B = 200
    case, m, x, w, Lh, t = _edge(precision, N=64, B=B)
    s = case.shape
    xg = torch.from_numpy(x).cuda()

    def engine():
        e = _engine(case, t, precision, mode, w, m["cond_b"], B)
        e.setFeatures(xg)
        return e

    e = engine()
    y16 = np.full((B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, 16, y16, 1, False)
    e.synchronize()
    e.slotsBegin(64)
    for col in (0, 17, 150, 199):
        e.slotStart(col, xg[col], col)
    for c in (64, 30, 64):
        assert e.slotsStep(c)
    e.slotsEnd()
    e.setFeatures(xg)                   # (a new batch: history to 128, rings cleared as far as launches have dirtied them)
    y = np.full((B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, B, y, 1, False)
    e.synchronize()
    e.close()
    f = engine()
    want = np.full((B, s.N), -1, dtype=np.int32)
    assert f.run(s.N, B, want, 1, False)
    f.synchronize()
    f.close()
    assert np.array_equal(y16[:16], want[:16])
    bad = np.nonzero((y != want).any(axis=1))[0]
    assert bad.size == 0, "columns %s differ from a fresh engine's run after a slot session" % bad[:10]


@pytest.mark.parametrize("precision", [32, 16])
def test_feature_layouts_fp16_sources_and_uids_near_2_32(precision):
    """Utterances fed as time-major views (cStride 1), sliced views (cStride > n_cond, tStride 3) and -- fp32 engine -- fp16
    tensors, with uids near 2**32.  The reference is a lockstep run fed the same values (fp16-rounded where the source is fp16)
    and the selectors of those uids from a table (oracle.philox_selectors_at); fp32: that run is held to the oracle as well."""
    case, m, x, w, Lh, t = _edge(precision, N=96, B=9, seed=625)
    s = case.shape
    uids = [2 ** 32 - 1 - 3 * u if u % 3 else 2 ** 31 + u for u in range(s.B)]
    uids[0] = 2 ** 32 - 1
    xg = torch.from_numpy(x).cuda()
    views, x_eff = [], x.copy()
    for u in range(s.B):
        if u % 3 == 0:
            views.append(xg[u].t().contiguous().t())                              # time-major
        elif u % 3 == 1:
            base = torch.zeros(x.shape[1], 3 * s.N + 2, device="cuda")
            base[:, 2::3] = xg[u]
            views.append(base[:, 2::3])                                           # sliced: cStride 3N + 2, tStride 3
        else:
            views.append(xg[u].half())                                            # fp16 source
            x_eff[u] = x[u].astype(np.float16).astype(np.float32)
    assert views[0].stride(0) == 1 and views[1].stride() == (3 * s.N + 2, 3)
    table = O.philox_selectors_at(SEED, np.arange(s.N)[:, None], np.array(uids)[None, :])
    e = _engine(case, t, precision, "wg", w, m["cond_b"], s.B)
    e.setFeatures(torch.from_numpy(x_eff).cuda())
    e.setSelectors(table, s.N)
    y_lock = np.full((s.B, s.N), -1, dtype=np.int32)
    assert e.run(s.N, s.B, y_lock, 1, False)
    e.synchronize()
    e.close()
    if precision == 32:
        t.Lh = _lh(s, x_eff, w, m["cond_b"])
        t.sel = table
        ref = util.teacher_forced_oracle(case, t, y_lock)
        _, unexplained = util.explain_mismatches(ref["y"], y_lock, ref["lo"], ref["hi"], table.T, 1e-5)
        assert not unexplained, unexplained[:5]
        assert (ref["y"] == y_lock).mean() >= 0.999
    plan, counts = _plan(s.B, s.B - 3, s.N, 35)
    e = _engine(case, t, precision, "wg", w, m["cond_b"], s.B - 3)
    got, _ = _slot_run(e, views, plan, counts, 64, uids=uids)
    e.close()
    _check_prefixes(got, y_lock, plan, "fp%d layouts / uids" % precision)


def test_side_stream_and_device_outputs():
    """The steps of a session on a non-default stream with samples and PCM in device memory, synchronised once at the end: the
    same samples and PCM as host outputs on the null stream."""
    case, m, x, w, Lh, t = _edge(16)
    s = case.shape
    xg = torch.from_numpy(x).cuda()
    plan, counts = _plan(s.B, s.B - 3, s.N, 36)
    cols = s.B - 3
    e = _engine(case, t, 16, "wg", w, m["cond_b"], cols)
    want, want_pcm = _slot_run(e, xg, plan, counts, 64)
    ys = [torch.full((cols, c), -1, dtype=torch.int32, device="cuda") for c in counts]
    ps = [torch.zeros((cols, c), dtype=torch.int16, device="cuda") for c in counts]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    e.slotsBegin(64)
    running = {}
    for step, c in enumerate(counts):
        for (s0, col, uid, n) in plan:
            if s0 == step:
                e.slotStart(col, xg[uid], uid, n)
                running[col] = n
        assert e.slotsStep(c, ys[step], ps[step], stream=side.cuda_stream)
        for col in list(running):
            running[col] -= min(c, running[col])
            if running[col] == 0:
                del running[col]
                e.slotStop(col)
    side.synchronize()
    e.slotsEnd()
    e.close()
    y = np.concatenate([a.cpu().numpy() for a in ys], axis=1)
    p = np.concatenate([a.cpu().numpy() for a in ps], axis=1)
    for (s0, col, uid, n) in plan:
        at = sum(counts[:s0])
        assert np.array_equal(y[col, at:at + n], want[uid]), "utterance %d" % uid
        assert np.array_equal(p[col, at:at + n], want_pcm[uid]), "PCM of utterance %d" % uid
