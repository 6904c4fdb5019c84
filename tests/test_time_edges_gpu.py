"""GPU tests of the time-parallel pass at the edges of the layer / dilation schedule and without the embedding tanh (`-m gpu`; cases and
why: tests/time_edge_cases.py).  Prefill, scoring and scoring with carried state state the schedule again in
nvWavenetInfer::timeModel(), in time_finish_kernel and in prefill_window / prefill_first; the generation kernels are held at these
schedules by tests/test_schedule_edges_gpu.py, the pass is held here:

  1. scoreSamples against the float64 reference (score_cases.bar), which tests/test_time_edges_cpu.py holds to the oracle;
  2. prefillStates against the sequentially primed column, byte for byte;
  3. scoreChunks against scoreSamples bit for bit, its out-states against prefillStates byte for byte;
  4. all of it, and the generation kernels' features path, slot sessions and primed columns, with tanhEmbed = False -- what the
     reference's PyTorch export sets (pytorch/wavenet.py:186);
  5. prefill and chunks from mel frames at two short schedules.

No tolerance is new: score_cases.bar, util.fp16_bars, the fp32 sample bars of test_schedule_edges_gpu._fp32_bars, or equality."""
import numpy as np
import pytest
import torch

import cases
import mel_time_cases as MT
import prefill_cases as PF
import schedule_edges as E
import score_carry_cases as CC
import score_cases as SC
import test_mel_time_gpu as TM
import test_parity_gpu as P
import test_prefill_gpu as TP
import test_schedule_edges_gpu as TSE
import test_score_carry_gpu as TC
import test_score_gpu as TS
import test_slots_gpu as TSL
import time_edge_cases as TE
import util
from oracle import oracle as O
from test_slots_state_gpu import Run

pytestmark = pytest.mark.gpu

_nets, _refs = {}, {}


class EdgeNet(TS.Net):
    """test_score_gpu.Net with the embedding tanh as a setting of the engine and of the reference"""

    def __init__(self, shape, seed, precision, L, maxD, N, tanh_embed=True):
        super().__init__(shape, seed, precision, L, maxD, N, TE.COLUMNS)
        self.tanh_embed = tanh_embed
        self.key = self.key + (tanh_embed,)

    def engine(self, **kw):
        kw.setdefault("tanh_embed", self.tanh_embed)
        return super().engine(**kw)

    def reference(self, c, n, T=1.0):
        key = self.key + (c, n, float(T))
        if key not in _refs:
            _refs[key] = SC.reference(self.t, self.s, self.y[c, :n], SC.lh_of(self.x[c], self.w, self.b, self.s.R, self.s.L), T, tanh_embed=self.tanh_embed)
        return _refs[key]


def _net(shape, seed, precision, L, maxD, N, tanh_embed=True):
    key = (shape, seed, precision, L, maxD, N, tanh_embed)
    if key not in _nets:
        _nets[key] = EdgeNet(shape, seed, precision, L, maxD, N, tanh_embed)
    return _nets[key]


def _run(run, precision):
    """(table, net) of a run: Lmax is what the library accepts in this precision"""
    tb = TE.table(run, TSE.lmax(precision) if run[1] == "Lmax" else None)
    return tb, _net(tb.shape, tb.seed, precision, tb.L, tb.maxD, tb.N)


# ---- the three checks, on any net ----------------------------------------------------------------------------------------------------

def _score(net, e, lengths, rows_at, what):
    """scoreSamples of every length (column i mod 3), one of them with rows, within the bar of the reference at every sample; the
    worst error in bars"""
    worst = 0.0
    for i, n in enumerate(lengths):
        c = i % TE.COLUMNS
        if n == rows_at:
            logp, rows = e.scoreSamples([net.req(c, n)], rows=True)[0]
        else:
            logp, rows = e.scoreSamples([net.req(c, n)])[0], None
        worst = max(worst, TS._hold(net, c, n, 1.0, logp, rows, what=what))
    return worst


def _prefill(net, e, lengths, what):
    """Every length through ONE prefillStates call against the column started, primed, stepped (at most D samples a call, in a session
    whose window is the largest dilation) and saved; the window, the blob size and the header words 5, 6, 7."""
    s = net.s
    dil = E.dilations(s.L, s.maxD)
    D, W = max(dil), PF.window(s.L, s.maxD)
    assert e.prefillWindow() == W, (e.prefillWindow(), W)
    assert e.slotStateBytes() == PF.HEADER_BYTES + sum(dil) * s.R * (2 if net.precision == 16 else 4)
    assert len(lengths) <= e.maxBatch - 1
    jobs = [((7 * i + 3) % (e.maxBatch - 1), i % TE.COLUMNS, net.yg[i % TE.COLUMNS, :n].contiguous(), 1.0) for i, n in enumerate(lengths)]
    pre = TP._check_equal(e, net.xg, jobs, D, what).cpu().numpy()
    for i, n in enumerate(lengths):
        words = np.frombuffer(pre[i].tobytes()[:PF.HEADER_BYTES], dtype="<i4")
        assert words[5] == s.maxD and words[6] == n and words[7] == i % TE.COLUMNS, (what, n, words)
        assert words[4] == s.L and words[3] == s.R and words[2] == net.precision, (what, n, words)


class _Watch:
    """an engine whose scoreChunks also shows that no in-state was written: its bytes before the call and after it"""

    def __init__(self, e):
        self.e, self.checked = e, 0

    def scoreChunks(self, reqs, **kw):
        before = [None if r[0] is None else r[0].cpu().numpy().tobytes() for r in reqs]
        out = self.e.scoreChunks(reqs, **kw)
        for r, b in zip(reqs, before):
            if b is not None:
                assert r[0].cpu().numpy().tobytes() == b, "an in-state was written"
                self.checked += 1
        return out


def _chunks(net, e, lists_of, what):
    """lists_of = {n: cut lists}: every list walked from silence with rows and states, three at a time: logp and rows bit for bit those
    of the whole pass, the blob behind every cut byte for byte that of prefillStates of the prefix, the history words of its header,
    and no in-state written."""
    y_host = net.y
    watch = _Watch(e)
    for n, lists in lists_of.items():
        whole = e.scoreSamples([net.req(c, n) for c in range(TE.COLUMNS)], rows=True)
        for g in range(0, len(lists), TE.COLUMNS):
            group = lists[g:g + TE.COLUMNS]
            jobs = [(net.yg[c, :n].contiguous(), net.xg[c], cuts, 1.0, 100 + c) for c, cuts in enumerate(group)]
            got = TC._walk(watch, jobs)
            pre = e.prefillStates([(net.yg[c, :k0 + m].contiguous(), net.xg[c], 100 + c, 1.0) for c, cuts in enumerate(group)
                                   for k0, m in CC.starts(cuts)]).cpu().numpy()
            row = 0
            for c, cuts in enumerate(group):
                logp, rows, blobs = got[c]
                where = "%s n = %d column %d cuts %s" % (what, n, c, cuts[:6])
                assert logp.shape == (n,) and rows.shape == (n, net.s.A), where
                bad = (TC._bits(logp) != TC._bits(whole[c][0])).nonzero().flatten()
                assert bad.numel() == 0, "%s: logp differs from the whole pass first at sample %d" % (where, int(bad[0]))
                assert torch.equal(TC._bits(rows), TC._bits(whole[c][1])), where + ": rows"
                done = 0
                for i, m in enumerate(cuts):
                    done += m
                    TC._same_blob(blobs[i], pre[row + i].tobytes(), "%s, behind sample %d" % (where, done))
                    words = np.frombuffer(blobs[i][:PF.HEADER_BYTES], dtype="<u4")
                    assert int(words[5]) == net.s.maxD and int(words[6]) == done and int(words[7]) == 100 + c, (where, done)
                    assert int(words[8]) == (int(y_host[c, done - 2]) if done >= 2 else 128) and int(words[9]) == int(y_host[c, done - 1]), (where, done)
                row += len(cuts)
    assert watch.checked >= 1


RUN_PARAMS = dict(argnames="run", argvalues=TE.RUNS, ids=TE.run_id)


# ---- 1. scoring against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**RUN_PARAMS)
def test_scores_at_the_edge_schedules_are_within_the_bar_of_the_reference(run, precision):
    tb, net = _run(run, precision)
    e = net.engine()
    worst = _score(net, e, tb.scored, tb.rows_at, tb.what())
    e.close()
    print("TIME_EDGE score %s fp%d: worst |d logp| = %.3f bars" % (tb.what(), precision, worst))


# ---- 2. prefill against the sequentially primed column ------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**RUN_PARAMS)
def test_prefilled_blobs_at_the_edge_schedules_equal_the_sequentially_primed_columns(run, precision):
    """Every prefill length of the table in one call.  The session's window is the largest dilation -- 8 at (4, 512), whose header
    carries maxDilation 512 --; (11, 1024) steps a column through 1 100 samples."""
    tb, net = _run(run, precision)
    e = net.engine()
    _prefill(net, e, tb.prefill, "%s fp%d" % (tb.what(), precision))
    e.close()


# ---- 3. chunks against the whole pass, out-states against prefill --------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**RUN_PARAMS)
def test_chunks_at_the_edge_schedules_equal_the_whole_pass_and_the_prefilled_blobs(run, precision):
    tb, net = _run(run, precision)
    e = net.engine()
    _chunks(net, e, {n: tb.cuts(n) for n in tb.scored}, "%s fp%d" % (tb.what(), precision))
    e.close()


# ---- 4. without the embedding tanh ---------------------------------------------------------------------------------------------------

NO_TANH = {"prime_shape": ("R64", 8, 16, 48), "R32_L5_maxD3": ("R32", 5, 3, 29)}          # shape, L, maxDilation, samples of the lockstep run
NO_TANH_PARAMS = dict(argnames="name", argvalues=sorted(NO_TANH))
_locks = {}


def _lock_modes(precision):
    return ("wg", "wg2", "wg3") if precision == 16 else ("wg", "wg2")


def _no_tanh_lockstep(name, precision):
    """The lockstep features path (RAW = 3, five channels handed over directly, in-kernel selectors) with tanhEmbed = False, held to
    the oracle with set_tanh_embed(False); per organisation the samples.  Once per (name, precision)."""
    key = (name, precision)
    if key not in _locks:
        shape, L, maxD, N = NO_TANH[name]
        R, S, A = E.SHAPES[shape]
        half = precision == 16
        case = cases.Case("notanh_%s" % name, 931 if name == "prime_shape" else TE.seed_of((shape, L, maxD), L), [],
                          cases.Shape(R, S, A, L, 19, N, maxD), 1, 1, 7)
        s = case.shape
        x, w, b = E.feature_model(case, half)
        xg = torch.from_numpy(x).cuda()
        t = util.gen_o1(case, half=half)
        t.Lh = E.feature_lh(case, x, w, b)
        t.sel = O.philox_selectors(TSL.SEED, s.N, s.B)
        y_lock = {}
        for mode in _lock_modes(precision):
            e = TSL._engine(case, t, precision, mode, w, b, s.B, tanh_embed=False)
            e.setFeatures(xg)
            assert "RAW=3" in e.kernelInfo(s.B, True), e.kernelInfo(s.B, True)
            y = np.full((s.B, s.N), -1, dtype=np.int32)
            assert e.run_chunks(case.chunk, None, s.N, s.B, y, 1, True)
            e.synchronize()
            got = util.engine_getters(e, s.L)
            got["y"] = y
            e.close()
            ref = P._teacher_forced_ref(case, t, y, tanh_embed=False)
            if half:
                st = util.fp16_bars(ref, got, t.sel.T, "no tanh, features %s/%s" % (name, mode))
                worst = max(st[k] for k in ("Xout_units", "skipOut_units", "Zs_units", "Za_units")) / util.FP16_K
                print("TIME_EDGE no tanh fp16 features %s %s: worst activation error %.3f of the bar, agreement %.4f" % (name, mode, worst, st["agreement"]))
            else:
                TSE._fp32_bars(ref, got, t.sel.T, s.B)
            y_lock[mode] = y
        _locks[key] = (case, t, w, b, xg, y_lock)
    return _locks[key]


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**NO_TANH_PARAMS)
def test_no_tanh_lockstep_features_path_against_the_oracle(name, precision):
    """4a.  fp32: exact samples and the activation bars of test_schedule_edges_gpu._fp32_bars; fp16: util.fp16_bars; the
    organisations (one, two and -- fp16 -- three tiles per workgroup) bit-identical."""
    case, t, w, b, xg, y_lock = _no_tanh_lockstep(name, precision)
    assert set(y_lock) == set(_lock_modes(precision))
    for mode, y in y_lock.items():
        assert np.array_equal(y, y_lock["wg"]), "wg and %s disagree without the tanh, fp%d" % (mode, precision)


def _steps(r, total, piece):
    while total:
        c = min(piece, total)
        r.step(c)
        total -= c


def _session_modes(precision):
    return ("wg", "wg3") if precision == 16 else ("wg", "wg2")


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**NO_TANH_PARAMS)
def test_no_tanh_slot_sessions_equal_their_lockstep_columns(name, precision):
    """4b.  Joins at counters 0 and 1 in both tiles, one utterance suspended in the second tile and resumed in the first a sample on;
    the window is the largest dilation.  Every utterance equals its lockstep column."""
    case, t, w, b, xg, y_lock = _no_tanh_lockstep(name, precision)
    s = case.shape
    D = TE.largest_dilation(s.L, s.maxD)
    for mode in _session_modes(precision):
        e = TSL._engine(case, t, precision, mode, w, b, s.B, tanh_embed=False)
        cols = e.maxBatch
        r = Run(e, xg, D)
        r.start(0, 0)
        r.start(cols - 2, 1)
        r.step(1)                                  # counter 1
        r.start(5, 2)
        r.start(cols - 3, 3)
        _steps(r, 9, D)
        blob, rec = r.suspend(cols - 2)            # the second tile, done = 10
        assert 0 < rec[2] < rec[3]
        r.step(1)
        r.resume(2, blob, rec)                     # the first tile, another counter
        k = 0
        while r.cols:
            r.step((D, 1)[k % 2])
            k += 1
        e.slotsEnd()
        e.close()
        r.check(y_lock[mode], "no tanh %s fp%d %s" % (name, precision, mode))
        assert len(r.got) == 4 and all(len(np.concatenate(v)) == s.N for v in r.got.values())


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**NO_TANH_PARAMS)
def test_no_tanh_primed_columns_continue_their_lockstep_samples(name, precision):
    """4c.  Columns of both tiles primed with the first half of their own lockstep samples deliver those and continue them bit for
    bit."""
    case, t, w, b, xg, y_lock = _no_tanh_lockstep(name, precision)
    s = case.shape
    D = TE.largest_dilation(s.L, s.maxD)
    for mode in _session_modes(precision):
        e = TSL._engine(case, t, precision, mode, w, b, s.B, tanh_embed=False)
        r = Run(e, xg, D)
        r.start(7, 6)                              # (unprimed, started a sample earlier)
        r.step(1)
        for col, uid in ((3, 4), (e.maxBatch - 1, 5)):
            r.start(col, uid)
            e.slotPrime(col, torch.from_numpy(np.ascontiguousarray(y_lock[mode][uid, :s.N // 2])).cuda())
            assert e.slotPrimed(col) == s.N // 2
        while r.cols:
            r.step(D)
        e.slotsEnd()
        e.close()
        r.check(y_lock[mode], "no tanh, primed, %s fp%d %s" % (name, precision, mode))
        assert len(r.got) == 3 and all(len(np.concatenate(v)) == s.N for v in r.got.values())


NO_TANH_LENGTHS = (1, 2, 17, 47, 48)
NO_TANH_CUTS = [(1, 47), (17, 31), TE.fives(48)]


def _no_tanh_net(name, precision, tanh_embed=False):
    if name == "prime_shape":
        shape, seed, L, maxD, N = SC.PRIME_SHAPE
    else:
        shape, seed, L, maxD, N = E.SHAPES["R32"], TE.seed_of(("R32", 5, 3), 5), 5, 3, 48
    return _net(shape, seed, precision, L, maxD, N, tanh_embed)


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**NO_TANH_PARAMS)
def test_no_tanh_scores_prefill_and_chunks(name, precision):
    """4d.  Tests 1, 2 and 3 on one engine built with tanhEmbed = False -- time_embed_kernel's other branch, and blobs whose layer-0
    slot holds an embedding sum that was never squashed --, against the reference with tanh_embed=False."""
    net = _no_tanh_net(name, precision)
    what = "no tanh %s fp%d" % (name, precision)
    e = net.engine()
    worst = _score(net, e, NO_TANH_LENGTHS, 47, what)
    print("TIME_EDGE score %s: worst |d logp| = %.3f bars" % (what, worst))
    _prefill(net, e, NO_TANH_LENGTHS, what)
    _chunks(net, e, {48: NO_TANH_CUTS}, what)
    e.close()


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize(**NO_TANH_PARAMS)
def test_the_prefilled_blob_sees_the_tanh_flag(name, precision):
    """4e, the control.  One prime on engines with and without the tanh, the same weights: the same header, another layer-0 slot (the
    first row behind the header is x_0 of the last sample, the embedding sum itself)."""
    net = _no_tanh_net(name, precision)
    row = net.s.R * (2 if precision == 16 else 4)
    blobs = []
    for flag in (False, True):
        e = net.engine(tanh_embed=flag)
        blobs.append(e.prefillStates([(net.yg[0, :17].contiguous(), net.xg[0], 3, 1.0)]).cpu().numpy()[0].tobytes())
        e.close()
    H = PF.HEADER_BYTES
    assert blobs[0][:H] == blobs[1][:H]
    assert blobs[0][H:H + row] != blobs[1][H:H + row], "the layer-0 slot does not depend on the tanh flag"
    plain = np.frombuffer(blobs[0][H:H + row], dtype=np.float16 if precision == 16 else np.float32)
    assert np.abs(plain.astype(np.float64)).max() > 1.0, "no element of the unsquashed embedding sum is outside tanh's range"


# ---- 5. from mel frames --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize("L,maxD", [(2, 1), (5, 3)])
def test_prefill_and_chunks_from_mel_at_short_windows(L, maxD, precision):
    """R 32 at the hop 8 / 2 of mel_time_cases.  W = 4 and 9: primes of 36 and 48 samples start the pass at t0 = 32 (16 at (5, 3),
    n = 36) -- prefillStatesMel upsamples from there, reading frames in front of t0, a range of 4 to 20 samples -- and give byte for
    byte the blobs of prefillStates fed the lockstep-upsampled rows of the same frames.  One scoreChunksMel walk with the cuts
    (5, 16, 27) equals scoreSamplesMel bit for bit, its out-states the blobs of prefillStatesMel."""
    hop = MT.PRIME_HOPS[0]
    assert hop == (8, 2)
    lengths = (36, 48)
    t0 = [PF.first_tile_sample(n, L, maxD) for n in lengths]
    assert t0 == ([32, 32] if L == 2 else [16, 32])
    assert [n - a for n, a in zip(lengths, t0)] == ([4, 16] if L == 2 else [20, 16])          # (4: a range shorter than a tile)
    ms = TM.MelSetup(E.SHAPES["R32"], TE.seed_of(("R32", L, maxD), L), precision, hop, L, maxD, 48, TE.COLUMNS)
    x = ms.lock()                                  # [columns][n_cond][48], T_data
    e = ms.engine()
    assert e.prefillWindow() == PF.window(L, maxD)
    jobs = [(ms.yg[c, :n].contiguous(), c, 20 + c) for c, n in zip((1, 2), lengths)]
    pre = e.prefillStatesMel([(y, ms.melg[c], uid, 1.0) for y, c, uid in jobs])
    via = e.prefillStates([(y, x[c], uid, 1.0) for y, c, uid in jobs])
    for i, n in enumerate(lengths):
        diff = TP._first_difference(via[i].cpu().numpy().tobytes(), pre[i].cpu().numpy().tobytes())
        assert diff is None, "(%d, %d) fp%d n = %d: prefillStatesMel differs from prefillStates fed the lockstep rows: %s" % (L, maxD, precision, n, diff)
    cuts = (5, 16, 27)
    y = ms.yg[0, :48].contiguous()
    logp, rows, blobs = TC._walk(e, [(y, ms.melg[0], cuts, 1.0, 60)], mel=True)[0]
    whole = e.scoreSamplesMel([(y, ms.melg[0], 1.0)], rows=True)[0]
    assert torch.equal(TC._bits(logp), TC._bits(whole[0])) and torch.equal(TC._bits(rows), TC._bits(whole[1])), (L, maxD, precision)
    want = e.prefillStatesMel([(ms.yg[0, :k0 + m].contiguous(), ms.melg[0], 60, 1.0) for k0, m in CC.starts(cuts)]).cpu().numpy()
    for i in range(len(cuts)):
        TC._same_blob(blobs[i], want[i].tobytes(), "(%d, %d) fp%d from mel, behind cut %d" % (L, maxD, precision, i))
    e.close()
