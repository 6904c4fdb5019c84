"""CPU tests for tests/test_time_edges_gpu.py (no GPU; cases: tests/time_edge_cases.py): the float64 reference of tests/score_cases.py
is held to the committed oracle, teacher-forced, at every edge schedule -- with and without the embedding tanh --, and the inputs of the
GPU tests are shown to tell: a reference with another schedule or with the tanh flag flipped moves some log-probability by many bars,
a blob laid out by another schedule differs at every prefill length, and the wrong carry rules of tests/score_carry_cases.py differ
from the whole pass on the cut lists the GPU tests walk."""
import copy

import numpy as np
import pytest

import cases
import prefill_cases as PF
import schedule_edges as E
import score_carry_cases as CC
import score_cases as SC
import time_edge_cases as TE
import util
from test_score_carry_cpu import _walk, _xs
from test_score_cpu import _network, _oracle_at

L_CPU = E.L_MAX           # "Lmax" here: no GPU decides it
NO_TANH = [("prime_shape", SC.PRIME_SHAPE), ("R32_L5_maxD3", ((32, 128, 256), TE.seed_of(("R32", 5, 3), 5), 5, 3, 48))]
_inputs = {}


def _run_inputs(run):
    """(table, case, t with t.Lh, Lh per column float64, y [columns][N]) of a run, once"""
    if run not in _inputs:
        tb = TE.table(run, L_CPU)
        _inputs[run] = (tb,) + _network(tb.shape, tb.seed, tb.L, tb.maxD, tb.N, TE.COLUMNS)
    return _inputs[run]


def _hold_to_oracle(case, t, lh, y, n, at, oracle_at, what, **kw):
    """reference against oracle at the samples `at`, logits and log-probability within the fp32 bar; returns the worst |d logp| in bars"""
    columns = y.shape[0]
    refs = [SC.reference(t, case.shape, y[c, :n], lh[c].astype(np.float32), **kw) for c in range(columns)]
    worst = 0.0
    for k in at:
        o = oracle_at(case, t, y, k)
        for c in range(columns):
            Za, logp = refs[c]
            top = np.abs(Za).max()
            dz = np.abs(o["Za"][c] - Za[k]).max()
            assert dz <= (cases.TOL["Za"] + 32 * SC.EPS32) * top, (what, k, c, dz)
            dl = abs(np.log(np.float64(o["P"][c, y[c, k]])) - logp[k])
            worst = max(worst, dl / SC.bar(Za, 1.0, 32))
            assert dl <= SC.bar(Za, 1.0, 32), (what, k, c, dl, SC.bar(Za, 1.0, 32))
    return worst


# ---- 1. the reference at every run ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", TE.RUNS, ids=TE.run_id)
def test_the_float64_reference_matches_the_teacher_forced_oracle_at_the_edge_schedules(run):
    """Within the fp32 bar of tests/test_score_cpu.py, logits and log-probability of the forced sample, at 0, 1, 2, 15, 16, 17, n - 1 and
    D - 1, D, D + 1 (D the largest dilation) of all N samples; Lmax is kMaxLayers = 128 here."""
    tb, case, t, lh, y = _run_inputs(run)
    worst = _hold_to_oracle(case, t, lh, y, tb.N, tb.positions(tb.N), _oracle_at, tb.what())
    print("float64 reference against the oracle, %s, n = %d: worst |d logp| = %.3g bars (fp32)" % (tb.what(), tb.N, worst))


# ---- 2. without the embedding tanh ---------------------------------------------------------------------------------------------------

def _oracle_at_no_tanh(case, t, y, k):
    """test_score_cpu._oracle_at on the oracle that does not squash the embedding sum"""
    ck = case._replace(shape=case.shape._replace(N=k + 1))
    tk = copy.copy(t)
    tk.Lh, tk.sel = np.ascontiguousarray(t.Lh[:k + 1]), np.ascontiguousarray(t.sel[:k + 1])
    return util.teacher_forced_oracle(ck, tk, np.ascontiguousarray(y[:, :k + 1]), tanh_embed=False)


@pytest.mark.parametrize("name,spec", NO_TANH, ids=[n for n, _ in NO_TANH])
def test_the_reference_without_the_embedding_tanh_matches_that_oracle(name, spec):
    shape, seed, L, maxD, N = spec
    case, t, lh, y = _network(shape, seed, L, maxD, N, TE.COLUMNS)
    D = TE.largest_dilation(L, maxD)
    at = sorted(set(SC.positions(N)) | {k for k in (D - 1, D, D + 1) if k < N})
    worst = _hold_to_oracle(case, t, lh, y, N, at, _oracle_at_no_tanh, name, tanh_embed=False)
    print("float64 reference without the tanh against the oracle, %s: worst |d logp| = %.3g bars (fp32)" % (name, worst))


# ---- 3. negative controls ------------------------------------------------------------------------------------------------------------

def _wide_bar(Za):
    return max(SC.bar(Za, 1.0, 16), SC.bar(Za, 1.0, 32))


@pytest.mark.parametrize("run", TE.RUNS, ids=TE.run_id)
def test_a_reference_with_another_schedule_misses_by_more_than_ten_bars(run):
    """maxDilation doubled (1024: halved): where that is another schedule, some logp of the scored request moves by more than ten bars
    of BOTH precisions -- a pass that walked the wrong schedule would not stay within one.  Where it is the same schedule -- (2, 2),
    (3, 4) and (4, 512) never reach their maxDilation -- the reference does not move at all."""
    tb, case, t, lh, y = _run_inputs(run)
    wrong = tb.wrong_maxD()
    other = case.shape._replace(maxD=2 * tb.maxD if wrong is None else wrong)
    moved = 0.0
    for c in range(TE.COLUMNS):
        Za, logp = SC.reference(t, case.shape, y[c], lh[c])
        _, bad = SC.reference(t, other, y[c], lh[c])
        if wrong is None:
            assert np.array_equal(bad, logp), tb.what()
        moved = max(moved, float(np.abs(bad - logp).max() / _wide_bar(Za)))
    print("%s: maxDilation %d in place of %d moves logp by %.1f fp16 bars" % (tb.what(), other.maxD, tb.maxD, moved))
    assert (moved > 10) == (wrong is not None), (tb.what(), moved)


@pytest.mark.parametrize("name,spec", NO_TANH, ids=[n for n, _ in NO_TANH])
def test_the_embedding_tanh_moves_the_reference_by_more_than_five_bars(name, spec):
    shape, seed, L, maxD, N = spec
    case, t, lh, y = _network(shape, seed, L, maxD, N, TE.COLUMNS)
    Za, logp = SC.reference(t, case.shape, y[0], lh[0], tanh_embed=False)
    _, with_tanh = SC.reference(t, case.shape, y[0], lh[0])
    moved = float(np.abs(with_tanh - logp).max() / _wide_bar(Za))
    print("%s: the embedding tanh moves logp by %.1f fp16 bars" % (name, moved))
    assert moved > 5, (name, moved)


@pytest.mark.parametrize("run", TE.RUNS, ids=TE.run_id)
def test_a_blob_laid_out_by_another_schedule_differs_at_every_prefill_length(run):
    """prefill_cases.blob_payload of the same x_l under the run's schedule and under the doubled (halved) maxDilation: another size or
    other rows at every prefill length of the table, where the schedules differ."""
    tb = TE.table(run, L_CPU)
    wrong = tb.wrong_maxD()
    if wrong is None:
        assert PF.schedule(tb.L, 2 * tb.maxD) == PF.schedule(tb.L, tb.maxD)
        return
    xs = _xs(tb.L, tb.N)
    for n in tb.prefill:
        a, b = PF.blob_payload(xs, n, tb.L, tb.maxD), PF.blob_payload(xs, n, tb.L, wrong)
        assert a.shape != b.shape or not np.array_equal(a, b), (tb.what(), n)


@pytest.mark.parametrize("run", TE.RUNS, ids=TE.run_id)
def test_the_wrong_carry_rules_differ_on_the_cut_lists_of_every_run(run):
    """The mutations of tests/score_carry_cases.py on this run's cut lists: the history taken from the chunk itself differs from the whole
    pass at every run; slots indexed by the chunk-relative sample and the tap slot taken from rp differ wherever a dilation above 1
    meets a chunk that does not start at a multiple of it -- every run with D > 1, through the cut (1, n - 1) or a cut at 17.  Dropping
    the old slots can matter only where a chunk WITH an in-state is shorter than a dilation (time_edge_cases.keeps_old_slots): that is
    so at D >= 4 (the fives' rest, the cuts of 300) and at (128, 2) (the rest of 1 after 42 fives); it cannot matter at D = 1 (no n is
    below 1), nor on the cut lists of (2, 2), (5, 3) and of an odd layer count at (Lmax, 2), whose chunks behind the first all hold two
    samples or more -- there the mutation is shown to change nothing instead."""
    tb = TE.table(run, L_CPU)
    xs = _xs(tb.L, tb.N)
    y = PF.primes(1, tb.N, 256)[0]
    sched = PF.schedule(tb.L, tb.maxD)
    lists = [cuts for n in tb.scored for cuts in tb.cuts(n)]
    want = {}

    def payload(done):
        if done not in want:
            want[done] = PF.blob_payload(xs, done, tb.L, tb.maxD)
        return want[done]

    hit = dict.fromkeys(CC.MUTATIONS, 0)
    for cuts in lists:
        for done, p in _walk(xs, cuts, tb.L, tb.maxD):
            assert np.array_equal(p, payload(done)), (tb.what(), cuts, done)          # (the right rule, at these schedules too)
        for m in ("relative_slots", "drop_old"):
            hit[m] += any(not np.array_equal(p, payload(done)) for done, p in _walk(xs, cuts, tb.L, tb.maxD, m))
        tap, hist_bad, hist = False, False, (128, 128)
        for k0, n in CC.starts(cuts):
            for l, (d, off) in enumerate(sched):
                for k in range(k0, min(k0 + n, k0 + d)):
                    want_x = xs[l][k - d] if k - d >= 0 else None
                    good = CC.tap_source(l, k, k0, tb.L, tb.maxD, have_state=k0 > 0)
                    if good[0] == "slot":
                        assert np.array_equal(payload(k0)[good[1]], want_x), (tb.what(), cuts, k0, l, k)
                    bad = CC.tap_source(l, k, k0, tb.L, tb.maxD, have_state=k0 > 0, mutate="tap_from_rp")
                    tap = tap or (bad[0] == "slot" and not np.array_equal(payload(k0)[bad[1]], want_x))
            for r in range(min(n, 2)):
                k = k0 + r
                whole = (int(y[k - 2]) if k >= 2 else 128, int(y[k - 1]) if k >= 1 else 128)
                assert CC.embed_history(r, y[k0:k0 + n], hist) == whole
                hist_bad = hist_bad or CC.embed_history(r, y[k0:k0 + n], hist, mutate="own_history") != whole
            hist = CC.history_after(y[k0:k0 + n], hist)
        hit["tap_from_rp"] += tap
        hit["own_history"] += hist_bad
    print("%s: the mutations differ on %s of %d cut lists" % (tb.what(), hit, len(lists)))
    assert hit["own_history"] >= 1, tb.what()
    assert (hit["relative_slots"] >= 1) == (tb.D > 1) and (hit["tap_from_rp"] >= 1) == (tb.D > 1), (tb.what(), hit)
    assert (hit["drop_old"] >= 1) == TE.keeps_old_slots(tb), (tb.what(), hit)
    if tb.D >= 4 or tb.L == 128:
        assert TE.keeps_old_slots(tb), tb.what()
