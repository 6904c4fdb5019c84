"""CPU tests of the rows, mirrors and wrong rules of tests/sampler_cases.py (no GPU), which tests/test_sampler_primitives_gpu.py holds
softmax_pick's floored and cutting forms to: the crafted rows are what they say, different in every utterance of a launch and
clear of rounding, so that the float64 comparison on the GPU may leave no row out; the three statements of the threshold agree on
them; every wrong rule changes a threshold, a kept set or a pick on them; the scan's mirror answers the last kept bin where it
falls off the end; and what the mirror predicts for the selectors next to 1 is printed."""
import numpy as np
import pytest

import cut_cases as CC
import sampler_cases as S

F32 = np.float32
LAYOUTS = [(A, 4 * nw) for A, nw in S.PAIRS] + [(256, 4)]           # (A, LPU); LPU = 4 is allowed by softmax_pick, built by no kernel


def _cut(row, e, LPU, form=2, mutate=None):
    """e behind form 1 (the floor alone) or a cutting form"""
    k, p = (row.k, row.p) if form >= 2 else (0, 1.0)
    return S.cut_e(e, k, p, row.tau, LPU, mutate)


@pytest.mark.parametrize("A,LPU", LAYOUTS)
def test_the_crafted_rows_are_what_they_say(A, LPU):
    rows = S.crafted(A, LPU)
    RPL = A // LPU
    assert len(rows) >= 32 and len({r.name for r in rows}) == len(rows)
    for at in range(0, len(rows), 16):
        settings = [r.setting for r in rows[at:at + 16]]
        assert len(set(settings)) == 16, "two utterances of one launch share their settings: %s" % (settings,)
    assert {r.T for r in rows} == {0.5, 1.0, 2.0}
    for r in rows:
        assert r.logits.dtype == F32 and r.logits.shape == (A,) and 0 <= r.k <= A and 0.0 <= r.p <= 1.0 and 0.0 <= r.tau <= 0.5
        e = S.e_of(r.logits, r.T)
        # no e is a denormal: whether the device flushes them would otherwise decide a kept set
        assert ((e == 0) | (e >= np.finfo(F32).tiny)).all(), r.name
        got = np.nonzero(_cut(r, e, LPU) > 0)[0]
        assert np.array_equal(got, r.keep), (r.name, got.tolist(), r.keep.tolist())
        assert np.array_equal(np.nonzero(kept64_where_e(r, e))[0], r.keep), r.name
    by = {r.name: r for r in rows}
    tied = by["five bit-equal bins at ranks 2 to 6 across lanes, quads and halves, k = 3"]
    spots = S.tie_spots(LPU, RPL)
    assert len(set(spots)) == 5 and spots[0] == RPL - 1 and spots[1] == RPL and len(set(tied.logits[spots])) == 1
    lanes = sorted({s // RPL for s in spots})
    assert len(lanes) >= min(LPU, 5) - (LPU == 4)
    if LPU == 16:
        assert lanes == [0, 1, 2, 5, 11]                             # both pairs of a quad, two quads, both halves of the row
    desc = np.sort(tied.logits)[::-1]
    assert desc[0] > desc[1] == desc[5] > desc[6]
    point = by["a point mass, the rest underflows to e = 0, k = 32"]
    e = S.e_of(point.logits, point.T)
    assert (e > 0).sum() == 1 and e[0] == 0 and e[77] > 0
    for sel in S.SELECTORS:                                                 # sel = 0 with bin 0 dropped: the pick is the peak
        assert S.scan_pick(_cut(point, e, LPU), sel, LPU, floored=True)[0] == 77
    tiny = by["p = 1e-40: the maximum alone"]
    e = S.e_of(tiny.logits, tiny.T)
    assert 0 < F32(tiny.p) < np.finfo(F32).tiny
    zero = by["p = 1e-46, zero in float32: the bound p S(0) is zero, the maximum alone"]
    assert F32(zero.p) * CC.group_sum(e, LPU) == 0
    for r in (tiny, zero):
        assert CC.bisect_threshold(e, 0, r.p, LPU) == CC.search_from_the_top(e, 0, r.p, LPU) == e.max()
    every_other = by["kept bins in every other lane (odd), k = LPU / 2"]
    lane_sums = _cut(every_other, S.e_of(every_other.logits, every_other.T), LPU).reshape(LPU, RPL).sum(axis=1)
    assert (lane_sums[0::2] == 0).all() and (lane_sums[1::2] > 0).all()


def kept64_where_e(row, e):
    """the float64 kept set on the bins that have an e at all in float32 (a bin whose e underflows has no mass to keep or drop)"""
    return S.kept64(row.logits, row.k, row.p, row.tau, row.T) & (e > 0)


@pytest.mark.parametrize("A,LPU", LAYOUTS)
def test_every_crafted_row_is_clear_of_rounding(A, LPU):
    """100 delta, delta the bound cut_cases.py derives for the distance between the kernel's float32 decision and a float64 one."""
    worst = (np.inf, None)
    for r in S.crafted(A, LPU):
        dist, need = S.clearance(r, A)
        assert dist >= need, (r.name, dist, need)
        worst = min(worst, (dist / need, r.name))
    print("A %d LPU %d: the closest row is %.1f x 100 delta from a decision (%s)" % (A, LPU, worst[0], worst[1]))


@pytest.mark.parametrize("A,LPU", LAYOUTS)
def test_the_three_statements_of_the_threshold_agree_on_the_crafted_rows(A, LPU):
    for r in S.crafted(A, LPU):
        e = S.e_of(r.logits, r.T)
        want = CC.sorted_threshold(e, r.k, r.p, LPU)
        assert CC.bisect_threshold(e, r.k, r.p, LPU) == want and CC.search_from_the_top(e, r.k, r.p, LPU) == want, r.name
        assert S.threshold(e, r.k, r.p, r.tau, LPU) == max(want, F32(r.tau)), r.name


def _rejections(A, LPU, mutation):
    """the crafted rows (and selectors) on which the wrong rule gives another threshold, kept set or pick than the right one"""
    out = []
    for r in S.crafted(A, LPU):
        e = S.e_of(r.logits, r.T)
        if mutation == "exact_prefix":
            ec = _cut(r, e, LPU)
            for sel in S.SELECTORS:
                if S.scan_pick(ec, sel, LPU, True, mutation)[0] != S.scan_pick(ec, sel, LPU, True)[0]:
                    out.append((r.name, sel))
        elif not np.array_equal(_cut(r, e, LPU, 2, mutation), _cut(r, e, LPU)):
            out.append((r.name, None))
    return out


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_a_wrong_rule_differs_on_the_crafted_rows(mutation):
    """Negative controls: cnt > kneed keeps one bin more; e > t drops the ties at the boundary; the smaller of the two thresholds
    is the union of the cuts; the floor ignored under a cut; the search from the top without cnt > 0 runs away when the bound
    p S(0) is zero; running sums restarted from the neighbour's inclusive sum are other sums than incl - lsum gives."""
    for A, LPU in LAYOUTS:
        got = _rejections(A, LPU, mutation)
        print("%s, A %d LPU %d: differs on %d: %s" % (mutation, A, LPU, len(got), sorted({n for n, _ in got})[:4]))
        assert got, (mutation, A, LPU)


def test_the_scan_answers_the_kept_bin_below_where_it_falls_off_or_stops_on_a_dropped_bin():
    e = np.zeros((3, 256), dtype=F32)
    e[0, [3, 40, 41]] = [1.0, 0.5, 0.25]
    e[1, 255] = 1.0
    e[2] = 1.0
    for LPU in (4, 8, 16):
        pick, total = S.scan_pick(e, 1.5, LPU, floored=True)             # a selector beyond the total: every scan falls off
        assert pick.tolist() == [41, 255, 255] and total.tolist() == [1.75, 1.0, 256.0]
        assert S.scan_pick(e, 1.5, LPU)[0].tolist() == [128, 128, 128]   # the plain form keeps the reference's answer
        assert S.falls_off(e, 1.5, LPU).all() and not S.falls_off(e, 0.5, LPU).any()
        assert S.scan_pick(e, 0.0, LPU, floored=True)[0].tolist() == [3, 255, 0]
        assert S.scan_pick(e[0], 0.6, LPU, floored=True) == (40, F32(1.75))


def test_what_the_mirror_predicts_for_the_selectors_next_to_one():
    """Printed, not asserted: on 1 500 rows of N(0, 2.5^2) logits with the k largest e kept, how often the scan's mirror falls off
    the end at the three selectors next to 1 -- before the forms with a floor or a cut answered the last kept bin, each of
    these was a draw of 128, a bin the cut had dropped."""
    rng = np.random.default_rng(1)
    for A, LPU in ((256, 16), (256, 8), (512, 16), (1024, 16)):
        e = S.e_of(rng.normal(0.0, 2.5, (1500, A)).astype(F32), 1.0)
        for k in (1, 2, 4, 32):
            kth = np.sort(e, axis=1)[:, -k][:, None]
            ek = np.where(e >= kth, e, F32(0))
            off = [int(S.falls_off(ek, sel, LPU).sum()) for sel in S.TOP]
            dropped = [int(S.stops_on_a_dropped_bin(ek, sel, LPU).sum()) for sel in S.TOP]
            print("A %4d LPU %2d k %2d, of 1500 rows at 1 - 2^-22 / 2^-23 / 2^-24: the scan falls off in %4d / %4d / %4d, stops on a dropped "
                  "bin in %4d / %4d / %4d" % ((A, LPU, k) + tuple(off) + tuple(dropped)))
            for sel in S.TOP:
                pick, _ = S.scan_pick(ek, sel, LPU, floored=True)
                assert (ek[np.arange(len(ek)), pick] > 0).all()           # with the kept bin below as the answer, every draw is kept
