"""Rows, float32 mirrors and deliberately wrong rules for the tests of softmax_pick's floored and cutting forms in isolation
(tests/test_sampler_primitives_cpu.py, tests/test_sampler_primitives_gpu.py; wn_kernels.hpp: softmax_pick<.., FLOOR = 1, 2, 3>,
cut_threshold, cut_threshold_dump).

THE SCAN.  scan_pick mirrors, in float32 and in the kernel's order of operations, what softmax_pick does behind the flooring: every
lane sums its RPL values of e in row order; the lane sums go through the inclusive row_shr 1 / 2 / 4 / 8 scan; the total is the
largest prefix sum; a lane's running sum starts at incl - lsum and takes its rows one by one; the pick is the first row, over the
lanes, whose running sum exceeds sel * total.  When no row does, the scan has fallen off the end: the plain form answers 128 (the
reference's behaviour).  incl - lsum is the exclusive prefix only up to rounding, so at the selectors next to 1 the scan may also
stop on the first row of a lane behind the last kept one, a bin the cut dropped.  The floored and cutting forms answer, in both
cases, the highest kept row (e > 0) below the row the scan stopped on -- the last kept bin when it fell off.

THE THRESHOLD is cut_cases.sorted_threshold (the definition by a sort, with S in the kernel's order: cut_cases.group_sum); the
kept set is e >= max(threshold, floor).

CRAFTED ROWS.  crafted(A, LPU) builds, for any lane layout, the rows at which a kernel of this kind goes wrong: exact ties at the
k-th place that straddle two lanes, two quads and the two halves of a DPP row, uniform rows, point masses whose rest underflows,
cuts that keep one lane only or every other lane, a top-p whose bound rounds to zero.  Every row has its own (k, p, tau, T), the
settings of the 16 rows of a launch are all different, and the row is built as T * log(e wanted), so that the tempered e is the
one the row's name describes.  Every row is CLEAR OF ROUNDING (clearance, asserted by the CPU test): its kept set is the same in
float64 and in the kernel's float32, so the GPU test may compare the two on every row.

MUTATIONS.  Wrong rules, each what a kernel that made the mistake would compute; the CPU test shows that every one changes a
threshold, a kept set or a pick on the crafted rows, so the GPU equalities can tell."""
import numpy as np

import cut_cases as CC

F32 = np.float32
PAIRS = [(256, 4), (256, 2), (512, 4), (1024, 4)]         # (A, waves): every softmax lane layout a generation kernel is built with
LOG2E = F32(1.44269504088896340736)
TOP = (1.0 - 2.0 ** -22, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -24)
SELECTORS = (0.0, 2.0 ** -24, 0.37) + TOP

MUTATIONS = ("count_gt", "ties_drop", "union", "floor_ignored", "mass_without_count", "exact_prefix")


def scale_of(T):
    """log2(e) / T in float32: the scale softmax_pick takes"""
    return (LOG2E / np.asarray(T, dtype=F32)).astype(F32)


def e_of(logits, T):
    """a stand-in for the device's e = exp2(fma(x, c, -(m c))) [.., A] float32 for the CPU tests: the fma and the exp2 in float64,
    rounded once each (v_exp_f32 may differ in the last bit; bit-equal logits give bit-equal e either way)"""
    x = np.asarray(logits, dtype=F32)
    c = scale_of(T)[..., None] if np.ndim(T) else scale_of(T)
    mneg = (-x.max(axis=-1, keepdims=True) * c).astype(F32)
    arg = (x.astype(np.float64) * np.float64(c) + mneg.astype(np.float64)).astype(F32)
    return np.exp2(arg.astype(np.float64)).astype(F32)


# ---- the scan ----------------------------------------------------------------------------------------------------------------------

def _scan(e, sel, LPU, mutate=None):
    """(first row whose running sum exceeds the target or A, total) of e [n][A] float32 and sel [n]"""
    e = np.asarray(e, dtype=F32)
    n, A = e.shape
    RPL = A // LPU
    v = e.reshape(n, LPU, RPL)
    lsum = np.zeros((n, LPU), dtype=F32)
    for i in range(RPL):
        lsum = lsum + v[:, :, i]
    incl = lsum.copy()
    for o in (1, 2, 4, 8):
        if o < LPU:
            up = incl[:, :-o].copy()
            incl[:, o:] = incl[:, o:] + up
    total = incl.max(axis=1)
    target = np.asarray(sel, dtype=F32) * total
    cum = incl - lsum
    if mutate == "exact_prefix":                          # every lane starts from its left neighbour's inclusive sum
        cum = np.concatenate([np.zeros((n, 1), dtype=F32), incl[:, :-1]], axis=1)
    assert lsum.dtype == incl.dtype == target.dtype == cum.dtype == F32
    first = np.zeros((n, LPU), dtype=np.int64)
    for i in range(RPL):
        cum = cum + v[:, :, i]
        first += cum <= target[:, None]
    cand = np.where(first < RPL, np.arange(LPU)[None, :] * RPL + first, A)
    return cand.min(axis=1), total


def scan_pick(e, sel, LPU, floored=False, mutate=None):
    """(pick, total) of softmax_pick's scan on e [A] or [n][A] float32 (after the flooring) with selector(s) sel.  floored: the
    forms with a floor or a cut, which answer the highest kept bin below the scan's row when the scan falls off the end or stops
    on a dropped bin (and the scan's row when nothing is kept below it); the plain form answers 128 when the scan falls off."""
    e = np.asarray(e, dtype=F32)
    one = e.ndim == 1
    e2 = e[None, :] if one else e
    n, A = e2.shape
    sel = np.broadcast_to(np.asarray(sel, dtype=F32), (n,))
    raw, total = _scan(e2, sel, LPU, mutate)
    if floored:
        below = (e2 > 0) & (np.arange(A)[None, :] < raw[:, None])
        last = A - 1 - np.argmax(below[:, ::-1], axis=1)
        bad = (raw == A) | (e2[np.arange(n), np.minimum(raw, A - 1)] == 0)
        pick = np.where(bad & below.any(axis=1), last, np.minimum(raw, A - 1))
    else:
        pick = np.where(raw < A, raw, 128)
    return (int(pick[0]), F32(total[0])) if one else (pick, total)


def falls_off(e, sel, LPU):
    """[n] bool: no running sum of e [n][A] exceeds sel * total"""
    e = np.asarray(e, dtype=F32)
    return _scan(e, np.broadcast_to(np.asarray(sel, dtype=F32), (len(e),)), LPU)[0] == e.shape[1]


def stops_on_a_dropped_bin(e, sel, LPU):
    """[n] bool: the scan of e [n][A] does not fall off, and the row it stops on has e = 0: the first row of a lane whose running
    sum starts, by the rounding of incl - lsum, above a target that the lanes before it had not reached"""
    e = np.asarray(e, dtype=F32)
    raw = _scan(e, np.broadcast_to(np.asarray(sel, dtype=F32), (len(e),)), LPU)[0]
    return (raw < e.shape[1]) & (e[np.arange(len(e)), np.minimum(raw, e.shape[1] - 1)] == 0)


# ---- the threshold and the kept set, with the wrong rules --------------------------------------------------------------------------

def threshold(e, k, p, tau, LPU, mutate=None):
    """the threshold the column floors at: max(theta_k, theta_p, tau) of e [A] float32 by the definition
    (cut_cases.sorted_threshold), or what one of MUTATIONS makes of it"""
    e = np.asarray(e, dtype=F32)
    A = len(e)
    if mutate == "count_gt":                              # cnt > kneed: the (k + 1)-th largest
        th_k = np.sort(e)[::-1][k] if 0 < k < A else F32(0)
        cut = max(th_k, CC.sorted_threshold(e, 0, p, LPU))
    elif mutate == "union":                               # the smaller of the two thresholds; an off cut's is 0
        cut = min(CC.sorted_threshold(e, k, 1.0, LPU), CC.sorted_threshold(e, 0, p, LPU))
    elif mutate == "mass_without_count" and p < 1.0 and F32(p) * CC.group_sum(e, LPU) == 0:
        # the search from the top with a bound of zero: the mass predicate holds at every pattern, the search ends at 0x7fffffff,
        # and fmaxf of that NaN and the floor is the floor
        return F32(tau)
    else:
        cut = CC.sorted_threshold(e, k, p, LPU)
    if mutate == "floor_ignored" and (k > 0 or p < 1.0):
        return F32(cut)
    return max(F32(cut), F32(tau))


def cut_e(e, k, p, tau, LPU, mutate=None):
    """e [A] float32 with the bins below the threshold zeroed: what the floored and cutting forms sum, scan and hand back"""
    e = np.asarray(e, dtype=F32)
    thr = threshold(e, k, p, tau, LPU, mutate)
    keep = e > thr if mutate == "ties_drop" else e >= thr
    return np.where(keep, e, F32(0))


# ---- the rule in float64 -----------------------------------------------------------------------------------------------------------

def kept64(logits, k, p, tau, T):
    """[A] bool: the kept set of one row by sorting in float64 -- the k-th largest with its ties, the smallest prefix whose mass
    reaches p, the floor relative to the maximum, and the intersection of the three (cut_cases.kept on the tempered logits)"""
    return CC.kept(np.asarray(logits, dtype=np.float64)[None, :] / float(T), int(k), float(F32(p)), float(F32(tau)))[0]


def clearance(row, A):
    """(smallest distance of the row from a decision that rounding could turn, 100 delta): the gap in log e between the kept and the
    dropped side of each cut that is on, the distance in log e of every bin from the floor, and |F_n - p| at every n where the
    sorted values step (inside a run of bit-equal values there is nothing to decide: ties stay together)"""
    x = np.asarray(row.logits, dtype=np.float64) / row.T
    lq = x - x.max()
    q = np.exp(lq)
    rows = lq - np.log(q.sum())
    dlt = CC.delta(row.T, float(np.abs(row.logits).max()), float(np.abs(rows).max()), A)
    dist = [np.inf]
    for k, p, tau in ((row.k, 1.0, 0.0), (0, row.p, 0.0), (0, 1.0, row.tau)):
        keep = kept64(row.logits, k, p, tau, row.T)
        if not keep.all():
            dist.append(lq[keep].min() - lq[~keep].max())
    if row.tau > 0.0:
        dist.append(np.abs(lq - np.log(float(F32(row.tau)))).min())
    if row.p < 1.0:
        desc = np.sort(q)[::-1]
        F = np.cumsum(desc) / desc.sum()
        step = np.append(desc[1:] != desc[:-1], True)      # n - 1 where the n-th and the (n + 1)-th value differ
        dist.append(np.abs(F[step] - float(F32(row.p))).min())
    return float(min(dist)), 100.0 * dlt


# ---- the rows ----------------------------------------------------------------------------------------------------------------------

class Row:
    def __init__(self, name, logits, k, p, tau, T, keep):
        self.name, self.logits, self.k, self.p, self.tau, self.T = name, logits, int(k), float(p), float(tau), float(T)
        self.keep = keep                                  # the bins with e > 0 behind the cut, as the row was built (sorted indices)

    @property
    def setting(self):
        return (self.k, self.p, self.tau, self.T)


def tie_spots(LPU, RPL):
    """five bins for a tie: the last row of lane 0 and the first of lane 1 (xor 1 partners), one in the quad's other pair, one in
    another quad (the other half of 8) and one in the other half of 16 -- as far as the layout has them"""
    return [min(lane, LPU - 1) * RPL + r for lane, r in ((0, RPL - 1), (1, 0), (2, 3), (5, 1), (11, 2))]


def crafted(A, LPU):
    """the crafted rows of the module docstring: a list of Row, a multiple of 16 of them, 16 different settings per launch"""
    RPL = A // LPU
    rows = []

    def bg(lo, hi):                                       # A distinct values in [lo, hi), in no order
        return lo + (hi - lo) * np.modf((np.arange(A) + 1) * 0.6180339887498949)[0]

    def add(name, loge, k=0, p=1.0, tau=0.0, T=1.0, keep=None):
        logits = (np.asarray(loge, dtype=np.float64) * T).astype(F32)
        rows.append(Row(name, logits, k, p, tau, T, np.arange(A) if keep is None else np.array(sorted(int(i) for i in keep))))

    x = bg(-9, -5)
    spots = tie_spots(LPU, RPL)
    x[7], x[spots] = 0.0, -1.0
    add("five bit-equal bins at ranks 2 to 6 across lanes, quads and halves, k = 3", x, k=3, T=1.0, keep=[7] + spots)
    x = bg(-9, -5)
    x[3] = x[A - 5] = 0.0
    add("two bit-equal maxima in the first and the last lane, k = 1", x, k=1, T=2.0, keep=[3, A - 5])
    add("uniform, k = 1", np.full(A, 0.75), k=1, T=0.5)
    add("uniform, k = 7", np.zeros(A), k=7, T=1.0)
    add("uniform, p = 0.3", np.full(A, -1.5), p=0.3, T=2.0)
    add("uniform, k = A - 1", np.full(A, 0.25), k=A - 1, T=2.0)
    x = np.full(A, -200.0)
    x[77] = 0.0
    add("a point mass, the rest underflows to e = 0, k = 32", x, k=32, T=1.0, keep=[77])
    x = np.full(A, -200.0)
    x[A - 1] = 0.0
    add("a point mass in the last bin, the rest underflows, p = 0.5", x, p=0.5, T=2.0, keep=[A - 1])
    x = np.full(A, -60.0)
    x[77] = 0.0
    add("a point mass, the rest tiny and tied, k = 32", x, k=32, T=0.5)
    x = bg(-3, 0)
    x[0] = -6.0
    add("k = A - 1, the unique minimum in bin 0", x, k=A - 1, T=1.0, keep=range(1, A))
    x = bg(-3, 0)
    x[A - 1] = -6.0
    add("k = A - 1, the unique minimum in bin A - 1", x, k=A - 1, T=0.5, keep=range(A - 1))
    add("k = A, everything off", bg(-6, 0), k=A, T=0.5)
    # four masses of 1.1e-8 in lane 0, then RPL - 1 of them in front of a mass of 1 in one lane, nothing else: that lane's lsum and
    # incl are multiples of 2^-23, so its running sum starts from 0 or from 2^-23, not from the 4.4e-8 in front of it, and at the
    # selector 2^-24 it crosses the target of 6e-8 at another row than a sum carried over exactly would
    x = np.full(A, -200.0)
    lane = LPU // 2 + 1
    at = [0, 1, 2, 3] + list(range(lane * RPL, lane * RPL + RPL - 1))
    x[at], x[lane * RPL + RPL - 1] = np.log(1.1e-8), 0.0
    add("k = 0, everything off: small masses in front of a large one in one lane", x, k=0, T=1.0, keep=at + [lane * RPL + RPL - 1])
    x = bg(-12, -8)
    at = [1, 4, 6, 9, RPL - 1]
    x[at] = [0.0, -0.5, -1.0, -1.5, -2.0]
    add("kept bins in lane 0 only, k = 5", x, k=5, T=1.0, keep=at)
    x = bg(-12, -8)
    at = [(LPU - 1) * RPL + r for r in (0, 3, 7, RPL - 1)]
    x[at] = [-1.0, 0.0, -1.5, -0.5]
    add("kept bins in the last lane only, floor 0.1", x, tau=0.1, T=2.0, keep=at)
    for odd in (0, 1):
        x = bg(-12, -8)
        at = [lane * RPL + (3 * lane + 1) % RPL for lane in range(odd, LPU, 2)]
        x[at] = -0.1 * np.arange(len(at))
        add("kept bins in every other lane (%s), k = LPU / 2" % ("odd" if odd else "even"), x, k=len(at), T=(0.5, 2.0)[odd], keep=at)
    x = bg(-12, -8)
    x[2:12] = -0.3 * np.arange(10)
    add("the kept set ends well before A - 1, k = 10", x, k=10, T=2.0, keep=range(2, 12))
    x = bg(-12, -8)
    at = np.arange(A // 2 + 1, A)
    x[at] = bg(-2, -0.05)[at]
    x[A // 2 + 5] = 0.0
    add("the kept set starts after bin 0, floor 0.1", x, tau=0.1, T=1.0, keep=at)
    x = np.full(A, -20.0)
    x[10], x[A - 30] = 0.0, np.log(0.5)
    add("masses 1 and 0.5, p = 0.6: the first alone", x, p=0.6, T=1.0, keep=[10])
    add("masses 1 and 0.5, p = 0.7: both", x, p=0.7, T=0.5, keep=[10, A - 30])
    x = np.full(A, -20.0)
    x[RPL - 1] = x[A - RPL] = 0.0
    add("two equal masses, p = 0.5: both", x, p=0.5, T=2.0, keep=[RPL - 1, A - RPL])
    # e = 0.67^r at ranks r = 0 .. 19: the floor 0.25 keeps 4 and 0.05 keeps 8, p = 0.925 keeps 7 and 0.6 keeps 3
    x = np.full(A, -25.0)
    pos = [(37 * r + 11) % A for r in range(20)]
    x[pos] = -0.4 * np.arange(20)
    add("the floor is the strictest of the three", x, k=8, p=0.925, tau=0.25, T=2.0, keep=pos[:4])
    add("top-k is the strictest of the three", x, k=2, p=0.925, tau=0.05, T=0.5, keep=pos[:2])
    add("top-p is the strictest of the three", x, k=8, p=0.6, tau=0.05, T=1.0, keep=pos[:3])
    x = bg(-9, -5)
    x[20], x[RPL + 1], x[2 * RPL] = 0.0, -0.4, -1.0
    add("floor 0.5", x, tau=0.5, T=1.0, keep=[20, RPL + 1])
    x = bg(-9, -5)
    x[5] = x[A - 6] = 0.0
    x[A // 2] = -0.4
    add("floor 0.5 under two bit-equal maxima", x, tau=0.5, T=0.5, keep=[5, A // 2, A - 6])
    x = bg(-9, -5)
    x[9] = 0.0
    add("p = 1e-40: the maximum alone", x, p=1e-40, T=1.0, keep=[9])
    add("p = 1e-46, zero in float32: the bound p S(0) is zero, the maximum alone", x, p=1e-46, T=2.0, keep=[9])
    add("p = the smallest normal float: the maximum alone", x, p=float(np.finfo(F32).tiny), T=0.5, keep=[9])
    big = 40.0 * np.tanh((np.arange(A) - 17.0) / 3.0)      # large magnitudes: the maximum's subtraction matters
    add("40 tanh((a - 17) / 3), k = A - 26", big, k=A - 26, T=1.0, keep=range(26, A))
    add("40 tanh((a - 17) / 3), floor 0.05", big, tau=0.05, T=1.0, keep=range(22, A))
    assert len(rows) % 16 == 0, len(rows)
    return rows


def random_rows(A, n=64, seed=20):
    """n seeded rows of N(0, 2.5^2) logits with k of (2, 4, 32) and p of (1, 0.9), neighbours never the same; for the exact
    comparisons and the membership check only (nothing keeps them clear of rounding)"""
    rng = np.random.default_rng(seed + A)
    out = []
    for i in range(n):
        u = i % 16
        k, p, T = (2, 4, 32)[u % 3], (1.0, 0.9)[(u // 3) % 2], (1.0, 0.5, 2.0)[(u // 6) % 3]
        out.append(Row("random %d" % i, rng.normal(0.0, 2.5, A).astype(F32), k, p, 0.0, T, None))
    return out


def launches(rows):
    """the rows in launches of 16: [(logits [16][A], k [16] int32, p [16], tau [16], T [16], rows)]"""
    out = []
    for at in range(0, len(rows), 16):
        g = rows[at:at + 16]
        out.append((np.stack([r.logits for r in g]).astype(F32), np.array([r.k for r in g], dtype=np.int32),
                    np.array([r.p for r in g], dtype=F32), np.array([r.tau for r in g], dtype=F32),
                    np.array([r.T for r in g], dtype=F32), g))
    return out


def in_force(row, form, A):
    """does form 1, 2 or 3 cut anything from this row's settings (form 1 takes the floor alone)"""
    return row.tau > 0.0 or (form >= 2 and (0 < row.k < A or row.p < 1.0))
