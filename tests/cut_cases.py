"""Cases, the numpy mirrors and the checks of the tail-cut tests (top-k and top-p; tests/test_cut_cpu.py, tests/test_cut_gpu.py;
DESIGN.md §6n).  Shapes: those of the probability-floor tests (tests/min_p_cases.py).  Column b draws with top-k TOP_KS[b % 5] (the
last entry stands for A), top-p TOP_PS[b % 4], floor MP.floors(B, 2)[b] at temperature MP.temperatures(B)[b]: four against five, so
every pair of cuts occurs, and every 16-lane row mixes all of them.

THE RULE.  With e_a = exp2(fma(z_a, c, -(m c))) as for the floor, theta_k is the k-th largest e (0 when k = 0), theta_p the largest
float with S(theta) >= p S(0) (0 when p = 1), S(theta) the float32 sum of the e >= theta in the kernel's order, and the column keeps
e_a >= max(theta_k, theta_p, tau): the intersection of the three cuts, each defined on the whole tempered distribution.

DELTA.  The GPU tests decide the kept set from the engine's own scoring rows in float64: q_a = exp(rows_a - max rows) stands for e_a.
  * log e_a and log q_a differ by one factor common to the row and by at most EPS per bin (tests/min_p_cases.py: the rounding of
    m c, of the fma, of v_exp_f32 and of the scoring pass).  The order of two bins, and whether two bins tie, is the kernel's own
    where their rows differ by more than 2 EPS; a bin is on the floor's side the kernel saw where it is more than EPS from it.
  * S(theta) and S(0) are float32 sums of non-negative terms, each through at most RPL + log2 LPU additions: relative error at most
    (RPL + log2 LPU) 2^-24 each; RPL = A / LPU and LPU >= 4 in every lane layout, so RPL + log2 LPU <= A / 4 + 2.  The product
    p S(0) rounds once: 2^-24.  With the terms themselves good to EPS each against q (the common factor cancels in the ratio), the
    kernel's S(theta) / S(0) is within 2 EPS + (2 (A / 4 + 2) + 1) 2^-24 of the prefix mass of q, relative, and the mass is <= 1.
DELTA = 2 EPS + (A / 4 + 3) eps32 (eps32 = 2^-23) covers every term above, in natural-log units for gaps and floors and as an
absolute distance for prefix masses: about 4e-5 at A = 256, 5e-5 at A = 512, 7e-5 at A = 1024.

CANDIDATES.  A row's bins in descending order of q.  Each cut gives the lengths of the prefix it may keep: top-k k; top-p the
smallest n whose prefix mass F_n reaches p, and n + 1 for every n with |F_n - p| <= DELTA; the floor every length between the
number of bins more than DELTA above tau and the number of bins not more than DELTA below it.  The kept length is the smallest of
the three, for every combination.  For a length n, the bins within DELTA of the n-th (its cluster) may be ordered otherwise or tie
in the kernel's e: the candidates are the bins above the cluster with every choice of the remaining ones from the cluster, and, as
ties at the boundary all stay, with every longer choice from it.  A row with no quantity within DELTA has one candidate."""
import itertools

import numpy as np

import min_p_cases as MP
import score_cases as SC

CASE, CASE_A512, CASE_A1024 = MP.CASE, MP.CASE_A512, MP.CASE_A1024
COND, COND_A512, COND_A1024 = MP.COND, MP.COND_A512, MP.COND_A1024

TOP_KS = (0, 1, 4, 32, None)                 # None: A, the alphabet of the shape
TOP_PS = (1.0, 0.5, 0.8, 0.9)
BAD_TOP_KS = (-1, None)                      # None: A + 1
BAD_TOP_PS = (0.0, -0.5, 1.0000001, 1.5, float("nan"), float("inf"))
EPS32 = SC.EPS32
MAX_MULTI = 0.10                             # of the rows of a run may have more than one candidate (the CPU test: 0.05)
MAX_CLUSTER = 6                              # bins within DELTA of a boundary; more would make the candidates meaningless


def top_ks(batch, A, shift=0):
    return [A if TOP_KS[(b + shift) % 5] is None else TOP_KS[(b + shift) % 5] for b in range(batch)]


def top_ps(batch, shift=0):
    return [TOP_PS[(b + shift) % 4] for b in range(batch)]


def floors(batch):
    return MP.floors(batch, 2)


def temperatures(batch):
    return MP.temperatures(batch)


def p_bits(p):
    """the word of a blob's header (word 13) that carries top-p: the bits of the float, zero for 1"""
    return int(np.array([p], dtype="<f4").view("<u4")[0]) if p != 1.0 else 0


def delta(T, za_max, rows_max, A):
    """DELTA of the module docstring for a column at temperature T"""
    return 2.0 * MP.epsilon(T, za_max, rows_max) + (A / 4.0 + 3.0) * EPS32


# ---- the kernel's search, mirrored in float32 --------------------------------------------------------------------------------------

def group_sum(v, LPU):
    """S of the rule: v [A] float32, each of the LPU lanes sums its A / LPU values in row order, then butterflies over xor 1 and
    xor 2 and mirrors in 8 and in 16 lanes -- group_reduce_f<LPU> with +; every lane ends with the same value"""
    v = np.asarray(v, dtype=np.float32).reshape(LPU, -1)
    lane = np.zeros(LPU, dtype=np.float32)
    for i in range(v.shape[1]):
        lane = (lane + v[:, i]).astype(np.float32)
    idx = np.arange(LPU)
    lane = (lane + lane[idx ^ 1]).astype(np.float32)
    lane = (lane + lane[idx ^ 2]).astype(np.float32)
    if LPU >= 8:
        lane = (lane + lane[(idx & ~7) | (7 - (idx & 7))]).astype(np.float32)
    if LPU >= 16:
        lane = (lane + lane[15 - idx]).astype(np.float32)
    assert (lane == lane[0]).all(), "the group's sum differs between its lanes"
    return np.float32(lane[0])


def bisect_threshold(e, k, p, LPU=16, steps=31):
    """cut_threshold of wn_kernels.hpp: max(theta_k, theta_p) of e [A] float32 (non-negative) by ONE bisection over bit patterns on
    the disjunction of the two predicates (it holds on [0, max of the two]); an off cut never holds"""
    e = np.asarray(e, dtype=np.float32)
    bits = lambda w: np.array([w], dtype=np.uint32).view(np.float32)[0]
    need = np.float32(np.float32(p) * group_sum(e, LPU)) if p < 1.0 else np.float32(np.inf)
    kneed = k if k > 0 else 2 ** 31 - 1
    lo, hi = 0, int(np.array([e.max()], dtype=np.float32).view(np.uint32)[0]) + 1
    for _ in range(steps):
        mid = lo + ((hi - lo) >> 1)
        keep = e >= bits(mid)
        if int(keep.sum()) >= kneed or group_sum(np.where(keep, e, np.float32(0)), LPU) >= need:
            lo = mid
        else:
            hi = mid
    return bits(lo)


def search_from_the_top(e, k, p, LPU=16):
    """cut_threshold_dump of wn_kernels.hpp (the activation-dump kernels): max(theta_k, theta_p) of e [A] float32 (non-negative) by ONE search over bit patterns on the
    disjunction of the two predicates (it holds on [0, max of the two]): the 31 bits of the pattern are set from the top, lo | step
    is kept where the disjunction holds; an off cut never holds, and the mass predicate counts only while some bin passes"""
    e = np.asarray(e, dtype=np.float32)
    bits = lambda w: np.array([w], dtype=np.uint32).view(np.float32)[0]
    need = np.float32(np.float32(p) * group_sum(e, LPU)) if p < 1.0 else np.float32(np.inf)
    kneed = k if k > 0 else 2 ** 31 - 1
    lo, step = 0, 1 << 30
    while step:
        mid = lo | step
        with np.errstate(invalid="ignore"):
            keep = e >= bits(mid)                     # (against the patterns of inf and NaN no bin passes)
        cnt = int(keep.sum())
        if cnt >= kneed or (cnt > 0 and group_sum(np.where(keep, e, np.float32(0)), LPU) >= need):
            lo = mid
        step >>= 1
    return bits(lo)


def sorted_threshold(e, k, p, LPU=16):
    """the same threshold by the definition, with a sort: theta_k the k-th largest e, theta_p the largest value of e whose S reaches
    p S(0) (S is a step function of theta with its steps at the values of e, so the largest float is one of them)"""
    e = np.asarray(e, dtype=np.float32)
    desc = np.sort(e)[::-1]
    th_k = desc[k - 1] if k > 0 else np.float32(0)
    th_p = np.float32(0)
    if p < 1.0:
        need = np.float32(np.float32(p) * group_sum(e, LPU))
        for v in np.unique(e)[::-1]:
            if group_sum(np.where(e >= v, e, np.float32(0)), LPU) >= need:
                th_p = v
                break
    return max(th_k, th_p)


# ---- the rule in float64 ----------------------------------------------------------------------------------------------------------

def kept(rows, k, p, tau):
    """[n][A] bool: the nominal kept set of every row (float64, by sorting): q >= max(theta_k, theta_p, tau)"""
    r = np.asarray(rows, dtype=np.float64)
    q = np.exp(r - r.max(axis=1, keepdims=True))
    out = np.zeros(q.shape, dtype=bool)
    for t in range(len(q)):
        desc = np.sort(q[t])[::-1]
        th_k = desc[k - 1] if k > 0 else 0.0
        th_p = 0.0
        if p < 1.0:
            cum = np.cumsum(desc)
            th_p = desc[int(np.argmax(cum >= p * cum[-1]))]
        out[t] = q[t] >= max(th_k, th_p, float(tau))
    return out


def rows_of_mask(rows, mask):
    """the log-probabilities of rows [n][A] restricted to mask and renormalised (-inf outside)"""
    r = np.asarray(rows, dtype=np.float64)
    rel = r - r.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        s = np.where(mask, np.exp(rel), 0.0).sum(axis=1, keepdims=True)
        return np.where(mask, rel - np.log(s), -np.inf)


def pick(rows, u, mask):
    """the inverse-CDF pick of the rule from rows [n][A] restricted to mask: the first bin whose cumulative sum exceeds u * total
    (the last kept bin when the scan falls off the end: under a cut the kernel never answers a dropped bin)"""
    r = np.asarray(rows, dtype=np.float64)
    e = np.where(mask, np.exp(r - r.max(axis=1, keepdims=True)), 0.0)
    cum = np.cumsum(e, axis=1)
    first = (cum <= (np.asarray(u, dtype=np.float64) * cum[:, -1])[:, None]).sum(axis=1)
    last = r.shape[1] - 1 - np.argmax((e > 0)[:, ::-1], axis=1)
    return np.where(first < r.shape[1], first, last).astype(np.int64)


def pick_cut(rows, u, k, p, tau):
    """the numpy mirror of the rule: y [n] of rows [n][A] (log-probabilities at the column's temperature) and draws u [n]"""
    return pick(rows, u, kept(rows, k, p, tau))


# ---- candidates and the check ------------------------------------------------------------------------------------------------------

def candidates(row, k, p, tau, dlt):
    """The candidate kept sets of one row [A] of log-probabilities (module docstring): a list of bool masks, the nominal one first."""
    r = np.asarray(row, dtype=np.float64)
    A = len(r)
    order = np.argsort(-r, kind="stable")
    lq = r[order] - r[order[0]]                       # log q, descending
    q = np.exp(lq)
    cum = np.cumsum(q)
    F = cum / cum[-1]
    n_k = {k} if k > 0 else {A}
    if p < 1.0:
        first = int(np.argmax(cum >= p * cum[-1])) + 1
        near = np.nonzero(np.abs(F - p) <= dlt)[0] + 1
        n_p = {first} | {int(n) for n in near} | {min(int(n) + 1, A) for n in near}
    else:
        first, n_p = A, {A}
    if tau > 0.0:
        lt = np.log(float(tau))
        at = max(1, int((q >= float(tau)).sum()))
        n_f = set(range(max(1, int((lq > lt + dlt).sum())), int((lq >= lt - dlt).sum()) + 1)) | {at}
    else:
        at, n_f = A, {A}
    nominal = min(k if k > 0 else A, first, at)
    # (the nominal set keeps exact ties in q at its boundary)
    while nominal < A and lq[nominal] == lq[nominal - 1]:
        nominal += 1
    lengths = sorted({min(a, b, c) for a in n_k for b in n_p for c in n_f})
    masks, seen = [], set()

    def add(sel):
        key = tuple(sorted(int(i) for i in sel))
        if key not in seen:
            seen.add(key)
            m = np.zeros(A, dtype=bool)
            m[order[list(key)]] = True
            masks.append(m)

    add(range(nominal))
    for n in lengths:
        cluster = [i for i in range(A) if abs(lq[i] - lq[n - 1]) <= dlt]
        assert len(cluster) <= MAX_CLUSTER, "%d bins within delta of a boundary" % len(cluster)
        above = list(range(cluster[0]))
        for size in range(n - len(above), len(cluster) + 1):
            if size < 0:
                continue
            for sub in itertools.combinations(cluster, size):
                if len(above) + size >= 1:
                    add(above + list(sub))
    return masks


def check_column(rows, y, u, k, p, tau, dlt, cut_rows):
    """One column, on the log-probabilities rows [n][A] of its own samples y [n] drawn with u [n]: every sample must lie in a kept
    set of one of its row's candidates, with u inside the picked bin of the CDF of that candidate's renormalised rows -- the
    nominal candidate's from cut_rows itself.  Returns (violations, rows with more than one candidate, rows)."""
    r = np.asarray(rows, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    n = len(y)
    nominal = np.asarray(cut_rows(r, int(k), float(p), float(tau)), dtype=np.float64)
    bad = multi = 0
    for t in range(n):
        cands = candidates(r[t], k, p, tau, dlt)
        multi += len(cands) > 1
        assert np.array_equal(np.isfinite(nominal[t]), cands[0]), "cut_rows keeps another set than the rule's nominal one"
        ok = False
        for i, m in enumerate(cands):
            if not m[y[t]]:
                continue
            rr = nominal[t:t + 1] if i == 0 else rows_of_mask(r[t:t + 1], m[None, :])
            inside, _, _ = SC.cdf_check(rr, y[t:t + 1], u[t:t + 1])
            if inside[0]:
                ok = True
                break
        bad += not ok
    return int(bad), int(multi), n


def check_run(rows_of, y, u, ks, ps, taus, delta_of, cut_rows):
    """check_column over the columns of a run: rows_of(b) [n][A], y [B][n], u [n][B].  Returns the totals (violations, rows with
    more than one candidate, rows)."""
    tot = np.zeros(3, dtype=np.int64)
    for b in range(len(ks)):
        tot += np.array(check_column(rows_of(b), y[b], u[:, b], ks[b], ps[b], taus[b], delta_of(b), cut_rows))
    return tuple(int(v) for v in tot)


def accepted(totals, cap=MAX_MULTI):
    """what the tests assert of check_run's totals: no violation, and at most `cap` of the rows with more than one candidate"""
    bad, multi, n = totals
    return bad == 0 and multi <= cap * n
