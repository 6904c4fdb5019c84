"""Cases, the numpy mirror and the checks of the probability-floor tests (tests/test_min_p_cpu.py, tests/test_min_p_gpu.py; DESIGN.md
§6m).  Shapes: those of the temperature tests (tests/temperature_cases.py) -- 40 columns make three tiles, A = 512 and A = 1024 the
other softmax lane layouts.  Column b draws with floor FLOORS[b % 5] at temperature POWERS[(b + 1) % 5]: every 16-lane row mixes all
five floors, and floor and temperature are not aligned.

THE RULE.  With c = log2(e) / T, m the largest logit and e_a = exp2(fma(z_a, c, -(m c))) -- which is p_a / p_max of the tempered
distribution up to the rounding of m c --, a column with floor tau keeps the bins with e_a >= tau, sets the others to 0, and runs
the sum, the scan, the target u * total and the row search on what is left.

EPSILON.  The GPU tests decide "kept" from the engine's own scoring rows, log softmax(Za / T) in float32, as
rows[a] - max rows >= log(tau).  That decision and the kernel's differ only for bins within EPS of the floor, in natural-log units:
  * the kernel's exponent is fma(z, c, mneg) with mneg = fl(-m c): half an ulp of m c, at most 2^-24 c max|Za| in log2 units.  It
    moves every e of the row by one factor, i.e. the kernel compares against p_max 2^r, |r| <= 2^-24 c max|Za|;
  * the fma rounds its result, |z c - m c| <= 2 c max|Za|: at most 2^-24 * 2 c max|Za|;
  * v_exp_f32 is good to one ulp of e: 2^-23 / ln 2 < 2^-22 in log2 units;
  * the scoring pass forms (fma(z, c, mneg) - log2 sum) * ln 2: the subtraction and the scaling round once each, at most
    2^-24 (|rows| / ln 2 + |rows|) per entry, and the decision takes the difference of two entries: 2 * 2.5 * 2^-24 max|rows|.
In natural-log units and with eps32 = 2^-23: ln 2 (1.5 eps32 c max|Za| + 2 eps32) + 2.5 eps32 max|rows|
  <= 4 eps32 (c max|Za| + max|rows| + 1) =: EPS  -- "a handful of eps32 times c max|Za| + max|rows|", about 1.6e-5 at these shapes.
max|Za| comes from the float64 reference of tests/score_cases.py (its own error is far inside the factor 4 / 1.04 left over)."""
import numpy as np

import score_cases as SC
import temperature_cases as TC

CASE, CASE_A512, CASE_A1024 = TC.CASE, TC.CASE_A512, TC.CASE_A1024
COND, COND_A512, COND_A1024 = TC.COND, TC.COND_A512, TC.COND_A1024

FLOORS = (0.0, 0.05, 0.1, 0.25, 0.5)
BAD_FLOORS = (-0.1, 0.6, float("nan"), float("inf"))
EPS32 = SC.EPS32
MAX_LEFT_OUT = 0.01          # of the rows may be left out of the CDF check (a bin within EPS of the floor)


def floors(batch, shift=0):
    return [FLOORS[(b + shift) % len(FLOORS)] for b in range(batch)]


def temperatures(batch):
    """POWERS shifted by one against the floors"""
    return TC.power_temperatures(batch, 1)


def bits(p):
    """the word of a blob's header (word 11) that carries floor p: the bits of the float, zero for 0"""
    return int(np.array([p], dtype="<f4").view("<u4")[0]) if p != 0.0 else 0


def epsilon(T, za_max, rows_max):
    """EPS of the module docstring for a column at temperature T whose logits are within za_max and whose rows within rows_max"""
    c = 1.4426950408889634 / float(T)
    return 4.0 * EPS32 * (c * float(za_max) + float(rows_max) + 1.0)


def kept(rows, tau):
    """[n][A] bool: the bins of every row that floor tau keeps, decided from log-probabilities in float64"""
    r = np.asarray(rows, dtype=np.float64)
    rel = r - r.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return rel >= np.log(float(tau))


def pick_min_p(rows, u, tau):
    """The numpy mirror of the rule on log-probabilities rows [n][A] (float64; already at the column's temperature), draws u [n]:
    e = p / p_max, e < tau -> 0, the pick is the first row whose cumulative sum exceeds u * total (the last kept bin when the scan
    falls off the end: under a floor the kernel never answers a dropped bin).  Returns y [n]."""
    r = np.asarray(rows, dtype=np.float64)
    e = np.exp(r - r.max(axis=1, keepdims=True))
    e = np.where(e >= float(tau), e, 0.0)
    cum = np.cumsum(e, axis=1)
    target = np.asarray(u, dtype=np.float64) * cum[:, -1]
    first = (cum <= target[:, None]).sum(axis=1)
    last = r.shape[1] - 1 - np.argmax((e > 0)[:, ::-1], axis=1)
    return np.where(first < r.shape[1], first, last).astype(np.int64)


def check_column(rows, y, u, tau, eps, min_p_rows):
    """The two checks of one column, on the log-probabilities `rows` [n][A] of its own samples y [n] drawn with u [n] under floor tau:
      support: rows[t][y] - max_a rows[t][a] >= log(tau) - eps for every sample;
      CDF:     u lies inside the picked bin of the CDF built from min_p_rows(rows, tau), for every row that has no bin within eps
               of the floor.
    Returns (support violations, CDF violations among the rows checked, rows left out, rows): numbers of samples."""
    r = np.asarray(rows, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    n = len(y)
    rel = r - r.max(axis=1, keepdims=True)
    if tau > 0.0:
        logt = np.log(float(tau))
        support_bad = int((rel[np.arange(n), y] < logt - eps).sum())
        near = (np.abs(rel - logt) <= eps).any(axis=1)
    else:
        support_bad, near = 0, np.zeros(n, dtype=bool)
    inside, _, _ = SC.cdf_check(np.asarray(min_p_rows(r, tau), dtype=np.float64), y, np.asarray(u, dtype=np.float64))
    return support_bad, int((~inside & ~near).sum()), int(near.sum()), n


def check_run(rows_of, y, u, taus, eps_of, min_p_rows):
    """check_column over the columns b of a run: rows_of(b) [n][A], y [B][n], u [n][B], taus [B], eps_of(b).  Returns the totals
    (support violations, CDF violations, rows left out, rows)."""
    tot = np.zeros(4, dtype=np.int64)
    for b, tau in enumerate(taus):
        tot += np.array(check_column(rows_of(b), y[b], u[:, b], tau, eps_of(b), min_p_rows))
    return tuple(int(v) for v in tot)


def accepted(totals):
    """what the tests assert of check_run's totals: no support violation, no CDF violation, at most MAX_LEFT_OUT of the rows left out"""
    support_bad, cdf_bad, left_out, n = totals
    return support_bad == 0 and cdf_bad == 0 and left_out <= MAX_LEFT_OUT * n
