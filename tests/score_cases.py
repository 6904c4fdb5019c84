"""Shapes, reference and bars of the scoring tests (tests/test_score_cpu.py, tests/test_score_gpu.py).

The reference is a float64 numpy model of the TEACHER-FORCED network, time-parallel like the pass it checks: every sample of y is
known, so layer l at all samples is two matrix products over [n][R].  It follows the oracle's arithmetic (oracle/wavenet_oracle.c;
tests/fp16_model.py states the same network sample by sample) and is held to the oracle itself by tests/test_score_cpu.py at the
positions POSITIONS -- the tile edges, the first samples (taps before the start), the last one, and around the longest dilation.

The bar is the project's logit bar carried through the log-softmax: d log p_y = dz_y - sum_a p_a dz_a, so |d logp| <= 2 delta / T
with delta = (cases.TOL["Za"] + 32 eps32) max|Za_ref| for an fp32 engine (util.compare_activations(atol_eps=32)) and
util.FP16_K util.FP16_U max|Za_ref| for an fp16 engine (util.fp16_bars), max|Za_ref| over the request."""
import numpy as np

import cases
import prefill_cases as PF
import prime_cases as PC
import util

EPS32 = 1.1920929e-07

# the prime tests' shape: R 64 / S 256 / A 256, 8 layers, dilations 1 .. 16, 48 samples
PRIME_SHAPE = ((PC.CASE.shape.R, PC.CASE.shape.S, PC.CASE.shape.A), 931, PC.CASE.shape.L, PC.CASE.shape.maxD, PC.CASE.shape.N)
assert PRIME_SHAPE == ((64, 256, 256), 931, 8, 16, 48)
LONG = PF.LONG                                   # R 64, 12 layers, maxDilation 128, 304 samples
LONG_N = 300
# every (R, S, A) the library builds: seed of util.gen_o1
BUILT = {(32, 128, 256): 941, (64, 128, 256): 942, (64, 256, 256): 943, (128, 256, 256): 944, (64, 128, 512): 945, (256, 256, 256): 946,
         (32, 256, 256): 947, (128, 256, 1024): 948}
# odd and minimal depth (Cfg::streamPos treats layers 0 and L - 1 specially): (shape, seed, L, maxD, N)
DEPTHS = [((64, 128, 256), 951, 7, 4, 48), ((64, 256, 256), 952, 2, 2, 48)]
LENGTHS = (1, 2, 15, 16, 17, 47, 48)             # the tile edge, and n below a dilation


def positions(n, long=False):
    """the samples at which reference and oracle / engine are compared"""
    ks = [0, 1, 2, 15, 16, 17, n - 1] + ([127, 128, 129, 271] if long else [])
    return sorted({k for k in ks if 0 <= k < n})


def setup(shape, seed, precision, L=8, maxD=16, N=48, columns=3):
    """(case, t, x [columns][n_cond][N], w, b): the network in the O(1) recipe and the features of prefill_cases; an fp16 engine
    takes fp16-rounded parameters and features"""
    case = PF.case_of(shape, seed, L, maxD, N, columns)
    half = precision == 16
    t = util.gen_o1(case, half=half)
    x, w, b = PF.features(columns, N, shape[0], L, half=half)
    return case, t, x, w, b


def lh_of(x, w, b, R, L):
    """Lh [N][L][2R] = Wcond x + bcond of one utterance x [n_cond][N], float64"""
    lh = w.astype(np.float64) @ x.astype(np.float64) + b.astype(np.float64)[:, None]
    return np.ascontiguousarray(lh.reshape(L, 2 * R, -1).transpose(2, 0, 1))


def log_softmax(Za, T=1.0):
    z = np.asarray(Za, dtype=np.float64) / float(T)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


MUTATIONS = ("no_skip_bias", "drop_last_skip", "restart_skip", "shift_y", "swap_history", "ignore_T", "feature_prev")


def reference(t, shape, y, Lh, T=1.0, mutate=None, tanh_embed=True):
    """(Za [n][A], logp [n]) in float64 of the network t teacher-forced on y [n] from silence, conditioning Lh [>= n][L][2R].
    shape: anything with R, S, A, L, maxD.  mutate: one of MUTATIONS, a deliberately broken model (negative controls).
    tanh_embed=False: the embedding sum enters layer 0 as it is (WavenetEngine(tanhEmbed=False), the oracle's set_tanh_embed(False))."""
    assert mutate is None or mutate in MUTATIONS
    R, S, A, L, maxD = shape.R, shape.S, shape.A, shape.L, shape.maxD
    f = lambda a: np.asarray(a, dtype=np.float64)
    y = np.clip(np.asarray(y, dtype=np.int64), 0, A - 1)
    n = len(y)
    fed = y if mutate != "shift_y" else np.concatenate([y[1:], y[-1:]])          # (the history one position early)
    cur = np.concatenate([[128], fed[:-1]])[:n]                                  # y[t-1]
    old = np.concatenate([[128, 128], fed[:-2]])[:n]                             # y[t-2]
    if mutate == "swap_history":
        cur, old = old, cur
    x = f(t.embP)[old] + f(t.embC)[cur]
    if tanh_embed:
        x = np.tanh(x)
    lh = f(Lh)[:n]
    if mutate == "feature_prev":
        lh = np.concatenate([lh[:1], lh[:-1]])
    skip = np.zeros((n, S))
    d = 1
    for l in range(L):
        xp = np.zeros_like(x)
        if d < n:
            xp[d:] = x[:-d]
        a = f(t.Bh[l])[None, :] + lh[:, l] + xp @ f(t.Wprev[l]) + x @ f(t.Wcur[l])
        h = np.tanh(a[:, :R]) / (1.0 + np.exp(-a[:, R:]))
        x = f(t.Bres[l])[None, :] + x + h @ f(t.Wres[l])
        if mutate == "restart_skip" and l == L // 2:
            skip[:] = 0
        if not (mutate == "drop_last_skip" and l == L - 1):
            skip = skip + h @ f(t.Wskip[l])
        if mutate != "no_skip_bias":
            skip = skip + f(t.Bskip[l])[None, :]
        d = d * 2 if d * 2 <= maxD else 1
    zs = np.maximum(f(t.Bzs)[None, :] + np.maximum(skip, 0) @ f(t.Wzs), 0)
    Za = f(t.Bza)[None, :] + zs @ f(t.Wza)
    rows = log_softmax(Za, 1.0 if mutate == "ignore_T" else T)
    return Za, rows[np.arange(n), y]


def bar(Za_ref, T, precision):
    """|d logp| allowed: 2 delta / T, delta the project's logit bar of the precision, max|Za_ref| over the request"""
    top = float(np.abs(Za_ref).max())
    delta = (cases.TOL["Za"] + 32 * EPS32) * top if precision == 32 else util.FP16_K * util.FP16_U * top
    return 2.0 * delta / float(T)


def cdf_check(rows, y, u):
    """rows [n][A] log-probabilities, y [n] picks, u [n] draws: per sample 0 when C[y-1] <= u < C[y] in the float64 CDF built from
    exp(rows); else (bins to the containing bin, distance of u from the violated edge)"""
    p = np.exp(np.asarray(rows, dtype=np.float64))
    C = np.cumsum(p, axis=1)
    C /= C[:, -1:]
    n = len(y)
    lo = np.where(y > 0, C[np.arange(n), np.maximum(y - 1, 0)], 0.0)
    hi = C[np.arange(n), y]
    inside = (lo <= u) & (u < hi)
    holds = np.array([int(np.searchsorted(C[k], u[k], side="right")) for k in range(n)])
    edge = np.where(u < lo, lo - u, np.where(u >= hi, u - hi, 0.0))
    return inside, np.abs(holds - y), edge


def wrapper_weights(t, shape):
    """the network t as the export_weights()-shaped tensors NVWaveNetEngine takes (numpy; the wrapper's output biases are zero and
    its last residual layer is unused, so Bzs and Bza of t must be zero)"""
    L = shape.L
    assert not t.Bzs.any() and not t.Bza.any()
    mk = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32).T)[:, :, None]          # [K][M] -> [M][K][1]
    return dict(embedding_prev=np.asarray(t.embP), embedding_curr=np.asarray(t.embC), conv_out_weight=mk(t.Wzs), conv_end_weight=mk(t.Wza),
                dilate_weights=[np.ascontiguousarray(np.stack([np.asarray(t.Wprev[l]).T, np.asarray(t.Wcur[l]).T], axis=2)) for l in range(L)],
                dilate_biases=[np.asarray(t.Bh[l]) for l in range(L)], max_dilation=shape.maxD,
                res_weights=[mk(t.Wres[l]) for l in range(L - 1)], res_biases=[np.asarray(t.Bres[l]) for l in range(L - 1)],
                skip_weights=[mk(t.Wskip[l]) for l in range(L)], skip_biases=[np.asarray(t.Bskip[l]) for l in range(L)], use_embed_tanh=True)
