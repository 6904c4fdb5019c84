"""Shapes of the prefill tests (tests/test_prefill_cpu.py, tests/test_prefill_gpu.py) and a Python mirror of what the
prefill pass relies on: the dilation schedule, the window W of trailing samples that determine a state, the first sample of every
layer that is computed from complete taps, and the rule that places x_l[k] in a state blob.

The equality cases are those of the prime tests (tests/prime_cases.py: R 64, 8 layers, dilations 1 .. 16, 48 samples, the lengths 1,
2, 15, 16, 17 around unwritten ring slots and the tile edge, 40, 47, 48 with a window that does not start at 0); one shape per other
R the library builds, at n = 17 and 47; and a long schedule (12 layers, maxDilation 128, sum 270) at n = 100 and 300: many time
tiles, taps that reach whole tiles back, a window that starts at 16."""
import numpy as np

import cases

HEADER_BYTES = 64
TILE = 16


def schedule(L, maxD):
    """[(d_l, off_l)]: dilation and first ring slot of every layer (d doubles per layer and restarts at 1 past maxD)."""
    out, d, off = [], 1, 0
    for _ in range(L):
        out.append((d, off))
        off += d
        d = d * 2 if d * 2 <= maxD else 1
    return out


def window(L, maxD):
    """W: the sum of the dilations + the two history samples the embedding reads."""
    return sum(d for d, _ in schedule(L, maxD)) + 2


def first_tile_sample(n, L, maxD):
    """t0: where the pass starts -- max(0, n - W) rounded down to a tile"""
    return (max(0, n - window(L, maxD)) // TILE) * TILE


def reach(l, L, maxD):
    """How far back in the prime the output of layer l at a sample t reaches: it depends on y[t - reach .. t - 1] and on nothing
    older (x_0[t] reads y[t-1] and y[t-2]; every layer k <= l adds its dilation)."""
    return sum(d for d, _ in schedule(L, maxD)[:l + 1]) + 2


def valid_from(n, l, L, maxD):
    """The first sample of x_l that a pass over [n - W, n) computes from complete taps: n - sum_{k >= l} d_k (x_0 is complete
    everywhere in the window; every layer below l costs its dilation)."""
    return n - sum(d for d, _ in schedule(L, maxD)[l:])


def blob_slot(l, k, L, maxD):
    """the blob slot that holds x_l[k]"""
    d, off = schedule(L, maxD)[l]
    return off + k % d


def blob_payload(xs, n, L, maxD):
    """numpy model of a payload after n samples: xs[l][k] = x_l[k] as a row (any width) -> [sum d][width]; slot off_l + i holds
    x_l[k] of the latest k < n with k mod d_l = i, zero where there is none."""
    sched = schedule(L, maxD)
    out = np.zeros((sum(d for d, _ in sched), xs[0].shape[1]), dtype=xs[0].dtype)
    for l, (d, off) in enumerate(sched):
        for i in range(d):
            ks = [k for k in range(n) if k % d == i]
            if ks:
                out[off + i] = xs[l][ks[-1]]
    return out


# one built shape per R other than the equality cases' 64: (R, S, A), seed of util.gen_o1; 8 layers, dilations 1 .. 16, 48 samples
OTHER_R = {32: ((32, 128, 256), 911), 128: ((128, 256, 256), 912), 256: ((256, 256, 256), 913)}
OTHER_N = (17, 47)
# the long window: R 64, 12 layers, maxDilation 128 (sum of the dilations 270, W = 272)
LONG = ((64, 128, 256), 914, 12, 128, 304)
LONG_N = (100, 300)
N_COND = 80
FEATURE_SEED = 77


def case_of(shape, seed, L=8, maxD=16, N=48, columns=2):
    R, S, A = shape
    return cases.Case("prefill_R%d" % R, seed, [], cases.Shape(R, S, A, L, columns, N, maxD), 1 if S <= 4 * R else 3, 1, 16)


def features(columns, N, R, L, half):
    """(x [columns][n_cond][N], w [2R L][n_cond], b [2R L]) from a fixed RandomState; half: x and w rounded through fp16"""
    rng = np.random.RandomState(FEATURE_SEED + R)
    x = rng.standard_normal((columns, N_COND, N)).astype(np.float32)
    w = ((rng.rand(2 * R * L, N_COND) - 0.5) * (3.46 * 0.5 / np.sqrt(N_COND))).astype(np.float32)
    b = ((rng.rand(2 * R * L) - 0.5) * 0.2).astype(np.float32)
    if half:
        x, w = x.astype(np.float16).astype(np.float32), w.astype(np.float16).astype(np.float32)
    return x, np.ascontiguousarray(w), b


def primes(columns, N, A, seed=5):
    """[columns][N] sample indices from a fixed RandomState, 0 and A - 1 among the first ones of every column"""
    p = np.random.RandomState(seed).randint(0, A, size=(columns, N)).astype(np.int32)
    p[:, 3], p[:, 7] = 0, A - 1
    return p
