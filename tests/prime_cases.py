"""Shapes and primes of the primed-generation tests (tests/test_prime_cpu.py, tests/test_prime_gpu.py).  The cases and
their committed conditioning fixtures are those of the temperature tests (tests/temperature_cases.py): R 64 / S 256 / A 256, 8 layers,
dilations 1 .. 16, 40 columns, 48 samples, chunk 20; and R 128 / A 1024 on 16 columns, the one-tile kernel whose softmax spreads an
utterance's logits over other lane groups."""
import numpy as np

import temperature_cases as TC
import util
from oracle import oracle as O

CASE, COND = TC.CASE, TC.COND
CASE_A1024, COND_A1024 = TC.CASE_A1024, TC.COND_A1024
SEED = 0x5EED0000000071                      # of the selectors (tests/test_slots_gpu.py's: its _engine sets it)

# Column b is primed with LENGTHS[b mod 11] samples: unprimed and primed columns share every 16-lane row; 15 / 16 / 17 sit at the
# edges of the longest ring (16), 20 and 40 on the chunk boundaries, 48 is an utterance that is forced to its end.
LENGTHS = (0, 1, 2, 15, 16, 17, 20, 31, 40, 47, 48)
FOREIGN_SEED = 3                             # of the foreign primes' RandomState (chosen on the CPU: test_prime_cpu.py holds the
                                             # oracle to the condition of test 2 with it)


def prime_lengths(batch):
    return [LENGTHS[b % len(LENGTHS)] for b in range(batch)]


def inner_columns(lengths, N):
    """the columns that are primed, but not to their end: what follows their prime is the model's"""
    return [b for b, n in enumerate(lengths) if 0 < n < N]


def foreign_primes(A, y0):
    """[B][N] indices from a fixed RandomState that differ from y0 everywhere, with 0 and A - 1 among the forced samples of the first
    column with the longest prime (column 10, 48 samples)."""
    B, N = y0.shape
    p = np.random.RandomState(FOREIGN_SEED).randint(0, A, size=(B, N)).astype(np.int32)
    p = np.where(p == y0, (p + 1) % A, p).astype(np.int32)
    lengths = prime_lengths(B)
    n = max(lengths)
    b = lengths.index(n)
    k0 = int(np.nonzero(y0[b, :n] != 0)[0][0])
    k1 = int(np.nonzero((y0[b, :n] != A - 1) & (np.arange(n) != k0))[0][0])
    p[b, k0], p[b, k1] = 0, A - 1
    assert not (p == y0).any() and p.min() == 0 and p.max() == A - 1
    return p


def inputs(cc, precision, cache={}):
    """(case, cond model m, features x, cond weight w, network t with t.sel and t.Lh) of a case, once per (case, precision)."""
    from test_features_gpu import _cond_inputs
    key = (cc.name, precision)
    if key not in cache:
        half = precision == 16
        case, m, x, w, Lh = _cond_inputs(cc, half=half)
        t = util.gen_o1(case, half=half)
        t.sel = O.philox_selectors(SEED, case.shape.N, case.shape.B)
        t.Lh = Lh
        cache[key] = (case, m, x, w, t)
    return cache[key]


def differing_columns(y, y0, lengths):
    """the columns of inner_columns whose samples behind the prime differ somewhere from y0"""
    N = y0.shape[1]
    return [b for b in inner_columns(lengths, N) if not np.array_equal(y[b, lengths[b]:], y0[b, lengths[b]:])]
