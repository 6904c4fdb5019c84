"""Cases of the tests of scoring with carried state (tests/test_score_carry_cpu.py, tests/test_score_carry_gpu.py) and
a numpy mirror of the rules the chunk pass relies on: how a chunk [k0, k0 + n) turns the payload of its in-state into the payload of
its out-state, where the dilated tap of a sample comes from, and which history words the embedding and the out-state's header take.

Every mirror takes `mutate`, one of MUTATIONS: a deliberately wrong rule -- what a kernel that made the mistake would compute.
tests/test_score_carry_cpu.py shows that each of them differs from prefill_cases.blob_payload, or from the whole pass's tap or
history, on the cut lists below: the GPU equalities can therefore tell."""
import numpy as np

import prefill_cases as PF

# cut lists of the prime shape (8 layers, dilations 1 .. 16, 48 samples): one chunk, chunks of 1, 2, around the tile edge, twenty
# chunks of 1 then 28, and fives with a rest of 3
PRIME_N = 48
PRIME_CUTS = [(48,), (1, 47), (2, 46), (15, 33), (16, 32), (17, 31), (1,) * 20 + (28,), (5,) * 9 + (3,)]
# ... of the long schedule (12 layers, maxDilation 128) at n = 300: chunks shorter than a dilation, taps that cross two boundaries,
# out-states that must keep old slots
LONG_N = 300
LONG_CUTS = [(100, 100, 100), (127, 1, 128, 44), (129, 171), (37,) * 8 + (4,)]
assert all(sum(c) == PRIME_N for c in PRIME_CUTS) and all(sum(c) == LONG_N for c in LONG_CUTS)

MUTATIONS = ("relative_slots", "drop_old", "tap_from_rp", "own_history")


def starts(cuts):
    """[(k0, n)] of a cut list"""
    out, k = [], 0
    for n in cuts:
        out.append((k, n))
        k += n
    return out


def carry_payload(prev, xs_chunk, k0, n, L, maxD, mutate=None):
    """The payload [sum d][width] behind the chunk [k0, k0 + n): xs_chunk[l][i] = x_l[k0 + i] as a row; prev = the payload at k0 (None:
    from silence, zeros).  The chunk's last min(n, d_l) samples go to slot off_l + (k mod d_l) by the ABSOLUTE k; the rest is kept."""
    sched = PF.schedule(L, maxD)
    width = xs_chunk[0].shape[1]
    out = np.zeros((sum(d for d, _ in sched), width), dtype=xs_chunk[0].dtype) if prev is None else prev.copy()
    for l, (d, off) in enumerate(sched):
        if mutate == "drop_old" and n < d:
            out[off:off + d] = 0
        for i in range(max(0, n - d), n):
            k = i if mutate == "relative_slots" else k0 + i
            out[off + k % d] = xs_chunk[l][i]
    return out


def tap_source(l, k, k0, L, maxD, have_state=True, mutate=None):
    """Where the dilated tap x_l[k - d_l] of sample k of a chunk that starts at k0 comes from: ("row", r) = scratch row r of the chunk,
    ("slot", s) = slot s of the in-state, or ("zero",) -- before the utterance's start, or no in-state."""
    d, off = PF.schedule(L, maxD)[l]
    r, rp = k - k0, k - k0 - d
    assert r >= 0
    if rp >= 0:
        return ("row", rp)
    if have_state and k0 + rp >= 0:
        return ("slot", off + (rp if mutate == "tap_from_rp" else k0 + rp) % d)
    return ("zero",)


def embed_history(r, y_chunk, hist, mutate=None):
    """(y(k - 2), y(k - 1)) for column r of a chunk with samples y_chunk; hist = (yInPrev, yInCur) of the in-state, (128, 128) from
    silence"""
    if mutate == "own_history":
        hist = (int(y_chunk[0]), int(y_chunk[min(1, len(y_chunk) - 1)]))
    cur = int(y_chunk[r - 1]) if r >= 1 else hist[1]
    old = int(y_chunk[r - 2]) if r >= 2 else hist[1] if r == 1 else hist[0]
    return old, cur


def history_after(y_chunk, hist):
    """(yInPrev, yInCur) of the out-state's header"""
    n = len(y_chunk)
    return (int(y_chunk[n - 2]) if n >= 2 else hist[1]), int(y_chunk[n - 1])
