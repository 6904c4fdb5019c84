"""Cases of the tests that hold the time-parallel pass -- prefill, scoring, scoring with carried state -- at the
edges of the layer / dilation schedule and without the embedding tanh (tests/test_time_edges_cpu.py, tests/test_time_edges_gpu.py).

The pass states the schedule again in three places of its own: nvWavenetInfer::timeModel() (d, off, dOut, offOut per layer),
time_finish_kernel (dil_next and the residues a chunk does not reach) and prefill_window / prefill_first (the first sample t0 of a
prime's window).  The runs are those of tests/schedule_edges.py, which the generation kernels are held at: every layer d = 1; a
maxDilation that is no power of two, or is never reached; a dilation of 1024, larger than every chunk; and as many layers as the
library accepts.  Networks and features are those of score_cases.setup (the O(1) recipe, 80 feature channels), samples those of
prefill_cases.primes (0 and A - 1 among them).

Per run, with D the largest dilation and W = prefill_cases.window(L, maxDilation):

  kind      samples N               scored lengths   prefill lengths (one prefillStates call)        cut lists of a scored length n
  general   max(48, W + 17)         47, 48           1, 2, W - 1, W, W + 1, 17, 48, W + 17           (n,), (1, n - 1), (D, n - D), (D + 1, n - D - 1),
                                                                                                     (17, n - 17), fives with a rest
  long      1100   [(11, 1024)]     1100             300, 1023, 1024, 1025, 1100                     (300, 300, 300, 200), (1023, 1, 76), (1024, 76),
                                                                                                     (1025, 75)
  lmax      W + 17 [(Lmax, 2)]      48, N            17, W - 1, W, W + 1, W + 17                     (17, n - 17), (W, n - W), fives with a rest

(a cut list whose pieces would not be positive at a length is not formed there: (D, n - D) needs D < n, (W, n - W) needs W < n).
W + 17 starts the pass at t0 = 16, past sample 0, over a chunk of W + 1 samples; on the short windows 48 starts it at 16 or 32.  At
(11, 1024) a prime of 300 leaves the rings of d = 512 and d = 1024 mostly unwritten, and the cuts of 300 cross sample 1024 with d > n
and an in-state whose slots must be kept."""
import prefill_cases as PF
import schedule_edges as E
import score_cases as SC

RUNS = E.RUNS
run_id = E.run_id
COLUMNS = 3
TILE = PF.TILE


def kind_of(run):
    shape, L, maxD = run
    return "lmax" if L == "Lmax" else "long" if maxD == 1024 else "general"


def layers_of(run, lmax=None):
    """L of a run; "Lmax" is what the caller found the library to accept (test_schedule_edges_gpu.lmax; schedule_edges.L_MAX where no
    GPU decides it)"""
    L = run[1]
    if L == "Lmax":
        assert lmax and 2 <= lmax <= E.L_MAX, "resolve Lmax first"
        L = lmax
    return L


def seed_of(run, L):
    """seed of util.gen_o1: that of schedule_edges.case_of"""
    return 7000 + 37 * L + run[2] + E.SHAPES[run[0]][0]


def largest_dilation(L, maxD):
    return max(E.dilations(L, maxD))


def fives(n):
    return (5,) * (n // 5) + ((n % 5,) if n % 5 else ())


def _unique(seq):
    out = []
    for v in seq:
        if v not in out:
            out.append(v)
    return out


class Table:
    """the lengths and cut lists of one run at L layers"""

    def __init__(self, run, L):
        shape, _, maxD = run
        self.run, self.kind, self.L, self.maxD = run, kind_of(run), L, maxD
        self.shape = E.SHAPES[shape]
        self.seed = seed_of(run, L)
        self.D = D = largest_dilation(L, maxD)
        self.W = W = PF.window(L, maxD)
        if self.kind == "general":
            self.N = max(48, W + 17)
            self.scored = (47, 48)
            self.prefill = _unique([1, 2, W - 1, W, W + 1, 17, 48, W + 17])
            self.rows_at = 47
        elif self.kind == "long":
            self.N = 1100
            self.scored = (1100,)
            self.prefill = [300, 1023, 1024, 1025, 1100]
            self.rows_at = 1100
        else:
            self.N = W + 17
            self.scored = (48, self.N)
            self.prefill = _unique([17, W - 1, W, W + 1, W + 17])
            self.rows_at = 48
        assert all(1 <= n <= self.N for n in self.prefill) and all(1 <= n <= self.N for n in self.scored) and self.rows_at in self.scored

    def cuts(self, n):
        """the cut lists of the scored length n"""
        D, W = self.D, self.W
        if self.kind == "long":
            lists = [(300, 300, 300, 200), (1023, 1, 76), (1024, 76), (1025, 75)]
        elif self.kind == "lmax":
            lists = [(17, n - 17)] + ([(W, n - W)] if W < n else []) + [fives(n)]
        else:
            lists = [(n,), (1, n - 1)] + ([(D, n - D)] if D < n else []) + ([(D + 1, n - D - 1)] if D + 1 < n else []) + [(17, n - 17), fives(n)]
        lists = _unique(lists)
        assert all(sum(c) == n and min(c) >= 1 for c in lists), (self.run, n, lists)
        return lists

    def t0(self, n):
        return PF.first_tile_sample(n, self.L, self.maxD)

    def positions(self, n):
        """score_cases.positions and the samples around the largest dilation"""
        D = self.D
        return sorted(set(SC.positions(n)) | {k for k in (D - 1, D, D + 1) if 0 <= k < n})

    def wrong_maxD(self):
        """another maxDilation for the negative controls: doubled, 1024 halved; None where that is the same schedule"""
        wrong = self.maxD // 2 if self.maxD == 1024 else 2 * self.maxD
        return wrong if E.dilations(self.L, wrong) != E.dilations(self.L, self.maxD) else None

    def what(self):
        return "%s (%d, %d)" % (self.run[0], self.L, self.maxD)


def table(run, lmax=None):
    return Table(run, layers_of(run, lmax))


def chunks_with_state(tb):
    """(k0, n) of every chunk of the run's cut lists that has an in-state"""
    return [(k0, m) for n in tb.scored for cuts in tb.cuts(n) for k0, m in _starts(cuts) if k0 > 0]


def _starts(cuts):
    out, k = [], 0
    for n in cuts:
        out.append((k, n))
        k += n
    return out


def keeps_old_slots(tb):
    """some chunk with an in-state is shorter than the largest dilation: its out-state must keep slots of the in-state"""
    return any(m < tb.D for _, m in chunks_with_state(tb))


# ---- what the tables are meant to reach, asserted on the tables themselves ----------------------------------------------------------

def _check_tables():
    short = []
    for run in RUNS:
        for lmax in ((E.L_MAX, E.L_MAX - 1) if run[1] == "Lmax" else (None,)):          # (an even and an odd layer count)
            tb = table(run, lmax)
            if tb.kind != "long":
                # W + 17 starts past sample 0, over a chunk of W + 1 samples
                assert tb.t0(tb.W + 17) == 16 and tb.W + 17 in tb.prefill, tb.what()
                assert tb.t0(tb.W) == tb.t0(tb.W + 1) == 0
            else:
                assert tb.W == 2049 and all(tb.t0(n) == 0 for n in tb.prefill)
                # d > n on chunks with an in-state: the cuts of 300 (d = 512, 1024) and the chunk of one sample at 1023
                assert (300, 300) in chunks_with_state(tb) and (1023, 1) in chunks_with_state(tb) and tb.D == 1024 > 300
            short += [(tb.what(), n) for n in tb.prefill if tb.t0(n) > 0 and n - tb.t0(n) < TILE]
    # every layer d = 1: W = 4 and 22, and 48 samples start the pass at 32 and at 16
    for L, W, t0 in ((2, 4, 32), (20, 22, 16)):
        tb = table(("R32", L, 1))
        assert (tb.W, tb.D, tb.t0(48)) == (W, 1, t0) and 48 in tb.prefill, tb.what()
    # a prefill chunk shorter than a tile behind t0 > 0 (yBefore = 2: the embedding's history words lie in front of the window)
    assert ("R32 (2, 1)", 21) in short and ("R32 (5, 3)", 26) in short, short
    assert table(("R32", "Lmax", 2), 128).W == 194 and table(("R32", 4, 512)).D == 8


_check_tables()
