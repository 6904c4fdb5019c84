"""CPU tests of scoring (no GPU): the new entries are declared, bound and exported; the float64 reference of
tests/score_cases.py is held to the committed oracle, teacher-forced, at the tile edges, the first samples, the last one and around
the longest dilation; deliberately broken references miss by more than ten bars; the reference's own distribution contains the
oracle's draws in the picked bins; and the score kernels of the built object use no scratch memory and spill nothing."""
import copy
import os
import re

import numpy as np
import pytest

import cases
import score_cases as SC
import util
from oracle import oracle as O
from test_code_objects_cpu import BUILD, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nvw_score_max_samples", "nvw_score_samples")


def test_the_score_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert re.search(r"int nvw_score_max_samples\(nvw_engine\* e\);", header)
    assert re.search(r"int nvw_score_samples\(nvw_engine\* e, const nvw_score_req\* reqs, int count, void\* stream\);", header)
    m = re.search(r"typedef struct \{([^}]*)\} nvw_score_req;", header)
    assert m and [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "const int* y", "int n", "const void* x", "int precision", "long long c_stride, t_stride", "float temperature", "float* logp",
        "float* rows"]
    assert "SCORING" in header
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import SCORE_REQ, WavenetEngine
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert SCORE_REQ.itemsize == 72 and [SCORE_REQ.fields[k][1] for k in SCORE_REQ.names] == [0, 8, 16, 24, 32, 40, 48, 56, 64]
    assert callable(WavenetEngine.scoreSamples) and callable(WavenetEngine.scoreMaxSamples)
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    from nv_wavenet_amd.slots import SlotStream
    assert callable(NVWaveNetEngine.score) and callable(SlotStream.score)


def _network(shape, seed, L, maxD, N, columns):
    """(case, t with t.Lh = Wcond x + bcond of prefill_cases.features, Lh per column [columns][N][L][2R] float64, y [columns][N])"""
    case, t, x, w, b = SC.setup(shape, seed, 32, L, maxD, N, columns)
    lh = np.stack([SC.lh_of(x[c], w, b, shape[0], L) for c in range(columns)])
    t.Lh = np.ascontiguousarray(lh.transpose(1, 2, 0, 3).astype(np.float32))              # [N][L][B][2R]
    return case, t, lh, SC.PF.primes(columns, N, shape[2])


def _oracle_at(case, t, y, k):
    """the oracle forced through y, run to k + 1 samples: its Za and P [B][A] are those of sample k"""
    ck = case._replace(shape=case.shape._replace(N=k + 1))
    tk = copy.copy(t)
    tk.Lh, tk.sel = np.ascontiguousarray(t.Lh[:k + 1]), np.ascontiguousarray(t.sel[:k + 1])
    return util.teacher_forced_oracle(ck, tk, np.ascontiguousarray(y[:, :k + 1]))


@pytest.mark.parametrize("which", ["prime_shape", "long"])
def test_the_float64_reference_matches_the_teacher_forced_oracle(which):
    """Within the fp32 bar, logits and log-probability of the forced sample, at every position of score_cases.positions."""
    shape, seed, L, maxD, N = SC.PRIME_SHAPE if which == "prime_shape" else SC.LONG
    n = N if which == "prime_shape" else SC.LONG_N
    columns = 2
    case, t, lh, y = _network(shape, seed, L, maxD, N, columns)
    refs = [SC.reference(t, case.shape, y[c, :n], lh[c].astype(np.float32)) for c in range(columns)]
    worst = 0.0
    for k in SC.positions(n, long=which == "long"):
        o = _oracle_at(case, t, y, k)
        for c in range(columns):
            Za, logp = refs[c]
            top = np.abs(Za).max()
            dz = np.abs(o["Za"][c] - Za[k]).max()
            assert dz <= (cases.TOL["Za"] + 32 * SC.EPS32) * top, (which, k, c, dz)
            dl = abs(np.log(np.float64(o["P"][c, y[c, k]])) - logp[k])
            worst = max(worst, dl / SC.bar(Za, 1.0, 32))
            assert dl <= SC.bar(Za, 1.0, 32), (which, k, c, dl, SC.bar(Za, 1.0, 32))
    print("float64 reference against the oracle, %s: worst |d logp| = %.3g bars (fp32)" % (which, worst))


@pytest.mark.parametrize("mutation", SC.MUTATIONS)
def test_a_broken_reference_misses_by_more_than_ten_bars(mutation):
    """Negative controls: each mutation of the float64 model moves some logp by more than ten bars of BOTH precisions (the fp16
    bar is the wider one) -- a kernel that made the same mistake would not pass."""
    shape, seed, L, maxD, N = SC.PRIME_SHAPE
    case, t, lh, y = _network(shape, seed, L, maxD, N, 2)
    T = 0.7 if mutation == "ignore_T" else 1.0
    Za, logp = SC.reference(t, case.shape, y[0], lh[0], T)
    _, bad = SC.reference(t, case.shape, y[0], lh[0], T, mutate=mutation)
    moved = np.abs(bad - logp).max()
    wide = max(SC.bar(Za, T, 16), SC.bar(Za, T, 32))
    print("%s moves logp by %.3g = %.1f fp16 bars" % (mutation, moved, moved / wide))
    assert moved > 10 * wide, (mutation, moved, wide)


def test_the_reference_distribution_contains_the_oracles_draws():
    """The oracle's own free run (t.sel, 16 columns x 48 samples), scored by the float64 reference: the CDF built from exp(rows)
    has C[y-1] <= u < C[y] for at least util.FP16_MIN_AGREEMENT of the samples, and every miss is an adjacent bin (the oracle sums
    its CDF in fp32).  The GPU test of the same name can therefore be passed."""
    shape, seed, L, maxD, N = SC.PRIME_SHAPE
    columns = 16
    case, t, lh, _ = _network(shape, seed, L, maxD, N, columns)
    o = O.Oracle(L, columns, N, *shape, maxD)
    o.set_model(t)
    o.set_tanh_embed(True)
    o.set_inputs(t.Lh, t.sel)
    y = o.run(N)
    o.close()
    inside, total = 0, 0
    for c in range(columns):
        Za, logp = SC.reference(t, case.shape, y[c], lh[c])
        ok, bins, edge = SC.cdf_check(SC.log_softmax(Za), y[c].astype(np.int64), t.sel[:N, c].astype(np.float64))
        assert (bins[~ok] <= 1).all(), (c, np.nonzero(~ok)[0], bins[~ok])
        inside += int(ok.sum())
        total += N
    print("draws inside the picked bin: %d of %d" % (inside, total))
    assert inside >= util.FP16_MIN_AGREEMENT * total


def test_the_score_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "score.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table("score.o") if "score_" in r[0] or "::time_" in r[0]]
    head = [r for r in rows if "score_head_kernel<" in r[0]]
    # (waves, S, A) of the eight built shapes, two precisions; the layer kernels of the (R, S) are score_carry.o's, for the whole
    # pass and the chunks, and are counted there (tests/test_score_carry_cpu.py)
    assert len(head) == 12 and len(rows) == 12, [r[0] for r in rows]
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr <= 512 and agpr <= 256, (name, vgpr, agpr, scratch, spill)
