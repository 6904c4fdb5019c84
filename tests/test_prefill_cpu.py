"""CPU tests of prefill (no GPU): the new entries are declared and exported; the window W and the per-layer reach
that the pass relies on are properties of the model, shown on the committed oracle, teacher-forced; the rule that places x_l[k]
in a state blob matches a numpy model; and the prefill kernels of the built object use no scratch memory and spill nothing."""
import os
import re

import numpy as np
import pytest

import cases
import prefill_cases as PF
import util
from oracle import oracle as O
from test_code_objects_cpu import BUILD, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nvw_prefill_window", "nvw_prefill_states")


def test_the_prefill_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert re.search(r"int nvw_prefill_window\(nvw_engine\* e\);", header)
    assert re.search(r"int nvw_prefill_states\(nvw_engine\* e, const nvw_prefill_req\* reqs, int count, void\* dst, long long stride, void\* stream\);", header)
    m = re.search(r"typedef struct \{([^}]*)\} nvw_prefill_req;", header)
    assert m and [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "const int* y", "int n", "const void* x", "int precision", "long long c_stride, t_stride", "unsigned uid", "float temperature"]
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import PREFILL_REQ, WavenetEngine
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert PREFILL_REQ.itemsize == 56 and [PREFILL_REQ.fields[k][1] for k in PREFILL_REQ.names] == [0, 8, 16, 24, 32, 40, 48, 52]
    assert callable(WavenetEngine.prefillStates) and callable(WavenetEngine.prefillWindow)
    from nv_wavenet_amd.slots import SlotStream
    assert callable(SlotStream.prefill)


def test_the_schedule_mirror():
    assert [d for d, _ in PF.schedule(8, 16)] == [1, 2, 4, 8, 16, 1, 2, 4] and PF.window(8, 16) == 40
    assert sum(d for d, _ in PF.schedule(12, 128)) == 270 and PF.window(12, 128) == 272
    assert sum(d for d, _ in PF.schedule(20, 512)) == 2046          # (the headline model: W = 2048)
    assert [PF.first_tile_sample(n, 8, 16) for n in (1, 40, 47, 48, 56, 57)] == [0, 0, 0, 0, 16, 16]
    for L, maxD in ((8, 16), (12, 128)):
        assert PF.reach(L - 1, L, maxD) == PF.window(L, maxD)
        assert [PF.valid_from(100, l, L, maxD) for l in (0, L - 1)] == [100 - PF.window(L, maxD) + 2, 100 - PF.schedule(L, maxD)[-1][0]]
        # a layer's ring reads back d_l samples from n: every one of them is computed from complete taps
        assert all(PF.valid_from(100, l, L, maxD) <= 100 - PF.schedule(L, maxD)[l][0] for l in range(L))


def _layer_outputs(case, t, histories, n):
    """Xout [L][B][R] of sample n (every layer's output there) of the oracle forced through `histories` [B][n + 1]"""
    s = case.shape
    o = O.Oracle(s.L, s.B, n + 1, s.R, s.S, s.A, s.maxD)
    o.set_model(t)
    o.set_tanh_embed(True)
    o.set_inputs(np.ascontiguousarray(t.Lh[:n + 1]), np.ascontiguousarray(t.sel[:n + 1]))
    o.run(n + 1, forced=np.ascontiguousarray(histories, dtype=np.int32))
    X = o.getters()["Xout"]
    o.close()
    return X


@pytest.mark.parametrize("L,maxD,n", [(8, 16, 44), (12, 128, 280)])
def test_the_window_rule_on_the_teacher_forced_oracle(L, maxD, n):
    """Column 0: a history.  Column 1: another one before sample n - W, the same from there on -> every layer's output at sample n
    is IDENTICAL (the state after n samples depends on the last W only).  Column 2 + l: differs from column 0 at the one sample
    n - reach(l) -- the oldest that layer l's output at sample n reads -- -> layers below l are identical, layer l is not; for l = L - 1
    that sample is n - W, the oldest of the window."""
    W = PF.window(L, maxD)
    B = 2 + L
    case = cases.Case("prefill_window", 921, [], cases.Shape(32, 128, 256, L, B, n + 1, maxD), 1, 1, 16)
    t = util.gen_o1(case, half=False)
    t.Lh[:] = t.Lh[:, :, :1]                                          # the same conditioning for every column
    rng = np.random.RandomState(9)
    base = rng.randint(0, 256, size=n + 1).astype(np.int32)
    h = np.tile(base, (B, 1))
    h[1, :n - W] = (h[1, :n - W] + 1 + rng.randint(0, 255, size=n - W)) % 256
    for l in range(L):
        at = n - PF.reach(l, L, maxD)
        h[2 + l, at] = (h[2 + l, at] + 128) % 256
    assert (h[1, :n - W] != base[:n - W]).all() and np.array_equal(h[1, n - W:], base[n - W:])
    X = _layer_outputs(case, t, h, n)
    assert np.array_equal(X[:, 1], X[:, 0]), "samples before n - W reach a layer's output at sample n"
    for l in range(L):
        assert np.array_equal(X[:l, 2 + l], X[:l, 0]), "layer %d: a sample beyond the reach of the layers below it reaches them" % l
        assert not np.array_equal(X[l, 2 + l], X[l, 0]), "layer %d: the oldest sample of its reach does not reach it" % l


@pytest.mark.parametrize("L,maxD", [(8, 16), (12, 128)])
def test_the_blob_slot_rule_against_a_numpy_model(L, maxD):
    """x_l[k] lies in slot off_l + (k mod d_l); after n samples a slot holds the latest such k < n, zero where there is none -- for
    n below, at and above every dilation.  The pass writes x_l[k] for k in [max(0, n - d_l), n) and zeroes residues n .. d_l - 1."""
    sched = PF.schedule(L, maxD)
    xs = [np.arange(1, 400 + 1, dtype=np.int64)[:, None] * 1000 + l for l in range(L)]      # x_l[k] = (k + 1) * 1000 + l: never zero
    for n in sorted({1, 2, 3, 15, 16, 17, maxD - 1, maxD, maxD + 1, 2 * maxD + 5, 300}):
        model = PF.blob_payload(xs, n, L, maxD)
        mine = np.zeros_like(model)
        written = np.zeros(len(model), dtype=int)
        for l, (d, off) in enumerate(sched):
            for k in range(max(0, n - d), n):
                mine[PF.blob_slot(l, k, L, maxD)] = xs[l][k]
                written[PF.blob_slot(l, k, L, maxD)] += 1
            for i in range(n, d):
                written[off + i] += 1                                 # (the blob step's zeroes)
        assert np.array_equal(mine, model), n
        assert (written == 1).all(), "n = %d: a slot is written twice or not at all" % n
        for l, (d, off) in enumerate(sched):
            assert (model[off:off + d] == 0).all(axis=1).sum() == max(0, d - n)


def test_the_prefill_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "prefill.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table("prefill.o") if "::time_" in r[0]]
    layer = [r for r in rows if "time_layer_kernel<" in r[0]]
    embed = [r for r in rows if "time_embed_kernel<" in r[0]]
    finish = [r for r in rows if "time_finish_kernel<" in r[0]]
    # R in {32, 64, 128, 256} x two precisions, all without the skip path (S = 0) and the in-state taps; two embedding and two
    # finish kernels
    assert len(layer) == 8 and len(embed) == 2 and len(finish) == 2 and len(rows) == 12, [r[0] for r in rows]
    assert all(re.search(r"time_layer_kernel<(true|false), \d+, 0, false>", r[0]) for r in layer), [r[0] for r in layer]
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr <= 512 and agpr <= 256, (name, vgpr, agpr, scratch, spill)
