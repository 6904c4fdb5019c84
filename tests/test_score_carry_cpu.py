"""CPU tests of scoring with carried state (no GPU): the new entries and request structs are declared, bound and
exported; the carry rule of tests/score_carry_cases.py -- the chunk's last min(n, d_l) samples to slots by absolute k, the rest kept
-- reproduces prefill_cases.blob_payload at every cut of fixed and random cut lists on both schedules; the tap of every sample comes
from the place that holds what the whole pass reads; deliberately wrong rules differ on those inputs; and the kernels of the built
object are the expected ones, use no scratch memory and spill nothing."""
import inspect
import os
import re

import numpy as np
import pytest

import prefill_cases as PF
import score_carry_cases as CC
import score_cases as SC
from test_code_objects_cpu import BUILD, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHUNK_FIELDS = ["const void* state", "const int* y", "int n", "const void* x", "int precision", "long long c_stride, t_stride", "unsigned uid",
                "float temperature", "float* logp", "float* rows", "void* state_out"]
CHUNK_MEL_FIELDS = ["const void* state", "const int* y", "int n", "const void* mel", "int precision", "long long c_stride, f_stride", "int frames",
                    "unsigned uid", "float temperature", "float* logp", "float* rows", "void* state_out"]


def test_the_chunk_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert re.search(r"int nvw_score_chunks\(nvw_engine\* e, const nvw_score_chunk_req\* reqs, int count, void\* stream\);", header)
    assert re.search(r"int nvw_score_chunks_mel\(nvw_engine\* e, const nvw_score_chunk_mel_req\* reqs, int count, void\* stream\);", header)
    for name, fields in (("nvw_score_chunk_req", CHUNK_FIELDS), ("nvw_score_chunk_mel_req", CHUNK_MEL_FIELDS)):
        m = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header)
        assert m and [f.strip() for f in m.group(1).split(";") if f.strip()] == fields, name
    assert "SCORING WITH CARRIED STATE" in header
    assert "Scoring in time chunks with carried state (utterances\n * past the cap), and on" not in header, "still listed as not offered"
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import SCORE_CHUNK_MEL_REQ, SCORE_CHUNK_REQ, WavenetEngine
    for name in ("nvw_score_chunks", "nvw_score_chunks_mel"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    # the C layout on the LP64 targets the library is built for: pointers and long long 8-byte aligned
    assert SCORE_CHUNK_REQ.itemsize == 88
    assert [SCORE_CHUNK_REQ.fields[k][1] for k in SCORE_CHUNK_REQ.names] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80]
    assert list(SCORE_CHUNK_REQ.names) == ["state", "y", "n", "x", "precision", "c_stride", "t_stride", "uid", "temperature", "logp", "rows", "state_out"]
    assert SCORE_CHUNK_MEL_REQ.itemsize == 96
    assert [SCORE_CHUNK_MEL_REQ.fields[k][1] for k in SCORE_CHUNK_MEL_REQ.names] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80, 88]
    assert callable(WavenetEngine.scoreChunks) and callable(WavenetEngine.scoreChunksMel)
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    from nv_wavenet_amd.slots import SlotStream
    assert callable(SlotStream.score_from)
    for fn in (NVWaveNetEngine.score, NVWaveNetEngine.score_mel):
        params = inspect.signature(fn).parameters
        assert params["chunk"].default is None and params["return_state"].default is False, fn


def test_the_field_offsets_are_those_of_the_c_structs(tmp_path):
    """offsetof and sizeof from the header itself, through the host compiler"""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    from nv_wavenet_amd.engine import SCORE_CHUNK_MEL_REQ, SCORE_CHUNK_REQ
    lines = []
    for struct, dt in (("nvw_score_chunk_req", SCORE_CHUNK_REQ), ("nvw_score_chunk_mel_req", SCORE_CHUNK_MEL_REQ)):
        for k in dt.names:
            lines.append('printf("%%s.%%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (struct, k, struct, k))
        lines.append('printf("%%s %%zu\\n", "%s", sizeof(%s));' % (struct, struct))
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nv_wavenet_c.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "offsets"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for struct, dt in (("nvw_score_chunk_req", SCORE_CHUNK_REQ), ("nvw_score_chunk_mel_req", SCORE_CHUNK_MEL_REQ)):
        assert int(got[struct]) == dt.itemsize
        for k in dt.names:
            assert int(got["%s.%s" % (struct, k)]) == dt.fields[k][1], (struct, k)


# ---- the carry rule ----------------------------------------------------------------------------------------------------------------

SCHEDULES = {"prime_shape": (SC.PRIME_SHAPE[2], SC.PRIME_SHAPE[3], CC.PRIME_N, CC.PRIME_CUTS),
             "long": (SC.LONG[2], SC.LONG[3], CC.LONG_N, CC.LONG_CUTS)}


def _xs(L, N, seed=3, width=4):
    rng = np.random.RandomState(seed)
    return [rng.standard_normal((N, width)).astype(np.float32) + 1.0 for _ in range(L)]      # (no row is zero)


def _random_cuts(L, maxD, N, count=6, seed=11):
    """cut lists that between them hold 1, every dilation - 1, every dilation + 1 and sizes off the tile grid -- dealt out over the
    lists, largest first to the emptiest list -- each in random order and filled up with random sizes"""
    rng = np.random.RandomState(seed)
    ds = sorted({d for d, _ in PF.schedule(L, maxD)})
    must = sorted([1] + [d - 1 for d in ds if d > 1] + [d + 1 for d in ds], reverse=True)
    share = [[] for _ in range(count)]
    for n in must:
        min(share, key=sum).append(n)
    assert all(sum(s) <= N for s in share)
    out = []
    for s in share:
        cuts, left = list(s), N - sum(s)
        while left > 0:
            n = min(int(rng.randint(1, 2 * maxD + 1)), left)
            cuts.append(n)
            left -= n
        out.append(tuple(int(n) for n in rng.permutation(cuts)))
    return out


def _walk(xs, cuts, L, maxD, mutate=None):
    """the payload after every cut, by the carry rule"""
    out, prev = [], None
    for k0, n in CC.starts(cuts):
        prev = CC.carry_payload(prev, [x[k0:k0 + n] for x in xs], k0, n, L, maxD, mutate)
        out.append((k0 + n, prev))
    return out


@pytest.mark.parametrize("which", sorted(SCHEDULES))
def test_the_carry_rule_gives_the_prefill_payload_at_every_cut(which):
    L, maxD, N, fixed = SCHEDULES[which]
    xs = _xs(L, N)
    lists = list(fixed) + _random_cuts(L, maxD, N)
    sizes = {n for cuts in lists for n in cuts}
    ds = sorted({d for d, _ in PF.schedule(L, maxD)})
    assert 1 in sizes and all(d + 1 in sizes for d in ds) and all(d - 1 in sizes for d in ds if d > 1) and any(n % 16 for n in sizes)
    assert any(k0 % 16 for cuts in lists for k0, _ in CC.starts(cuts))
    want = {}
    for cuts in lists:
        assert sum(cuts) == N
        for done, payload in _walk(xs, cuts, L, maxD):
            if done not in want:
                want[done] = PF.blob_payload(xs, done, L, maxD)
            assert np.array_equal(payload, want[done]), (which, cuts, done)


@pytest.mark.parametrize("which", sorted(SCHEDULES))
def test_every_tap_comes_from_where_the_whole_pass_reads_it(which):
    """x_l[k - d_l] of the whole pass (zero before the start) is the scratch row, the in-state's slot, or the zero operand that
    tap_source names -- with the in-state's payload that of prefill at k0, and a zero operand whatever it holds without one"""
    L, maxD, N, fixed = SCHEDULES[which]
    xs = _xs(L, N)
    sched = PF.schedule(L, maxD)
    kinds = set()
    for cuts in fixed:
        for k0, n in CC.starts(cuts):
            state = PF.blob_payload(xs, k0, L, maxD)
            for l, (d, off) in enumerate(sched):
                for k in range(k0, k0 + n):
                    want = xs[l][k - d] if k - d >= 0 else np.zeros_like(xs[l][0])
                    src = CC.tap_source(l, k, k0, L, maxD, have_state=k0 > 0)
                    got = xs[l][k0 + src[1]] if src[0] == "row" else state[src[1]] if src[0] == "slot" else np.zeros_like(want)
                    assert np.array_equal(got, want), (cuts, k0, l, k, src)
                    kinds.add(src[0])
                    if k0 == 0:
                        assert CC.tap_source(l, k, k0, L, maxD, have_state=False)[0] in ("row", "zero")
    assert kinds == {"row", "slot", "zero"}


def test_the_history_words_are_those_of_the_whole_pass():
    y = PF.primes(1, CC.PRIME_N, 256)[0]
    whole = lambda k: (int(y[k - 2]) if k >= 2 else 128, int(y[k - 1]) if k >= 1 else 128)
    for cuts in CC.PRIME_CUTS:
        hist = (128, 128)
        for k0, n in CC.starts(cuts):
            for r in range(n):
                assert CC.embed_history(r, y[k0:k0 + n], hist) == whole(k0 + r), (cuts, k0, r)
            hist = CC.history_after(y[k0:k0 + n], hist)
            assert hist == whole(k0 + n), (cuts, k0)


@pytest.mark.parametrize("mutation", CC.MUTATIONS)
def test_a_wrong_rule_differs(mutation):
    """Negative controls: slots indexed by the chunk-relative sample, old slots dropped when n < d_l, the tap slot taken from rp
    instead of k0 + rp, the history taken from the chunk's own first samples -- each differs from the whole pass on the cut lists
    the GPU tests run."""
    assert mutation in CC.MUTATIONS
    differs = {}
    for which, (L, maxD, N, fixed) in sorted(SCHEDULES.items()):
        xs = _xs(L, N)
        sched = PF.schedule(L, maxD)
        hit = 0
        for cuts in fixed:
            if mutation in ("relative_slots", "drop_old"):
                hit += any(not np.array_equal(p, PF.blob_payload(xs, done, L, maxD)) for done, p in _walk(xs, cuts, L, maxD, mutation))
            elif mutation == "tap_from_rp":
                bad = False
                for k0, n in CC.starts(cuts):
                    state = PF.blob_payload(xs, k0, L, maxD)
                    for l, (d, off) in enumerate(sched):
                        for k in range(k0, min(k0 + n, k0 + d)):
                            src = CC.tap_source(l, k, k0, L, maxD, have_state=k0 > 0, mutate=mutation)
                            if src[0] == "slot" and not np.array_equal(state[src[1]], xs[l][k - d]):
                                bad = True
                hit += bad
            else:
                y = PF.primes(1, N, 256)[0]
                bad = False
                hist = (128, 128)
                for k0, n in CC.starts(cuts):
                    for r in range(min(n, 2)):
                        k = k0 + r
                        whole = (int(y[k - 2]) if k >= 2 else 128, int(y[k - 1]) if k >= 1 else 128)
                        bad = bad or CC.embed_history(r, y[k0:k0 + n], hist, mutate=mutation) != whole
                    hist = CC.history_after(y[k0:k0 + n], hist)
                hit += bad
        differs[which] = hit
        # (not every list tells: a single chunk from silence carries nothing, and a cut at 16 is a multiple of every dilation of
        # the prime shape -- but on each schedule some list does)
        assert hit >= 1, (mutation, which)
    print("%s: differs on %s cut lists" % (mutation, differs))


# ---- the built object --------------------------------------------------------------------------------------------------------------

def test_the_carry_kernels_are_the_expected_ones_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "score_carry.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table("score_carry.o") if "::time_" in r[0]]
    layer = [r for r in rows if "time_layer_kernel<" in r[0]]
    embed = [r for r in rows if "time_embed_kernel<" in r[0]]
    finish = [r for r in rows if "time_finish_kernel<" in r[0]]
    # the six (R, S) of the eight built shapes in two precisions, with the in-state taps -- the whole pass runs them too --; two
    # embedding and two finish kernels; the head is score.o's
    assert len(layer) == 12 and len(embed) == 2 and len(finish) == 2 and len(rows) == 16, [r[0] for r in rows]
    assert all(re.search(r"time_layer_kernel<(true|false), \d+, (128|256), true>", r[0]) for r in layer), [r[0] for r in layer]
    assert not [r for r in kernel_table("score_carry.o") if "score_head_kernel" in r[0]], "a second copy of the head"
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr <= 512 and agpr <= 256, (name, vgpr, agpr, scratch, spill)
