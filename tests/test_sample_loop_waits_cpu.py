"""Static properties of the sample loop of the straight-line kernel (wn::wavenet_wg_sl: dilation cycle AND layer count compiled in,
the kernel the L = 20 three-tile fp16 launch takes; no GPU): no wait for the whole vector-memory queue (`s_waitcnt vmcnt(0)`) inside
a sample, and fewer register copies than the cycle-loop kernel it replaces there.  Read from the built code object with
scripts/isa_stats.py, like test_code_objects_cpu.py does."""
import os
import sys

import pytest

from test_code_objects_cpu import BUILD, ROOT, kernel_table

sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_stats  # noqa: E402

OBJ = "inst_64_256_256_p16.o"
# copies (v_accvgpr_mov/read/write, v_mov_b32/_b64) in the sample loop of wn::wavenet_wg_cs<true, 64, 256, 256, 3, EMB, 10, LD> of the parent
# commit, measured once with `isa_stats.py mix` (profiles/r09_isa_mix.txt): {(EMB, LD): copies}
PARENT_COPIES = {("true", 1): 333, ("true", 2): 381, ("false", 1): 331, ("false", 2): 383}
_loops = {}


def _sample_loops():
    if not os.path.exists(os.path.join(BUILD, OBJ)):
        pytest.skip("build the library first (__graft_entry__.build())")
    if not _loops:
        _loops.update(isa_stats.sample_loop(OBJ, "wn::wavenet_wg_sl<"))
    return _loops


@pytest.mark.parametrize("ld", (1, 2))
@pytest.mark.parametrize("emb", ("true", "false"))
def test_no_full_drain_inside_a_sample_and_fewer_copies(emb, ld):
    """EMB = true: no vmcnt(0) at all.  EMB = false: exactly one, and it is no fallback of the wait-count pass: with no embedding
    table in LDS the first instruction of a sample that needs anything is the conversion of the current tap's embedding row, gathered
    from memory by the pick that closed the previous sample (one barrier earlier) -- the YOUNGEST request in the queue, so the exact
    count of that wait is zero.  It stands in front of the sample's first barrier, where it is checked to be."""
    name = "wn::wavenet_wg_sl<true,64,256,256,3,%s,10,2,%d>" % (emb, ld)
    loops = _sample_loops()
    assert name in loops, sorted(loops)
    drains, copies, total = loops[name]
    print("%s: %d full drains, %d copies, %d instructions in the sample loop" % (name, drains, copies, total))
    assert drains == (0 if emb == "true" else 1), (name, drains)
    if drains:
        (_, lines, lps), = isa_stats.kernels_of(OBJ, name)
        lo, hi = sorted(lps, key=lambda l: l[0] - l[1])[0]
        at = [i for i in range(lo, hi + 1) if isa_stats.is_full_drain(lines[i][1], lines[i][2])][0]
        first_barrier = [i for i in range(lo, hi + 1) if lines[i][1] == "s_barrier"][0]
        assert at < first_barrier, "the full drain is not the wait for the embedding gather at the top of the sample"
        before = [lines[i][1] for i in range(lo, at)]
        assert any(op.startswith("global_load") for op in before) and not any(op.startswith("buffer_load") for op in before), before
    assert copies < PARENT_COPIES[(emb, ld)], (name, copies)


def test_straight_line_kernels_fit_the_register_files_without_scratch():
    if not os.path.exists(os.path.join(BUILD, OBJ)):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table(OBJ) if r[0].startswith("wn::wavenet_wg_sl<")]
    assert len(rows) == 4, rows
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0, (name, scratch, spill)
        assert vgpr <= 512 and agpr <= 256 and sgpr <= 106, (name, vgpr, agpr, sgpr)
