"""The LDS layout of wn::wavenet_wg, checked on the host from the Cfg constants (no GPU): tests/cpp/lds_layout.hip, compiled
host-only against nv_wavenet_amd/csrc/wn_kernels.hpp for every (R, S, A, precision) the library's Makefile instantiates and every
tile count the engine builds for it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nv_wavenet_amd", "csrc")


def _instances():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*=\s*(.*)$" % name, mk, re.M).group(1).split()
    inst = ["X(%s,%s)" % (s.replace("_", ","), p) for s in var("SHAPES") for p in var("PRECS")]
    inst += ["X(%s)" % e.replace("_p", "_").replace("_", ",") for e in var("EXTRA_INST")]
    return inst


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_layout") / "lds_layout")
    inst = _instances()
    assert "X(64,256,256,16)" in inst and len(inst) >= 16, inst
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-x", "hip", "-O1", "-std=c++17", "-Wno-unused-result",
                        "-DWN_LAYOUT_INSTANCES=" + " ".join(inst), "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lds_layout.hip"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return out.returncode, out.stdout.splitlines(), len(inst)


def test_no_live_regions_overlap_and_every_ring_slot_is_inside_the_launch(report):
    """Layers: x, h, tap image, ring slots, bias + tables, y; head: skip, zs / logits, y, ring slots, bias + tables -- pairwise
    disjoint in every Cfg, for several layer counts and dilation ranges and 0, 1 or 2 embedding tables in LDS; every planned slot
    16-byte aligned and inside the launch's LDS, ringSlotOffset injective over them, the planner's total within 160 KiB."""
    code, lines, n_inst = report
    fails = [l for l in lines if l.startswith("FAIL")]
    assert not fails, "\n".join(fails[:20])
    assert code == 0 and lines[-1] == "failures=0", lines[-3:]
    ok = [l for l in lines if l.startswith("ok ")]
    assert len(ok) >= 2 * n_inst                                   # (packed and features, one tile at least, per instantiation)
    # the headline configurations carry the overlay and its three in-place slots
    for bt in (1, 2, 3, 4):
        assert "ok Cfg<fp16,64,256,256,BT=%d,KFC=0> overlay=1 in_place_slots=3" % bt in ok, ok


def test_ring_placement_at_c3_by_tile_count(report):
    """placeLdsRing / planEmb restated from the Cfg constants for C3 (20 layers, maxDilation 512, fp16, dump-free, packed), in
    the words of kernelInfo (tests/test_ring_lds_overlay_gpu.py asserts the same dilations on the engine): three tiles keep d <= 2
    with the current tap's table and ask for three slots behind it; four tiles hold d <= 1 in place and ask for nothing."""
    _, lines, _ = report
    plan = [l for l in lines if l.startswith("plan ")]
    assert plan == ["plan BT=1,EMBLDS=2 lds=145728 ring_in_lds=d<=4 slots=14 tail_slots=11",
                    "plan BT=2,EMBLDS=1 lds=141952 ring_in_lds=d<=2 slots=6 tail_slots=3",
                    "plan BT=3,EMBLDS=1 lds=162752 ring_in_lds=d<=2 slots=6 tail_slots=3",
                    "plan BT=4,EMBLDS=0 lds=142592 ring_in_lds=d<=1 slots=2 tail_slots=0"], plan
