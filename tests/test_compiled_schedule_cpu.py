"""Static properties of the kernels with the dilation schedule compiled in (wn::wavenet_wg_cs; no GPU): they are in the code objects
of the two fp16 shapes with a three-tile kernel that BASELINE runs (C2, C3), for both embedding placements and LD = 1, 2, they use no
scratch and stay inside the register files -- and the kernels with a run-time schedule kept their names."""
import os

import pytest

from test_code_objects_cpu import BUILD, kernel_table


@pytest.mark.parametrize("obj,shape", [("inst_64_256_256_p16.o", "64,256,256"), ("inst_64_128_256_p16.o", "64,128,256")])
def test_compiled_schedule_kernels_exist_and_use_no_scratch(obj, shape):
    if not os.path.exists(os.path.join(BUILD, obj)):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = {r[0].replace(" ", ""): r for r in kernel_table(obj)}
    for emb in ("true", "false"):
        for ld in (1, 2):
            name = "wn::wavenet_wg_cs<true,%s,3,%s,10,%d>" % (shape, emb, ld)
            assert name in rows, name
            _, vgpr, agpr, sgpr, scratch, spill = rows[name]
            assert scratch == 0 and spill == 0, rows[name]
            assert vgpr <= 512 and agpr <= 256 and sgpr <= 106, rows[name]
        assert "wn::wavenet_wg<true,%s,3,%s,false,0,true>" % (shape, emb) in rows, "the run-time-schedule kernel lost its name"
    assert not any(k.startswith("wn::wavenet_wg_cs<") and not k.startswith("wn::wavenet_wg_cs<true,%s,3," % shape) for k in rows), \
        "only the three-tile fp16 kernel has a compiled schedule"
