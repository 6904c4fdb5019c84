"""The bias denoiser without a GPU: its three entries are declared, bound and exported, and its kernels use no
scratch memory and spill no register."""
import os
import re
import subprocess

import pytest

from test_code_objects_cpu import BUILD, ROOT, kernel_table

NAMES = ("nvw_set_denoiser", "nvw_denoise_ready", "nvw_denoise")


def test_the_entries_are_declared_bound_and_exported():
    from nv_wavenet_amd._lib import SIGNATURES
    from nv_wavenet_amd.engine import DENOISE_REQ
    assert DENOISE_REQ.itemsize == 64
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    so = os.path.join(ROOT, "nv_wavenet_amd", "libwavenet_infer.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout if os.path.exists(so) else None
    for name in NAMES:
        assert re.search(r"\b%s\(nvw_engine\* e" % name, header), name
        assert name in SIGNATURES, name
        assert exported is None or re.search(r" T %s$" % name, exported, re.M), name


def test_the_kernels_use_no_scratch_and_spill_nothing():
    obj = os.path.join(BUILD, "denoise.o")
    if not os.path.exists(obj):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table(obj) if "denoise_kernel" in r[0]]
    assert len(rows) == 9, rows
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr + agpr <= 512, (name, vgpr, agpr, scratch, spill)
