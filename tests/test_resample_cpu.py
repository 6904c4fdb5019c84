"""CPU tests of sample-rate conversion (no GPU): the three entries and the record are declared, bound and exported,
the default design gives coprime factors and odd symmetric taps, and the kernels of the built object use no scratch memory and spill
nothing.  (An engine cannot be created without a GPU: the refusals are in test_resample_gpu.py.)"""
import math
import os
import re

import numpy as np
import pytest

from test_code_objects_cpu import BUILD, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_resample_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert "int nvw_set_resampler(nvw_engine* e, int slot, int up, int down, const double* taps, int n_taps);" in header
    assert "long long nvw_resample_count(nvw_engine* e, int slot, long long n);" in header
    assert "int nvw_resample(nvw_engine* e, int slot, const nvw_resample_req* reqs, int count, void* stream);" in header
    m = re.search(r"typedef struct \{([^}]*)\} nvw_resample_req;", header)
    assert m and [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "const void* in", "int in_type", "long long first", "int n_in", "int last", "void* out", "int out_type", "long long m0", "int count"]
    assert "#define NVW_ABI_VERSION 7" in header
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import RESAMPLE_REQ, WavenetEngine
    for name in ("nvw_set_resampler", "nvw_resample_count", "nvw_resample"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert RESAMPLE_REQ.itemsize == 64 and [RESAMPLE_REQ.fields[k][1] for k in RESAMPLE_REQ.names] == [0, 8, 16, 24, 28, 32, 40, 48, 56]
    for name in ("setResampler", "resampleCount", "resample"):
        assert callable(getattr(WavenetEngine, name)), name
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    assert callable(NVWaveNetEngine.resample) and callable(NVWaveNetEngine.resample_stream)


@pytest.mark.parametrize("rate_in, rate_out, L, M", [(48000, 24000, 1, 2), (22050, 8000, 160, 441), (24000, 16000, 2, 3),
                                                    (22050, 24000, 160, 147)])
def test_the_default_design_is_coprime_odd_and_symmetric(rate_in, rate_out, L, M):
    from nv_wavenet_amd.nv_wavenet import resample_taps
    up, down, h = resample_taps(rate_in, rate_out)
    assert (up, down) == (L, M) and math.gcd(up, down) == 1
    assert h.dtype == np.float64 and len(h) == 2 * 16 * max(L, M) + 1 and np.array_equal(h, h[::-1])
    assert abs(h.sum() - L) < 1e-3 * L                     # the gain of L is folded in


def test_the_resample_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(BUILD, "resample.o")):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table("resample.o") if "resample_kernel" in r[0]]
    assert len(rows) == 8, [r[0] for r in rows]            # G = 4 with one to three row tiles, G = 1 with one to five a wave
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr + agpr <= 512 and sgpr <= 106, (name, vgpr, agpr, sgpr, scratch, spill)
