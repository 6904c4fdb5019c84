"""CPU tests of the analysis front end (no GPU): the three entries are declared, bound and exported, and the kernels
of the built object use no scratch memory and spill nothing.  (An engine cannot be created without a GPU: the refusals of
nvw_set_analysis are in test_analysis_gpu.py.)"""
import os
import re

import pytest

from test_code_objects_cpu import BUILD, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_analysis_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "nv_wavenet_c.h")).read()
    assert "int nvw_set_analysis(nvw_engine* e, int n_fft, int hop, int n_mel, const float* mel_basis);" in header
    assert "int nvw_analysis_frames(nvw_engine* e, int n);" in header
    assert "int nvw_analyse(nvw_engine* e, const nvw_analysis_req* reqs, int count, void* stream);" in header
    m = re.search(r"typedef struct \{([^}]*)\} nvw_analysis_req;", header)
    assert m and [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "const short* pcm", "int n", "void* mel", "int precision", "long long c_stride, f_stride", "int* y"]
    assert "#define NVW_ABI_VERSION 7" in header
    from nv_wavenet_amd import _lib
    from nv_wavenet_amd.engine import ANALYSIS_REQ, WavenetEngine
    for name in ("nvw_set_analysis", "nvw_analysis_frames", "nvw_analyse"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert ANALYSIS_REQ.itemsize == 56 and [ANALYSIS_REQ.fields[k][1] for k in ANALYSIS_REQ.names] == [0, 8, 16, 24, 32, 40, 48]
    for name in ("setAnalysis", "analysisFrames", "analyse"):
        assert callable(getattr(WavenetEngine, name)), name
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    assert callable(NVWaveNetEngine.set_analysis) and callable(NVWaveNetEngine.analyse) and callable(NVWaveNetEngine.score_audio)


def test_the_analysis_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(BUILD, "analysis.o")):
        pytest.skip("build the library first (__graft_entry__.build())")
    rows = [r for r in kernel_table("analysis.o") if "analysis_kernel" in r[0]]
    assert len(rows) == 5, [r[0] for r in rows]          # one to five bin tiles a wave
    for name, vgpr, agpr, sgpr, scratch, spill in rows:
        assert scratch == 0 and spill == 0 and vgpr + agpr <= 512 and sgpr <= 106, (name, vgpr, agpr, sgpr, scratch, spill)
