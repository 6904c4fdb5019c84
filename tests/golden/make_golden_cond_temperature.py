#!/usr/bin/env python3
"""Generate tests/golden/cond_temp_*.npz: make_golden_cond.py for the shapes of tests/temperature_cases.py (the reference's own
WaveNet.get_cond_input evaluated on the seeded tensors of condgen.make_cond_model; runs only where the reference is installed).

    python tests/golden/make_golden_cond_temperature.py
"""
import os

import numpy as np
import torch

import make_golden_cond as G      # (puts tests/ and the reference's pytorch/ on sys.path)

import cases  # noqa: E402
import condgen  # noqa: E402
import temperature_cases as TC  # noqa: E402


def main():
    torch.set_num_threads(1)
    for cc in TC.TEMP_CONDS:
        shape = cases.BY_NAME[cc.case_name].shape
        m = condgen.make_cond_model(cc, shape)
        ci = G.reference_cond_input(cc, shape, m)
        assert ci.shape == (2 * shape.R, shape.B, shape.L, shape.N), ci.shape
        path = os.path.join(G.HERE, cc.name + ".npz")
        np.savez(path, **condgen.record_of(ci))
        print("%-22s cond_input %s std %.3f  (fixture %d bytes)" % (cc.name, ci.shape, ci.std(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
