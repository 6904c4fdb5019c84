"""Shapes of the sampling-temperature tests (tests/test_temperature_gpu.py), shared with the generator of their
conditioning fixtures (tests/golden/make_golden_cond_temperature.py).  R 64 / S 256 / A 256, 8 layers, dilations 1 .. 16, 40
columns -- two full tiles and a ragged third -- and 48 samples: three wraps of the longest ring; one 16-column case each at A = 512
and A = 1024, whose softmax spreads an utterance's logits over other lane groups.  Importing this module makes the cases known to
cases.BY_NAME / condgen.COND_BY_NAME (the helpers of tests/test_features_gpu.py look them up there); the lists that parametrise the
existing tests are left alone."""
import cases
import condgen

CASE = cases.Case("T_R64S256A256_L8_B40", 77, [], cases.Shape(64, 256, 256, 8, 40, 48, 16), 1, 1, 20)
CASE_A512 = cases.Case("T_R64S128A512_L8_B16", 78, [], cases.Shape(64, 128, 512, 8, 16, 48, 16), 1, 1, 20)
CASE_A1024 = cases.Case("T_R128S256A1024_L8_B16", 79, [], cases.Shape(128, 256, 1024, 8, 16, 48, 16), 1, 1, 20)

COND = condgen.CondCase("cond_temp_B40", 601, CASE.name, 80, 8, 4)
COND_A512 = condgen.CondCase("cond_temp_A512_B16", 602, CASE_A512.name, 80, 8, 4)
COND_A1024 = condgen.CondCase("cond_temp_A1024_B16", 603, CASE_A1024.name, 80, 8, 4)

TEMP_CASES = (CASE, CASE_A512, CASE_A1024)
TEMP_CONDS = (COND, COND_A512, COND_A1024)

for _c in TEMP_CASES:
    cases.BY_NAME.setdefault(_c.name, _c)
for _c in TEMP_CONDS:
    condgen.COND_BY_NAME.setdefault(_c.name, _c)

POWERS = (0.25, 0.5, 1.0, 2.0, 4.0)      # column b samples at POWERS[b % 5]: every 16-lane row mixes all five


def power_temperatures(batch, shift=0):
    return [POWERS[(b + shift) % len(POWERS)] for b in range(batch)]
