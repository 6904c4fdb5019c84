"""The layer / dilation schedules at the edges of what the engine accepts, shared by tests/test_schedule_edges_cpu.py (oracle against
oracle: do these inputs make the schedule matter?) and tests/test_schedule_edges_gpu.py (the kernels against the oracle).

The schedule is d = 1, 2, 4, ... back to 1 past maxDilation (nv_wavenet.cuh:99,110-111), over L layers.  Everything else in the
suite runs L in {3, 6, 7, 8, 12, 20, 30} and a maxDilation that is a power of two which the schedule reaches; these do not:"""
import numpy as np

import cases
import util

L_MAX = 128                     # wn::kMaxLayers
SCHEDULES = [                   # (L, maxDilation); "Lmax": the most layers nvw_create_ex accepts at R32 (test_schedule_edges_gpu.lmax)
    (2, 1),                     # the fewest layers, every layer d = 1
    (2, 2),                     # the fewest layers: layers l+1, l+2 of the kernel's travelling schedule entries are the NEXT sample's
    (3, 1),
    (3, 4),                     # never reaches maxDilation, odd
    (20, 1),                    # twenty one-slot layers for the ring in LDS
    (4, 512),                   # largest dilation 8: what slot mode's window, rotation and blob go by, not maxDilation
    (5, 3),                     # no power of two: 1, 2, 1, 2, 1
    (7, 6),                     # 1, 2, 4, 1, 2, 4, 1
    (11, 1024),                 # a dilation above the largest one the ring in LDS takes (512)
    ("Lmax", 2),                # the schedule table and the bias table at their longest
]
SHAPES = {"R32": (32, 128, 256), "R64": (64, 256, 256)}
R64_SCHEDULES = [(2, 2), (20, 1), (5, 3), (4, 512)]      # also at the headline instantiation
RUNS = [("R32", L, D) for L, D in SCHEDULES] + [("R64", L, D) for L, D in R64_SCHEDULES]


def run_id(run):
    return "%s_L%s_maxD%d" % run


def dilations(L, maxD):
    out, d = [], 1
    for _ in range(L):
        out.append(d)
        d *= 2
        if d > maxD:
            d = 1
    return out


def case_of(shape, L, maxD, lmax=None):
    """The cases.Case of a run: batch 19 (a ragged second tile), 29 samples in chunks of 7; (11, 1024): batch 3, 1100 samples in
    chunks of 300 (the d = 1024 ring wraps, the tap is live for 76 samples); Lmax: batch 5, 24 samples."""
    R, S, A = SHAPES[shape]
    B, N, chunk = 19, 29, 7
    if maxD == 1024:
        B, N, chunk = 3, 1100, 300
    if L == "Lmax":
        assert lmax, "resolve Lmax on the GPU first"
        L, B, N = lmax, 5, 24
    seed = 7000 + 37 * L + maxD + R
    return cases.Case("edge_%s_L%d_maxD%d" % (shape, L, maxD), seed, [], cases.Shape(R, S, A, L, B, N, maxD), 1, 1, chunk)


def oracle_free_run(case, t, maxD=None, Lh=None, forced=None):
    """The oracle's own samples for `t` (maxD: another maxDilation over the same tensors) and its last-sample activations."""
    from oracle import oracle as O
    s = case.shape
    o = O.Oracle(s.L, s.B, s.N, s.R, s.S, s.A, s.maxD if maxD is None else maxD)
    o.set_model(t)
    o.set_tanh_embed(True)
    o.set_inputs(t.Lh if Lh is None else Lh, t.sel)
    y = o.run(s.N, forced=forced)
    act = o.getters()
    o.close()
    return y, act


# ---- features handed over directly (slot mode and the lockstep features path): n_cond channels, no upsampling ----
N_COND = 5


def feature_model(case, half):
    """x [B][N_COND][N] features, Wcond [2R L][N_COND], bcond [2R L] from the case's seed, scaled so that Lh = Wcond x + bcond is of
    order 0.5 like the O(1) recipe's conditioning; half: x and Wcond rounded through fp16 (what an fp16 engine stores; bcond joins
    the fp32 bias table)."""
    s = case.shape
    rng = np.random.default_rng(case.seed)
    x = rng.standard_normal((s.B, N_COND, s.N)).astype(np.float32)
    w = (rng.standard_normal((2 * s.R * s.L, N_COND)) * (0.5 / np.sqrt(N_COND))).astype(np.float32)
    b = (rng.standard_normal(2 * s.R * s.L) * 0.1).astype(np.float32)
    if half:
        x, w = x.astype(np.float16).astype(np.float32), w.astype(np.float16).astype(np.float32)
    return x, w, b


def feature_lh(case, x, w, b):
    """Lh [N][L][B][2R] = Wcond x + bcond in float64, for the oracle."""
    s = case.shape
    lh = np.einsum("oc,bct->bot", w.astype(np.float64), x.astype(np.float64)) + b.astype(np.float64)[None, :, None]
    return np.ascontiguousarray(lh.reshape(s.B, s.L, 2 * s.R, s.N).transpose(3, 1, 0, 2).astype(np.float32))
