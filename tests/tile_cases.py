"""Shared case definitions of the multi-tile tests (tests/test_tiles_cpu.py, tests/test_tiles_gpu.py): wavenet_wg with two, three
and four tiles of 16 utterances per workgroup, every tile holding utterances of its own.

The five (R, S, A) whose instantiations build multi-tile kernels, 8 layers with dilations 1, 2, 4, 8 twice, 24 samples (the d = 8
rings wrap three times) in chunks of 7.  Inputs: util.gen_o1 for COLUMNS = 85 columns, one seed per shape; every column is its own
utterance and an engine of batch B takes the first B columns.  Batches are 16 (BT + 1) + 5: workgroup 0 has every tile full,
workgroup 1 a full tile, a ragged tile of 5 and -- four tiles per workgroup -- padding tiles."""
import numpy as np

import cases
import condgen
import util

L, MAXD, N, CHUNK, COLUMNS = 8, 8, 24, 7, 85
SHAPES = {                 # name: (R, S, A), seed
    "R32S128": ((32, 128, 256), 701),
    "S8R": ((32, 256, 256), 702),
    "R64S128": ((64, 128, 256), 703),
    "C3": ((64, 256, 256), 704),
    "A512": ((64, 128, 512), 705),
}
NAMES = list(SHAPES)
BT_OF = {"wg": 1, "wg2": 2, "wg3": 3, "wg4": 4}
SEED = 0x5EED000000007117          # in-kernel selectors (Philox key)
N_COND, WINDOW, STRIDE = 80, 8, 4   # the feature conditioning: cond_layers + upsample of condgen.make_cond_model


def batch_of(bt):
    return 16 * (bt + 1) + 5


def launched_bt(name, mode, dump=False, raw=0):
    """Tiles per workgroup the engine launches for a request: four tiles exist dump-free and for packed conditioning only, and at
    A = 512 they do not fit the LDS (184 064 B of 160 KiB at 8 layers): three run instead."""
    bt = BT_OF[mode]
    if bt == 4 and (dump or raw != 0 or name == "A512"):
        return 3
    return bt


def case_of(name, B=COLUMNS, samples=N):
    (R, S, A), seed = SHAPES[name]
    return cases.Case("tiles_" + name, seed, [], cases.Shape(R, S, A, L, B, samples, MAXD), 1, 1, CHUNK)


_inputs = {}


def inputs(name, half):
    """util.gen_o1 of the shape's 85 columns (memoised: treat as read-only); half: parameters rounded through fp16."""
    key = (name, bool(half))
    if key not in _inputs:
        _inputs[key] = util.gen_o1(case_of(name), half)
    return _inputs[key]


def first_columns(t, B):
    """(Lh [N][L][B][2R], sel [N][B]) of the first B columns."""
    return np.ascontiguousarray(t.Lh[:, :, :B, :]), np.ascontiguousarray(t.sel[:, :B])


def with_inputs(t, Lh=None, sel=None):
    """A shallow copy of the inputs t with other conditioning / selectors (the model tensors are shared)."""
    import copy
    t2 = copy.copy(t)
    if Lh is not None:
        t2.Lh = np.ascontiguousarray(Lh, dtype=np.float32)
    if sel is not None:
        t2.sel = np.ascontiguousarray(sel, dtype=np.float32)
    return t2


def philox_sel(B=COLUMNS, samples=N):
    return util.O.philox_selectors(SEED, samples, B)


_features = {}


def features(name, half):
    """The feature conditioning of the shape's 85 columns: (m, x [85][n_cond][N] upsampled features, w [2R L][n_cond], Lh
    [N][L][85][2R] = Wcond x + bcond in float64 for the oracle).  half: x and Wcond rounded through fp16 (what an fp16 engine
    stores; bcond joins the fp32 bias table)."""
    key = (name, bool(half))
    if key in _features:
        return _features[key]
    import torch
    import torch.nn.functional as F
    case = case_of(name)
    s = case.shape
    cc = condgen.CondCase(case.name, case.seed, case.name, N_COND, WINDOW, STRIDE)
    m = condgen.make_cond_model(cc, s)
    x = F.conv_transpose1d(torch.from_numpy(m["features"]), torch.from_numpy(m["up_w"]), torch.from_numpy(m["up_b"]), stride=STRIDE)
    x = x[:, :, :-(WINDOW - STRIDE)].contiguous().numpy()
    w = m["cond_w"][:, :, 0]
    if half:
        x, w = x.astype(np.float16).astype(np.float32), w.astype(np.float16).astype(np.float32)
    lh = np.einsum("oc,bct->bot", w.astype(np.float64), x.astype(np.float64)) + m["cond_b"].astype(np.float64)[None, :, None]
    Lh = np.ascontiguousarray(lh.reshape(s.B, s.L, 2 * s.R, s.N).transpose(3, 1, 0, 2).astype(np.float32))
    _features[key] = (m, x, np.ascontiguousarray(w), Lh)
    return _features[key]


def columns_of(ref, B):
    """The first B columns of a teacher-forced oracle record (util.teacher_forced_oracle) or of an engine's dump."""
    out = {}
    for k, v in ref.items():
        out[k] = v[:, :B] if k in ("Xout", "skipOut") else v[:B]
    return out
