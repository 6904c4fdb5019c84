"""Shared case definitions of the conditioning-contract tests (tests/test_cond_contracts_cpu.py, tests/test_cond_contracts_gpu.py):
the five ways an engine takes its conditioning -- packed by setInputs, the caller's fragment-order buffer, an fp32 or fp16 tensor
read in place, features plus cond_layers weights -- and the fused producer of fragment-order buffers, at every (R, S, A) the library
builds, in both precisions.

One shallow model per instantiation: 5 layers (an odd count: the layer loop's tail; maxDilation 4, so the dilations are 1, 2, 4, 1,
2), 14 samples in chunks of 5 (5 + 5 + 4: the second and third launch start mid-tensor; the d = 4 ring wraps three times) and
B = 21 columns (one full tile of 16 and a ragged one of 5).  Inputs: util.gen_o1, one seed per shape.  These are the smallest
shapes at which every index of a conditioning row still varies -- sample, layer, utterance within a tile, tile, gate half, wave --
and tests/test_cond_contracts_cpu.py shows that the bars of the GPU tests reject a row bound to the wrong one of each.

CAP = 37 is the capacity of the engines that run the 21 columns as a prefix of a larger batch: the in-place tensor is then
[N][L][37][2R] (the layout include/nv_wavenet_c.h documents for nvw_set_conditioning_direct: the batch axis is the engine's).

The fused producer's cases (PRODUCER_CASES) and their operands are made here as well, on the CPU, from a seed, together with the
float64 evaluation they are held to, its derived error bar and an fp32-accumulating model of the kernel."""
from collections import namedtuple

import numpy as np

import cases
import condgen
import util

L, MAXD, N, CHUNK, B, CAP = 5, 4, 14, 5, 21, 37
SHAPES = {                 # name: (R, S, A), seed
    "R32S128": ((32, 128, 256), 901),
    "S8R": ((32, 256, 256), 902),
    "R64S128": ((64, 128, 256), 903),
    "C3": ((64, 256, 256), 904),
    "A512": ((64, 128, 512), 905),
    "C4": ((128, 256, 256), 906),
    "A1024": ((128, 256, 1024), 907),
    "R256": ((256, 256, 256), 908),
}
NAMES = list(SHAPES)
N_COND, WINDOW, STRIDE = 80, 8, 2   # the feature conditioning: cond_layers + upsample of condgen.make_cond_model
CONTRACTS = ("packed", "frags", "raw32", "raw16", "feat")
RAW_OF = {"packed": 0, "frags": 0, "raw32": 1, "raw16": 2, "feat": 3}
MIN_DISTINCT_PICKS = 100


def contracts_of(precision):
    """raw16 -- an fp16 tensor read in place -- exists for fp16 engines only."""
    return [c for c in CONTRACTS if c != "raw16" or precision == 16]


def impl_of(name):
    """An Implementation value that accepts the shape (the organisation is forced: SINGLE_BLOCK refuses S > 4R as the reference's does)."""
    (R, S, _), _ = SHAPES[name]
    return 1 if S <= 4 * R else 3


def case_of(name, columns=B):
    (R, S, A), seed = SHAPES[name]
    return cases.Case("cond_" + name, seed, [], cases.Shape(R, S, A, L, columns, N, MAXD), impl_of(name), 1, CHUNK)


def oracle_macs(name):
    """Multiply-adds of one oracle run over the shape's 21 columns and 14 samples."""
    (R, S, A), _ = SHAPES[name]
    return B * N * (L * (5 * R * R + S * R) + A * S + A * A)


# per model, in G multiply-adds (gate 4 R^2 + residual R^2 + skip S R per layer, head A S + A^2, times 21 x 14):
#   R32S128 0.04   S8R 0.06   R64S128 0.07   C3 0.09   A512 0.14   C4 0.21   A1024 0.55   R256 0.62      the table: 1.78
# one teacher-forced run of every model together takes a few seconds (tests/test_cond_contracts_cpu.py holds the table to a minute)
ORACLE_BUDGET_SECONDS = 60.0

_inputs = {}


def inputs(name, half):
    """util.gen_o1 of the shape's 21 columns (memoised: treat as read-only); half: parameters rounded through fp16."""
    key = (name, bool(half))
    if key not in _inputs:
        _inputs[key] = util.gen_o1(case_of(name), half)
    return _inputs[key]


def with_inputs(t, Lh=None, sel=None):
    """A shallow copy of the inputs t with other conditioning / selectors (the model tensors are shared)."""
    import copy
    t2 = copy.copy(t)
    if Lh is not None:
        t2.Lh = np.ascontiguousarray(Lh, dtype=np.float32)
        t2.B = t2.Lh.shape[2]
    if sel is not None:
        t2.sel = np.ascontiguousarray(sel, dtype=np.float32)
    return t2


_features = {}


def features(name, half):
    """The feature conditioning of the shape's 21 columns: (m, x [21][n_cond][N] upsampled features, w [2R L][n_cond], Lh
    [N][L][21][2R] = Wcond x + bcond in float64 for the oracle).  half: x and Wcond rounded through fp16 (what an fp16 engine
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


def capacity_tensor(Lh, fill):
    """[N][L][CAP][2R]: the 21 columns of Lh as the prefix of an engine's CAP columns, the other columns holding `fill` (a number, or
    "other": other columns' negated rows, finite values that belong to no live column)."""
    n, l, b, c = Lh.shape
    out = np.empty((n, l, CAP, c), dtype=np.float32)
    out[:, :, :b] = Lh
    out[:, :, b:] = -Lh[:, :, :CAP - b] if isinstance(fill, str) else fill
    return out


# ---- what a mis-bound conditioning row would deliver ------------------------------------------------------------------------------
def _swap_utterances(Lh, R):
    m = Lh.copy()
    m[:, :, 3], m[:, :, 4] = Lh[:, :, 4], Lh[:, :, 3]
    return m


def _tile0_for_tile1(Lh, R):
    m = Lh.copy()
    m[:, :, 16:] = Lh[:, :, :Lh.shape[2] - 16]
    return m


def _next_row(Lh, rows_per_step):
    """Every (sample, layer) row replaced by the one `rows_per_step` further on; past the end: the zero padding sample."""
    n, l = Lh.shape[:2]
    flat = Lh.reshape((n * l,) + Lh.shape[2:])
    return np.concatenate([flat[rows_per_step:], np.zeros_like(flat[:rows_per_step])]).reshape(Lh.shape)


def _zero_wave(Lh, R):
    m = Lh.copy()
    m[..., 16:32] = 0          # wave 1's 16 rows of the tanh half (R = 32: the second of two waves)
    return m


def _batch_stride(Lh, R):
    cap = capacity_tensor(Lh, "other")
    return cap.reshape(-1)[:Lh.size].reshape(Lh.shape).copy()


MUTATIONS = {
    "two_utterances_swapped_within_a_tile": _swap_utterances,
    "tile_0_row_used_for_tile_1": _tile0_for_tile1,
    "layer_taken_from_the_next_layer": lambda Lh, R: _next_row(Lh, 1),
    "tanh_and_sigmoid_halves_swapped": lambda Lh, R: np.roll(Lh, R, axis=3),
    "sample_taken_from_the_next_sample": lambda Lh, R: _next_row(Lh, Lh.shape[1]),
    "one_wave_slice_zeroed": _zero_wave,
    "batch_stride_21_in_a_tensor_of_37": _batch_stride,
}


# ---- the bars -----------------------------------------------------------------------------------------------------------------------
def fp32_picks(ref, got, sel_bn, what=""):
    """fp32 engines: every pick is the oracle's given the same history (ref = util.teacher_forced_oracle(.., got["y"])), or the draw
    sits within 1e-5 of a CDF edge of the oracle's pick and the engine's pick is the neighbouring bin.  Returns the number of such
    picks."""
    _, unexplained = util.explain_mismatches(ref["y"], got["y"], ref["lo"], ref["hi"], sel_bn, 1e-5)
    assert not unexplained, "%s: unexplained sample mismatches (b,t,ref,got,edge distance): %s" % (what, unexplained[:5])
    misses = np.argwhere(ref["y"] != got["y"])
    for b, n in misses:
        near = min(abs(float(sel_bn[b, n]) - float(ref["lo"][b, n])), abs(float(sel_bn[b, n]) - float(ref["hi"][b, n])))
        assert near <= 1e-5 and abs(int(ref["y"][b, n]) - int(got["y"][b, n])) <= 1, \
            "%s: pick (%d,%d): engine %d, oracle %d, draw %.3g from the oracle's CDF edge" % (what, b, n, got["y"][b, n], ref["y"][b, n], near)
    return len(misses)


def fp32_bars(ref, got, sel_bn, what=""):
    """fp32_picks and the reference harness's activation bars on the last sample's dump."""
    n = fp32_picks(ref, got, sel_bn, what)
    util.compare_activations(ref, got, atol_eps=32)
    return n


def columns_of(rec, columns):
    """The first `columns` columns of a teacher-forced oracle record or of an engine's dump."""
    return {k: (v[:, :columns] if k in ("Xout", "skipOut") else v[:columns]) for k, v in rec.items()}


# ---- the fused producer (csrc/cond_producer.hip) ------------------------------------------------------------------------------------
Producer = namedtuple("Producer", "R n_cond samples tiles seed")
_P = Producer
# nwf = 2R/32 = 2, 4, 8, 16 at KF = 3 (tiles: condTiles() of a B = 21 engine, asserted by the GPU test); KF = 1 .. 4 at R = 64;
# fewer samples than the kernel's block of 8, exactly one block, a ragged last block; one tile and three (tiles * 2 tasks over the
# four waves of a workgroup: idle waves in the last workgroup)
PRODUCER_ENGINE_CASES = [_P(32, 80, N, 2, 951), _P(64, 80, N, 2, 952), _P(128, 80, N, 2, 953), _P(256, 80, N, 2, 954)]
PRODUCER_CASES = PRODUCER_ENGINE_CASES + [_P(64, c, N, 3, 960 + c) for c in (20, 33, 96, 128)] + \
    [_P(64, 80, n, tl, 970 + 10 * tl + n) for n in (5, 8, N) for tl in (1, 3)]
producer_id = lambda p: "R%d-ncond%d-N%d-tiles%d" % p[:4]


def producer_operands(p):
    """fp16 operands of the fused producer, as float32 arrays holding fp16-representable values: cond_w [2R L][n_cond], cond_b [2R L],
    x [tiles 16][samples][32 KF] (zeros beyond n_cond).  Conditioning of standard deviation ~0.5, as the O(1) recipe's."""
    rng = np.random.Generator(np.random.PCG64(p.seed))
    KF = (p.n_cond + 31) // 32
    h = lambda a: a.astype(np.float16).astype(np.float32)
    w = h((rng.random((2 * p.R * L, p.n_cond)) * 2 - 1) * 0.5 * np.sqrt(3.0 / p.n_cond))
    b = h((rng.random(2 * p.R * L) * 2 - 1) * 0.1 * np.sqrt(3.0))
    x = np.zeros((p.tiles * 16, p.samples, 32 * KF), dtype=np.float32)
    x[:, :, :p.n_cond] = h(rng.standard_normal((p.tiles * 16, p.samples, p.n_cond)))
    return w, b, x


def producer_position_operands(w, b, R):
    """What the kernel multiplies, derived from nv_wavenet.py:cond_fragment_order alone: (wpos [L][2R][n_cond] = fp16(w[perm] *
    scale), bpos [L][2R] = fp32(b[perm] * scale)), rows in fragment-position order, the gate's pre-scale folded in."""
    from nv_wavenet_amd.nv_wavenet import cond_fragment_order
    perm, scale = cond_fragment_order(R, 16)
    perm, sc = np.asarray(perm), np.asarray(scale, dtype=np.float32)
    wl = w.reshape(L, 2 * R, -1)[:, perm, :] * sc[None, :, None]
    bl = b.reshape(L, 2 * R)[:, perm] * sc[None, :]
    return wl.astype(np.float32).astype(np.float16).astype(np.float32), bl.astype(np.float32)


def producer_wfrag_rows(wfrag):
    """The position-order rows an operand tensor of nv_wavenet.py:cond_producer_weights holds: wfrag [L][NWF][2][KF][64][8] ->
    [L][NWF 32][32 KF] (lane = 16 ga + i holds k = 32 kf + 8 ga .. + 7 of row m = i of row tile tt; row m = 4 g + r of row tile tt
    of fragment wf is position (wf 4 + g) 8 + tt 4 + r)."""
    Lw, NWF, _, KF = wfrag.shape[:4]
    a = np.asarray(wfrag, dtype=np.float32).reshape(Lw, NWF, 2, KF, 4, 4, 4, 8)       # [l][wf][tt][kf][ga][g][r][e]
    return a.transpose(0, 1, 5, 2, 6, 3, 4, 7).reshape(Lw, NWF * 32, KF * 32)          # [l][wf][g][tt][r] x [kf][ga][e]


def producer_want(wpos, bpos, x):
    """float64 evaluation of the producer's sums and the derived bar.  Returns (want, bar), both [samples][L][tiles 16][2R] in
    position order.  The kernel accumulates Σ_k w_k x_k onto the bias in fp32 over 32 KF products and rounds the sum ONCE to fp16:
    every fp32 addition errs by at most 2^-24 of a partial sum, which Σ_k |w_k x_k| + |bias| bounds, 32 KF + 1 times; the final
    rounding by 2^-11 |want| (normal) or 2^-25 (subnormal)."""
    K = x.shape[2]
    w64 = np.zeros(wpos.shape[:2] + (K,))
    w64[:, :, :wpos.shape[2]] = wpos
    x64 = x.astype(np.float64)
    want = np.einsum("lpk,bnk->nlbp", w64, x64) + bpos.astype(np.float64)[None, :, None, :]
    mag = np.einsum("lpk,bnk->nlbp", np.abs(w64), np.abs(x64)) + np.abs(bpos.astype(np.float64))[None, :, None, :]
    bar = 2.0 ** -11 * np.abs(want) + (K + 1) * 2.0 ** -24 * mag + 2.0 ** -25
    return want, bar


def producer_fp32_model(wpos, bpos, x):
    """The kernel's arithmetic on the CPU: the bias, then the K = 32 KF products added one by one in fp32 in ascending k (the order
    of the MFMA's k index, fragment after fragment), the sum rounded once to fp16.  [samples][L][tiles 16][2R], position order."""
    K = x.shape[2]
    acc = np.broadcast_to(bpos[None, :, None, :], (x.shape[1], wpos.shape[0], x.shape[0], wpos.shape[1])).astype(np.float32)
    for k in range(min(K, wpos.shape[2])):
        acc = (acc + (wpos[None, :, None, :, k] * x.transpose(1, 0, 2)[:, None, :, None, k]).astype(np.float32)).astype(np.float32)
    return acc.astype(np.float16).astype(np.float32)


def fragments_of_positions(v, tiles):
    """[n][L][tiles 16][2R] in position order -> the packed buffer's [n][L][tiles][NWF][4 g][16 j][8] (position = (wf 4 + g) 8 + e)."""
    n, l, _, c2 = v.shape
    return np.ascontiguousarray(v.reshape(n, l, tiles, 16, c2 // 32, 4, 8).transpose(0, 1, 2, 4, 5, 3, 6))


def positions_of_fragments(f):
    """The inverse of fragments_of_positions."""
    n, l, tiles, nwf = f.shape[:4]
    return np.ascontiguousarray(f.transpose(0, 1, 2, 5, 3, 4, 6)).reshape(n, l, tiles * 16, nwf * 32)
