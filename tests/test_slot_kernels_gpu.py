"""The two kernels of slot mode in isolation (GPU, `-m gpu`), bit for bit against plain torch / numpy restatements:

  slot_feed_kernel   (wn::slots_feed<F16>)  window rows (T + i) mod W of the feature fragments -- the order of pack_features_kernel,
                     restated by nv_wavenet_amd.nv_wavenet.feature_fragments -- and of the selectors, philox_selector(seed, {k, uid})
                     for live samples and 0.5 otherwise, from per-column descriptors;
  slot_reset_kernel  (wn::slots_reset)      lanes 16g + (b & 15) of every fragment of every ring slot of each restarted column's tile
                     zeroed, the descriptors written, the history of the restarted columns set to 128.

Everything the kernels do not own keeps a canary pattern.  The kernels come from tests/cpp/wn_primitives.hip (libwn_primitives.so),
which compiles the product's slots.hip as it is and calls its launchers."""
import ctypes as C
import os

import numpy as np
import pytest

from nv_wavenet_amd.nv_wavenet import feature_fragments
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x5EED0000000071           # (high word not zero)

DESC = np.dtype([("x", "<u8"), ("cStride", "<i8"), ("tStride", "<i8"), ("start", "<i8"), ("length", "<i4"), ("uid", "<u4"),
                 ("precision", "<i4"), ("active", "<i4")])
UPD = np.dtype([("column", "<i4"), ("reset", "<i4"), ("pad0", "<i4"), ("pad1", "<i4"), ("d", DESC)])


@pytest.fixture(scope="module")
def prim():
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    path = os.path.join(HERE, "cpp", "libwn_primitives.so")
    assert os.path.exists(path), "build it with python -c 'import __graft_entry__ as g; g.build()'"
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.wnp_slot_feed.argtypes = [i, vp, vp, vp, i, i, i, i, C.c_longlong, i, i, i, C.c_ulonglong]
    lib.wnp_slot_reset.argtypes = [vp, vp, i, vp, i, vp, i, i, vp, vp]
    assert lib.wnp_slot_desc_bytes() == DESC.itemsize and lib.wnp_slot_update_bytes() == UPD.itemsize
    return lib


def _dev(a):
    """numpy array -> CUDA uint8 tensor with its bytes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _canary(n, dtype, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device="cuda", generator=g).view(dtype)


def _first_diff(got, want):
    import torch
    bad = torch.nonzero(got.reshape(-1) != want.reshape(-1))
    return None if bad.numel() == 0 else int(bad[0, 0])


# ---- feed ------------------------------------------------------------------------------------------------------------------------

KFC = {16: 3, 32: 5}             # feature fragments per tile (80 channels: 3 of 32 in fp16, 5 of 16 in fp32)
EPL = {16: 8, 32: 4}


def _sources(n_cond, n, rng):
    """Six device views of [n_cond][n] features, each (view, its values as fp32 on the device): contiguous, time-major (cStride 1)
    and sliced (cStride > n_cond, tStride 3), each fp32 and fp16."""
    import torch
    out = []
    for half in (False, True):
        dt = torch.float16 if half else torch.float32
        v = torch.from_numpy(rng.standard_normal((n_cond, n)).astype(np.float32)).to(dt).cuda()
        out.append(v)
        out.append(torch.from_numpy(rng.standard_normal((n, n_cond)).astype(np.float32)).to(dt).cuda().t())
        base = torch.from_numpy(rng.standard_normal((n_cond, 3 * n + 5)).astype(np.float32)).to(dt).cuda()
        out.append(base[:, 1::3][:, :n])
    assert out[1].stride() == (1, n_cond) and out[2].stride() == (3 * n + 5, 3) and out[2].stride(0) > n_cond
    return [(v, v.float()) for v in out]


def _feed_case(prim, precision, n_cond, srcs, col_src, start, length, uid, active, cols, maxBatch, tiles, counter, T, W, count):
    """Runs the feed on canaried buffers and returns (got feat, want feat, got sel, want sel); everything on the device."""
    import torch
    tilesUsed = (cols + 15) // 16
    desc = np.zeros(cols, dtype=DESC)
    for b in range(cols):
        v = srcs[col_src[b]][0]
        desc[b] = (v.data_ptr(), v.stride(0), v.stride(1), start[b], length[b], uid[b], 16 if v.dtype == torch.float16 else 32,
                   active[b])
    elems = W * tiles * KFC[precision] * 64 * EPL[precision]
    fdt = torch.float16 if precision == 16 else torch.float32
    feat = _canary(elems * (2 if precision == 16 else 4) // 4, fdt, 1)
    slack = 64                                                  # (a write of a column >= maxBatch of the last row would land here)
    sel = _canary(W * maxBatch + slack, torch.float32, 2)
    feat0, sel0 = feat.clone(), sel.clone()
    d = _dev(desc)
    assert prim.wnp_slot_feed(precision, feat.data_ptr(), sel.data_ptr(), d.data_ptr(), cols, maxBatch, tiles, n_cond, counter, T, W,
                              count, SEED) == 0
    # features: column b, step sample i reads local sample k = counter + i - start[b] where 0 <= k < length[b] and the column is active
    lmax = max(s[1].shape[1] for s in srcs)
    vals = torch.zeros(len(srcs), n_cond, lmax, device="cuda")
    for i, (_, f) in enumerate(srcs):
        vals[i, :, :f.shape[1]] = f
    k = counter + np.arange(count)[None, :] - np.asarray(start, dtype=np.int64)[:, None]          # [cols][count]
    live = (k >= 0) & (k < np.asarray(length)[:, None]) & (np.asarray(active)[:, None] != 0)
    kc = torch.from_numpy(np.where(live, k, 0)).cuda()
    g = vals[torch.as_tensor(np.asarray(col_src), device="cuda")[:, None], :, kc]                 # [cols][count][n_cond]
    g = torch.where(torch.from_numpy(live).cuda()[:, :, None], g, torch.zeros((), device="cuda"))     # (+0, as the kernel writes)
    x = torch.zeros(tilesUsed * 16, n_cond, count, device="cuda")
    x[:cols] = g.permute(0, 2, 1)
    frag = feature_fragments(x, tilesUsed, precision)                                             # [count][tilesUsed][KFC][4][16][EPL]
    rows = torch.from_numpy((T + np.arange(count)) % W).cuda()
    want_feat = feat0.view(W, tiles, KFC[precision], 4, 16, EPL[precision]).clone()
    want_feat[rows, :tilesUsed] = frag
    # selectors: columns below min(16 x tilesUsed, maxBatch) of the step's rows
    ncol = min(tilesUsed * 16, maxBatch)
    kk = np.zeros((count, ncol), dtype=np.int64)
    uu = np.zeros((count, ncol), dtype=np.int64)
    lv = np.zeros((count, ncol), dtype=bool)
    kk[:, :cols], lv[:, :cols] = np.where(live, k, 0).T, live.T
    uu[:, :cols] = np.asarray(uid, dtype=np.int64)[None, :]
    s = np.where(lv, O.philox_selectors_at(SEED, kk, uu), np.float32(0.5)).astype(np.float32)
    want_sel = sel0.clone()
    want_sel[:W * maxBatch].view(W, maxBatch)[rows, :ncol] = torch.from_numpy(s).cuda()
    return feat.view(want_feat.shape), want_feat, sel, want_sel


def _assert_feed(got_f, want_f, got_s, want_s, what):
    import torch
    i = _first_diff(got_f.view(torch.int16), want_f.view(torch.int16))
    assert i is None, "%s: feature fragments differ first at element %d of [W][tiles][KFC][4][16][EPL] %s" % (what, i, tuple(want_f.shape))
    i = _first_diff(got_s.view(torch.int32), want_s.view(torch.int32))
    assert i is None, "%s: selectors differ first at element %d (row-major [W][maxBatch] + slack)" % (what, i)


@pytest.mark.parametrize("count", [1, 7, 9, 64])
@pytest.mark.parametrize("n_cond", [1, 37, 80])
@pytest.mark.parametrize("precision", [16, 32])
def test_feed_writes_the_window_rows_of_every_column(prim, precision, n_cond, count):
    """37 columns (three tiles, the last one ragged; maxBatch 37 and one tile more in the buffer), fp32 and fp16 sources in three
    layouts, utterances that start inside the step, end inside it, ended long before it, and idle columns; a window of 64 whose
    rows wrap; uids 0, 2**31, 2**32 - 1; a sample counter beyond 2**32."""
    rng = np.random.default_rng(1000 * precision + 10 * n_cond + count)
    W, cols = 64, 37
    T = W - 1 if count == 1 else W - 4
    n = 2 * W + 40
    srcs = _sources(n_cond, n, rng)
    counter = 5_000_000_123
    col_src, start, length, uid, active = [], [], [], [], []
    for b in range(cols):
        ln = int(rng.integers(1, n + 1))
        kind = b % 5
        if kind == 0:
            k0 = int(rng.integers(-count - 2, 1))               # starts inside the step (or just after it)
        elif kind == 1:
            k0 = max(0, ln - int(rng.integers(0, count + 2)))   # ends inside the step
        elif kind == 2:
            k0 = ln + 1000                                      # ended long ago: k >= length throughout
        else:
            k0 = int(rng.integers(0, ln))
        col_src.append(b % len(srcs))
        start.append(counter - k0)
        length.append(ln)
        uid.append([0, 2 ** 31, 2 ** 32 - 1][b % 3] if b < 6 else int(rng.integers(0, 2 ** 32)))
        active.append(0 if b % 7 == 6 else 1)
    got_f, want_f, got_s, want_s = _feed_case(prim, precision, n_cond, srcs, col_src, start, length, uid, active, cols, cols, 4,
                                              counter, T, W, count)
    _assert_feed(got_f, want_f, got_s, want_s, "fp%d n_cond %d count %d" % (precision, n_cond, count))


def test_feed_second_grid_stride_pass_at_769_tiles(prim):
    """769 tiles and a chunk of W = 1024 samples: 769 x 128 = 98 432 tasks on a grid capped at 65 536 workgroups, so the rows of
    samples >= 8 x ceil(65 536 / 769) = 688 come from the kernel's second pass.  Every row and column is checked."""
    rng = np.random.default_rng(769)
    W, count, n_cond, tiles = 1024, 1024, 37, 769
    cols = tiles * 16
    assert tiles * -(-count // 8) > 65536
    srcs = _sources(n_cond, 2 * W, rng)
    counter = 77_777
    start = [counter - int(rng.integers(-900, 2 * W)) for _ in range(cols)]
    length = [int(rng.integers(1, 2 * W + 1)) for _ in range(cols)]
    uid = [int(u) for u in rng.integers(0, 2 ** 32, size=cols)]
    uid[:3] = [0, 2 ** 31, 2 ** 32 - 1]
    active = [0 if b % 11 == 10 else 1 for b in range(cols)]
    col_src = [b % len(srcs) for b in range(cols)]
    got_f, want_f, got_s, want_s = _feed_case(prim, 16, n_cond, srcs, col_src, start, length, uid, active, cols, cols, tiles, counter,
                                              300, W, count)
    second = 8 * -(-65536 // tiles)
    rows = (300 + np.arange(second, count)) % W
    import torch
    r = torch.from_numpy(rows).cuda()
    assert _first_diff(got_f[r].view(torch.int16), want_f[r].view(torch.int16)) is None, "rows of the second pass differ"
    _assert_feed(got_f, want_f, got_s, want_s, "769 tiles")


# ---- reset -----------------------------------------------------------------------------------------------------------------------

def _ring_slots(L, maxD):
    d, n = 1, 0
    for _ in range(L):
        n += d
        d = 1 if 2 * d > maxD else 2 * d
    return n


def _reset_case(prim, R, precision, cols_list, upd_cols, resets, tiles, maxBatch, seed):
    import torch
    esz = 2 if precision == 16 else 4
    frags = R * 16 * esz // 1024                       # fragsPerSlot, as the engine computes it
    slots = _ring_slots(20, 512)
    ring = _canary(tiles * slots * frags * 256, torch.int32, seed)
    hist = [_canary(maxBatch, torch.int32, seed + 1), _canary(maxBatch, torch.int32, seed + 2)]
    for h in hist:
        h[h == 128] = 129
    rng = np.random.default_rng(seed)
    desc0 = np.frombuffer(rng.integers(0, 256, size=maxBatch * DESC.itemsize, dtype=np.uint8).tobytes(), dtype=DESC)
    upd = np.zeros(len(upd_cols), dtype=UPD)
    upd["column"] = upd_cols
    upd["reset"] = resets
    upd["d"] = np.frombuffer(rng.integers(0, 256, size=len(upd_cols) * DESC.itemsize, dtype=np.uint8).tobytes(), dtype=DESC)
    want_ring = ring.clone().view(tiles, slots * frags, 4, 16, 4)
    want_hist = [h.clone() for h in hist]
    desc = _dev(desc0)
    cl = torch.tensor(np.asarray(cols_list, dtype=np.int32), device="cuda")
    u = _dev(upd)
    assert prim.wnp_slot_reset(desc.data_ptr(), u.data_ptr(), len(upd), cl.data_ptr(), len(cols_list), ring.data_ptr(), slots, frags,
                               hist[0].data_ptr(), hist[1].data_ptr()) == 0
    c = torch.tensor(np.asarray(cols_list, dtype=np.int64), device="cuda")
    want_ring[c // 16, :, :, c % 16, :] = 0            # lanes 16g + (b & 15), every fragment of every slot of the column's tile
    i = _first_diff(ring, want_ring)
    if i is not None:
        lane = (i // 4) % 64
        raise AssertionError("R%d fp%d: ring differs first at 16-byte piece of lane %d (tile %d, fragment %d of the tile)" % (
            R, precision, lane, i // (slots * frags * 256), (i // 256) % (slots * frags)))
    want_desc = desc0.copy()
    want_desc[np.asarray(upd_cols)] = upd["d"]
    assert np.array_equal(desc.cpu().numpy().view(DESC).view(np.uint8), want_desc.view(np.uint8)), "descriptors"
    rs = torch.tensor([b for b, r in zip(upd_cols, resets) if r], dtype=torch.int64, device="cuda")
    for h, w in zip(hist, want_hist):
        w[rs] = 128
        assert _first_diff(h, w) is None, "history"


@pytest.mark.parametrize("precision", [16, 32])
@pytest.mark.parametrize("R", [32, 64, 128, 256])
def test_reset_zeroes_exactly_the_lanes_of_the_restarted_columns(prim, R, precision):
    """A ring of 70 tiles with the slot count of a maxD-512 schedule (L = 20: 2 046 slots of R x 16 elements).  First several
    columns of one tile and columns of distant tiles, with 20 000 updates (more than the 64 x 256 threads of the launch's row 0):
    every descriptor written, the history at 128 where reset = 1 only.  Then 1 030 restarted columns of 1 120 (more than the
    launch's 1 024 rows of workgroups)."""
    tiles, maxBatch = 70, 20000
    rng = np.random.default_rng(R * 100 + precision)
    few = [0, 3, 15, 16 * 37 + 9, 16 * 69 + 15]
    upd_cols = [int(b) for b in rng.permutation(maxBatch)]
    resets = [1 if (b in few or b % 997 == 5) else 0 for b in upd_cols]
    _reset_case(prim, R, precision, few, upd_cols, resets, tiles, maxBatch, 10 * R + precision)
    many = sorted(int(b) for b in rng.choice(tiles * 16, size=1030, replace=False))
    upd_cols = many + [b for b in range(tiles * 16, tiles * 16 + 5)]
    _reset_case(prim, R, precision, many, upd_cols, [1] * len(many) + [0] * 5, tiles, tiles * 16 + 5, 10 * R + precision + 5)
