"""Shared case definitions of the multi-tile chain tests (tests/test_chain_tiles_cpu.py, tests/test_chain_tiles_gpu.py): wavenet_chain
with two to eight tiles of 16 utterances per chain, every tile holding utterances of its own.

A chain's stages walk its tiles `tile = tile0 + q * chains + chainIdx`, q = 0 .. tiles per chain - 1: the tiles a stage could confuse
are `chains` apart, and a full-chip launch has hundreds of them.  An oracle run of that many utterances is out of reach, so every
shape has K distinct columns (util.gen_o1, one seed per shape; K is no multiple of 16) and a launch of B columns takes column idx[b]
of them, idx = default_rng(seed).integers(0, K, B) (gather_map).  The map is only returned when every two tiles of the launch differ
in at least half of the lanes that are live in both -- 8 of 16 for full tiles; a pair of full tiles misses that with probability
C(16, 9) K^-9 = 1.4e-8 at K = 21 -- so no tile can stand in for another one, at whatever CU count the batches were derived from.

The launch plan is mirrored here from the shape alone (plan / expected_info): stages, layers per stage, chains, tiles per chain and
whether the launch runs the HOIST instantiation, as nv_wavenet.hpp's chainLpcMax / chainStagesFor / chainTpc / kChainHoistBuilt
compute them from CCfg::LPC.  Every shape is deep, so that a chain has many stages and the GPU few chains."""
from collections import namedtuple

import numpy as np

import cases
import tile_cases as TC
import util

Model = namedtuple("Model", "rsa L maxD K N chunk seed map_seed")
MODELS = {
    "C4": Model((128, 256, 256), 30, 4, 35, 12, 5, 801, 9101),
    "C3": Model((64, 256, 256), 20, 8, 53, 24, 7, 802, 9102),
    "R32": Model((32, 128, 256), 24, 8, 85, 24, 7, 803, 9103),
    "A512": Model((64, 128, 512), 16, 8, 53, 24, 7, 804, 9104),
    "A1024": Model((128, 256, 1024), 12, 4, 21, 12, 5, 805, 9105),
}
NAMES = list(MODELS)
SEED = 0x5EED00000000C4A1          # in-kernel selectors (Philox key)
CU_COUNTS = (32, 64, 120, 256, 304)

# CCfg<F16, R, S, A>::LPC, the most layers whose weights one CU keeps resident (wn_chain.hpp: pickLpc), obtained by instantiating CCfg
# on the host; 0: no chain for the shape
LPC = {
    16: {(32, 128, 256): 8, (32, 256, 256): 8, (64, 128, 256): 8, (64, 256, 256): 5, (64, 128, 512): 8, (128, 256, 256): 2,
         (128, 256, 1024): 2, (256, 256, 256): 0},
    32: {(32, 128, 256): 7, (32, 256, 256): 5, (64, 128, 256): 4, (64, 256, 256): 3, (64, 128, 512): 4, (128, 256, 256): 1,
         (128, 256, 1024): 1, (256, 256, 256): 0},
}
TPC_MAX = 8
HOIST_FROM = 4          # launches with MORE tiles per chain than this hoist (wn_experiments.hpp: WN_CHAIN_HOIST_FROM)

# (name, precision, organisation, tiles per chain)
_TABLE = [
    ("C4", 16, "chain", (2, 4, 5, 8)),          # 2 layers/stage -> 16 stages (16 chains at 256 CUs); HOIST=1 beyond four tiles
    ("C4", 32, "chain", (2, 3)),                # 1 layer/stage -> 31 stages (8)
    ("C3", 16, "chain", (2,)),                  # 5 layers/stage -> 5 stages (51)
    ("C3", 16, "chain1", (3, 8)),               # 21 stages (12)
    ("C3", 32, "chain1", (3, 8)),
    ("R32", 16, "chain1", (2, 3, 7, 8)),        # 25 stages (10: the grid rounds the chains up to 8s, idle workgroups)
    ("R32", 32, "chain1", (2, 3, 7, 8)),
    ("A512", 16, "chain1", (2, 5)),             # 17 stages (15)
    ("A1024", 16, "chain", (2,)),               # 2 layers/stage -> 7 stages (36): head weights streamed, embedding tables not both in LDS
]
CASES = [(n, p, o, tpc) for n, p, o, tpcs in _TABLE for tpc in tpcs]
ORGS = sorted({(n, p, o) for n, p, o, _ in _TABLE})
case_id = lambda c: "%s-fp%d-%s-tpc%d" % c if len(c) == 4 else "%s-fp%d-%s" % c


def case_of(name, B=None, samples=None):
    m = MODELS[name]
    R, S, A = m.rsa
    return cases.Case("chain_" + name, m.seed, [], cases.Shape(R, S, A, m.L, m.K if B is None else B, m.N if samples is None else samples,
                                                               m.maxD), 1, 1, m.chunk)


def oracle_macs(name):
    """Multiply-adds of one oracle run over the shape's K columns."""
    m = MODELS[name]
    R, S, A = m.rsa
    return m.K * m.N * (m.L * (5 * R * R + S * R) + A * S + A * A)


_inputs = {}


def inputs(name, half):
    """util.gen_o1 of the shape's K columns (memoised: treat as read-only); half: parameters rounded through fp16."""
    key = (name, bool(half))
    if key not in _inputs:
        _inputs[key] = util.gen_o1(case_of(name), half)
    return _inputs[key]


def gathered(t, idx):
    """The inputs t with columns idx of its conditioning and selectors (host copy: for the oracle, small batches only)."""
    return TC.with_inputs(t, Lh=t.Lh[:, :, idx, :], sel=t.sel[:, idx])


def gather_columns(ref, idx):
    """Columns idx of a teacher-forced oracle record (util.teacher_forced_oracle) or of an engine's dump."""
    return {k: (v[:, idx] if k in ("Xout", "skipOut") else v[idx]) for k, v in ref.items()}


# ---- the gather map ------------------------------------------------------------------------------------------------------------
def tile_distances(idx):
    """(differ, live) [tiles][tiles]: lanes in which two tiles of the batch idx hold different columns, of the lanes live in both."""
    idx = np.asarray(idx)
    tiles = (idx.size + 15) // 16
    T = np.full(tiles * 16, -1, dtype=np.int64)
    T[:idx.size] = idx
    T = T.reshape(tiles, 16)
    both = (T >= 0)[:, None, :] & (T >= 0)[None, :, :]
    return ((T[:, None, :] != T[None, :, :]) & both).sum(axis=2), both.sum(axis=2)


def check_map(idx):
    """Every two different tiles differ in at least half of the lanes live in both (full tiles: 8 of 16)."""
    differ, live = tile_distances(idx)
    ok = 2 * differ >= live
    np.fill_diagonal(ok, True)
    bad = np.argwhere(~ok)
    assert bad.size == 0, "tiles %d and %d agree in %d of %d live lanes" % (bad[0, 0], bad[0, 1], (live - differ)[tuple(bad[0])],
                                                                           live[tuple(bad[0])])
    return idx


def gather_map(K, B, seed):
    """idx [B]: the column of the K distinct ones that column b of a launch takes; asserts check_map."""
    assert K % 16 != 0 and K >= 21
    return check_map(np.random.default_rng(seed).integers(0, K, B))


def map_of(name, B):
    m = MODELS[name]
    return gather_map(m.K, B, m.map_seed)


# ---- the plan, mirrored ---------------------------------------------------------------------------------------------------------
def chain_stages_for(L, lpc):
    return (L + lpc - 1) // lpc + 1


def chain_lpc_max(L, lpc_cfg):
    """Layers per stage of organisation "chain": the fewest stages that keep every layer resident, balanced."""
    if lpc_cfg == 0:
        return 0
    ns = (L + lpc_cfg - 1) // lpc_cfg
    return (L + ns - 1) // ns


def chain_tpc(tiles, ncu, stages):
    per_launch = ncu // stages
    tpc = (tiles + per_launch - 1) // per_launch if per_launch > 0 else 1
    return min(max(tpc, 1), TPC_MAX)


def hoist_built(name, precision):
    lpc_cfg = LPC[precision][MODELS[name].rsa]
    return precision == 16 and 0 < lpc_cfg <= 2 and MODELS[name].rsa[2] <= 512


Plan = namedtuple("Plan", "name precision org ncu stages lpc chains tpc max_batch batch")


def plan(name, precision, org, ncu, tpc):
    """The launch plan of an engine of `org` ("chain" / "chain1") on ncu CUs with `tpc` tiles per chain: max_batch = the capacity of
    that layout, batch = the running batch of a case, 16 (chains tpc - chains // 2) - 5: the upper half of the chains serves one tile
    fewer and the last tile is ragged."""
    m = MODELS[name]
    lpc = 1 if org == "chain1" else chain_lpc_max(m.L, LPC[precision][m.rsa])
    assert lpc > 0 and 1 <= tpc <= TPC_MAX
    stages = chain_stages_for(m.L, lpc)
    chains = ncu // stages
    assert chains >= 1, "%d CUs hold no chain of %d stages" % (ncu, stages)
    batch = 16 * (chains * tpc - chains // 2) - 5
    assert chain_tpc((batch + 15) // 16, ncu, stages) == tpc
    return Plan(name, precision, org, ncu, stages, lpc, chains, tpc, 16 * chains * tpc, batch)


def expected_info(pl, capacity, batch, dump):
    """What kernelInfo(batch, dump) of an engine of capacity `capacity` must say: (the fields, HOIST=1 present)."""
    tpc = chain_tpc((capacity + 15) // 16, pl.ncu, pl.stages)
    chains = min((batch + 15) // 16, pl.chains)
    fields = "DUMP=%d%s> stages=%d layers/stage=%d chains=%d tiles/chain=%d wgs=%d " % (
        1 if dump else 0, ",HOIST=1" if hoists(pl, tpc, dump) else "", pl.stages, pl.lpc, chains, tpc, pl.stages * chains)
    return fields, hoists(pl, tpc, dump)


def hoists(pl, tpc, dump):
    return hoist_built(pl.name, pl.precision) and tpc > HOIST_FROM and not dump


def where(b, chains):
    """Column b of a single chain launch: (tile, q, chain)."""
    tile = b // 16
    return tile, tile // chains, tile % chains


def assert_same_as_reference(y, y_ref, idx, chains, what):
    """Column b of the launch's samples y [B][N] holds the samples of reference column idx[b]; names the first one that does not with
    its place in the launch (tile, q = tile // chains, chain) and the utterances whose samples it holds instead."""
    bad = np.argwhere((y != y_ref[idx[:y.shape[0]]]).any(axis=1))
    if bad.size:
        b = int(bad[0, 0])
        tile, q, chain = where(b, chains)
        thief = [int(k) for k in range(y_ref.shape[0]) if np.array_equal(y_ref[k], y[b])]
        raise AssertionError("%s: column %d (tile %d = tile q = %d of chain %d, lane %d; utterance %d) differs from the one-tile run, first at "
                             "sample %d; %d columns differ; its samples are those of utterances %s" % (
                                 what, b, tile, q, chain, b % 16, int(idx[b]), int(np.argmax(y[b] != y_ref[idx[b]])), len(bad), thief))
