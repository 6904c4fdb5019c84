"""GPU tests of scoring with carried state (`-m gpu`): nvw_score_chunks scores a time chunk [k0, k0 + n) of an
utterance from the state blob at done = k0 and leaves the blob at done = k0 + n.  The contract is equality: logp and rows BIT FOR BIT
those of the whole pass (scoreSamples), blobs BYTE FOR BYTE those of prefillStates and of a sequentially primed column.  Only one
check uses a bar: one request against the float64 reference, within score_cases.bar.  Cut lists: tests/score_carry_cases.py."""
import struct

import numpy as np
import pytest
import torch

import mel_time_cases as MT
import prefill_cases as PF
import score_carry_cases as CC
import score_cases as SC
import test_mel_time_gpu as TM
import test_prefill_gpu as TP
import test_score_gpu as TS
from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import SCORE_CHUNK_MEL_REQ, SCORE_CHUNK_REQ
from nv_wavenet_amd.slots import SlotState, SlotStream

pytestmark = pytest.mark.gpu

GUARD = TS.GUARD
INT_MAX = 2 ** 31 - 1


def _bits(a):
    return a.contiguous().view(torch.int32)


def _walk(e, jobs, mel=False, rows=True):
    """jobs = [(y CUDA int32 [n], source, cuts, T, uid)] advance together, each along its own cut list, from silence: per job
    (logp [n], rows [n][A], [blob bytes behind every cut]).  source: features [n_cond][>= n], or (mel=True) the utterance's frames."""
    state = [None] * len(jobs)
    at = [0] * len(jobs)
    lp, rw, blobs = [[] for _ in jobs], [[] for _ in jobs], [[] for _ in jobs]
    for step in range(max(len(j[2]) for j in jobs)):
        live = [i for i, j in enumerate(jobs) if step < len(j[2])]
        reqs = []
        for i in live:
            y, src, cuts, T, uid = jobs[i]
            k0, m = at[i], cuts[step]
            reqs.append((state[i], y[k0:k0 + m], src if mel else src[:, k0:k0 + m], uid, T))
        got, out = (e.scoreChunksMel if mel else e.scoreChunks)(reqs, rows=rows, states=True)
        for i, g, b in zip(live, got, out):
            lp[i].append(g[0] if rows else g)
            if rows:
                rw[i].append(g[1])
            state[i] = b
            blobs[i].append(b)
            at[i] += jobs[i][2][step]
    torch.cuda.synchronize()
    return [(torch.cat(lp[i]), torch.cat(rw[i]) if rows else None, [b.cpu().numpy().tobytes() for b in blobs[i]]) for i in range(len(jobs))]


def _same_blob(got, want, what):
    if got != want:
        g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        first = int(np.nonzero(g != w)[0][0])
        raise AssertionError("%s: %d bytes differ, the first at %d (header words %s against %s)" %
                             (what, int((g != w).sum()), first, np.frombuffer(got[:64], dtype="<u4"), np.frombuffer(want[:64], dtype="<u4")))


# ---- 4, 5. chunks equal the whole pass, out-states equal prefill --------------------------------------------------------------------

_walks = {}


def _cut_walk(which, precision):
    """Per schedule and precision, computed once: every cut list walked at T = 1 and 0.5, three columns at a time; with it the whole
    pass of every column and the prefilled blob behind every cut."""
    key = (which, precision)
    if key not in _walks:
        if which == "prime_shape":
            net, n, lists = TS._prime_net(precision), CC.PRIME_N, CC.PRIME_CUTS
        else:
            shape, seed, L, maxD, N = SC.LONG
            net, n, lists = TS._net(shape, seed, precision, L, maxD, N), CC.LONG_N, CC.LONG_CUTS
        e = net.engine()
        out = []
        for T in (1.0, 0.5):
            whole = e.scoreSamples([net.req(c, n, T) for c in range(3)], rows=True)
            for g in range(0, len(lists), 3):
                group = lists[g:g + 3]
                jobs = [(net.yg[c, :n].contiguous(), net.xg[c], cuts, T, 100 + c) for c, cuts in enumerate(group)]
                got = _walk(e, jobs)
                pre = e.prefillStates([(net.yg[c, :k0 + m].contiguous(), net.xg[c], 100 + c, T) for c, cuts in enumerate(group)
                                       for k0, m in CC.starts(cuts)]).cpu().numpy()
                row = 0
                for c, cuts in enumerate(group):
                    want = [pre[row + i].tobytes() for i in range(len(cuts))]
                    row += len(cuts)
                    out.append(dict(T=T, c=c, cuts=cuts, logp=got[c][0], rows=got[c][1], blobs=got[c][2], whole=whole[c], prefilled=want))
        e.close()
        _walks[key] = (net, n, out)
    return _walks[key]


@pytest.mark.parametrize("which", ["prime_shape", "long"])
@pytest.mark.parametrize("precision", [16, 32])
def test_chunks_equal_the_whole_pass_bit_for_bit(which, precision):
    net, n, walks = _cut_walk(which, precision)
    assert len(walks) == 2 * len(CC.PRIME_CUTS if which == "prime_shape" else CC.LONG_CUTS)
    for w in walks:
        what = "%s fp%d T = %g column %d cuts %s" % (which, precision, w["T"], w["c"], w["cuts"][:6])
        assert w["logp"].shape == (n,) and w["rows"].shape == (n, net.s.A)
        assert torch.equal(_bits(w["logp"]), _bits(w["whole"][0])), what + ": logp"
        assert torch.equal(_bits(w["rows"]), _bits(w["whole"][1])), what + ": rows"
    if which == "long":
        w = next(w for w in walks if w["T"] == 1.0 and w["cuts"] == (127, 1, 128, 44))
        TS._hold(net, w["c"], n, 1.0, w["logp"], w["rows"], what="chunks (127, 1, 128, 44)")


@pytest.mark.parametrize("which", ["prime_shape", "long"])
@pytest.mark.parametrize("precision", [16, 32])
def test_out_states_equal_the_prefilled_blobs_byte_for_byte(which, precision):
    net, n, walks = _cut_walk(which, precision)
    for w in walks:
        done = 0
        for i, m in enumerate(w["cuts"]):
            done += m
            what = "%s fp%d T = %g column %d cuts %s, behind sample %d" % (which, precision, w["T"], w["c"], w["cuts"][:6], done)
            _same_blob(w["blobs"][i], w["prefilled"][i], what)
            words = np.frombuffer(w["blobs"][i][:64], dtype="<u4")
            y = net.y[w["c"]]
            assert int(words[6]) == done and int(words[7]) == 100 + w["c"], what
            assert int(words[8]) == (int(y[done - 2]) if done >= 2 else 128) and int(words[9]) == int(y[done - 1]), what
            assert int(words[10]) == (0 if w["T"] == 1.0 else struct.unpack("<I", struct.pack("<f", w["T"]))[0]), what


@pytest.mark.parametrize("precision", [16, 32])
def test_an_out_state_equals_a_column_started_primed_and_saved(precision):
    """(15, 33) and (17, 31) at T = 0.5: the blobs behind samples 15 and 17 and behind 48 against slotStart + slotSetTemperature +
    slotPrime + steps + slotSave."""
    net = TS._prime_net(precision)
    e = net.engine()
    jobs = [(net.yg[1, :48].contiguous(), net.xg[1], (15, 33), 0.5, 1), (net.yg[2, :48].contiguous(), net.xg[2], (17, 31), 0.5, 2)]
    got = _walk(e, jobs, rows=False)
    seq = TP._sequential_blobs(e, net.xg, [(3, 1, net.yg[1, :15].contiguous(), 0.5), (4, 2, net.yg[2, :17].contiguous(), 0.5),
                                           (5, 1, net.yg[1, :48].contiguous(), 0.5)], net.s.maxD)
    e.close()
    _same_blob(got[0][2][0], seq[3], "behind sample 15")
    _same_blob(got[1][2][0], seq[4], "behind sample 17")
    _same_blob(got[0][2][1], seq[5], "behind sample 48")


# ---- 6, 7. from a running column; candidates -----------------------------------------------------------------------------------------

_runs = {}


def _running_column(precision):
    """A slot session at the prime shape, one free-running column (utterance 1, uid 1, T = 0.5) saved at done = 1, 17, 40 and 48:
    (net, y [48] CUDA int32 = its samples, {done: blob CUDA uint8})"""
    if precision not in _runs:
        net = TS._prime_net(precision)
        e = net.engine()
        e.slotsBegin(net.s.maxD)
        col = 2
        e.slotStart(col, net.xg[1], 1)
        e.slotSetTemperature(col, 0.5)
        ys, blobs, done = [], {}, 0
        for upto in (1, 17, 33, 40, 48):
            out = torch.zeros((e.maxBatch, upto - done), dtype=torch.int32, device="cuda")
            assert e.slotsStep(upto - done, out)
            ys.append(out[col].clone())
            done = upto
            if upto != 33:
                blob, got = e.slotSave(col)
                assert got == upto
                blobs[upto] = blob
        torch.cuda.synchronize()
        e.slotsEnd()
        e.close()
        _runs[precision] = (net, torch.cat(ys).contiguous(), blobs)
    return _runs[precision]


@pytest.mark.parametrize("precision", [16, 32])
def test_chunks_behind_the_saved_state_of_a_running_column(precision):
    net, y, blobs = _running_column(precision)
    e = net.engine()
    x = net.xg[1]
    whole_lp, whole_rows = e.scoreSamples([(y, x, 0.5)], rows=True)[0]
    final = blobs[48].cpu().numpy().tobytes()
    for k in (1, 17, 40):
        before = blobs[k].cpu().numpy().tobytes()
        got, out = e.scoreChunks([(blobs[k], y[k:], x[:, k:48], 999, 0.5)], rows=True, states=True)
        assert torch.equal(_bits(got[0][0]), _bits(whole_lp[k:])) and torch.equal(_bits(got[0][1]), _bits(whole_rows[k:])), "from done = %d" % k
        _same_blob(out[0].cpu().numpy().tobytes(), final, "the out-state at 48 from done = %d against the column's own save" % k)
        assert blobs[k].cpu().numpy().tobytes() == before, "the in-state was written"
    e.close()


@pytest.mark.parametrize("precision", [16, 32])
def test_candidates_share_one_in_state(precision):
    net, y, blobs = _running_column(precision)
    e = net.engine()
    x, A = net.xg[1], net.s.A
    state = blobs[17]
    before = state.cpu().numpy().tobytes()
    rng = np.random.RandomState(21)
    cands = [torch.from_numpy(rng.randint(0, A, size=31).astype(np.int32)).cuda() for _ in range(5)]
    reqs = [(state, c, x[:, 17:48], 7, 0.5) for c in cands]
    together, out = e.scoreChunks(reqs, rows=True, states=True)
    assert state.cpu().numpy().tobytes() == before, "the shared in-state was written"
    for i, c in enumerate(cands):
        full = torch.cat([y[:17], c]).contiguous()
        lp, rows = e.scoreSamples([(full, x, 0.5)], rows=True)[0]
        assert torch.equal(_bits(together[i][0]), _bits(lp[17:])) and torch.equal(_bits(together[i][1]), _bits(rows[17:])), "candidate %d" % i
        _same_blob(out[i].cpu().numpy().tobytes(), e.prefillStates([(full, x, 1, 0.5)])[0].cpu().numpy().tobytes(), "candidate %d" % i)
    alone = e.scoreChunks([reqs[3]], rows=True)[0]
    assert torch.equal(_bits(alone[0]), _bits(together[3][0])) and torch.equal(_bits(alone[1]), _bits(together[3][1])), "alone differs from among others"
    e.close()


# ---- 8. every built shape and both odd depths ---------------------------------------------------------------------------------------

def _shape_check(net, n=48, cuts=(17, 31)):
    e = net.engine()
    jobs = [(net.yg[c, :n].contiguous(), net.xg[c], cuts, 1.0, 40 + c) for c in range(2)]
    got = _walk(e, jobs)
    whole = e.scoreSamples([net.req(c, n) for c in range(2)], rows=True)
    pre = e.prefillStates([(net.yg[c, :k].contiguous(), net.xg[c], 40 + c, 1.0) for c in range(2) for k in (17, 48)]).cpu().numpy()
    e.close()
    for c in range(2):
        assert torch.equal(_bits(got[c][0]), _bits(whole[c][0])) and torch.equal(_bits(got[c][1]), _bits(whole[c][1])), c
        for i in range(2):
            _same_blob(got[c][2][i], pre[2 * c + i].tobytes(), "column %d behind cut %d" % (c, i))


@pytest.mark.parametrize("shape", sorted(SC.BUILT))
@pytest.mark.parametrize("precision", [16, 32])
def test_every_built_shape(shape, precision):
    _shape_check(TS._net(shape, SC.BUILT[shape], precision))


@pytest.mark.parametrize("depth", range(len(SC.DEPTHS)))
@pytest.mark.parametrize("precision", [16, 32])
def test_odd_and_minimal_depth(depth, precision):
    shape, seed, L, maxD, N = SC.DEPTHS[depth]
    _shape_check(TS._net(shape, seed, precision, L, maxD, N))


# ---- 9. mel ------------------------------------------------------------------------------------------------------------------------

# (window, stride), n a little over two frames, cut lists with k0 inside a frame and at a frame edge
MEL_CASES = [((8, 2), 48, 5, [(1, 2, 2), (2, 3), (3, 1, 1)]), ((8, 2), 48, 47, [(5, 16, 26), (16, 31)]),
             ((1024, 256), 768, 517, [(100, 156, 261), (256, 261), (511, 6)])]


@pytest.mark.parametrize("case", range(len(MEL_CASES)))
@pytest.mark.parametrize("precision", [16, 32])
def test_chunks_from_mel_equal_the_whole_pass_and_the_prefilled_blobs(case, precision):
    hop, N, n, lists = MEL_CASES[case]
    assert hop in ((MT.PRIME_HOPS[0]), (1024, 256)) and n > 2 * hop[1] and n < 3 * hop[1] or n == 47
    assert any(k0 % hop[1] for cuts in lists for k0, _ in CC.starts(cuts)[1:]) and any(k0 % hop[1] == 0 for cuts in lists for k0, _ in CC.starts(cuts)[1:])
    shape, seed, L, maxD, _ = SC.PRIME_SHAPE
    ms = TM.MelSetup(shape, seed, precision, hop, L, maxD, N)
    e = ms.engine()
    for T in (1.0, 0.5):
        jobs = [(ms.yg[c, :n].contiguous(), ms.melg[c], cuts, T, 60 + c) for c, cuts in enumerate(lists)]
        got = _walk(e, jobs, mel=True)
        whole = e.scoreSamplesMel([(ms.yg[c, :n].contiguous(), ms.melg[c], T) for c in range(len(lists))], rows=True)
        pre = e.prefillStatesMel([(ms.yg[c, :k0 + m].contiguous(), ms.melg[c], 60 + c, T) for c, cuts in enumerate(lists)
                                  for k0, m in CC.starts(cuts)]).cpu().numpy()
        row = 0
        for c, cuts in enumerate(lists):
            assert torch.equal(_bits(got[c][0]), _bits(whole[c][0])) and torch.equal(_bits(got[c][1]), _bits(whole[c][1])), (hop, cuts, T)
            for i in range(len(cuts)):
                _same_blob(got[c][2][i], pre[row + i].tobytes(), "hop %s cuts %s T = %g behind cut %d" % (hop, cuts, T, i))
            row += len(cuts)
    e.close()


# ---- 10. nothing else is written or read -------------------------------------------------------------------------------------------

def _raw(e, reqs, count=None, mel=False):
    dt = SCORE_CHUNK_MEL_REQ if mel else SCORE_CHUNK_REQ
    arr = np.zeros(max(len(reqs), 1), dtype=dt)
    for i, r in enumerate(reqs):
        arr[i] = tuple(r[k] for k in dt.names)
    got = (lib.nvw_score_chunks_mel if mel else lib.nvw_score_chunks)(e._h, arr.ctypes.data, len(reqs) if count is None else count, None)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("precision", [16, 32])
def test_nothing_else_is_written_and_nothing_outside_the_chunk_is_read(precision):
    net = TS._prime_net(precision)
    A, N = net.s.A, 48
    e = net.engine()
    nbytes = e.slotStateBytes()
    for k0, n, pinned in ((0, 17, False), (17, 14, False), (17, 14, True), (31, 17, False)):
        y, x = net.yg[0, :N], net.xg[0]
        state = e.prefillStates([(y[:k0].contiguous(), x, 5, 1.0)])[0].contiguous() if k0 else None
        (ref_lp, ref_rows), ref_blob = [g[0] for g in e.scoreChunks([(state, y[k0:k0 + n], x[:, k0:k0 + n], 5, 1.0)], rows=True, states=True)]
        ref_blob = ref_blob.cpu().numpy().tobytes()
        # poison: the features outside the chunk's columns, y outside the chunk
        xp = torch.full_like(x, float("nan"))
        xp[:, k0:k0 + n] = x[:, k0:k0 + n]
        yp = (y + 97) % A
        yp[k0:k0 + n] = y[k0:k0 + n]
        lbuf = torch.full((n + 64,), GUARD, dtype=torch.int32)
        lbuf = lbuf.pin_memory() if pinned else lbuf.cuda()
        rbuf = torch.full(((n + 2) * A,), GUARD, dtype=torch.int32, device="cuda")
        sbuf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8)
        sbuf = sbuf.pin_memory() if pinned else sbuf.cuda()
        req = dict(state=state.data_ptr() if k0 else 0, y=yp.data_ptr() + 4 * k0, n=n, x=xp[:, k0:].data_ptr(), precision=32, c_stride=xp.stride(0),
                   t_stride=xp.stride(1), uid=5, temperature=1.0, logp=lbuf.data_ptr() + 4 * 29, rows=rbuf.data_ptr() + 4 * A,
                   state_out=sbuf.data_ptr() + 64)
        assert _raw(e, [req]) == 1
        lb, rb, sb = lbuf.cpu().numpy(), rbuf.cpu().numpy(), sbuf.cpu().numpy()
        assert (lb[:29] == GUARD).all() and (lb[29 + n:] == GUARD).all(), (k0, n)
        assert (rb[:A] == GUARD).all() and (rb[(n + 1) * A:] == GUARD).all(), (k0, n)
        assert (sb[:64] == 0xA5).all() and (sb[64 + nbytes:] == 0xA5).all(), (k0, n)
        assert np.array_equal(lb[29:29 + n], _bits(ref_lp).cpu().numpy()), "poison outside the chunk changed logp (k0 = %d)" % k0
        assert np.array_equal(rb[A:(n + 1) * A], _bits(ref_rows).cpu().numpy().ravel())
        _same_blob(sb[64:64 + nbytes].tobytes(), ref_blob, "k0 = %d n = %d" % (k0, n))
    e.close()


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_return_0_write_nothing_and_raise_in_python():
    net = TS._prime_net(16)
    s = net.s
    A, k0, n = s.A, 17, 31
    e = net.engine()
    nbytes = e.slotStateBytes()
    y, x = net.yg[0, k0:k0 + n].contiguous(), net.xg[0][:, k0:]
    good = e.prefillStates([(net.yg[0, :k0].contiguous(), net.xg[0], 5, 1.0)])[0].contiguous()
    torch.cuda.synchronize()
    lbuf = torch.full((n + 8,), GUARD, dtype=torch.int32, device="cuda")
    rbuf = torch.full((n * A + 8,), GUARD, dtype=torch.int32, device="cuda")
    sbuf = torch.full((3 * nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    other = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((lbuf == GUARD).all()) and bool((rbuf == GUARD).all()) and bool((sbuf == 0xA5).all()) and bool((other == 0xA5).all())

    def base(**kw):
        req = dict(state=good.data_ptr(), y=y.data_ptr(), n=n, x=x.data_ptr(), precision=32, c_stride=x.stride(0), t_stride=x.stride(1), uid=5,
                   temperature=1.0, logp=lbuf.data_ptr(), rows=rbuf.data_ptr(), state_out=sbuf.data_ptr())
        req.update(kw)
        return req

    def call(engine=e, count=None, second=None, **kw):
        reqs = [base(**kw)] + ([second] if second is not None else [])
        got = _raw(engine, reqs, count)
        assert got or untouched(), "a refused call wrote into its outputs (%s)" % (kw,)
        return got

    def mutated(word, value):
        b = good.clone()
        b.view(torch.int32)[word] = value
        return b

    # everything nvw_score_samples refuses
    bare = net.engine(weights=False)
    assert call(engine=bare) == 0                                                                          # no conditioning weights
    with pytest.raises(ValueError):
        bare.scoreChunks([(None, y, x, 5, 1.0)])
    bare.close()
    assert call(count=0) == 0 and call(count=-1) == 0 and call(count=65536) == 0
    assert call(n=0) == 0 and call(n=-3) == 0
    for T in (2.0 ** -11, 2.0 ** 11, float("nan"), 0.0):
        assert call(temperature=T) == 0, T
    assert call(precision=8) == 0 and call(c_stride=0) == 0 and call(t_stride=-1) == 0
    assert call(y=0) == 0 and call(x=0) == 0
    host_y = np.ascontiguousarray(net.y[0, k0:k0 + n])
    assert call(y=host_y.ctypes.data) == 0
    assert call(logp=0) == 0 and call(logp=lbuf.data_ptr() + 2) == 0 and call(rows=rbuf.data_ptr() + 4) == 0
    # the in-state
    keep = [mutated(0, 0x12345678), mutated(1, 2), mutated(2, 32), mutated(3, 128), mutated(4, s.L + 1), mutated(5, 2 * s.maxD),
            mutated(10, 1), mutated(10, struct.unpack("<i", struct.pack("<f", 2.0 ** 11))[0]), mutated(6, -1)]
    torch.cuda.synchronize()
    for i, b in enumerate(keep):
        assert call(state=b.data_ptr()) == 0, "mutation %d of the header" % i                             # magic, version, precision, R, L, maxD, word 10, done
    pageable = np.frombuffer(good.cpu().numpy().tobytes(), dtype=np.uint8).copy()
    assert call(state=pageable.ctypes.data) == 0                                                          # pageable host memory
    shifted = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    shifted[8:8 + nbytes] = good
    torch.cuda.synchronize()
    assert call(state=shifted.data_ptr() + 8) == 0                                                        # misaligned
    late = mutated(6, INT_MAX - 16 - n + 1)
    assert call(state=late.data_ptr()) == 0                                                               # done + n beyond INT_MAX - 16
    # the out-state
    assert call(state_out=sbuf.data_ptr() + 8) == 0                                                       # misaligned
    host_out = np.full(nbytes, 0xA5, dtype=np.uint8)
    assert call(state_out=host_out.ctypes.data) == 0 and (host_out == 0xA5).all()                          # unreachable
    before = good.cpu().numpy().tobytes()
    assert call(state_out=good.data_ptr()) == 0                                                           # the request's own in-state
    inside = torch.full((2 * nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    inside[nbytes - 64:2 * nbytes - 64] = good
    torch.cuda.synchronize()
    assert call(state=inside.data_ptr() + nbytes - 64, state_out=inside.data_ptr()) == 0                  # ... overlapping its tail
    assert call(second=base(logp=lbuf.data_ptr(), state_out=sbuf.data_ptr())) == 0                         # two requests, one out-state
    assert call(second=base(state_out=sbuf.data_ptr() + nbytes - 64)) == 0                                 # ... overlapping out-states
    twin = good.clone()
    assert call(state=0, state_out=twin.data_ptr(), second=base(state=twin.data_ptr(), state_out=0)) == 0  # request 0's out-state is request 1's in-state
    assert good.cpu().numpy().tobytes() == before and twin.cpu().numpy().tobytes() == before
    # a total over the cap
    cap = e.scoreMaxSamples()
    big = cap + 16
    by, bx, bl = torch.zeros(big, dtype=torch.int32, device="cuda"), torch.zeros((80, big), dtype=torch.float16, device="cuda"), \
        torch.full((big,), GUARD, dtype=torch.int32, device="cuda")
    over = dict(state=0, y=by.data_ptr(), n=big, x=bx.data_ptr(), precision=16, c_stride=bx.stride(0), t_stride=bx.stride(1), logp=bl.data_ptr(), rows=0)
    assert call(**over) == 0 and bool((bl == GUARD).all())
    half = dict(over, n=cap // 2 + 16)
    assert call(second=base(**dict(half, state_out=0)), **half) == 0 and bool((bl == GUARD).all())       # ... the SUM of the padded n
    del by, bx, bl
    assert untouched()
    # ... and the call they all vary
    assert call() == 1
    assert bool((lbuf[:n] != GUARD).all()) and bool((lbuf[n:] == GUARD).all()) and bool((sbuf[nbytes:] == 0xA5).all())
    _same_blob(sbuf[:nbytes].cpu().numpy().tobytes(), e.prefillStates([(net.yg[0, :48].contiguous(), net.xg[0], 5, 1.0)])[0].cpu().numpy().tobytes(),
               "the accepted call")
    with pytest.raises(ValueError):
        e.scoreChunks([])
    with pytest.raises(ValueError):
        e.scoreChunks([(good, y, x, 5, 0.0)])
    with pytest.raises(ValueError):
        e.scoreChunks([(mutated(0, 1), y, x, 5, 1.0)])
    with pytest.raises(ValueError):
        e.scoreChunks([(good[:-16], y, x, 5, 1.0)])
    with pytest.raises(ValueError):
        e.scoreChunks([(good.cpu(), y, x, 5, 1.0)])
    e.close()


def test_mel_chunks_refuse_frames_that_do_not_cover_the_chunk():
    shape, seed, L, maxD, N = SC.PRIME_SHAPE
    ms = TM.MelSetup(shape, seed, 16, (12, 4), L, maxD, N)
    e = ms.engine()
    y, mel = ms.yg[0, :48].contiguous(), ms.melg[0]
    state = e.prefillStatesMel([(y[:17].contiguous(), mel, 3, 1.0)])[0].contiguous()
    lbuf = torch.full((40,), GUARD, dtype=torch.int32, device="cuda")
    sbuf = torch.full((e.slotStateBytes(),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(eng=e, **kw):
        req = dict(state=state.data_ptr(), y=y.data_ptr() + 4 * 17, n=31, mel=mel.data_ptr(), precision=32, c_stride=mel.stride(0),
                   f_stride=mel.stride(1), frames=12, uid=3, temperature=1.0, logp=lbuf.data_ptr(), rows=0, state_out=sbuf.data_ptr())
        req.update(kw)
        got = _raw(eng, [req], mel=True)
        assert got or (bool((lbuf == GUARD).all()) and bool((sbuf == 0xA5).all()))
        return got

    assert call(frames=11) == 0                                        # 44 < 17 + 31
    assert call(frames=4, n=1) == 0                                    # 16 < 17 + 1: the chunk starts past the frames
    assert call(mel=0) == 0 and call(f_stride=0) == 0 and call(state=state.data_ptr() + 8) == 0
    bare = TM._engine(ms.case, ms.t, 16, "wg", ms.w, ms.b, 2)            # no upsampling table
    assert call(eng=bare) == 0
    with pytest.raises(ValueError):
        bare.scoreChunksMel([(None, y, mel, 3, 1.0)])
    bare.close()
    with pytest.raises(ValueError):
        e.scoreChunksMel([(state, y[17:], mel, 3, 1.0, 11)])
    assert call() == 1
    want = e.scoreSamplesMel([(y, mel, 1.0)])[0]
    assert np.array_equal(lbuf[:31].cpu().numpy(), _bits(want[17:]).cpu().numpy()) and bool((lbuf[31:] == GUARD).all())
    e.close()


# ---- 12. wrappers ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [16, 32, 20])
def test_the_wrapper_scores_utterances_over_the_cap_in_chunks(chunk):
    """NVWaveNetEngine.score(chunk=) with the engine's scoreMaxSamples replaced by 32, as the split test of tests/test_score_gpu.py
    replaces it: the 48-sample utterances that chunk=None refuses score, bit for bit as the unpatched whole pass; a step of
    batch x chunk over the cap is split over the batch; the final blobs are those of prefillStates."""
    NW, wrapper, case, t, x, w, b, xg, cw, cb = TS._wrapper(32)
    s = case.shape
    y = torch.from_numpy(PF.primes(s.B, s.N, s.A, seed=8)).cuda()
    lengths = [48, 0, 17, 33] + [48] * (s.B - 4)
    temps = [1.0, 0.5] * (s.B // 2)
    whole, whole_rows = wrapper.score(xg, cw, cb, y, lengths=lengths, temperature=temps, return_rows=True)
    e = next(iter(wrapper._engines.values()))
    calls = []
    real = e.scoreChunks
    e.scoreMaxSamples = lambda: 32
    e.scoreChunks = lambda reqs, **kw: (calls.append(len(reqs)), real(reqs, **kw))[1]
    with pytest.raises(ValueError):
        wrapper.score(xg, cw, cb, y)                                       # chunk=None: as it was
    with pytest.raises(ValueError):
        wrapper.score(xg, cw, cb, y, chunk=33)                             # one chunk of one utterance over the cap
    with pytest.raises(ValueError):
        wrapper.score(xg, cw, cb, y, chunk=0)
    assert not calls
    logp, rows, blobs = wrapper.score(xg, cw, cb, y, lengths=lengths, temperature=temps, return_rows=True, chunk=chunk, return_state=True)
    step = -(-chunk // 16) * 16
    assert max(calls) == 32 // step and sum(calls) == sum(-(-k // step) for k in lengths), calls
    del e.scoreMaxSamples, e.scoreChunks
    assert torch.equal(_bits(logp), _bits(whole)) and torch.equal(_bits(rows), _bits(whole_rows))
    pre = e.prefillStates([(y[c, :lengths[c]].int().contiguous(), xg[c], c, temps[c]) for c in range(s.B) if lengths[c]]).cpu().numpy()
    have = [c for c in range(s.B) if lengths[c]]
    got = blobs.cpu().numpy()
    for i, c in enumerate(have):
        _same_blob(got[c].tobytes(), pre[i].tobytes(), "utterance %d" % c)
    assert not got[1].any()
    wrapper.close()


def test_the_wrapper_scores_mel_in_chunks():
    from nv_wavenet_amd import nv_wavenet as NW
    shape, seed, L, maxD, N = SC.PRIME_SHAPE
    ms = TM.MelSetup(shape, seed + 7, 16, (12, 4), L, maxD, N, columns=4)
    ms.t.Bzs[:] = 0
    ms.t.Bza[:] = 0
    kw = SC.wrapper_weights(ms.t, ms.s)
    dev = {k: ([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in v] if isinstance(v, list) else
               torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    wrapper = NW.NVWaveNetEngine(**dev, precision=16)
    up_w, up_b = torch.from_numpy(ms.up_w).cuda(), torch.from_numpy(ms.up_b).cuda()
    cw, cb = torch.from_numpy(ms.w[:, :, None].copy()).cuda(), torch.from_numpy(ms.b).cuda()
    args = (ms.melg, up_w, up_b, ms.stride, cw, cb, ms.yg)
    whole = wrapper.score_mel(*args, lengths=[48, 47, 5, 33])
    e = next(iter(wrapper._engines.values()))
    e.scoreMaxSamples = lambda: 32
    with pytest.raises(ValueError):
        wrapper.score_mel(*args, lengths=[48, 47, 5, 33])
    logp, blobs = wrapper.score_mel(*args, lengths=[48, 47, 5, 33], chunk=16, return_state=True)
    del e.scoreMaxSamples
    assert torch.equal(_bits(logp), _bits(whole))
    pre = e.prefillStatesMel([(ms.yg[c, :k].contiguous(), ms.melg[c], c, 1.0) for c, k in enumerate([48, 47, 5, 33])]).cpu().numpy()
    for c in range(4):
        _same_blob(blobs[c].cpu().numpy().tobytes(), pre[c].tobytes(), "mel utterance %d" % c)
    wrapper.close()


def _deliver(stream, sink):
    steps = 0
    while stream.busy():
        for h, (y, _) in stream.step(7).items():
            sink.setdefault(h, []).append(np.array(y))
        stream.finished()
        steps += 1
        assert steps < 200


def test_slot_stream_score_from():
    """score_from on a suspended request, on a prefill state, on a never-started state and on a state after to_bytes / from_bytes;
    resume(score_from(..., return_state=True)[1]) delivers from done + m on what a request primed with the same samples, without
    prefill, delivers."""
    net = TS._prime_net(16)
    s, N = net.s, 48
    e, e2 = net.engine(), net.engine()
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, s.maxD, pcm=False)
    # a suspended request: 14 samples of free generation at T = 0.5, then its state
    h = st.submit(net.xg[1], uid=1, temperature=0.5)
    got = {}
    for _ in range(2):
        for hh, (y, _) in st.step(7).items():
            got.setdefault(hh, []).append(np.array(y))
    head = np.concatenate(got[h])
    state = st.suspend(h)
    assert state.done == 14 and state.temperature == 0.5
    cont = net.yg[1, 14:31].contiguous()                                            # 17 known samples behind it
    full = torch.cat([torch.from_numpy(head).cuda().int(), cont]).contiguous()
    whole = e.scoreSamples([(full, net.xg[1], 0.5)])[0]
    lp = st.score_from(state, cont)                                                 # (the state's temperature)
    assert torch.equal(_bits(lp), _bits(whole[14:]))
    assert not torch.equal(_bits(st.score_from(state, cont, temperature=1.0)), _bits(lp))
    lp2, after = st.score_from(state, cont.cpu(), return_state=True)
    assert torch.equal(_bits(lp2), _bits(lp)) and after.done == 31 and after.uid == 1 and after.kind == "features" and state.done == 14
    _same_blob(after.blob.cpu().numpy().tobytes(), e.prefillStates([(full, net.xg[1], 1, 0.5)])[0].cpu().numpy().tobytes(), "score_from's state")
    # ... after to_bytes / from_bytes, scored again and resumed
    back = SlotState.from_bytes(after.to_bytes(), net.xg[1])
    assert back.done == 31 and back.temperature == 0.5
    more = net.yg[1, 31:40].contiguous()
    lp3 = st.score_from(back, more)
    assert torch.equal(_bits(lp3), _bits(e.scoreSamples([(torch.cat([full, more]).contiguous(), net.xg[1], 0.5)])[0][31:]))
    sink, sink2 = {}, {}
    hr = st.resume(back)
    h2 = st2.submit(net.xg[1], uid=1, temperature=0.5, prime=full.cpu())
    # a prefill state and a never-started state
    pre = st.prefill(net.xg[2], net.yg[2, :17].cpu(), uid=2)
    lp4, after4 = st.score_from(pre, net.yg[2, 17:33], return_state=True)
    assert torch.equal(_bits(lp4), _bits(e.scoreSamples([(net.yg[2, :33].contiguous(), net.xg[2], 1.0)])[0][17:])) and after4.done == 33
    hq = st.submit(net.xg[0], uid=9, temperature=2.0)
    fresh = st.suspend(hq)
    assert fresh.blob is None and fresh.done == 0
    lp5, after5 = st.score_from(fresh, net.yg[0, :20], return_state=True)
    assert torch.equal(_bits(lp5), _bits(e.scoreSamples([(net.yg[0, :20].contiguous(), net.xg[0], 2.0)])[0])) and after5.done == 20 and after5.uid == 9
    _same_blob(after5.blob.cpu().numpy().tobytes(), e.prefillStates([(net.yg[0, :20].contiguous(), net.xg[0], 9, 2.0)])[0].cpu().numpy().tobytes(),
               "from a state that never started")
    with pytest.raises(ValueError):
        st.score_from(after4, net.yg[2, :16])                                        # 16 samples behind 33 of 48
    h4 = st.resume(after4)
    h42 = st2.submit(net.xg[2], uid=2, prime=net.yg[2, :33].cpu())
    _deliver(st, sink)
    _deliver(st2, sink2)
    for a, b, done in ((hr, h2, 31), (h4, h42, 33)):
        g, f = np.concatenate(sink[a]), np.concatenate(sink2[b])
        assert len(f) == N and len(g) == N - done and np.array_equal(g, f[done:]), "from %d on" % done
    st.close(), st2.close()
    e.close(), e2.close()


def test_slot_stream_score_from_mel():
    ms = TM.MelSetup(SC.PRIME_SHAPE[0], 961, 16, (12, 4), columns=4)
    e = ms.engine()
    st = SlotStream(e, ms.s.maxD, pcm=False)
    h = st.submit_mel(ms.melg[1], uid=1)
    got = []
    for _ in range(3):
        for hh, (y, _) in st.step(5).items():
            got.append(np.array(y))
    state = st.suspend(h)
    assert state.kind == "mel" and state.done == 15
    head = torch.from_numpy(np.concatenate(got)).cuda().int()
    cont = ms.yg[1, 15:37].contiguous()
    full = torch.cat([head, cont]).contiguous()
    lp, after = st.score_from(state, cont, return_state=True)
    assert torch.equal(_bits(lp), _bits(e.scoreSamplesMel([(full, ms.melg[1], 1.0)])[0][15:]))
    assert after.kind == "mel" and after.done == 37 and after.frames == state.frames and after.final == state.final
    _same_blob(after.blob.cpu().numpy().tobytes(), e.prefillStatesMel([(full, ms.melg[1], 1, 1.0)])[0].cpu().numpy().tobytes(), "mel score_from")
    st.close()
    e.close()


# ---- 13. no interference -----------------------------------------------------------------------------------------------------------

def test_generation_is_the_same_with_chunk_calls_in_between():
    NW, wrapper, case, t, x, w, b, xg, cw, cb = TS._wrapper(16)
    y1 = wrapper.infer_features(xg, cw, cb, NW.Impl.SINGLE_BLOCK, seed=9)
    logp = wrapper.score(xg, cw, cb, y1, chunk=16)
    assert len(wrapper._engines) == 1, "score(chunk=) made an engine of its own"
    y2 = wrapper.infer_features(xg, cw, cb, NW.Impl.SINGLE_BLOCK, seed=9)
    assert torch.equal(_bits(wrapper.score(xg, cw, cb, y1)), _bits(logp))
    wrapper.close()
    assert torch.equal(y1, y2)


def test_slot_streams_prefill_and_scoring_are_the_same_with_chunk_calls_in_between():
    net = TS._prime_net(16)
    s = net.s
    e, e2 = net.engine(), net.engine()
    st, st2 = SlotStream(e, s.maxD, pcm=False), SlotStream(e2, s.maxD, pcm=False)
    blob = e.prefillStates([(net.yg[0, :31].contiguous(), net.xg[0], 3, 1.0)]).cpu()
    whole = e.scoreSamples([net.req(1, 33)])[0].clone()
    state = st.prefill(net.xg[1], net.yg[1, :17].cpu(), uid=50)
    hs = [st.submit(net.xg[c], uid=c) for c in range(3)]
    hs2 = [st2.submit(net.xg[c], uid=c) for c in range(3)]
    got, got2, scored = {}, {}, []
    while st.busy():
        for h, (y, _) in st.step(7).items():
            got.setdefault(h, []).append(np.array(y))
        st.finished()
        scored.append(st.score_from(state, net.yg[1, 17:33]))
    _deliver(st2, got2)
    for h, h2 in zip(hs, hs2):
        a, b = np.concatenate(got[h]), np.concatenate(got2[h2])
        assert len(a) == s.N and np.array_equal(a, b), "a stream with chunk calls in between delivers other samples"
    assert all(torch.equal(_bits(v), _bits(whole[17:])) for v in scored)
    assert torch.equal(_bits(e.scoreSamples([net.req(1, 33)])[0]), _bits(whole)), "a whole pass after chunk calls gives other values"
    assert torch.equal(e.prefillStates([(net.yg[0, :31].contiguous(), net.xg[0], 3, 1.0)]).cpu(), blob), "a prefill after chunk calls gives another blob"
    st.close(), st2.close()
    e.close(), e2.close()
