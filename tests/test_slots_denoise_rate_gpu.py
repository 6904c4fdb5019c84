"""GPU tests of slot mode's denoised delivery at the caller's rate in one launch (`-m gpu`): the session of
tests/test_slots_denoise_gpu.py -- R = 32, a window of 40, 20 columns, six utterances of 152, 20, 33, 96, 77 and 101 samples behind
16 fillers, two joining five samples apart, strengths 0.1 and 1 by utterance.  Per utterance the pieces, concatenated, are held bit
for bit to nvw_resample of nvw_denoise of its whole model-rate PCM, computed through the stateless entries on a second engine; and
to the float64 polyphase definition of nvw_denoise's int16 output within test_resample_gpu's own bar (the cleaned stream itself is
held to the float64 STFT by the tests of §6r and §6s: an end-to-end float64 bar would have to absorb rounding flips of the int16
intermediate, about sum |h| each, and would hide an off-by-one tail)."""
import functools

import numpy as np
import pytest
import torch

from nv_wavenet_amd import WavenetEngine
from nv_wavenet_amd.slots import SlotState, SlotStream, rate_tail_len
from oracle import oracle as O
from test_denoise_gpu import _bias
from test_resample_gpu import _bar, _reference
from test_slots_gpu import _engine
from test_slots_rate_gpu import CANARY, COLUMNS, FILLERS, W, _setup, _taps

pytestmark = pytest.mark.gpu

LENGTHS = [152, 20, 33, 96, 77, 101]          # n_fft = 64: 20 <= n_fft / 2 < 33
STRENGTHS = [0.1, 1.0]                        # of the even and the odd utterances
# L, M, n_fft, hop, step, window: the last two give a piece more than 16 frames, hence sub-range launches with all three states
# flipping (at 64 / 4 a finishing sub-range has exactly the 16 frames that a launch takes)
RUNS = [(L, M, 64, 16, step, W) for L, M in ((2, 1), (1, 3), (147, 80)) for step in (1, 37, 24)] + \
    [(147, 80, 64, 8, 150, 160), (2, 1, 64, 4, 37, W)]


def _stream(L, M, n_fft, hop, window):
    case, m, x, w, t = _setup()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], COLUMNS)
    e.setDenoiser(n_fft, hop, _bias(n_fft))
    e.setResampler(0, L, M, _taps(L, M))
    return SlotStream(e, window, owns_engine=True, deliver=0, denoise=STRENGTHS[0])


def _service(L, M, n_fft, hop, step, window, compact_at=None, suspend_at=None, drop=()):
    """uid -> (samples, PCM, [(first output, outputs) of every piece]) of the six utterances; suspend_at: utterance 0 goes through
    bytes to a second stream before that step, without the fields of its state named in `drop`."""
    x = _setup()[2]
    st, st2 = _stream(L, M, n_fft, hop, window), (_stream(L, M, n_fft, hop, window) if suspend_at is not None else None)
    who = {}
    got = {u: ([], [], []) for u in range(6)}

    def submit(u):
        who[(id(st), st.submit(x[u][:, :LENGTHS[u]], uid=u, denoise_strength=STRENGTHS[1] if u % 2 else None))] = u

    for f in range(FILLERS):
        st.submit(x[0][:, :1], uid=100 + f)
    for u in range(4):
        submit(u)
    for it, size in enumerate([step, 5] + [step] * (LENGTHS[0] + 8)):      # utterances 4 and 5 join 5 samples apart
        if it in (1, 2):
            submit(3 + it)
        if it == compact_at:
            assert st.compact() >= 2
        if it == suspend_at:
            state = st.suspend(next(h for (s, h), u in who.items() if u == 0))
            assert 0 < state.done < LENGTHS[0] and state.denoise is not None and state.tail is not None
            state = SlotState.from_bytes(state.to_bytes(), state.source)
            for field in drop:
                setattr(state, field, None)
            who[(id(st2), st2.resume(state))] = 0
        busy = [s for s in (st, st2) if s is not None and s.busy()]
        if not busy:
            break
        for s in busy:
            out = s.step_async(size).result()
            for i, h in enumerate(out.handles):
                u = who.get((id(s), int(h)))
                if u is not None:
                    y, pcm = out._slice(i)
                    got[u][0].append(y.copy())
                    got[u][1].append(pcm.copy())
                    got[u][2].append((int(out.pcm_first[i]), len(pcm)))
    for s in (st, st2):
        if s is not None:
            assert not s.busy()
            s.close()
    return {u: (np.concatenate(y), np.concatenate(p), m0s) for u, (y, p, m0s) in got.items()}


_undisturbed = functools.lru_cache(maxsize=None)(_service)


@pytest.fixture(scope="module")
def stateless():
    e = WavenetEngine(64, 256, 256, 3, 4, 1, 64, precision=32)
    yield e
    e.close()


def _whole(e, L, M, n_fft, hop, y, strength):
    """(nvw_resample of z, z) with z = nvw_denoise of the utterance's whole model-rate PCM, both int16 and last = 1; a stream that
    nvw_denoise refuses is its own z"""
    z = torch.from_numpy(O.mulaw_pcm_table(256)[y]).cuda()
    if len(y) > n_fft // 2:
        x, z = z, torch.zeros(len(y), dtype=torch.int16, device="cuda")
        e.setDenoiser(n_fft, hop, _bias(n_fft))
        e.denoise([(x, 0, True, z, 0, strength)])
    out = torch.zeros(-(-len(y) * L // M), dtype=torch.int16, device="cuda")
    e.setResampler(1, L, M, _taps(L, M))
    e.resample(1, [(z, 0, True, out, 0)])
    e.synchronize()
    return out.cpu().numpy(), z.cpu().numpy()


@pytest.mark.parametrize("L, M, n_fft, hop, step, window", RUNS)
def test_pieces_concatenated_are_resample_of_denoise_bit_for_bit(stateless, L, M, n_fft, hop, step, window):
    for u, (y, pcm, m0s) in _undisturbed(L, M, n_fft, hop, step, window).items():
        assert len(y) == LENGTHS[u]
        want, z = _whole(stateless, L, M, n_fft, hop, y, STRENGTHS[u % 2])
        assert [m0 for m0, _ in m0s] == list(np.cumsum([0] + [n for _, n in m0s[:-1]])), (u, m0s)      # contiguous from output 0
        assert len(pcm) == -(-LENGTHS[u] * L // M) and np.array_equal(pcm, want), (u, np.flatnonzero(pcm != want)[:8])
        assert (LENGTHS[u] <= n_fft // 2) == np.array_equal(z, O.mulaw_pcm_table(256)[y])              # only the short one is unchanged


def test_against_the_float64_definition_of_the_rate_stage(stateless):
    L, M = 147, 80
    h = _taps(L, M)
    for u, (y, pcm, _) in _undisturbed(L, M, 64, 16, 37, W).items():
        z = _whole(stateless, L, M, 64, 16, y, STRENGTHS[u % 2])[1]
        want, S = _reference(z, h, L, M, len(pcm))
        err = np.abs(pcm.astype(np.float64) - np.clip(want, -32768, 32767))
        print("utterance %d, %d outputs: largest error / bar %.3g" % (u, len(pcm), ((err - 0.5) / _bar(h, L, S).clip(1e-300)).max()))
        assert (err <= 0.5 + _bar(h, L, S)).all(), (u, err.max())


def test_moves_and_a_trip_through_bytes_change_nothing(stateless):
    L, M = 147, 80
    plain = _undisturbed(L, M, 64, 16, 37, W)
    moved = _service(L, M, 64, 16, 37, W, compact_at=1, suspend_at=2)
    for u in plain:
        assert np.array_equal(plain[u][0], moved[u][0]) and np.array_equal(plain[u][1], moved[u][1]), u
    # with its denoise state but without its tail utterance 0 differs within the first H L / M + 1 outputs after the seam only
    # (suspended a step later, behind 79 samples: 16 cleaned samples are out by then, more than the H = 8 of the tail)
    cut = _service(L, M, 64, 16, 37, W, suspend_at=3, drop=("tail",))
    seam = plain[0][2][3][0]                                  # the first output of its fourth piece (step 3)
    H = rate_tail_len(L, (len(_taps(L, M)) - 1) // 2)
    differs = np.flatnonzero(plain[0][1] != cut[0][1])
    assert [m0 for m0, _ in cut[0][2]] == [m0 for m0, _ in plain[0][2]]
    assert len(differs) > 0 and seam <= differs.min() and differs.max() < seam + H * L // M + 1, (seam, differs)
    # without its denoise state it goes on as a stream of its own, numbered from 0, whether the tail came along or not
    for drop in (("denoise",), ("denoise", "tail")):
        cut = _service(L, M, 64, 16, 37, W, suspend_at=2, drop=drop)
        done, before = 37 + 5, sum(n for _, n in cut[0][2][:2])
        assert np.array_equal(cut[0][0], plain[0][0]) and np.array_equal(cut[0][1][:before], plain[0][1][:before])
        assert cut[0][2][2][0] == 0
        assert np.array_equal(cut[0][1][before:], _whole(stateless, L, M, 64, 16, plain[0][0][done:], STRENGTHS[0])[0])


def test_the_shipping_geometry_bit_for_bit(stateless):
    """800 / 200 at 147 / 80: utterances of n_fft + 5 hop + 37 and of 5 hop samples, a window of 512 that the second step of 300 wraps."""
    L, M, n_fft, hop, lengths = 147, 80, 800, 200, [1837, 1000]
    x = _setup()[2]
    st = _stream(L, M, n_fft, hop, 512)
    feats = [torch.cat([x[u]] * (n // x[u].size(1) + 1), dim=1)[:, :n].contiguous() for u, n in enumerate(lengths)]
    who = {st.submit(f, uid=u): u for u, f in enumerate(feats)}
    got = {u: ([], []) for u in who.values()}
    while st.busy():
        out = st.step_async(300).result()
        for h, (y, pcm) in out.items():
            got[who[h]][0].append(y.copy())
            got[who[h]][1].append(pcm.copy())
    st.close()
    for u, (y, pcm) in got.items():
        y, pcm = np.concatenate(y), np.concatenate(pcm)
        want = _whole(stateless, L, M, n_fft, hop, y, STRENGTHS[0])[0]
        assert len(y) == lengths[u] and np.array_equal(pcm, want), (u, np.flatnonzero(pcm != want)[:8])


def test_canaries_and_refusals():
    case, m, x, w, t = _setup()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], COLUMNS)
    y, _ = e.slotsPinned(COLUMNS * 40)
    buf = torch.full((8 + 1200,), CANARY, dtype=torch.int16).pin_memory()
    pageable = torch.zeros(1200, dtype=torch.int16)
    e.slotsBegin(W)
    assert e.slotsDenoiseRateCapacity(8) == -1
    e.slotsSetDenoiseRate(None)                                # off already
    e.setResampler(0, 2, 1, _taps(2, 1))
    with pytest.raises(ValueError):
        e.slotsSetDenoiseRate(0, 0.1)                          # no denoiser set
    e.setDenoiser(64, 16, _bias(64))
    with pytest.raises(ValueError):
        e.slotsSetDenoiseRate(1, 0.1)                          # no resampler in that slot
    for on, off in ((lambda: e.slotsSetDelivery(0), lambda: e.slotsSetDelivery(None)), (lambda: e.slotsSetDenoise(0.1), lambda: e.slotsSetDenoise(None))):
        on()
        with pytest.raises(ValueError):
            e.slotsSetDenoiseRate(0, 0.1)                      # each of the single modes excludes it ...
        e.slotsSetDenoiseRate(None)                            # (... and is not its to turn off)
        assert e.slotsTailLen() >= 0 or e.slotsDenoiseStateBytes() > 0
        off()
    with pytest.raises(ValueError):
        e.slotsStepRaggedDenoiseRate(8, y, buf[8:])            # the mode is not on
    e.slotsSetDenoiseRate(0, 0.1)
    assert e.slotsDenoiseStateBytes() == 2 * 64 + 4 * 48 + 16 and e.slotsTailLen() == rate_tail_len(2, (len(_taps(2, 1)) - 1) // 2)
    assert e.slotsDenoiseRateCapacity(37) >= 2 * COLUMNS * 40 and e.slotsRateCapacity(37) == -1 and e.slotsDenoiseCapacity(37) == -1
    for col, n in ((0, 150), (7, 3), (19, 61)):
        e.slotStart(col, x[col % 6][:, :n], col)
    for refused in (lambda: e.slotsSetDelivery(0), lambda: e.slotsSetDelivery(None), lambda: e.slotsSetDenoise(0.1), lambda: e.slotsSetDenoise(None),
                    lambda: e.setDenoiser(64, 8, _bias(64)), lambda: e.setResampler(0, 1, 3, _taps(1, 3)),
                    lambda: e.slotsStepRagged(8, y, None), lambda: e.slotsStepRaggedRate(8, y, buf[8:]), lambda: e.slotsStepRaggedDenoise(8, y, buf[8:])):
        with pytest.raises(ValueError):
            refused()
    assert not e.slotsStep(8)
    for pcm in (buf[8:8 + 5], None, pageable):                 # too little capacity (column 7 delivers its 3 samples as 6 outputs), no PCM, not pinned
        with pytest.raises((ValueError, AssertionError)):
            e.slotsStepRaggedDenoiseRate(37, y, pcm)
    assert (buf == CANARY).all()
    for _ in range(3):
        total, pcm_total, pieces, rate, ticket = e.slotsStepRaggedDenoiseRate(37, y, buf[8:])
        e.slotsWait(ticket)
        keep = np.ones(len(buf), dtype=bool)
        for r in rate:
            assert r["offset"] % 8 == 0
            keep[8 + r["offset"]:8 + r["offset"] + r["count"]] = False
        assert len(rate) == len(pieces) > 0 and pcm_total == max(r["offset"] + r["count"] for r in rate if r["count"]) > 0
        assert (buf.numpy()[keep] == CANARY).all() and not (buf.numpy()[~keep] == CANARY).all()      # gaps, front and back survive
        buf.fill_(CANARY)
    e.slotsSetDenoiseRate(None)
    assert e.slotsDenoiseStateBytes() == -1 and e.slotsTailLen() == -1 and e.slotsStep(8)
    e.close()
