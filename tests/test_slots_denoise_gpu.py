"""GPU tests of slot mode's denoised delivery (`-m gpu`): the session of tests/test_slots_rate_gpu.py -- the smallest
built model (R = 32, 8 layers), a window of 40 samples that every run wraps, 20 columns, six utterances in columns 16 .. 19 behind
16 one-sample fillers, two joining five samples apart: 152 samples, one of n_fft / 2 or fewer (delivered unchanged), one of n_fft / 2
+ 1, one ending on a hop boundary and two others; the odd ones at strength 1, the even ones at the stream's 0.1.  Per utterance the
denoised pieces, concatenated, are held to nvw_denoise of its whole model-rate PCM bit for bit, and to the float64 definition
within test_denoise_gpu's bar for int16 outputs."""
import functools

import numpy as np
import pytest
import torch

from nv_wavenet_amd import WavenetEngine
from nv_wavenet_amd.slots import SlotState, SlotStream
from oracle import oracle as O
from test_denoise_gpu import _bias, _reference
from test_slots_gpu import _engine
from test_slots_rate_gpu import CANARY, COLUMNS, FILLERS, N, W, _setup

pytestmark = pytest.mark.gpu

LENGTHS = [N, 20, 33, 96, 77, 101]            # n_fft = 64: 20 <= n_fft / 2 < 33; 96 is a multiple of both hops
STRENGTHS = [0.1, 1.0]                        # of the even and the odd utterances
# n_fft, hop, step, window: 37 and 24 cross the wrap of the window of 40; at hop 8 a 37-sample step gives a piece 4 - 5 frames; the
# last two give a piece more than 16 (at 64 / 4 a finishing 24-sample sub-range has exactly the 16 that a launch takes)
RUNS = [(n_fft, hop, step, W) for n_fft, hop in ((64, 16), (64, 8)) for step in (1, 37, 24)] + [(64, 8, 150, 160), (64, 4, 37, W)]


def _stream(n_fft, hop, window):
    case, m, x, w, t = _setup()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], COLUMNS)
    e.setDenoiser(n_fft, hop, _bias(n_fft))
    return SlotStream(e, window, owns_engine=True, denoise=STRENGTHS[0])


def _service(n_fft, hop, step, window, compact_at=None, suspend_at=None, keep_state=True):
    """uid -> (samples, PCM, [(first output, outputs) of every piece]) of the six utterances; suspend_at: utterance 0 goes through
    bytes to a second stream before that step."""
    x = _setup()[2]
    st, st2 = _stream(n_fft, hop, window), (_stream(n_fft, hop, window) if suspend_at is not None else None)
    who = {}
    got = {u: ([], [], []) for u in range(6)}

    def submit(u):
        who[(id(st), st.submit(x[u][:, :LENGTHS[u]], uid=u, denoise_strength=STRENGTHS[1] if u % 2 else None))] = u

    for f in range(FILLERS):
        st.submit(x[0][:, :1], uid=100 + f)
    for u in range(4):
        submit(u)
    for it, size in enumerate([step, 5] + [step] * (N + 8)):      # utterances 4 and 5 join 5 samples apart, in columns the fillers left
        if it in (1, 2):
            submit(3 + it)
        if it == compact_at:
            assert st.compact() >= 2
        if it == suspend_at:
            state = st.suspend(next(h for (s, h), u in who.items() if u == 0))
            assert 0 < state.done < N and state.denoise is not None
            state = SlotState.from_bytes(state.to_bytes(), state.source)
            if not keep_state:
                state.denoise = None
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
    return {u: (np.concatenate(y), np.concatenate(p), t0s) for u, (y, p, t0s) in got.items()}


_undisturbed = functools.lru_cache(maxsize=None)(_service)


@pytest.fixture(scope="module")
def cleaner():
    e = WavenetEngine(64, 256, 256, 3, 4, 1, 64, precision=32)
    yield e
    e.close()


def _whole(cleaner, n_fft, hop, y, strength):
    """nvw_denoise of an utterance's whole model-rate PCM, last = 1 (a stream it refuses comes unchanged); and that PCM"""
    x = O.mulaw_pcm_table(256)[y]
    if len(x) <= n_fft // 2:
        return x, x
    out = torch.zeros(len(x), dtype=torch.int16, device="cuda")
    cleaner.setDenoiser(n_fft, hop, _bias(n_fft))
    cleaner.denoise([(torch.from_numpy(x).cuda(), 0, True, out, 0, strength)])
    cleaner.synchronize()
    return out.cpu().numpy(), x


@pytest.mark.parametrize("n_fft, hop, step, window", RUNS)
def test_pieces_concatenated_are_the_whole_call_bit_for_bit(cleaner, n_fft, hop, step, window):
    for u, (y, pcm, t0s) in _undisturbed(n_fft, hop, step, window).items():
        assert len(y) == LENGTHS[u]
        want, x = _whole(cleaner, n_fft, hop, y, STRENGTHS[u % 2])
        assert [t0 for t0, _ in t0s] == list(np.cumsum([0] + [n for _, n in t0s[:-1]])), (u, t0s)      # contiguous from output 0
        assert len(pcm) == LENGTHS[u] and np.array_equal(pcm, want), (u, LENGTHS[u], np.flatnonzero(pcm != want)[:8])
        assert LENGTHS[u] <= n_fft // 2 or np.abs(pcm.astype(np.int64) - x).max() > 100                # the subtraction moves the signal


@pytest.mark.parametrize("n_fft, hop", [(64, 16), (64, 8)])
def test_against_the_float64_definition(n_fft, hop):
    table = O.mulaw_pcm_table(256)
    for u, (y, pcm, _) in _undisturbed(n_fft, hop, 37, W).items():
        if LENGTHS[u] <= n_fft // 2:
            continue
        want = _reference(torch.from_numpy(table[y]), n_fft, hop, _bias(n_fft), STRENGTHS[u % 2]).clamp(-32768, 32767).numpy()
        err = np.abs(pcm.astype(np.float64) - want).max()
        print("%d / %d, utterance %d, %d outputs, strength %g: largest error %.4f" % (n_fft, hop, u, len(pcm), STRENGTHS[u % 2], err))
        assert err <= 0.75, (u, err)


def test_the_shipping_geometry_bit_for_bit(cleaner):
    """800 / 200: five bin tiles and eight sample tiles per wave; utterances of n_fft + 5 hop + 37 and of 5 hop samples, a window of
    512 that the second step of 300 wraps."""
    n_fft, hop, lengths = 800, 200, [800 + 5 * 200 + 37, 1000]
    x = _setup()[2]
    st = _stream(n_fft, hop, 512)
    feats = [torch.cat([x[u]] * (n // N + 1), dim=1)[:, :n].contiguous() for u, n in enumerate(lengths)]
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
        want, _ = _whole(cleaner, n_fft, hop, y, STRENGTHS[0])
        assert len(y) == lengths[u] and np.array_equal(pcm, want), (u, np.flatnonzero(pcm != want)[:8])


def test_moves_and_a_trip_through_bytes_change_nothing(cleaner):
    plain = _undisturbed(64, 16, 37, W)
    moved = _service(64, 16, 37, W, compact_at=1, suspend_at=2)
    for u in plain:
        assert np.array_equal(plain[u][0], moved[u][0]) and np.array_equal(plain[u][1], moved[u][1]) and plain[u][2] == moved[u][2], u
    # without its state utterance 0 goes on as a stream of its own: the outputs from the seam on are nvw_denoise of the remaining samples
    cut = _service(64, 16, 37, W, suspend_at=2, keep_state=False)
    done = 37 + 5
    before = sum(n for _, n in cut[0][2][:2])
    assert np.array_equal(cut[0][0], plain[0][0]) and np.array_equal(cut[0][1][:before], plain[0][1][:before])
    assert cut[0][2][2][0] == 0 and len(cut[0][1]) == before + N - done
    assert np.array_equal(cut[0][1][before:], _whole(cleaner, 64, 16, plain[0][0][done:], STRENGTHS[0])[0])


def test_canaries_and_refusals():
    case, m, x, w, t = _setup()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], COLUMNS)
    y, _ = e.slotsPinned(COLUMNS * 40)
    buf = torch.full((8 + 600,), CANARY, dtype=torch.int16).pin_memory()
    pageable = torch.zeros(600, dtype=torch.int16)
    assert e.slotsDenoiseStateBytes() == -1 and e.slotsDenoiseCapacity(8) == -1
    e.slotsBegin(W)
    with pytest.raises(ValueError):
        e.slotsSetDenoise(0.1)                                 # no denoiser set
    with pytest.raises(ValueError):
        e.slotsStepRaggedDenoise(8, y, buf[8:])                # denoised delivery not on
    e.setDenoiser(64, 16, _bias(64))
    e.setResampler(0, 2, 1, np.ones(5))
    e.slotsSetDelivery(0)
    with pytest.raises(ValueError):
        e.slotsSetDenoise(0.1)                                 # rate delivery on
    e.slotsSetDelivery(None)
    with pytest.raises(ValueError):
        e.slotsSetDenoise(-1.0)
    e.slotsSetDenoise(0.1)
    assert e.slotsDenoiseStateBytes() == 2 * 64 + 4 * 48 + 16 and e.slotsDenoiseCapacity(37) >= COLUMNS * 40
    for col, n in ((0, 150), (7, 3), (19, 61)):
        e.slotStart(col, x[col % 6][:, :n], col)
    with pytest.raises(ValueError):
        e.slotsSetDelivery(0)                                  # each refuses while the other is on
    with pytest.raises(ValueError):
        e.setDenoiser(64, 8, _bias(64))                        # the geometry a session delivers through
    with pytest.raises(ValueError):
        e.slotsStepRagged(8, y, None)                          # a plain step would leave a hole in every stream
    with pytest.raises(ValueError):
        e.slotsStepRaggedRate(8, y, buf[8:])
    assert not e.slotsStep(8)
    for pcm in (buf[8:8 + 2], None, pageable):                 # too little capacity (column 7 delivers its 3 samples unchanged), no PCM, not pinned
        with pytest.raises((ValueError, AssertionError)):
            e.slotsStepRaggedDenoise(37, y, pcm)
    with pytest.raises(ValueError):
        e.slotDenoiseStateGet(3)                               # no utterance
    assert (buf == CANARY).all()
    for _ in range(3):
        total, pcm_total, pieces, rate, ticket = e.slotsStepRaggedDenoise(37, y, buf[8:])
        e.slotsWait(ticket)
        keep = np.ones(len(buf), dtype=bool)
        for r in rate:
            assert r["offset"] % 8 == 0
            keep[8 + r["offset"]:8 + r["offset"] + r["count"]] = False
        assert len(rate) == len(pieces) > 0 and pcm_total == max(r["offset"] + r["count"] for r in rate if r["count"]) > 0
        assert (buf.numpy()[keep] == CANARY).all() and not (buf.numpy()[~keep] == CANARY).all()      # gaps, front and back survive
        buf.fill_(CANARY)
    e.slotsSetDenoise(None)
    assert e.slotsDenoiseStateBytes() == -1 and e.slotsStep(8)
    e.close()
