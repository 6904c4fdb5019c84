"""GPU tests of slot mode's delivery at the caller's rate (`-m gpu`): the smallest built model (R = 32, 8 layers), a
window of 40 samples (5 x the largest dilation) that every run wraps, 20 columns, six utterances of ragged lengths -- one shorter
than the history H, one shorter than the filter, two that join at later steps five samples apart, all behind 16 one-sample fillers
so that they run in columns 16 .. 19 and compact() has moves to make.  Per utterance the rate pieces, concatenated, are held to
nvw_resample of its whole model-rate PCM bit for bit, and for one ratio to the float64 definition within test_resample_gpu's bound."""
import functools

import numpy as np
import pytest
import torch

from nv_wavenet_amd import WavenetEngine
from nv_wavenet_amd.nv_wavenet import resample_taps
from nv_wavenet_amd.slots import SlotState, SlotStream, rate_tail_len
from oracle import oracle as O
from test_resample_gpu import _bar, _reference
from test_slots_gpu import FAMILIES, _engine, _synth

pytestmark = pytest.mark.gpu

RATIOS = [(2, 1), (1, 3), (147, 80)]
STEPS = [1, 37, 24]            # 37 and 24: the second step's rows (37 .. 73, 24 .. 47) cross the wrap of the window of 40
W, COLUMNS, N, FILLERS = 40, 20, 152, 16
CANARY = -7


@functools.lru_cache(maxsize=None)
def _setup():
    case, m, x, w, _, t = _synth("rate_C1_R32", FAMILIES["C1_R32"][0]._replace(N=N, B=6), 16, 611)
    return case, m, torch.from_numpy(x).cuda(), w, t


def _taps(L, M):
    return resample_taps(M, L, zeros=4)[2]


def _lengths(L, M):
    c = (len(_taps(L, M)) - 1) // 2
    return [N, max(1, rate_tail_len(L, c) // 2), 2 * c // L, 77, 101, 58]      # the filter spans 2 c // L + 1 inputs


def _stream(L, M, deliver=True):
    case, m, x, w, t = _setup()
    e = _engine(case, t, 16, "wg", w, m["cond_b"], COLUMNS)
    if deliver:
        e.setResampler(0, L, M, _taps(L, M))
    return SlotStream(e, W, owns_engine=True, deliver=0 if deliver else None)


def _service(L, M, step, deliver=True, compact_at=None, suspend_at=None, keep_tail=True):
    """uid -> (samples, PCM, [(first output, outputs) of every piece]) of the six utterances; suspend_at: utterance 0 goes through
    bytes to a second stream before that step."""
    x, lengths = _setup()[2], _lengths(L, M)
    st, st2 = _stream(L, M, deliver), (_stream(L, M, deliver) if suspend_at is not None else None)
    who = {}
    got = {u: ([], [], []) for u in range(6)}

    def submit(u):
        who[(id(st), st.submit(x[u][:, :lengths[u]], uid=u))] = u

    for f in range(FILLERS):
        st.submit(x[0][:, :1], uid=100 + f)
    for u in range(4):
        submit(u)
    for it, size in enumerate([step, 5] + [step] * (N + 8)):      # utterances 4 and 5 join 5 samples apart, in columns the fillers left
        if it in (1, 2):
            submit(3 + it)
        if it == compact_at:
            assert st.compact() >= 2                            # utterances 0 and 3 at the least leave columns 16 and 19
        if it == suspend_at:
            handle = next(h for (s, h), u in who.items() if u == 0)
            state = st.suspend(handle)
            assert 0 < state.done < N and (state.tail is not None) == deliver
            state = SlotState.from_bytes(state.to_bytes(), state.source)
            if not keep_tail:
                state.tail = None
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
def converter():
    e = WavenetEngine(64, 256, 256, 3, 4, 1, 64, precision=32)
    yield e
    e.close()


def _whole(converter, L, M, y):
    """nvw_resample of the whole utterance's model-rate PCM, last = 1; and that PCM"""
    x = O.mulaw_pcm_table(256)[y]
    out = torch.zeros(-(-len(x) * L // M), dtype=torch.int16, device="cuda")
    converter.setResampler(1, L, M, _taps(L, M))
    converter.resample(1, [(torch.from_numpy(x).cuda(), 0, True, out, 0)])
    converter.synchronize()
    return out.cpu().numpy(), x


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("L, M", RATIOS)
def test_pieces_concatenated_are_the_whole_call_bit_for_bit(converter, L, M, step):
    lengths = _lengths(L, M)
    for u, (y, pcm, m0s) in _undisturbed(L, M, step).items():
        assert len(y) == lengths[u]
        want, _ = _whole(converter, L, M, y)
        assert [m0 for m0, _ in m0s] == list(np.cumsum([0] + [n for _, n in m0s[:-1]])), (u, m0s)      # contiguous from output 0
        assert len(pcm) == -(-lengths[u] * L // M) and np.array_equal(pcm, want), (u, lengths[u])


def test_against_the_float64_definition():
    L, M = 147, 80
    h = _taps(L, M)
    table = O.mulaw_pcm_table(256)
    for u, (y, pcm, _) in _undisturbed(L, M, 37).items():
        want, S = _reference(table[y], h, L, M, len(pcm))
        err = np.abs(pcm.astype(np.float64) - np.clip(want, -32768, 32767))
        print("utterance %d, %d outputs: largest error / bar %.3g" % (u, len(pcm), ((err - 0.5) / _bar(h, L, S).clip(1e-300)).max()))
        assert (err <= 0.5 + _bar(h, L, S)).all(), (u, err.max())


@pytest.mark.parametrize("L, M", RATIOS)
def test_moves_and_a_trip_through_bytes_change_nothing(L, M):
    plain = _undisturbed(L, M, 37)
    moved = _service(L, M, 37, compact_at=1, suspend_at=2)
    for u in plain:
        assert np.array_equal(plain[u][0], moved[u][0]) and np.array_equal(plain[u][1], moved[u][1]), u
    # without its history utterance 0 differs within the first H L / M + 1 outputs after the seam, and nowhere else
    cut = _service(L, M, 37, suspend_at=2, keep_tail=False)
    seam = plain[0][2][2][0]                                  # the first output of its third piece (step 2)
    H = rate_tail_len(L, (len(_taps(L, M)) - 1) // 2)
    differs = np.flatnonzero(plain[0][1] != cut[0][1])
    assert [m0 for m0, _ in cut[0][2]] == [m0 for m0, _ in plain[0][2]]
    assert len(differs) > 0 and seam <= differs.min() and differs.max() < seam + H * L // M + 1, (seam, differs)


def test_delivery_off_is_the_plain_stream_and_the_samples_do_not_depend_on_the_rate():
    off, on = _service(2, 1, 37, deliver=False), _undisturbed(2, 1, 37)
    table = O.mulaw_pcm_table(256)
    for u in off:
        assert np.array_equal(off[u][0], on[u][0]) and np.array_equal(off[u][1], table[off[u][0]])
        assert [f for f, _ in off[u][2]] == list(np.cumsum([0] + [n for _, n in off[u][2][:-1]]))      # pcm_first: the pieces' first samples


def test_canaries_and_refusals():
    case, m, x, w, t = _setup()
    L, M = 1, 3
    e = _engine(case, t, 16, "wg", w, m["cond_b"], COLUMNS)
    y, _ = e.slotsPinned(COLUMNS * 40)
    buf = torch.full((8 + 400,), CANARY, dtype=torch.int16).pin_memory()
    assert e.slotsTailLen() == -1 and e.slotsRateCapacity(8) == -1
    with pytest.raises(ValueError):
        e.slotsSetDelivery(0)                                  # not in slot mode
    e.slotsBegin(W)
    with pytest.raises(ValueError):
        e.slotsSetDelivery(0)                                  # a slot that is not set
    with pytest.raises(ValueError):
        e.slotsStepRaggedRate(8, y, buf[8:])                   # delivery not set
    e.setResampler(0, L, M, _taps(L, M))
    for col, n in ((0, 150), (7, 3), (19, 61)):
        e.slotStart(col, x[col % 6][:, :n], col)
    e.slotsStepRagged(37, y, None)
    with pytest.raises(ValueError):
        e.slotsSetDelivery(0)                                  # a ragged step in flight
    e.synchronize()
    e.slotsSetDelivery(0)
    H = rate_tail_len(L, (len(_taps(L, M)) - 1) // 2)
    assert e.slotsTailLen() == H and e.slotsRateCapacity(37) >= COLUMNS * 16
    assert not e.slotsStep(8) and not np.any(e.slotTailGet(0))
    with pytest.raises(ValueError):
        e.slotsStepRagged(8, y, None)                          # a plain step would leave a hole in the histories
    with pytest.raises(ValueError):
        e.slotsStepRaggedRate(37, y, buf[8:8 + 8])             # too little PCM capacity: column 0 alone has 12 or 13 outputs
    with pytest.raises(ValueError):
        e.slotTailGet(3)                                       # no utterance
    with pytest.raises(ValueError):
        e.setResampler(0, 2, 1, _taps(2, 1))                   # the slot a session delivers through
    for _ in range(3):
        total, pcm_total, pieces, rate, ticket = e.slotsStepRaggedRate(37, y, buf[8:])
        e.slotsWait(ticket)
        keep = np.ones(len(buf), dtype=bool)
        for r in rate:
            assert r["offset"] % 8 == 0
            keep[8 + r["offset"]:8 + r["offset"] + r["count"]] = False
        assert len(rate) == len(pieces) > 0 and pcm_total == max(r["offset"] + r["count"] for r in rate if r["count"]) > 0
        assert (buf.numpy()[keep] == CANARY).all() and not (buf.numpy()[~keep] == CANARY).all()      # gaps, front and back survive
        buf.fill_(CANARY)
    e.slotsSetDelivery(None)
    assert e.slotsTailLen() == -1 and e.slotsStep(8)
    e.close()
