"""GPU tests of sample-rate conversion: nvw_resample against a float64 evaluation of its definition within the
worst-case fp32 bound of the dot product (derived, not measured), saturation, ranges and streams bit for bit the whole call, the
refusals, and analyse(rate=) as resample followed by analyse."""
import numpy as np
import pytest
import torch

from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import RESAMPLE_REQ, WavenetEngine
from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine, resample_taps

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RATIOS = [(1, 2), (2, 1), (2, 3), (7, 5), (160, 147)]
DTYPES = {16: torch.int16, 32: torch.float32}


@pytest.fixture(scope="module")
def engine():
    e = WavenetEngine(64, 256, 256, 3, 4, 1, 64, precision=32)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model():
    R, S, A, L = 64, 256, 256, 3
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: (0.1 * torch.randn(*s, generator=g)).cuda()
    m = NVWaveNetEngine(embedding_prev=mk(A, R), embedding_curr=mk(A, R), conv_out_weight=mk(A, S, 1), conv_end_weight=mk(A, A, 1),
                        dilate_weights=[mk(2 * R, R, 2) for _ in range(L)], dilate_biases=[mk(2 * R) for _ in range(L)], max_dilation=4,
                        res_weights=[mk(R, R, 1) for _ in range(L - 1)], res_biases=[mk(R) for _ in range(L - 1)],
                        skip_weights=[mk(S, R, 1) for _ in range(L)], skip_biases=[mk(S) for _ in range(L)], use_embed_tanh=False, precision=16)
    yield m
    m.close()


def _reference(x, h, L, M, count):
    """(out, sum |h| |x|) of outputs 0 .. count - 1 of the complete stream x in float64: the definition, term by term."""
    c = (len(h) - 1) // 2
    m = np.arange(count)[:, None]
    i = -((c - m * M) // L) + np.arange(2 * c // L + 1)[None, :]          # from ceil((m M - c) / L) on, every input that can count
    k = c + m * M - i * L
    ok = (k >= 0) & (k < len(h)) & (i >= 0) & (i < len(x))
    terms = np.where(ok, x.astype(np.float64)[np.clip(i, 0, len(x) - 1)] * h[np.clip(k, 0, len(h) - 1)], 0.0)
    return terms.sum(1), np.abs(terms).sum(1)


def _bar(h, L, S):
    """The worst case of an fp32 dot product of K = floor(2 c / L) + 1 terms against the exact one: every product and every sum
    rounds once (K operations on partial sums that sum |h| |x| bounds), the table's rounding to fp32 is one more per term and the
    inputs are exact in fp32, so |error| <= gamma(K + 2) sum |h| |x| with gamma(n) = n u / (1 - n u), u = 2^-24."""
    K = (len(h) - 1) // L + 1
    return (K + 2) * U / (1 - (K + 2) * U) * S


def _guarded(count, bits):
    return torch.full((count + 4,), 777, dtype=DTYPES[bits], device="cuda")


@pytest.mark.parametrize("out_bits", [16, 32])
@pytest.mark.parametrize("in_bits", [16, 32])
@pytest.mark.parametrize("L, M", RATIOS)
def test_a_ragged_call_against_the_float64_definition(engine, L, M, in_bits, out_bits):
    _, _, h = resample_taps(M, L, zeros=4)
    engine.setResampler(1, L, M, h)
    Q = L * next(q for q in range(1, 17) if L * q >= 16 and q * M >= 4)
    counts = [1, 16 * Q - 1, 16 * Q, 16 * Q + 1, 64 * Q + 3, -(-3 * L // M)]      # (the last: three or four inputs, shorter than the filter)
    rng = np.random.RandomState(L * 1000 + M)
    xs, outs = [], []
    for cnt in counts:
        n = -(-cnt * M // L)                                                       # the fewest inputs with cnt outputs
        assert engine.resampleCount(1, n) == -(-n * L // M) >= cnt
        xs.append(rng.randint(-32768, 32768, n).astype(np.int16))
        outs.append(_guarded(cnt, out_bits))
    engine.resample(1, [(torch.from_numpy(x).cuda().to(DTYPES[in_bits]), 0, True, o[:cnt], 0) for x, o, cnt in zip(xs, outs, counts)])
    engine.synchronize()
    for x, o, cnt in zip(xs, outs, counts):
        got = o.double().cpu().numpy()
        assert (got[cnt:] == 777).all(), "written past its end"
        want, S = _reference(x, h, L, M, cnt)
        bar = _bar(h, L, S)
        err = np.abs(got[:cnt] - (np.clip(want, -32768, 32767) if out_bits == 16 else want))
        slack = 0.5 if out_bits == 16 else 0.0
        print("%d / %d, %d outputs, in %d out %d: largest error / bar %.3g" % (L, M, cnt, in_bits, out_bits, ((err - slack) / bar.clip(1e-300)).max()))
        assert (err <= slack + bar).all(), (cnt, err.max(), bar.max())


def test_int16_outputs_saturate(engine):
    _, _, h = resample_taps(1, 2, zeros=4)
    engine.setResampler(1, 2, 1, h)
    x = (32767 * np.where(np.arange(400) // 8 % 2, -1, 1)).astype(np.int16)      # a full-scale square wave: the filter overshoots
    out = _guarded(800, 16)
    engine.resample(1, [(torch.from_numpy(x).cuda(), 0, True, out[:800], 0)])
    engine.synchronize()
    got = out.cpu().numpy()
    want, S = _reference(x, h, 2, 1, 800)
    bar = _bar(h, 2, S)
    over, under = want > 32767 + bar, want < -32768 - bar
    assert over.sum() > 10 and under.sum() > 10 and (got[:800][over] == 32767).all() and (got[:800][under] == -32768).all()
    assert (got[800:] == 777).all()


@pytest.mark.parametrize("L, M", [(2, 3), (160, 147)])
def test_ranges_and_streams_are_the_whole_call_bit_for_bit(engine, model, L, M):
    _, _, h = resample_taps(M, L, zeros=4)
    c = (len(h) - 1) // 2
    engine.setResampler(1, L, M, h)
    x = torch.from_numpy(np.random.RandomState(7).randint(-20000, 20000, 1500).astype(np.int16)).cuda()
    total = -(-1500 * L // M)
    for bits in (16, 32):
        whole = _guarded(total, bits)
        engine.resample(1, [(x, 0, True, whole[:total], 0)])
        for m0, cnt in ((total // 3, 1), (total // 2 + 1, 333), (total - 40, 40)):
            first, end = -((c - m0 * M) // L), ((m0 + cnt - 1) * M + c) // L + 1      # the inputs that the range needs
            assert first > 0
            part = _guarded(cnt, bits)
            engine.resample(1, [(x[first:min(end, 1500)], first, end >= 1500, part[:cnt], m0)])
            assert torch.equal(part[:cnt], whole[m0:m0 + cnt]) and (part[cnt:] == 777).all(), (bits, m0, cnt)
        assert (whole[total:] == 777).all()
    whole = model.resample(x[None], M, L, taps=h)
    assert whole.shape == (1, total) and whole.dtype == torch.int16
    for chunk in (1, 37, 1000):
        s = model.resample_stream(M, L, taps=h)
        got = torch.cat([s.feed(x[None, k:k + chunk], last=k + chunk >= 1500) for k in range(0, 1500, chunk)], dim=1)
        assert torch.equal(got, whole), chunk


def test_what_the_entries_refuse_and_that_nothing_is_written():
    e = WavenetEngine(64, 256, 256, 3, 4, 1, 64, precision=32)
    _, _, h = resample_taps(3, 2, zeros=4)                                          # 2 / 3: c = 12, output 60 needs inputs 84 .. 96
    x = torch.ones(200, dtype=torch.int16, device="cuda")
    out = _guarded(100, 32)
    host = np.zeros(400, dtype=np.float32)

    def call(requests=1, slot=0, **fields):
        r = np.zeros(max(requests, 1), dtype=RESAMPLE_REQ)
        r[:] = (x.data_ptr(), 16, 0, 200, 1, out.data_ptr(), 32, 0, 100)
        for k, v in fields.items():
            r[k] = v
        return lib.nvw_resample(e._h, slot, r.ctypes.data, requests, None)

    assert e.resampleCount(0, 200) == 0 and call() == 0                              # the slot is unset
    for slot, up, down, taps, n in ((0, 4, 6, h, len(h)), (0, 0, 3, h, len(h)), (0, 2, 641, h, len(h)), (0, 2, 3, h, len(h) - 1), (0, 2, 3, h, 0),
                                    (0, 2, 3, None, 25), (4, 2, 3, h, len(h)), (0, 1, 640, h, len(h))):      # (the last: 2.5 MB of LDS)
        assert lib.nvw_set_resampler(e._h, slot, up, down, None if taps is None else taps.ctypes.data, n) == 0, (slot, up, down, n)
    e.setResampler(0, 2, 3, h)
    assert e.resampleCount(0, 200) == 134 and e.resampleCount(1, 200) == 0
    assert lib.nvw_set_resampler(e._h, 0, 4, 6, h.ctypes.data, len(h)) == 0 and e.resampleCount(0, 200) == 134      # refused: the taps stay
    for kw in (dict(slot=1), dict(slot=4), dict(requests=0), dict(requests=65536), {"in": host.ctypes.data}, dict(out=host.ctypes.data),
               dict(in_type=8), dict(out_type=64), dict(n_in=0), dict(count=0), dict(first=-1), dict(m0=-1),
               dict(first=85, m0=60, count=10),                                      # a needed input (84) below first
               dict(n_in=96, last=0, m0=60, count=1)):                               # a needed input (96) past the buffer, which is not the end
        assert call(**kw) == 0, kw
    e.synchronize()
    assert (out == 777).all()
    assert call(n_in=97, last=0, m0=60, count=1) == 1 and call() == 1 and call(requests=2) == 2
    e.synchronize()
    want, _ = _reference(np.ones(200), h, 2, 3, 100)
    assert np.abs(out[:100].double().cpu().numpy() - want).max() < 1e-3 and (out[100:] == 777).all()
    e.close()


def test_analyse_at_another_rate_is_resample_then_analyse(model):
    n_fft, hop, C = 64, 16, 16
    basis = torch.rand(C, n_fft // 2 + 1, generator=torch.Generator().manual_seed(3))
    pcm48 = (8000 * torch.randn(2, 700, generator=torch.Generator().manual_seed(4))).clamp(-32768, 32767).to(torch.int16).cuda()
    model.set_analysis(n_fft, hop, basis)
    plain = model.analyse(pcm48, lengths=[700, 451])
    model.set_analysis(n_fft, hop, basis, sample_rate=24000)
    for got, want in zip(model.analyse(pcm48, lengths=[700, 451]), plain):          # no rate: as before
        assert torch.equal(got, want)
    for got, want in zip(model.analyse(pcm48, lengths=[700, 451], rate=24000), plain):
        assert torch.equal(got, want)
    pcm24 = model.resample(pcm48, 48000, 24000, lengths=[700, 451])
    assert pcm24.shape == (2, 350) and not pcm24[1, 226:].any() and pcm24[1, :226].any()
    for got, want in zip(model.analyse(pcm48, lengths=[700, 451], rate=48000), model.analyse(pcm24, lengths=[350, 226])):
        assert torch.equal(got, want)
