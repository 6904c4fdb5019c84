"""GPU tests of the bias denoiser: nvw_denoise against float64 torch.stft -> gain -> torch.istft, the identity at
strength 0, streams bit for bit the whole call, and the refusals.

The bar of 0.25 PCM units is 14 x the error of an fp32 emulation of exactly this scheme against float64 (0.018 at these geometries,
lengths and strengths, measured on the CPU; torch's own fp32 FFT path: 0.008).  The rigorous worst-case bound of the two dot
products (5 - 900 units here) would hide a wrong c_k or a window off by one, so it is not the bar.  An int16 output adds its
rounding: 0.75.  Largest error measured on the GPU: see LABNOTES.md."""
import functools

import numpy as np
import pytest
import torch

from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import DENOISE_REQ, WavenetEngine
from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1024, 256), (800, 200), (64, 16), (64, 8)]
DTYPES = {16: torch.int16, 32: torch.float32}
STRENGTHS = [0.0, 0.1, 1.0]


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


def _signal(n, i, rng):
    """As tests/test_analysis_gpu.py: a 0.5 sine plus 0.2 uniform noise at full scale, rounded to int16."""
    x = 0.5 * np.sin(2 * np.pi * (0.013 + 0.02 * i) * np.arange(n) + i) + 0.2 * rng.uniform(-1, 1, n)
    return torch.from_numpy(np.round(x * 32767).astype(np.int16))


def _bias(n_fft):
    return torch.randn(n_fft // 2 + 1, generator=torch.Generator().manual_seed(n_fft), dtype=torch.float64).abs() * 2000 * n_fft ** 0.5


def _reference(x, n_fft, hop, bias, strength):
    """The definition in float64."""
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    X = torch.stft(x.double(), n_fft, hop, n_fft, w, center=True, pad_mode="reflect", return_complex=True)
    m = X.abs()
    gain = torch.where(m > 0, (1 - strength * bias[:, None] / m).clamp(min=0), torch.zeros_like(m))
    return torch.istft(X * gain, n_fft, hop, n_fft, w, center=True, length=x.numel())


@functools.lru_cache(maxsize=None)
def _case(n_fft, hop):
    """(signals, strengths, float64 references) of the ragged call of one geometry: computed once, shared by its four type cases."""
    edge = (17 - n_fft // hop) * hop                                                # where the second tile's frames begin
    lengths = [n_fft // 2 + 1, edge - 1, edge, edge + 1, 5 * hop + hop // 2 + 1, 40 * hop + 3]
    rng = np.random.RandomState(n_fft + hop)
    xs = [_signal(n, i, rng) for i, n in enumerate(lengths)]
    ss = [STRENGTHS[i % 3] for i in range(len(lengths))]
    return xs, ss, [_reference(x, n_fft, hop, _bias(n_fft), s) for x, s in zip(xs, ss)]


def _guarded(count, bits):
    return torch.full((count + 4,), 777, dtype=DTYPES[bits], device="cuda")


@pytest.mark.parametrize("out_bits", [16, 32])
@pytest.mark.parametrize("in_bits", [16, 32])
@pytest.mark.parametrize("n_fft, hop", GEOMETRIES)
def test_a_ragged_call_against_float64(engine, n_fft, hop, in_bits, out_bits):
    xs, ss, refs = _case(n_fft, hop)
    engine.setDenoiser(n_fft, hop, _bias(n_fft))
    outs = [_guarded(x.numel(), out_bits) for x in xs]
    engine.denoise([(x.cuda().to(DTYPES[in_bits]), 0, True, o[2:-2], 0, s) for x, o, s in zip(xs, outs, ss)])
    engine.synchronize()
    bar = 0.25 if out_bits == 32 else 0.75
    for x, o, s, ref in zip(xs, outs, ss, refs):
        got = o.double().cpu()
        assert (got[:2] == 777).all() and (got[-2:] == 777).all(), "written outside its range"
        assert s < 1 or (ref - x.double()).abs().max() > 1000                       # the subtraction moves the signal by thousands of units
        err = (got[2:-2] - ref.clamp(-32768, 32767)).abs().max().item()
        print("%d / %d, n %d, strength %g, in %d out %d: largest error %.4f" % (n_fft, hop, x.numel(), s, in_bits, out_bits, err))
        assert err <= bar, (x.numel(), s, err)


def test_strength_zero_is_the_identity_on_int16(model):
    model.set_denoiser(1024, 256, _bias(1024))
    rng = np.random.RandomState(3)
    pcm = torch.stack([_signal(40 * 256 + 3, i, rng) for i in range(3)]).cuda()
    lengths = [40 * 256 + 3, 513, 13 * 256]
    got = model.denoise(pcm, lengths=lengths, strength=0.0)
    assert got.dtype == torch.int16
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, :n], pcm[b, :n]) and not got[b, n:].any(), b


@pytest.mark.parametrize("n_fft, hop", [(1024, 256), (64, 8)])
def test_a_stream_in_chunks_is_the_whole_call_bit_for_bit(model, n_fft, hop):
    model.set_denoiser(n_fft, hop, _bias(n_fft))
    e = model._denoiser()[0]
    n = 40 * hop + 3
    x = torch.stack([_signal(n, i, np.random.RandomState(i)) for i in range(2)]).cuda()
    chunks = [1, hop - 1, n_fft, 3 * n_fft + 5]
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + chunks[(len(cuts) - 1) % 4]))
    for k in cuts[1:-1]:                                                            # the outputs whose every covering frame lies below k
        assert e.denoiseReady(k) == (max(0, ((k - n_fft // 2) // hop + 1) * hop - n_fft // 2) if k > n_fft // 2 else 0), k
    assert e.denoiseReady(n, True) == n and e.denoiseReady(n_fft // 2, True) == 0
    for dtype in (torch.int16, torch.float32):
        whole = model.denoise(x, strength=[0.1, 1.0], out_dtype=dtype)
        s = model.denoise_stream(batch=2, strength=[0.1, 1.0], out_dtype=dtype)
        got = torch.cat([s.feed(x[:, a:b], last=b == n) for a, b in zip(cuts, cuts[1:])], dim=1)
        assert torch.equal(got, whole), dtype


def test_what_the_entries_refuse_and_that_nothing_is_written():
    e = WavenetEngine(64, 256, 256, 3, 4, 1, 64, precision=32)
    x = torch.ones(200, dtype=torch.int16, device="cuda")
    out = _guarded(100, 32)
    host = np.zeros(400, dtype=np.float32)
    bias = np.ones(1025, dtype=np.float32)
    negative = -bias

    def call(requests=1, **fields):
        r = np.zeros(max(requests, 1), dtype=DENOISE_REQ)
        r[:] = (x.data_ptr(), 16, 0, 200, 1, out[2:].data_ptr(), 32, 0, 100, 0.0)
        for k, v in fields.items():
            r[k] = v
        return lib.nvw_denoise(e._h, r.ctypes.data, requests, None)

    assert e.denoiseReady(200, True) == 0 and call() == 0                            # no geometry set
    # hop not dividing n_fft, O = 2, n_fft = 2048, n_fft not a multiple of 4, O = 32, a hop that is no multiple of 4, a negative bias
    for n_fft, hop in ((64, 24), (64, 32), (2048, 512), (66, 11), (64, 2), (72, 6)):
        assert lib.nvw_set_denoiser(e._h, n_fft, hop, bias.ctypes.data) == 0, (n_fft, hop)
    assert lib.nvw_set_denoiser(e._h, 64, 16, None) == 0 and lib.nvw_set_denoiser(e._h, 64, 16, negative.ctypes.data) == 0
    e.setDenoiser(64, 16, bias[:33])
    assert lib.nvw_set_denoiser(e._h, 64, 32, bias.ctypes.data) == 0 and e.denoiseReady(200, True) == 200      # refused: the geometry stays
    for kw in (dict(requests=0), dict(requests=65536), {"in": host.ctypes.data}, dict(out=host.ctypes.data), dict(in_type=8),
               dict(out_type=64), dict(n_in=0), dict(count=0), dict(first=-1), dict(t0=-1), dict(strength=-0.5), dict(strength=np.nan),
               dict(strength=np.inf), dict(n_in=32, count=1),                         # a whole stream of n_fft / 2 samples
               dict(t0=101),                                                         # outputs past the stream's end
               dict(first=1, n_in=199),                                              # output 0 reflects about sample 0
               dict(first=33, n_in=167, t0=80, count=10),                            # output 80 needs sample 32 (frame 4 starts there)
               dict(last=0, t0=144, count=1)):                                       # output 144 lies in frame 11, which ends at sample 207
        assert call(**kw) == 0, kw
    e.synchronize()
    assert (out == 777).all()
    assert call(first=32, n_in=168, t0=80, count=10) == 1 and call(last=0, t0=100, count=44) == 1 and call(strength=0.5) == 1 and call(requests=2) == 2
    e.synchronize()
    assert (out[2:102] - 1).abs().max() < 1e-3 and (out[:2] == 777).all() and (out[102:] == 777).all()
    e.close()
