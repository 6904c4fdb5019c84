"""GPU tests of the analysis front end: nvw_analyse against the float64 definition -- mu-law exactly on every int16
value, the log-mel frames within the worst-case fp32 bound of the two dot products (derived, not measured) at the tile's and the
reflection's edges -- its refusals, and score_audio as analyse followed by score_mel."""
import math

import numpy as np
import pytest
import torch

from nv_wavenet_amd._lib import lib
from nv_wavenet_amd.engine import ANALYSIS_REQ, WavenetEngine

pytestmark = pytest.mark.gpu

SHAPES = {256: (64, 256, 256), 512: (64, 128, 512), 1024: (128, 256, 1024)}       # a built (R, S, A) per A
FLOOR = math.log(1e-5)
U = 2.0 ** -24


def _engine(A=256):
    R, S, A = SHAPES[A]
    return WavenetEngine(R, S, A, 3, 4, 1, 64, precision=32)


@pytest.fixture(scope="module")
def engine():
    e = _engine()
    yield e
    e.close()


def _mulaw(pcm, A):
    x, mu = pcm.astype(np.float64) / 32768.0, A - 1.0
    return ((np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu) + 1) / 2 * mu + 0.5).astype(np.int64)


@pytest.mark.parametrize("A", sorted(SHAPES))
def test_mulaw_equals_the_float64_formula_on_every_int16_value(A):
    e = _engine(A)
    e.setAnalysis(64, 16, np.ones((1, 33), dtype=np.float32))
    pcm = np.arange(-32768, 32768).astype(np.int16)
    y = torch.full((65536,), -7, dtype=torch.int32, device="cuda")
    e.analyse([(torch.from_numpy(pcm).cuda(), None, y)])
    e.synchronize()
    assert np.array_equal(y.cpu().numpy(), _mulaw(pcm, A))
    e.close()


def _basis(n_mel, bins):
    """Non-negative triangular filters, evenly spaced, at least two bins wide."""
    step = (bins - 1) / (n_mel + 1.0)
    centre = step * (1 + np.arange(n_mel))[:, None]
    return np.maximum(0.0, 1.0 - np.abs(np.arange(bins)[None, :] - centre) / max(step, 1.0)).astype(np.float32)


def _reference(pcm, n_fft, hop, M):
    """(m [n_mel][frames], its bar) in float64: the definition, and the bound of the issue for an fp32 implementation."""
    x = torch.from_numpy(pcm.astype(np.float64) / 32768.0)
    w = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    spec = torch.stft(x, n_fft, hop, n_fft, w, center=True, pad_mode="reflect", return_complex=True).abs().numpy()
    padded = torch.nn.functional.pad(x[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    S = (padded.unfold(0, n_fft, hop) * w).abs().sum(1).numpy()
    M = M.astype(np.float64)
    m = M @ spec
    assert m.shape[1] == len(pcm) // hop + 1 == len(S)
    kp = 16 * -(-(n_fft // 2 + 1) // 16)
    bar = 2 * (n_fft + 8) * U * S[None, :] * M.sum(1)[:, None] + 2 * (kp + 8) * U * m + 2.0 ** -20 * np.maximum(m, 1e-5)
    return m, bar


@pytest.mark.parametrize("dtype, transposed", [(torch.float32, False), (torch.float32, True), (torch.float16, False), (torch.float16, True)],
                         ids=["fp32", "fp32_t", "fp16", "fp16_t"])
@pytest.mark.parametrize("n_mel", [16, 80])
@pytest.mark.parametrize("n_fft, hop", [(1024, 256), (800, 200), (64, 16), (128, 128)])
def test_mel_and_samples_of_a_ragged_call_against_float64(engine, n_fft, hop, n_mel, dtype, transposed):
    M = _basis(n_mel, n_fft // 2 + 1)
    engine.setAnalysis(n_fft, hop, M)
    lengths = [n_fft // 2 + 1, 16 * hop - 1, 16 * hop, 16 * hop + 1, 5 * hop + hop // 2 + 1, 16 * hop]      # (the last: silence)
    rng = np.random.RandomState(n_fft + n_mel)
    pcms, reqs, outs = [], [], []
    for i, n in enumerate(lengths):
        t = np.arange(n)
        x = 0.5 * np.sin(2 * np.pi * (0.013 + 0.02 * i) * t + i) + 0.2 * rng.uniform(-1, 1, n)
        pcm = np.zeros(n, dtype=np.int16) if i == 5 else np.round(32767 * x).astype(np.int16)
        frames = engine.analysisFrames(n)
        assert frames == n // hop + 1
        buf = torch.full((frames + 2, n_mel) if transposed else (n_mel, frames + 2), 777.0, dtype=dtype, device="cuda")
        mel = buf.t() if transposed else buf
        y = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
        # (request 1 asks for frames only, request 3 for samples only)
        reqs.append((torch.from_numpy(pcm).cuda(), None if i == 3 else mel, None if i == 1 else y[:n]))
        pcms.append(pcm)
        outs.append((mel, y, frames))
    engine.analyse(reqs)
    engine.synchronize()
    slack = 2.0 ** -11 if dtype == torch.float16 else 0.0
    for i, (pcm, (mel, y, frames)) in enumerate(zip(pcms, outs)):
        n = len(pcm)
        got_y, got = y.cpu().numpy(), mel.double().cpu().numpy()
        assert (got_y[n:] == -7).all() and (got[:, frames:] == 777).all(), "request %d: written past its end" % i
        if i == 1:
            assert (got_y == -7).all()
        else:
            assert np.array_equal(got_y[:n], _mulaw(pcm, 256)), "request %d: samples" % i
        if i == 3:
            assert (got == 777).all()
            continue
        if i == 5:
            assert (mel[:, :frames] == torch.tensor(FLOOR, dtype=dtype)).all(), "silence is the floor, exactly"
            continue
        m, bar = _reference(pcm, n_fft, hop, M)
        mc = np.maximum(m, 1e-5)
        with np.errstate(divide="ignore"):
            lo, hi = np.log(np.maximum(mc - bar, 0.0)), np.log(mc + bar)
        pad = slack * np.abs(np.log(mc))
        out = got[:, :frames]
        excess = np.maximum(lo - pad - out, out - hi - pad)
        print("n_fft %d hop %d n_mel %d %s n %d: largest |exp(out) - m| / bar %.3g (the bar itself in fp32), nearest to its bar in the log "
              "domain %.3g" % (n_fft, hop, n_mel, str(dtype)[6:], n, (np.abs(np.exp(out) - mc) / bar).max(), excess.max()))
        assert (excess <= 0).all(), "request %d (n = %d): %d values beyond the bar, by up to %.3g" % (i, n, (excess > 0).sum(), excess.max())


def test_what_the_entries_refuse_and_that_nothing_is_written():
    e = _engine()
    pcm = torch.zeros(600, dtype=torch.int16, device="cuda")
    mel = torch.full((16, 40), 777.0, device="cuda")
    y = torch.full((600,), -7, dtype=torch.int32, device="cuda")

    def call(count=1, **kw):
        r = np.zeros(max(count, 1), dtype=ANALYSIS_REQ)
        r[:] = (pcm.data_ptr(), 600, mel.data_ptr(), 32, 40, 1, y.data_ptr())
        for k, v in kw.items():
            r[k] = v
        return lib.nvw_analyse(e._h, r.ctypes.data, count, None)

    assert e.analysisFrames(600) == 0 and call() == 0                                      # no geometry yet
    for n_fft, hop, n_mel in ((66, 16, 16), (60, 16, 16), (2052, 256, 16), (64, 0, 16), (64, 65, 16), (64, 16, 0), (64, 16, 129),
                              (2048, 2048, 16)):                                           # (the last: 194 KiB of LDS)
        basis = np.ones((max(n_mel, 1), n_fft // 2 + 1), dtype=np.float32)
        assert lib.nvw_set_analysis(e._h, n_fft, hop, n_mel, basis.ctypes.data) == 0, (n_fft, hop, n_mel)
    assert lib.nvw_set_analysis(e._h, 64, 16, 16, None) == 0 and e.analysisFrames(600) == 0
    e.setAnalysis(64, 16, np.ones((16, 33), dtype=np.float32))
    assert e.analysisFrames(600) == 38 and e.analysisFrames(32) == 0 and e.analysisFrames(33) == 3
    host = np.zeros(600, dtype=np.int16)
    for kw in (dict(count=0), dict(count=65536), dict(pcm=host.ctypes.data), dict(n=32), dict(mel=0, y=0), dict(c_stride=0), dict(f_stride=-1),
               dict(precision=8), dict(y=host.ctypes.data)):
        assert call(**kw) == 0, kw
    e.synchronize()
    assert (mel == 777).all() and (y == -7).all()
    assert call() == 1 and call(count=2) == 2
    e.synchronize()
    assert (mel[:, :38] == torch.tensor(FLOOR)).all() and (mel[:, 38:] == 777).all() and (y == 128).all()
    e.close()


def test_score_audio_is_analyse_then_score_mel():
    from nv_wavenet_amd.nv_wavenet import NVWaveNetEngine
    R, S, A, L, C, hop = 64, 256, 256, 3, 16, 16
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: (0.1 * torch.randn(*s, generator=g)).cuda()
    model = NVWaveNetEngine(embedding_prev=mk(A, R), embedding_curr=mk(A, R), conv_out_weight=mk(A, S, 1), conv_end_weight=mk(A, A, 1),
                            dilate_weights=[mk(2 * R, R, 2) for _ in range(L)], dilate_biases=[mk(2 * R) for _ in range(L)], max_dilation=4,
                            res_weights=[mk(R, R, 1) for _ in range(L - 1)], res_biases=[mk(R) for _ in range(L - 1)],
                            skip_weights=[mk(S, R, 1) for _ in range(L)], skip_biases=[mk(S) for _ in range(L)], use_embed_tanh=False,
                            precision=16)
    up = (mk(C, C, 2 * hop), mk(C), hop, mk(L * 2 * R, C, 1), mk(L * 2 * R))
    pcm = (8000 * torch.randn(2, 80, generator=g)).clamp(-32768, 32767).to(torch.int16).cuda()
    with pytest.raises(ValueError):
        model.score_audio(pcm, *up)                                                        # no set_analysis
    model.set_analysis(64, hop, torch.from_numpy(_basis(C, 33)))
    with pytest.raises(ValueError):
        model.score_audio(pcm, up[0], up[1], 8, up[3], up[4])                              # hop is not the stride
    with pytest.raises(ValueError):
        model.score_audio(pcm, mk(8, 8, 2 * hop), mk(8), hop, mk(L * 2 * R, 8, 1), up[4])  # n_mel is not the upsampling's channels
    mel, y = model.analyse(pcm, lengths=[80, 49])
    assert mel.shape == (2, C, 6) and mel.dtype == torch.float16 and y.shape == (2, 80) and y.dtype == torch.int32
    assert not y[1, 49:].any() and not mel[1, :, 4:].any() and np.array_equal(y[0].cpu().numpy(), _mulaw(pcm[0].cpu().numpy(), A))
    want = model.score_mel(mel, *up, y, lengths=[80, 49], temperature=[1.0, 0.7])
    got = model.score_audio(pcm, *up, lengths=[80, 49], temperature=[1.0, 0.7])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.isfinite(got).all() and (got[0] < 0).all()
    model.close()
