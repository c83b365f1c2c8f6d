"""The feature oracle (oracle/fft.py) pinned on its own: against a direct DFT, against the framing arithmetic of asr.fft, and its float32
option against the float64 default (the yardstick of tests/test_fbank_edges_gpu.py).  No GPU."""
import numpy as np
import pytest

from oracle import fft as offt


def frame_max_error(got, ref):
    """max_k |got - ref| / max_k ref per frame (last axis), over the frames whose reference maximum is non-zero; the largest of them"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = ref.max(axis=-1)
    live = top > 0
    if not live.any():
        return 0.0
    return float((np.abs(got - ref).max(axis=-1)[live] / top[live]).max())


def silence_in_the_middle():
    rs = np.random.RandomState(11)
    return np.concatenate([np.round(rs.randn(1500) * 3000), np.zeros(1200), np.round(rs.randn(1300) * 3000)]).astype(np.int16)


@pytest.mark.parametrize("n,nfft", [(64, 64), (50, 64), (512, 512), (400, 512)])
def test_powspec_against_a_direct_dft(n, nfft):
    """|X[k]|^2 / nfft with X[k] = sum_n x[n] exp(-2 pi i k n / nfft) written out (O(n^2), float64): independent of numpy.fft"""
    rs = np.random.RandomState(n + nfft)
    frames = rs.randn(3, n) * 1000
    k, t = np.arange(nfft // 2 + 1)[:, None], np.arange(n)[None, :]
    ang = -2.0 * np.pi * ((k * t) % nfft) / nfft
    re, im = frames @ np.cos(ang).T, frames @ np.sin(ang).T
    ref = (re ** 2 + im ** 2) / nfft
    got = offt.powspec(frames, nfft)
    assert got.shape == (3, nfft // 2 + 1)
    # both are float64 sums of n <= 512 terms: n eps relative to the frame's largest bin bounds either one
    assert frame_max_error(got, ref) <= 2 * n * np.finfo(np.float64).eps
    assert frame_max_error(offt.powspec(frames.astype(np.float32), nfft, np.float32), ref) <= 4e-6      # (float32: eps 1.2e-7, log2 n stages)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 672, 673])
def test_framesig_frame_counts(n):
    from asr.fft import num_frames
    frames = offt.framesig(np.arange(1, n + 1, dtype=np.float64), 512, 160)
    assert frames.shape == (num_frames(n, 512, 160), 512)
    assert frames.shape[0] == {1: 1, 511: 1, 512: 1, 513: 2, 672: 2, 673: 3}[n]
    flat = np.zeros((frames.shape[0] - 1) * 160 + 512)
    flat[:n] = np.arange(1, n + 1)
    for f in range(frames.shape[0]):            # frame f is samples 160 f .. 160 f + 511, zeros behind the signal's end
        assert np.array_equal(frames[f], flat[160 * f:160 * f + 512])


def test_float32_option_finds_the_same_exact_zeros():
    sig = silence_in_the_middle()
    fb = offt.get_filterbanks(40, 512, 16000)
    out = {}
    for dt in (np.float64, np.float32):
        ps = offt.get_specgram(sig, 16000, 0.032, 0.01, 512, 0.97, np.hanning, dtype=dt)
        lm = offt.compute_logmel(ps, fb, dtype=dt)
        assert ps.dtype == dt and lm.dtype == dt
        out[dt] = (ps, np.dot(ps, fb.astype(dt).T), lm)
    z64, z32 = out[np.float64][1] == 0, out[np.float32][1] == 0
    assert z64.sum() == 160 and np.array_equal(z64, z32)
    assert np.all(out[np.float64][2][z64] == np.log(np.finfo(float).eps))
    assert np.all(out[np.float32][2][z32] == np.log(np.float32(np.finfo(float).eps)))
    # the figures the GPU tests' caps start from (power spectrum 3.1e-7, mel energies 1.1e-6 over ten trial signals)
    assert frame_max_error(out[np.float32][0], out[np.float64][0]) <= 3.1e-7
    assert frame_max_error(out[np.float32][1], out[np.float64][1]) <= 1.1e-6


def test_float32_option_leaves_the_default_alone():
    sig = silence_in_the_middle()
    a = offt.get_specgram(sig, 16000, 0.032, 0.01, 512, 0.97, np.hanning)
    b = offt.powspec(offt.framesig(offt.preemphasis(sig, 0.97), 512, 160, np.hanning), 512)
    assert a.dtype == np.float64 and np.array_equal(a, b)
    x64, l64 = offt.logfbank_minibatch([sig])
    x32, l32 = offt.logfbank_minibatch([sig], dtype=np.float32)
    assert np.array_equal(l64, l32) and x64.shape == x32.shape
    live = x64[0, 0] > -30                     # (away from the log(eps) plateau both agree on)
    assert np.abs(x64[0, 0][live] - x32[0, 0][live]).max() <= 2e-4
