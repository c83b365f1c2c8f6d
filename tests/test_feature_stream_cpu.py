"""The recurrence of the streaming log-mel front end (tests/feature_stream_reference.py, the float64 form of include/asr_hip.h's
asr_fbank_stream_*) against oracle.fft on the whole signal: the same frame counts for every length and every way of cutting it, the
same values to 1e-12 (float64 rounding of a different summation order is 1e-15 here), and the arithmetic FeatureStream does on the host."""
import random

import numpy as np
import pytest

import feature_stream_reference as ref
from oracle import fft as o

CHUNKS = [0, 1, 3, 15, 16, 17, 63, 64, 65, 200]


def _run(stream, sig, cuts):
    """feed sig in chunks of `cuts` (cycled while samples are left), flush -> (T, 3, nfilt)"""
    outs, i, j = [], 0, 0
    while i < len(sig):
        n = cuts[j % len(cuts)]
        j += 1
        before = stream.c
        got = stream.advance(sig[i:i + n])
        assert len(stream.pend) < stream.L
        assert len(got) == max(0, stream.c - 2) - max(0, before - 2)
        outs.append(got)
        i += n
    tail = stream.flush()
    assert len(tail) <= 1
    outs.append(tail)
    return np.concatenate(outs)


def _check(L, S, nfft, fbank, sig, cuts):
    want = ref.oneshot(sig, L, S, nfft, fbank)
    s = ref.Stream(L, S, nfft, fbank)
    got = _run(s, sig, cuts)
    assert got.shape == want.shape, (len(sig), cuts[:8], got.shape, want.shape)
    assert s.emitted == len(want) == max(o_frames(len(sig), L, S) - 2, 0)
    if want.size:
        assert np.abs(got - want).max() <= 1e-12, (len(sig), np.abs(got - want).max())
    return s


def o_frames(N, L, S):
    return 1 if N <= L else 1 + -((L - N) // S)


def test_small_analogue_every_length_many_cuts():
    L, S, nfft, nfilt = 64, 16, 64, 8
    fbank = o.get_filterbanks(nfilt, nfft, 16000)
    rng, nprng = random.Random(0), np.random.RandomState(0)
    schedules = 0
    for N in list(range(0, 200)) + [rng.randrange(200, 900) for _ in range(60)]:
        sig = nprng.randint(-3000, 3000, N).astype(np.float64)
        for trial in range(3):
            cuts = [rng.choice(CHUNKS) for _ in range(64)] + [200]       # (ends the walk if the draws were all zeros)
            _check(L, S, nfft, fbank, sig, cuts)
            schedules += 1
    assert schedules >= 700


def test_small_analogue_fixed_cuts():
    L, S, nfft, nfilt = 64, 16, 64, 8
    fbank = o.get_filterbanks(nfilt, nfft, 16000)
    sig = np.random.RandomState(1).randint(-3000, 3000, 333).astype(np.float64)
    for cut in (1, 15, 16, 17, 333, 1000):
        _check(L, S, nfft, fbank, sig, [cut])


@pytest.mark.parametrize("N", [1, 3, 400, 511, 512, 513, 672, 673, 1153, 12345, 512 - 160 + 1, 512 + 160])
def test_real_frame_sizes(N):
    """L = 512, S = 160: the lengths of tests/test_fbank_edges_gpu.py's EDGE_FRAMES, and the two where the flush rule turns"""
    L, S, nfft, nfilt = 512, 160, 512, 40
    fbank = o.get_filterbanks(nfilt, nfft, 16000)
    sig = np.random.RandomState(N).randint(-3000, 3000, N).astype(np.float64)
    rng = random.Random(N)
    for cuts in ([N], [160], [159, 161, 0, 1], [rng.choice([0, 1, 100, 353, 511, 512, 513, 800]) for _ in range(40)] + [4000]):
        _check(L, S, nfft, fbank, sig, cuts)


def test_a_slot_starts_over_after_a_flush():
    L, S, nfft, nfilt = 64, 16, 64, 8
    fbank = o.get_filterbanks(nfilt, nfft, 16000)
    rs = np.random.RandomState(2)
    s = ref.Stream(L, S, nfft, fbank)
    for N in (150, 0, 7, 300):
        sig = rs.randint(-3000, 3000, N).astype(np.float64)
        before = s.emitted
        got = _run(s, sig, [37])
        want = ref.oneshot(sig, L, S, nfft, fbank)
        assert got.shape == want.shape and (want.size == 0 or np.abs(got - want).max() <= 1e-12)
        assert s.emitted == (len(want) if N > 0 else before)         # (a slot that is fed nothing keeps the finished count)


def test_chunk_arithmetic():
    from asr import fft
    assert [ref.chunk_frames(n, 160) for n in (0, 1, 160, 161, 320, 321)] == [0, 1, 1, 2, 2, 3]
    assert [fft.stream_frames(n, 160) for n in (0, 1, 160, 161, 320, 321)] == [0, 1, 1, 2, 2, 3]
    # the k new frames of a window [m < L pending | n new] never exceed the chunk's Tc
    for L, S in ((64, 16), (512, 160), (256, 80)):
        for m in (0, 1, L - S, L - 1):
            for n in range(1, 4 * S + 2):
                k = 0 if m + n < L else 1 + (m + n - L) // S
                assert k <= ref.chunk_frames(n, S)


def test_host_side_refusals():
    """what FeatureStream refuses before it touches a device"""
    from asr import fft
    proc = fft.Processor(device="cpu")
    for bad in (dict(B=0, max_samples=1280), dict(B=2, max_samples=0), dict(B=2, max_samples=128 * 160 + 1)):
        with pytest.raises(ValueError):
            fft.FeatureStream(proc, **bad)
    with pytest.raises(ValueError):
        fft.FeatureStream(fft.Processor(num_mel_filters=65, device="cpu"), 2, 1280)
    with pytest.raises(ValueError):
        fft.FeatureStream(proc, 2, 1280, mean=np.zeros((3, 40), dtype=np.float32))
