"""The log-mel front end (csrc/fbank.hip) at its edges, against the float64 oracle (oracle/fft.py).

Metric for spectra and mel energies: the error relative to the frame's own maximum, max_k |got - ref| / max_k ref per frame, over frames
whose reference maximum is non-zero (an absolute log-mel bar cannot hold for tonal inputs even in a correct float32 implementation).
Caps: what the FLOAT32 ORACLE (oracle/fft.py with dtype=np.float32; its mel energies, like the device's, read back through a float32
logarithm) reaches against the float64 oracle on the same input, times 4 (another butterfly order, sincospi twiddles against a library
transform), never above the 1e-6 x maximum convention of tests/test_nn_gpu.py for the power spectrum.  Each test prints its figures
(``pytest -s``); DESIGN.md records them.
"""
import numpy as np
import pytest
import torch

from oracle import fft as offt

pytestmark = pytest.mark.gpu
F32 = torch.float32
EPS32 = np.float32(2.220446049250313e-16)
LOG_EPS = np.log(EPS32)                     # float32: what a zero mel energy must come out as
CANARY = -7777.0
MARGIN = 4.0


def frame_max_error(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = ref.max(axis=-1)
    live = top > 0
    if not live.any():
        return 0.0
    return float((np.abs(got - ref).max(axis=-1)[live] / top[live]).max())


def _noise(seed, n, amp=3000):
    return np.round(np.random.RandomState(seed).randn(n) * amp).astype(np.int16)


def _signals():
    n = 4000
    t = np.arange(n)
    s = {}
    s["noise"] = _noise(21, n)
    s["silence_mid"] = np.concatenate([_noise(22, 1500), np.zeros(1200, np.int16), _noise(23, 1300)])
    s["all_zero"] = np.zeros(n, np.int16)
    s["leading_silence"] = np.concatenate([np.zeros(1700, np.int16), _noise(24, n - 1700)])
    s["trailing_silence"] = np.concatenate([_noise(25, n - 1700), np.zeros(1700, np.int16)])
    s["lsb"] = np.random.RandomState(26).choice([-1, 1], n).astype(np.int16)
    s["dc"] = np.full(n, 1000, np.int16)
    s["square"] = np.where((t // 20) % 2 == 0, 32767, -32768).astype(np.int16)
    s["sine"] = np.round(20000 * np.sin(2 * np.pi * 440 * t / 16000)).astype(np.int16)
    s["impulse"] = np.zeros(n, np.int16)
    s["impulse"][1234] = 12000
    # sample 511 is the last of frame 0, where np.hanning(512) is exactly zero (and its pre-emphasis echo, sample 512, is outside frame 0)
    s["impulse_at_window_zero"] = np.zeros(n, np.int16)
    s["impulse_at_window_zero"][511] = 12000
    return s


SIGNALS = _signals()
BROADBAND = ("noise", "silence_mid", "lsb", "impulse")
HANN = np.hanning(512)
_FB = {}
_ORACLE = {}


def fbank(nfilt, nfft=512):
    if (nfilt, nfft) not in _FB:
        _FB[(nfilt, nfft)] = offt.get_filterbanks(nfilt, nfft, 16000).astype(np.float32)
    return _FB[(nfilt, nfft)]


def oracle(sig, frame_len, step, nfft, window, fb, key=None):
    """float64 power spectrum, mel energies (zeros kept) and log-mel of one signal, and the two caps: 4 x the float32 oracle's error"""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    out = {}
    for dt in (np.float64, np.float32):
        ps = offt.powspec(offt.framesig(offt.preemphasis(sig, 0.97, dt), frame_len, step, lambda n: window, dt), nfft, dt)
        out[dt] = (ps, None if fb is None else offt.compute_logmel(ps, fb, dt))
    ps64, lm64 = out[np.float64]
    ps32, lm32 = out[np.float32]
    mel64 = None if fb is None else np.dot(ps64, fb.astype(np.float64).T)
    res = dict(ps=ps64, mel=mel64, lm=lm64, ps_f32=frame_max_error(ps32, ps64),
               mel_f32=0.0 if fb is None else frame_max_error(np.exp(lm32.astype(np.float64)), mel64))
    res["ps_cap"] = min(MARGIN * res["ps_f32"], 1e-6)
    res["mel_cap"] = MARGIN * res["mel_f32"]
    if key is not None:
        _ORACLE[key] = res
    return res


def dev_i32(v, device):
    return torch.tensor(list(v), dtype=torch.int32, device=device)


def pad_rows(sigs, pitch=None, dtype=np.int16):
    """rows of 4 n samples, zeros behind each signal"""
    n = max(len(s) for s in sigs)
    pitch = (n + 3) // 4 * 4 if pitch is None else pitch
    host = np.zeros((len(sigs), pitch), dtype=dtype)
    for i, s in enumerate(sigs):
        host[i, :len(s)] = s
    return host


def specgram_raw(sig, lens, frames, Fmax, frame_len, step, nfft, window, fb=None, bands=None, want_pspec=True):
    """asr_specgram_bands into canary-filled outputs (asr.fft._specgram allocates its own with torch.empty)"""
    from asr import _lib
    dev = sig.device
    B = sig.shape[0]
    nfilt = 0 if fb is None else fb.shape[0]
    pspec = torch.full((B, Fmax, nfft // 2 + 1), CANARY, dtype=F32, device=dev) if want_pspec else None
    logmel = torch.full((B, Fmax, nfilt), CANARY, dtype=F32, device=dev) if fb is not None else None
    lens_d, nfr_d = dev_i32(lens, dev), dev_i32(frames, dev)
    rc = _lib.lib().asr_specgram_bands(_lib.stream(), _lib.ptr(sig), 1 if sig.dtype == F32 else 0, _lib.ptr(lens_d), sig.stride(0), B, frame_len,
                                       step, nfft, 0.97, _lib.ptr(window), _lib.ptr(nfr_d), Fmax, _lib.ptr(pspec), _lib.ptr(fb), nfilt,
                                       _lib.ptr(logmel), _lib.ptr(bands) if fb is not None else None)
    torch.cuda.synchronize()
    return rc, pspec, logmel


def eps_positions(lm):
    """where a float32 log-mel array holds log(eps), to 1 ulp"""
    return np.abs(lm.astype(np.float64) - np.float64(LOG_EPS)) <= np.spacing(np.abs(LOG_EPS))


def check_against_oracle(tag, ref, ps, lm, abs_logmel=None):
    """ps (F, nbins) / lm (F, nfilt) float32 arrays from the device (either may be None) against oracle()'s record"""
    if ps is not None:
        assert ps.shape == ref["ps"].shape and np.isfinite(ps).all(), tag
        e = frame_max_error(ps, ref["ps"])
        print("fbank-edges %-44s pspec %.3g (float32 oracle %.3g, cap %.3g)" % (tag, e, ref["ps_f32"], ref["ps_cap"]))
        assert e <= ref["ps_cap"], (tag, "pspec", e, ref["ps_cap"])
        dead = ref["ps"].max(axis=-1) == 0
        assert (ps[dead] == 0).all(), (tag, "a silent frame has a non-zero bin")
    if lm is not None:
        assert lm.shape == ref["lm"].shape and np.isfinite(lm).all(), tag
        zero = ref["mel"] == 0
        got_zero = eps_positions(lm)
        assert np.array_equal(got_zero, zero), (tag, "log(eps) positions", int(got_zero.sum()), int(zero.sum()))
        e = frame_max_error(np.exp(lm.astype(np.float64)), ref["mel"])
        print("fbank-edges %-44s mel   %.3g (float32 oracle %.3g, cap %.3g), %d exact zeros" % (tag, e, ref["mel_f32"], ref["mel_cap"], zero.sum()))
        assert e <= ref["mel_cap"], (tag, "mel", e, ref["mel_cap"])
        if abs_logmel is not None:
            d = float(np.abs(lm - ref["lm"]).max())
            print("fbank-edges %-44s logmel abs %.3g" % (tag, d))
            assert d <= abs_logmel, (tag, "log-mel", d)


def run_one(device, sig, frame_len, step, nfft, window, fb, with_table=True, pitch=None):
    """one utterance through fft._specgram; the fast kernel is taken for nfft 512, step % 4 == 0, step <= 168 and rows of 4 n samples"""
    from asr import fft
    sig_d = torch.from_numpy(pad_rows([sig], pitch, sig.dtype)).to(device)
    F = fft.num_frames(len(sig), frame_len, step)
    win_d = torch.tensor(window, dtype=F32, device=device)
    fb_d = None if fb is None else torch.from_numpy(fb).to(device)
    bands = fft.mel_bands(fb_d) if (fb is not None and with_table) else None
    ps, lm = fft._specgram(sig_d, dev_i32([len(sig)], device), dev_i32([F], device), F, frame_len, step, nfft, 0.97, win_d, fb_d, True, bands)
    return ps[0].cpu().numpy(), None if lm is None else lm[0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ a. signal content
@pytest.mark.parametrize("step", [160, 162], ids=["fast", "general"])
@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_signal_content(device, name, step):
    """dc is the case that found two things in csrc/fbank.hip: the pre-emphasis coefficient rounded to float32 (power
    spectrum 1.04e-6 / 2.06e-6 against a cap of 1.5e-7) and logf's own ulp on top of the float32 spacing of the stored logarithm"""
    sig = SIGNALS[name]
    fb = fbank(40)
    ref = oracle(sig, 512, step, 512, HANN, fb, key=(name, step))
    ps, lm = run_one(device, sig, 512, step, 512, HANN, fb)
    if name == "silence_mid" and step == 160:
        assert int((ref["mel"] == 0).sum()) == 160
    if name == "impulse_at_window_zero":
        assert (ref["mel"][0] == 0).all() and (ref["mel"][1] > 0).all()      # frame 0 sees the impulse only through a zero of the window
    if name == "all_zero":
        assert (ref["mel"] == 0).all()
    check_against_oracle("%s/step%d" % (name, step), ref, ps, lm, abs_logmel=2e-4 if name in BROADBAND else None)
    zero = ref["mel"] == 0                      # log(float32(eps)) there, to 1 ulp (check_against_oracle: and nowhere else)
    assert (np.abs(lm[zero].astype(np.float64) - np.float64(LOG_EPS)) <= np.spacing(np.abs(LOG_EPS))).all()


# ------------------------------------------------------------------------------------------------ b. framing edges on the fast path
EDGE_BATCHES = [(1, 400, 512, 672, 1153, 12345), (12345, 3, 511, 513, 673)]
EDGE_FRAMES = {1: 1, 3: 1, 400: 1, 511: 1, 512: 1, 513: 2, 672: 2, 673: 3, 1153: 6, 12345: 75}


def _edge_signals(which):
    return [_noise(100 * which + i, n) for i, n in enumerate(EDGE_BATCHES[which])]


@pytest.mark.parametrize("extra_frames", [0, 9], ids=["Fmax_tight", "Fmax_beyond_every_utterance"])
@pytest.mark.parametrize("which", [0, 1])
def test_framing_edges_fast_path(device, which, extra_frames):
    from asr import fft
    sigs = _edge_signals(which)
    lens = [len(s) for s in sigs]
    frames = [fft.num_frames(n, 512, 160) for n in lens]
    assert frames == [EDGE_FRAMES[n] for n in lens]
    Fmax = max(frames) + extra_frames
    host = pad_rows(sigs)
    assert host.shape[1] % 4 == 0 and host.shape[1] >= 12345
    sig_d = torch.from_numpy(host).to(device)
    fb = fbank(40)
    fb_d, win_d = torch.from_numpy(fb).to(device), torch.tensor(HANN, dtype=F32, device=device)
    rc, ps, lm = specgram_raw(sig_d, lens, frames, Fmax, 512, 160, 512, win_d, fb_d, fft.mel_bands(fb_d))
    assert rc == 0
    ps, lm = ps.cpu().numpy(), lm.cpu().numpy()
    for b, s in enumerate(sigs):
        ref = oracle(s, 512, 160, 512, HANN, fb, key=("edge", which, b))
        check_against_oracle("edges%d/len%d/Fmax%d" % (which, lens[b], Fmax), ref, ps[b, :frames[b]], lm[b, :frames[b]], abs_logmel=2e-4)
        assert (ps[b, frames[b]:] == CANARY).all() and (lm[b, frames[b]:] == CANARY).all(), (b, "rows past nframes were written")
    if extra_frames == 0:           # the same through asr.fft._specgram (its own torch.empty outputs): identical live rows
        ps2, lm2 = fft._specgram(sig_d, dev_i32(lens, device), dev_i32(frames, device), Fmax, 512, 160, 512, 0.97, win_d, fb_d, True,
                                 fft.mel_bands(fb_d))
        for b in range(len(sigs)):
            assert np.array_equal(ps2[b, :frames[b]].cpu().numpy(), ps[b, :frames[b]])
            assert np.array_equal(lm2[b, :frames[b]].cpu().numpy(), lm[b, :frames[b]])


@pytest.mark.parametrize("form", ["list", "tuple"])
@pytest.mark.parametrize("which", [0, 1])
def test_logfbank_batch_short_utterances(device, which, form):
    from asr import fft
    sigs = _edge_signals(which)
    lens = [len(s) for s in sigs]
    proc = fft.Processor(device=device)
    arg = sigs if form == "list" else (torch.from_numpy(pad_rows(sigs)).to(device), lens)
    xr, xlr = offt.logfbank_minibatch(sigs)
    rs = np.random.RandomState(7)
    mean, std = rs.randn(3, 40).astype(np.float32), (rs.rand(3, 40) + 0.5).astype(np.float32)
    x, xl = proc.logfbank_batch(arg)
    xn, xln = proc.logfbank_batch(arg, mean, std)
    x, xn = x.cpu().numpy(), xn.cpu().numpy()
    assert np.array_equal(xl.cpu().numpy(), xlr) and np.array_equal(xln.cpu().numpy(), xlr)
    assert list(xlr) == [max(EDGE_FRAMES[n] - 2, 0) for n in lens] and x.shape == xr.shape == (len(sigs), 3, 40, 73)
    np.testing.assert_allclose(x, xr, rtol=0, atol=2e-4)                    # (the bars of test_logfbank_batch_matches_oracle)
    xrn = (xr - mean[None, ..., None]) / std[None, ..., None]
    np.testing.assert_allclose(xn, xrn, rtol=0, atol=5e-4)
    pad_value = (np.float32(0) - mean) / std                                 # float32, like the kernel
    for b, T in enumerate(xlr):
        assert (x[b, :, :, T:] == 0).all(), b
        assert np.array_equal(xn[b, :, :, T:], np.broadcast_to(pad_value[..., None], xn[b, :, :, T:].shape)), b
        if EDGE_FRAMES[lens[b]] <= 2:
            assert T == 0


# ------------------------------------------------------------------------------------------------ c. parameters
@pytest.mark.parametrize("n", [4000, 3998, 4001], ids=["len4000_fast", "len3998_general", "len4001_general"])
def test_get_specgram_defaults(device, n):
    """frame_len 400 in nfft 512, step 160, rectangular window: fft.get_specgram's own defaults; the single row's pitch is its length"""
    from asr import fft
    sig = _noise(31, n)
    ref = oracle(sig, 400, 160, 512, np.ones(400), None)
    ps = fft.get_specgram(torch.from_numpy(sig).to(device)).cpu().numpy()
    check_against_oracle("get_specgram defaults/len%d" % n, ref, ps, None)
    assert np.array_equal(ref["ps"], offt.get_specgram(sig))


@pytest.mark.parametrize("step", [160, 162], ids=["fast", "general"])
@pytest.mark.parametrize("frame_len", [512, 400])
def test_hamming_window(device, frame_len, step):
    sig, fb, win = SIGNALS["noise"], fbank(40), np.hamming(frame_len)
    ref = oracle(sig, frame_len, step, 512, win, fb)
    ps, lm = run_one(device, sig, frame_len, step, 512, win, fb)
    check_against_oracle("hamming%d/step%d" % (frame_len, step), ref, ps, lm, abs_logmel=2e-4)


@pytest.mark.parametrize("step,n", [(4, 1000), (168, 4000), (172, 4000)], ids=["step4_smallest", "step168_last_fast", "step172_first_general"])
def test_frame_steps(device, step, n):
    from asr import fft
    sig, fb = _noise(40 + step, n), fbank(40)
    assert fft.num_frames(n, 512, step) == {4: 123, 168: 22, 172: 22}[step]
    ref = oracle(sig, 512, step, 512, HANN, fb)
    ps, lm = run_one(device, sig, 512, step, 512, HANN, fb)
    check_against_oracle("step%d" % step, ref, ps, lm, abs_logmel=2e-4)


@pytest.mark.parametrize("how", ["pitch_not_4n", "pointer_off_by_one_sample"])
def test_unaligned_rows_take_the_general_kernel(device, how):
    """what the fast kernel's four-sample loads cannot take goes through the general kernel and gives the fast path's answer"""
    from asr import fft
    sigs = [_noise(51, 4001), _noise(52, 2222)]
    lens = [len(s) for s in sigs]
    frames = [fft.num_frames(n, 512, 160) for n in lens]
    fb = fbank(40)
    fb_d, win_d = torch.from_numpy(fb).to(device), torch.tensor(HANN, dtype=F32, device=device)
    bands = fft.mel_bands(fb_d)
    aligned = torch.from_numpy(pad_rows(sigs, 4004)).to(device)
    if how == "pitch_not_4n":
        odd = torch.from_numpy(pad_rows(sigs, 4001)).to(device)
    else:
        flat = torch.zeros(1 + 2 * 4004, dtype=torch.int16, device=device)
        odd = flat[1:].view(2, 4004)
        odd.copy_(aligned)
        assert odd.data_ptr() % 8 == 2 and odd.is_contiguous()
    rc, ps_f, lm_f = specgram_raw(aligned, lens, frames, max(frames), 512, 160, 512, win_d, fb_d, bands)
    rc2, ps_g, lm_g = specgram_raw(odd, lens, frames, max(frames), 512, 160, 512, win_d, fb_d, bands)
    assert rc == 0 and rc2 == 0
    for b, s in enumerate(sigs):
        ref = oracle(s, 512, 160, 512, HANN, fb, key=("unaligned", b))
        F = frames[b]
        check_against_oracle("%s/utt%d/fast" % (how, b), ref, ps_f[b, :F].cpu().numpy(), lm_f[b, :F].cpu().numpy(), abs_logmel=2e-4)
        check_against_oracle("%s/utt%d/general" % (how, b), ref, ps_g[b, :F].cpu().numpy(), lm_g[b, :F].cpu().numpy(), abs_logmel=2e-4)
        assert (ps_g[b, F:] == CANARY).all() and (lm_g[b, F:] == CANARY).all()
        # two kernels, one input: the bar of test_mel_band_table_and_its_fallbacks
        np.testing.assert_allclose(ps_g[b, :F].cpu().numpy(), ps_f[b, :F].cpu().numpy(), rtol=2e-4, atol=float(ps_f[b, :F].max()) * 1e-6)


@pytest.mark.parametrize("full", [True, False], ids=["frame_len_nfft", "frame_len_0.8nfft"])
@pytest.mark.parametrize("nfft", [64, 128, 256, 1024])
def test_general_kernel_other_transform_sizes(device, nfft, full):
    frame_len = nfft if full else int(0.8 * nfft)
    step = max(frame_len // 3, 1) | 1
    sig, fb = _noise(60 + nfft, 3001), fbank(26, nfft)
    win = np.hanning(frame_len)
    ref = oracle(sig, frame_len, step, nfft, win, fb)
    ps, lm = run_one(device, sig, frame_len, step, nfft, win, fb)
    check_against_oracle("nfft%d/frame_len%d/step%d" % (nfft, frame_len, step), ref, ps, lm)


@pytest.mark.parametrize("nfft,frame_len", [(2048, 2048), (500, 500), (32, 32), (512, 513), (256, 257)],
                         ids=["nfft2048", "nfft500", "nfft32", "frame_len513_nfft512", "frame_len257_nfft256"])
def test_refused_sizes_raise_and_write_nothing(device, nfft, frame_len):
    from asr import fft
    from asr._lib import AsrHipError
    sig_d = torch.from_numpy(pad_rows([SIGNALS["noise"]])).to(device)
    win_d = torch.ones(frame_len, dtype=F32, device=device)
    fb_d = torch.rand(8, nfft // 2 + 1, dtype=F32, device=device)
    F = fft.num_frames(4000, frame_len, 160)
    rc, ps, lm = specgram_raw(sig_d, [4000], [F], F, frame_len, 160, nfft, win_d, fb_d, None)
    assert rc == -3
    assert (ps == CANARY).all() and (lm == CANARY).all()
    with pytest.raises(AsrHipError):
        fft._specgram(sig_d, dev_i32([4000], device), dev_i32([F], device), F, frame_len, 160, nfft, 0.97, win_d, fb_d, True)
    with pytest.raises(AsrHipError):
        fft.get_specgram(sig_d[0], 16000, frame_len / 16000.0, 0.01, nfft)


# ------------------------------------------------------------------------------------------------ d. float32 signals
@pytest.mark.parametrize("step", [160, 162], ids=["fast", "general"])
def test_float32_signals_equal_int16_bit_for_bit(device, step):
    """integer-valued float32 samples: the same arithmetic after the load's conversion, so the same bits"""
    from asr import fft
    sigs = [SIGNALS[k] for k in ("noise", "silence_mid", "square", "sine", "impulse_at_window_zero")]
    lens = [3999, 4000, 3001, 513, 4000]
    frames = [fft.num_frames(n, 512, step) for n in lens]
    host = pad_rows([s[:n] for s, n in zip(sigs, lens)])
    fb_d, win_d = torch.from_numpy(fbank(40)).to(device), torch.tensor(HANN, dtype=F32, device=device)
    bands = fft.mel_bands(fb_d)
    out = {}
    for dt in (np.int16, np.float32):
        rc, ps, lm = specgram_raw(torch.from_numpy(host.astype(dt)).to(device), lens, frames, max(frames) + 1, 512, step, 512, win_d, fb_d, bands)
        assert rc == 0
        out[dt] = (ps.cpu().numpy(), lm.cpu().numpy())
    assert np.array_equal(out[np.int16][0].view(np.uint32), out[np.float32][0].view(np.uint32))
    assert np.array_equal(out[np.int16][1].view(np.uint32), out[np.float32][1].view(np.uint32))
    assert (out[np.float32][0][0, frames[0]:] == CANARY).all() and (out[np.float32][0][0, :frames[0]] != CANARY).all()


@pytest.mark.parametrize("step", [160, 162], ids=["fast", "general"])
def test_float32_signal_with_fractions(device, step):
    rs = np.random.RandomState(71)
    sig = (rs.randn(4000) * 1000.37).astype(np.float32)
    sig[2000:2400] = 0
    fb = fbank(40)
    ref = oracle(sig, 512, step, 512, HANN, fb)
    ps, lm = run_one(device, sig, 512, step, 512, HANN, fb)
    check_against_oracle("float32 fractions/step%d" % step, ref, ps, lm, abs_logmel=2e-4)


# ------------------------------------------------------------------------------------------------ e. the persistent loop wrapping
def test_more_groups_than_workgroups(device):
    """6 x 110000 samples: 686 frames = 172 groups of four each, 1032 groups for the 1024 persistent workgroups -- the look-ahead fetch and
    the group loop wrap once.  The first, the shorter fourth and the last utterance against the oracle."""
    from asr import fft
    lens = [110000, 110000, 110000, 54321, 110000, 110000]
    sigs = [_noise(80 + i, n) for i, n in enumerate(lens)]
    frames = [fft.num_frames(n, 512, 160) for n in lens]
    Fmax = max(frames)
    assert Fmax == 686 and 1024 < len(lens) * ((Fmax + 3) // 4) <= 1032
    fb = fbank(40)
    fb_d, win_d = torch.from_numpy(fb).to(device), torch.tensor(HANN, dtype=F32, device=device)
    rc, ps, lm = specgram_raw(torch.from_numpy(pad_rows(sigs)).to(device), lens, frames, Fmax, 512, 160, 512, win_d, fb_d, fft.mel_bands(fb_d))
    assert rc == 0
    assert (ps[3, frames[3]:] == CANARY).all() and (lm[3, frames[3]:] == CANARY).all()
    assert (ps[:, 0] != CANARY).all() and (ps[5, Fmax - 1] != CANARY).all()
    for b in (0, 3, 5):
        ref = oracle(sigs[b], 512, 160, 512, HANN, fb)
        check_against_oracle("wrap/utt%d" % b, ref, ps[b, :frames[b]].cpu().numpy(), lm[b, :frames[b]].cpu().numpy())


# ------------------------------------------------------------------------------------------------ f. mel band tables
def _mel_matrices():
    rs = np.random.RandomState(90)
    m = {}
    for nfilt in (1, 26, 63, 64, 65, 80):
        m["mel%d" % nfilt] = fbank(nfilt).copy()
    assert (m["mel80"] == 0).all(axis=1).sum() == 1            # (80 filters on 257 bins: one empty triangle, by construction)
    m["mel64_row0_zeroed"] = fbank(64).copy()
    m["mel64_row0_zeroed"][0] = 0
    m["mel64_row31_zeroed"] = fbank(64).copy()
    m["mel64_row31_zeroed"][31] = 0
    hole = fbank(64).copy()
    nz = np.nonzero(hole[50])[0]
    assert len(nz) >= 5
    hole[50, nz[1]:nz[-2]] = 0                                  # the first and the last two taps stay: one band, a hole inside it
    m["band_with_a_hole"] = hole
    dense = fbank(40).copy()
    dense[5] = rs.rand(257).astype(np.float32) * 0.01 + 1e-4
    m["row_dense_over_257_bins"] = dense
    taps1024 = np.zeros((64, 257), np.float32)
    for r in range(64):                                         # band lengths 9 .. 16: 16 padded taps each, 64 x 16 = 1024
        taps1024[r, 3 * r:3 * r + 9 + r % 8] = rs.rand(9 + r % 8).astype(np.float32) + 0.1
    m["exactly_1024_padded_taps"] = taps1024
    taps1032 = taps1024.copy()                                  # one band of 17 -> 24 padded taps: 1032
    taps1032[40, 120:137] = rs.rand(17).astype(np.float32) + 0.1
    m["1032_padded_taps"] = taps1032
    return m


MEL = _mel_matrices()
MEL_FITS = {"mel1": True, "mel26": True, "mel63": True, "mel64": True, "mel65": False, "mel80": False, "mel64_row0_zeroed": True,
            "mel64_row31_zeroed": True, "band_with_a_hole": True, "row_dense_over_257_bins": True, "exactly_1024_padded_taps": True,
            "1032_padded_taps": False}


def expected_table(fb):
    """csrc/fbank.hip's table: int start[64], len8[64], off[64]; float taps[1024] -- per filter its first non-zero bin, the band's length
    rounded up to a multiple of 8, the offset of its taps; a band's taps in ascending bin order, zeros behind its end.  None: does not fit
    (more than 64 filters or more than 1024 padded taps)."""
    if fb.shape[0] > 64:
        return None
    start, len8, off, taps = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(1024, np.float32)
    at = 0
    rows = []
    for r in range(64):
        nz = np.nonzero(fb[r])[0] if r < fb.shape[0] else []
        if len(nz):
            start[r], len8[r] = nz[0], (nz[-1] - nz[0] + 1 + 7) // 8 * 8
            rows.append((at, fb[r, nz[0]:nz[-1] + 1]))
        off[r] = at
        at += len8[r]
    if at > 1024:
        return None
    for o, band in rows:
        taps[o:o + len(band)] = band
    return start, len8, off, taps


@pytest.mark.parametrize("name", sorted(MEL))
def test_mel_band_tables(device, name):
    from asr import fft
    fb = MEL[name]
    fb_d = torch.from_numpy(fb).to(device)
    bands = fft.mel_bands(fb_d)
    table = bands.cpu().numpy()
    want = expected_table(fb)
    assert (want is not None) == MEL_FITS[name]
    assert (table[64] == -1) == (want is None)
    if want is not None:
        start, len8, off, taps = want
        if name == "exactly_1024_padded_taps":
            assert len8.sum() == 1024
        assert np.array_equal(table[:64], start) and np.array_equal(table[64:128], len8) and np.array_equal(table[128:192], off)
        assert np.array_equal(table[192:].view(np.float32), taps)
    elif name == "1032_padded_taps":
        assert expected_table(fb[:40])[1].sum() + 24 + expected_table(fb[41:])[1].sum() == 1032
    # the transform with the table and with the dense rows, against the float64 product of the oracle's spectrum and the same matrix
    sigs = [SIGNALS["silence_mid"], SIGNALS["noise"][:2001]]
    lens = [len(s) for s in sigs]
    frames = [fft.num_frames(n, 512, 160) for n in lens]
    sig_d = torch.from_numpy(pad_rows(sigs)).to(device)
    win_d = torch.tensor(HANN, dtype=F32, device=device)
    got = {}
    for tag, tb in (("table", bands), ("dense", None)):
        rc, _, lm = specgram_raw(sig_d, lens, frames, max(frames), 512, 160, 512, win_d, fb_d, tb, want_pspec=False)
        assert rc == 0
        got[tag] = lm.cpu().numpy()
    for b, s in enumerate(sigs):
        ref = oracle(s, 512, 160, 512, HANN, fb, key=("mel", name, b))
        for tag in ("table", "dense"):
            check_against_oracle("%s/utt%d/%s" % (name, b, tag), ref, None, got[tag][b, :frames[b]])
            assert (got[tag][b, frames[b]:] == CANARY).all()


@pytest.mark.parametrize("name", sorted(MEL))
def test_standalone_logmel_on_the_same_matrices(device, name):
    """asr_logmel: a float32 sum of products in ascending bin order.  With non-negative terms its relative error is at most (n + 1) 2^-24
    for n non-zero taps (each product and each addition rounds once, zeros add exactly), and logf adds at most 2 ulp of the result."""
    from asr import fft
    fb = MEL[name]
    ps = offt.get_specgram(SIGNALS["silence_mid"], 16000, 0.032, 0.01, 512, 0.97, np.hanning).astype(np.float32)
    ps[3] = 0
    assert (ps.max(axis=1) == 0).sum() >= 4                     # the frames inside the silence, and the one zeroed here
    lm = fft.compute_logmel(torch.from_numpy(ps).to(device), fbank=torch.from_numpy(fb).to(device)).cpu().numpy()
    mel = np.dot(ps.astype(np.float64), fb.astype(np.float64).T)
    zero = mel == 0
    assert zero.any() and np.array_equal(eps_positions(lm), zero)
    ref = np.log(np.where(zero, np.float64(EPS32), mel))
    ntaps = (fb != 0).sum(axis=1)[None, :]
    bound = (ntaps + 1) * 2.0 ** -24 + 2 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    bound = np.where(zero, np.spacing(np.abs(LOG_EPS)), bound)
    worst = float((np.abs(lm - ref) / bound).max())
    print("fbank-edges asr_logmel %-30s worst error / bound %.3g" % (name, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ g. deltas in isolation
DELTA_F = [1, 2, 3, 4, 5, 33, 34, 35, 65, 66, 67]
_DELTA = {}


def _delta_case(nfilt):
    """synthetic float32 log-mel rows (B, Fmax, nfilt): values near +13 beside the -36.04 of silence; NaN behind each utterance's end"""
    if nfilt not in _DELTA:
        rs = np.random.RandomState(300 + nfilt)
        B, Fmax = len(DELTA_F), max(DELTA_F)
        lm = (13 + 1.5 * rs.randn(B, Fmax, nfilt)).astype(np.float32)
        lm[rs.rand(B, Fmax, nfilt) < 0.2] = LOG_EPS
        lm[:, ::7, 0] = LOG_EPS
        mean, std = rs.randn(3, nfilt).astype(np.float32), (rs.rand(3, nfilt) + 0.5).astype(np.float32)
        refs = []
        for b, F in enumerate(DELTA_F):
            refs.append(np.stack([c.T for c in offt.compute_deltas(lm[b, :F].astype(np.float64))]))      # (3, nfilt, F - 2)
            lm[b, F:] = np.nan
        _DELTA[nfilt] = (lm, mean, std, refs)
    return _DELTA[nfilt]


def _run_deltas(device, lm, Tmax, mean=None, std=None):
    from asr import fft
    m = None if mean is None else torch.from_numpy(mean).to(device).reshape(-1)
    s = None if std is None else torch.from_numpy(std).to(device).reshape(-1)
    return fft._deltas(torch.from_numpy(lm).to(device), dev_i32(DELTA_F, device), Tmax, m, s).cpu().numpy()


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "mean_std"])
@pytest.mark.parametrize("Tmax", [65, 96, 74], ids=["Tmax65_tight", "Tmax96", "Tmax74_not_32n"])
@pytest.mark.parametrize("nfilt", [1, 40, 64, 65, 80], ids=["tile1", "tile40", "tile64", "generic65", "generic80"])
def test_deltas_in_isolation(device, nfilt, Tmax, normalise):
    lm, mean, std, refs = _delta_case(nfilt)
    out = _run_deltas(device, lm, Tmax, mean if normalise else None, std if normalise else None)
    assert out.shape == (len(DELTA_F), 3, nfilt, Tmax)
    # every output is at most three float32 subtractions and exact halvings of float32 inputs: 4 x spacing(max |logmel|); the normalised
    # ones that bound over std, plus 2 ulp of the result for the subtraction of the mean and the division
    atol = 4 * float(np.spacing(np.float32(np.nanmax(np.abs(lm)))))
    pad_value = (np.float32(0) - mean) / std
    worst = 0.0
    for b, F in enumerate(DELTA_F):
        T = max(F - 2, 0)
        got = out[b, :, :, :T].astype(np.float64)
        if normalise:
            want = (refs[b] - mean[..., None].astype(np.float64)) / std[..., None].astype(np.float64)
            bound = atol / std[..., None].astype(np.float64) + 2 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            pad = np.broadcast_to(pad_value[..., None], out[b, :, :, T:].shape)
        else:
            want, bound, pad = refs[b], atol, np.zeros_like(out[b, :, :, T:])
        assert np.isfinite(out[b]).all(), (b, F)
        if T:
            worst = max(worst, float((np.abs(got - want) / bound).max()))
        assert np.array_equal(out[b, :, :, T:], pad), (b, F, "padding beyond T_b")
    print("fbank-edges deltas nfilt %d Tmax %d %s: worst error / bound %.3g" % (nfilt, Tmax, "mean_std" if normalise else "raw", worst))
    assert worst <= 1.0


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "mean_std"])
def test_tile_and_generic_delta_kernels_agree_bit_for_bit(device, normalise):
    """deltas_tile_kernel (64 filters) and deltas_kernel (65 filters, the last one dropped afterwards) on the same values: both form
    (a - b) / 2, ((c - d) / 2 - (e - f) / 2) / 2 and (v - mean) / std from the same clamped rows in the same order, and halving is exact,
    so a contraction of the middle expression cannot change a bit either"""
    lm, mean, std, _ = _delta_case(65)
    for Tmax in (65, 74):
        g = _run_deltas(device, lm, Tmax, mean if normalise else None, std if normalise else None)
        t = _run_deltas(device, np.ascontiguousarray(lm[..., :64]), Tmax, np.ascontiguousarray(mean[:, :64]) if normalise else None,
                        np.ascontiguousarray(std[:, :64]) if normalise else None)
        assert np.array_equal(g[:, :, :64].view(np.uint32), t.view(np.uint32)), Tmax
