"""asr.fft.FeatureStream: the log-mel front end fed chunk by chunk against ``Processor.logfbank_batch`` of the whole signals on the
same device.  The stream runs every frame through the one-shot transform, mel and logarithm kernels on the same float32 samples and
restates only the delta expressions, so the comparison is ``torch.equal``: for every way of cutting the signals the valid columns of
all ``advance`` calls plus ``flush`` are the one-shot ``x[b, :, :, :x_length[b]]`` bit for bit.  The one-shot path is not the code
under test; tests/test_feature_stream_cpu.py checks the recurrence itself against the float64 oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 4
# every batch mixes edge lengths (0, 1, L - 1, L, L + 1, the flush rule's turn at 672 / 673, 833 = L + 2 S + 1) with ordinary ones
BATCHES = {"a": [5000, 513, 0, 672], "b": [2400, 1, 833, 512], "c": [673, 511, 2400, 1], "short": [700, 512, 673, 1],
           "long": [5000, 2400, 833, 673]}
CANARY = 9.0


def _signals(key, rate=16000):
    """int16 noise; slot 0 is a tone with a little noise on it"""
    rs = np.random.RandomState(sum(ord(ch) for ch in key))
    sigs = [np.round(rs.randn(n) * 3000).astype(np.int16) for n in BATCHES[key]]
    t = np.arange(len(sigs[0]))
    sigs[0] = np.round(8000 * np.sin(2 * np.pi * 440.0 * t / rate) + rs.randn(len(t)) * 20).astype(np.int16)
    return sigs


def _norm():
    rs = np.random.RandomState(7)
    return rs.randn(3, 40).astype(np.float32), (rs.rand(3, 40) + 0.5).astype(np.float32)


_PROC, _ONE = {}, {}


def _proc(device, rate=16000):
    from asr import fft
    if rate not in _PROC:
        _PROC[rate] = fft.Processor(sampling_rate=rate, device=device)
    return _PROC[rate]


def _oneshot(device, key, norm, rate=16000):
    """the yardstick, once per (batch, normalisation): per slot x[b, :, :, :x_length[b]] on the host, x_length, and a padding column"""
    if (key, norm, rate) not in _ONE:
        mean, std = _norm() if norm else (None, None)
        x, xl = _proc(device, rate).logfbank_batch(_signals(key, rate), mean, std)
        xl = xl.cpu().tolist()
        short = int(np.argmin(xl))
        assert xl[short] < x.shape[3]
        _ONE[(key, norm, rate)] = ([x[b, :, :, :xl[b]].cpu() for b in range(B)], xl, x[short, :, :, -1].cpu())
    return _ONE[(key, norm, rate)]


def _schedule(kind, lens, seed=0):
    """per call: the samples every slot gets"""
    rng = np.random.default_rng(seed)
    left = np.array(lens)
    calls, turn = [], 0
    while left.sum() > 0:
        turn += 1
        if kind == "whole":
            n = left.copy()
        elif isinstance(kind, int):
            n = np.minimum(left, kind)
        else:
            n = np.minimum(left, rng.integers(0, 700, size=len(lens)))
            n[turn % len(lens)] = 0
            if n.sum() == 0:
                continue
        calls.append(n)
        left = left - n
    return calls


def _feed(fs, sigs, calls, f32=False, device_n=False, start=None, Nc_of=None, canary_out=False):
    """run `calls` -> per call (x, lengths).  Samples of a chunk beyond a slot's share hold 77, which nothing may read."""
    pos = np.zeros(B, dtype=np.int64) if start is None else np.array(start)
    outs = []
    for i, n in enumerate(calls):
        Nc = int(n.max()) if Nc_of is None else Nc_of[i]
        chunk = np.full((B, Nc), 77, dtype=np.int16)
        for b, nb in enumerate(n):
            chunk[b, :nb] = sigs[b][pos[b]:pos[b] + nb]
        pos += n
        t = torch.from_numpy(chunk).to(fs.device)
        if f32:
            t = t.to(torch.float32)
        nn = torch.tensor(n, dtype=torch.int32)
        Tc = 1 + (Nc - 1) // fs.frame_step if Nc else 0
        out = torch.full((B, 3, fs.n_mel, Tc), CANARY, device=fs.device) if canary_out else None
        x, lengths = fs.advance(t, nn.to(fs.device) if device_n else nn, out=out)
        assert tuple(x.shape) == (B, 3, fs.n_mel, Tc) and x.dtype == torch.float32 and lengths.dtype == torch.int32 and lengths.is_cuda
        outs.append((x, lengths))
    return outs


def _per_slot(outs):
    lens = [o[1].cpu().tolist() for o in outs]
    return [torch.cat([o[0][b, :, :, :l[b]] for o, l in zip(outs, lens)], dim=2).cpu() for b in range(B)]


def _check_padding(outs, pad_col):
    """columns at or beyond lengths[b]: what the one-shot writes into its padding"""
    for x, lengths in outs:
        for b, l in enumerate(lengths.cpu().tolist()):
            tail = x[b, :, :, l:].cpu()
            assert torch.equal(tail, pad_col[:, :, None].expand_as(tail))


def _stream(device, max_samples, norm, rate=16000, cls=None):
    from asr import fft
    mean, std = _norm() if norm else (None, None)
    return (cls or fft.FeatureStream)(_proc(device, rate), B, max_samples, mean, std)


def _run_and_compare(device, key, kind, norm, f32=False, device_n=False, rate=16000, seed=0):
    want, xl, pad_col = _oneshot(device, key, norm, rate)
    calls = _schedule(kind, BATCHES[key], seed)
    fs = _stream(device, max(int(c.max()) for c in calls), norm, rate)
    outs = _feed(fs, _signals(key, rate), calls, f32=f32, device_n=device_n, canary_out=True)
    emitted = fs.frames.cpu().tolist()
    tail = fs.flush(out=torch.full((B, 3, fs.n_mel, 1), CANARY, device=device))
    assert tuple(tail[0].shape) == (B, 3, fs.n_mel, 1) and max(tail[1].cpu().tolist()) <= 1
    assert fs.frames.cpu().tolist() == xl == [e + t for e, t in zip(emitted, tail[1].cpu().tolist())]
    got = _per_slot(outs + [tail])
    for b in range(B):
        assert got[b].shape == want[b].shape, (key, kind, b, got[b].shape, want[b].shape)
        assert torch.equal(got[b], want[b]), (key, kind, b, float((got[b] - want[b]).abs().max()))
    _check_padding(outs + [tail], pad_col)
    again = fs.flush()                                                           # nothing is pending any more: N = 0 utterances, no frame
    assert again[1].cpu().tolist() == [0] * B and fs.frames.cpu().tolist() == xl


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
@pytest.mark.parametrize("kind", ["whole", 159, 160, 161, "ragged_host", "ragged_device"])
def test_bit_identity_under_every_cut(device, kind, f32, norm):
    for key in ("a", "b", "c"):
        _run_and_compare(device, key, "ragged" if isinstance(kind, str) and kind.startswith("ragged") else kind, norm, f32,
                         device_n=kind == "ragged_device", seed=3)


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("f32", [False, True], ids=["int16", "float32"])
def test_one_sample_chunks(device, f32, norm):
    _run_and_compare(device, "short", 1, norm, f32)


def test_the_general_transform_kernel(device):
    """8 kHz: nfft = 256, frame step 80 -- asr_specgram's one-workgroup-per-frame kernel, a different transform from the nfft = 512 one"""
    proc = _proc(device, 8000)
    assert (proc.num_fft, proc.frame_len, proc.frame_step) == (256, 256, 80)
    _run_and_compare(device, "b", "ragged", True, rate=8000, seed=5)
    _run_and_compare(device, "c", 81, False, rate=8000)


def _guarded():
    """FeatureStream whose buffers lie between canary guards"""
    from asr import fft
    G = 64                      # elements: 256 bytes, the buffers keep their alignment

    class Guarded(fft.FeatureStream):
        def _alloc(self, shape, dtype):
            numel = int(np.prod(shape))
            big = torch.full((numel + 2 * G,), 1234.5 if dtype == torch.float32 else 0x5A5A5A5A, dtype=dtype, device=self.device)
            self.__dict__.setdefault("guards", []).append((big, numel))
            return big[G:G + numel].view(shape)

        def guards_intact(self):
            for big, numel in self.guards:
                canary = 1234.5 if big.dtype == torch.float32 else 0x5A5A5A5A
                if not (bool((big[:G] == canary).all()) and bool((big[G + numel:] == canary).all())):
                    return False
            return len(self.guards) == 7

    return Guarded


def _bits(fs):
    return {k: v.clone().view(torch.int32) for k, v in fs.state().items()}


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
def test_padding_untouched_slots_and_guards(device, norm):
    want, xl, pad_col = _oneshot(device, "long", norm)
    sigs = _signals("long")
    calls = _schedule("ragged", BATCHES["long"], seed=11)
    fs = _stream(device, 700, norm, cls=_guarded())
    pos = np.zeros(B, dtype=np.int64)
    outs = []
    for n in calls:
        before = _bits(fs)
        outs += _feed(fs, sigs, [n], start=pos, canary_out=True)
        pos += n
        after = _bits(fs)
        lengths = outs[-1][1].cpu().tolist()
        for b in range(B):
            if n[b] == 0:
                assert lengths[b] == 0
                for name in before:
                    assert torch.equal(before[name][b], after[name][b]), (name, b)
    before = _bits(fs)
    tail = fs.flush([1, 0, 1, 0], out=torch.full((B, 3, fs.n_mel, 1), CANARY, device=device))
    after = _bits(fs)
    for b in (1, 3):                                                             # not flushed: not touched
        for name in before:
            assert torch.equal(before[name][b], after[name][b]), (name, b)
    rest = fs.flush([0, 1, 0, 1])
    got = _per_slot(outs + [tail, rest])
    for b in range(B):
        assert torch.equal(got[b], want[b])
    _check_padding(outs + [tail, rest], pad_col)
    assert fs.guards_intact()


def test_restart_of_one_slot(device):
    """slot 2 ends its utterance in the middle and starts another one while the others go on: they do not notice, the new utterance
    comes out as its one-shot features, and `frames` says so"""
    want, xl, _ = _oneshot(device, "long", False)
    sigs = _signals("long")
    second = np.round(np.random.RandomState(99).randn(1000) * 3000).astype(np.int16)
    want2 = _proc(device).logfbank_batch([second])
    want2 = want2[0][0, :, :, :int(want2[1][0])].cpu()
    calls = _schedule(400, BATCHES["long"])
    cut = 3                                                                      # 833 samples are through after three calls
    assert sum(int(c[2]) for c in calls[:cut]) == 833 and len(calls) > cut + 3
    rest, left2 = [], 1000
    for c in calls[cut:]:
        c = c.copy()
        c[2] = min(left2, 400)
        left2 -= c[2]
        rest.append(c)
    assert left2 == 0
    sigs2 = list(sigs)
    sigs2[2] = second
    pos = np.sum(calls[:cut], axis=0)
    pos2 = pos.copy()
    pos2[2] = 0
    # run A: with the restart
    a = _stream(device, 400, False)
    outs_a = _feed(a, sigs, calls[:cut])
    tail_a = a.flush([0, 0, 1, 0])
    assert tail_a[1].cpu().tolist()[:2] == [0, 0] and tail_a[1].cpu().tolist()[3] == 0 and a.frames.cpu().tolist()[2] == xl[2]
    first = _per_slot(outs_a + [tail_a])[2]
    assert torch.equal(first, want[2])
    outs_a2 = _feed(a, sigs2, rest, start=pos2)
    end_a = a.flush()
    assert a.frames.cpu().tolist() == [xl[0], xl[1], want2.shape[2], xl[3]]
    assert torch.equal(_per_slot(outs_a2 + [end_a])[2], want2)
    # run B: slot 2 just stays idle after its first utterance
    b = _stream(device, 400, False)
    idle = [np.array([c[0], c[1], 0, c[3]]) for c in rest]
    outs_b = _feed(b, sigs, calls[:cut])
    tail_b = (torch.zeros_like(tail_a[0]), torch.zeros_like(tail_a[1]))          # (no flush here: the other slots emit nothing in A's)
    outs_b2 = _feed(b, sigs, idle, start=pos, Nc_of=[int(c.max()) for c in rest])
    end_b = b.flush()
    for (xa, la), (xb, lb) in zip(outs_a + [tail_a] + outs_a2 + [end_a], outs_b + [tail_b] + outs_b2 + [end_b]):
        la, lb = la.cpu().tolist(), lb.cpu().tolist()
        for slot in (0, 1, 3):
            assert la[slot] == lb[slot] and torch.equal(xa[slot, :, :, :la[slot]], xb[slot, :, :, :lb[slot]])
    got = _per_slot(outs_a + [tail_a] + outs_a2 + [end_a])
    for slot in (0, 1, 3):
        assert torch.equal(got[slot], want[slot])


def test_limits(device):
    from asr import _lib, _ops, fft
    proc = _proc(device)
    S, M = proc.frame_step, _ops.FBANK_STREAM_MAX_FRAMES
    assert M == 128
    # a chunk of exactly the limit passes
    rs = np.random.RandomState(4)
    sigs = [np.round(rs.randn(M * S) * 3000).astype(np.int16) for _ in range(B)]
    fs = fft.FeatureStream(proc, B, M * S)
    assert fs.max_frames == M and fs.delay_samples == 512 + 2 * 160
    x, lengths = fs.advance(torch.from_numpy(np.stack(sigs)).to(device))
    tail = fs.flush()
    one, xl = proc.logfbank_batch(sigs)
    assert tuple(x.shape) == (B, 3, 40, M) and (lengths + tail[1]).cpu().tolist() == xl.cpu().tolist()
    for b in range(B):
        n = int(lengths[b])
        assert torch.equal(torch.cat([x[b, :, :, :n], tail[0][b, :, :, :int(tail[1][b])]], dim=2), one[b, :, :, :int(xl[b])])
    # one sample more is refused, by the class and by the entries, and nothing is written
    with pytest.raises(ValueError):
        fft.FeatureStream(proc, B, M * S + 1)
    Nc = M * S + 1
    chunk = torch.zeros((B, Nc), dtype=torch.int16, device=device)
    state = [torch.full(shape, 5, dtype=dt, device=device) for shape, dt in
             (((B, 512), torch.float32), ((B,), torch.float32), ((B, _ops.FBANK_STREAM_META), torch.int32),
              ((B, 512 + Nc + 8), torch.float32), ((B,), torch.int32), ((B,), torch.int32))]
    pend, last, meta, window, wlen, k = state
    with pytest.raises(_lib.AsrHipError, match="unsupported"):
        _ops.fbank_stream_push(chunk, None, None, pend, last, meta, window, wlen, k, 512, S, 0.97)
    logmel = torch.full((B, 4 + M + 1, 40), 5.0, device=device)
    out = torch.full((B, 3, 40, M + 1), 5.0, device=device)
    with pytest.raises(_lib.AsrHipError, match="unsupported"):
        _ops.fbank_stream_deltas(logmel, k, None, meta, out, wlen)
    wide = torch.full((B, 4 + 8, 65), 5.0, device=device)
    out65 = torch.full((B, 3, 65, 8), 5.0, device=device)
    with pytest.raises(_lib.AsrHipError, match="unsupported"):
        _ops.fbank_stream_deltas(wide, k, None, meta, out65, wlen)
    torch.cuda.synchronize()
    for t in state + [logmel, out, wide, out65]:
        assert bool((t == 5).all())


def test_refusals(device):
    from asr import fft
    fs = fft.FeatureStream(_proc(device), B, 800)
    ok = torch.zeros((B, 800), dtype=torch.int16, device=device)
    for bad in (torch.zeros((B, 801), dtype=torch.int16, device=device), ok[:3], ok.to(torch.int32), ok.to(torch.float64), ok[0]):
        with pytest.raises(ValueError):
            fs.advance(bad)
    with pytest.raises(ValueError):
        fs.advance(ok, [800, 801, 0, 1])                                        # a host n above Nc
    with pytest.raises(ValueError):
        fs.advance(ok, [800, 800, 800])
    with pytest.raises(ValueError):
        fs.flush([1, 0])
    with pytest.raises(ValueError):
        fs.reset([1, 0, 0, 0, 0])
    with pytest.raises(ValueError):
        fs.advance(ok, out=torch.zeros((B, 3, 40, 4), device=device))           # Tc is 5
    assert fs.frames.cpu().tolist() == [0] * B                                  # (nothing was consumed)
    x, lengths = fs.advance(ok[:, :0])
    assert tuple(x.shape) == (B, 3, 40, 0) and lengths.cpu().tolist() == [0] * B
    # a device n is clamped to [0, Nc]
    x, lengths = fs.advance(ok, torch.tensor([900, -5, 800, 0], dtype=torch.int32, device=device))
    assert fs.state()["meta"][:, 0].cpu().tolist() == [800 - 2 * 160, 0, 800 - 2 * 160, 0]      # pending: 800 = 512 + 160 + 128 -> k = 2


def test_against_the_float64_oracle(device):
    """the bars of tests/test_nn_gpu.py::test_logfbank_batch_matches_oracle on that test's own signals (noise, log-mel ~ 13 +- 1: what
    the bars were set for), fed in one ragged schedule.  Given the bit identity above the stream is exactly as far from the oracle
    as the one-shot path; this stands here so the file says so on its own.  (The tone of the other tests is not under these bars,
    neither streamed nor one-shot: in its empty bands, ten decades below the tone, float32 transforms are 2.7e-3 off in the
    logarithm -- measured on an MI355X at log-mel -5.9 -- which tests/test_fbank_edges_gpu.py bounds with tolerances derived for it.)"""
    from oracle import fft as offt
    rs = np.random.RandomState(0)
    lens = (16000, 9000, 12345, 700)
    sigs = [np.round(rs.randn(n) * 3000).astype(np.int16) for n in lens]
    mean = rs.randn(3, 40).astype(np.float32)
    std = (rs.rand(3, 40) + 0.5).astype(np.float32)
    for norm, atol in ((False, 2e-4), (True, 5e-4)):
        xr, xlr = offt.logfbank_minibatch(sigs, mean=mean if norm else None, std=std if norm else None)
        from asr import fft
        fs = fft.FeatureStream(_proc(device), B, 700, mean if norm else None, std if norm else None)
        outs = _feed(fs, sigs, _schedule("ragged", lens, seed=2))
        got = _per_slot(outs + [fs.flush()])
        assert [g.shape[2] for g in got] == xlr.tolist()
        for b in range(B):
            err = float(np.abs(got[b].numpy() - xr[b, :, :, :xlr[b]]).max())
            print("feature stream vs float64 oracle: normalised %s slot %d max abs error %.3e (bar %.0e)" % (norm, b, err, atol))
            np.testing.assert_allclose(got[b].numpy(), xr[b, :, :, :xlr[b]], rtol=0, atol=atol)


def test_into_the_acoustic_stream(device):
    """samples -> FeatureStream -> AcousticStream -> BeamStream in chunks of 800 samples, against the same AcousticStream fed the
    one-shot features cut into the same (Tc, lengths) chunks with the same padding: logits and hypotheses bit for bit"""
    import test_acoustic_stream_gpu as tas
    from asr import error
    from asr.model.stream import AcousticStream
    _, model = tas._build(device, lookahead=3)
    V = tas.V
    want, xl, _ = _oneshot(device, "long", False)
    sigs = _signals("long")
    calls = _schedule(800, BATCHES["long"])

    def run(chunks):
        """chunks: iterable of (x, lengths) -> (per call (logits, lengths), beam result)"""
        ac = AcousticStream(model, B, max_chunk=64)
        beam = error.BeamStream(B, V, max_frames=256, beam_width=8, top_k=8)
        outs = []
        for x, lengths in chunks:
            logits, ll = ac.advance(x, lengths)
            beam.advance(logits, ll)
            outs.append((logits, ll))
        logits, ll = ac.flush()
        beam.advance(logits, ll)
        outs.append((logits, ll))
        assert ac.frames.cpu().tolist() == xl
        return outs, beam.result()

    fs = _stream(device, 800, False)
    assert fs.max_frames == 5 and fs.max_frames <= 64
    feats = _feed(fs, sigs, calls)
    feats.append(fs.flush())
    outs_s, hyp_s = run(feats)
    cut, pos = [], [0] * B
    for x, lengths in feats:                                                     # the one-shot features in the same chunks
        ref = torch.zeros_like(x)
        for b, l in enumerate(lengths.cpu().tolist()):
            ref[b, :, :, :l] = want[b][:, :, pos[b]:pos[b] + l].to(device)
            pos[b] += l
        assert torch.equal(ref, x)
        cut.append((ref, lengths.clone()))
    assert pos == xl
    outs_r, hyp_r = run(cut)
    for (ls, ns), (lr, nr) in zip(outs_s, outs_r):
        ns, nr = ns.cpu().tolist(), nr.cpu().tolist()
        assert ns == nr
        for b in range(B):
            assert torch.equal(ls[:ns[b], b], lr[:nr[b], b])
    for s, r in zip(hyp_s, hyp_r):
        assert torch.equal(s, r)
