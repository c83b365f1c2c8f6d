"""The latency-controlled bidirectional GRU without a GPU: the restatement of tests/lc_bigru_reference.py against a per-frame brute
force and against the plain bidirectional layer, the adjoint identities of the window copies, the streaming push under random cut
schedules (the chunked layer = the one-shot layer), and the host side of the feature: ``stream_plan``, the configuration, the
checkpoint round trip.

The last test measures how far the four ways to get the layer wrong (lc_bigru_reference.MUTANTS) are from the right one on the
end-to-end case of tests/test_lc_bigru_gpu.py, in float64, and holds every one of them to five times the bar the GPU tests use.  The
bars are those of a run on an MI355X (bf16): twice the distance of the plain bidirectional model to its
float32 oracle, FORWARD_BAR for the logits and GRADIENT_BAR for the worst gradient among the recurrent layers' parameters (the GPU
test holds every parameter to the plain model's worst parameter, the first convolution's weight, and the recurrent parameters to this
tighter bar of their own: it is the one that reaches a mutant of the recurrent layer's backward pass).  The GPU tests repeat the
five-bar check at run time against the bars of their own run."""
import numpy as np
import pytest
import torch

import lc_bigru_reference as lc

CASES = [(1, 0), (4, 0), (8, 4), (5, 7), (3, 11), (64, 0)]
FORWARD_BAR = {1: 2 * 5.745e-3, 2: 2 * 5.446e-3}        # by time_reduction: twice the plain bidirectional model's E1 on the logits
GRADIENT_BAR = {1: 2 * 2.713e-2, 2: 2 * 4.613e-2}       # ... and twice its worst gradient distance over the recurrent layers' parameters


def _params(rng, I, H, dtype=torch.float64):
    k = 1.0 / np.sqrt(H)
    return [torch.from_numpy(rng.uniform(-k, k, size=s)).to(dtype) for s in ((2, 3 * H, I), (2, 3 * H, H), (2, 3 * H), (2, 3 * H))]


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("Nc,Nr", CASES)
def test_restatement_against_the_per_frame_brute_force(Nc, Nr):
    rng = np.random.default_rng(100 * Nc + Nr)
    I, H, B = 5, 6, 3
    p = _params(rng, I, H)
    for T in sorted({1, max(Nc - 1, 1), Nc, Nc + 1, Nc + Nr, min(2 * Nc + Nr + 1, 21)}):
        x = torch.from_numpy(rng.normal(size=(T, B, I)))
        for x_len in (None, [T, 0, max(T - 2, 0)], [1, T + 3, T // 2]):
            y = lc.layer(x, *p, Nc, Nr, x_len)
            want = lc.brute_force(x, *p, Nc, Nr, x_len)
            assert float((y - want).abs().max()) <= 1e-12, (T, x_len)
            for b, n in enumerate(lc.lengths(x_len, T, B)):
                assert not y[n:, b].any()


def test_a_block_as_long_as_the_utterance_is_the_bidirectional_layer():
    from oracle import nn as onn
    rng = np.random.default_rng(3)
    I, H, B, T = 7, 8, 2, 13
    p = _params(rng, I, H, torch.float32)
    x = torch.from_numpy(rng.normal(size=(T, B, I))).float()
    want, _ = onn.bigru_sum(x, dict(zip(("w_ih", "w_hh", "b_ih", "b_hh"), p)), H)
    for Nc, Nr in ((T, 0), (T, 5), (T + 9, 0), (64, 3)):
        assert float((lc.layer(x, *p, Nc, Nr) - want.detach()).abs().max()) <= 1e-6, (Nc, Nr)
    assert float((lc.layer(x, *p, T - 1, 0) - want.detach()).abs().max()) > 1e-3       # one frame shorter is another layer


# ------------------------------------------------------------------------------------------------------------ gather and scatter
@pytest.mark.parametrize("Nc,Nr", CASES)
def test_gather_and_scatter_are_adjoint_in_pairs(Nc, Nr):
    """<A x, y> = <x, A^T y> in float64: the input gather (keep = W) with the overlap-add (span = W), the forward pass's scatter
    (span = Nc) with the gradient gather (keep = Nc); with and without lengths and switched-off windows"""
    rng = np.random.default_rng(7 + 10 * Nc + Nr)
    B, R = 3, 4
    for T in sorted({1, max(Nc - 1, 1), Nc, Nc + 1, Nc + Nr, 2 * Nc + Nr + 1}):
        W, C = lc.window_shape(T, B, Nc, Nr)
        for x_len, n_win in ((None, None), ([T, 0, T // 2 + 1], None), ([T + 2, 1, max(T - 1, 0)], [C, 0, max(C - 1, 0)])):
            for block_only in (False, True):
                x, yw = rng.normal(size=(T, B, R)), rng.normal(size=(W, C * B, R))
                ax, w_len = lc.gather(x, Nc, Nr, block_only, x_len, n_win)
                aty = lc.scatter(yw, T, B, Nc, Nr, not block_only, None, x_len, n_win)
                assert abs(float((ax * yw).sum()) - float((x * aty).sum())) <= 1e-9 * max(1.0, float(np.abs(ax * yw).sum())), (T, x_len, block_only)
                assert w_len.max(initial=0) <= W
            # the scatter's addend passes through below the length, and nothing lies beyond it
            add = rng.normal(size=(T, B, R))
            y = lc.scatter(np.zeros((W, C * B, R)), T, B, Nc, Nr, False, add, x_len, n_win)
            for b, n in enumerate(lc.lengths(x_len, T, B)):
                assert np.array_equal(y[:n, b], add[:n, b]) and not y[n:, b].any()


def test_the_rounding_of_the_scatter():
    """float32 sums, one rounding, in both 16-bit formats: 1 + ulp / 2 + ulp / 4 is 1 + ulp, but 1 when every partial sum is rounded
    (the tie goes to the even 1, and ulp / 4 more is lost again)"""
    for fmt in ("bf16", "f16"):
        vals = np.array([1.0, 2.0 ** -8, 2.0 ** -9, 3.0], dtype=np.float32) if fmt == "bf16" else \
            np.array([1.0, 2.0 ** -11, 2.0 ** -12, 3.0], dtype=np.float32)
        words = lc.encode(vals, fmt)
        assert np.array_equal(lc.decode(words, fmt), vals)
        # Nc = 1, Nr = 1, T = 2: frame 1 lies in window 0 (as right context) and in window 1; the overlap-add sums both and the addend
        yw = np.zeros((2, 2, 8), dtype=np.int16)
        yw[0, 0], yw[0, 1] = words[1], words[2]             # window 0 row 0 = frame 1, window 1 row 0 = frame 1
        yw[1, 0] = words[3]                                 # window 0 row 1 = frame 0
        add = np.zeros((2, 1, 8), dtype=np.int16)
        add[1, 0] = words[0]
        y = lc.scatter(yw, 2, 1, 1, 1, True, add, None, None, fmt)
        ulp = 2.0 ** -7 if fmt == "bf16" else 2.0 ** -10
        assert np.all(lc.decode(y, fmt)[1, 0] == 1.0 + ulp) and np.all(lc.decode(y, fmt)[0, 0] == 3.0)


# ------------------------------------------------------------------------------------------------------------ the push
def _cuts(rng, lens, most):
    """random per-call frame counts per slot until every slot is through: zeros, single frames and several blocks at once"""
    left, calls = np.array(lens), []
    while left.sum() > 0:
        n = np.minimum(left, rng.integers(0, most + 1, size=len(lens)))
        if rng.random() < 0.3:
            n[rng.integers(len(lens))] = 0
        if n.sum():
            calls.append(n)
            left = left - n
    return calls


@pytest.mark.parametrize("Nc,Nr", [(1, 0), (4, 0), (8, 4), (5, 7), (3, 11)])
def test_the_chunked_layer_is_the_one_shot_layer(Nc, Nr):
    """Random cut schedules with n = 0, fewer rows than the right context, several blocks per chunk; every slot flushed when it is
    through (slot 1 in the middle of the others, and restarted with a second utterance): the rows a slot emits are the one-shot
    layer's of its utterance, to 1e-12, and there are exactly as many."""
    rng = np.random.default_rng(50 + 10 * Nc + Nr)
    I, H, B = 4, 5, 3
    p = _params(rng, I, H)
    lens = [23, 7, 31]
    utts = [torch.from_numpy(rng.normal(size=(n, 1, I))) for n in lens] + [torch.from_numpy(rng.normal(size=(12, 1, I)))]
    want = [lc.layer(u, *p, Nc, Nr)[:, 0].numpy() for u in utts]
    for most in (1, 3, 2 * (Nc + Nr) + 3):
        chunked = lc.ChunkedLayer(*p, Nc, Nr, B)
        calls = _cuts(rng, lens, most)
        pos, got = np.zeros(B, dtype=np.int64), [[] for _ in range(B + 1)]
        source = [0, 1, 2]                                  # the utterance every slot is in
        extra = 12
        step = 0
        while step < len(calls) or extra > 0:
            n = calls[step].copy() if step < len(calls) else np.zeros(B, dtype=np.int64)
            step += 1
            if source[1] == 3:                              # slot 1's second utterance, a few frames per call
                n[1] = min(extra, int(rng.integers(0, most + 1)))
                extra -= n[1]
            Tc = int(n.max())
            chunk = np.full((Tc, B, I), 9.0)
            for b in range(B):
                chunk[:n[b], b] = utts[source[b]][pos[b]:pos[b] + n[b], 0].numpy()
            before = (chunked.carry.state.copy(), chunked.carry.m.copy(), chunked.h.clone())
            y, emit = chunked.push(chunk if Tc else None, n.astype(np.int32))
            pos += n
            for b in range(B):
                got[source[b]].append(y[:emit[b], b])
                if n[b] == 0:                               # an unfed slot is left as it is
                    assert emit[b] == 0 and np.array_equal(chunked.carry.state[:, b], before[0][:, b]) and chunked.carry.m[b] == before[1][b]
                    assert torch.equal(chunked.h[b], before[2][b])
                assert chunked.carry.m[b] <= Nc + Nr - 1
            if source[1] == 1 and pos[1] == lens[1]:        # slot 1 ends here: flush it alone, then start it over
                mask = np.array([0, 1, 0])
                y, emit = chunked.push(None, np.zeros(B, dtype=np.int32), mask)
                assert emit[0] == 0 and emit[2] == 0 and y.shape[0] == Nc + Nr - 1
                got[1].append(y[:emit[1], 1])
                chunked.reset(mask)
                source[1], pos[1] = 3, 0
        y, emit = chunked.push(None, None, np.ones(B, dtype=np.int32))
        for b in range(B):
            got[source[b]].append(y[:emit[b], b])
        for u in range(B + 1):
            rows = np.concatenate(got[u])
            assert rows.shape == want[u].shape, (most, u, rows.shape)
            assert float(np.abs(rows - want[u]).max()) <= 1e-12, (most, u)


def test_push_counts():
    """a, w and emit of asr_lc_push as the header states them, and a flush of chunk and pending rows together"""
    c = lc.Carry(4, 3, 2, 8, dtype=np.float64)
    rng = np.random.default_rng(0)
    window, a, w, emit = c.push(rng.normal(size=(6, 2, 8)), np.array([6, 2]))
    assert window.shape[0] == 6 + 6 and a.tolist() == [6, 2] and w.tolist() == [0, 0] and emit.tolist() == [0, 0] and c.m.tolist() == [6, 2]
    window, a, w, emit = c.push(rng.normal(size=(5, 2, 8)), np.array([5, 0]))
    assert a.tolist() == [11, 2] and w.tolist() == [2, 0] and emit.tolist() == [8, 0] and c.m.tolist() == [3, 2]
    window, a, w, emit = c.push(rng.normal(size=(1, 2, 8)), np.array([1, 1]), np.array([0, 1]))
    assert a.tolist() == [4, 3] and w.tolist() == [0, 1] and emit.tolist() == [0, 3] and c.m.tolist() == [4, 0] and not c.state[:, 1].any()


# ------------------------------------------------------------------------------------------------------------ the host side
def _config(**fields):
    from asr.model import ds2
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers = 32, 16, 64, 32, 2
    for name, value in fields.items():
        setattr(cfg, name, value)
    return cfg


def test_configuration():
    from asr import nn
    from asr.model import ds2
    assert ds2.configure().latency_control is None
    plain = ds2.Model(_config())
    assert all(isinstance(layer, nn.BiGRU) for layer in plain.rnn_blocks.layers[::2]) and plain.latency_control is None
    model = ds2.Model(_config(latency_control=(8, 4), time_reduction=2))
    layers = model.rnn_blocks.layers[::2]
    assert len(layers) == 2 and all(isinstance(layer, nn.LCBiGRU) and (layer.block, layer.right) == (8, 4) for layer in layers)
    assert not any(isinstance(layer, nn.BiGRU) for layer in layers) and model.latency_control == (8, 4)
    assert ds2.Model(_config(latency_control=[5, 0])).latency_control == (5, 0)         # (a configuration read back from JSON)
    assert list(model.state_dict().keys()) == list(ds2.Model(_config(time_reduction=2)).state_dict().keys())     # no name moves
    for bad in ((0, 4), (8, -1), (8.0, 4), (True, 4), (8,), (8, 4, 2), 8, "8,4", (4000, 97)):
        with pytest.raises(ValueError):
            ds2.Model(_config(latency_control=bad))
    with pytest.raises(ValueError):
        ds2.Model(_config(latency_control=(8, 4), bidirectional=False))
    with pytest.raises(ValueError):
        ds2.Model(_config(latency_control=(8, 4), lookahead=2))
    with pytest.raises(ValueError):
        ds2.Model(_config(latency_control=(8, 4), bidirectional=False, lookahead=2))
    with pytest.raises(ValueError):
        nn.LCBiGRU(8, 8, block=0)
    with pytest.raises(ValueError):
        nn.LCBiGRU(8, 8)(torch.zeros(1, 8, 3), hx=torch.zeros(2, 1, 8))


def test_stream_plan_entries_and_refusals():
    from asr import nn
    from asr.model import ds2
    from asr.model.stream import stream_plan
    model = ds2.Model(_config(latency_control=(8, 4)))
    plan = stream_plan(model)
    entries = [e for e in plan["layers"] if e["kind"] == "lc"]
    assert entries == [{"kind": "lc", "H": 64, "index": 0, "Nc": 8, "Nr": 4, "K": 11, "R": 96},
                       {"kind": "lc", "H": 64, "index": 2, "Nc": 8, "Nr": 4, "K": 11, "R": 64}]
    assert plan["delay"] == 22 and [e["kind"] for e in plan["layers"]] == ["context", "context", "lc", "lc"]
    plan = stream_plan(ds2.Model(_config(latency_control=(5, 7), time_reduction=2, num_rnn_layers=3)))
    assert [e["R"] for e in plan["layers"] if e["kind"] == "lc"] == [192, 64, 64] and plan["delay"] == 33 and plan["time_reduction"] == 2
    assert [e["kind"] for e in plan["layers"]] == ["context", "context", "stack", "lc", "lc", "lc"]
    assert stream_plan(ds2.Model(_config(latency_control=(1, 0))))["delay"] == 0
    with pytest.raises(ValueError, match="a bidirectional model cannot be streamed: its reverse recurrences start at the end of the utterance"):
        stream_plan(ds2.Model(_config()))
    mixed = ds2.Model(_config(latency_control=(8, 4)))
    mixed.rnn_blocks.layers[2] = nn.BiGRU(None, 64)                                  # one plain layer among them is refused as ever
    with pytest.raises(ValueError, match="a bidirectional model cannot be streamed"):
        stream_plan(mixed)
    mixed.rnn_blocks.layers[2] = nn.GRU(None, 64)
    with pytest.raises(ValueError, match="latency-controlled"):
        stream_plan(mixed)
    behind = ds2.Model(_config(latency_control=(8, 4)))
    behind.lookahead = nn.LookaheadConvolution(64, 2)
    with pytest.raises(ValueError, match="latency-controlled"):
        stream_plan(behind)


def test_checkpoint_round_trip(tmp_path):
    """a BiGRU checkpoint loads into an LCBiGRU and back: the layer, and the model through its own save and load"""
    from asr import nn
    from asr.model import ds2
    torch.manual_seed(1)
    a, b = nn.BiGRU(12, 8), nn.LCBiGRU(12, 8, block=4, right=2)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) == ["w_ih", "w_hh", "b_ih", "b_hh"]
    assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]
    b.load_state_dict(a.state_dict())
    back = nn.BiGRU(12, 8)
    back.load_state_dict(b.state_dict())
    for name, value in a.state_dict().items():
        assert torch.equal(value, b.state_dict()[name]) and torch.equal(value, back.state_dict()[name])
    plain, control = ds2.Model(_config()), ds2.Model(_config(latency_control=(8, 4)))
    for model in (plain, control):                          # (size what the first call would size)
        width = 96
        for layer in model.rnn_blocks.layers[::2]:
            layer._initialize_params(width)
            width = 64
        model.dense_blocks.layers[0]._initialize_params(64)
        model.dense_blocks.layers[-1].norm._initialize_params(32)
    path = str(tmp_path / "bigru.model")
    plain.save(path)
    assert control.load(path)
    for (name, value), (other, loaded) in zip(plain.state_dict().items(), control.state_dict().items()):
        assert name == other and torch.equal(value, loaded), name
    path = str(tmp_path / "lc.model")
    control.save(path)
    fresh = ds2.Model(_config())
    assert fresh.load(path)
    for (name, value), (other, loaded) in zip(plain.state_dict().items(), fresh.state_dict().items()):
        assert name == other and torch.equal(value, loaded), name


# ------------------------------------------------------------------------------------------------------------ the mutants
def _sized_state(cfg, seed):
    from asr.model import ds2
    torch.manual_seed(seed)
    model = ds2.Model(cfg)
    width = 96 * cfg.time_reduction
    for layer in model.rnn_blocks.layers[::2]:
        layer._initialize_params(width)
        width = cfg.ndim_rnn
    model.dense_blocks.layers[0]._initialize_params(cfg.ndim_rnn)
    model.dense_blocks.layers[-1].norm._initialize_params(cfg.vocab_size)
    return {name: v.detach().clone() for name, v in model.state_dict().items()}


def _rel(got, want):
    a = torch.cat([g.double().flatten() for g in got])
    b = torch.cat([w.double().flatten() for w in want])
    return float((a - b).norm() / b.norm())


def _labels(k):
    """the synthetic transcripts, cut against the frames the loss sees (tests/test_lc_bigru_gpu.py::_labels)"""
    from asr.data.processing import truncate_labels_for_ctc
    from oracle import model as omodel
    labels, l_len = omodel.synthetic_batch(4, 41, 32, Lmin=3, Lmax=9, seed=0, ragged=True)[1::2]
    labels, l_len = labels.clone(), l_len.clone()
    for b, n in enumerate([-(-n // k) for n in (41, 29, 5, 36)]):
        ids = labels[b, :l_len[b]].tolist()
        keep = len(truncate_labels_for_ctc(ids, ids, n)[0])
        labels[b, keep:] = 0
        l_len[b] = keep
    return labels, l_len


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("Nc,Nr", [(8, 4), (5, 7)])
def test_mutants_are_far_from_the_layer(Nc, Nr, k):
    """The end-to-end case of the GPU tests (V = 32, conv 16, GRU 64, dense 32, B = 4, T = 41, lengths 41 / 29 / 5 / 36, the same
    seed, both time reductions) in float64: the logits of the restated model with the right context dropped, the window's rows taken
    one frame late or the reverse state carried across blocks, against the right one, over the valid frames; and, for right-context
    outputs given gradient (the forward pass is the same), the CTC gradients of the recurrent layers' parameters, as the GPU test
    measures them: the worst relative distance among them.  Every one must be at least five times the GPU bar away.  Measured
    (DESIGN.md section 41.6), right context dropped / rows one frame late / state carried / right-context gradient:
    k = 1: (8, 4): 1.52e-1, 1.54e-1, 9.10e-2, 4.72e-1; (5, 7): 2.18e-1, 1.53e-1, 7.56e-2, 1.74; five bars: 5.75e-2 and 2.71e-1.
    k = 2: (8, 4): 1.34e-1, 1.67e-1, 5.88e-2, 5.09e-1; (5, 7): 2.21e-1, 1.66e-1, 6.13e-2, 1.43; five bars: 5.45e-2 and 4.61e-1."""
    from oracle import model as omodel
    V, B, T, x_len = 32, 4, 41, torch.tensor([41, 29, 5, 36], dtype=torch.int32)
    out_len = (x_len + k - 1) // k
    cfg = _config(latency_control=(Nc, Nr), time_reduction=k)
    state = _sized_state(cfg, 1)
    x = omodel.synthetic_batch(B, T, V, Lmin=3, Lmax=9, seed=0, ragged=True)[0]
    labels, l_len = _labels(k)
    valid = (lambda tbv: [tbv[:n, b] for b, n in enumerate(out_len.tolist())])

    def run(variant):
        ref = lc.oracle(state, cfg, variant, torch.float64)
        logits = ref(x, x_len)
        omodel.ctc_mean_loss(logits, labels, out_len, l_len).backward()
        return valid(logits.detach()), {name: p.grad.clone() for name, p in ref.p.items() if name.startswith("rnn_blocks")}

    want, want_grad = run(None)
    assert len(want_grad) == 8
    far = {}
    for variant in lc.MUTANTS:
        logits, grad = run(variant)
        if variant == "right_context_gradient":
            assert _rel(logits, want) == 0.0
            far[variant] = (max(_rel([grad[name]], [want_grad[name]]) for name in grad), GRADIENT_BAR[k])
        else:
            far[variant] = (_rel(logits, want), FORWARD_BAR[k])
    print("latency control (%d, %d) k=%d: mutants at %s" % (Nc, Nr, k, {name: "%.3e (bar %.3e)" % v for name, v in far.items()}))
    for variant, (distance, bar) in far.items():
        assert distance >= 5 * bar, (variant, distance, bar)
