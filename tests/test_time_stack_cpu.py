"""Time reduction by frame stacking, host side: the numpy restatement of csrc/time_stack.hip (tests/time_stack_reference.py)
against a plain triple loop, the adjoint identity, push = one-shot under random cut schedules, and what the model, the plan and
the data side do with ``time_reduction``.  No GPU."""
import numpy as np
import pytest
import torch

import time_stack_reference as ts

KS = [1, 2, 3, 4, 8]


def _lengths(T, B, rng):
    """0 / 1 / T / ragged / above T (clamped) and NULL"""
    return [None, np.zeros(B, np.int32), np.full(B, min(1, T), np.int32), np.full(B, T, np.int32),
            rng.integers(0, T + 1, size=B).astype(np.int32), np.full(B, T + 5, np.int32), np.full(B, -3, np.int32)]


def _loop_fwd(x, k, x_len):
    T, B, R = x.shape
    G = (T + k - 1) // k
    y = np.zeros((G, B, k * R), dtype=x.dtype)
    y_len = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = T if x_len is None else min(max(int(x_len[b]), 0), T)
        y_len[b] = (n + k - 1) // k
        for g in range(G):
            for j in range(k):
                for r in range(R):
                    if g * k + j < n:
                        y[g, b, j * R + r] = x[g * k + j, b, r]
    return y, y_len


def _loop_bwd(gy, k, T, x_len):
    G, B, KR = gy.shape
    R = KR // k
    dx = np.full((T, B, R), -99, dtype=gy.dtype)
    for t in range(T):
        for b in range(B):
            n = T if x_len is None else min(max(int(x_len[b]), 0), T)
            for r in range(R):
                dx[t, b, r] = gy[t // k, b, (t % k) * R + r] if t < n else 0
    return dx


@pytest.mark.parametrize("k", KS)
def test_restatement_against_a_triple_loop(k):
    rng = np.random.default_rng(k)
    B, R = 3, 4
    for T in sorted({0, 1, max(k - 1, 0), k, k + 1, 2 * k + 1}):
        x = rng.integers(1, 1000, size=(T, B, R)).astype(np.int16)
        for x_len in _lengths(T, B, rng):
            y, y_len = ts.fwd(x, k, x_len)
            want, want_len = _loop_fwd(x, k, x_len)
            assert y.shape == ((T + k - 1) // k, B, k * R) and np.array_equal(y, want), (T, x_len)
            assert y_len.dtype == np.int32 and np.array_equal(y_len, want_len)
            gy = rng.integers(1, 1000, size=y.shape).astype(np.int16)
            assert np.array_equal(ts.bwd(gy, k, T, x_len), _loop_bwd(gy, k, T, x_len)), (T, x_len)
    if k == 1:                                  # a plain copy
        x = rng.integers(1, 1000, size=(5, B, R)).astype(np.int16)
        assert np.array_equal(ts.fwd(x, 1)[0], x) and np.array_equal(ts.bwd(x, 1, 5), x)


@pytest.mark.parametrize("k", KS)
def test_backward_is_the_exact_adjoint_of_forward(k):
    rng = np.random.default_rng(10 + k)
    B, R = 4, 5
    for T in (1, k, k + 1, 2 * k + 1, 19):
        for x_len in _lengths(T, B, rng):
            x = rng.integers(-50, 50, size=(T, B, R)).astype(np.int64)
            gy = rng.integers(-50, 50, size=((T + k - 1) // k, B, k * R)).astype(np.int64)
            assert int((gy * ts.fwd(x, k, x_len)[0]).sum()) == int((ts.bwd(gy, k, T, x_len) * x).sum())


def _run_schedule(k, B, R, seqs, cuts, rng):
    """feed slot b its sequence seqs[b] in the per-step shares cuts[step][b]; -> the emitted groups per slot and the stacker"""
    st = ts.Stacker(k, B, R, dtype=np.int16)
    pos = [0] * B
    out = [[] for _ in range(B)]
    for step, n in enumerate(cuts):
        Tc = max(max(n), 1)
        chunk = rng.integers(1, 1000, size=(Tc, B, R)).astype(np.int16)             # rows beyond n[b]: never used
        for b in range(B):
            chunk[:n[b], b] = seqs[b][pos[b]:pos[b] + n[b]]
        before, m_before = st.state.copy(), st.m.copy()
        y, emit = st.push(chunk, np.array(n, dtype=np.int32))
        assert y.shape == ((k - 1 + Tc + k - 1) // k, B, k * R)
        for b in range(B):
            pos[b] += n[b]
            assert emit[b] == (m_before[b] + n[b]) // k and st.m[b] == (m_before[b] + n[b]) % k
            if n[b] == 0:
                assert np.array_equal(st.state[:, b], before[:, b]) and st.m[b] == m_before[b]
            out[b].extend(y[:emit[b], b])
            assert not y[emit[b] + 1:, b].any()                                     # zeros behind the (partial) group
            assert len(out[b]) == pos[b] // k                                       # floor of the rows so far
    return st, out, pos


@pytest.mark.parametrize("k", KS)
def test_push_concatenates_to_the_one_shot_forward(k):
    rng = np.random.default_rng(100 + k)
    B, R = 5, 3
    for trial in range(6):
        lens = [int(v) for v in rng.integers(0, 4 * k + 6, size=B)]
        seqs = [rng.integers(1, 1000, size=(n, R)).astype(np.int16) for n in lens]
        left, cuts = list(lens), []
        while any(left):
            kind = trial % 3
            n = []
            for b in range(B):
                top = [left[b], 1, max(k - 2, 0), k + 1 + int(rng.integers(0, 3))][int(rng.integers(0, 4))] if kind else 1
                take = min(left[b], int(rng.integers(0, top + 1)) if kind != 2 else top)
                n.append(take)
            if not any(n):
                n = [min(v, 1) for v in left]
            left = [a - c for a, c in zip(left, n)]
            cuts.append(n)
        st, out, pos = _run_schedule(k, B, R, seqs, cuts, rng)
        assert pos == lens
        y, emit = st.push(None, None, flush=np.ones(B, dtype=np.int32))             # the flush at the end
        assert y.shape == ((1 if k > 1 else 0), B, k * R)
        for b in range(B):
            assert emit[b] == (1 if lens[b] % k else 0)
            out[b].extend(y[:emit[b], b])
            want, want_len = ts.fwd(seqs[b][:, None, :], k, np.array([lens[b]]))
            assert len(out[b]) == (lens[b] + k - 1) // k == want_len[0]
            if out[b]:
                assert np.array_equal(np.stack(out[b]), want[:, 0])
        assert not st.state.any() and not st.m.any()


@pytest.mark.parametrize("k", [2, 3, 8])
def test_push_flush_and_restart_in_mid_stream(k):
    """slot 1 is flushed after its first utterance and fed a second one while the others go on; a reset drops a slot's rows"""
    rng = np.random.default_rng(200 + k)
    B, R = 3, 2
    first, second = 2 * k + 1, k + 2
    total = first + second
    seqs = [rng.integers(1, 1000, size=(total, R)).astype(np.int16) for _ in range(B)]
    st = ts.Stacker(k, B, R)
    out = [[] for _ in range(B)]

    def feed(lo, hi):
        pos = lo
        while pos < hi:
            Tc = min(int(rng.integers(1, k + 3)), hi - pos)
            chunk = np.stack([s[pos:pos + Tc] for s in seqs], axis=1)
            y, emit = st.push(chunk)
            for b in range(B):
                out[b].extend(y[:emit[b], b])
            pos += Tc
    feed(0, first)
    mask = np.array([0, 1, 0], dtype=np.int32)
    before = st.state.copy()
    y, emit = st.push(None, None, flush=mask)
    assert list(emit) == [0, 1 if first % k else 0, 0] and not y[:, 0].any() and not y[:, 2].any()
    assert np.array_equal(st.state[:, 0], before[:, 0]) and np.array_equal(st.state[:, 2], before[:, 2]) and st.m[1] == 0
    out[1].extend(y[:emit[1], 1])
    feed(first, total)
    y, emit = st.push(None, None, flush=np.ones(B, dtype=np.int32))
    for b in range(B):
        out[b].extend(y[:emit[b], b])
    for b in (0, 2):
        assert np.array_equal(np.stack(out[b]), ts.fwd(seqs[b][:, None], k)[0][:, 0])
    two = np.concatenate([ts.fwd(seqs[1][:first, None], k)[0][:, 0], ts.fwd(seqs[1][first:, None], k)[0][:, 0]])
    assert np.array_equal(np.stack(out[1]), two)
    y, emit = st.push(None, None, flush=np.ones(B, dtype=np.int32))                 # flushing empty slots emits nothing
    assert not emit.any() and not y.any()
    st.push(seqs[0][:k - 1, None].repeat(B, axis=1))
    assert list(st.m) == [k - 1] * B
    st.reset(np.array([1, 0, 0]))
    assert list(st.m) == [0, k - 1, k - 1] and not st.state[:, 0].any() and st.state[:, 1].any()
    st.reset()
    assert not st.m.any() and not st.state.any()


# --------------------------------------------------------------------------------------------------------- model, plan, data
def _ds2_small(**fields):
    from asr.model import ds2
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers = 17, 8, 32, 16, 2
    for name, value in fields.items():
        assert hasattr(cfg, name), name
        setattr(cfg, name, value)
    return cfg, ds2.Model(cfg)


@pytest.mark.parametrize("k", [2, 3])
def test_plan_gains_one_stack_entry(k):
    from asr.model.stream import stream_plan
    cfg, model = _ds2_small(bidirectional=False, lookahead=5, time_reduction=k)
    plan = stream_plan(model)
    assert plan["time_reduction"] == k and plan["delay"] == 5
    assert [e["kind"] for e in plan["layers"]] == ["context", "context", "stack", "state", "state", "lookahead"]
    # the conv stack leaves 8 channels x 6 rows: 40 -> conv 38 -> pool 3: 13 -> conv 11 -> pool 2: 6
    assert model._merged == (8, 6)
    assert plan["layers"][2] == {"kind": "stack", "K": k - 1, "R": 48, "k": k}
    cfg0, same = _ds2_small(bidirectional=False, lookahead=5)
    assert [e for e in plan["layers"] if e["kind"] != "stack"] == stream_plan(same)["layers"]


def test_plan_at_k_1_is_the_plan_without_the_field():
    from asr.model import ds2
    from asr.model.stream import stream_plan
    cfg, plain = _ds2_small(bidirectional=False, lookahead=2)
    cfg1, one = _ds2_small(bidirectional=False, lookahead=2, time_reduction=1)
    assert stream_plan(one) == stream_plan(plain) and sorted(stream_plan(one)) == ["delay", "layers"]
    assert not hasattr(one, "time_stack") and one.time_reduction == 1 and ds2.Configuration.FIELDS["time_reduction"] == 1
    assert one.column_permutations() == {"rnn_blocks._sequential_0.w_ih": (8, 6)}


def test_refusals():
    from asr import _ops, nn
    from asr.model.stream import AcousticStream, stream_plan
    assert _ops.TIME_STACK_MAX == 8
    for bad in (0, -1, 9, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            _ds2_small(time_reduction=bad)
    for bad in (0, 9, 1.5):
        with pytest.raises(ValueError):
            nn.TimeStack(bad)
    assert nn.TimeStack(8).k == 8
    cfg, model = _ds2_small(time_reduction=2)                                        # bidirectional: still no stream
    with pytest.raises(ValueError):
        stream_plan(model)
    with pytest.raises(ValueError):
        AcousticStream(model, 2, device="cpu")
    cfg, model = _ds2_small(bidirectional=False, time_reduction=2, ndim_conv=3)      # 6 rows x 3 channels: no 16-byte lanes
    with pytest.raises(ValueError):
        AcousticStream(model, 2, device="cpu")


def test_time_reduction_moves_no_parameter_name():
    for bidirectional in (False, True):
        cfg, plain = _ds2_small(bidirectional=bidirectional)
        cfg3, three = _ds2_small(bidirectional=bidirectional, time_reduction=3)
        assert list(three.state_dict().keys()) == list(plain.state_dict().keys())
        assert isinstance(three.time_stack.k, int) and three.time_stack.k == 3 and three.time_reduction == 3
        assert three.column_permutations() == {"rnn_blocks._sequential_0.w_ih": (8, 18)}


def test_output_length():
    cfg, model = _ds2_small(time_reduction=3)
    assert [model.output_length(n) for n in (0, 1, 2, 3, 4, 41)] == [0, 1, 1, 1, 2, 14]
    assert model.output_length([41, 29, 5, 36, 0]) == [14, 10, 2, 12, 0]
    t = model.output_length(torch.tensor([41, 29, 5, 36, 0], dtype=torch.int32))
    assert t.dtype == torch.int32 and t.tolist() == [14, 10, 2, 12, 0]
    assert model.output_length(np.array([41, 3])).tolist() == [14, 1]
    cfg1, one = _ds2_small()
    assert one.output_length(41) == 41 and one.output_length([7, 8]) == [7, 8]


def test_minibatch_labels_are_cut_against_the_reduced_length():
    from asr.data.processing import Processor, truncate_labels_for_ctc

    class Self(object):
        using_delta = True
        using_delta_delta = True
        num_mel_filters = 40
        device = "cpu"
    ids = {"ア": 1, "イ": 2, "ウ": 3, "アイ": 4, "イウ": 5}
    sents = ["アイウアイウ", "アイウ", "アア"]
    lens = [13, 13, 7]
    feats = [tuple(np.zeros((40, n), dtype=np.float32) for _ in range(3)) for n in lens]
    args = (Self(), feats, sents, max(lens), 6, ids, 0)
    x, xl, t, tl, bg = Processor.features_to_minibatch(*args)
    x1, xl1, t1, tl1, bg1 = Processor.features_to_minibatch(*args, time_reduction=1)
    assert tl == [6, 3, 2] and tl1 == tl and np.array_equal(t, t1) and np.array_equal(bg, bg1) and xl1 == xl == lens
    for k in (2, 3, 4):
        xk, xlk, tk, tlk, bgk = Processor.features_to_minibatch(*args, time_reduction=k)
        assert xlk == lens and torch.equal(xk, x)                                   # the input-rate lengths, the same features
        for i, s in enumerate(sents):
            uni = [ids[c] for c in s]
            keep = len(truncate_labels_for_ctc(uni, uni, -(-lens[i] // k))[0])
            assert tlk[i] == keep and list(tk[i, :keep]) == uni[:keep] and not tk[i, keep:].any()
    assert Processor.features_to_minibatch(*args, time_reduction=2)[3] == [3, 3, 0]
    # by hand: 7 frames hold (7 - 0 - 1) // 2 = 3 of the 6 tokens and all 3 of "アイウ" (2 * 3 + 1 = 7); "アア" counts 2 repeats (the
    # cyclic comparison), needs 7 frames and gets 4: (4 - 2 - 1) // 2 = 0
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            Processor.features_to_minibatch(*args, time_reduction=bad)
