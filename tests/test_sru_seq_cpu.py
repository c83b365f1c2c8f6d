"""The SRU sequence layer's float64 restatement (tests/sru_seq_reference.py) pinned on the CPU, and the model plan for rnn="sru".

The restatement is what tests/test_sru_seq_gpu.py and tests/test_sru_model_gpu.py hold the kernels to, so it is pinned first: to the
reference's own forward (tests/golden/sru.npz, oracle.nn.sru_fwd), to finite differences, and to the properties the header states.
The golden file holds the float32 results of the reference's float32 ``forward_cpu``: the float64 restatement agrees with
``oracle.nn.sru_fwd`` in float64 to 1e-12 and with the stored float32 arrays to what float32 storage allows (the bar of
tests/test_oracle_misc.py::test_sru_forward_matches_reference on the same file, rtol 1e-5 / atol 1e-6)."""
import os

import numpy as np
import pytest

import sru_seq_reference as R
from oracle import nn as onn


def _case(seed, T, B, I, D, ndir, scale=0.5):
    rs = np.random.RandomState(seed)
    k = 3 if I == D else 4
    return dict(x=rs.randn(T, B, I), W=rs.randn(ndir, k * D, I) * scale, bias=rs.randn(ndir, 2 * D) * 0.3, cx=rs.randn(ndir, B, D),
                gy=rs.randn(T, B, D), dcy=rs.randn(ndir, B, D))


# ------------------------------------------------------------------------------------------------ the reference's own forward
@pytest.mark.parametrize("name", ["tanh", "linear"])
def test_restatement_is_the_reference_forward(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "sru.npz"))
    assert np.all(g[name + ".mask"] == 1)           # (the sequence layer has no per-(b, d) mask)
    X, W, Bias, c0 = (g["%s.%s" % (name, k)].astype(np.float64) for k in ("X", "W", "B", "c0"))
    use_tanh = bool(g[name + ".use_tanh"])
    y, C, cy = R.layer_fwd(X.transpose(2, 0, 1), W[None], Bias[None], c0[None], None, use_tanh)
    y, C = y.transpose(1, 2, 0), C[0].transpose(1, 2, 0)
    H, Co, cT = onn.sru_fwd(X, W, Bias, c0, use_tanh)
    for mine, theirs in ((y, H), (C, Co), (cy[0], cT)):
        assert np.abs(mine - theirs).max() <= 1e-12
    for mine, key in ((y, "H"), (C, "C"), (cy[0], "cT")):
        np.testing.assert_allclose(mine, g["%s.%s" % (name, key)], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ backward by finite differences
@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("I", [4, 5])
@pytest.mark.parametrize("use_tanh", [True, False])
def test_backward_matches_central_differences(ndir, I, use_tanh):
    """Central differences at two steps h and h / 2: their truncation errors are e and e / 4, so |fd(h) - fd(h / 2)| = 3 e / 4 is what
    was observed of it and bounds the error of fd(h / 2) (e / 4) three times over; the bar is that observed difference plus the
    float64 round-off of a difference quotient (2^-52 |loss| / h)."""
    T, B, D = 7, 3, 4
    c = _case(11 + ndir + I, T, B, I, D, ndir)
    x_len = [7, 0, 4]
    args = [c["x"], c["W"], c["bias"], c["cx"]]

    def loss(a):
        y, _, cy = R.layer_fwd(a[0], a[1], a[2], a[3], x_len, use_tanh)
        return (y * c["gy"]).sum() + (cy * c["dcy"]).sum()
    grads = R.layer_bwd(c["x"], c["W"], c["bias"], c["cx"], x_len, c["gy"], c["dcy"], use_tanh)
    rs = np.random.RandomState(5)
    scale = abs(loss(args)) + 1.0
    for which, (arr, grad) in enumerate(zip(args, grads)):
        picks = [tuple(rs.randint(s) for s in arr.shape) for _ in range(12)]
        if which == 0:
            picks += [(5, 2, 0), (0, 1, 1)]         # padding of utterance 2, an utterance without frames: exactly no gradient
        for idx in picks:
            fd = []
            for h in (2e-4, 1e-4):
                a = [q.copy() for q in args]
                a[which][idx] += h
                up = loss(a)
                a[which][idx] -= 2 * h
                fd.append((up - loss(a)) / (2 * h))
            bar = abs(fd[0] - fd[1]) + 2.0 ** -52 * scale / 1e-4 * 4
            assert abs(fd[1] - grad[idx]) <= bar, (which, idx, fd, grad[idx], bar)
    assert np.all(grads[0][4:, 2] == 0) and np.all(grads[0][:, 1] == 0)
    assert np.array_equal(grads[3][:, 1], c["dcy"][:, 1])       # x_len = 0: dcx = dcy


# ------------------------------------------------------------------------------------------------ the stated properties
def _same(a, b):
    """equal up to the last places of float64: the projection of a slice or of a flipped block is another BLAS call, whose sums may
    round differently (values are O(1), sums of <= 12 products)"""
    return np.abs(np.nan_to_num(a) - np.nan_to_num(b)).max() <= 1e-13


@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("I", [6, 9])
def test_ragged_batch_equals_every_utterance_alone(ndir, I):
    T, B, D = 9, 4, 6
    c = _case(3, T, B, I, D, ndir)
    x_len = [9, 0, 1, 5]
    y, C, cy = R.layer_fwd(c["x"], c["W"], c["bias"], c["cx"], x_len)
    for b, n in enumerate(x_len):
        assert np.all(y[n:, b] == 0)                                     # the padding is exactly 0
        if n == 0:
            assert np.array_equal(cy[:, b], c["cx"][:, b])               # x_len = 0 leaves cx untouched
            continue
        ya, Ca, cya = R.layer_fwd(c["x"][:n, b:b + 1], c["W"], c["bias"], c["cx"][:, b:b + 1])
        assert _same(y[:n, b], ya[:, 0]) and _same(cy[:, b], cya[:, 0]) and _same(C[:, :n, b], Ca[:, :, 0])


def _flip(a, x_len):
    """every utterance's own frames in reverse order, the padding where it was"""
    out = np.zeros_like(a)
    for b, n in enumerate(x_len):
        out[:n, b] = a[:n, b][::-1]
    return out


@pytest.mark.parametrize("I", [5, 8])
def test_direction_one_is_direction_zero_on_the_flipped_utterance(I):
    T, B, D = 8, 3, 5
    c = _case(4, T, B, I, D, 2)
    x_len = [8, 3, 6]
    y, C, cy = R.layer_fwd(c["x"], c["W"], c["bias"], c["cx"], x_len)
    y0, C0, cy0 = R.layer_fwd(c["x"], c["W"][:1], c["bias"][:1], c["cx"][:1], x_len)
    # direction 1's parameters as the only (forward) direction of a layer, on the flipped utterances
    y1, C1, cy1 = R.layer_fwd(_flip(c["x"], x_len), c["W"][1:], c["bias"][1:], c["cx"][1:], x_len)
    assert _same(cy[0], cy0[0]) and _same(cy[1], cy1[0])
    assert _same(C[1], _flip(np.nan_to_num(C1[0]), x_len))
    assert _same(y, y0 + _flip(y1, x_len))


@pytest.mark.parametrize("I", [5, 7])
def test_pieces_with_the_state_carried_equal_the_whole(I):
    T, B, D = 10, 3, 5
    c = _case(6, T, B, I, D, 1)
    x_len = np.array([10, 4, 7])
    y, _, cy = R.layer_fwd(c["x"], c["W"], c["bias"], c["cx"], x_len)
    state, rows = c["cx"], []
    for lo, hi in ((0, 3), (3, 4), (4, 10)):
        n = np.clip(x_len - lo, 0, hi - lo)
        yp, _, state = R.layer_fwd(c["x"][lo:hi], c["W"], c["bias"], state, n)
        rows.append(yp)
    assert _same(np.concatenate(rows), y) and _same(state, cy)
    assert np.array_equal(state[:, 1], R.layer_fwd(c["x"][:4], c["W"], c["bias"], c["cx"], [4, 4, 4])[2][:, 1])    # frozen after frame 3


# ------------------------------------------------------------------------------------------------ the caps tell right from wrong
MUTANT_FACTOR = 50.0


@pytest.mark.parametrize("mutant, I, ndir", [("thaw", 8, 1), ("thaw", 8, 2), ("reverse_T", 8, 2), ("highway_x", 12, 1), ("highway_x", 6, 2)])
def test_mutants_are_far_outside_the_gpu_caps(mutant, I, ndir):
    """The GPU caps are slack x (error shape) + half a unit of the stored format, slack <= 2 (tests/test_sru_seq_gpu.py asserts that the
    measured slack is; here the largest is taken).  Every mutant puts at least one element of y or cy beyond MUTANT_FACTOR times its cap
    -- measured: reverse_T 2.3e4, highway_x 4.5e4 and 3.1e5; thaw writes into the padding, where the cap is that of an exact zero."""
    T, B, D = 12, 3, 8
    c = _case(8, T, B, I, D, ndir)
    x_len = [12, 5, 9]
    U = R.project(c["x"], c["W"])
    y, C, cy, (Ey, EC, Ecy) = R.scan_fwd(U, c["x"], c["bias"], c["cx"], x_len, bounds=True)
    ym, Cm, cym = R.scan_fwd(U, c["x"], c["bias"], c["cx"], x_len, mutant=mutant)
    cap_y = 2.0 * Ey + R.half_unit(np.abs(y) + 2.0 * Ey)
    cap_c = 2.0 * Ecy + R.half_unit(cy, 23)
    worst = max((np.abs(ym - y) / cap_y).max(), (np.abs(cym - cy) / cap_c).max())
    print("mutant %s (I = %d, ndir = %d): %.1e caps off" % (mutant, I, ndir, worst))
    assert worst >= MUTANT_FACTOR
    # and the restatement itself evaluated in float32 stays inside
    y32, _, cy32 = _float32_scan(U, c["x"], c["bias"], c["cx"], x_len)
    assert np.all(np.abs(y32 - y) <= cap_y) and np.all(np.abs(cy32 - cy) <= cap_c)


def _float32_scan(U, x, bias, cx, x_len):
    """the forward scan in float32 arithmetic on the CPU (numpy's own exp and division)"""
    f32 = np.float32
    U, x, bias, cx = U.astype(f32), x.astype(f32), bias.astype(f32), cx.astype(f32)
    T, B, ndir, k, D = U.shape
    bias = bias.reshape(ndir, 2, D)
    y = np.zeros((T, B, D), dtype=f32)
    cy = cx.copy()
    sig = lambda a: (f32(1) / (f32(1) + np.exp(-a))).astype(f32)
    for d in range(ndir):
        for b, n in enumerate(x_len):
            c = cx[d, b]
            for t in (range(n) if d == 0 else range(n - 1, -1, -1)):
                f, r = sig(U[t, b, d, 1] + bias[d, 0]), sig(U[t, b, d, 2] + bias[d, 1])
                c = f * (c - U[t, b, d, 0]) + U[t, b, d, 0]
                xh = x[t, b] if k == 3 else U[t, b, d, 3]
                y[t, b] += r * (np.tanh(c) - xh) + xh
            cy[d, b] = c
    return y.astype(np.float64), None, cy.astype(np.float64)


# ------------------------------------------------------------------------------------------------ the model plan
def _config(**kw):
    from asr.model import ds2
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers = 32, 16, 64, 32, 2
    for key, value in kw.items():
        setattr(cfg, key, value)
    return cfg


def test_the_field_defaults_to_gru_and_a_gru_model_is_what_it_was():
    from asr import nn
    from asr.model import ds2
    assert ds2.Configuration.FIELDS["rnn"] == "gru"
    cfg = _config()
    del cfg.rnn                                     # a configuration from before the field
    for model in (ds2.Model(cfg), ds2.Model(_config()), ds2.Model(_config(rnn="gru"))):
        assert not hasattr(model, "rnn")
        names = [n for n, _ in model.named_parameters()]
        assert [n for n in names if n.startswith("rnn_blocks.")] == [
            "rnn_blocks._sequential_%d.%s" % (i, p) for i in (0, 2) for p in ("w_ih", "w_hh", "b_ih", "b_hh")]
        assert all(type(layer) is nn.BiGRU for layer in model.rnn_blocks.layers if hasattr(layer, "w_ih"))
        assert list(model.column_permutations()) == ["rnn_blocks._sequential_0.w_ih"]
        assert not any(isinstance(m, (nn.SeqSRU, nn.BiSeqSRU)) for m in model.modules())


def test_an_sru_model_holds_sru_layers_and_names_its_first_weight():
    from asr import nn
    from asr.model import ds2
    for bidirectional, kind in ((True, nn.BiSeqSRU), (False, nn.SeqSRU)):
        model = ds2.Model(_config(rnn="sru", bidirectional=bidirectional, time_reduction=2))
        layers = [layer for layer in model.rnn_blocks.layers if hasattr(layer, "W")]
        assert len(layers) == 2 and all(type(layer) is kind and layer.out_size == 64 for layer in layers)
        assert [n for n, _ in model.named_parameters() if n.startswith("rnn_blocks.")] == [
            "rnn_blocks._sequential_%d.%s" % (i, p) for i in (0, 2) for p in ("W", "B")]
        assert model.column_permutations() == {"rnn_blocks._sequential_0.W": (model._merged[0], model._merged[1] * 2)}
        assert tuple(layers[0].B.shape) == (2 if bidirectional else 1, 128)
    layer = nn.SeqSRU(64)
    layer._initialize_params(64)
    assert layer.k == 3 and tuple(layer.W.shape) == (1, 192, 64)
    layer = nn.BiSeqSRU(48, 64)
    assert layer.k == 4 and tuple(layer.W.shape) == (2, 256, 48)


def test_refusals_at_construction():
    from asr.model import ds2
    with pytest.raises(ValueError, match="latency_control"):
        ds2.Model(_config(rnn="sru", latency_control=(8, 4)))
    for bad in ("lstm", "SRU", None, 1):
        with pytest.raises(ValueError, match="rnn must be"):
            ds2.Model(_config(rnn=bad))


def test_stream_plan_for_the_sru_stack():
    from asr.model import ds2
    from asr.model.stream import stream_plan
    plan = stream_plan(ds2.Model(_config(rnn="sru", bidirectional=False, lookahead=3, time_reduction=2)))
    states = [e for e in plan["layers"] if e["kind"] == "state"]
    assert states == [{"kind": "state", "H": 64, "index": 0, "cell": "sru"}, {"kind": "state", "H": 64, "index": 2, "cell": "sru"}]
    assert plan["delay"] == 3 and plan["time_reduction"] == 2
    assert [e["kind"] for e in plan["layers"]] == ["context", "context", "stack", "state", "state", "lookahead"]
    gru = stream_plan(ds2.Model(_config(bidirectional=False)))
    assert [e for e in gru["layers"] if e["kind"] == "state"] == [{"kind": "state", "H": 64, "index": 0}, {"kind": "state", "H": 64, "index": 2}]
    with pytest.raises(ValueError, match="bidirectional"):
        stream_plan(ds2.Model(_config(rnn="sru")))
