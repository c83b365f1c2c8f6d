"""The float64 restatement of the lookahead convolution (tests/lookahead_reference.py) is what the GPU tests measure the kernels
against: here it is checked itself -- against a brute-force triple loop, its gradients against central differences, and tau = 0."""
import numpy as np
import pytest

import lookahead_reference as ref


def _case(seed, T, B, D, tau, ragged):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, B, D))
    W = rng.standard_normal((D, tau + 1))
    lengths = None
    if ragged:
        lengths = rng.integers(0, T + 1, size=B)
        lengths[0], lengths[-1] = T, 0
        if B > 2:
            lengths[1] = 1
    return x, W, lengths


def _brute(x, W, lengths):
    T, B, D = x.shape
    y = np.zeros((T, B, D))
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        for t in range(n):
            for d in range(D):
                y[t, b, d] = sum(W[d, j] * x[t + j, b, d] for j in range(W.shape[1]) if t + j < n)
    return y


@pytest.mark.parametrize("T,B,D,tau,ragged", [(7, 3, 4, 2, True), (5, 2, 3, 6, True), (6, 4, 2, 0, True), (9, 1, 5, 3, False),
                                              (1, 3, 2, 4, True)])
def test_forward_against_the_triple_loop(T, B, D, tau, ragged):
    x, W, lengths = _case(T * 31 + tau, T, B, D, tau, ragged)
    np.testing.assert_allclose(ref.forward(x, W, lengths), _brute(x, W, lengths), rtol=0, atol=1e-13)


def test_forward_ignores_what_lies_beyond_the_length():
    x, W, lengths = _case(5, 8, 4, 3, 2, True)
    y = ref.forward(x, W, lengths)
    x2 = x.copy()
    for b, n in enumerate(lengths):
        x2[n:, b] = 1e6
        assert np.all(y[n:, b] == 0)
    assert np.array_equal(ref.forward(x2, W, lengths), y)


@pytest.mark.parametrize("T,B,D,tau,ragged", [(7, 3, 3, 2, True), (6, 2, 2, 5, True), (8, 1, 3, 3, False)])
def test_gradients_against_central_differences(T, B, D, tau, ragged):
    x, W, lengths = _case(T * 17 + tau, T, B, D, tau, ragged)
    rng = np.random.default_rng(3)
    gy = rng.standard_normal(x.shape)
    dx, dW = ref.backward(gy, x, W, lengths)
    loss = lambda xx, ww: float((ref.forward(xx, ww, lengths) * gy).sum())
    h = 1e-6
    ndx, ndW = np.zeros_like(x), np.zeros_like(W)
    for idx in np.ndindex(*x.shape):
        e = np.zeros_like(x)
        e[idx] = h
        ndx[idx] = (loss(x + e, W) - loss(x - e, W)) / (2 * h)
    for idx in np.ndindex(*W.shape):
        e = np.zeros_like(W)
        e[idx] = h
        ndW[idx] = (loss(x, W + e) - loss(x, W - e)) / (2 * h)
    np.testing.assert_allclose(dx, ndx, rtol=0, atol=1e-7)
    np.testing.assert_allclose(dW, ndW, rtol=0, atol=1e-7)
    if lengths is not None:
        for b, n in enumerate(lengths):
            assert np.all(dx[n:, b] == 0)


def test_tau_zero_is_the_identity_times_the_first_tap():
    x, W, lengths = _case(11, 6, 3, 4, 0, True)
    live = (np.arange(6)[:, None] < np.asarray(lengths)[None, :])[:, :, None]
    assert np.array_equal(ref.forward(x, W, lengths), x * W[None, None, :, 0] * live)
    assert np.array_equal(ref.forward(x, np.ones((4, 1)), None), x)


def test_term_counts():
    assert ref.dw_terms(5, 3, 2, [5, 1, 0]).tolist() == [6, 4, 3]
    assert ref.dw_terms(4, 2, 1, None).tolist() == [8, 6]
