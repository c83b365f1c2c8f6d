"""float64 numpy restatement of the lookahead convolution (include/asr_hip.h: asr_lookahead_fwd / asr_lookahead_bwd) in the physical
(T, B, D) layout.  W (D, tau + 1); lengths (B) integers or None (= T).

    y[t, b, d]  = sum_j W[d, j] x[t + j, b, d]       x = 0 at and beyond len[b]; y = 0 there
    dx[t, b, d] = sum_j W[d, j] gy[t - j, b, d]      gy ignored at and beyond len[b]; dx = 0 there
    dW[d, j]    = sum_{t, b} gy[t, b, d] x[t + j, b, d]
"""
import numpy as np


def _live(T, B, lengths):
    n = np.full((B,), T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    return (np.arange(T)[:, None] < n[None, :]).astype(np.float64)[:, :, None]          # (T, B, 1)


def forward(x, W, lengths=None):
    x, W = np.asarray(x, dtype=np.float64), np.asarray(W, dtype=np.float64)
    T, B, D = x.shape
    live = _live(T, B, lengths)
    xm = x * live
    y = np.zeros_like(xm)
    for j in range(W.shape[1]):
        if j < T:
            y[:T - j] += W[None, None, :, j] * xm[j:]
    return y * live


def forward_abs(x, W, lengths=None):
    """sum_j |W_j x_{t+j}|: the magnitude the float32 accumulation error of an output scales with"""
    return forward(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(W, dtype=np.float64)), lengths)


def backward(gy, x, W, lengths=None):
    """-> (dx, dW)"""
    gy, x, W = (np.asarray(a, dtype=np.float64) for a in (gy, x, W))
    T, B, D = x.shape
    live = _live(T, B, lengths)
    gm, xm = gy * live, x * live
    dx = np.zeros_like(xm)
    dW = np.zeros_like(W)
    for j in range(W.shape[1]):
        if j < T:
            dx[j:] += W[None, None, :, j] * gm[:T - j]
            dW[:, j] = (gm[:T - j] * xm[j:]).sum(axis=(0, 1))
    return dx * live, dW


def backward_abs(gy, x, W, lengths=None):
    """the same sums over absolute values: (sum_j |W_j gy_{t-j}|, sum_{t,b} |gy_t x_{t+j}|)"""
    return backward(np.abs(np.asarray(gy, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64)),
                    np.abs(np.asarray(W, dtype=np.float64)), lengths)


def dw_terms(T, B, tau, lengths=None):
    """number of products that dW[:, j] sums: sum_b max(0, len[b] - j), per j"""
    n = np.full((B,), T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    return np.array([np.maximum(n - j, 0).sum() for j in range(tau + 1)], dtype=np.int64)
