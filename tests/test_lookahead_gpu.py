"""The lookahead convolution kernels (csrc/lookahead.hip) element by element against the float64 restatement
(tests/lookahead_reference.py, itself checked in tests/test_lookahead_cpu.py) on the device's own 16-bit inputs.

Caps (derived, not tuned; u32 = 2^-24, u_act = the activation format's unit roundoff, 2^-8 for bfloat16):
  forward   an output is a chain of tau + 1 float32 fused multiply-adds (products of two 16-bit values and a float32 weight are not
            exact, each fma rounds once) and one rounding to the activation format at the store:
                |y_dev - y| <= (tau + 2) u32 sum_j |W_j x_{t+j}| + u_act |y|
  dx        the mirrored chain:  (tau + 2) u32 sum_j |W_j gy_{t-j}| + u_act |dx|
  dW        dW[d, j] adds n_j = sum_b max(0, len_b - j) products gy x (a product of two 16-bit values is exact in float32; the
            fma adds it with one rounding).  The kernels add them in chains per workgroup, add the workgroups' partial sums in
            order and add the total once to the gradient buffer g0.  An addition with a zero operand is exact, and every other
            addition of the chains and of the partial sums consumes one of the n_j terms or one non-zero partial sum (of which
            there are at most n_j chains' worth, each started by an exact first addition): at most n_j inexact additions, one
            more for g0.  A term passes through at most that many roundings, so with k = n_j + 1
                |dW_dev - (g0 + dW)| <= k u32 / (1 - k u32) (sum_{t,b} |gy x| + |g0|)
Beyond an utterance's length the outputs are exactly 0; nothing is written outside the output; two runs give the same bits."""
import numpy as np
import pytest
import torch

import lookahead_reference as ref

pytestmark = pytest.mark.gpu
F32 = torch.float32
U32 = 2.0 ** -24


def _ops():
    from asr import _ops
    return _ops


def _u_act():
    return 2.0 ** -8 if _ops().BF16 == torch.bfloat16 else 2.0 ** -11


TAU_MAX, TT = 96, 64


def test_the_limits_are_the_header_s():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert int(re.search(r"#define ASR_LOOKAHEAD_MAX_TAU (\d+)", text).group(1)) == TAU_MAX == _ops().LOOKAHEAD_MAX_TAU >= 80
    assert int(re.search(r"#define ASR_LOOKAHEAD_TIME_TILE (\d+)", text).group(1)) == TT == _ops().LOOKAHEAD_TIME_TILE


def _lengths(B, T, tau, variant):
    if B == 1:
        return None if variant == 0 else [T // 2]
    return [T, min(1, T), 0] if variant == 0 else [max(T - tau // 2 - 1, 0), T, (2 * T) // 3]


def _guarded(shape, dtype, device, fill):
    """a tensor of `shape` inside a larger buffer of `fill`: (view, check) -- check() asserts that nothing outside was written"""
    n = int(np.prod(shape))
    pad = 4096
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=device)
    view = buf[pad:pad + n].view(shape)

    def check():
        assert bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all()), "written outside the buffer"
    return view, check


def _times(tau):
    return sorted({t for t in (1, tau, tau + 1, TT - 1, TT, TT + 1, 2 * TT + tau + 1) if t >= 1})


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [8, 32, 40, 520])
@pytest.mark.parametrize("tau", [0, 1, 2, 7, TAU_MAX])
def test_forward_and_backward_against_float64(device, tau, D, B):
    ops = _ops()
    g = torch.Generator().manual_seed(1000 * tau + 10 * D + B)
    u_act = _u_act()
    worst = {"y": 0.0, "dx": 0.0, "dW": 0.0}
    times = _times(tau)
    for i, T in enumerate(times):
        for variant in ((0, 1) if T == times[-1] else (i % 2,)):        # (both length sets at the longest T, alternating below)
            lengths = _lengths(B, T, tau, variant)
            x = torch.randn((T, B, D), generator=g).to(device, ops.BF16)
            gy = torch.randn((T, B, D), generator=g).to(device, ops.BF16)
            W = torch.randn((D, tau + 1), generator=g).to(device)
            g0 = torch.randn((D, tau + 1), generator=g).to(device)
            x_len = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=device)
            y, check_y = _guarded((T, B, D), ops.BF16, device, 7.0)
            ops.lookahead_fwd(x, W, x_len, out=y)
            dW = g0.clone()
            dx = ops.lookahead_bwd(gy, x, W, x_len, dW)
            dW2 = g0.clone()
            dx2 = ops.lookahead_bwd(gy, x, W, x_len, dW2)
            torch.cuda.synchronize()
            check_y()
            assert torch.equal(dW, dW2) and torch.equal(dx, dx2), "two runs of the backward differ"
            xh, gh, Wh = x.double().cpu().numpy(), gy.double().cpu().numpy(), W.double().cpu().numpy()
            yr, ya = ref.forward(xh, Wh, lengths), ref.forward_abs(xh, Wh, lengths)
            dxr, dWr = ref.backward(gh, xh, Wh, lengths)
            dxa, dWa = ref.backward_abs(gh, xh, Wh, lengths)
            yd, dxd, dWd = y.double().cpu().numpy(), dx.double().cpu().numpy(), dW.double().cpu().numpy()
            n = np.full((B,), T) if lengths is None else np.asarray(lengths)
            for b in range(B):
                assert np.all(yd[n[b]:, b] == 0) and np.all(dxd[n[b]:, b] == 0), "non-zero beyond the length"
            cap_y = (tau + 2) * U32 * ya + u_act * np.abs(yr)
            cap_dx = (tau + 2) * U32 * dxa + u_act * np.abs(dxr)
            k = (ref.dw_terms(T, B, tau, lengths) + 1).astype(np.float64)[None, :]
            g0h = g0.double().cpu().numpy()
            cap_dW = k * U32 / (1 - k * U32) * (dWa + np.abs(g0h))
            for name, dev, want, cap in (("y", yd, yr, cap_y), ("dx", dxd, dxr, cap_dx), ("dW", dWd, g0h + dWr, cap_dW)):
                err = np.abs(dev - want)
                bad = ~(err <= cap)
                assert not bad.any(), "%s: T=%d lengths=%s: %d elements outside the cap, worst %.3g x cap" % (
                    name, T, lengths, bad.sum(), float((err / np.maximum(cap, 1e-300))[bad].max()))
                live = cap > 0
                if live.any():
                    worst[name] = max(worst[name], float((err[live] / cap[live]).max()))
    print("lookahead tau=%d D=%d B=%d: worst error / cap  y %.3f  dx %.3f  dW %.3f" % (tau, D, B, worst["y"], worst["dx"], worst["dW"]))


def test_without_a_weight_gradient_and_without_an_input_gradient(device):
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    T, B, D, tau = 70, 2, 16, 3
    x = torch.randn((T, B, D), generator=g).to(device, ops.BF16)
    gy = torch.randn((T, B, D), generator=g).to(device, ops.BF16)
    W = torch.randn((D, tau + 1), generator=g).to(device)
    dW = torch.zeros_like(W)
    dx = ops.lookahead_bwd(gy, x, W, None, dW)
    assert torch.equal(ops.lookahead_bwd(gy, None, W, None, None), dx)
    dW2 = torch.zeros_like(W)
    assert ops.lookahead_bwd(gy, x, W, None, dW2, need_dx=False) is None and torch.equal(dW, dW2)


@pytest.mark.parametrize("tau,D", [(TAU_MAX + 1, 16), (3, 12)])
def test_refusals_write_nothing(device, tau, D):
    from asr import _lib
    ops = _ops()
    T, B = 5, 2
    x = torch.ones((T, B, D), dtype=ops.BF16, device=device)
    W = torch.ones((D, tau + 1), dtype=F32, device=device)
    y, check_y = _guarded((T, B, D), ops.BF16, device, 7.0)
    dx, check_dx = _guarded((T, B, D), ops.BF16, device, 7.0)
    dW, check_dW = _guarded((D, tau + 1), F32, device, 7.0)
    ws = torch.full((1 << 16,), 7.0, dtype=F32, device=device)
    lib = _lib.lib()
    assert lib.asr_lookahead_ws_bytes(T, B, D, tau) == 0
    assert lib.asr_lookahead_fwd(_lib.stream(), x.data_ptr(), W.data_ptr(), None, y.data_ptr(), T, B, D, tau) == -3
    assert lib.asr_lookahead_bwd(_lib.stream(), x.data_ptr(), x.data_ptr(), W.data_ptr(), None, dx.data_ptr(), dW.data_ptr(),
                                 ws.data_ptr(), ws.numel() * 4, T, B, D, tau) == -3
    torch.cuda.synchronize()
    for t, check in ((y, check_y), (dx, check_dx), (dW, check_dW)):
        check()
        assert bool((t == 7.0).all())
    assert bool((ws == 7.0).all())
    with pytest.raises(_lib.AsrHipError):
        ops.lookahead_fwd(x, W)


@pytest.mark.parametrize("tau", [1, 7, 20])
def test_a_cut_sequence_gives_the_same_bits(device, tau):
    """the forward over [0, T) equals, bit for bit, the forward over any window [a, c) on the rows [a, c - tau)"""
    ops = _ops()
    g = torch.Generator().manual_seed(tau)
    T, B, D = 2 * TT + tau + 9, 3, 40
    x = torch.randn((T, B, D), generator=g).to(device, ops.BF16)
    W = torch.randn((D, tau + 1), generator=g).to(device)
    whole = ops.lookahead_fwd(x, W)
    for a, c in ((0, T), (1, T), (5, TT + 3), (TT - 1, TT + tau + 1), (TT, 2 * TT + tau), (17, 17 + tau + 1), (T - tau - 1, T)):
        part = ops.lookahead_fwd(x[a:c].contiguous(), W)
        assert torch.equal(part[:c - a - tau], whole[a:c - tau]), (a, c)
    # ... and the rows that do reach past the cut are what a zero future gives: the length rule
    x_len = torch.tensor([T - 4, TT, 3], dtype=torch.int32, device=device)
    ragged = ops.lookahead_fwd(x, W, x_len)
    for b, n in enumerate(x_len.tolist()):
        alone = ops.lookahead_fwd(x[:n, b:b + 1].contiguous(), W)
        assert torch.equal(alone[:, 0], ragged[:n, b]) and bool((ragged[n:, b] == 0).all())


def test_the_link_and_its_gradients(device):
    """nn.LookaheadConvolution: a fresh layer is the identity; its autograd function hands the kernels' dx and dW on"""
    from asr import nn
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    B, D, T, tau = 3, 24, 50, 4
    layer = nn.LookaheadConvolution(D, tau).to_gpu()
    assert tuple(layer.W.shape) == (D, tau + 1)
    x = torch.randn((B, D, T), generator=g).to(device)
    x_len = torch.tensor([T, 20, 0], dtype=torch.int32, device=device)
    p = x.permute(2, 0, 1).to(ops.BF16).contiguous()
    y = layer(x, x_len)
    live = (torch.arange(T, device=device)[:, None] < x_len[None, :])[:, :, None]
    assert tuple(y.shape) == (B, D, T) and torch.equal(y.permute(2, 0, 1), torch.where(live, p, torch.zeros_like(p)))
    with torch.no_grad():
        layer.W.copy_(torch.randn((D, tau + 1), generator=g).to(device))
    xg = x.clone().requires_grad_(True)
    y = layer(xg, x_len)
    gy = torch.randn((T, B, D), generator=g).to(device, ops.BF16)
    y.backward(gy.permute(1, 2, 0))
    dW = torch.zeros_like(layer.W.data)
    dx = ops.lookahead_bwd(gy, p, layer.W.data, x_len, dW)
    assert torch.equal(layer.W.grad, dW)
    assert torch.equal(xg.grad.permute(2, 0, 1), dx.float())
    lazy = nn.LookaheadConvolution(lookahead=2).to_gpu()
    assert torch.equal(lazy(x).permute(2, 0, 1), p) and tuple(lazy.W.shape) == (D, 3)
