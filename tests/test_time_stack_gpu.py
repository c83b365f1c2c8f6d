"""The frame-stacking kernels (csrc/time_stack.hip) bit for bit against their numpy restatement (tests/time_stack_reference.py,
whose semantics tests/test_time_stack_cpu.py checks): forward, backward and the streaming push, in buffers with NaN guard rows in
front and behind, compared on the raw 16-bit words."""
import numpy as np
import pytest
import torch

import time_stack_reference as ts

pytestmark = pytest.mark.gpu

GUARD = 2           # rows (of B * width 16-bit words) of NaN in front of and behind every buffer
NAN = 0x7FC1        # as int16: a NaN in bfloat16 (exponent 0xFF) and in IEEE half (exponent 0x1F) alike


class _Guarded:
    """(rows, B, width) int16 tensor, NaN-filled, inside a buffer with GUARD NaN rows on both sides"""

    def __init__(self, rows, B, width, device):
        self.buf = torch.full((rows + 2 * GUARD, B, width), NAN, dtype=torch.int16, device=device)
        self.view = self.buf[GUARD:GUARD + rows]

    def check(self):
        assert bool((self.buf[:GUARD] == NAN).all()) and bool((self.buf[GUARD + self.view.shape[0]:] == NAN).all()), "guard rows written"


def _words(rng, shape, device):
    """random 16-bit words without the guard pattern: (host int16, device int16)"""
    a = rng.integers(-32768, 32768, size=shape).astype(np.int16)
    a[a == NAN] = 1
    return a, torch.from_numpy(a).to(device)


def _length_cases(T, B, rng):
    cases = [None, np.zeros(B, np.int32), np.full(B, min(1, T), np.int32), np.full(B, T, np.int32),
             rng.integers(0, T + 1, size=B).astype(np.int32), np.full(B, T + 7, np.int32)]
    return cases


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [8, 24, 832])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_forward_and_backward_on_bits(device, k, R, B):
    from asr import _ops
    rng = np.random.default_rng(1000 * k + 10 * R + B)
    for T in sorted({1, k - 1, k, k + 1, 2 * k + 1, 65, 129}):
        G = (T + k - 1) // k
        x_host, x = _words(rng, (T, B, R), device)
        gy_host, gy = _words(rng, (G, B, k * R), device)
        for case, x_len in enumerate(_length_cases(T, B, rng)):
            dev_len = None if x_len is None else torch.from_numpy(x_len).to(device)
            want_y, want_len = ts.fwd(x_host, k, x_len)
            want_dx = ts.bwd(gy_host, k, T, x_len)
            got = []
            for run in range(2):                                             # the same bits on a second run
                y, dx = _Guarded(G, B, k * R, device), _Guarded(T, B, R, device)
                y_len = torch.full((B + 2,), 77, dtype=torch.int32, device=device)
                # through the C ABI, so that the guarded views are written in place; y_len NULL on every other case
                from asr import _lib
                lib, st = _lib.lib(), _lib.stream()
                ptr = (lambda t: None if t is None else t.data_ptr())
                rc = lib.asr_time_stack_fwd(st, ptr(x) if T else None, ptr(dev_len), ptr(y.view) if T else None,
                                            y_len[1:].data_ptr() if case % 2 == 0 else None, T, B, R, k)
                assert rc == 0
                if T:
                    rc = lib.asr_time_stack_bwd(st, gy.data_ptr(), ptr(dev_len), dx.view.data_ptr(), T, B, R, k)
                    assert rc == 0
                torch.cuda.synchronize()
                y.check()
                dx.check()
                assert y_len[0] == 77 and y_len[-1] == 77
                if case % 2 == 0:
                    assert np.array_equal(y_len[1:-1].cpu().numpy(), want_len), (T, case)
                else:
                    assert bool((y_len == 77).all())
                assert np.array_equal(y.view.cpu().numpy(), want_y), ("y", T, case)
                assert np.array_equal(dx.view.cpu().numpy(), want_dx), ("dx", T, case)       # (NaN-prefilled: every element written)
                got.append((y.view.clone(), dx.view.clone()))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
        if T in (k + 1, 129):                                                # the Python wrappers: same kernels, own allocations
            x_len = rng.integers(0, T + 1, size=B).astype(np.int32)
            xb = x.view(_ops.BF16)
            y, y_len = _ops.time_stack_fwd(xb, k, torch.from_numpy(x_len).to(device))
            dx = _ops.time_stack_bwd(gy.view(_ops.BF16), k, T, torch.from_numpy(x_len).to(device))
            want_y, want_len = ts.fwd(x_host, k, x_len)
            assert y.dtype == _ops.BF16 and np.array_equal(y.view(torch.int16).cpu().numpy(), want_y)
            assert np.array_equal(y_len.cpu().numpy(), want_len)
            assert np.array_equal(dx.view(torch.int16).cpu().numpy(), ts.bwd(gy_host, k, T, x_len))
            assert _ops.time_stack_fwd(xb, k, None, want_len=False)[1] is None


def test_zero_frames_write_only_the_lengths(device):
    from asr import _lib
    y_len = torch.full((4,), 77, dtype=torch.int32, device=device)
    x_len = torch.tensor([0, 5], dtype=torch.int32, device=device)
    assert _lib.lib().asr_time_stack_fwd(_lib.stream(), None, x_len.data_ptr(), None, y_len[1:].data_ptr(), 0, 2, 8, 3) == 0
    assert _lib.lib().asr_time_stack_bwd(_lib.stream(), None, x_len.data_ptr(), None, 0, 2, 8, 3) == 0
    torch.cuda.synchronize()
    assert y_len.tolist() == [77, 0, 0, 77]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [8, 24, 832])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_push_on_bits(device, k, R, B):
    from asr import _lib, _ops
    rng = np.random.default_rng(5000 + 1000 * k + 10 * R + B)
    lib = _lib.lib()
    state = _Guarded(k - 1, B, R, device)
    state.view.zero_()
    m = torch.full((B + 2,), 77, dtype=torch.int32, device=device)           # m[1:-1] is the kernel's, the ends are guards
    m[1:-1] = 0
    ref = ts.Stacker(k, B, R, dtype=np.int16)
    ptr = (lambda t: None if t is None or t.numel() == 0 else t.data_ptr())

    def push(chunk, n, flush):
        Tc = 0 if chunk is None else chunk.shape[0]
        G = (k - 1 + Tc + k - 1) // k
        y = _Guarded(G, B, k * R, device)
        emit = torch.full((B + 2,), 77, dtype=torch.int32, device=device)
        dn = None if n is None else torch.from_numpy(n).to(device)
        df = None if flush is None else torch.from_numpy(flush).to(device)
        rc = lib.asr_time_stack_push(_lib.stream(), ptr(state.view), m[1:].data_ptr(), ptr(chunk), ptr(dn), ptr(df), ptr(y.view),
                                     emit[1:].data_ptr(), Tc, B, R, k)
        assert rc == 0
        torch.cuda.synchronize()
        for g in (state, y):
            g.check()
        assert m[0] == 77 and m[-1] == 77 and emit[0] == 77 and emit[-1] == 77
        return y.view.cpu().numpy(), emit[1:-1].cpu().numpy()

    sizes = [s for s in (1, k - 1, k, k + 1, 64) if s >= 1]
    schedule = sizes + [int(rng.choice(sizes)) for _ in range(5)]
    for step, Tc in enumerate(schedule):
        chunk_host, chunk = _words(rng, (Tc, B, R), device)
        if step == 0:
            n = None                                                         # (NULL: all Tc rows of every slot)
        else:
            n = np.array([[0, Tc, rng.integers(0, Tc + 1), min(Tc, max(k - 2, 0)), 1][(b + step) % 5] for b in range(B)], dtype=np.int32)
        before = state.view.cpu().numpy().copy()
        m_before = m[1:-1].cpu().numpy().copy()
        y, emit = push(chunk, n, None)
        want_y, want_emit = ref.push(chunk_host, n)
        assert np.array_equal(y, want_y), "y, step %d" % step
        assert np.array_equal(emit, want_emit)
        assert np.array_equal(state.view.cpu().numpy(), ref.state), "state, step %d" % step
        assert np.array_equal(m[1:-1].cpu().numpy(), ref.m)
        if n is not None:
            for b in np.nonzero(n == 0)[0]:
                assert np.array_equal(state.view.cpu().numpy()[:, b], before[:, b]) and m[1 + b] == m_before[b], "an unfed slot changed"
        if step % 3 == 1:                                                    # one slot ends its utterance (m == 0 or m > 0), the others go on
            mask = np.zeros(B, dtype=np.int32)
            mask[step % B] = 1
            before = state.view.cpu().numpy().copy()
            y, emit = push(None, None, mask)
            want_y, want_emit = ref.push(None, None, mask)
            assert np.array_equal(y, want_y) and np.array_equal(emit, want_emit)
            assert np.array_equal(state.view.cpu().numpy(), ref.state) and np.array_equal(m[1:-1].cpu().numpy(), ref.m)
            for b in np.nonzero(mask == 0)[0]:
                assert np.array_equal(state.view.cpu().numpy()[:, b], before[:, b])
        if step % 3 == 2:                                                    # ... or is dropped
            mask = np.zeros(B, dtype=np.int32)
            mask[step % B] = 1
            if k > 1:
                _ops.time_stack_push_reset(state.view.view(_ops.BF16), m[1:-1], torch.from_numpy(mask).to(device))
            ref.reset(mask)
            torch.cuda.synchronize()
            state.check()
            assert np.array_equal(state.view.cpu().numpy(), ref.state) and np.array_equal(m[1:-1].cpu().numpy(), ref.m)
    y, emit = push(None, None, np.ones(B, dtype=np.int32))                   # everybody ends: both m == 0 and m > 0 occur over the cases
    want_y, want_emit = ref.push(None, None, np.ones(B, dtype=np.int32))
    assert np.array_equal(y, want_y) and np.array_equal(emit, want_emit) and not state.view.any() and not m[1:-1].any()
    chunk_host, chunk = _words(rng, (max(k - 1, 1), B, R), device)           # fill, then a reset without a mask
    push(chunk, None, None)
    ref.push(chunk_host, None)
    assert np.array_equal(m[1:-1].cpu().numpy(), ref.m)
    assert lib.asr_time_stack_push_reset(_lib.stream(), ptr(state.view), m[1:].data_ptr(), None, B, R, k) == 0
    torch.cuda.synchronize()
    state.check()
    assert not state.view.any() and m.tolist() == [77] + [0] * B + [77]


def test_push_through_the_wrapper(device):
    from asr import _ops
    rng = np.random.default_rng(9)
    k, B, R = 3, 2, 16
    state = torch.zeros((k - 1, B, R), dtype=_ops.BF16, device=device)
    m = torch.zeros((B,), dtype=torch.int32, device=device)
    ref = ts.Stacker(k, B, R)
    for Tc in (4, 1, 5):
        host, chunk = _words(rng, (Tc, B, R), device)
        y = torch.empty(((k - 1 + Tc + k - 1) // k, B, k * R), dtype=_ops.BF16, device=device)
        emit = _ops.time_stack_push(state, m, chunk.view(_ops.BF16), None, y, k)
        want_y, want_emit = ref.push(host)
        assert np.array_equal(y.view(torch.int16).cpu().numpy(), want_y) and np.array_equal(emit.cpu().numpy(), want_emit)
    y = torch.empty((1, B, k * R), dtype=_ops.BF16, device=device)
    emit = _ops.time_stack_push(state, m, None, None, y, k, flush=torch.ones((B,), dtype=torch.int32, device=device))
    assert emit.tolist() == [1, 1] and np.array_equal(y.view(torch.int16).cpu().numpy(), ref.push(None, None, np.ones(B))[0])


def test_refusals(device):
    from asr import _lib
    lib, st = _lib.lib(), _lib.stream()
    B = 2
    x = torch.ones((4, B, 24), dtype=torch.int16, device=device)
    y = torch.full((4, B, 24), 5, dtype=torch.int16, device=device)
    state = torch.full((8, B, 24), 6, dtype=torch.int16, device=device)
    m = torch.full((B,), 1, dtype=torch.int32, device=device)
    emit = torch.full((B,), 9, dtype=torch.int32, device=device)
    UNSUPPORTED, BAD_ARG = -3, -1
    p = (lambda t: t.data_ptr())
    # rows must be whole 16-byte lanes (R = 12: the 24 columns read as (2, B, 12) x 2), k within 1..ASR_TIME_STACK_MAX
    for R, k in ((12, 2), (8, 0), (8, 9), (12, 1)):
        assert lib.asr_time_stack_fwd(st, p(x), None, p(y), p(emit), 4, B, R, k) == UNSUPPORTED
        assert lib.asr_time_stack_bwd(st, p(x), None, p(y), 4, B, R, k) == UNSUPPORTED
        assert lib.asr_time_stack_push(st, p(state), p(m), p(x), None, None, p(y), p(emit), 2, B, R, k) == UNSUPPORTED
        assert lib.asr_time_stack_push_reset(st, p(state), p(m), None, B, R, k) == UNSUPPORTED
    # null pointers and counts
    assert lib.asr_time_stack_fwd(st, None, None, p(y), None, 4, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_fwd(st, p(x), None, None, None, 4, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_fwd(st, p(x), None, p(y), None, -1, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_fwd(st, p(x), None, p(y), None, 4, 0, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_bwd(st, None, None, p(y), 4, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_bwd(st, p(x), None, None, 4, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_push(st, None, p(m), p(x), None, None, p(y), p(emit), 2, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_push(st, p(state), None, p(x), None, None, p(y), p(emit), 2, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_push(st, p(state), p(m), None, None, None, p(y), p(emit), 2, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_push(st, p(state), p(m), p(x), None, None, None, p(emit), 2, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_push(st, p(state), p(m), p(x), None, None, p(y), None, 2, B, 8, 2) == BAD_ARG
    assert lib.asr_time_stack_push_reset(st, None, p(m), None, B, 8, 2) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((y == 5).all()) and bool((state == 6).all()) and bool((m == 1).all()) and bool((emit == 9).all()), "a refused call wrote"
