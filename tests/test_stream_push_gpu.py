"""The carry kernels (csrc/stream.hip) bit for bit against their numpy restatement (tests/stream_push_reference.py, whose
semantics tests/test_stream_push_cpu.py checks): both modes, every slot on its own cut schedule, single-slot restarts and
flushes between the chunks, guard rows around every buffer."""
import numpy as np
import pytest
import torch

import stream_push_reference as sp

pytestmark = pytest.mark.gpu

B, MAX_CHUNK = 5, 24
GUARD = 3           # rows (of B * R features) of sentinel in front of and behind every buffer


class _Guarded:
    """(rows, B, R) 16-bit tensor inside a buffer with GUARD sentinel rows on both sides"""

    def __init__(self, rows, R, dtype, device, fill=0.0):
        self.buf = torch.full((rows + 2 * GUARD, B, R), 3.0, dtype=dtype, device=device)
        self.view = self.buf[GUARD:GUARD + rows]
        self.view.fill_(fill)

    def check(self):
        assert bool((self.buf[:GUARD] == 3.0).all()) and bool((self.buf[GUARD + self.view.shape[0]:] == 3.0).all()), "guard rows written"


def _bits(t):
    return t.view(torch.int16).cpu().numpy()


@pytest.mark.parametrize("R", [8, 120, 2432])
@pytest.mark.parametrize("K", [1, 4, 20])
@pytest.mark.parametrize("mode", [sp.CONTEXT, sp.LOOKAHEAD])
def test_push_against_the_restatement(device, mode, K, R):
    from asr import _ops
    rng = np.random.default_rng(1000 * mode + 10 * K + R)
    dt = _ops.BF16
    state = _Guarded(K, R, dt, device)
    m = torch.full((B + 2,), 77, dtype=torch.int32, device=device)            # m[1:-1] is the kernel's, the ends are guards
    m[1:-1] = 0
    line = sp.Line(K, B, R, mode, dtype=np.int16)
    # chunk sizes: 1, K - 1, K, K + 1, max_chunk -- and per slot its own share of each chunk (0, all, or anything between)
    sizes = [s for s in (1, K - 1, K, K + 1, MAX_CHUNK) if 1 <= s <= MAX_CHUNK]
    schedule = sizes + [int(rng.choice(sizes)) for _ in range(7)]
    for step, Tc in enumerate(schedule):
        chunk = torch.from_numpy(rng.standard_normal((Tc, B, R)).astype(np.float32)).to(device, dt)
        if step == 0:
            n = None                                                         # (NULL: all Tc rows of every slot)
        else:
            n = np.array([[0, Tc, rng.integers(0, Tc + 1), min(Tc, max(K - 1, 0)), rng.integers(0, Tc + 1)][(b + step) % 5]
                          for b in range(B)], dtype=np.int32)
        window = _Guarded(K + Tc, R, dt, device, fill=5.0)
        before = _bits(state.view).copy()
        wlen, emit = _ops.stream_push(state.view, m[1:-1] if mode == sp.LOOKAHEAD else None, chunk,
                                      None if n is None else torch.from_numpy(n).to(device), window.view, mode)
        want_window, want_wlen, want_emit = line.push(_bits(chunk), n)
        torch.cuda.synchronize()
        for g in (state, window):
            g.check()
        assert m[0] == 77 and m[-1] == 77
        assert np.array_equal(_bits(window.view), want_window), "window, step %d" % step
        assert np.array_equal(wlen.cpu().numpy(), want_wlen) and np.array_equal(emit.cpu().numpy(), want_emit)
        assert np.array_equal(_bits(state.view), line.state), "state, step %d" % step
        if mode == sp.LOOKAHEAD:
            assert np.array_equal(m[1:-1].cpu().numpy(), line.m)
        if n is not None:
            for b in np.nonzero(n == 0)[0]:
                assert np.array_equal(_bits(state.view)[:, b], before[:, b]), "an unfed slot's state changed"
        if step % 3 == 2:                                                    # one slot starts over, the others go on
            mask = np.zeros(B, dtype=np.int32)
            mask[step % B] = 1
            if mode == sp.LOOKAHEAD and step % 2 == 0:                       # ... at its utterance's end: the pending rows come out
                window = _Guarded(K, R, dt, device, fill=5.0)
                wlen, emit = _ops.stream_push(state.view, m[1:-1], None, None, window.view, mode, flush=torch.from_numpy(mask).to(device))
                want_window, want_wlen, want_emit = line.push(None, None, mask)
                torch.cuda.synchronize()
                window.check()
                assert np.array_equal(_bits(window.view), want_window)
                assert np.array_equal(wlen.cpu().numpy(), want_wlen) and np.array_equal(emit.cpu().numpy(), want_emit)
            else:
                _ops.stream_push_reset(state.view, m[1:-1] if mode == sp.LOOKAHEAD else None, torch.from_numpy(mask).to(device))
                line.reset(mask)
            torch.cuda.synchronize()
            state.check()
            assert np.array_equal(_bits(state.view), line.state)
            if mode == sp.LOOKAHEAD:
                assert np.array_equal(m[1:-1].cpu().numpy(), line.m) and m[0] == 77 and m[-1] == 77
    _ops.stream_push_reset(state.view, m[1:-1] if mode == sp.LOOKAHEAD else None, None)
    torch.cuda.synchronize()
    state.check()
    assert not _bits(state.view).any() and (mode == sp.CONTEXT or not m[1:-1].any())


def test_refusals(device):
    from asr import _lib, _ops
    state = torch.zeros((2, B, 12), dtype=_ops.BF16, device=device)
    window = torch.full((5, B, 12), 5.0, dtype=_ops.BF16, device=device)
    chunk = torch.ones((3, B, 12), dtype=_ops.BF16, device=device)
    with pytest.raises(_lib.AsrHipError):                                    # rows must be whole 16-byte lanes
        _ops.stream_push(state, None, chunk, None, window, sp.CONTEXT)
    torch.cuda.synchronize()
    assert bool((window == 5.0).all()) and not bool(state.any())
    state = torch.zeros((2, B, 16), dtype=_ops.BF16, device=device)
    with pytest.raises(_lib.AsrHipError):                                    # the lookahead mode needs its counts
        _ops.stream_push(state, None, torch.ones((3, B, 16), dtype=_ops.BF16, device=device), None,
                         torch.zeros((5, B, 16), dtype=_ops.BF16, device=device), sp.LOOKAHEAD)
