"""The window kernels of the latency-controlled BiGRU (csrc/lc_window.hip) bit for bit against their NumPy restatement
(tests/lc_bigru_reference.py, whose semantics tests/test_lc_bigru_cpu.py checks): gather, scatter and the streaming push, in both
builds of the library (bfloat16 and IEEE half: the scatter's rounding is the only thing that differs), in buffers with NaN guard
rows in front and behind, compared on the raw 16-bit words.  The copies run on random words; the scatter's sums on finite values."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lc_bigru_reference as lc

pytestmark = pytest.mark.gpu

GUARD = 2           # rows (of B * width 16-bit words) of NaN in front of and behind every buffer
NAN = 0x7FC1        # as int16: a NaN in bfloat16 (exponent 0xFF) and in IEEE half (exponent 0x1F) alike
CASES = [(1, 0), (4, 0), (8, 4), (5, 7), (3, 11), (64, 0)]
WINDOW, BLOCK = 0, 1
BAD_ARG = -1

_LIBS = {}


def _library(fmt):
    """the build of the library with activation format `fmt`: the process's own, or its twin loaded beside it"""
    if not _LIBS:
        from asr import _lib
        own = "f16" if _lib.act_dtype() == torch.float16 else "bf16"
        _LIBS[own] = _lib.lib()
        other = ctypes.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libasr_hip.so" if own == "f16" else "libasr_hip_f16.so"))
        for name in ("asr_lc_gather", "asr_lc_scatter", "asr_lc_push", "asr_act_dtype"):
            getattr(other, name).restype, getattr(other, name).argtypes = _lib.SIGNATURES[name]
        assert bool(other.asr_act_dtype()) == (own == "bf16")
        _LIBS["bf16" if own == "f16" else "f16"] = other
    return _LIBS[fmt]


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


def _values(rng, shape, device, fmt):
    """finite values of the format as words"""
    a = lc.encode(rng.normal(size=shape).astype(np.float32) * 3.0, fmt)
    return a, torch.from_numpy(a).to(device)


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _dev(a, device):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.int32)).to(device)


def _sizes(Nc, Nr):
    return sorted({T for T in (1, Nc - 1, Nc, Nc + 1, Nc + Nr, 2 * Nc + Nr + 1) if T >= 1})


def _length_cases(T, B, rng):
    return [None, np.zeros(B, np.int32), np.full(B, 1, np.int32), np.full(B, T, np.int32),
            rng.integers(0, T + 1, size=B).astype(np.int32), np.full(B, T + 7, np.int32)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [8, 40, 520])
@pytest.mark.parametrize("Nc,Nr", CASES)
def test_gather_and_scatter_on_bits(device, Nc, Nr, R, B):
    from asr import _lib
    rng = np.random.default_rng(10000 * Nc + 100 * Nr + 10 * R + B)
    st = _lib.stream()
    for fmt in ("bf16", "f16"):
        lib = _library(fmt)
        for T in _sizes(Nc, Nr):
            W, C = lc.window_shape(T, B, Nc, Nr)
            x_host, x = _words(rng, (T, B, R), device)
            yw_host, yw = _values(rng, (W, C * B, R), device, fmt)
            add_host, add = _values(rng, (T, B, R), device, fmt)
            for case, x_len in enumerate(_length_cases(T, B, rng)):
                n_wins = [None, rng.integers(0, C + 2, size=B).astype(np.int32)]
                for mode in (WINDOW, BLOCK):
                    for n_win in n_wins:
                        d_len, d_win = _dev(x_len, device), _dev(n_win, device)
                        xw = _Guarded(W, C * B, R, device)
                        w_len = torch.full((C * B + 2,), 77, dtype=torch.int32, device=device)
                        want_len = (case + mode) % 2 == 0                        # w_len NULL on every other call
                        rc = lib.asr_lc_gather(st, _ptr(x), _ptr(d_len), _ptr(d_win), _ptr(xw.view),
                                               w_len[1:].data_ptr() if want_len else None, T, B, R, Nc, Nr, mode)
                        assert rc == 0
                        want_xw, want_w = lc.gather(x_host, Nc, Nr, mode == BLOCK, x_len, n_win)
                        torch.cuda.synchronize()
                        xw.check()
                        assert np.array_equal(xw.view.cpu().numpy(), want_xw), ("gather", fmt, T, case, mode, n_win)
                        assert w_len[0] == 77 and w_len[-1] == 77
                        assert np.array_equal(w_len[1:-1].cpu().numpy(), want_w) if want_len else bool((w_len == 77).all())
                        for addend in (None, add):
                            got = []
                            for run in range(2):                                 # the same bits on a second run
                                y = _Guarded(T, B, R, device)
                                rc = lib.asr_lc_scatter(st, _ptr(yw), _ptr(addend), _ptr(d_len), _ptr(d_win), _ptr(y.view), T, B, R, Nc, Nr, mode)
                                assert rc == 0
                                torch.cuda.synchronize()
                                y.check()
                                got.append(y.view.clone())
                            want_y = lc.scatter(yw_host, T, B, Nc, Nr, mode == WINDOW, None if addend is None else add_host, x_len, n_win, fmt)
                            assert np.array_equal(got[0].cpu().numpy(), want_y), ("scatter", fmt, T, case, mode, n_win, addend is not None)
                            assert torch.equal(got[0], got[1])


def test_a_single_term_is_a_copy(device):
    """the forward pass's scatter without an addend moves every finite word unchanged, and gather then scatter is the identity
    below the lengths"""
    from asr import _ops
    rng = np.random.default_rng(4)
    T, B, R, Nc, Nr = 37, 3, 40, 5, 7
    fmt = "f16" if _ops.BF16 == torch.float16 else "bf16"
    host, x = _values(rng, (T, B, R), device, fmt)
    x_len = torch.tensor([37, 0, 20], dtype=torch.int32, device=device)
    xw, w_len = _ops.lc_gather(x.view(_ops.BF16), Nc, Nr, _ops.LC_WINDOW, x_len)
    assert xw.dtype == _ops.BF16 and tuple(xw.shape) == (12, 8 * B, R) and w_len.dtype == torch.int32
    assert np.array_equal(w_len.cpu().numpy(), lc.gather(host, Nc, Nr, False, x_len.cpu().numpy())[1])
    y = _ops.lc_scatter(xw, T, B, Nc, Nr, _ops.LC_BLOCK, None, x_len)
    want = host.copy()
    want[0:, 1] = 0
    want[20:, 2] = 0
    assert np.array_equal(y.view(torch.int16).cpu().numpy(), want)
    with pytest.raises(ValueError):
        _ops.lc_scatter(xw[:5].contiguous(), T, B, Nc, Nr, _ops.LC_BLOCK)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [8, 40, 520])
@pytest.mark.parametrize("Nc,Nr", CASES)
def test_push_on_bits(device, Nc, Nr, R, B):
    from asr import _lib, _ops
    rng = np.random.default_rng(7000 + 10000 * Nc + 100 * Nr + 10 * R + B)
    K = Nc + Nr - 1
    for fmt in ("bf16", "f16"):
        lib = _library(fmt)
        state = _Guarded(K, B, R, device)
        state.view.zero_()
        m = torch.full((B + 2,), 77, dtype=torch.int32, device=device)       # m[1:-1] is the kernel's, the ends are guards
        m[1:-1] = 0
        ref = lc.Carry(Nc, Nr, B, R, dtype=np.int16)

        def push(chunk, n, flush):
            Tc = 0 if chunk is None else chunk.shape[0]
            window = _Guarded(K + Tc, B, R, device)
            counts = torch.full((3, B + 2), 77, dtype=torch.int32, device=device)
            d_n, d_flush = _dev(n, device), _dev(flush, device)
            rc = lib.asr_lc_push(_lib.stream(), _ptr(state.view), m[1:].data_ptr(), _ptr(chunk), _ptr(d_n), _ptr(d_flush),
                                 _ptr(window.view), counts[0, 1:].data_ptr(), counts[1, 1:].data_ptr(), counts[2, 1:].data_ptr(),
                                 Tc, B, R, Nc, Nr)
            assert rc == 0
            torch.cuda.synchronize()
            state.check()
            window.check()
            assert m[0] == 77 and m[-1] == 77 and bool((counts[:, 0] == 77).all()) and bool((counts[:, -1] == 77).all())
            return (window.view.cpu().numpy(),) + tuple(counts[i, 1:-1].cpu().numpy() for i in range(3))

        def same(got, want, what):
            for g, w, name in zip(got, want, ("window", "a", "w", "emit")):
                assert np.array_equal(g, w), (name, what)
            assert np.array_equal(state.view.cpu().numpy(), ref.state) and np.array_equal(m[1:-1].cpu().numpy(), ref.m), ("state", what)

        sizes = sorted({s for s in (1, Nr - 1, Nr, Nc, Nc + Nr, 2 * Nc + Nr + 1) if s >= 1})
        schedule = sizes + [int(rng.choice(sizes)) for _ in range(4)]
        for step, Tc in enumerate(schedule):
            chunk_host, chunk = _words(rng, (Tc, B, R), device)
            if step == 0:
                n = None                                                         # (NULL: all Tc rows of every slot)
            else:
                n = np.array([[0, Tc, rng.integers(0, Tc + 1), 1, Tc + 3][(b + step) % 5] for b in range(B)], dtype=np.int32)
            flush = None
            if step % 4 == 3:                                                    # one slot ends with this chunk, fed or not
                flush = np.zeros(B, dtype=np.int32)
                flush[step % B] = 1
            before, m_before = state.view.cpu().numpy().copy(), m[1:-1].cpu().numpy().copy()
            same(push(chunk, n, flush), ref.push(chunk_host, n, flush), (fmt, step))
            for b in range(B):
                if n is not None and n[b] == 0 and not (flush is not None and flush[b]):
                    assert np.array_equal(state.view.cpu().numpy()[:, b], before[:, b]) and m[1 + b] == m_before[b], "an unfed slot changed"
            if step % 4 == 1:                                                    # a slot ends between two chunks: nothing is fed
                mask = np.zeros(B, dtype=np.int32)
                mask[step % B] = 1
                before = state.view.cpu().numpy().copy()
                same(push(None, None, mask), ref.push(None, None, mask), (fmt, step, "flush"))
                for b in np.nonzero(mask == 0)[0]:
                    assert np.array_equal(state.view.cpu().numpy()[:, b], before[:, b])
            if step % 4 == 2:                                                    # ... or is dropped
                mask = np.zeros(B, dtype=np.int32)
                mask[step % B] = 1
                _ops.stream_push_reset(state.view.view(_ops.BF16), m[1:-1], torch.from_numpy(mask).to(device))
                ref.reset(mask)
                torch.cuda.synchronize()
                state.check()
                assert np.array_equal(state.view.cpu().numpy(), ref.state) and np.array_equal(m[1:-1].cpu().numpy(), ref.m)
        got = push(None, None, np.ones(B, dtype=np.int32))                       # everybody ends
        same(got, ref.push(None, None, np.ones(B, dtype=np.int32)), (fmt, "end"))
        assert not state.view.any() and not m[1:-1].any()


def test_push_through_the_wrapper(device):
    from asr import _ops
    rng = np.random.default_rng(9)
    Nc, Nr, B, R = 4, 3, 2, 16
    state = torch.zeros((Nc + Nr - 1, B, R), dtype=_ops.BF16, device=device)
    m = torch.zeros((B,), dtype=torch.int32, device=device)
    ref = lc.Carry(Nc, Nr, B, R)
    for Tc in (5, 1, 9):
        host, chunk = _words(rng, (Tc, B, R), device)
        window = torch.empty((Nc + Nr - 1 + Tc, B, R), dtype=_ops.BF16, device=device)
        got = _ops.lc_push(state, m, chunk.view(_ops.BF16), None, window, Nc, Nr)
        want = ref.push(host)
        assert np.array_equal(window.view(torch.int16).cpu().numpy(), want[0])
        for g, w in zip(got, want[1:]):
            assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
    window = torch.empty((Nc + Nr - 1, B, R), dtype=_ops.BF16, device=device)
    a, w, emit = _ops.lc_push(state, m, None, None, window, Nc, Nr, flush=torch.ones((B,), dtype=torch.int32, device=device))
    want = ref.push(None, None, np.ones(B))
    assert a.tolist() == want[1].tolist() and w.tolist() == want[2].tolist() and emit.tolist() == a.tolist() and not m.any()


def test_guards(device):
    """every refusal of the header: ASR_ERR_BAD_ARG and nothing written"""
    from asr import _lib
    st = _lib.stream()
    B, T, R = 2, 12, 8
    x = torch.ones((T, B, 24), dtype=torch.int16, device=device)
    out = torch.full((64, B, 24), 5, dtype=torch.int16, device=device)
    state = torch.full((16, B, 24), 6, dtype=torch.int16, device=device)
    ints = torch.full((4, 64), 9, dtype=torch.int32, device=device)
    p = (lambda t: t.data_ptr())
    for fmt in ("bf16", "f16"):
        lib = _library(fmt)

        def gather(x_=p(x), xw=p(out), T_=T, B_=B, R_=R, Nc=4, Nr=2, mode=WINDOW):
            return lib.asr_lc_gather(st, x_, None, None, xw, p(ints[0]), T_, B_, R_, Nc, Nr, mode)

        def scatter(yw=p(x), y=p(out), T_=T, B_=B, R_=R, Nc=4, Nr=2, mode=BLOCK):
            return lib.asr_lc_scatter(st, yw, None, None, None, y, T_, B_, R_, Nc, Nr, mode)

        def push(state_=p(state), m=p(ints[0]), chunk=p(x), window=p(out), a=p(ints[1]), w=p(ints[2]), emit=p(ints[3]), Tc=2, B_=B, R_=R,
                 Nc=4, Nr=2):
            return lib.asr_lc_push(st, state_, m, chunk, None, None, window, a, w, emit, Tc, B_, R_, Nc, Nr)

        assert gather() == 0 and scatter() == 0 and push() == 0                  # (the calls are good ones before they are spoilt)
        torch.cuda.synchronize()
        out.fill_(5)
        state.fill_(6)
        ints.fill_(9)
        for call in (gather, scatter, push):
            for bad in (dict(Nc=0), dict(Nc=-3), dict(Nr=-1), dict(R_=12), dict(R_=4), dict(R_=0), dict(B_=0)):
                assert call(**bad) == BAD_ARG, (call.__name__, bad)
        for call in (gather, scatter):
            assert call(T_=-1) == BAD_ARG and call(mode=2) == BAD_ARG and call(mode=-1) == BAD_ARG
            assert call(T_=(1 << 30) + 1, Nc=1 << 20) == BAD_ARG                                        # T beyond the index arithmetic
            assert call(T_=1 << 30, Nc=1 << 30, Nr=0) == BAD_ARG                                        # a window above ASR_LC_MAX_WINDOW
            assert call(T_=8192, Nc=4097, Nr=0) == BAD_ARG and call(T_=8192, Nc=4000, Nr=97) == BAD_ARG
            assert call(T_=1 << 30, Nc=1, Nr=0, B_=2) == BAD_ARG                                        # C * B windows past 31 bits
            assert call(T_=1 << 28, Nc=2048, Nr=2048, B_=64, R_=1024) == BAD_ARG                        # lanes of the window batch past 31 bits
            assert call(T_=1 << 26, Nc=4096, Nr=0, B_=1, R_=512) == BAD_ARG                             # lanes of (T, B, R) past 31 bits
            assert call(T_=0) == 0                                                                      # nothing to do is no error
        assert gather(x_=None) == BAD_ARG and gather(xw=None) == BAD_ARG
        assert scatter(yw=None) == BAD_ARG and scatter(y=None) == BAD_ARG
        assert push(Tc=-1) == BAD_ARG and push(Nc=4000, Nr=97) == BAD_ARG and push(Nc=1 << 30, Nr=1 << 30) == BAD_ARG
        assert push(Tc=1 << 24, R_=1024, B_=64) == BAD_ARG                                              # lanes of the window past 31 bits
        for missing in ("state_", "m", "chunk", "window", "a", "w", "emit"):
            assert push(**{missing: None}) == BAD_ARG, missing
        assert push(state_=None, m=None, Nc=1, Nr=0, Tc=1) == 0                                         # K = 0: no state to carry
        assert push(state_=None, m=None, chunk=None, window=None, Nc=1, Nr=0, Tc=0) == 0                # ... and no rows: only the counts
        torch.cuda.synchronize()
        assert ints[1:, :B].tolist() == [[0] * B] * 3
        ints.fill_(9)
        out.fill_(5)
    torch.cuda.synchronize()
    assert bool((out == 5).all()) and bool((state == 6).all()) and bool((ints == 9).all()), "a refused call wrote"
