"""NumPy restatement of csrc/time_stack.hip (include/asr_hip.h, "time reduction by frame stacking"): forward, backward and the
streaming push, on arrays of any dtype (the GPU tests run it on the raw 16-bit words).  tests/test_time_stack_cpu.py checks it
against a plain triple loop, the adjoint identity and the stream = one-shot property; the GPU tests check the kernels against it."""
import numpy as np


def clamp_len(x_len, T, B):
    if x_len is None:
        return np.full((B,), T, dtype=np.int64)
    return np.clip(np.asarray(x_len, dtype=np.int64), 0, T)


def fwd(x, k, x_len=None):
    """x (T, B, R) -> (y (ceil(T / k), B, k * R), y_len (B) int32)"""
    T, B, R = x.shape
    G = -(-T // k)
    length = clamp_len(x_len, T, B)
    padded = np.zeros((G * k, B, R), dtype=x.dtype)
    padded[:T] = x
    padded[np.arange(G * k)[:, None] >= length[None, :]] = 0
    y = padded.reshape(G, k, B, R).transpose(0, 2, 1, 3).reshape(G, B, k * R)
    return np.ascontiguousarray(y), (-(-length // k)).astype(np.int32)


def bwd(gy, k, T, x_len=None):
    """gy (ceil(T / k), B, k * R) -> dx (T, B, R), zero at and beyond x_len[b]"""
    G, B, KR = gy.shape
    R = KR // k
    assert G == -(-T // k) and R * k == KR
    dx = gy.reshape(G, B, k, R).transpose(0, 2, 1, 3).reshape(G * k, B, R)[:T].copy()
    dx[np.arange(T)[:, None] >= clamp_len(x_len, T, B)[None, :]] = 0
    return dx


class Stacker:
    """asr_time_stack_push on the host: state (k - 1, B, R), m (B)"""

    def __init__(self, k, B, R, dtype=np.int16):
        self.k, self.B, self.R = k, B, R
        self.state = np.zeros((k - 1, B, R), dtype=dtype)
        self.m = np.zeros((B,), dtype=np.int32)

    def push(self, chunk, n=None, flush=None):
        """-> (y (ceil((k - 1 + Tc) / k), B, k * R): the forward of [pending | new] per slot, the trailing partial group
        zero-completed; emit (B) int32)"""
        k, B, R = self.k, self.B, self.R
        Tc = 0 if chunk is None else chunk.shape[0]
        rows = k - 1 + Tc
        seq = np.zeros((rows, B, R), dtype=self.state.dtype)
        total = np.zeros((B,), dtype=np.int64)
        emit = np.zeros((B,), dtype=np.int32)
        for b in range(B):
            mb = int(self.m[b])
            if flush is not None:
                if flush[b]:
                    seq[:mb, b] = self.state[:mb, b]
                    total[b] = mb
                    emit[b] = 1 if mb > 0 else 0
                    self.state[:, b] = 0
                    self.m[b] = 0
                continue
            nb = Tc if n is None else int(min(max(n[b], 0), Tc))
            seq[:mb, b] = self.state[:mb, b]
            seq[mb:mb + nb, b] = chunk[:nb, b]
            total[b] = mb + nb
            emit[b] = (mb + nb) // k
            if nb > 0:
                rest = (mb + nb) % k
                self.state[:, b] = 0
                self.state[:rest, b] = seq[mb + nb - rest:mb + nb, b]
                self.m[b] = rest
        y, _ = fwd(seq, k, total) if rows > 0 else (np.zeros((0, B, k * R), dtype=self.state.dtype), None)
        return y, emit

    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.state[:, b] = 0
                self.m[b] = 0
