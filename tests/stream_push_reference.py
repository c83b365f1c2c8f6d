"""numpy restatement of the carry kernels (include/asr_hip.h: asr_stream_push / asr_stream_push_reset): a per-slot delay line of
K rows of R features.  ``Line`` holds ``state`` (K, B, R) and ``m`` (B); ``push`` returns what the kernel writes."""
import numpy as np

CONTEXT, LOOKAHEAD = 0, 1


class Line:
    def __init__(self, K, B, R, mode, dtype=np.float32):
        self.K, self.B, self.R, self.mode = K, B, R, mode
        self.state = np.zeros((K, B, R), dtype=dtype)
        self.m = np.full((B,), K if mode == CONTEXT else 0, dtype=np.int32)

    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.state[:, b] = 0
                self.m[b] = self.K if self.mode == CONTEXT else 0

    def push(self, chunk, n=None, flush=None):
        """chunk (Tc, B, R) or None (Tc = 0), n (B) or None (all Tc), flush (B) or None (lookahead mode: end of utterance)
        -> (window (K + Tc, B, R), wlen (B), emit (B)); updates state and m"""
        K, B, R = self.K, self.B, self.R
        Tc = 0 if chunk is None else chunk.shape[0]
        window = np.zeros((K + Tc, B, R), dtype=self.state.dtype)
        wlen, emit = np.zeros((B,), dtype=np.int32), np.zeros((B,), dtype=np.int32)
        for b in range(B):
            mb = int(self.m[b])
            nb = 0 if flush is not None else (Tc if n is None else int(n[b]))
            window[:mb, b] = self.state[:mb, b]
            if nb:
                window[mb:mb + nb, b] = chunk[:nb, b]
            wlen[b] = mb + nb
            if self.mode == CONTEXT:
                emit[b] = nb
            elif flush is not None:
                emit[b] = mb if flush[b] else 0
            else:
                emit[b] = max(0, mb + nb - K)
            if flush is not None:
                if flush[b]:
                    self.state[:, b] = 0
                    self.m[b] = 0
            elif nb > 0:
                keep = min(K, mb + nb)
                new = window[mb + nb - keep:mb + nb, b].copy()
                self.state[:, b] = 0
                self.state[:keep, b] = new
                self.m[b] = keep
        return window, wlen, emit
