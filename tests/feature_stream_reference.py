"""Float64 restatement of the streaming log-mel front end (include/asr_hip.h: asr_fbank_stream_*; asr.fft.FeatureStream), one slot.

What is carried: the pending pre-emphasised samples (always fewer than L), the last raw sample, the last <= 4 log-mel rows and two
counters.  The transform of a frame is the oracle's own (oracle.fft: window, powspec, compute_logmel); what is restated here is only
the bookkeeping -- which samples make which frame, which frames a chunk completes, which feature frames it may emit."""
import numpy as np

from oracle import fft as o


def chunk_frames(n_samples, frame_step):
    """Tc of a chunk of n samples: 1 + (n - 1) // S, 0 for an empty chunk"""
    return 1 + (n_samples - 1) // frame_step if n_samples > 0 else 0


class Stream(object):
    def __init__(self, L, S, nfft, fbank, winfunc=np.hanning, coeff=0.97):
        self.L, self.S, self.nfft, self.fbank, self.window, self.coeff = L, S, nfft, fbank, winfunc(L), coeff
        self.nfilt = fbank.shape[0]
        self.reset()

    def reset(self):
        self.pend = np.zeros(0)                     # pre-emphasised samples of the frames not yet complete
        self.last = None                            # last raw sample
        self.rows = np.zeros((0, self.nfilt))       # the last min(4, c) log-mel rows
        self.c = 0                                  # log-mel frames so far
        self.emitted = 0                            # feature frames so far
        self.ended = False                          # flushed and not fed since: `emitted` is the finished utterance's count

    def _logmel(self, w, k):
        """the first k frames of the window w, the last one zero padded where w ends early"""
        if k == 0:
            return np.zeros((0, self.nfilt))
        frames = np.zeros((k, self.L))
        for f in range(k):
            seg = w[f * self.S:f * self.S + self.L]
            frames[f, :len(seg)] = seg
        return o.compute_logmel(o.powspec(frames * self.window[None, :], self.nfft), self.fbank)

    def _emit(self, new):
        """feature frames max(0, c - 2) .. max(0, c' - 2) - 1 from [carried rows | new rows] -> (count, 3, nfilt)"""
        win = np.concatenate([self.rows, new])
        base = self.c - len(self.rows)              # absolute frame of win[0]
        c2 = self.c + len(new)
        e0, e1 = max(0, self.c - 2), max(0, c2 - 2)

        def at(q):
            return win[max(q, 0) - base]

        def dl(q):
            return (at(max(q, 0) + 1) - at(max(q, 0) - 1)) * 0.5

        out = np.zeros((e1 - e0, 3, self.nfilt))
        for t in range(e0, e1):
            out[t - e0] = at(t), dl(t), (dl(t + 1) - dl(t - 1)) * 0.5
        self.rows, self.c = win[-4:], c2
        self.emitted += e1 - e0
        return out

    def advance(self, x):
        x = np.asarray(x, dtype=np.float64)
        if len(x) == 0:
            return np.zeros((0, 3, self.nfilt))     # an untouched slot
        if self.ended:
            self.emitted, self.ended = 0, False
        prev = np.concatenate([[0.0 if self.last is None else self.last], x[:-1]])
        y = x - self.coeff * prev
        if self.last is None:
            y[0] = x[0]
        self.last = x[-1]
        w = np.concatenate([self.pend, y])
        k = 0 if len(w) < self.L else 1 + (len(w) - self.L) // self.S
        new = self._logmel(w, k)
        self.pend = w[k * self.S:]
        before = self.c
        out = self._emit(new)
        assert len(self.pend) < self.L
        assert len(out) == max(0, self.c - 2) - max(0, before - 2) and len(out) <= chunk_frames(len(x), self.S)
        return out

    def flush(self):
        m = len(self.pend)
        k = 1 if (self.c == 0 or m > self.L - self.S) else 0
        out = self._emit(self._logmel(self.pend, k))
        total = self.emitted
        self.reset()
        self.emitted, self.ended = total, True      # (stands until the slot is fed again)
        return out


def oneshot(signal, L, S, nfft, fbank, winfunc=np.hanning):
    """oracle.fft on the whole signal -> (T, 3, nfilt), T = max(F - 2, 0)"""
    signal = np.asarray(signal, dtype=np.float64)
    pre = o.preemphasis(signal) if len(signal) else signal
    lm = o.compute_logmel(o.powspec(o.framesig(pre, L, S, winfunc), nfft), fbank)
    return np.stack([np.asarray(f) for f in o.compute_deltas(lm)], axis=1)
