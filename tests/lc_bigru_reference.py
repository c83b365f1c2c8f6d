"""Restatement of the latency-controlled bidirectional GRU (include/asr_hip.h, "latency-controlled bidirectional GRU") from its
definition: the layer in torch CPU operators (float64 or float32, so autograd gives its gradients), NumPy restatements of the window
kernels of csrc/lc_window.hip (gather, scatter with float32 sums in the fixed order and one rounding, the streaming push), the
chunked layer built from them, and a DS2Oracle whose recurrent layers are the restated one.  tests/test_lc_bigru_cpu.py checks all
of it against a per-frame brute force, the adjoint identities and the stream = one-shot property; the GPU tests check the kernels,
the layer and the stream against it.

`variant` of the layer is None or one of the ways to get it wrong (MUTANTS): the tests measure how far each is from the right one.
"""
import numpy as np
import torch

MUTANTS = ("no_right_context", "shifted", "carried_state", "right_context_gradient")


# ------------------------------------------------------------------------------------------------------------ the layer
def cell(x_t, h, w_ih, w_hh, b_ih, b_hh):
    """one GRU step, cuDNN's / torch.nn.GRU's gate convention (asr/nn/gru.py): rows are (r, z, n)"""
    H = h.shape[-1]
    gi = x_t @ w_ih.T + b_ih
    gh = h @ w_hh.T + b_hh
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + z * h


def lengths(x_len, T, B):
    if x_len is None:
        return [T] * B
    return [int(min(max(int(v), 0), T)) for v in x_len]


def layer(x, w_ih, w_hh, b_ih, b_hh, Nc, Nr, x_len=None, variant=None):
    """x (T, B, I), parameters stacked over the two directions -> y (T, B, H), straight from the definition: a loop over the slots,
    the forward direction over the utterance, the reverse direction block by block from a zero state at the end of the block's
    right context, outputs kept for the block's own frames, the two summed, zero at and beyond the length."""
    T, B, _ = x.shape
    H = w_hh.shape[2]
    p0, p1 = [w[0] for w in (w_ih, w_hh, b_ih, b_hh)], [w[1] for w in (w_ih, w_hh, b_ih, b_hh)]
    zero = torch.zeros(H, dtype=x.dtype)
    cols = []
    for b, n in enumerate(lengths(x_len, T, B)):
        fwd, h = [], zero
        for t in range(n):
            h = cell(x[t, b], h, *p0)
            fwd.append(h)
        rev, extra = [None] * n, [zero] * n
        starts = [c * Nc for c in range(-(-n // Nc))]
        ends = starts[1:] + [n]
        carried = zero
        for c in reversed(range(len(starts))):
            e = min(ends[c] + (0 if variant == "no_right_context" else Nr), n)
            h = carried if variant == "carried_state" else zero
            for t in range(e - 1, starts[c] - 1, -1):
                # "shifted": the window's rows are taken one frame late (the utterance's last frame twice)
                h = cell(x[min(t + 1, n - 1) if variant == "shifted" else t, b], h, *p1)
                if t < ends[c]:
                    rev[t] = h
                elif variant == "right_context_gradient":
                    extra[t] = extra[t] + (h - h.detach())      # the same value, but the cropped outputs receive gradient
            carried = h
        rows = [fwd[t] + rev[t] + extra[t] for t in range(n)] + [zero] * (T - n)
        cols.append(torch.stack(rows) if rows else torch.zeros(0, H, dtype=x.dtype))
    return torch.stack(cols, dim=1)


def brute_force(x, w_ih, w_hh, b_ih, b_hh, Nc, Nr, x_len=None):
    """the same layer frame by frame: every output frame's reverse state from its own run, nothing shared between frames"""
    T, B, _ = x.shape
    H = w_hh.shape[2]
    p0, p1 = [w[0] for w in (w_ih, w_hh, b_ih, b_hh)], [w[1] for w in (w_ih, w_hh, b_ih, b_hh)]
    y = torch.zeros(T, B, H, dtype=x.dtype)
    for b, n in enumerate(lengths(x_len, T, B)):
        for t in range(n):
            h = torch.zeros(H, dtype=x.dtype)
            for s in range(t + 1):
                h = cell(x[s, b], h, *p0)
            c = t // Nc
            g = torch.zeros(H, dtype=x.dtype)
            for s in range(min((c + 1) * Nc + Nr, n) - 1, t - 1, -1):
                g = cell(x[s, b], g, *p1)
            y[t, b] = h + g
    return y


# ------------------------------------------------------------------------------------------------------------ 16-bit formats
def decode(words, fmt):
    """int16 words of the activation format -> float32"""
    if fmt == "f16":
        return words.view(np.float16).astype(np.float32)
    return (words.view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def encode(values, fmt):
    """float32 -> int16 words, round to nearest even (finite values)"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    if fmt == "f16":
        return values.astype(np.float16).view(np.int16)
    u = values.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


# ------------------------------------------------------------------------------------------------------------ the window kernels
def window_shape(T, B, Nc, Nr):
    """(W, C): the rows of a window and the windows per slot"""
    return min(Nc + Nr, T), -(-T // Nc)


def live_rows(n, c, Nc, W, n_win_b=None):
    if n_win_b is not None and c >= n_win_b:
        return 0
    return int(min(max(n - c * Nc, 0), W))


def gather(x, Nc, Nr, block_only=False, x_len=None, n_win=None):
    """asr_lc_gather: x (T, B, R) -> (xw (W, C * B, R), w_len (C * B) int32).  block_only: ASR_LC_BLOCK (keep = Nc)"""
    T, B, R = x.shape
    W, C = window_shape(T, B, Nc, Nr)
    keep = Nc if block_only else W
    xw = np.zeros((W, C * B, R), dtype=x.dtype)
    w_len = np.zeros((C * B,), dtype=np.int32)
    for b, n in enumerate(lengths(x_len, T, B)):
        for c in range(C):
            L = live_rows(n, c, Nc, W, None if n_win is None else int(n_win[b]))
            w_len[c * B + b] = L
            for j in range(L):
                if L - 1 - j < keep:
                    xw[j, c * B + b] = x[c * Nc + L - 1 - j, b]
    return xw, w_len


def scatter(yw, T, B, Nc, Nr, all_windows=False, addend=None, x_len=None, n_win=None, fmt=None):
    """asr_lc_scatter: yw (W, C * B, R) -> y (T, B, R).  all_windows: ASR_LC_WINDOW.  fmt None: sums in the arrays' own dtype (the
    float64 algebra); "bf16" / "f16": the arrays are int16 words, summed in float32 -- addend first, then ascending block -- and
    rounded once."""
    W, C = window_shape(T, B, Nc, Nr)
    R = yw.shape[2]
    assert yw.shape[:2] == (W, C * B)
    val = (lambda a: a) if fmt is None else (lambda a: decode(a, fmt))
    y = np.zeros((T, B, R), dtype=yw.dtype if fmt is None else np.float32)
    for b, n in enumerate(lengths(x_len, T, B)):
        for t in range(n):
            acc = np.zeros((R,), dtype=y.dtype)
            if addend is not None:
                acc = acc + val(addend[t, b])
            blocks = range(C) if all_windows else (t // Nc,)
            for c in blocks:
                L = live_rows(n, c, Nc, W, None if n_win is None else int(n_win[b]))
                off = t - c * Nc
                if 0 <= off < L:
                    acc = acc + val(yw[L - 1 - off, c * B + b])
            y[t, b] = acc
    if fmt is None:
        return y
    out = encode(y, fmt)
    out[np.arange(T)[:, None] >= np.array(lengths(x_len, T, B))[None, :]] = 0
    return out


class Carry:
    """asr_lc_push on the host: state (K, B, R), K = Nc + Nr - 1, m (B)"""

    def __init__(self, Nc, Nr, B, R, dtype=np.int16):
        self.Nc, self.Nr, self.B, self.R, self.K = Nc, Nr, B, R, Nc + Nr - 1
        self.state = np.zeros((self.K, B, R), dtype=dtype)
        self.m = np.zeros((B,), dtype=np.int32)

    def push(self, chunk, n=None, flush=None):
        """-> (window (K + Tc, B, R), a, w, emit), (B) int32 each"""
        Nc, Nr, B, K = self.Nc, self.Nr, self.B, self.K
        Tc = 0 if chunk is None else chunk.shape[0]
        window = np.zeros((K + Tc, B, self.R), dtype=self.state.dtype)
        a, w, emit = (np.zeros((B,), dtype=np.int32) for _ in range(3))
        for b in range(B):
            mb = int(self.m[b])
            nb = Tc if n is None else int(min(max(n[b], 0), Tc))
            ended = flush is not None and bool(flush[b])
            window[:mb, b] = self.state[:mb, b]
            window[mb:mb + nb, b] = chunk[:nb, b] if nb else 0
            a[b] = mb + nb
            w[b] = -(-a[b] // Nc) if ended else max(0, a[b] - Nr) // Nc
            emit[b] = a[b] if ended else w[b] * Nc
            if nb > 0 or ended:
                rest = a[b] - emit[b]
                assert 0 <= rest <= K
                self.state[:, b] = 0
                self.state[:rest, b] = window[emit[b]:a[b], b]
                self.m[b] = rest
        return window, a, w, emit

    def reset(self, mask=None):
        for b in range(self.B):
            if mask is None or mask[b]:
                self.state[:, b] = 0
                self.m[b] = 0


class ChunkedLayer:
    """The layer fed chunk by chunk, the way asr.model.stream.AcousticStream runs it: the push, the forward direction from the carried
    state over the emitted frames, the reverse direction over the whole blocks as gathered windows, the scatter.  float64."""

    def __init__(self, w_ih, w_hh, b_ih, b_hh, Nc, Nr, B):
        self.p = [w.detach().double() for w in (w_ih, w_hh, b_ih, b_hh)]
        self.Nc, self.Nr, self.B, self.H = Nc, Nr, B, w_hh.shape[2]
        self.carry = Carry(Nc, Nr, B, w_ih.shape[2], dtype=np.float64)
        self.h = torch.zeros(B, self.H, dtype=torch.float64)

    def push(self, chunk, n=None, flush=None):
        """chunk (Tc, B, I) float64 array or None -> (y (K + Tc, B, H) array, of which emit[b] rows are the slot's; emit)"""
        Nc, Nr, B = self.Nc, self.Nr, self.B
        window, a, w, emit = self.carry.push(chunk, n, flush)
        rows = window.shape[0]
        p0, p1 = [q[0] for q in self.p], [q[1] for q in self.p]
        xt = torch.from_numpy(window)
        fwd = np.zeros((rows, B, self.H))
        for b in range(B):
            for t in range(int(emit[b])):
                self.h[b] = cell(xt[t, b], self.h[b], *p0)
                fwd[t, b] = self.h[b].numpy()
        xw, w_len = gather(window, Nc, Nr, False, a, w)
        yw = np.zeros(xw.shape[:2] + (self.H,))
        xwt = torch.from_numpy(xw)
        for i, L in enumerate(w_len):
            h = torch.zeros(self.H, dtype=torch.float64)
            for j in range(int(L)):
                h = cell(xwt[j, i], h, *p1)
                yw[j, i] = h.numpy()
        y = scatter(yw, rows, B, Nc, Nr, False, fwd, a, w) if rows else np.zeros((0, B, self.H))
        return y, emit

    def reset(self, mask=None):
        self.carry.reset(mask)
        for b in range(self.B):
            if mask is None or mask[b]:
                self.h[b] = 0


# ------------------------------------------------------------------------------------------------------------ the model
def stack_frames(h, k, x_len):
    """tests/time_stack_reference.py::fwd in differentiable torch: h (T, B, R) -> ((ceil(T / k), B, k * R), lengths)"""
    Tn, Bn, R = h.shape
    G = -(-Tn // k)
    n = torch.full((Bn,), Tn, dtype=torch.long) if x_len is None else x_len.long().clamp(0, Tn)
    live = (torch.arange(Tn).reshape(Tn, 1) < n.reshape(1, Bn)).unsqueeze(2)
    z = torch.where(live, h, torch.zeros_like(h))
    z = torch.cat([z, torch.zeros(G * k - Tn, Bn, R, dtype=h.dtype)]).reshape(G, k, Bn, R)
    return z.permute(0, 2, 1, 3).reshape(G, Bn, k * R), ((n + k - 1) // k).to(torch.int32)


def oracle(state, cfg, variant=None, dtype=torch.float32):
    """oracle.model.DS2Oracle (float32, or float64 for the distances between restatements) of a ds2.Model built from `cfg`, with the
    restated frame stacking in front of the recurrent layers and, where cfg.latency_control is set, the restated layer for each of
    them (`variant`: one of MUTANTS in every layer)"""
    from oracle import bf16 as Q
    from oracle import model as omodel
    from oracle import nn as onn
    k, control = getattr(cfg, "time_reduction", 1), getattr(cfg, "latency_control", None)

    class LCOracle(omodel.DS2Oracle):
        def forward(self, x, x_len=None):
            h = x.to(dtype)
            for i, pool in enumerate([3] + [2] * (self.nconv - 1)):
                W, b = self.g("conv_blocks._sequential_%d.W" % (4 * i)), self.g("conv_blocks._sequential_%d.b" % (4 * i))
                h = onn.maxpool_h(onn.maxout2(onn.conv2d_causal(h, W, b, 0)), pool)
            Bn, C, H, Tn = h.shape
            h = h.permute(3, 0, 2, 1).reshape(Tn, Bn, H * C)
            if k > 1:
                h, x_len = stack_frames(h, k, x_len)
                Tn = h.shape[0]
            for i in range(self.nrnn):
                pre = "rnn_blocks._sequential_%d." % (2 * i)
                params = [self.g(pre + n) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]
                if control is None:
                    h = Q.gru(h, *params, x_len, False, False, None, False)
                else:
                    h = layer(h, *params, control[0], control[1], x_len, variant)
            for idx in (0, 3):
                W, b = self.g("dense_blocks._sequential_%d.W" % idx), self.g("dense_blocks._sequential_%d.b" % idx)
                h = Q.linear(h, W[:, :, 0], b, False)
                h = h.reshape(Tn, Bn, -1, 2).max(dim=3)[0]
            W, b = self.g("dense_blocks._sequential_6.W"), self.g("dense_blocks._sequential_6.b")
            h = Q.linear(h, W[:, :, 0], b, False, f32_out=True)
            return Q.layer_norm_rows(h, self.g("dense_blocks._sequential_7.norm.gamma"), self.g("dense_blocks._sequential_7.norm.beta"))

    ref = LCOracle(state, cfg.num_conv_layers, cfg.num_rnn_layers, bidirectional=cfg.bidirectional, matched=False)
    return ref.to(dtype)
