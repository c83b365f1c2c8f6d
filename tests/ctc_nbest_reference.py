"""Float64 restatement of the N-best CTC scoring (csrc/ctc_nbest.hip) and of the MWER arithmetic (asr/loss/nbest.py); a test
helper, not collected.  It is the oracle of tests/test_ctc_nbest_cpu.py and tests/test_ctc_nbest_gpu.py.

log p(h_n | x_b) per slot, by case:
  * hyp_len < 0 (unused) and hypotheses without a path (x_len < len + number of adjacent repeats, decided HERE, explicitly):
    -inf, zero gradient.  oracle.ctc does not handle them (it returns 1e10 for an infeasible path);
  * hyp_len == 0: the closed form sum_{t < x_len} log softmax(x[t])[blank], gradient onehot(blank) - softmax (kept as a statement
    of its own beside oracle.ctc's empty labelling);
  * everything else: oracle.ctc.ctc_loss_grad on that utterance's logits, reduce="no": logp = -loss, d logp = -d loss.
"""
import numpy as np

from oracle import ctc as octc

NEG = -np.inf


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def feasible(h, length, x_len):
    """a labelling of `length` tokens needs one frame per token and one blank frame between equal neighbours"""
    if length < 0:
        return False
    h = np.asarray(h[:length])
    repeats = int((h[1:] == h[:-1]).sum()) if length > 1 else 0
    return x_len >= length + repeats and x_len > 0


def slot_logp_grad(x_b, h, length, x_len, blank=0):
    """x_b (T, V) logits of one utterance -> (log p(h | x_b) float64, d log p / d x_b (T, V) float64)"""
    x_b = np.asarray(x_b, np.float64)
    T, V = x_b.shape
    g = np.zeros((T, V))
    if not feasible(h, length, x_len):
        return NEG, g
    if length == 0:
        lp = log_softmax64(x_b[:x_len])
        g[:x_len] = -np.exp(lp)
        g[:x_len, blank] += 1.0
        return float(lp[:, blank].sum()), g
    loss, grad = octc.ctc_loss_grad(x_b[:, None, :], np.asarray(h)[None, :], blank, np.array([x_len]), np.array([length]), "no")
    return -float(loss[0]), -grad[:, 0]


def nbest_logp_grad(xs, hyps, hyp_len, x_len=None, blank=0, want_grad=True):
    """xs (T, B, V), hyps (B, N, L), hyp_len (B, N), x_len (B) or None -> logp (B, N) float64 and, with want_grad, the list
    g[b][n] of (T, V) gradients of logp[b, n] with respect to xs[:, b]"""
    xs = np.asarray(xs)
    T, B, V = xs.shape
    N = hyps.shape[1]
    if x_len is None:
        x_len = np.full(B, T)
    logp = np.full((B, N), NEG)
    grads = [[None] * N for _ in range(B)]
    for b in range(B):
        for n in range(N):
            logp[b, n], g = slot_logp_grad(xs[:, b], hyps[b, n], int(hyp_len[b, n]), int(x_len[b]), blank)
            if want_grad:
                grads[b][n] = g
    return (logp, grads) if want_grad else logp


def weighted_grad(grads, gy, B, N, T, V):
    """(sum_n gy[b, n] g[b][n], sum_n |gy[b, n] g[b][n]|) as (T, B, V) arrays; slots whose gradient is all zero (unused /
    infeasible) are skipped whatever their gy holds"""
    tot = np.zeros((T, B, V))
    mag = np.zeros((T, B, V))
    for b in range(B):
        for n in range(N):
            if np.any(grads[b][n]):
                tot[:, b] += gy[b, n] * grads[b][n]
                mag[:, b] += np.abs(gy[b, n] * grads[b][n])
    return tot, mag


def levenshtein(r, h):
    r, h = list(r), list(h)
    if len(r) == 0:
        return len(h)
    d = list(range(len(h) + 1))
    for i in range(1, len(r) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(h) + 1):
            cur = d[j]
            d[j] = min(prev + (r[i - 1] != h[j - 1]), d[j] + 1, d[j - 1] + 1)
            prev = cur
    return d[len(h)]


def errors(hyps, hyp_len, ref, ref_len, normalize=False):
    """(B, N) float64 edit distance of every slot to its utterance's transcript (unused slots count as empty)"""
    B, N = hyp_len.shape
    e = np.zeros((B, N))
    for b in range(B):
        r = ref[b, :ref_len[b]]
        for n in range(N):
            e[b, n] = levenshtein(r, hyps[b, n, :max(0, hyp_len[b, n])])
            if normalize:
                e[b, n] /= max(1, ref_len[b])
    return e


def mwer(logp, e):
    """logp, e (B, N) float64 -> (loss_b (B), posteriors (B, N), coefficients d loss_b / d logp (B, N), spread sum_n |e_n - mean e|
    (B)), all over the slots with finite logp; the others get posterior and coefficient 0"""
    logp, e = np.asarray(logp, np.float64), np.asarray(e, np.float64)
    B, N = logp.shape
    loss, post, coef, spread = np.zeros(B), np.zeros((B, N)), np.zeros((B, N)), np.zeros(B)
    for b in range(B):
        S = np.nonzero(np.isfinite(logp[b]))[0]
        if len(S) == 0:
            continue
        p = np.exp(logp[b, S] - logp[b, S].max())
        p /= p.sum()
        ebar = e[b, S].mean()
        post[b, S] = p
        loss[b] = (p * (e[b, S] - ebar)).sum()
        coef[b, S] = p * (e[b, S] - (p * e[b, S]).sum())
        spread[b] = np.abs(e[b, S] - ebar).sum()
    return loss, post, coef, spread


def with_reference(hyps, hyp_len, ref, ref_len, blank=0):
    """the hypothesis set of mwer_loss(add_reference=True): the transcript appended as slot N, unused (-1) where a slot in use
    already equals it"""
    B, N, L = hyps.shape
    W = max(L, ref.shape[1])
    out = np.full((B, N + 1, W), blank, np.int32)
    out[:, :N, :L] = hyps
    out[:, N, :ref.shape[1]] = ref
    lens = np.concatenate([hyp_len, np.zeros((B, 1), hyp_len.dtype)], axis=1).astype(np.int32)
    for b in range(B):
        r = list(ref[b, :ref_len[b]])
        listed = any(hyp_len[b, n] >= 0 and list(hyps[b, n, :hyp_len[b, n]]) == r for n in range(N))
        lens[b, N] = -1 if listed else ref_len[b]
    return out, lens


def random_case(T, B, V, N, L, seed):
    """The inputs of the random GPU cases: ragged x_len with x_len[0] = T, ragged hyp_len with one slot at full L, a repeated label
    in every hypothesis (hyp[..., 2] = hyp[..., 1]), one empty hypothesis, one unused slot, one infeasible hypothesis (the last
    utterance's x_len is cut below len + repeats of ITS slot 0, which is at full L), gy ~ N(0, 1) with NaN at the unused and the
    infeasible slot.  -> xs (T, B, V) f32, hyps (B, N, L) i32, hyp_len (B, N) i32, x_len (B) i32, gy (B, N) f32, dead (B, N) bool"""
    assert B >= 2 and N >= 2 and L >= 3
    rs = np.random.RandomState(seed)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    hyps = rs.randint(1, min(V, 119), size=(B, N, L)).astype(np.int32)
    hyps[..., 2] = hyps[..., 1]
    hyp_len = rs.randint(max(3, L // 2), L + 1, size=(B, N)).astype(np.int32)
    x_len = rs.randint(3 * L, T + 1, size=B).astype(np.int32)
    x_len[0] = T
    hyp_len[0, 0] = L                           # full length, feasible
    hyp_len[0, 1] = 0                           # the empty hypothesis
    hyp_len[B - 1, N - 1] = -1                  # unused
    hyp_len[B - 1, 0] = L                       # infeasible: L tokens + at least one repeat > x_len = L
    x_len[B - 1] = L
    dead = np.zeros((B, N), bool)
    dead[B - 1, N - 1] = True
    for n in range(N):                          # whatever else does not fit into L frames in the last utterance
        dead[B - 1, n] |= not feasible(hyps[B - 1, n], int(hyp_len[B - 1, n]), L)
    assert dead[B - 1, 0]
    gy = rs.randn(B, N).astype(np.float32)
    gy[dead] = np.nan
    return xs, hyps, hyp_len, x_len, gy, dead
