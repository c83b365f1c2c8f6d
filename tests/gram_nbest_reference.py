"""Float64 restatement of the N-best Gram-CTC scoring (asr_gram_ctc_nbest_*, csrc/ctc_nbest.hip); a test helper, not collected.
It is the oracle of tests/test_gram_ctc_nbest_cpu.py and tests/test_gram_ctc_nbest_gpu.py.  The MWER arithmetic, the edit
distance and the hypothesis set with the transcript appended are tests/ctc_nbest_reference.py's (re-exported here): they do not
depend on the lattice.

log p(string_n | x_b) per slot, by case, each decided HERE, explicitly:
  * hyp_len < 0 (unused), x_len <= 0, or a character without a unigram token in the table (a negative or out-of-range character
    included): -inf, zero gradient.  oracle.ctc models only dead BIGRAM nodes, and the device treats such a slot as unused;
  * hyp_len == 0: the closed form sum_{t < x_len} log softmax(x[t])[blank], gradient onehot(blank) - softmax;
  * everything else: oracle.ctc.gram_ctc_loss_grad on that utterance's logits, reduce="no", with
    label_unigram[i] = the token of (s[i]) (gram_beam_reference.unigram_ids) and label_bigram[i] = the token of (s[i-1], s[i]) or
    -1 (gram_beam_reference.label_bigrams): logp = -loss and d logp = -d loss where the oracle's total is finite (its loss is not
    the 1e10 it reports for a lattice without a path, e.g. a string of more than 2 x_len characters), else -inf and zero.
"""
import numpy as np

import gram_beam_reference as gref
from ctc_nbest_reference import NEG, errors, levenshtein, log_softmax64, mwer, weighted_grad, with_reference  # noqa: F401
from oracle import ctc as octc

INFEASIBLE = 1e10            # oracle.ctc._loss_grad's loss of a lattice without a path


def slot_logp_grad(x_b, s, length, x_len, gram, blank=0, uni=None):
    """x_b (T, V) logits of one utterance, s the characters -> (log p(s | x_b) float64, d log p / d x_b (T, V) float64)"""
    x_b = np.asarray(x_b, np.float64)
    T, V = x_b.shape
    g = np.zeros((T, V))
    uni = gref.unigram_ids(gram) if uni is None else uni
    if length < 0 or x_len <= 0:
        return NEG, g
    s = [int(c) for c in np.asarray(s)[:length]]
    if any(c not in uni for c in s):
        return NEG, g
    if length == 0:
        lp = log_softmax64(x_b[:x_len])
        g[:x_len] = -np.exp(lp)
        g[:x_len, blank] += 1.0
        return float(lp[:, blank].sum()), g
    lu = np.array([[uni[c] for c in s]])
    lb = np.array([gref.label_bigrams(s, gram)])
    loss, grad = octc.gram_ctc_loss_grad(x_b[:, None, :], lu, lb, blank, np.array([x_len]), np.array([length]), "no")
    if loss[0] >= INFEASIBLE:
        return NEG, g
    return -float(loss[0]), -grad[:, 0]


def nbest_logp_grad(xs, hyps, hyp_len, gram, x_len=None, blank=0, want_grad=True):
    """xs (T, B, V), hyps (B, N, L) characters, hyp_len (B, N), gram (V, 2), x_len (B) or None -> logp (B, N) float64 and, with
    want_grad, the list g[b][n] of (T, V) gradients of logp[b, n] with respect to xs[:, b]"""
    xs = np.asarray(xs)
    T, B, V = xs.shape
    N = hyps.shape[1]
    if x_len is None:
        x_len = np.full(B, T)
    uni = gref.unigram_ids(gram)
    logp = np.full((B, N), NEG)
    grads = [[None] * N for _ in range(B)]
    for b in range(B):
        for n in range(N):
            length = min(int(hyp_len[b, n]), hyps.shape[2])
            logp[b, n], g = slot_logp_grad(xs[:, b], hyps[b, n], length, int(x_len[b]), gram, blank, uni)
            if want_grad:
                grads[b][n] = g
    return (logp, grads) if want_grad else logp


def shuffled_table(U, G, seed, extra=0):
    """A table whose unigram token ids differ from the characters they spell, so that nothing works without the spelling index:
    V = 1 + U + G + extra, blank 0, characters 1..U; the U unigram rows and G distinct random ordered pairs are dealt onto the
    token ids 1..V-1 in random order, `extra` ids spell nothing.  -> gram (V, 2) int32"""
    rs = np.random.RandomState(seed)
    V = 1 + U + G + extra
    every = [(a, b) for a in range(1, U + 1) for b in range(1, U + 1)]
    pairs = [every[i] for i in rs.choice(len(every), size=G, replace=False)]
    rows = [(u, -1) for u in range(1, U + 1)] + pairs + [(-1, -1)] * extra
    gram = np.full((V, 2), -1, np.int32)
    gram[1 + rs.permutation(V - 1)] = np.array(rows, np.int32)
    assert sum(int(gram[u, 0]) == u and gram[u, 1] < 0 for u in range(1, U + 1)) < U      # some unigram is not its own id
    return gram


def table_pairs(gram):
    return [(int(a), int(b)) for a, b in np.asarray(gram).tolist() if a >= 0 and b >= 0]


def random_case(T, B, N, L, gram, seed):
    """The inputs of the random GPU cases over the table `gram`: ragged x_len (x_len[0] = T; 3 T / 4 if B = 1) and ragged hyp_len.
    Every string has a doubled character at positions 1, 2 (the u[i] != u[i-1] guard) and, for L >= 7, "abab" at positions 3..6
    with (a, b) a bigram of the table (the g[i] != g[i-2] guard); for L < 7 slot (0, 0) is "abab" + one character.  Slots, as far
    as B * N has room for them (a character outside the table makes a slot unused on the device, so it goes before the plain
    unused slot):
      (0, 0)      full length L, ending (L >= 7) in a pair of different characters that the table does not have; for L < 7 that
                  pair ends slot (1, 0), also at full length (needs B >= 3)
      (0, 1)      the empty string
      (0, 2)      a character outside the table (V + 3) in the middle       [N = 2: slot (B-1, N-1) instead]
      (0, 3)      a negative character                                      [N >= 4]
      (B-1, 0)    too long: L characters, and the last utterance's x_len = (L - 1) // 2 < L / 2        [B >= 2]
      (B-1, N-1)  unused (hyp_len -1)                                       [B >= 2 and N >= 3]
    -> xs (T, B, V) f32, hyps (B, N, L) i32, hyp_len (B, N) i32, x_len (B) i32, gy (B, N) f32 ~ N(0, 1).  The caller puts NaN
    into gy where the restatement's log p is -inf."""
    assert N >= 2 and L >= 5 and (L >= 7 or B >= 3)
    gram = np.asarray(gram)
    V = len(gram)
    rs = np.random.RandomState(seed)
    chars = sorted(gref.unigram_ids(gram))
    pairs = table_pairs(gram)
    have = set(pairs)
    missing = [(p, q) for p in chars for q in chars if (p, q) not in have and p != q]
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    hyps = np.array(chars, np.int32)[rs.randint(len(chars), size=(B, N, L))]
    hyps[..., 2] = hyps[..., 1]
    hyp_len = rs.randint(max(3, L // 2), L + 1, size=(B, N)).astype(np.int32)
    a, b = pairs[rs.randint(len(pairs))]
    pq = missing[rs.randint(len(missing))]
    hyp_len[0, 0] = L
    if L >= 7:
        hyps[..., 3:7] = (a, b, a, b)
        hyps[0, 0, L - 2:L] = pq
    else:
        hyps[0, 0, 0:4] = (a, b, a, b)
        hyps[1, 0, L - 2:L] = pq
        hyp_len[1, 0] = L
    x_len = rs.randint(min(3 * L, T), T + 1, size=B).astype(np.int32)
    x_len[0] = T if B > 1 else 3 * T // 4
    hyp_len[0, 1] = 0
    outside = (0, 2) if N >= 3 else (B - 1, N - 1)
    hyp_len[outside] = L
    hyps[outside][L // 2] = V + 3
    if N >= 4:
        hyp_len[0, 3] = L
        hyps[0, 3, 0] = -1
    if B >= 2:
        hyp_len[B - 1, 0] = L
        x_len[B - 1] = (L - 1) // 2
        if N >= 3:
            hyp_len[B - 1, N - 1] = -1
    gy = rs.randn(B, N).astype(np.float32)
    return xs, hyps, hyp_len, x_len, gy
