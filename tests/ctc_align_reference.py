"""Float64 restatement of the CTC / Gram-CTC forced alignment of csrc/ctc_align.hip (a test helper, not collected).

The lattice is the one of ``oracle.ctc`` (``ctc_lattice`` / ``gram_lattice``), which is pinned to the reference's goldens.  The
sweep is ``cur[s] = max_j prev[s - k_j] + float64(logit[t, s])`` on the RAW f32 logits -- exactly one IEEE float64 addition per
step, as on the device, so the two sides take bit-identical decisions.  Tie rule: among equal candidates the smallest diagonal
offset wins (a later candidate replaces an earlier one only if it is strictly larger); among equal final nodes the largest node
index.  ``brute_force`` enumerates all V^T paths of a tiny case instead.
"""
import itertools

import numpy as np

from oracle import ctc as octc

NEG = -np.inf
NAMES = ("frames", "tokens", "positions", "starts", "ends", "token_logp", "n_tokens", "score")


def _lattice(uni, big, L, blank):
    if big is None:
        if L == 0:          # oracle.ctc_lattice cannot take L = 0: the path is the one blank node
            return np.array([blank]), np.ones(1, bool), np.ones((3, 1), bool) & (np.arange(3)[:, None] == 0), np.ones(1, bool)
        return octc.ctc_lattice(uni, L, blank)
    return octc.gram_lattice(uni, big, L, blank)


def align_one(x, uni, big, xl, L, blank):
    """x (T, V) f32 logits, uni / big (Lmax,) labels (big None: CTC) -> dict of the ABI's outputs for one utterance"""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    Lmax = len(uni)
    xl = T if xl is None else min(int(xl), T)
    L = Lmax if L is None else min(max(int(L), 0), Lmax)
    gram = big is not None
    ks = octc.GRAM_KS if gram else octc.CTC_KS
    out = dict(frames=np.full(T, blank, np.int32), tokens=np.full(Lmax, blank, np.int32), positions=np.zeros(Lmax, np.int32),
               starts=np.zeros(Lmax, np.int32), ends=np.zeros(Lmax, np.int32), token_logp=np.zeros(Lmax, np.float64),
               n_tokens=0, score=NEG)
    if xl <= 0:
        return out
    labels, alive, allowed, final = _lattice(np.asarray(uni), None if big is None else np.asarray(big), L, blank)
    N = labels.shape[0]
    dead = ~alive | (labels < 0) | (labels >= V)            # the device drops every id outside [0, V)
    logit = np.where(dead[None, :], NEG, x[:xl][:, np.where(dead, 0, labels)].astype(np.float64))
    prev = np.full(N, NEG)
    prev[0] = 0.0
    bp = np.zeros((xl, N), np.int8)
    for t in range(xl):
        best = np.where(allowed[0], prev, NEG)
        code = np.zeros(N, np.int8)
        for j, k in enumerate(ks):
            if j == 0 or k >= N:
                continue
            cand = np.full(N, NEG)
            cand[k:] = np.where(allowed[j, k:], prev[:N - k], NEG)
            better = cand > best
            best = np.where(better, cand, best)
            code = np.where(better, j, code).astype(np.int8)
        prev = best + logit[t]
        bp[t] = code
    s, bv = -1, NEG
    for q in range(N - 1, -1, -1):                          # equal final nodes: the largest index
        if final[q] and not dead[q] and prev[q] > bv:
            s, bv = q, prev[q]
    if s < 0:
        return out
    states = np.zeros(xl, np.int64)
    for t in range(xl - 1, -1, -1):
        states[t] = s
        s -= ks[bp[t, s]]
    lp = octc.log_softmax(x[:xl].astype(np.float64), axis=1)
    per = 3 if gram else 2
    n = 0
    for t in range(xl):
        s = states[t]
        out["frames"][t] = labels[s]
        if s % per == 0:
            continue
        if t == 0 or states[t - 1] != s:
            out["tokens"][n] = labels[s]
            out["positions"][n] = (s - 1) // 2 if not gram else (s // 3 if s % 3 == 1 else s // 3 - 1)
            out["starts"][n] = t
            n += 1
        out["ends"][n - 1] = t + 1
        out["token_logp"][n - 1] += lp[t, labels[s]]
    out["n_tokens"] = n
    out["score"] = float(lp[np.arange(xl), out["frames"][:xl]].sum())
    return out


def align_batch(xs, uni, big, x_len, l_len, blank):
    """xs (T, B, V); returns a dict of stacked arrays, named as the fields of asr.loss.Alignment"""
    xs = np.asarray(xs)
    B = xs.shape[1]
    rows = [align_one(xs[:, b], uni[b], None if big is None else big[b], None if x_len is None else x_len[b],
                      None if l_len is None else l_len[b], blank) for b in range(B)]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in NAMES}


def _accept_ctc(path, target, blank):
    col, prev = [], blank
    for c in path:
        if c != blank and c != prev:
            col.append(c)
        prev = c
    return col == target


def _accept_gram(path, u, g, blank):
    col, prev = [], blank
    for c in path:
        if c != blank and c != prev:
            col.append(c)
        prev = c
    p, L = 0, len(u)
    for c in col:
        if p < L and c == u[p]:
            p += 1
        elif p + 1 < L and g[p + 1] != -1 and c == g[p + 1]:
            p += 2
        else:
            return False
    return p == L


def brute_force(x, uni, big, L, blank):
    """best path among all V^T paths of x (T, V) that spell the labels: (score, frames) or (-inf, None)"""
    lp = octc.log_softmax(np.asarray(x, np.float64), axis=1)
    T, V = lp.shape
    u = [int(v) for v in uni[:L]]
    g = None if big is None else [int(v) for v in big[:L]]
    best, arg = NEG, None
    for path in itertools.product(range(V), repeat=T):
        if not (_accept_ctc(path, u, blank) if g is None else _accept_gram(path, u, g, blank)):
            continue
        s = float(sum(lp[t, path[t]] for t in range(T)))
        if s > best:
            best, arg = s, path
    return best, (None if arg is None else np.array(arg, np.int32))


# ------------------------------------------------------------------------------------------------ cases
def tiny_ctc_cases():
    """(x (T, V), uni (Lmax,), L): random ones, then repeated labels, a too-short input (infeasible) and an empty transcript"""
    rs = np.random.RandomState(11)
    cases = []
    for _ in range(12):
        T, V = rs.randint(1, 6), rs.randint(2, 5)
        L = rs.randint(0, min(T, 3) + 1)
        cases.append(((rs.randn(T, V) * 2).astype(np.float32), rs.randint(1, V, size=max(L, 1)).astype(np.int32), L))
    x = (rs.randn(5, 3) * 2).astype(np.float32)
    cases.append((x, np.array([1, 1, 2], np.int32), 3))             # repeat: needs the blank between
    cases.append((x[:3], np.array([1, 1, 2], np.int32), 3))         # 3 frames cannot hold 1 _ 1 2: infeasible
    cases.append((x, np.array([2, 2], np.int32), 2))
    cases.append((x, np.array([1, 2], np.int32), 0))
    return cases


def tiny_gram_cases():
    """(x (T, 7), uni, big, L): V = 7 = blank, unigrams 1-2, bigram ids 3-6; 70 % of the bigrams on offer.  Includes repeated
    unigrams, equal bigrams two apart, absent bigrams and an infeasible case"""
    rs = np.random.RandomState(12)
    cases = []
    for _ in range(14):
        T = rs.randint(1, 6)
        L = rs.randint(1, 5)
        u = rs.randint(1, 3, size=L).astype(np.int32)
        g = np.where(rs.rand(L) < 0.7, rs.randint(3, 7, size=L), -1).astype(np.int32)
        g[0] = -1
        cases.append(((rs.randn(T, 7) * 2).astype(np.float32), u, g, L))
    x = (rs.randn(5, 7) * 2).astype(np.float32)
    x2 = x.copy()
    x2[:, 3] += 4.0
    cases.append((x2, np.array([1, 2, 1, 2], np.int32), np.array([-1, 3, 4, 3], np.int32), 4))    # bigram 3 twice, two apart
    cases.append((x, np.array([1, 1, 1], np.int32), np.array([-1, -1, -1], np.int32), 3))         # repeats, no bigrams
    cases.append((x[:2], np.array([1, 1, 1], np.int32), np.array([-1, -1, 5], np.int32), 3))      # infeasible in 2 frames
    cases.append((x2, np.array([2, 2, 1], np.int32), np.array([-1, 3, 3], np.int32), 3))
    return cases


def _perturb(rs, labels, lo, hi):
    out = []
    for c in labels:
        r = rs.rand()
        if r < 0.08:
            continue                                    # deleted
        out.append(int(rs.randint(lo, hi)) if r < 0.20 else int(c))      # substituted
        if r > 0.93:
            out.append(int(rs.randint(lo, hi)))         # inserted
    return out


def full_case(kind, gram, seed, B=32, T=1000, V=3000, Lmax=120, blank=0):
    """The BASELINE shape: L ~ U{40..120}, x_len ~ U{600..1000}.  kind "randn": flat logits; "peaky": a peaked path whose labels
    the transcript perturbs (substitutions, deletions, insertions), so the alignment has to disagree with the argmax.
    Gram-CTC: unigram ids U{1..118}, bigram ids U{119..2999}, P(-1) = 0.3, bigram[:, 0] = -1; its peaky variant boosts, per label
    position and on a short run of frames, either the unigram or the bigram on offer."""
    from ctc_beam_reference import peaky
    rs = np.random.RandomState(seed)
    x_len = rs.randint(600, T + 1, size=B).astype(np.int32)
    l_len = rs.randint(40, Lmax + 1, size=B).astype(np.int32)
    uhi = 119 if gram else V
    uni = rs.randint(1, uhi, size=(B, Lmax)).astype(np.int32)
    big = None
    if gram:
        big = np.where(rs.rand(B, Lmax) < 0.3, -1, rs.randint(119, V, size=(B, Lmax))).astype(np.int32)
        big[:, 0] = -1
    xs = rs.randn(T, B, V).astype(np.float32)
    if kind == "peaky" and not gram:
        for b in range(B):
            xs[:, b] = peaky(rs, T, V, blank)
            ids = xs[:x_len[b], b].argmax(axis=1)
            col = [int(c) for i, c in enumerate(ids) if c != blank and (i == 0 or c != ids[i - 1])]
            lab = _perturb(rs, col, 1, V)[:l_len[b]]
            l_len[b] = len(lab)
            uni[b, :len(lab)] = lab
    elif kind == "peaky":
        for b in range(B):
            L, xl = int(l_len[b]), int(x_len[b])
            toks, i = [], 0
            while i < L:
                if i + 1 < L and big[b, i + 1] >= 0 and rs.rand() < 0.5:
                    toks.append(int(big[b, i + 1]))
                    i += 2
                else:
                    toks.append(int(uni[b, i]))
                    i += 1
            starts = np.sort(rs.choice(np.arange(1, xl - 4, 4), size=len(toks), replace=False))
            tgt = np.full(T, blank)
            for k, s in enumerate(starts):
                tgt[s:s + rs.randint(1, 4)] = toks[k]
            xs[np.arange(T), b, tgt] += rs.uniform(7.0, 14.0, size=T).astype(np.float32)
            sub = rs.rand(L) < 0.12                      # the transcript differs from what was boosted
            uni[b, :L] = np.where(sub, rs.randint(1, 119, size=L), uni[b, :L])
    return xs, uni, big, x_len, l_len
