"""NumPy float64 restatement of the Gram-CTC keyword search (csrc/ctc_kws.hip: gram_sweep_kernel), a brute
force over every span and every label sequence for tiny cases, and the case generators of tests/test_gram_keyword_cpu.py and
tests/test_gram_keyword_gpu.py.  Test infrastructure: nothing in the package imports it.

A phrase is a string of characters (unigram ids); `gram` is the (V, 2) table of asr.vocab.gram_table.  Position i (1-based) has the
nodes U_i (the token spelled c_i), G_i (the token spelled c_{i-1} c_i, i >= 2) and B_i (the blank between positions i-1 and i,
i >= 2).  The restatement runs the recurrences of include/asr_hip.h as written: IEEE float64 max and ONE addition per step on
c(t, v) = (double)x[t][v] - (double)xmax[t], `best` scanning its candidates in the order written (a later one wins only if it is
strictly larger), the start frame travelling with the winner, start -1 for a node whose new value is -inf.  It is vectorised over
keywords and positions, with one Python loop over the frames.  The non-maximum suppression is keyword_reference.hits, imported.
"""
import itertools

import numpy as np

from keyword_reference import hits, peaked, random_logits  # noqa: F401  (re-exported for the tests)

NEG = -np.inf


def is_dead(p, V, blank):
    return len(p) == 0 or min(p) < 0 or max(p) >= V or blank in p


def token_maps(gram):
    """character -> its unigram token id, (c1, c2) -> its bigram token id"""
    g = np.asarray(gram)
    uni = {int(a): v for v, (a, b) in enumerate(g) if a >= 0 and b < 0}
    big = {(int(a), int(b)): v for v, (a, b) in enumerate(g) if a >= 0 and b >= 0}
    return uni, big


def _best(cands):
    """the first maximum of [(value, start), ..] element-wise, in the order given"""
    m, s = cands[0]
    for v, st in cands[1:]:
        w = v > m
        m = np.where(w, v, m)
        s = np.where(w, st, s)
    return m, s


def _shift(a, d, fill):
    out = np.full_like(a, fill)
    out[:, d:] = a[:, :a.shape[1] - d]
    return out


def detect(x, xl, phrases, gram, blank=0, state=None):
    """x (T, V) f32, xl valid frames, phrases: list of character sequences -> det (K, T) f32, start (K, T) int32, fill (T) f32.
    `state`: None, or the dict a previous call returned as its fourth value (the stream form)."""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    K = len(phrases)
    Lmax = max(1, max(len(p) for p in phrases))
    uni, big = token_maps(gram)
    ch = np.full((K, Lmax), -1, np.int64)               # the characters; -1 where padded and in a dead phrase
    uid = np.zeros((K, Lmax), np.int64)
    gid = np.zeros((K, Lmax), np.int64)
    has_u = np.zeros((K, Lmax), bool)
    has_g = np.zeros((K, Lmax), bool)
    has_b = np.zeros((K, Lmax), bool)
    for k, p in enumerate(phrases):
        if is_dead(p, V, blank):
            continue
        ch[k, :len(p)] = p
        has_b[k, 1:len(p)] = True
        for i, c in enumerate(p):
            if c in uni:
                uid[k, i], has_u[k, i] = uni[c], True
            if i and (p[i - 1], c) in big:
                gid[k, i], has_g[k, i] = big[(p[i - 1], c)], True
    live = ch[:, 0] >= 0
    last = np.array([max(len(p), 1) - 1 for p in phrases])
    same_u = np.zeros((K, Lmax), bool)                  # c_i == c_{i-1}
    same_u[:, 1:] = (ch[:, 1:] == ch[:, :-1]) & (ch[:, 1:] >= 0)
    same_g = np.zeros((K, Lmax), bool)                  # g_i == g_{i-2}: the same two characters two positions back
    same_g[:, 3:] = (ch[:, 3:] == ch[:, 1:-2]) & (ch[:, 2:-1] == ch[:, :-3]) & (ch[:, 3:] >= 0)
    if state is None:
        neg, none = np.full((K, Lmax), NEG), np.full((K, Lmax), -1, np.int64)
        state = dict(u=neg, b=neg.copy(), g=neg.copy(), us=none, bs=none.copy(), gs=none.copy(), base=0)
    u, b, g, us, bs, gs, base = (state[n] for n in ("u", "b", "g", "us", "bs", "gs", "base"))
    det = np.full((K, T), NEG, np.float32)
    start = np.full((K, T), -1, np.int32)
    fill = np.zeros(T, np.float32)
    rows = np.arange(K)
    for t in range(min(xl, T)):
        xmax = x[t].max()                               # f32
        xd = x[t].astype(np.float64) - np.float64(xmax)
        cu = np.where(has_u, xd[uid], NEG)
        cg = np.where(has_g, xd[gid], NEG)
        cb = np.where(has_b, xd[blank], NEG)
        u1, u1s = _shift(u, 1, NEG), _shift(us, 1, -1)
        g1, g1s = _shift(g, 1, NEG), _shift(gs, 1, -1)
        b1, b1s = _shift(b, 1, NEG), _shift(bs, 1, -1)
        u2, u2s = _shift(u, 2, NEG), _shift(us, 2, -1)
        g2, g2s = _shift(g, 2, NEG), _shift(gs, 2, -1)
        u1[:, 0], u1s[:, 0] = 0.0, base + t             # the fresh start of U_1
        if Lmax > 1:
            u2[:, 1], u2s[:, 1] = 0.0, base + t         # the fresh start of G_2
        u1g = np.where(same_u, NEG, u1)
        g2g = np.where(same_g, NEG, g2)
        nb, nbs = _best([(b, bs), (u1, u1s), (g1, g1s)])
        nu, nus = _best([(u, us), (b, bs), (u1g, u1s), (g1, g1s)])
        ng, ngs = _best([(g, gs), (b1, b1s), (u2, u2s), (g2g, g2s)])
        u, b, g = cu + nu, cb + nb, cg + ng
        us, bs, gs = np.where(np.isneginf(u), -1, nus), np.where(np.isneginf(b), -1, nbs), np.where(np.isneginf(g), -1, ngs)
        d, ds = _best([(u[rows, last], us[rows, last]), (g[rows, last], gs[rows, last])])
        det[:, t] = np.where(live, d, NEG).astype(np.float32)
        start[:, t] = np.where(live, ds, -1)
        lse = np.float64(xmax) + np.log(np.exp(x[t].astype(np.float64) - np.float64(xmax)).sum())
        fill[t] = np.float64(xmax) - lse
    return det, start, fill, dict(u=u, b=b, g=g, us=us, bs=bs, gs=gs, base=base + min(xl, T))


def search(xs, lengths, phrases, gram, blank=0, max_hits=4, min_score=NEG):
    """xs (T, B, V) -> dict of det, start (B, K, T), fill (B, T), hit_start, hit_end, hit_score, hit_logp (B, K, H), n_hits (B, K)"""
    T, B, V = xs.shape
    K = len(phrases)
    out = dict(det=np.zeros((B, K, T), np.float32), start=np.zeros((B, K, T), np.int32), fill=np.zeros((B, T), np.float32),
               hit_start=np.zeros((B, K, max_hits), np.int32), hit_end=np.zeros((B, K, max_hits), np.int32),
               hit_score=np.zeros((B, K, max_hits), np.float32), hit_logp=np.zeros((B, K, max_hits), np.float32),
               n_hits=np.zeros((B, K), np.int32))
    for b in range(B):
        xl = T if lengths is None else int(lengths[b])
        out["det"][b], out["start"][b], out["fill"][b], _ = detect(xs[:, b], xl, phrases, gram, blank)
        for k in range(K):
            h = hits(out["det"][b, k], out["start"][b, k], out["fill"][b], xl, max_hits, min_score)
            (out["hit_start"][b, k], out["hit_end"][b, k], out["hit_score"][b, k], out["hit_logp"][b, k], out["n_hits"][b, k]) = h
    return out


def tokenisations(phrase, gram):
    """every way of cutting `phrase` into tokens of the inventory, as tuples of token ids (Fibonacci(L) at the most)"""
    uni, big = token_maps(gram)
    p = tuple(phrase)

    def cut(i):
        if i == len(p):
            yield ()
            return
        if p[i] in uni:
            for rest in cut(i + 1):
                yield (uni[p[i]],) + rest
        if i + 1 < len(p) and (p[i], p[i + 1]) in big:
            for rest in cut(i + 2):
                yield (big[(p[i], p[i + 1])],) + rest

    return list(cut(0))


# ------------------------------------------------------------------------------------------------ brute force
def spell(seq, gram, blank):
    """collapse repeated labels, drop blanks, spell the rest in characters; None if a label is no token"""
    out, prev = [], None
    for v in seq:
        if v != prev and v != blank:
            a, b = gram[v]
            if a < 0:
                return None
            out += [int(a)] if b < 0 else [int(a), int(b)]
        prev = v
    return out


def brute_force(x, phrase, gram, blank=0):
    """x (T, V) f32, tiny -> best (T, T) float64: best[s, e] = the maximum, over every label sequence on frames s..e that starts
    and ends on a token and spells `phrase`, of the left-to-right float64 sum of c(t, label); -inf where there is none.
    Shares nothing with the lattice: it enumerates all V^(e - s + 1) sequences, collapses them as CTC does and spells the rest."""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    c = x.astype(np.float64) - x.max(axis=1).astype(np.float64)[:, None]
    best = np.full((T, T), NEG)
    for s in range(T):
        for e in range(s, T):
            for seq in itertools.product(range(V), repeat=e - s + 1):
                if seq[0] == blank or seq[-1] == blank or spell(seq, gram, blank) != list(phrase):
                    continue
                v = 0.0
                for t, lab in zip(range(s, e + 1), seq):
                    v = v + c[t, lab]
                best[s, e] = max(best[s, e], v)
    return best


# ------------------------------------------------------------------------------------------------ inventories
def table(V, unigrams, bigrams):
    """(V, 2) int32: `unigrams` {token id: character}, `bigrams` {token id: (c1, c2)}; every other row (-1, -1)"""
    g = np.full((V, 2), -1, np.int32)
    for v, c in unigrams.items():
        g[v, 0] = c
    for v, cc in bigrams.items():
        g[v] = cc
    return g


A, Bc = 1, 2
SMALL = table(6, {1: A, 2: Bc}, {3: (A, Bc), 4: (A, A), 5: (Bc, A)})          # a, b, ab, aa, ba
NO_B = table(6, {1: A}, {3: (A, Bc), 4: (A, A), 5: (Bc, A)})                  # the character b has no unigram token (id 2 is unused)
NINE = table(9, {1: 1, 2: 2, 3: 3, 4: 4}, {5: (1, 2), 6: (2, 1), 7: (3, 3), 8: (3, 4)})   # a b c d, ab ba cc cd


def plain(V):
    """an inventory without bigrams: token v spells the character v"""
    return table(V, {v: v for v in range(1, V)}, {})


def big_table(n_uni=20, V=300, seed=0):
    """characters 1..n_uni with their unigram tokens, then V - 1 - n_uni random bigrams"""
    rs = np.random.RandomState(seed)
    pairs = [(a, b) for a in range(1, n_uni + 1) for b in range(1, n_uni + 1)]
    pick = rs.permutation(len(pairs))[:V - 1 - n_uni]
    return table(V, {v: v for v in range(1, n_uni + 1)}, {n_uni + 1 + i: pairs[j] for i, j in enumerate(pick)})


def tiny_cases(count=40, seed=0):
    """(x (T, 6) f32, phrase, table): T <= 5, V = 6, L <= 4; repeated characters and repeated bigrams in the rotation, every third
    case with logits rounded to halves so that candidates tie; every fifth on the inventory without the unigram b"""
    rs = np.random.RandomState(seed)
    fixed = [(A, A, A, A), (A, Bc, A, Bc), (Bc, A, A, Bc), (A, A), (A, Bc), (Bc,), (A, A, A), (Bc, A, Bc), (A,), (Bc, Bc)]
    for i in range(count):
        T = 1 + (i * 3) % 5
        p = fixed[(i // 2) % len(fixed)] if i % 2 == 0 else tuple(rs.randint(1, 3, size=rs.randint(1, 5)).tolist())
        x = (rs.randn(T, 6) * 2.0).astype(np.float32)
        if i % 3 == 0:
            x = (np.round(x * 2.0) / 2.0).astype(np.float32)
        yield x, p, (NO_B if i % 5 == 4 else SMALL)


def random_strings(K, n_chars, lo, hi, seed):
    rs = np.random.RandomState(seed)
    return [tuple(int(c) for c in rs.randint(1, n_chars + 1, size=rs.randint(lo, hi + 1))) for _ in range(K)]


def planted(T, phrases, gram, seed, blank=0, p_big=0.5):
    """a frame path of length T that spells every phrase once, in order, each with a random mix of unigram and bigram tokens
    (a bigram with probability p_big where the inventory has it, and wherever the unigram is missing), every token held 1-3
    frames, a blank between equal tokens and now and then elsewhere, 2-4 blanks between phrases
    -> (path (T) ints, [(k, start, end)], [the token ids used per phrase]); raises if T is too short"""
    rs = np.random.RandomState(seed)
    uni, big = token_maps(gram)
    path, spans, used = [blank] * int(rs.randint(1, 4)), [], []
    for k, p in enumerate(phrases):
        toks, i = [], 0
        while i < len(p):
            pair = big.get((p[i], p[i + 1])) if i + 1 < len(p) else None
            if pair is not None and (p[i] not in uni or rs.rand() < p_big):
                toks.append(pair)
                i += 2
            else:
                toks.append(uni[p[i]])
                i += 1
        s = len(path)
        for j, v in enumerate(toks):
            if j and toks[j - 1] == v:
                path += [blank] * int(rs.randint(1, 3))
            elif j and rs.rand() < 0.3:
                path += [blank]
            path += [v] * int(rs.randint(1, 4))
        spans.append((k, s, len(path)))
        used.append(toks)
        path += [blank] * int(rs.randint(2, 5))
    if len(path) > T:
        raise ValueError("T = %d is too short for %d frames" % (T, len(path)))
    return np.array(path + [blank] * (T - len(path))), spans, used
