"""Float64 restatement of the Gram-CTC beam search over spelled strings (asr_gram_ctc_beam_search, csrc/ctc_beam.hip), in the
same canonical order (a test helper, not collected).  It is the oracle of tests/test_gram_beam_cpu.py and
tests/test_gram_beam_gpu.py, and makes their inputs.

`gram` (V, 2) spells every token: (u, -1) a unigram, (u1, u2) a bigram, (-1, -1) the blank or an id that is never emitted.  A
hypothesis is a string s of unigrams with three masses: pb (paths ending in blank), pu (ending in the unigram token of s[-1]) and
pg (ending in the bigram token of s[-2:]).  Per frame t < length: candidates as in ctc_beam_reference.candidates, those that
spell nothing dropped afterwards; stays in beam order (pb' = total + lp[blank], pu' = pu + lp[uni(s[-1])], pg' = pg +
lp[bi(s[-2:])]), then extensions in (parent rank, candidate rank) order: the unigram (a) gives s + a its pu, from pb + pg if s
ends in a and from the total otherwise; the bigram (a, b) gives s + ab its pg, from pb + pu if s ends in ab and from the total
otherwise.  Equal strings merge component by component and keep their first position; entries with total -inf are dropped and
the beam_width best by total stay, exact ties to the earlier position.  String identity here is exact (tuples).
"""
import math

import numpy as np

import ctc_beam_reference as ref
from ctc_beam_reference import NEG, lae


def lae3(a, b, c):
    return lae(lae(a, b), c)


def _f32(v):
    return float(np.float32(v))


def beam_search(x, gram, beam_width, top_k, blank=0, length=None, min_logp=None, f32=False):
    """x (T, V) f32 logits of one utterance -> the final beam [(string tuple, total)] sorted by total descending.  With `f32`
    every stored mass is rounded to float32 (an accumulation like the kernel's, for judging the tolerance of a comparison)."""
    x = np.asarray(x, np.float32)
    gram = np.asarray(gram)
    rnd = _f32 if f32 else float
    T = x.shape[0] if length is None else int(length)
    lp, cands = ref.candidates(x[:T], blank, top_k, min_logp)
    spell = [tuple(int(u) for u in row if u >= 0) if row[0] >= 0 else () for row in gram.tolist()]
    uni = {s[0]: v for v, s in enumerate(spell) if len(s) == 1}
    big = {s: v for v, s in enumerate(spell) if len(s) == 2}
    beam = [((), 0.0, NEG, NEG)]      # (string, pb, pu, pg), best first
    for t in range(T):
        lpt = lp[t].tolist()
        entries = {}                  # string -> [pb, pu, pg]; insertion order is the canonical position
        for s, pb, pu, pg in beam:
            e = entries.setdefault(s, [NEG, NEG, NEG])
            e[0] = lae(e[0], lae3(pb, pu, pg) + lpt[blank])
            if pu > NEG:
                e[1] = lae(e[1], pu + lpt[uni[s[-1]]])
            if pg > NEG:
                e[2] = lae(e[2], pg + lpt[big[s[-2:]]])
        for s, pb, pu, pg in beam:
            tot = lae3(pb, pu, pg)
            for c in cands[t]:
                w = spell[c]
                if not w:
                    continue
                e = entries.setdefault(s + w, [NEG, NEG, NEG])
                if len(w) == 1:
                    base = lae(pb, pg) if s[-1:] == w else tot
                    e[1] = lae(e[1], base + lpt[c])
                else:
                    base = lae(pb, pu) if s[-2:] == w else tot
                    e[2] = lae(e[2], base + lpt[c])
        scored = []
        for pos, (s, (pb, pu, pg)) in enumerate(entries.items()):
            pb, pu, pg = rnd(pb), rnd(pu), rnd(pg)
            tot = rnd(lae3(pb, pu, pg))
            if tot > NEG:
                scored.append((-tot, pos, s, pb, pu, pg))
        scored.sort()
        beam = [(s, pb, pu, pg) for _, _, s, pb, pu, pg in scored[:beam_width]]
    return [(s, lae3(pb, pu, pg)) for s, pb, pu, pg in beam]


def enumerate_strings(x, gram, blank=0):
    """every string with p > 0 and its exact log-probability: all V^T paths of x (T, V) in float64, repeats collapsed, blanks (and
    ids that spell nothing) dropped, the rest spelled.  A path through an id that spells nothing counts for no string."""
    lp = ref.log_softmax64(x)
    T, V = lp.shape
    gram = np.asarray(gram)
    spell = [tuple(int(u) for u in row if u >= 0) if row[0] >= 0 else () for row in gram.tolist()]
    out = {}
    for path in np.ndindex(*([V] * T)):
        if any(c != blank and not spell[c] for c in path):
            continue
        s = float(sum(lp[t, path[t]] for t in range(T)))
        string, prev = (), blank
        for c in path:
            if c != blank and c != prev:
                string += spell[c]
            prev = c
        out[string] = lae(out.get(string, NEG), s)
    return out


def table(rows):
    """blank 0, then the given spellings: [(1,), (2,), (1, 2)] -> (V, 2) int32"""
    g = np.full((len(rows) + 1, 2), -1, np.int32)
    for v, r in enumerate(rows, 1):
        g[v, :len(r)] = r
    return g


# the exhaustive cases of both test files: (T, rows after the blank, seed) and the number of distinct strings with p > 0; blank 0,
# unigrams 1 and 2, V = 1 + len(rows); a beam of 128 with top_k = V - 1 holds every one of them
EXHAUSTIVE = [
    ((4, ((1,), (2,), (1, 2)), 0), 44),
    ((4, ((1,), (2,), (1, 2), (2, 2)), 1), 101),
    ((5, ((1,), (2,), (1, 1)), 2), 88),
    ((3, ((1,), (2,), (1, 2), (2, 1), (1, 1)), 3), 61),
    ((5, ((1,), (1, 1)), 4), 9),
    ((1, ((1,), (2,), (1, 2)), 5), 4),
]


def exhaustive_logits(T, V, seed):
    return (np.random.RandomState(seed).randn(T, V) * 2).astype(np.float32)


def label_bigrams(string, gram):
    """for asr.loss.gram_ctc: label_bigram[i] = the id of (u[i-1], u[i]) if the table has it, else -1; [0] = -1"""
    big = {(int(a), int(b)): v for v, (a, b) in enumerate(np.asarray(gram).tolist()) if a >= 0 and b >= 0}
    return [-1] + [big.get((string[i - 1], string[i]), -1) for i in range(1, len(string))]


def unigram_ids(gram):
    """{unigram: token id}"""
    return {int(a): v for v, (a, b) in enumerate(np.asarray(gram).tolist()) if a >= 0 and b < 0}


# ---------------------------------------------------------------------------------------------------- the pruned-search inputs
T_P, B_P, U_P, G_P, W_P, K_P = 160, 8, 20, 150, 16, 16          # V = 1 + 20 unigrams + 150 bigrams = 171


def uni_bigram_table(U, G, seed):
    """blank 0, unigrams 1..U (token id = unigram id), then G distinct random ordered pairs of them"""
    rs = np.random.RandomState(seed)
    pairs = [(a, b) for a in range(1, U + 1) for b in range(1, U + 1)]
    pick = rs.choice(len(pairs), size=G, replace=False)
    return table([(u,) for u in range(1, U + 1)] + [pairs[i] for i in pick])


def pruned_table(seed=5):
    return uni_bigram_table(U_P, G_P, seed)


def peaky_gram(rs, T, gram, blank=0):
    """ctc_beam_reference.peaky over token ids, plus confusers that make decompositions compete: on a bigram token's frame its
    first unigram there and its second unigram on the next frame come to within 0-2 of the peak; on a unigram token's frame,
    half of the time, a bigram token that starts with it does"""
    gram = np.asarray(gram)
    V = gram.shape[0]
    x = ref.peaky(rs, T, V, blank)
    uni = unigram_ids(gram)
    starts_with = {}
    for v, (a, b) in enumerate(gram.tolist()):
        if a >= 0 and b >= 0:
            starts_with.setdefault(a, []).append(v)
    xb = x.copy()
    xb[:, blank] = -np.inf
    top = xb.argmax(axis=1)
    for t in range(T - 1):
        c = int(top[t])
        if x[t, c] < x[t, blank] or (t > 0 and top[t - 1] == c):
            continue                                    # a blank frame, or the same run going on
        peak = float(x[t, c])
        a, b = gram[c].tolist()
        if b >= 0:
            if a in uni and b in uni:
                x[t, uni[a]] = peak - rs.uniform(0, 2.0)
                x[t + 1, uni[b]] = float(x[t + 1].max()) - rs.uniform(0, 2.0)
        elif a >= 0 and a in starts_with and rs.rand() < 0.5:
            g = starts_with[a]
            x[t, g[rs.randint(len(g))]] = peak - rs.uniform(0, 2.0)
    return x.astype(np.float32)


def pruned_inputs():
    """(gram (171, 2), x (160, 8, 171) f32, lengths (8) in [T/2, T]): the inputs of tests 2, 3, 4 and 7 of the GPU file"""
    gram = pruned_table()
    rs = np.random.RandomState(20261017)
    x = np.stack([peaky_gram(rs, T_P, gram) for _ in range(B_P)], axis=1)
    lengths = np.random.RandomState(1017).randint(T_P // 2, T_P + 1, size=B_P).astype(np.int32)
    return gram, x, lengths


def token_nbest_by_string(hyps, gram):
    """a token-level N-best [(token ids, score)] spelled through the table and summed per string -> {string: score}"""
    spell = [tuple(int(u) for u in row if u >= 0) for row in np.asarray(gram).tolist()]
    out = {}
    for lab, sc in hyps:
        s = tuple(u for c in lab for u in spell[c])
        out[s] = lae(out.get(s, NEG), sc)
    return out


# ---------------------------------------------------------------------------------------------------------- edge-case inputs
def random_table(V, U, seed, blank=0, dead=0, all_bigram=False):
    """U of the non-blank token ids are unigrams (a unigram's id is its token id), `dead` rows spell nothing, the others are
    distinct random pairs of the unigrams.  all_bigram: the U unigrams have no token of their own (every row is a pair)."""
    rs = np.random.RandomState(seed)
    toks = [v for v in range(V) if v != blank]
    unis = sorted(int(v) for v in rs.choice(toks, size=U, replace=False))
    pairs = [(a, b) for a in unis for b in unis]
    order = rs.permutation(len(pairs))
    g = np.full((V, 2), -1, np.int32)
    rest = toks if all_bigram else [v for v in toks if v not in unis]
    if not all_bigram:
        for u in unis:
            g[u] = (u, -1)
    gone = set(int(v) for v in rs.choice(rest, size=dead, replace=False)) if dead else set()
    k = 0
    for v in rest:
        if v in gone:
            continue
        g[v] = pairs[order[k]]
        k += 1
    return g


def bigram_run(T, gram, seed, blank=0):
    """every frame peaks on a bigram token, never the same one twice in a row: the best string has 2 T characters"""
    gram = np.asarray(gram)
    rs = np.random.RandomState(seed)
    x = (rs.randn(T, len(gram)) * 2).astype(np.float32)
    bigs = [v for v, (a, b) in enumerate(gram.tolist()) if b >= 0]
    prev = -1
    for t in range(T):
        c = prev
        while c == prev:
            c = bigs[rs.randint(len(bigs))]
        x[t, c] += 12.0
        prev = c
    return x


def known_strings(B, T, gram, seed, blank=0):
    """B random strings, each cut at random into the table's unigram and bigram tokens and laid out with one or two frames per
    token and blanks between, 20 above the noise -> (x (T, B, V) f32, strings)"""
    gram = np.asarray(gram)
    rs = np.random.RandomState(seed)
    uni = unigram_ids(gram)
    big = {(int(a), int(b)): v for v, (a, b) in enumerate(gram.tolist()) if a >= 0 and b >= 0}
    chars = sorted(uni)
    x = rs.randn(T, B, len(gram)).astype(np.float32)
    strings = []
    for b in range(B):
        s, t = [], 1
        path = np.full(T, blank)
        while t < T - 4:
            a = chars[rs.randint(len(chars))]
            c = chars[rs.randint(len(chars))]
            if (a, c) in big and rs.rand() < 0.5:
                tok, add = big[(a, c)], [a, c]
            else:
                tok, add = uni[a], [a]
            n = rs.randint(1, 3)
            path[t:t + n] = tok
            s += add
            t += n + 1                                   # a blank frame after every token
        x[np.arange(T), b, path] += 20.0
        strings.append(tuple(s))
    return x, strings
