"""Float64 restatement of the CTC prefix beam search of csrc/ctc_beam.hip, in the same canonical order (a test helper, not
collected).  It is the oracle of tests/test_ctc_beam_cpu.py and tests/test_ctc_beam_gpu.py; `peaky` makes their logits.

Per frame t < length: candidates = the top_k non-blank ids by f32 logit (value descending, lower id on equal values; top_k above
V - 1 acts as V - 1), kept where lp >= min_logp; stays of every hypothesis (pb += total + lp[blank], pnb += pnb + lp[last]) in
beam order, then extensions (parent rank, candidate rank): pnb(h + c) += (pb(h) if c == last(h) else total(h)) + lp[c]; equal
prefixes merge by log-sum-exp and keep their first position; entries with total -inf are dropped and the beam_width best by
total stay, exact ties to the earlier position.  Prefix identity here is exact: each (parent prefix, token) pair is interned
once, so an id stands for one whole prefix.
"""
import math

import numpy as np

NEG = -math.inf


def lae(a, b):
    """log(exp(a) + exp(b)) in float64"""
    if a == NEG:
        return b
    if b == NEG:
        return a
    if a >= b:
        return a + math.log1p(math.exp(b - a))
    return b + math.log1p(math.exp(a - b))


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def candidates(x, blank, top_k, min_logp=None):
    """x (T, V) f32 -> (lp (T, V) float64, [candidate ids of frame t in rank order])"""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    lp = log_softmax64(x)
    k = max(0, min(top_k, V - 1))
    order = np.argsort(-x, axis=1, kind="stable")          # value descending; the stable sort keeps lower ids first on ties
    cands = []
    for t in range(T):
        row = order[t]
        row = row[row != blank][:k]
        if min_logp is not None:
            row = row[lp[t, row] >= min_logp]
        cands.append([int(c) for c in row])
    return lp, cands


def beam_search(x, beam_width, top_k, blank=0, length=None, min_logp=None):
    """x (T, V) f32 logits of one utterance -> the final beam [(labels tuple, total)] sorted by total descending"""
    x = np.asarray(x, np.float32)
    T = x.shape[0] if length is None else int(length)
    lp, cands = candidates(x[:T], blank, top_k, min_logp)
    intern = {}                 # (parent id, token) -> prefix id; id 0 is the empty prefix
    parent, last = [-1], [-1]
    beam = [(0, 0.0, NEG)]      # (prefix id, pb, pnb), best first
    for t in range(T):
        lpt = lp[t].tolist()
        lpb = lpt[blank]
        entries = {}            # prefix id -> [pb, pnb]; insertion order is the canonical position
        for h, pb, pnb in beam:
            e = entries.setdefault(h, [NEG, NEG])
            e[0] = lae(e[0], lae(pb, pnb) + lpb)
            if h != 0:
                e[1] = lae(e[1], pnb + lpt[last[h]])
        for h, pb, pnb in beam:
            tot = lae(pb, pnb)
            for c in cands[t]:
                hc = intern.get((h, c))
                if hc is None:
                    hc = intern[(h, c)] = len(parent)
                    parent.append(h)
                    last.append(c)
                base = pb if (h != 0 and last[h] == c) else tot
                e = entries.setdefault(hc, [NEG, NEG])
                e[1] = lae(e[1], base + lpt[c])
        scored = []
        for pos, (h, (pb, pnb)) in enumerate(entries.items()):
            tot = lae(pb, pnb)
            if tot > NEG:
                scored.append((-tot, pos, h, pb, pnb))
        scored.sort()
        beam = [(h, pb, pnb) for _, _, h, pb, pnb in scored[:beam_width]]
    out = []
    for h, pb, pnb in beam:
        labels = []
        while h != 0:
            labels.append(last[h])
            h = parent[h]
        out.append((tuple(labels[::-1]), lae(pb, pnb)))
    return out


def enumerate_paths(x, blank=0):
    """every labelling with p > 0 and its exact log-probability, by summing all V^T paths of x (T, V) in float64"""
    lp = log_softmax64(x)
    T, V = lp.shape
    out = {}
    for path in np.ndindex(*([V] * T)):
        s = float(sum(lp[t, path[t]] for t in range(T)))
        labels, prev = [], blank
        for c in path:
            if c != blank and c != prev:
                labels.append(int(c))
            prev = c
        key = tuple(labels)
        out[key] = lae(out.get(key, NEG), s)
    return out


# the exhaustive cases of both test files: (T, V, beam_width, seed) and the number of labellings with p > 0 (every path of
# length T over V symbols, collapsed); top_k = V - 1
EXHAUSTIVE = [((5, 3, 64, 0), 25), ((4, 4, 128, 1), 61), ((6, 3, 128, 2), 41), ((7, 3, 128, 4), 67), ((1, 3, 4, 3), 3)]


def exhaustive_logits(T, V, seed):
    return (np.random.RandomState(seed).randn(T, V) * 2).astype(np.float32)


def peaky(rs, T, V, blank=0):
    """logits with a peaked best path (a run of 1-3 frames per label, 7-14 above the rest) and confusable frames where a
    second token is close behind: the full-size inputs of tests/test_ctc_beam_gpu.py"""
    x = rs.randn(T, V).astype(np.float32)
    L = rs.randint(T // 12, T // 6)
    labels = rs.randint(1, V, size=L)
    starts = np.sort(rs.choice(np.arange(1, T - 4), size=L, replace=False))
    tgt = np.full(T, blank)
    for k, s in enumerate(starts):
        tgt[s:s + rs.randint(1, 4)] = labels[k]
    boost = rs.uniform(7.0, 14.0, size=T)
    x[np.arange(T), tgt] += boost.astype(np.float32)
    conf = rs.rand(T) < 0.15                      # confusable frames: a second token close behind
    alt = rs.randint(1, V, size=T)
    x[np.arange(T)[conf], alt[conf]] += (boost[conf] - rs.uniform(0, 2.0, size=conf.sum())).astype(np.float32)
    return x
