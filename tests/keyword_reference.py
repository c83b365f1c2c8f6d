"""NumPy float64 restatement of the CTC keyword search (csrc/ctc_kws.hip), a brute force over every span and
every path for tiny cases, and the case generators of tests/test_keyword_cpu.py and tests/test_keyword_gpu.py.  Test
infrastructure: nothing in the package imports it.

The restatement runs the recurrence of include/asr_hip.h as written: IEEE float64 max and ONE addition per step on
c(t, v) = (double)x[t][v] - (double)xmax[t], the first maximum in the order stay, from the blank, from the previous token (for the
first token: stay, fresh start), the start frame travelling with the winner.  It is vectorised over keywords and nodes, with one
Python loop over the frames.  The device does the same operations on the same f32 logits, so det (after the cast to f32), every
start and every hit must agree exactly; fill and hit_logp contain a log-sum-exp and are compared within a tolerance.
"""
import itertools

import numpy as np

NEG = -np.inf


def is_dead(p, V, blank):
    return len(p) == 0 or min(p) < 0 or max(p) >= V or blank in p


def detect(x, xl, phrases, blank=0, state=None):
    """x (T, V) f32, xl valid frames, phrases: list of id sequences -> det (K, T) f32, start (K, T) int32, fill (T) f32.
    `state`: None, or the dict a previous call returned as its fourth value (the stream form)."""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    K = len(phrases)
    Lmax = max(1, max(len(p) for p in phrases))
    ids = np.zeros((K, Lmax), np.int64)
    node = np.zeros((K, Lmax), bool)                    # token nodes that exist
    for k, p in enumerate(phrases):
        if not is_dead(p, V, blank):
            ids[k, :len(p)] = p
            node[k, :len(p)] = True
    last = np.array([max(len(p), 1) - 1 for p in phrases])
    live = node[:, 0]
    has_blk = node.copy()
    has_blk[:, 0] = False                               # blk_i exists for i >= 2
    diff = np.ones((K, Lmax), bool)
    diff[:, 1:] = ids[:, 1:] != ids[:, :-1]
    if state is None:
        state = dict(tok=np.full((K, Lmax), NEG), blk=np.full((K, Lmax), NEG), ts=np.full((K, Lmax), -1, np.int64),
                     bs=np.full((K, Lmax), -1, np.int64), base=0)
    tok, blk, ts, bs, base = state["tok"], state["blk"], state["ts"], state["bs"], state["base"]
    det = np.full((K, T), NEG, np.float32)
    start = np.full((K, T), -1, np.int32)
    fill = np.zeros(T, np.float32)
    rows = np.arange(K)
    with np.errstate(invalid="ignore"):
        for t in range(min(xl, T)):
            xmax = x[t].max()                           # f32
            xd = x[t].astype(np.float64) - np.float64(xmax)
            ct = np.where(node, xd[ids], NEG)
            cb = np.where(has_blk, xd[blank], NEG)
            up_v = np.empty_like(tok)
            up_s = np.empty_like(ts)
            up_v[:, 1:], up_s[:, 1:] = tok[:, :-1], ts[:, :-1]
            up_v[:, 0], up_s[:, 0] = 0.0, base + t      # the fresh start
            ub = up_v.copy()
            ub[:, 0] = NEG
            uv = np.where(diff, up_v, NEG)
            m1 = np.maximum(tok, blk)
            s1 = np.where(blk > tok, bs, ts)
            nblk = cb + np.maximum(blk, ub)
            nbs = np.where(ub > blk, up_s, bs)
            ntok = ct + np.maximum(m1, uv)
            nts = np.where(uv > m1, up_s, s1)
            tok, blk, ts, bs = ntok, nblk, nts, nbs
            det[:, t] = np.where(live, tok[rows, last], NEG).astype(np.float32)
            start[:, t] = np.where(live, ts[rows, last], -1)
            lse = np.float64(xmax) + np.log(np.exp(x[t].astype(np.float64) - np.float64(xmax)).sum())
            fill[t] = np.float64(xmax) - lse
    return det, start, fill, dict(tok=tok, blk=blk, ts=ts, bs=bs, base=base + min(xl, T))


def hits(det, start, fill, xl, max_hits=4, min_score=NEG):
    """one (utterance, keyword): det (T) f32, start (T), fill (T) f32 -> hit_start, hit_end, hit_score, hit_logp (max_hits), n"""
    T = det.shape[0]
    xl = min(xl, T)
    hs, he = np.full(max_hits, -1, np.int32), np.full(max_hits, -1, np.int32)
    sc, lp = np.full(max_hits, NEG, np.float32), np.full(max_hits, NEG, np.float32)
    e_all = np.arange(T)
    free = (e_all < xl) & np.isfinite(det) & (det >= np.float32(min_score))
    n = 0
    while n < max_hits and free.any():
        cand = e_all[free]
        # the largest det, then the smaller start, then the larger e
        e = int(cand[np.lexsort((-cand, start[cand], -det[cand].astype(np.float64)))[0]])
        s = int(start[e])
        hs[n], he[n], sc[n] = s, e + 1, det[e]
        lp[n] = np.float32(np.float64(det[e]) + np.cumsum(fill[s:e + 1].astype(np.float64))[-1])
        free &= ~((start <= e) & (e_all >= s))
        n += 1
    return hs, he, sc, lp, n


def search(xs, lengths, phrases, blank=0, max_hits=4, min_score=NEG):
    """xs (T, B, V) -> dict of det, start (B, K, T), fill (B, T), hit_start, hit_end, hit_score, hit_logp (B, K, H), n_hits (B, K)"""
    T, B, V = xs.shape
    K = len(phrases)
    out = dict(det=np.zeros((B, K, T), np.float32), start=np.zeros((B, K, T), np.int32), fill=np.zeros((B, T), np.float32),
               hit_start=np.zeros((B, K, max_hits), np.int32), hit_end=np.zeros((B, K, max_hits), np.int32),
               hit_score=np.zeros((B, K, max_hits), np.float32), hit_logp=np.zeros((B, K, max_hits), np.float32),
               n_hits=np.zeros((B, K), np.int32))
    for b in range(B):
        xl = T if lengths is None else int(lengths[b])
        out["det"][b], out["start"][b], out["fill"][b], _ = detect(xs[:, b], xl, phrases, blank)
        for k in range(K):
            h = hits(out["det"][b, k], out["start"][b, k], out["fill"][b], xl, max_hits, min_score)
            (out["hit_start"][b, k], out["hit_end"][b, k], out["hit_score"][b, k], out["hit_logp"][b, k], out["n_hits"][b, k]) = h
    return out


# ------------------------------------------------------------------------------------------------ brute force
def collapse(seq, blank):
    out, prev = [], None
    for c in seq:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def brute_force(x, phrase, blank=0):
    """x (T, V) f32, tiny -> best (T, T) float64: best[s, e] = the maximum, over every label sequence on frames s..e that starts
    and ends on a token and collapses to `phrase`, of the left-to-right float64 sum of c(t, label); -inf where there is none.
    Shares nothing with the lattice: it enumerates all V^(e - s + 1) sequences and collapses them as CTC does."""
    x = np.asarray(x, np.float32)
    T, V = x.shape
    c = x.astype(np.float64) - x.max(axis=1).astype(np.float64)[:, None]
    best = np.full((T, T), NEG)
    for s in range(T):
        for e in range(s, T):
            for seq in itertools.product(range(V), repeat=e - s + 1):
                if seq[0] == blank or seq[-1] == blank or collapse(seq, blank) != list(phrase):
                    continue
                v = 0.0
                for t, lab in zip(range(s, e + 1), seq):
                    v = v + c[t, lab]
                best[s, e] = max(best[s, e], v)
    return best


def tiny_cases(count=30, seed=0):
    """(x (T, 3) f32, phrase): T <= 5, V = 3, L <= 3; the repeated token "1 1" and its longer kin are in the rotation"""
    rs = np.random.RandomState(seed)
    fixed = [(1, 1), (1, 2), (2,), (1, 1, 2), (2, 1, 2), (1, 1, 1)]
    for i in range(count):
        T = 1 + i % 5
        p = fixed[i % len(fixed)] if i % 2 == 0 else tuple(rs.randint(1, 3, size=rs.randint(1, 4)).tolist())
        yield (rs.randn(T, 3) * 2.0).astype(np.float32), p


# ------------------------------------------------------------------------------------------------ generators
def random_logits(T, B, V, seed, scale=3.0):
    return (np.random.RandomState(seed).randn(T, B, V) * scale).astype(np.float32)


def peaked(path, V, seed=0, peak=12.0):
    """(T, V) f32 logits whose per-frame argmax is `path` by a wide margin"""
    path = np.asarray(path)
    x = (np.random.RandomState(seed).randn(len(path), V) * 0.5).astype(np.float32)
    x[np.arange(len(path)), path] += np.float32(peak)
    return x


def random_phrases(K, V, lo, hi, seed, blank=0):
    rs = np.random.RandomState(seed)
    ids = [v for v in range(V) if v != blank]
    return [tuple(int(ids[j]) for j in rs.randint(0, len(ids), size=rs.randint(lo, hi + 1))) for _ in range(K)]


def planted(T, V, phrases, seed, blank=0):
    """a frame path of length T that spells every phrase once, in order, each token held 1-3 frames, blanks between repeated
    tokens and 2-4 blanks between phrases -> (path (T) ints, [(k, start, end)]); raises if T is too short"""
    rs = np.random.RandomState(seed)
    path, spans = [blank] * int(rs.randint(1, 4)), []
    for k, p in enumerate(phrases):
        s = len(path)
        for i, c in enumerate(p):
            if i and p[i - 1] == c:
                path += [blank] * int(rs.randint(1, 3))
            elif i and rs.rand() < 0.3:
                path += [blank]
            path += [c] * int(rs.randint(1, 4))
        spans.append((k, s, len(path)))
        path += [blank] * int(rs.randint(2, 5))
    if len(path) > T:
        raise ValueError("T = %d is too short for %d frames" % (T, len(path)))
    return np.array(path + [blank] * (T - len(path))), spans
