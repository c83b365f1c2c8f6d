"""TEST INFRASTRUCTURE -- pure Python / NumPy restatement of csrc/edit_align.hip: the full Levenshtein table, the trace-back by the
pinned rule, the pairwise distance matrix of an N-best list and minimum-Bayes-risk decoding in float64.

The rule, from (i, j) = (n, m) back to (0, 0): i == 0 insertion; j == 0 deletion; r[i-1] == h[j-1] match; d[i][j] == d[i-1][j-1] + 1
substitution; d[i][j] == d[i-1][j] + 1 deletion; otherwise insertion."""
import numpy as np


def table(r, h):
    """the full (n + 1, m + 1) int64 table, row by row with NumPy: d[i][j] = the distance of r[:i] and h[:j]"""
    r, h = np.asarray(r, np.int64), np.asarray(h, np.int64)
    n, m = len(r), len(h)
    d = np.zeros((n + 1, m + 1), np.int64)
    d[0] = np.arange(m + 1)
    cols = np.arange(m + 1)
    for i in range(1, n + 1):
        # without the insertion term: c[j] = min(d[i-1][j-1] + cost, d[i-1][j] + 1); then d[i][j] = min(c[j], d[i][j-1] + 1) is a
        # running minimum of c[j] - j
        c = np.empty(m + 1, np.int64)
        c[0] = i
        c[1:] = np.minimum(d[i - 1, :-1] + (h != r[i - 1]), d[i - 1, 1:] + 1)
        d[i] = np.minimum.accumulate(c - cols) + cols
    return d


def align(r, h):
    """-> (distance, substitutions, deletions, insertions, ref_to_hyp (n), hyp_to_ref (m)) of the pinned path"""
    r, h = [int(v) for v in r], [int(v) for v in h]
    d = table(r, h)
    i, j = len(r), len(h)
    r2h, h2r = [-1] * i, [-1] * j
    S = D = I = 0
    while i > 0 or j > 0:
        if i == 0:
            op = "I"
        elif j == 0:
            op = "D"
        elif r[i - 1] == h[j - 1]:
            assert d[i, j] == d[i - 1, j - 1]
            op = "H"
        elif d[i, j] == d[i - 1, j - 1] + 1:
            op = "S"
        elif d[i, j] == d[i - 1, j] + 1:
            op = "D"
        else:
            assert d[i, j] == d[i, j - 1] + 1
            op = "I"
        if op in "HS":
            i, j = i - 1, j - 1
            r2h[i], h2r[j] = j, i
            S += op == "S"
        elif op == "D":
            i -= 1
            D += 1
        else:
            j -= 1
            I += 1
    return int(d[-1, -1]), S, D, I, r2h, h2r


def carried_counts(r, h):
    """(distance, S, D, I) without a trace-back, the way the kernel gets them: every cell carries the substitutions of the pinned
    path that reaches it, taken over from the predecessor the rule names; D and I follow from n - m = D - I and d = S + D + I"""
    n, m = len(r), len(h)
    d = table(r, h)
    s = np.zeros((n + 1, m + 1), np.int64)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if r[i - 1] == h[j - 1]:
                s[i, j] = s[i - 1, j - 1]
            elif d[i, j] == d[i - 1, j - 1] + 1:
                s[i, j] = s[i - 1, j - 1] + 1
            elif d[i, j] == d[i - 1, j] + 1:
                s[i, j] = s[i - 1, j]
            else:
                s[i, j] = s[i, j - 1]
    dist, S = int(d[n, m]), int(s[n, m])
    D = (dist - S + n - m) // 2
    return dist, S, D, D - (n - m)


def pairwise(ids, lens):
    """ids (B, N, L), lens (B, N) (negative: unused) -> (B, N, N) int64; rows and columns of unused slots and the diagonal are 0"""
    ids, lens = np.asarray(ids), np.asarray(lens)
    B, N = lens.shape
    out = np.zeros((B, N, N), np.int64)
    for b in range(B):
        for i in range(N):
            for j in range(i + 1, N):
                if lens[b, i] >= 0 and lens[b, j] >= 0:
                    out[b, i, j] = out[b, j, i] = table(ids[b, i, :lens[b, i]], ids[b, j, :lens[b, j]])[-1, -1]
    return out


def posterior(scores, scale=1.0):
    """softmax(scale * scores) over the finite scores in float64, 0 elsewhere (an all-unused row is all 0)"""
    s = np.asarray(scores, np.float64)
    used = np.isfinite(s)
    post = np.zeros_like(s)
    for b in range(s.shape[0]):
        if used[b].any():
            z = scale * s[b, used[b]]
            e = np.exp(z - z.max())
            post[b, used[b]] = e / e.sum()
    return post


def confidence(ids, lens, post, b, pivot):
    """conf (L) float64 of utterance b against slot `pivot` (the reference of every alignment); all 0 for pivot < 0"""
    ids, lens = np.asarray(ids), np.asarray(lens)
    conf = np.zeros(ids.shape[2], np.float64)
    if pivot < 0 or lens[b, pivot] < 0:
        return conf
    r = ids[b, pivot, :lens[b, pivot]]
    for j in range(lens.shape[1]):
        if lens[b, j] < 0:
            continue
        h = ids[b, j, :lens[b, j]]
        r2h = align(r, h)[4]
        for l, k in enumerate(r2h):
            if k >= 0 and h[k] == r[l]:
                conf[l] += post[b, j]
    return conf


def mbr(ids, lengths, scores, scale=1.0):
    """-> dict(index (B), risk (B, N), posterior (B, N), dist (B, N, N), lens (B, N) with -1 for unused slots, conf (B, L) for the
    argmin pivot); a slot is used iff its score is finite; ties in the risk go to the lowest index"""
    ids, lengths = np.asarray(ids), np.asarray(lengths)
    s = np.asarray(scores, np.float64)
    used = np.isfinite(s)
    B, N, L = ids.shape
    lens = np.where(used, np.clip(lengths, 0, L), -1)
    dist = pairwise(ids, lens)
    post = posterior(s, scale)
    risk = np.where(used, (post[:, None, :] * dist).sum(axis=2), np.inf)
    index = np.where(used.any(axis=1), risk.argmin(axis=1), -1)
    conf = np.stack([confidence(ids, lens, post, b, int(index[b])) for b in range(B)])
    return dict(index=index, risk=risk, posterior=post, dist=dist, lens=lens, conf=conf)


def brute_force_mbr(hyps, scores, scale=1.0):
    """one utterance as Python lists (None: an unused slot) -> (index, risks): the definition, with oracle-free plain loops"""
    used = [k for k, h in enumerate(hyps) if h is not None]
    if not used:
        return -1, []
    top = max(scale * scores[k] for k in used)
    w = {k: np.exp(scale * scores[k] - top) for k in used}
    z = sum(w.values())
    risks = {i: sum(w[j] / z * _plain_levenshtein(hyps[i], hyps[j]) for j in used) for i in used}
    best = min(used, key=lambda i: (risks[i], i))
    return best, risks


def _plain_levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[-1]


def pack(rows, width=None, fill=0):
    """lists of ids -> ((len(rows), width) int32 padded with `fill`, lengths int32)"""
    width = max(1, max([len(r) for r in rows] + [0])) if width is None else width
    out = np.full((len(rows), width), fill, np.int32)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out, np.asarray([len(r) for r in rows], np.int32)


# hand-made lists shared by the CPU and the GPU test: (name, hypotheses (None: unused slot), scores (-inf: unused), expected index).
# Every gap between the least and the second least risk is decisive (> 0.05).
NEG = float("-inf")
HAND_LISTS = [
    # two near-identical runners-up (0.35 + 0.25) outweigh the top (0.4): risks 1.2, 1.05, 1.15 -- slot 0 is not the pivot
    ("runners_up", [[1, 2, 3, 4], [1, 5, 3, 6], [1, 5, 3, 7]], [np.log(0.4), np.log(0.35), np.log(0.25)], 1),
    ("empty_hypothesis", [[], [1], [1, 2]], [np.log(0.45), np.log(0.3), np.log(0.25)], 1),
    ("empty_wins", [[], [1, 2, 3], [4, 5, 6]], [np.log(0.6), np.log(0.2), np.log(0.2)], 0),
    ("unused_slot", [[1, 2, 3], None, [1, 2, 4], [1, 2, 4, 5]], [np.log(0.2), NEG, np.log(0.5), np.log(0.3)], 2),
    ("all_unused", [None, None, None], [NEG, NEG, NEG], -1),
    ("single", [[3, 3, 3]], [-7.5], 0),
]


def hand_batch():
    """HAND_LISTS as one padded batch: ids (B, N, L) int32, lengths (B, N) int32, scores (B, N) f64, expected index (B).  Unused
    slots hold junk ids and a positive length: only the score says that they are unused"""
    N = max(len(h) for _, h, _, _ in HAND_LISTS)
    L = max(len(x) for _, h, _, _ in HAND_LISTS for x in h if x is not None) + 2
    B = len(HAND_LISTS)
    ids = np.full((B, N, L), 9, np.int32)
    lens = np.full((B, N), 2, np.int32)
    scores = np.full((B, N), NEG, np.float64)
    for b, (_, hyps, sc, _) in enumerate(HAND_LISTS):
        for k, h in enumerate(hyps):
            if h is not None:
                ids[b, k, :len(h)] = h
                lens[b, k] = len(h)
            scores[b, k] = sc[k]
    return ids, lens, scores, np.asarray([w for _, _, _, w in HAND_LISTS])
