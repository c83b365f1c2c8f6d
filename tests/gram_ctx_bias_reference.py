"""Float64 restatement of the Gram-CTC beam search with contextual phrase biasing (asr_gram_ctc_beam_search_bias,
csrc/ctc_beam.hip), in the canonical order of gram_beam_reference.beam_search (a test helper, not collected).  It is the oracle of
tests/test_gram_ctx_bias_cpu.py and tests/test_gram_ctx_bias_gpu.py, and makes their inputs.

beam_search_bias is gram_beam_lm_reference.beam_search_lm plus: every string S carries bias_open(S) and state(S), functions of the
string alone -- state(()) the root, bias_open(()) = 0, bias_open(S + c) = bias_open(S) + delta(state(S), c), memoised per string
and summed left to right by walking ctx_bias_reference.DictGraph, so a bigram extension takes its two steps in string order and
every route to a string gives the same value; after all merges of a frame its entries are ranked by
(total + (alpha * lm + beta * len)) + bias_open, or total + bias_open with `lm` None; after the last frame
bias = bias_open + ret(state), the eos term is added and the beam is sorted again (stable: ties to the earlier slot).  The three
masses stay pure Gram-CTC quantities.

`f32=True` is the twin that tells whether inputs separate the two precisions: as in beam_search_lm, and the automaton is a
ctx_bias_reference.Image32 over the host image (the device's bits per step), every addition of a delta rounded to float32.
"""
import numpy as np

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref
import gram_beam_reference as gref
from ctc_beam_reference import NEG


def beam_search_bias(x, gram, graph, lm, alpha, beta, beam_width, top_k, blank=0, length=None, min_logp=None, use_eos=True,
                     f32=False, img=None, memo=None):
    """x (T, V) f32 logits of one utterance, gram (V, 2), graph a ctx_bias_reference.DictGraph (an Image32 with `f32`) over the
    unigram ids, lm a ctc_beam_lm_reference.DictLM over them or None -> the final beam [(string, score, ctc, lm, bias)] sorted by
    score descending.  With `f32` and a model the steps are step32's over `img` (lm.host_image() of the same model).  `memo`: a
    dictionary that receives {string: (bias_open, state)} of every string the search created."""
    x = np.asarray(x, np.float32)
    gram = np.asarray(gram)
    lae = lmref.lae32 if f32 else ref.lae
    rnd = lmref._r32 if f32 else float
    T = x.shape[0] if length is None else int(length)
    lp, cands = ref.candidates(x[:T], blank, top_k, min_logp)
    if f32:
        lp = lp.astype(np.float32).astype(np.float64)
        assert lm is None or img is not None

    def lae3(a, b, c):
        return lae(lae(a, b), c)

    def step(ctx, c):
        return float(lmref.step32(img, ctx, c)) if f32 else lm.step(ctx, c)
    spell = [tuple(int(u) for u in row if u >= 0) if row[0] >= 0 else () for row in gram.tolist()]
    uni = {s[0]: v for v, s in enumerate(spell) if len(s) == 1}
    big = {s: v for v, s in enumerate(spell) if len(s) == 2}
    start = lm.start() if lm is not None else ()
    keep = max(lm.order - 1, 0) if lm is not None else 0
    lm_of = {(): 0.0}
    bias_of = {(): (0.0, graph.start())} if memo is None else memo
    bias_of.setdefault((), (0.0, graph.start()))

    def context(s):
        return (start + s)[-keep:] if keep else ()

    def lm_value(s):
        """lm(s): the left-to-right sum of the steps of its characters, memoised per string; 0 without a model"""
        if lm is None:
            return 0.0
        v = lm_of.get(s)
        if v is None:
            v = lm_of[s] = rnd(lm_value(s[:-1]) + step(context(s[:-1]), s[-1]))
        return v

    def bias_value(s):
        """(bias_open(s), state(s)): the left-to-right sum of the deltas of its characters, memoised per string"""
        v = bias_of.get(s)
        if v is None:
            bo, st = bias_value(s[:-1])
            ns, d = graph.step(st, s[-1])
            v = bias_of[s] = (rnd(bo + float(d)), ns)
        return v

    def rank(tot, s):
        if lm is not None:
            tot = rnd(tot + rnd(rnd(alpha * lm_value(s)) + rnd(beta * len(s))))
        return rnd(tot + bias_value(s)[0])

    beam = [((), 0.0, NEG, NEG)]      # (string, pb, pu, pg), best first
    for t in range(T):
        lpt = lp[t].tolist()
        entries = {}                  # string -> [pb, pu, pg]; insertion order is the canonical position
        for s, pb, pu, pg in beam:
            e = entries.setdefault(s, [NEG, NEG, NEG])
            e[0] = lae(e[0], rnd(lae3(pb, pu, pg) + lpt[blank]))
            if pu > NEG:
                e[1] = lae(e[1], rnd(pu + lpt[uni[s[-1]]]))
            if pg > NEG:
                e[2] = lae(e[2], rnd(pg + lpt[big[s[-2:]]]))
        for s, pb, pu, pg in beam:
            tot = lae3(pb, pu, pg)
            for c in cands[t]:
                w = spell[c]
                if not w:
                    continue
                e = entries.setdefault(s + w, [NEG, NEG, NEG])
                if len(w) == 1:
                    base = lae(pb, pg) if s[-1:] == w else tot
                    e[1] = lae(e[1], rnd(base + lpt[c]))
                else:
                    base = lae(pb, pu) if s[-2:] == w else tot
                    e[2] = lae(e[2], rnd(base + lpt[c]))
        scored = []
        for pos, (s, (pb, pu, pg)) in enumerate(entries.items()):
            pb, pu, pg = rnd(pb), rnd(pu), rnd(pg)
            tot = rnd(lae3(pb, pu, pg))
            if tot > NEG:
                scored.append((-rank(tot, s), pos, s, pb, pu, pg))
        scored.sort()
        beam = [(s, pb, pu, pg) for _, _, s, pb, pu, pg in scored[:beam_width]]
    out = []
    for s, pb, pu, pg in beam:
        ctc, l = lae3(pb, pu, pg), lm_value(s)
        if lm is not None and use_eos and lm.eos is not None:
            l = rnd(l + step(context(s), lm.eos))
        bo, st = bias_value(s)
        bias = rnd(bo + float(graph.ret(st)))
        sc = ctc
        if lm is not None:
            sc = rnd(ctc + rnd(rnd(alpha * l) + rnd(beta * len(s))))
        out.append((s, rnd(sc + bias), ctc, l, bias))
    out.sort(key=lambda e: -e[1])           # stable: ties keep the earlier slot
    return out


def windows(s, n):
    return [tuple(s[i:i + n]) for i in range(len(s) - n + 1)]


# ------------------------------------------------------------------------------------------------ the exhaustive phrase sets
def exhaustive_phrases(rows, seed):
    """phrases over the characters 1 and 2 of gram_beam_reference.EXHAUSTIVE's tables with the cases where the bigram step can go
    wrong, for the first bigram row (a, b) of the table: a phrase that ends on a (the first character of the bigram token), one that
    starts on b (its second), the one-character phrases (a) or (b) inside it, then ctx_bias_reference.tricky_phrases' nested and
    suffix phrases.  Weights are multiples of 0.5, so every float32 sum of deltas is exact."""
    import ctx_bias_reference as cref
    a, b = [r for r in rows if len(r) == 2][0]
    chars = sorted({c for r in rows for c in r})
    other = ([c for c in chars if c != a] + [a])[0]
    first = [(other, a), (b, other), (b,) if seed % 2 else (a,), (a, b, a)]
    rs = np.random.RandomState(300 + seed)
    more, _ = cref.tricky_phrases(rs, chars, 4, 3)
    phrases = []
    for p in first + more:
        if p not in phrases:
            phrases.append(tuple(p))
    weights = [float(w) for w in rs.choice([0.5, 1.0, 1.5, 2.0], size=len(phrases))]
    return phrases, weights


# ------------------------------------------------------------------------------------------------ the pruned-search inputs
T_P, B_P, V_P, W_P, K_P = 160, 8, 300, 16, 8
U_P = 24                                      # unigrams 1 .. 24, then 275 bigram rows: V = 300


def pruned_table(seed=7):
    return gref.uni_bigram_table(U_P, V_P - 1 - U_P, seed)


def pruned_ngrams(plain, seed):
    """a trigram model over the characters 1 .. U_P around the unbiased restatement's top-1 strings, <s> / </s> as the ids V_P and
    V_P + 1 -> the n-gram dictionary for asr.lm.NGramLM.from_ngrams(ng, V_P, V_P, V_P + 1)"""
    import gram_beam_lm_reference as glm
    ng = lmref.random_model(np.random.RandomState(seed), U_P + 1, 3, [p[0][0] for p in plain], n_random=300)
    return glm.relabel_marks(ng, U_P + 1, V_P)


def pruned_inputs(seed):
    """T = 160, B = 8, V = 300 peaky logits over pruned_table(), odd utterances ragged, and about 400 phrases over the unigram ids:
    the 3-character windows of the unbiased restatement's strings ranked 2-6 that its top-1 lacks (weight 1.5), 2-5-character
    spans of the top-1 and random phrases (weights from {0.5, 1, 2}) -> (gram, x, lengths, phrases, weights, the unbiased
    restatement's lists)"""
    import ctx_bias_reference as cref
    gram = pruned_table()
    rs = np.random.RandomState(seed)
    x = np.stack([gref.peaky_gram(rs, T_P, gram) for _ in range(B_P)], axis=1)
    lengths = np.full(B_P, T_P, np.int32)
    lengths[1::2] = rs.randint(T_P // 2, T_P + 1, size=B_P)[1::2]
    plain = [gref.beam_search(x[:, b], gram, W_P, K_P, 0, int(lengths[b])) for b in range(B_P)]
    table = {}
    for b in range(B_P):
        top = plain[b][0][0]
        have = set(windows(top, 3))
        for s, _ in plain[b][1:6]:
            for w in windows(s, 3):
                if w not in have:
                    table.setdefault(w, 1.5)
    for b in range(B_P):
        top = plain[b][0][0]
        for _ in range(8):
            n = int(rs.randint(2, 6))
            i = int(rs.randint(0, max(1, len(top) - n + 1)))
            if len(top[i:i + n]) == n:
                table.setdefault(tuple(top[i:i + n]), float(rs.choice([0.5, 1.0, 2.0])))
    want = max(400, len(table) + 50)
    while len(table) < want:
        p = tuple(int(c) for c in rs.randint(1, U_P + 1, size=rs.randint(2, 5)))
        if p not in table:
            table[p] = float(rs.choice([0.5, 1.0, 2.0]))
    return gram, x, lengths, list(table), list(table.values()), plain
