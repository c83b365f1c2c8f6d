"""Float64 restatement of the Gram-CTC beam search fused with a character n-gram language model (asr_gram_ctc_beam_search_lm,
csrc/ctc_beam.hip), in the canonical order of gram_beam_reference.beam_search (a test helper, not collected).  It is the oracle
of tests/test_gram_beam_lm_cpu.py and tests/test_gram_beam_lm_gpu.py.

beam_search_lm is gram_beam_reference.beam_search plus: every string S carries lm(S), a function of the string alone -- lm(()) = 0
and lm(S + c) = lm(S) + step(context(S), c), memoised per string and summed left to right, so a bigram extension adds its two
steps in string order and every route to a string gives the same value; after all merges of a frame its entries are ranked by
total + (alpha * lm + beta * len), len in characters; after the last frame the eos term is added and the beam is sorted again
(stable: ties to the earlier slot).  The three masses stay pure Gram-CTC quantities.

`f32=True` is the twin that tells whether inputs separate the two precisions: every mass, every logaddexp (each addition, exp
and log1p of it), the lm sums and the ranking key are rounded to float32, and the steps come from ctc_beam_lm_reference.step32
over the host image `img` (the device's bits per step).
"""
import numpy as np

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref
from ctc_beam_reference import NEG


def beam_search_lm(x, gram, lm, alpha, beta, beam_width, top_k, blank=0, length=None, min_logp=None, use_eos=True, f32=False,
                   img=None):
    """x (T, V) f32 logits of one utterance, gram (V, 2), lm a ctc_beam_lm_reference.DictLM over the unigram ids -> the final beam
    [(string, score, ctc, lm)] sorted by score descending, score = ctc + alpha * lm + beta * len(string).  With `f32` the steps
    are step32's over `img` (lm.host_image() of the same model)."""
    x = np.asarray(x, np.float32)
    gram = np.asarray(gram)
    lae = lmref.lae32 if f32 else ref.lae
    rnd = lmref._r32 if f32 else float
    T = x.shape[0] if length is None else int(length)
    lp, cands = ref.candidates(x[:T], blank, top_k, min_logp)
    if f32:
        lp = lp.astype(np.float32).astype(np.float64)
        assert img is not None

    def lae3(a, b, c):
        return lae(lae(a, b), c)

    def step(ctx, c):
        return float(lmref.step32(img, ctx, c)) if f32 else lm.step(ctx, c)
    spell = [tuple(int(u) for u in row if u >= 0) if row[0] >= 0 else () for row in gram.tolist()]
    uni = {s[0]: v for v, s in enumerate(spell) if len(s) == 1}
    big = {s: v for v, s in enumerate(spell) if len(s) == 2}
    start = lm.start()
    keep = max(lm.order - 1, 0)
    lm_of = {(): 0.0}

    def context(s):
        return (start + s)[-keep:] if keep else ()

    def lm_value(s):
        """lm(s): the left-to-right sum of the steps of its characters, memoised per string"""
        v = lm_of.get(s)
        if v is None:
            v = lm_of[s] = rnd(lm_value(s[:-1]) + step(context(s[:-1]), s[-1]))
        return v

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
                key = rnd(tot + rnd(rnd(alpha * lm_value(s)) + rnd(beta * len(s))))
                scored.append((-key, pos, s, pb, pu, pg))
        scored.sort()
        beam = [(s, pb, pu, pg) for _, _, s, pb, pu, pg in scored[:beam_width]]
    out = []
    for s, pb, pu, pg in beam:
        ctc, l = lae3(pb, pu, pg), lm_value(s)
        if use_eos and lm.eos is not None:
            l = rnd(l + step(context(s), lm.eos))
        out.append((s, rnd(ctc + rnd(rnd(alpha * l) + rnd(beta * len(s)))), ctc, l))
    out.sort(key=lambda e: -e[1])           # stable: ties keep the earlier slot
    return out


def relabel_marks(ng, old_bos, new_bos):
    """the model dictionary with <s> / </s> moved from the ids old_bos / old_bos + 1 to new_bos / new_bos + 1 (the values do not
    change): a model made over the unigram ids 1 .. U becomes one for a device inventory of V >= U + 1 token ids"""
    move = {old_bos: new_bos, old_bos + 1: new_bos + 1}
    return {tuple(move.get(c, c) for c in k): v for k, v in ng.items()}
