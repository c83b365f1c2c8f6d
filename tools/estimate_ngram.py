"""Estimate a back-off n-gram model over token ids and write it as ARPA text: a host tool for asr.lm.NGramLM.from_arpa (there
is no language-model toolkit to lean on).  Interpolated absolute discounting in back-off form, with <s> and </s>:

    P(w | h) = max(c(h w) - D, 0) / c(h) + gamma(h) * P(w | h'),   gamma(h) = D * N1+(h .) / c(h),   h' = h without its oldest token
    P(w)     = max(c(w) - D, 0) / N + gamma() / |W|,               W = the inventory's non-blank ids plus </s>

c are plain counts over the sentences wrapped in <s> ... </s>, c(h) = sum_w c(h w).  An n-gram that was seen is written with the
full interpolated value and its context with log10 gamma(h) as the back-off weight; for an unseen w the back-off product
gamma(h) * P(w | h') is exactly the formula's value, so every distribution sums to one over W.  <s> is written with -99.

usage: python tools/estimate_ngram.py --order 3 --out lm.arpa (--ids FILE | --text FILE) [--vocab-size V] [--discount 0.75]
  --ids FILE   one sentence per line, token ids separated by blanks; the ARPA words are the ids in decimal (read them back with
               token_to_id = {str(i): i}); --vocab-size gives the inventory (default: the largest id + 1)
  --text FILE  one sentence per line, tokenised with the project's unigram vocabulary (asr.vocab); the ARPA words are its tokens
"""
import argparse
import collections
import math
import os
import sys

LN10 = math.log(10.0)


def estimate(sentences, order, V, discount=0.75, blank=0):
    """sentences: iterable of id lists (ids 0 .. V - 1, no blank) -> {ngram tuple: (ln p, ln backoff)} with <s> = V, </s> = V + 1"""
    assert 1 <= order <= 4 and 0.0 < discount < 1.0
    bos, eos = V, V + 1
    counts = [collections.Counter() for _ in range(order + 1)]       # counts[n][ngram]
    for s in sentences:
        seq = [bos] + [int(c) for c in s] + [eos]
        for n in range(1, order + 1):
            for i in range(len(seq) - n + 1):
                g = tuple(seq[i:i + n])
                if n == 1 and g[0] == bos:
                    continue
                counts[n][g] += 1
    words = [i for i in range(V) if i != blank] + [eos]
    ctx_total = [collections.Counter() for _ in range(order + 1)]    # ctx_total[n][h]: c(h) over n-grams h w
    ctx_types = [collections.Counter() for _ in range(order + 1)]
    for n in range(1, order + 1):
        for g, c in counts[n].items():
            ctx_total[n][g[:-1]] += c
            ctx_types[n][g[:-1]] += 1
    N = ctx_total[1][()]
    gamma0 = discount * ctx_types[1][()] / N if N else 1.0
    prob = [None, {}]
    for w in words:
        prob[1][(w,)] = max(counts[1][(w,)] - discount, 0.0) / N + gamma0 / len(words) if N else 1.0 / len(words)

    def p_of(g):                                                     # interpolated P(g[-1] | g[:-1]), seen or not
        n = len(g)
        if n == 1:
            return prob[1][g]
        if g in prob[n]:
            return prob[n][g]
        h = g[:-1]
        if ctx_total[n][h] == 0:
            return p_of(g[1:])
        return discount * ctx_types[n][h] / ctx_total[n][h] * p_of(g[1:])

    for n in range(2, order + 1):
        prob.append({})
        for g, c in counts[n].items():
            h = g[:-1]
            prob[n][g] = max(c - discount, 0.0) / ctx_total[n][h] + discount * ctx_types[n][h] / ctx_total[n][h] * p_of(g[1:])
    model = {}
    for n in range(1, order + 1):
        for g, p in prob[n].items():
            bo = 0.0
            if n < order and ctx_total[n + 1][g]:
                bo = math.log(discount * ctx_types[n + 1][g] / ctx_total[n + 1][g])
            model[g] = (math.log(p), bo)
    if order > 1 and ctx_total[2][(bos,)]:
        model[(bos,)] = (-99.0 * LN10, math.log(discount * ctx_types[2][(bos,)] / ctx_total[2][(bos,)]))
    else:
        model[(bos,)] = (-99.0 * LN10, 0.0)
    return model


def write_arpa(model, order, id_to_word, path):
    """natural log in, log10 out, seven decimals"""
    levels = [sorted(g for g in model if len(g) == n) for n in range(1, order + 1)]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for n, lv in enumerate(levels, 1):
            f.write("ngram %d=%d\n" % (n, len(lv)))
        for n, lv in enumerate(levels, 1):
            f.write("\n\\%d-grams:\n" % n)
            for g in lv:
                lp, bo = model[g]
                line = "%.7f\t%s" % (lp / LN10, " ".join(id_to_word[i] for i in g))
                if n < order and bo != 0.0:
                    line += "\t%.7f" % (bo / LN10)
                f.write(line + "\n")
        f.write("\n\\end\\\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids")
    ap.add_argument("--text")
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--discount", type=float, default=0.75)
    ap.add_argument("--vocab-size", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if bool(a.ids) == bool(a.text):
        ap.error("give one of --ids and --text")
    if a.ids:
        with open(a.ids) as f:
            sents = [[int(t) for t in line.split()] for line in f if line.strip()]
        V = a.vocab_size or max(max(s) for s in sents if s) + 1
        words = {i: str(i) for i in range(V)}
    else:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chainer-speech-recognition_amd"))
        from asr import vocab
        tok, inv = vocab.get_unigram_ids()
        with open(a.text, encoding="utf-8") as f:
            sents = [vocab.convert_sentence_to_unigram_ids(line.strip(), tok) for line in f if line.strip()]
        V = a.vocab_size or max(inv) + 1
        words = dict(inv)
    words[V], words[V + 1] = "<s>", "</s>"
    model = estimate(sents, a.order, V, a.discount)
    write_arpa(model, a.order, words, a.out)
    print("wrote %s: %s" % (a.out, ", ".join("%d %d-grams" % (sum(1 for g in model if len(g) == n), n) for n in range(1, a.order + 1))))


if __name__ == "__main__":
    main()
