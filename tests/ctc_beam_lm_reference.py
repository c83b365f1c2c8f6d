"""Float64 restatement of the n-gram language model of asr/lm.py + csrc/ngram.hpp and of the fused beam search
asr_ctc_beam_search_lm (a test helper, not collected).  It is the oracle of tests/test_ctc_beam_lm_cpu.py and
tests/test_ctc_beam_lm_gpu.py, and makes their models and inputs.

DictLM        the model as a dictionary: step / score in float64 (ARPA back-off: the longest suffix of the context whose
              extension is in the model gives the log-probability; every longer suffix adds its back-off weight if it is in the
              model, 0 otherwise).
probe, step32 the table look-up over the host-built arrays, probe by probe, and the float32 twin of `step` with the addition
              order of include/asr_hip.h: it must give the device's bits.
beam_search_lm  ctc_beam_reference.beam_search plus: every prefix carries lm(h) = lm(parent) + step(parent, c), fixed when the
              prefix is first created; a frame's entries are ranked by total + alpha * lm + beta * len; after the last frame
              the eos term is added and the beam is sorted again (stable: ties to the earlier slot).  Candidates come from
              ctc_beam_reference.candidates, so the candidate sets are those of the unfused restatement.  `f32=True` rounds
              every addition, exp and log1p to float32: the twin that tells whether inputs separate the two precisions.
"""
import math

import numpy as np

import ctc_beam_reference as ref

NEG = ref.NEG
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the model
class DictLM:
    def __init__(self, ngrams, order, bos=None, eos=None):
        self.ng, self.order, self.bos, self.eos = ngrams, order, bos, eos

    @classmethod
    def of(cls, lm):
        """from an asr.lm.NGramLM (its dictionary holds the dense unigram level too)"""
        return cls(lm.ngrams, lm.order, lm.bos, lm.eos)

    def start(self):
        return () if self.bos is None else (self.bos,)

    def context(self, ctx, c):
        return (tuple(ctx) + (c,))[-(self.order - 1):] if self.order > 1 else ()

    def step(self, ctx, c):
        ctx = tuple(ctx)[-(self.order - 1):] if self.order > 1 else ()
        bo = 0.0
        for k in range(len(ctx), 0, -1):
            hit = self.ng.get(ctx[-k:] + (c,))
            if hit is not None:
                return bo + hit[0]
            ent = self.ng.get(ctx[-k:])
            bo += ent[1] if ent is not None else 0.0
        return bo + self.ng[(c,)][0]

    def score(self, seq, use_bos=True, use_eos=True):
        ctx, s = (self.start() if use_bos else ()), 0.0
        for c in seq:
            s += self.step(ctx, c)
            ctx = self.context(ctx, c)
        if use_eos and self.eos is not None:
            s += self.step(ctx, self.eos)
        return s


def slot_hash(key):
    """the hash of include/asr_hip.h on Python integers; key: four ints, -1 padded"""
    h = 0x9E3779B97F4A7C15
    for k in key:
        h = ((h ^ (int(k) & 0xFFFFFFFF)) * 0xBF58476D1CE4E5B9) & M64
        h ^= h >> 32
    return h


def probe(img, ngram):
    """look `ngram` (2-4 ids, oldest first) up in the host image as the kernels do: from its slot on, until a full-key match, an
    unused slot or max_probe slots -> (logp, backoff) as float32, or None"""
    if not img["slots"]:
        return None
    key = tuple(int(c) for c in ngram) + (-1,) * (4 - len(ngram))
    mask = img["slots"] - 1
    s = slot_hash(key) & mask
    keys = img["keys"]
    for _ in range(img["max_probe"]):
        row = keys[s]
        if row[0] == key[0] and row[1] == key[1] and row[2] == key[2] and row[3] == key[3]:
            return img["vals"][s, 0], img["vals"][s, 1]
        if row[0] == -1:
            return None
        s = (s + 1) & mask
    return None


def step32(img, ctx, c):
    """float32 twin of DictLM.step over the host image, additions in the device's order: 0, + back-offs from the longest context
    down (0 where absent), + the log-probability"""
    order = img["order"]
    ctx = tuple(ctx)[-(order - 1):] if order > 1 else ()
    acc = np.float32(0.0)
    for k in range(len(ctx), 0, -1):
        hit = probe(img, ctx[-k:] + (c,))
        if hit is not None:
            return acc + hit[0]
        if k == 1:
            acc = acc + img["uni"][ctx[-1], 1]
        else:
            ent = probe(img, ctx[-k:])
            acc = acc + (ent[1] if ent is not None else np.float32(0.0))
    return acc + img["uni"][c, 0]


def score32(img, seq, bos=None):
    """per-token float32 steps of one sequence"""
    ctx = () if bos is None else (bos,)
    out = []
    for c in seq:
        out.append(step32(img, ctx, c))
        ctx = (ctx + (c,))[-3:]
    return out


# ------------------------------------------------------------------------------------------------ the fused search
def _r32(v):
    return float(np.float32(v))


def lae32(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return _r32(hi + _r32(math.log1p(_r32(math.exp(_r32(lo - hi))))))


def beam_search_lm(x, lm, alpha, beta, beam_width, top_k, blank=0, length=None, min_logp=None, use_eos=True, f32=False):
    """x (T, V) f32 logits of one utterance, lm a DictLM -> the final beam [(labels, score, ctc, lm)] sorted by score descending,
    score = ctc + alpha * lm + beta * len(labels)"""
    x = np.asarray(x, np.float32)
    T = x.shape[0] if length is None else int(length)
    lp, cands = ref.candidates(x[:T], blank, top_k, min_logp)
    lae = lae32 if f32 else ref.lae
    rnd = _r32 if f32 else float
    if f32:
        lp = lp.astype(np.float32).astype(np.float64)
    intern = {}
    parent, last, plen, lmv, ctxs = [-1], [-1], [0], [0.0], [lm.start()]
    beam = [(0, 0.0, NEG)]
    for t in range(T):
        lpt = lp[t].tolist()
        lpb = lpt[blank]
        entries = {}
        for h, pb, pnb in beam:
            e = entries.setdefault(h, [NEG, NEG])
            e[0] = lae(e[0], rnd(lae(pb, pnb) + lpb))
            if h != 0:
                e[1] = lae(e[1], rnd(pnb + lpt[last[h]]))
        for h, pb, pnb in beam:
            tot = lae(pb, pnb)
            for c in cands[t]:
                hc = intern.get((h, c))
                if hc is None:
                    hc = intern[(h, c)] = len(parent)
                    parent.append(h)
                    last.append(c)
                    plen.append(plen[h] + 1)
                    lmv.append(rnd(lmv[h] + lm.step(ctxs[h], c)))
                    ctxs.append(lm.context(ctxs[h], c))
                base = pb if (h != 0 and last[h] == c) else tot
                e = entries.setdefault(hc, [NEG, NEG])
                e[1] = lae(e[1], rnd(base + lpt[c]))
        scored = []
        for pos, (h, (pb, pnb)) in enumerate(entries.items()):
            tot = lae(pb, pnb)
            if tot > NEG:
                scored.append((-rnd(tot + rnd(rnd(alpha * lmv[h]) + rnd(beta * plen[h]))), pos, h, pb, pnb))
        scored.sort()
        beam = [(h, pb, pnb) for _, _, h, pb, pnb in scored[:beam_width]]
    out = []
    for h, pb, pnb in beam:
        ctc, l = lae(pb, pnb), lmv[h]
        if use_eos and lm.eos is not None:
            l = rnd(l + lm.step(ctxs[h], lm.eos))
        n, labels = plen[h], []
        while h != 0:
            labels.append(last[h])
            h = parent[h]
        out.append((tuple(labels[::-1]), rnd(ctc + rnd(rnd(alpha * l) + rnd(beta * n))), ctc, l))
    out.sort(key=lambda e: -e[1])           # stable: ties keep the earlier slot
    return out


# ------------------------------------------------------------------------------------------------ models and inputs
def random_model(rs, V, order, transcripts=(), n_random=200000, keep=0.7, bos=True):
    """{ngram: (logp, backoff)} over ids 1 .. V - 1 plus <s> = V and </s> = V + 1 (with `bos`): Dirichlet(0.5) unigrams,
    back-offs U(-1.5, 0), log-probabilities U(-6, -0.3); `keep` of the 2 .. order-grams of `transcripts` (wrapped in <s> </s>),
    n_random random bigrams and, per higher order, n_random random extensions of n-grams already present."""
    vlm = V + 2 if bos else V
    p = rs.dirichlet(np.full(vlm, 0.5))
    ng = {}
    for i in range(vlm):
        ng[(i,)] = (float(np.log(max(p[i], 1e-30))), float(rs.uniform(-1.5, 0.0)))
    levels = {n: [] for n in range(2, order + 1)}
    for tr in transcripts:
        seq = ([V] if bos else []) + [int(c) for c in tr] + ([V + 1] if bos else [])
        for n in range(2, order + 1):
            for i in range(len(seq) - n + 1):
                if rs.rand() < keep:
                    levels[n].append(tuple(seq[i:i + n]))
    if order >= 2 and n_random:
        a = rs.randint(1, V, size=(n_random, 2))
        levels[2] += [tuple(r) for r in a.tolist()]
    for n in range(2, order + 1):
        if n > 2 and n_random:
            prev = sorted(set(levels[n - 1]))
            pick = rs.randint(0, len(prev), size=n_random)
            ext = rs.randint(1, V, size=n_random)
            levels[n] += [prev[i] + (int(c),) for i, c in zip(pick.tolist(), ext.tolist())]
        keys = sorted(set(k for k in levels[n] if k[-1] != V and (V + 1) not in k[:-1] and V not in k[1:]))
        lps = rs.uniform(-6.0, -0.3, size=len(keys))
        bos_ = rs.uniform(-1.5, 0.0, size=len(keys))
        for k, a, b in zip(keys, lps.tolist(), bos_.tolist()):
            ng[k] = (a, b if n < order else 0.0)
    return ng


def exhaustive_model(V, seed):
    """the order-3 model (with <s> and </s>) of the exhaustive cases of both test files -> {ngram: (logp, backoff)}"""
    rs = np.random.RandomState(100 + seed)
    return random_model(rs, V, 3, [rs.randint(1, V, size=4).tolist() for _ in range(6)], n_random=40)


def greedy(x, blank=0, length=None):
    """argmax per frame, repeats merged, blanks dropped: x (T, V)"""
    path = np.argmax(x[:length], axis=1)
    out, prev = [], blank
    for c in path.tolist():
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return out


T_FULL, B_FULL, V_FULL = 1000, 16, 3000


def full_inputs(B=B_FULL, T=T_FULL, V=V_FULL, order=3):
    """the full-size inputs of tests/test_ctc_beam_lm_gpu.py (and, with B = 32, of tools/time_ctc_beam_lm.py): peaky logits, odd
    utterances ragged, and the model dictionary built around their greedy transcripts"""
    rs = np.random.RandomState(20261017)
    x = np.stack([ref.peaky(rs, T, V) for _ in range(B)], axis=1)
    cut = np.random.RandomState(1017).randint(T // 2, T + 1, size=B)
    lengths = np.full(B, T, np.int32)
    lengths[1::2] = cut[1::2]
    tr = [greedy(x[:, b], 0, int(lengths[b])) for b in range(B)]
    ng = random_model(np.random.RandomState(20261018), V, order, tr)
    return x, lengths, ng
