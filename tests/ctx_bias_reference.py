"""Float64 restatement of the phrase-biasing automaton of asr/bias.py + csrc/ctxgraph.hpp and of the biased beam search
asr_ctc_beam_search_bias (a test helper, not collected).  It is the oracle of tests/test_ctx_bias_cpu.py and
tests/test_ctx_bias_gpu.py, and makes their phrase lists.

occurrences   brute force: the sum of weight * length over every occurrence of every phrase in a string.
DictGraph     the dense automaton as a dictionary over strings, in float64, from the definitions of include/asr_hip.h rather
              than from fail links: the state of a string is its longest suffix that is a prefix of a phrase; out, phi and adv
              are sums over the phrase list.  step(state, c) -> (state', delta).
Image32       the float32 twin over the host image of ContextGraph.host_image(): the table look-up probe by probe and the
              additions in the device's order (hit; miss + root hit: ret[s] + delta0; miss at both: ret[s]).  It must give the
              device's bits.  States are the image's integers.
beam_search_bias  ctc_beam_lm_reference.beam_search_lm plus the bias: every prefix carries bias_open = bias_open(parent) + delta
              and its state, fixed when the prefix is first created; a frame's entries are ranked by
              (total + (alpha * lm + beta * len)) + bias_open, or total + bias_open without a model; after the last frame
              bias = bias_open + ret(state), the eos term is added and the beam is sorted again (stable).  Candidates come from
              ctc_beam_reference.candidates.  `f32=True` rounds every addition to float32 and wants an Image32.
"""
import numpy as np

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref

NEG = ref.NEG


def occurrences(h, phrases, weights):
    h = tuple(int(c) for c in h)
    reward = {tuple(p): w * len(p) for p, w in zip(phrases, weights)}
    lens = sorted(set(len(p) for p in reward))
    s = 0.0
    for i in range(len(h)):                      # every window of every phrase length, looked up in the list
        for n in lens:
            if i + n <= len(h):
                s += reward.get(h[i:i + n], 0.0)
    return s


class DictGraph:
    def __init__(self, phrases, weights):
        self.phrases = [tuple(int(c) for c in p) for p in phrases]
        self.weights = [float(w) for w in weights]
        self.end = dict(zip(self.phrases, self.weights))
        self.edge = {}                           # trie node (a tuple) -> the largest weight of the phrases through it
        for p, w in zip(self.phrases, self.weights):
            for k in range(1, len(p) + 1):
                self.edge[p[:k]] = max(self.edge.get(p[:k], 0.0), w)
        self._step = {}

    @classmethod
    def of(cls, graph):
        """from an asr.bias.ContextGraph"""
        return cls(graph.phrases, graph.weights)

    def start(self):
        return ()

    def phi(self, s):
        return sum(self.edge[s[:k]] for k in range(1, len(s) + 1))

    def adv(self, s):
        for k in range(len(s), 0, -1):
            if s[:k] in self.end:
                return self.phi(s) - self.phi(s[:k])
        return self.phi(s)

    def out(self, s):
        return sum(self.end[s[k:]] * (len(s) - k) for k in range(len(s)) if s[k:] in self.end)

    def ret(self, s):
        return -self.adv(s)

    def step(self, s, c):
        hit = self._step.get((s, c))
        if hit is None:
            t = s + (c,)
            while t and t not in self.edge:
                t = t[1:]
            hit = self._step[(s, c)] = (t, self.out(t) + self.adv(t) - self.adv(s))
        return hit

    def score(self, seq, finalize=True):
        s, total = (), 0.0
        for c in seq:
            s, d = self.step(s, c)
            total += d
        return total + (self.ret(s) if finalize else 0.0)

    def state_of(self, seq):
        s = ()
        for c in seq:
            s = self.step(s, c)[0]
        return s


def probe(img, s, c):
    """look (s, c) up in the host image as the kernels do: from its slot on, until a full-key match, an unused slot or
    max_probe slots -> (next, delta as float32), or None"""
    if not img["slots"]:
        return None
    mask = img["slots"] - 1
    i = lmref.slot_hash((s, c, -1, -1)) & mask
    keys = img["keys"]
    for _ in range(img["max_probe"]):
        if keys[i, 0] == s and keys[i, 1] == c:
            return int(img["vals"][i, 0]), img["vals"][i, 1:2].view(np.float32)[0]
        if keys[i, 0] == -1:
            return None
        i = (i + 1) & mask
    return None


def probes_needed(img, s, c):
    """the number of slots the look-up of (s, c) reads"""
    if not img["slots"]:
        return 0
    mask = img["slots"] - 1
    i = lmref.slot_hash((s, c, -1, -1)) & mask
    for p in range(1, img["max_probe"] + 1):
        if (img["keys"][i, 0] == s and img["keys"][i, 1] == c) or img["keys"][i, 0] == -1:
            return p
        i = (i + 1) & mask
    return img["max_probe"]


class Image32:
    def __init__(self, img):
        self.img = img

    def start(self):
        return 0

    def ret(self, s):
        return self.img["ret"][s]

    def step(self, s, c):
        img = self.img
        hit = probe(img, s, c)
        r = img["ret"][s]
        if hit is not None:
            nx, d = hit
        else:
            hit = probe(img, 0, c)
            if hit is not None:
                nx, d = hit[0], np.float32(r + hit[1])
            else:
                nx, d = 0, r
        if not 0 <= nx < img["n_states"]:
            nx = 0
        return nx, np.float32(d)

    def tokens(self, seq):
        """per-token float32 deltas of one sequence and the final state"""
        s, out = 0, []
        for c in seq:
            s, d = self.step(s, c)
            out.append(d)
        return out, s


# ------------------------------------------------------------------------------------------------ the biased search
def beam_search_bias(x, graph, lm, alpha, beta, beam_width, top_k, blank=0, length=None, min_logp=None, use_eos=True, f32=False):
    """x (T, V) f32 logits of one utterance, graph a DictGraph (or an Image32 with `f32`), lm a DictLM or None -> the final
    beam [(labels, score, ctc, lm, bias)] sorted by score descending"""
    x = np.asarray(x, np.float32)
    T = x.shape[0] if length is None else int(length)
    lp, cands = ref.candidates(x[:T], blank, top_k, min_logp)
    lae = lmref.lae32 if f32 else ref.lae
    rnd = lmref._r32 if f32 else float
    if f32:
        lp = lp.astype(np.float32).astype(np.float64)

    def rank(tot, h):
        if lm is not None:
            tot = rnd(tot + rnd(rnd(alpha * lmv[h]) + rnd(beta * plen[h])))
        return rnd(tot + bo[h])

    intern = {}
    parent, last, plen, lmv, ctxs = [-1], [-1], [0], [0.0], [lm.start() if lm is not None else ()]
    bo, state = [0.0], [graph.start()]
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
                    if lm is not None:
                        lmv.append(rnd(lmv[h] + lm.step(ctxs[h], c)))
                        ctxs.append(lm.context(ctxs[h], c))
                    else:
                        lmv.append(0.0)
                        ctxs.append(())
                    ns, d = graph.step(state[h], c)
                    bo.append(rnd(bo[h] + float(d)))
                    state.append(ns)
                base = pb if (h != 0 and last[h] == c) else tot
                e = entries.setdefault(hc, [NEG, NEG])
                e[1] = lae(e[1], rnd(base + lpt[c]))
        scored = []
        for pos, (h, (pb, pnb)) in enumerate(entries.items()):
            tot = lae(pb, pnb)
            if tot > NEG:
                scored.append((-rank(tot, h), pos, h, pb, pnb))
        scored.sort()
        beam = [(h, pb, pnb) for _, _, h, pb, pnb in scored[:beam_width]]
    out = []
    for h, pb, pnb in beam:
        ctc, l = lae(pb, pnb), lmv[h]
        if lm is not None and use_eos and lm.eos is not None:
            l = rnd(l + lm.step(ctxs[h], lm.eos))
        bias = rnd(bo[h] + float(graph.ret(state[h])))
        sc = ctc
        if lm is not None:
            sc = rnd(ctc + rnd(rnd(alpha * l) + rnd(beta * plen[h])))
        sc = rnd(sc + bias)
        labels = []
        while h != 0:
            labels.append(last[h])
            h = parent[h]
        out.append((tuple(labels[::-1]), sc, ctc, l, bias))
    out.sort(key=lambda e: -e[1])           # stable: ties keep the earlier slot
    return out


# ------------------------------------------------------------------------------------------------ phrase lists
def tricky_phrases(rs, symbols, count, max_len=4):
    """`count` different phrases over `symbols` with the hard cases first: a phrase, its last token alone, a proper prefix of it, a
    proper suffix of it, one that overlaps its end, then random ones; weights from {0.5, 1, 1.5, 2}"""
    symbols = list(symbols)
    a = [int(symbols[i]) for i in rs.randint(0, len(symbols), size=max(3, max_len))]
    seed = [tuple(a), (a[-1],), tuple(a[:-1]), tuple(a[1:]), tuple(a[-2:]) + (int(symbols[rs.randint(len(symbols))]),)]
    phrases = []
    for p in seed:
        if p and p not in phrases:
            phrases.append(p)
    tries = 0
    while len(phrases) < count and tries < 100 * count:
        tries += 1
        p = tuple(int(symbols[i]) for i in rs.randint(0, len(symbols), size=rs.randint(1, max_len + 1)))
        if p not in phrases:
            phrases.append(p)
    phrases = phrases[:count]
    weights = [float(w) for w in rs.choice([0.5, 1.0, 1.5, 2.0], size=len(phrases))]
    return phrases, weights


def random_phrases(rs, V, count, min_len, max_len, have=(), blank=0):
    """`count` random phrases over the non-blank ids that are not in `have`"""
    seen, out = set(have), []
    ids = [i for i in range(V) if i != blank] if V <= 64 else None
    while len(out) < count:
        n = rs.randint(min_len, max_len + 1)
        if ids is not None:
            p = tuple(ids[i] for i in rs.randint(0, len(ids), size=n))
        else:
            p = tuple(int(c) for c in rs.randint(0, V, size=n))
            if blank in p:
                continue
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out
