"""Contextual phrase biasing for the CTC beam search: an Aho-Corasick automaton over a list of phrases that lives on the device.

Data preparation only, like ``asr/lm.py``: this module builds the automaton with NumPy, lays it out as the sparse
"default-to-root" image that ``include/asr_hip.h`` describes (one open-addressing table of transitions and the array `ret`) and
uploads it once.  Every bonus is looked up and summed inside ``libasr_hip`` (csrc/ctxgraph.hpp: asr_ctx_score,
asr_ctc_beam_search_bias); there is no scoring path on the CPU here (the float64 restatement is tests/ctx_bias_reference.py,
test infrastructure).  The reference has no biasing; ``asr.error.beam_decode_biased`` is the caller, and for a Gram-CTC model
``asr.error.gram_beam_decode_biased``, with the graph over the unigram ids that the spelling table uses.
"""
import math

import numpy as np
import torch

from . import _ops
from .lm import build_table

MAX_TRANSITIONS = 1 << 22          # stored transitions; the table then has at most 2^23 slots (128 MiB of keys and values)


class ContextGraph:
    """``phrases``: token-id sequences of length >= 1 over [0, V) without `blank`, all different; ``weights``: one per-token
    weight per phrase (None: all 1), multiplied by ``boost``; every product must be finite and positive.  A phrase of n tokens
    with weight w adds w * n to the score of a hypothesis for every occurrence in it."""

    def __init__(self, phrases, V, weights=None, boost=1.0, blank=0, dropped=0):
        self.V, self.blank, self.dropped = int(V), int(blank), int(dropped)
        phrases = [tuple(int(c) for c in p) for p in phrases]
        if weights is None:
            weights = [1.0] * len(phrases)
        weights = [float(w) * float(boost) for w in weights]
        if len(weights) != len(phrases):
            raise ValueError("%d weights for %d phrases" % (len(weights), len(phrases)))
        if len(set(phrases)) != len(phrases):
            raise ValueError("a phrase is listed twice")
        for p, w in zip(phrases, weights):
            if not p:
                raise ValueError("an empty phrase")
            if min(p) < 0 or max(p) >= self.V or self.blank in p:
                raise ValueError("phrase %r has an id outside [0, %d) or the blank" % (p, self.V))
            if not (math.isfinite(w) and w > 0.0):
                raise ValueError("phrase %r: the weight %r is not finite and positive" % (p, w))
        self.phrases, self.weights = phrases, weights
        self._compile()
        self._images = {}
        self.image = None

    @classmethod
    def from_text(cls, lines, token_to_id, V=None, weights=None, boost=1.0, blank=0):
        """one phrase per line, its characters mapped through `token_to_id` (the project's vocab_token_to_id); a phrase with a
        character outside the vocabulary is dropped and counted in `.dropped`; empty lines are skipped.  For a Gram-CTC
        inventory (``asr.error.gram_beam_decode_biased``, ``GramBeamStream(graph=...)``) the graph runs over the unigram ids
        that the table spells with: pass the unigram part of the vocabulary, ``from_text(lines, unigram_token_to_id, V=V)``
        with V the size of the logits' inventory, as ``NGramLM.from_arpa`` is used for ``gram_beam_decode_lm``."""
        V = (max(token_to_id.values()) + 1) if V is None else int(V)
        phrases, kept, dropped = [], [], 0
        for i, line in enumerate(lines):
            line = line.strip()
            if not line:
                continue
            if any(ch not in token_to_id for ch in line):
                dropped += 1
                continue
            phrases.append([token_to_id[ch] for ch in line])
            kept.append(i)
        if weights is not None:
            weights = [weights[i] for i in kept]
        return cls(phrases, V, weights, boost, blank, dropped)

    def _compile(self):
        # the trie: node 0 is the root; edge weight = the largest weight of the phrases through the node
        child, parent, edge, end = [{}], [0], [0.0], [0.0]
        for p, w in zip(self.phrases, self.weights):
            s = 0
            for c in p:
                nx = child[s].get(c)
                if nx is None:
                    nx = len(child)
                    child[s][c] = nx
                    child.append({})
                    parent.append(s)
                    edge.append(0.0)
                    end.append(0.0)
                edge[nx] = max(edge[nx], w)
                s = nx
            end[s] = w * len(p)
        n = len(child)
        order = [0]                                  # breadth first: a node's fail target comes before it
        for s in order:
            order.extend(child[s].values())
        phi, base = np.zeros(n), np.zeros(n)         # base: phi of the deepest node on the path at which a phrase ends
        fail, out = np.zeros(n, np.int64), np.zeros(n)
        trans = [None] * n                           # s != 0: {c: goto(s, c)} where it differs from goto(0, c)
        trans[0] = child[0]
        for s in order[1:]:
            p = parent[s]
            phi[s] = phi[p] + edge[s]
            base[s] = phi[s] if end[s] > 0.0 else base[p]
        for s in order:
            for c, nx in child[s].items():
                if s == 0:
                    fail[nx] = 0
                else:
                    f = int(fail[s])
                    fail[nx] = trans[f].get(c, child[0].get(c, 0)) if f else child[0].get(c, 0)
            if s:
                f = int(fail[s])
                out[s] = end[s] + out[f]
                trans[s] = dict(trans[f]) if f else {}
                trans[s].update(child[s])
        adv = phi - base
        count = sum(len(t) for t in trans)
        if count > MAX_TRANSITIONS:
            raise ValueError("the phrase list needs %d stored transitions, above the limit of %d" % (count, MAX_TRANSITIONS))
        keys = np.zeros((count, 2), np.int32)
        nxt = np.zeros(count, np.int32)
        delta = np.zeros(count, np.float64)
        k = 0
        for s in range(n):
            for c, nx in trans[s].items():
                keys[k] = (s, c)
                nxt[k] = nx
                delta[k] = out[nx] + adv[nx] - adv[s]
                k += 1
        self.n_states = n
        self._keys, self._next, self._delta = keys, nxt, delta.astype(np.float32)
        self._ret = (0.0 - adv).astype(np.float32)
        self._host = None

    def host_image(self):
        """the image of include/asr_hip.h as NumPy arrays: keys (S, 2) int32, vals (S, 2) int32 (next, the bits of the f32
        delta), ret (n_states) f32, slots, max_probe, n_states"""
        if self._host is None:
            M = self._keys.shape[0]
            k4 = np.full((M, 4), -1, np.int32)
            k4[:, :2] = self._keys
            idx = np.zeros((M, 2), np.float32)
            idx[:, 0] = np.arange(M)                 # the table builder carries the row number (exact in f32: M <= 2^22)
            tk, tv, S, probes = build_table(k4, idx)
            keys = np.ascontiguousarray(tk[:, :2])
            vals = np.zeros((S, 2), np.int32)
            used = keys[:, 0] >= 0
            row = tv[used, 0].astype(np.int64)
            vals[used, 0] = self._next[row]
            vals[used, 1] = self._delta[row].view(np.int32)
            self._host = dict(keys=keys, vals=vals, ret=self._ret, slots=S, max_probe=probes, n_states=self.n_states)
        return self._host

    def to(self, device):
        """build the image on the host (once) and upload it (once per device); returns self with `.image` on that device"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._images:
            h = self.host_image()
            img = dict(slots=h["slots"], max_probe=h["max_probe"], n_states=h["n_states"], ret=torch.from_numpy(h["ret"]).to(device))
            img["keys"] = torch.from_numpy(h["keys"]).to(device) if h["slots"] else None
            img["vals"] = torch.from_numpy(h["vals"]).to(device) if h["slots"] else None
            self._images[device] = img
        self.image = self._images[device]
        return self

    def score(self, ids, lengths=None, finalize=True):
        """ids (N, Lmax) int32 on the GPU, lengths (N) int32 or None -> (the bonus step of every token (N, Lmax) f32, their sum
        per sequence (N) f32: with `finalize` the bias of the sequence, the sum of weight * length over every occurrence of
        every phrase; without it bias_open, which still holds the advance of an unfinished match): asr_ctx_score"""
        self.to(ids.device)
        ids = ids.to(torch.int32).contiguous()
        if lengths is not None:
            lengths = lengths.to(ids.device, torch.int32).contiguous()
        return _ops.ctx_score(self.image, self.V, ids, lengths, finalize)
