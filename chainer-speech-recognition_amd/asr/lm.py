"""A back-off n-gram language model over token ids (order 1-4, natural log, ARPA semantics) that lives on the device.

Data preparation only, like ``asr/vocab.py``: this module parses ARPA text, lays the model out as the image that
``include/asr_hip.h`` describes (a dense unigram array and one open-addressing table for the orders 2-4) and uploads it once.
Every probability is looked up and summed inside ``libasr_hip`` (csrc/ngram.hpp: asr_ngram_score, asr_ctc_beam_search_lm);
there is no scoring path on the CPU here (the float64 restatement is tests/ctc_beam_lm_reference.py, test infrastructure).
The reference has no language model; ``asr.error.beam_decode_lm`` is the caller.
"""
import math
import os

import numpy as np
import torch

from . import _ops

MAX_ORDER = 4
LN10 = math.log(10.0)
_SEED = np.uint64(0x9E3779B97F4A7C15)
_MUL = np.uint64(0xBF58476D1CE4E5B9)
_S32 = np.uint64(32)


def hash_keys(keys):
    """keys (M, 4) int32 -> uint64 hash of every row: the function of include/asr_hip.h on vectorised uint64"""
    k = np.ascontiguousarray(keys, np.int32).view(np.uint32).astype(np.uint64)
    h = np.full(k.shape[0], _SEED, np.uint64)
    with np.errstate(over="ignore"):
        for i in range(4):
            h = (h ^ k[:, i]) * _MUL
            h ^= h >> _S32
    return h


def build_table(keys, vals):
    """keys (M, 4) int32 rows (tokens oldest first, -1 padded, all different), vals (M, 2) f32 -> (table keys (S, 4) int32 with
    unused rows -1, table vals (S, 2) f32, S, max_probe): S the power of two with 2 * M <= S, linear probing; max_probe is the
    longest displacement + 1, the bound every kernel probes within.  M = 0 gives no table (S = 0)."""
    keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 4)
    vals = np.ascontiguousarray(vals, np.float32).reshape(-1, 2)
    M = keys.shape[0]
    if M == 0:
        return np.zeros((0, 4), np.int32), np.zeros((0, 2), np.float32), 0, 0
    S = 2
    while S < 2 * M:
        S *= 2
    tk = np.full((S, 4), -1, np.int32)
    tv = np.zeros((S, 2), np.float32)
    used = np.zeros(S, bool)
    slot = (hash_keys(keys) & np.uint64(S - 1)).astype(np.int64)
    pending = np.arange(M)
    probes = 0
    while pending.size:
        probes += 1
        s = slot[pending]
        # one claimant per slot and round (the first in input order); the others, and those that met a used slot, move on
        _, first = np.unique(s, return_index=True)
        win = np.zeros(pending.size, bool)
        win[first] = True
        win &= ~used[s]
        w = pending[win]
        tk[slot[w]] = keys[w]
        tv[slot[w]] = vals[w]
        used[slot[w]] = True
        pending = pending[~win]
        slot[pending] = (slot[pending] + 1) & (S - 1)
    return tk, tv, S, probes


class NGramLM:
    """``ngrams``: {tuple of ids: (logp, backoff)} in natural log, every order from 1 to `order`; `V` is the size of the logits'
    inventory; `bos` / `eos` are ids at or above V (or None).  Use the constructors below."""

    def __init__(self, ngrams, V, order, bos=None, eos=None, unk_logp=-20.0, dropped=0):
        if not 1 <= order <= MAX_ORDER:
            raise ValueError("order must be 1..%d" % MAX_ORDER)
        self.V, self.order, self.bos, self.eos = int(V), int(order), bos, eos
        self.vlm = max([self.V] + [i + 1 for i in (bos, eos) if i is not None])
        self.dropped = dropped                  # n-grams of the source left out (from_arpa: words outside the inventory)
        self.unk_logp = float(unk_logp)
        self.ngrams = {}
        for key, (lp, bo) in ngrams.items():
            key = tuple(int(t) for t in key)
            if not 1 <= len(key) <= order or min(key) < 0 or max(key) >= self.vlm:
                raise ValueError("n-gram %r does not fit order %d over %d ids" % (key, order, self.vlm))
            if not (math.isfinite(lp) and math.isfinite(bo)):
                raise ValueError("n-gram %r: values must be finite" % (key,))
            self.ngrams[key] = (float(lp), float(bo))
        for i in range(self.vlm):               # the unigram level is dense: a back-off chain always ends there
            self.ngrams.setdefault((i,), (self.unk_logp, 0.0))
        self._host = None
        self._images = {}
        self.image = None

    @property
    def bos_id(self):
        return -1 if self.bos is None else int(self.bos)

    @property
    def eos_id(self):
        return -1 if self.eos is None else int(self.eos)

    @classmethod
    def from_ngrams(cls, ngrams, V, bos=None, eos=None, unk_logp=-20.0):
        order = max([len(k) for k in ngrams] + [1])
        return cls(ngrams, V, order, bos, eos, unk_logp)

    @classmethod
    def from_arpa(cls, path_or_text, token_to_id, unk_logp=-20.0, V=None):
        """ARPA text (or the path of a file holding it) -> model.  log10 becomes natural log; words go through `token_to_id`
        (the project's vocab_token_to_id); <s> and </s> get the ids V and V + 1; an n-gram with a word outside the inventory
        is dropped and counted in `.dropped`; an id below V without a unigram gets the <unk> entry's log-probability, or
        `unk_logp` (natural log) when the file has none."""
        text = path_or_text
        if "\\data\\" not in text and os.path.exists(text):
            with open(text, encoding="utf-8") as f:
                text = f.read()
        V = (max(token_to_id.values()) + 1) if V is None else int(V)
        ids = dict(token_to_id)
        ids["<s>"], ids["</s>"] = V, V + 1
        ngrams, dropped, n, order, unk = {}, 0, 0, 1, None
        for line in text.splitlines():
            line = line.strip()
            if not line or line.startswith("ngram ") or line == "\\data\\":
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                n = int(line[1:-len("-grams:")])
                order = max(order, n)
                continue
            if n == 0:
                continue
            f = line.split()
            if len(f) not in (n + 1, n + 2):
                raise ValueError("malformed %d-gram line: %r" % (n, line))
            lp = float(f[0]) * LN10
            bo = float(f[n + 1]) * LN10 if len(f) == n + 2 else 0.0
            words = f[1:n + 1]
            if n == 1 and words[0] == "<unk>":
                unk = lp
                continue
            if any(w not in ids for w in words):
                dropped += 1
                continue
            ngrams[tuple(ids[w] for w in words)] = (lp, bo)
        return cls(ngrams, V, order, V, V + 1, unk_logp if unk is None else unk, dropped)

    def host_image(self):
        """the image of include/asr_hip.h as NumPy arrays: uni (vlm, 2) f32, keys (S, 4) int32, vals (S, 2) f32, slots,
        max_probe, order"""
        if self._host is None:
            uni = np.zeros((self.vlm, 2), np.float32)
            rows, vals = [], []
            for key, v in self.ngrams.items():
                if len(key) == 1:
                    uni[key[0]] = v
                else:
                    rows.append(key + (-1,) * (4 - len(key)))
                    vals.append(v)
            tk, tv, S, probes = build_table(np.array(rows, np.int32).reshape(-1, 4), np.array(vals, np.float32).reshape(-1, 2))
            self._host = dict(uni=uni, keys=tk, vals=tv, slots=S, max_probe=probes, order=self.order)
        return self._host

    def to(self, device):
        """build the image on the host (once) and upload it (once per device); returns self with `.image` on that device"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._images:
            h = self.host_image()
            img = dict(slots=h["slots"], max_probe=h["max_probe"], order=h["order"], uni=torch.from_numpy(h["uni"]).to(device))
            img["keys"] = torch.from_numpy(h["keys"]).to(device) if h["slots"] else None
            img["vals"] = torch.from_numpy(h["vals"]).to(device) if h["slots"] else None
            self._images[device] = img
        self.image = self._images[device]
        return self

    def score(self, ids, lengths=None, use_bos=True, use_eos=True):
        """ids (N, Lmax) int32 on the GPU, lengths (N) int32 or None -> (log P(token | context) of every token (N, Lmax) f32,
        log p_lm of every sequence (N) f32, with the </s> term when the model has an eos and `use_eos`): asr_ngram_score"""
        self.to(ids.device)
        ids = ids.to(torch.int32).contiguous()
        if lengths is not None:
            lengths = lengths.to(ids.device, torch.int32).contiguous()
        return _ops.ngram_score(self.image, ids, lengths, self.bos_id if use_bos else -1, self.eos_id if use_eos else -1)
