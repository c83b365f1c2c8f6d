"""CTC and Gram-CTC keyword spotting: does an utterance contain a phrase, on which frames, and how sure is the model.

Data preparation and plumbing only, like ``asr/bias.py``: this module lays a phrase list out as the keyword image that
``include/asr_hip.h`` describes (NumPy on the host, no arithmetic) and uploads it once.  The search itself -- a free-boundary
Viterbi sweep over every phrase's own lattice and the non-maximum suppression of its hits -- runs inside ``libasr_hip``
(csrc/ctc_kws.hip: asr_kws_detect, asr_gram_kws_detect, asr_kws_hits); there is no path on the CPU here (the float64
restatements are tests/keyword_reference.py and tests/gram_keyword_reference.py, test infrastructure).  The reference has no
keyword search.

    kws = KeywordSet([[5, 9, 2], [7, 7]], V)                         # CTC: a phrase is a sequence of token ids
    hits = keyword_search(logits, kws, lengths, max_hits=4)          # logits (T, B, V) f32 on the device
    hits.start[b, k, :hits.count[b, k]], hits.end[...]               # the frames [start, end) of every occurrence, best first

    kws = GramKeywordSet([[5, 9, 2], [7, 7]], gram)                  # Gram-CTC: a phrase is a string of characters (unigram ids);
    hits = keyword_search(logits, kws, lengths, max_hits=4)          # every cut into unigram and bigram tokens is searched at once
"""
import collections

import numpy as np
import torch

from . import _ops

MAX_LEN = 64            # tokens of one phrase: one wave owns a lattice, one token and its blank per lane
SWEEP_GROUP = 4         # keywords per workgroup of the sweep          (csrc/ctc_kws.hip: kGroup)
SWEEP_TILE = 32         # frames per register tile of the sweep        (csrc/ctc_kws.hip: kTile)
GRAM_SWEEP_TILE = 32    # frames per register tile of the Gram sweep   (csrc/ctc_kws.hip: kGramTile)

Detection = collections.namedtuple("Detection", "score start fill")
Hits = collections.namedtuple("Hits", "start end score logp count")


class KeywordSet:
    """``phrases``: token-id sequences over [0, V) without `blank`.  A phrase that is empty or has an id outside [0, V) or the
    blank is kept as a dead keyword (it never hits), so the rows of the outputs stay those of the list; the same phrase may be
    listed twice.  A phrase of more than 64 tokens raises ValueError."""

    def __init__(self, phrases, V, blank=0):
        self.V, self.blank = int(V), int(blank)
        self.phrases = [tuple(int(c) for c in p) for p in phrases]
        if not self.phrases:
            raise ValueError("an empty phrase list")
        if not 0 <= self.blank < self.V:
            raise ValueError("blank %d outside [0, %d)" % (self.blank, self.V))
        for p in self.phrases:
            if len(p) > MAX_LEN:
                raise ValueError("a phrase of %d tokens: the limit is %d" % (len(p), MAX_LEN))
        self.dead = [not p or min(p) < 0 or max(p) >= self.V or self.blank in p for p in self.phrases]
        self.K = len(self.phrases)
        self.Lmax = max(1, max(len(p) for p in self.phrases))
        self._host = None
        self._images = {}
        self.image = None

    def host_image(self):
        """the image of include/asr_hip.h as NumPy int32 arrays: uniq (U), node_tok (K, Lmax), kw_len (K)"""
        if self._host is None:
            live = [p for p, d in zip(self.phrases, self.dead) if not d]
            uniq = sorted(set(c for p in live for c in p)) or [self.blank]      # never empty: a list without a live phrase
            slot = {c: i for i, c in enumerate(uniq)}
            node_tok = np.full((self.K, self.Lmax), -1, np.int32)
            kw_len = np.zeros(self.K, np.int32)
            for k, (p, d) in enumerate(zip(self.phrases, self.dead)):
                kw_len[k] = len(p)
                if not d:
                    node_tok[k, :len(p)] = [slot[c] for c in p]
            self._host = dict(uniq=np.asarray(uniq, np.int32), node_tok=node_tok, kw_len=kw_len)
        return self._host

    @property
    def U(self):
        return int(self.host_image()["uniq"].shape[0])

    def to(self, device):
        """build the image on the host (once) and upload it (once per device); returns self with `.image` on that device"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._images:
            self._images[device] = {k: torch.from_numpy(v).to(device) for k, v in self.host_image().items()}
        self.image = self._images[device]
        return self


class GramKeywordSet:
    """``phrases``: strings of characters, each a unigram id as in the rows of `gram` and in the ids ``gram_beam_decode``
    returns; `gram` is the (V, 2) table of ``asr.vocab.gram_table``.  One lattice per phrase holds every way of cutting it into
    unigram and bigram tokens of the inventory.  A phrase that is empty or has a character outside [0, V) or the blank is kept
    as a dead row; a character without a unigram token is not dead -- its unigram node is absent and a bigram may still cover
    it (a phrase with no spelling at all simply never hits).  A phrase of more than 64 characters raises ValueError."""

    def __init__(self, phrases, gram, blank=0, dropped=0):
        from .error import check_gram_table
        self.gram = np.ascontiguousarray(np.asarray(gram))
        self.V, self.blank = int(self.gram.shape[0]), int(blank)
        check_gram_table(self.gram, self.V, self.blank)
        self.phrases = [tuple(int(c) for c in p) for p in phrases]
        if not self.phrases:
            raise ValueError("an empty phrase list")
        for p in self.phrases:
            if len(p) > MAX_LEN:
                raise ValueError("a phrase of %d characters: the limit is %d" % (len(p), MAX_LEN))
        self.dead = [not p or min(p) < 0 or max(p) >= self.V or self.blank in p for p in self.phrases]
        self.K = len(self.phrases)
        self.Lmax = max(1, max(len(p) for p in self.phrases))
        self.dropped = int(dropped)
        self._host = None
        self._images = {}
        self.image = None

    @classmethod
    def from_text(cls, lines, vocab_token_to_id, blank=0):
        """one phrase per line, cut into characters by the project's tokeniser (``convert_sentence_to_unigram_ids``); the table is
        ``asr.vocab.gram_table(vocab_token_to_id)``.  A phrase with a character outside the inventory is dropped and counted in
        `.dropped`; empty lines are skipped"""
        from .vocab import convert_sentence_to_unigram_ids, gram_table
        phrases, dropped = [], 0
        for line in lines:
            line = line.strip()
            if not line:
                continue
            try:
                phrases.append(convert_sentence_to_unigram_ids(line, vocab_token_to_id))
            except AssertionError:
                dropped += 1
        return cls(phrases, gram_table(vocab_token_to_id, blank), blank, dropped)

    def host_image(self):
        """the image of include/asr_hip.h as NumPy int32 arrays: uniq (U), node_uni, node_big (K, Lmax), kw_len (K)"""
        if self._host is None:
            g = self.gram
            uni = {int(a): v for v, (a, b) in enumerate(g) if a >= 0 and b < 0}          # character -> its unigram token
            big = {(int(a), int(b)): v for v, (a, b) in enumerate(g) if a >= 0 and b >= 0}
            toks = []                                   # per phrase: (u_i or None), (g_i or None)
            for p, d in zip(self.phrases, self.dead):
                toks.append(None if d else ([uni.get(c) for c in p], [None] + [big.get(cc) for cc in zip(p, p[1:])]))
            uniq = sorted(set(v for t in toks if t for row in t for v in row if v is not None)) or [self.blank]
            slot = {v: i for i, v in enumerate(uniq)}
            node_uni = np.full((self.K, self.Lmax), -1, np.int32)
            node_big = np.full((self.K, self.Lmax), -1, np.int32)
            kw_len = np.zeros(self.K, np.int32)
            for k, (p, t) in enumerate(zip(self.phrases, toks)):
                kw_len[k] = len(p)
                if t:
                    node_uni[k, :len(p)] = [slot.get(v, -1) for v in t[0]]
                    node_big[k, :len(p)] = [slot.get(v, -1) for v in t[1]]
            self._host = dict(uniq=np.asarray(uniq, np.int32), node_uni=node_uni, node_big=node_big, kw_len=kw_len)
        return self._host

    U = KeywordSet.U
    to = KeywordSet.to


def _backend(keywords):
    """(detect, state, state_reset) of the set's kind"""
    if isinstance(keywords, GramKeywordSet):
        return _ops.gram_kws_detect, _ops.gram_kws_state, _ops.gram_kws_state_reset
    return _ops.kws_detect, _ops.kws_state, _ops.kws_state_reset


def _lengths(lengths, B, device):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths).to(device, torch.int32).contiguous()
    if tuple(lengths.shape) != (B,):
        raise ValueError("lengths must have one entry per utterance (%d)" % B)
    return lengths


def _check_logits(logits, keywords, B=None):
    if logits.dim() != 3 or logits.shape[2] != keywords.V or (B is not None and logits.shape[1] != B):
        raise ValueError("logits must be (T, %s, %d), got %s" % ("B" if B is None else B, keywords.V, tuple(logits.shape)))
    if logits.shape[0] == 0 or logits.shape[1] == 0:
        raise ValueError("empty logits")
    return logits.to(torch.float32).contiguous()


def keyword_detect(logits, keywords, lengths=None):
    """(T, B, V) f32 logits on the device -> Detection(score (B, K, T) f32, start (B, K, T) int32, fill (B, T) f32):
    score[b, k, e] is the best, over all start frames s and all CTC paths of keyword k on frames s..e that begin and end on a
    token, of log p(path) - log p(greedy path on s..e): at most 0, exactly 0.0 where the greedy path spells the keyword, -inf
    where there is no path and for e >= lengths[b]; start is that s (-1 where score is -inf); fill[b, t] is the greedy path's
    log-probability of frame t.  `keywords`: a ``KeywordSet``, or a ``GramKeywordSet`` -- then the best is also taken over every
    decomposition of the phrase into unigram and bigram tokens, and 0.0 means the greedy path spells it with any mix of them."""
    logits = _check_logits(logits, keywords)
    keywords.to(logits.device)
    detect = _backend(keywords)[0]
    return Detection(*detect(logits, _lengths(lengths, logits.shape[1], logits.device), keywords.blank, keywords.image))


def keyword_hits(detection, lengths=None, max_hits=4, min_score=None):
    """non-maximum suppression of a Detection -> Hits(start, end (B, K, max_hits) int32: the frames [start, end), score, logp
    (B, K, max_hits) f32, count (B, K) int32), best first: of the frames whose score is at least `min_score` (None: any finite
    score) the best one is taken (ties: the earlier start, then the later end), every frame whose span meets its span is
    dropped, and so on `max_hits` times.  logp is the log-probability of the best path of the occurrence.  Unused slots hold
    -1 / -1 / -inf / -inf."""
    if max_hits <= 0:
        raise ValueError("max_hits must be positive")
    det, start, fill = (t.contiguous() for t in detection)
    return Hits(*_ops.kws_hits(det, start, fill, _lengths(lengths, det.shape[0], det.device), max_hits,
                               float("-inf") if min_score is None else min_score))


def keyword_search(logits, keywords, lengths=None, max_hits=4, min_score=None):
    """``keyword_detect`` then ``keyword_hits``"""
    return keyword_hits(keyword_detect(logits, keywords, lengths), lengths, max_hits, min_score)


class KeywordStream:
    """``keyword_detect`` fed chunk by chunk, beside ``asr.error.BeamStream``: the lattices of `B` utterances by K keywords live
    on the device between the calls (12 bytes per lattice node: 24 per token of a ``KeywordSet``, 36 per character of a
    ``GramKeywordSet``).  However the frames are cut, each utterance's outputs, taken
    over its valid frames in order, are bit for bit the one-shot ``keyword_detect`` of the frames fed so far; start frames count the utterance's
    own frames since its last reset.  With full-length chunks the Detections concatenated along T go straight into
    ``keyword_hits``.  ``reset()`` starts all utterances over, ``reset(mask)`` only those with mask[b] != 0.  Nothing here
    synchronises with the host."""

    def __init__(self, B, V, keywords, device=None):
        if B <= 0 or V != keywords.V:
            raise ValueError("B must be positive and V (%d) the keyword set's (%d)" % (V, keywords.V))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.B, self.V, self.keywords = int(B), int(V), keywords.to(self.device)
        self._detect, state, self._reset = _backend(keywords)
        self.state = state(self.B, keywords.K, keywords.Lmax, self.device)

    def reset(self, mask=None):
        """start every utterance over, or those with mask[b] != 0 (`mask`: (B) integers, host or device)"""
        if mask is not None:
            mask = torch.as_tensor(mask).to(self.device, torch.int32).contiguous()
            if tuple(mask.shape) != (self.B,):
                raise ValueError("mask must have one entry per utterance (%d)" % self.B)
        self._reset(self.state, self.B, self.keywords.K, self.keywords.Lmax, mask)

    def advance(self, chunk, lengths=None):
        """consume a chunk (Tc, B, V) of f32 logits -> its Detection (B, K, Tc); `lengths` (B): the valid frames of this chunk
        per utterance (0: the utterance is left as it is; frames past the length are never read), None: all Tc"""
        chunk = _check_logits(chunk, self.keywords, self.B).to(self.device)
        self.keywords.to(self.device)
        return Detection(*self._detect(chunk, _lengths(lengths, self.B, self.device), self.keywords.blank, self.keywords.image,
                                       self.state))
