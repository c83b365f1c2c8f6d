"""Greedy-decode error rates with the reference's function names (asr/error.py:7-68), and the beam decoder.

``compute_minibatch_error`` keeps the reference's signature.  Given device tensors it runs the blank / repeat collapse and
the Levenshtein distances of the whole minibatch on the GPU (``libasr_hip``: asr_ctc_collapse, asr_edit_distance) and brings
back only one distance and two lengths per utterance; given host arrays it moves them to the GPU first.  There is no CPU
implementation of the batch path here (the CPU restatement lives in ``oracle/text.py``, test infrastructure).
"""
import collections

import numpy as np
import torch

from . import _ops
from .vocab import convert_sentence_to_unigram_ids


def compute_character_error_rate(r, h):
    """Levenshtein(r, h) / len(r) for one pair of id sequences; len(h) when r is empty (asr/error.py:7-24).
    Goes through the same device kernel as the batch path.  (The reference keeps its table in uint8, i.e. it is defined
    for sequences of up to 255 tokens; this one is exact beyond.)"""
    if len(r) == 0:
        return len(h)
    dev = torch.device("cuda", torch.cuda.current_device())
    rr = torch.tensor([list(r)], dtype=torch.int32, device=dev)
    hh = torch.tensor([list(h) if len(h) else [0]], dtype=torch.int32, device=dev)
    d = _ops.edit_distance(rr, torch.tensor([len(r)], dtype=torch.int32, device=dev), hh,
                           torch.tensor([len(h)], dtype=torch.int32, device=dev))
    return float(d.item()) / len(r)


def greedy_decode(logits, blank=0, lengths=None):
    """(T, B, V) f32 logits on the GPU -> (ids (B, T) int32 padded with blank, lengths (B) int32): argmax per frame,
    repeats merged, blanks dropped (run/ctc/cnn/dev.py:106 + asr/error.py:38-47).  `lengths` (frames per utterance)
    restricts the decode to the valid frames; the reference decodes all T frames (lengths=None)."""
    ids = _ops.argmax_rows(logits.contiguous())
    return _ops.ctc_collapse(ids, lengths, blank, True)


def _needs_retokenisation(vocab_id_to_token, vocab_token_to_id):
    """The reference turns the predicted ids into a sentence and tokenises it again (asr/error.py:49-53): an identity
    unless some token of the inventory is spelled by several unigrams (bigram entries of the Gram-CTC inventory)."""
    if vocab_id_to_token is None or vocab_token_to_id is None:
        return False
    for tid, tok in vocab_id_to_token.items():
        if tid == 0 or tok == "_":
            continue
        if convert_sentence_to_unigram_ids(tok, vocab_token_to_id) != [tid]:
            return True
    return False


def _prepared(logits, blank, lengths, gram=None, lm=None, lm_weight=0.0, length_bonus=0.0, use_eos=True, graph=None):
    """What the six decode functions do before their search, in the order their errors are raised: `graph` must have been built
    for the logits' V and blank; `gram` is validated (``_gram_table``) and, in the Gram-CTC searches, ``lm.vlm`` against V;
    `lengths`, `graph` and `lm` go to the logits' device.  -> (contiguous logits, lengths, the gram table or None, the model's
    arguments (image, alpha, beta, bos, eos) with `eos` from `use_eos` (no model: None, 0, 0, -1, -1), the graph's image or None)"""
    V, dev = logits.shape[2], logits.device
    if graph is not None and (graph.V != V or graph.blank != blank):
        raise ValueError("the context graph was built for %d ids with blank %d, the logits have %d with blank %d"
                         % (graph.V, graph.blank, V, blank))
    table = None if gram is None else _gram_table(gram, V, blank, dev)
    if gram is not None and lm is not None and lm.vlm < V:
        raise ValueError("the language model covers %d ids, fewer than the %d of the logits" % (lm.vlm, V))
    if lengths is not None:
        lengths = lengths.to(dev, torch.int32).contiguous()
    image = None if graph is None else graph.to(dev).image
    model = (None, 0.0, 0.0, -1, -1)
    if lm is not None:
        lm = lm.to(dev)
        model = (lm.image, lm_weight, length_bonus, lm.bos_id, lm.eos_id if use_eos else -1)
    return logits.contiguous(), lengths, table, model, image


def beam_decode(logits, beam_width=16, top_k=16, blank=0, lengths=None, min_logp=None):
    """(T, B, V) f32 logits on the GPU -> (ids (B, beam_width, T) int32 padded with blank, lengths (B, beam_width) int32,
    scores (B, beam_width) f32): the N-best labellings of a CTC prefix beam search, best first, each with its log-probability
    log p(labelling | x) as far as the beam kept its paths (a lower bound on it).  Unused slots: length 0, score -inf.
    Per frame the candidates are the `top_k` non-blank ids with the largest logits, restricted to those whose log-softmax is
    at least `min_logp` (None: no threshold).  `lengths` (B) int32 restricts the decode to the valid frames, as in
    ``greedy_decode``.  The search runs over token ids: with the Gram-CTC inventory two token sequences that spell the same
    string (a bigram token and its two unigrams) stay two hypotheses here; ``gram_beam_decode`` is the search that merges them.
    The reference has no beam decoder; this extends its greedy call sites (run/ctc/cnn/dev.py:102, run/ctc/cnn/test.py:102)."""
    x, lengths, _, _, _ = _prepared(logits, blank, lengths)
    return _ops.ctc_beam_search(x, lengths, blank, beam_width, top_k, min_logp)


def beam_decode_lm(logits, lm, lm_weight, length_bonus, beam_width=16, top_k=16, blank=0, lengths=None, min_logp=None,
                   use_eos=True):
    """``beam_decode`` with an n-gram language model in the ranking while the beam is open: hypotheses are kept and sorted by
    log p_ctc(h | x) + lm_weight * log p_lm(h) + length_bonus * |h|.  `lm` is an ``asr.lm.NGramLM`` (moved to the logits' device
    on first use); its `bos` starts every context and, with `use_eos`, its `eos` closes every hypothesis after the last frame.
    -> (ids, lengths, scores (the combined score), ctc_scores, lm_scores), the last three (B, beam_width) f32, so that a caller
    can re-weight the N-best without decoding again.  Unused slots: length 0, scores and ctc_scores -inf, lm_scores 0."""
    x, lengths, _, model, _ = _prepared(logits, blank, lengths, None, lm, lm_weight, length_bonus, use_eos)
    return _ops.ctc_beam_search_lm(x, lengths, blank, beam_width, top_k, *model, min_logp)


def beam_decode_biased(logits, graph, lm=None, lm_weight=0.0, length_bonus=0.0, beam_width=16, top_k=16, blank=0, lengths=None,
                       min_logp=None, use_eos=True):
    """``beam_decode`` (`lm` None) or ``beam_decode_lm`` with contextual phrase biasing in the ranking while the beam is open:
    `graph` is an ``asr.bias.ContextGraph`` over the logits' inventory (moved to the logits' device on first use).  Every
    hypothesis carries the bonus of the phrases it contains plus an advance on the phrase it is in the middle of, which is
    taken back if the phrase is not completed, so the beam keeps the start of a listed phrase alive until its last token
    arrives.  Hypotheses are kept and sorted by log p_ctc(h | x) + lm_weight * log p_lm(h) + length_bonus * |h| + bias(h),
    bias(h) the sum of weight * length over every occurrence of every phrase in h.
    -> (ids, lengths, scores (the combined score), ctc_scores, lm_scores, bias_scores), the last four (B, beam_width) f32.
    Unused slots: length 0, scores and ctc_scores -inf, lm_scores and bias_scores 0.  Without `lm`, lm_scores is all 0 and
    `lm_weight`, `length_bonus` and `use_eos` have no effect."""
    x, lengths, _, model, image = _prepared(logits, blank, lengths, None, lm, lm_weight, length_bonus, use_eos, graph)
    return _ops.ctc_beam_search_bias(x, lengths, blank, beam_width, top_k, image, *model, min_logp)


class _Stream:
    """What ``BeamStream`` and ``GramBeamStream`` share: the dimensions and options, the device, the frame counts (`fed` on the
    host, `frames` on the device), the argument checks of ``reset`` and ``advance``, and ``commit``, which lets a stream run
    for any number of frames."""

    # what a family is, for the methods below: its functions in _ops (``_OPS`` + "reset" ...), whether it is the Gram-CTC stream
    # (the table `gram` goes to advance, and a frame gives two tokens, i.e. table nodes per beam slot, not one), and where the
    # model's <s> goes: to reset, or to advance and result
    _OPS = "ctc_beam_stream_"
    _GRAM = False
    _BOS_AT_RESET = True

    def __init__(self, B, V, max_frames, beam_width, top_k, blank, min_logp, lm, lm_weight, length_bonus, device):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.B, self.V, self.max_frames, self.beam_width, self.top_k = int(B), int(V), int(max_frames), int(beam_width), int(top_k)
        self.blank, self.min_logp = int(blank), min_logp
        self.lm = None if lm is None else lm.to(self.device)
        self.lm_weight, self.length_bonus = (float(lm_weight), float(length_bonus)) if lm is not None else (0.0, 0.0)
        self.fed = 0                              # frames fed since the last full reset: the capacity every slot has used
        self.frames = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.committed = [[] for _ in range(self.B)]          # per utterance: the tokens ``commit`` has made final
        self.frames_base = torch.zeros((self.B,), dtype=torch.int32, device=self.device)   # frames - the table rows in use

    def _new_state(self, graph):
        self.graph = None if graph is None else graph.to(self.device)
        nbytes = self._op("state_bytes")(self.B, self.beam_width, self.max_frames, self.lm is not None, graph is not None)
        self.state = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        self.reset()

    def _op(self, verb):
        return getattr(_ops, self._OPS + verb)

    def _bos(self, at_reset):
        """the model's <s> as one positional argument of the calls that take it, none of the others"""
        return (-1 if self.lm is None else self.lm.bos_id,) if at_reset == self._BOS_AT_RESET else ()

    def _images(self):
        return (None if self.lm is None else self.lm.image), (None if self.graph is None else self.graph.image)

    def reset(self, mask=None):
        """start every utterance over, or those with mask[b] != 0 (`mask`: (B) integers, host or device)"""
        self._op("reset")(self.state, self.B, self.beam_width, self.max_frames, self.lm is not None, self.graph is not None,
                          *self._bos(True), self._reset_mask(mask))

    def advance(self, logits, lengths=None):
        """consume a chunk (Tc, B, V) of f32 logits; `lengths` (B): the valid frames of this chunk per utterance (0: the
        utterance is left as it is; frames past the length are never read), None: all Tc"""
        chunk = self._chunk(logits, lengths)
        if chunk is None:
            return
        self._op("advance")(self.state, chunk[0], chunk[1], self.blank, self.beam_width, self.top_k,
                            *((self.gram,) if self._GRAM else ()), self.fed, self.max_frames, *self._images(), self.lm_weight,
                            self.length_bonus, *self._bos(False), self.min_logp)
        self.fed += chunk[0].shape[0]

    def result(self, use_eos=True):
        """the N-best of the frames fed so far: the tuple of the one-shot function without a model or a graph (3), with `lm` (5)
        or with `graph` (6), with ids of shape (B, beam_width, tokens the frames fed can give: one per frame, Gram-CTC two); the
        search goes on unchanged.  Sets ``frames`` (B) int32 on the device: the frames every utterance has consumed."""
        width = (2 if self._GRAM else 1) * self.fed
        eos = self.lm.eos_id if self.lm is not None and use_eos else -1
        out, rows = self._op("result")(self.state, self.B, self.beam_width, self.max_frames, self.blank, max(width, 1),
                                       *self._images(), self.lm_weight, self.length_bonus, *self._bos(False), eos)
        self._set_frames(rows)
        return (out[0][:, :, :width],) + out[1:]

    def _reset_mask(self, mask):
        """`mask` of ``reset`` as a (B) int32 device tensor; None (a full reset) also starts the frame count over.  Once tokens
        have been committed the masked slots' ``committed`` lists are emptied here, for which a mask given as a device tensor
        is copied to the host (a synchronisation; a mask given as a list or a host array costs none)."""
        if mask is None:
            self.fed = 0
            self.committed = [[] for _ in range(self.B)]
            self.frames_base.zero_()
            return None
        host = mask
        mask = torch.as_tensor(mask).to(self.device, torch.int32).contiguous()
        if tuple(mask.shape) != (self.B,):
            raise ValueError("mask must have one entry per utterance (%d)" % self.B)
        self.frames_base.masked_fill_(mask != 0, 0)   # (a commit of no tokens compacts as well: not only where tokens are committed)
        if any(self.committed):                   # (only a stream that has committed tokens looks at the mask on the host)
            for b, on in enumerate(torch.as_tensor(host).tolist()):
                if on:
                    self.committed[b] = []
        return mask

    def _set_frames(self, rows):
        """``frames`` from result's out_frames, which counts table rows once something has been committed"""
        self.frames = torch.where(rows < 0, rows, rows + self.frames_base)

    def commit(self, prefix=None, lengths=None, compact=True):
        """Make a prefix final and free the table rows behind it.  `prefix` (B, n) token ids (characters for the Gram-CTC stream)
        with `lengths` (B) or None (all n), host or device: per utterance the hypotheses whose tokens after the committed ones
        do not start with it are dropped, the prefix is appended to ``self.committed[b]``, and ``result()`` returns what comes
        after it from then on.  `prefix` None, or a negative length: the longest common prefix of the live hypotheses, which
        drops nothing.  An utterance none of whose hypotheses starts with its prefix is refused and stays as it is.
        `compact` False only reports.  -> (tokens (B, width) int32: the first counts[b] of a row are what this call committed,
        the rest is 0, and width = max(the table's tokens per slot in use, n, 1), i.e. what an auto commit could commit;
        counts (B); status (B): 1 applied, 0 refused, -1 another stream's state) on the device.  Unlike the other methods this
        one synchronises with the host: it reads the counts to keep ``committed`` and the capacity check of ``advance``, which
        counts table rows in use after a commit.  (``reset(mask)`` with a device mask does too, once tokens are committed.)"""
        per = 2 if self._GRAM else 1
        pitch = per * self.fed
        if prefix is not None:
            prefix = torch.as_tensor(prefix).to(self.device, torch.int32)
            if prefix.dim() != 2 or prefix.shape[0] != self.B:
                raise ValueError("prefix must be (%d, n), got %s" % (self.B, tuple(prefix.shape)))
            n = prefix.shape[1]
            if lengths is None:
                lengths = torch.full((self.B,), n, dtype=torch.int32, device=self.device)
            else:
                lengths = torch.as_tensor(lengths).to(self.device, torch.int32).clamp(max=n).contiguous()
                if tuple(lengths.shape) != (self.B,):
                    raise ValueError("lengths must have one entry per utterance (%d)" % self.B)
            if n == 0:                            # nothing to compare: a row of one unused token keeps the pitch positive
                prefix = torch.zeros((self.B, 1), dtype=torch.int32, device=self.device)
            prefix = prefix.contiguous()
            pitch = max(pitch, n)
        before = self.state[:self.B * 32].view(torch.int32).view(self.B, 8)[:, 6].clone()       # the header's rows in use
        tokens, counts, _, rows, status = _ops.beam_stream_commit(self.state, self._GRAM, self.B, self.beam_width, self.max_frames,
                                                                   self.lm is not None, self.graph is not None, prefix, lengths,
                                                                   compact, None, pitch)
        if compact:
            self.frames_base += torch.where(status == 1, before - rows, torch.zeros_like(rows))
            host_tokens, host_counts = tokens.cpu().tolist(), counts.cpu().tolist()
            for b in range(self.B):
                self.committed[b].extend(host_tokens[b][:host_counts[b]])
            self.fed = max(int(rows.max()), 0)
        return tokens, counts, status

    def commit_best(self, hold=8):
        """the usual policy: commit the best hypothesis of every utterance without its last `hold` tokens -> ``commit``'s tuple"""
        out = self.result()
        return self.commit(out[0][:, 0], (out[1][:, 0] - int(hold)).clamp(min=0))

    def full_result(self, use_eos=True):
        """``result()`` with ``self.committed`` put back in front of every hypothesis: the tuple an uncommitted stream returns, as
        long as every commit was of the common prefix; ids (B, beam_width, longest committed + the tails' width)"""
        out = self.result(use_eos)
        ids, lens, scores = out[0], out[1], out[2]
        counts = [len(c) for c in self.committed]
        width = max(counts)
        if width == 0:
            return out
        live = scores > -float("inf")
        full = torch.full((self.B, self.beam_width, width + ids.shape[2]), self.blank, dtype=ids.dtype, device=self.device)
        for b, done in enumerate(self.committed):
            full[b, :, len(done):len(done) + ids.shape[2]] = ids[b]
            if done:
                full[b, :, :len(done)] = torch.tensor(done, dtype=ids.dtype, device=self.device)
        full = torch.where(live[:, :, None], full, torch.full_like(full, self.blank))
        lens = torch.where(live, lens + torch.tensor(counts, dtype=lens.dtype, device=self.device)[:, None], lens)
        return (full, lens) + tuple(out[2:])

    def _chunk(self, logits, lengths):
        """the arguments of ``advance``, checked -> (logits, lengths) on the device, or None for an empty chunk"""
        if logits.dim() != 3 or logits.shape[1] != self.B or logits.shape[2] != self.V:
            raise ValueError("the chunk must be (Tc, %d, %d), got %s" % (self.B, self.V, tuple(logits.shape)))
        Tc = logits.shape[0]
        if Tc == 0:
            return None
        if self.fed + Tc > self.max_frames:
            raise ValueError("%d frames fed since the last full reset, %d more exceed max_frames = %d"
                             % (self.fed, Tc, self.max_frames))
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(self.device, torch.int32).contiguous()
            if tuple(lengths.shape) != (self.B,):
                raise ValueError("lengths must have one entry per utterance (%d)" % self.B)
        return logits.to(self.device, torch.float32).contiguous(), lengths


class BeamStream(_Stream):
    """``beam_decode`` / ``beam_decode_lm`` (`lm`) / ``beam_decode_biased`` (`graph`, with or without `lm`) fed chunk by chunk:
    the beam of `B` utterances lives on the device between the calls.  However the frames are cut into chunks, ``result()``
    after a chunk is bit for bit what the one-shot function returns for the frames fed so far.

        s = BeamStream(B, V, max_frames, beam_width=16, top_k=16, lm=lm, lm_weight=0.5, length_bonus=1.0)
        for chunk in chunks:                    # (Tc, B, V) f32 logits on the device
            s.advance(chunk)                    # lengths=(B) int32: the valid frames of this chunk per utterance
            ids, lens, scores, ctc, lms = s.result()

    ``reset()`` starts all utterances over; ``reset(mask)`` only those with mask[b] != 0, so a serving loop can put a new
    utterance into a batch slot while the others go on.  The prefix table holds `max_frames` frames per utterance: the frames
    fed are counted on the host from the last full reset, a partial reset does not lower that count, and feeding beyond
    `max_frames` raises ValueError.  Nothing here synchronises with the host, except ``commit`` and, once tokens have been
    committed, ``reset(mask)`` with a mask that is a device tensor (a list or a host array costs nothing).

    A stream longer than `max_frames` commits as it goes: ``commit(prefix)`` makes a prefix of the hypotheses final, drops the
    hypotheses that disagree with it and frees the table rows behind it, and ``commit_best(hold)`` does so with the best
    hypothesis minus its last `hold` tokens.  From then on ``result()`` returns tails, the tokens after ``self.committed[b]``,
    with the scores of the whole hypotheses; ``full_result()`` puts the committed tokens back in front; the capacity check counts
    the table rows in use, and ``frames`` still counts the frames consumed."""

    def __init__(self, B, V, max_frames, beam_width=16, top_k=16, blank=0, min_logp=None, lm=None, lm_weight=0.0, length_bonus=0.0,
                 graph=None, device=None):
        if B <= 0 or V <= 0 or max_frames <= 0:
            raise ValueError("B, V and max_frames must be positive")
        if graph is not None and (graph.V != V or graph.blank != blank):
            raise ValueError("the context graph was built for %d ids with blank %d, the stream has %d with blank %d"
                             % (graph.V, graph.blank, V, blank))
        super().__init__(B, V, max_frames, beam_width, top_k, blank, min_logp, lm, lm_weight, length_bonus, device)
        self._new_state(graph)



def check_gram_table(gram, V, blank=0):
    """Raise ValueError unless `gram` (NumPy) is a (V, 2) integer table as ``asr.vocab.gram_table`` makes it: (-1, -1) for the
    blank, every other row (-1, -1), (u, -1) or (u1, u2) with ids in [0, V), and no two tokens with the same spelling."""
    g = np.asarray(gram)
    if g.ndim != 2 or g.shape != (V, 2) or g.dtype.kind not in "iu":
        raise ValueError("gram must be an integer array of shape (V, 2) = (%d, 2)" % V)
    if not 0 <= blank < V or tuple(g[blank]) != (-1, -1):
        raise ValueError("the blank row of gram must be (-1, -1)")
    if np.any(g >= V) or np.any(g < -1):
        raise ValueError("gram spells with ids outside [0, V)")
    if np.any((g[:, 0] < 0) & (g[:, 1] >= 0)):
        raise ValueError("a bigram row of gram must name its first unigram")
    used = g[g[:, 0] >= 0]
    if len(np.unique(used, axis=0)) != len(used):
        raise ValueError("two tokens of gram have the same spelling")


def _gram_table(gram, V, blank, device):
    """`gram` (NumPy or a device tensor), checked, as a contiguous (V, 2) int32 tensor on `device`"""
    if isinstance(gram, torch.Tensor):
        check_gram_table(gram.cpu().numpy(), V, blank)
        return gram.to(device, torch.int32).contiguous()
    check_gram_table(gram, V, blank)
    return torch.from_numpy(np.ascontiguousarray(gram, np.int32)).to(device)


def gram_beam_decode(logits, gram, beam_width=16, top_k=16, blank=0, lengths=None, min_logp=None):
    """``beam_decode`` for the Gram-CTC inventory, over spelled strings: (T, B, V) f32 logits on the GPU and the table `gram`
    (V, 2) of ``asr.vocab.gram_table`` (NumPy, checked here; or an int32 device tensor, checked too, at the cost of a copy to
    the host) -> (ids (B, beam_width, 2T) int32 padded with blank, lengths (B, beam_width) int32, scores (B, beam_width) f32).
    A hypothesis is a string of unigrams; its score sums every way of cutting it into unigram and bigram tokens that the beam
    kept, so it is log p(string | x) under Gram-CTC (a lower bound on it), no string takes two slots, and the ranking and the
    pruning see whole strings.  The ids are unigram ids already: one slot goes straight into
    ``compute_sequence_error(ids[:, k], lengths[:, k], t_batch, blank, None, None)`` with no retokenisation on the host.
    Candidates, `lengths` and `min_logp` as in ``beam_decode``.  ``gram_ctc_align`` on a decoded string gives its best cut.
    ``gram_beam_decode_lm`` is this search with a character n-gram language model in the ranking."""
    x, lengths, table, _, _ = _prepared(logits, blank, lengths, gram)
    return _ops.gram_ctc_beam_search(x, lengths, blank, beam_width, top_k, table, min_logp)


def gram_beam_decode_lm(logits, gram, lm, lm_weight, length_bonus, beam_width=16, top_k=16, blank=0, lengths=None, min_logp=None,
                        use_eos=True):
    """``gram_beam_decode`` with an n-gram language model over the spelled characters in the ranking while the beam is open:
    strings are kept and sorted by log p_gram_ctc(s | x) + lm_weight * log p_lm(s) + length_bonus * |s|, |s| in characters.
    `gram` is validated as in ``gram_beam_decode``.  `lm` is an ``asr.lm.NGramLM`` over the unigram ids that the table spells
    with (moved to the logits' device on first use): make it with ``NGramLM.from_arpa(text, unigram_token_to_id, V=V)``, V the
    size of the logits' inventory, so that <s> / </s> become the ids V and V + 1 above every token id; a model with
    ``lm.vlm < V`` raises ValueError.  Its `bos` starts every context and, with `use_eos`, its `eos` closes every string after
    the last frame.  A bigram token adds the steps of its two characters, so log p_lm(s) does not depend on how s was cut.
    -> (ids (B, beam_width, 2T), lengths, scores (the combined score), ctc_scores, lm_scores), the last three (B, beam_width)
    f32.  Unused slots: length 0, scores and ctc_scores -inf, lm_scores 0."""
    x, lengths, table, model, _ = _prepared(logits, blank, lengths, gram, lm, lm_weight, length_bonus, use_eos)
    return _ops.gram_ctc_beam_search_lm(x, lengths, blank, beam_width, top_k, table, *model, min_logp)


def gram_beam_decode_biased(logits, gram, graph, lm=None, lm_weight=0.0, length_bonus=0.0, beam_width=16, top_k=16, blank=0,
                            lengths=None, min_logp=None, use_eos=True):
    """``gram_beam_decode`` (`lm` None) or ``gram_beam_decode_lm`` with contextual phrase biasing in the ranking while the beam is
    open, ``beam_decode_biased`` for the Gram-CTC inventory.  `graph` is an ``asr.bias.ContextGraph`` over the unigram ids that
    the table spells with, built for the logits' V and blank (``ContextGraph.from_text(lines, unigram_token_to_id, V=V)``; moved to
    the logits' device on first use); a phrase with an id that no row of `gram` spells never matches.  A bigram token advances
    the automaton by its two characters in string order, so the bonus of a string does not depend on how it was cut into tokens.
    Strings are kept and sorted by log p_gram_ctc(s | x) + lm_weight * log p_lm(s) + length_bonus * |s| + bias(s), bias(s) the
    sum of weight * length over every occurrence of every phrase in s.  `gram` and `lm` are validated as in
    ``gram_beam_decode_lm``.
    -> (ids (B, beam_width, 2T), lengths, scores (the combined score), ctc_scores, lm_scores, bias_scores), the last four
    (B, beam_width) f32; ids, lengths and the score to rank by go into ``mbr_decode`` unchanged.  Unused slots: length 0, scores and ctc_scores
    -inf, lm_scores and bias_scores 0.  Without `lm`, lm_scores is all 0 and `lm_weight`, `length_bonus` and `use_eos` have no
    effect."""
    x, lengths, table, model, image = _prepared(logits, blank, lengths, gram, lm, lm_weight, length_bonus, use_eos, graph)
    return _ops.gram_ctc_beam_search_bias(x, lengths, blank, beam_width, top_k, table, image, *model, min_logp)


class GramBeamStream(_Stream):
    """``gram_beam_decode`` / ``gram_beam_decode_lm`` (`lm`) / ``gram_beam_decode_biased`` (`graph`, with or without `lm`) fed chunk
    by chunk: the beam of strings of `B` utterances lives on the device between the calls.  However the frames are cut into
    chunks, ``result()`` after a chunk is bit for bit what the one-shot function returns for the frames fed so far.

        s = GramBeamStream(B, V, max_frames, gram, beam_width=16, top_k=16, lm=lm, lm_weight=0.5, length_bonus=1.0)
        for chunk in chunks:                    # (Tc, B, V) f32 logits on the device
            s.advance(chunk)                    # lengths=(B) int32: the valid frames of this chunk per utterance
            ids, lens, scores, ctc, lms = s.result()

    `gram` is validated once, here, as ``gram_beam_decode`` validates it; `lm` as in ``gram_beam_decode_lm`` (``lm.vlm < V`` raises
    ValueError); `graph` as in ``gram_beam_decode_biased`` (built for another V or blank raises ValueError), and with it
    ``result()`` returns the 6-tuple.  ``reset``, partial resets, the frame count and `max_frames` behave as in ``BeamStream``;
    the prefix table holds two characters per frame.  Nothing here synchronises with the host, except ``commit``, which works
    as in ``BeamStream`` with characters for tokens."""

    # the entries with a graph argument are the family: without a graph they are the narrow ones, size for size and byte for byte
    _OPS = "gram_ctc_beam_bias_stream_"
    _GRAM = True
    _BOS_AT_RESET = False

    def __init__(self, B, V, max_frames, gram, beam_width=16, top_k=16, blank=0, min_logp=None, lm=None, lm_weight=0.0,
                 length_bonus=0.0, device=None, graph=None):
        if B <= 0 or V <= 0 or max_frames <= 0:
            raise ValueError("B, V and max_frames must be positive")
        if lm is not None and lm.vlm < V:
            raise ValueError("the language model covers %d ids, fewer than the %d of the logits" % (lm.vlm, V))
        if graph is not None and (graph.V != V or graph.blank != blank):
            raise ValueError("the context graph was built for %d ids with blank %d, the stream has %d with blank %d"
                             % (graph.V, graph.blank, V, blank))
        super().__init__(B, V, max_frames, beam_width, top_k, blank, min_logp, lm, lm_weight, length_bonus, device)
        self.gram = _gram_table(gram, self.V, self.blank, self.device)
        self._new_state(graph)


def _retokenised(pred, pred_len, BLANK, vocab_token_to_id, vocab_id_to_token):
    """collapsed predictions as unigram ids: themselves, unless the inventory has multi-unigram tokens (asr/error.py:49-53)"""
    if not _needs_retokenisation(vocab_id_to_token, vocab_token_to_id):
        return pred, pred_len
    # string work: inherently host side (only for inventories with multi-unigram tokens)
    dev = pred.device
    ph, pl = pred.cpu().numpy(), pred_len.cpu().numpy()
    rows = []
    for b in range(ph.shape[0]):
        sentence = "".join(vocab_id_to_token[int(i)] for i in ph[b, :pl[b]])
        rows.append(convert_sentence_to_unigram_ids(sentence, vocab_token_to_id))
    width = max(1, max(len(r) for r in rows))
    host = np.full((len(rows), width), BLANK, dtype=np.int32)
    for b, r in enumerate(rows):
        host[b, :len(r)] = r
    return torch.from_numpy(host).to(dev), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)


def _error_rate(pred, pred_len, true, true_len, BLANK, vocab_token_to_id, vocab_id_to_token, print_sequences):
    """mean over the batch of Levenshtein(pred, true) / len(true) for collapsed id rows on the GPU (asr/error.py:49-68)"""
    pred, pred_len = _retokenised(pred, pred_len, BLANK, vocab_token_to_id, vocab_id_to_token)
    dist = _ops.edit_distance(true, true_len, pred, pred_len)
    d, n = dist.cpu().numpy().astype(np.float64), true_len.cpu().numpy()
    _ops.gru_check_all()        # the ids came from a forward pass nobody else checks: raise if a recurrence gave up a wait
    per = np.where(n > 0, d / np.maximum(n, 1), d)         # len(r) == 0: the distance is len(h), returned as it is
    if print_sequences and vocab_id_to_token is not None:
        ph, pl, th, tl = pred.cpu().numpy(), pred_len.cpu().numpy(), true.cpu().numpy(), true_len.cpu().numpy()
        for b in range(ph.shape[0]):
            print("#{}".format(b + 1))
            print("pred:\t" + "".join(vocab_id_to_token[int(i)] for i in ph[b, :pl[b]]))
            print("true:\t" + "".join(vocab_id_to_token[int(i)] for i in th[b, :tl[b]]))
    return float(per.sum() / len(per))


def _device_ids(a, dev):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(dev, torch.int32).contiguous()


def compute_minibatch_error(y_batch, t_batch, BLANK, vocab_token_to_id, vocab_id_to_token, print_sequences=False):
    """y_batch (B, T): argmax ids per frame; t_batch (B, L): labels padded with BLANK.  Mean over the minibatch of
    Levenshtein(pred, true) / len(true)  (len(pred) where the transcription is empty)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    y = _device_ids(y_batch, dev)
    t = _device_ids(t_batch, dev)
    pred, pred_len = _ops.ctc_collapse(y, None, BLANK, True)
    true, true_len = _ops.ctc_collapse(t, None, BLANK, False)
    return _error_rate(pred, pred_len, true, true_len, BLANK, vocab_token_to_id, vocab_id_to_token, print_sequences)


def compute_sequence_error(pred, pred_len, t_batch, BLANK, vocab_token_to_id, vocab_id_to_token, print_sequences=False):
    """The error rate of ``compute_minibatch_error`` for hypotheses that are already collapsed label sequences, e.g. one slot
    of ``beam_decode``: pred (B, L) ids (entries past pred_len[b] are ignored), pred_len (B); t_batch (B, L') labels padded
    with BLANK.  Same retokenisation (Gram-CTC inventories) and the same edit-distance tail."""
    dev = torch.device("cuda", torch.cuda.current_device())
    p = _device_ids(pred, dev)
    pl = _device_ids(pred_len, dev)
    if p.dim() != 2 or pl.shape != (p.shape[0],):
        raise ValueError("pred must be (B, L) and pred_len (B)")
    pl = pl.clamp(0, p.shape[1]).contiguous()
    if p.shape[1] == 0:
        p = torch.full((p.shape[0], 1), BLANK, dtype=torch.int32, device=dev)
    t = _device_ids(t_batch, dev)
    true, true_len = _ops.ctc_collapse(t, None, BLANK, False)
    return _error_rate(p, pl, true, true_len, BLANK, vocab_token_to_id, vocab_id_to_token, print_sequences)


# ------------------------------------------------------------------------------------------ edit alignment, counts, consensus
# Back-pointer bytes one launch of asr_edit_align / asr_nbest_consensus may ask for; beyond it the wrappers split the pairs (the
# utterances) over several launches that reuse the same workspace.  One cell is one byte, stored diagonal by diagonal in
# (Lr + Lh - 1) * min(Lr, Lh) bytes per pair: 256 MiB hold 2048 pairs of 256 x 256.
ALIGN_WORKSPACE_BUDGET = 256 << 20

EditAlignment = collections.namedtuple("EditAlignment", "distance substitutions deletions insertions ref_to_hyp hyp_to_ref")
ErrorCounts = collections.namedtuple("ErrorCounts", "substitutions deletions insertions reference_length")
MBR = collections.namedtuple("MBR", "ids lengths index risk posterior confidence")


def _id_rows(a, a_len, dev):
    """a padded id matrix and its lengths as contiguous int32 device tensors -> (ids, at least one column wide; lengths, which
    the kernel clamps to [0, L]; L)"""
    a, a_len = _device_ids(a, dev), _device_ids(a_len, dev)
    if a.dim() != 2 or tuple(a_len.shape) != (a.shape[0],):
        raise ValueError("ids must be (pairs, L) and lengths (pairs)")
    L = a.shape[1]
    if L == 0:          # no column to point at: one of padding, and every length 0
        a, a_len = torch.zeros((a.shape[0], 1), dtype=torch.int32, device=dev), torch.zeros_like(a_len)
    return a, a_len, L


def edit_alignment(ref, ref_len, hyp, hyp_len, paths=True):
    """Row-wise Levenshtein alignment of two padded int32 id matrices ref (pairs, Lr) / ref_len (pairs) and hyp (pairs, Lh) /
    hyp_len (pairs) on the GPU -> ``EditAlignment(distance, substitutions, deletions, insertions, ref_to_hyp, hyp_to_ref)`` of
    device tensors: four (pairs) int32 counts with distance = substitutions + deletions + insertions; ref_to_hyp (pairs, Lr) the
    hypothesis position aligned to each reference position by a match or a substitution, -1 where the position is deleted or
    beyond the length; hyp_to_ref (pairs, Lh) likewise, -1 for an insertion.  Lengths are clamped to [0, L]; ids beyond them are
    never read.  ``paths=False`` returns the same counts, None for the maps, and needs no workspace.

    Several alignments reach the same distance (``ab`` against ``ba``: two substitutions, or a deletion and an insertion around
    either match); the one reported walks back from the ends and takes, in this order, a match, a substitution, a deletion, an
    insertion.  The back-pointers take (Lr + Lh - 1) * min(Lr, Lh) bytes per pair: beyond
    ``ALIGN_WORKSPACE_BUDGET`` bytes the pairs are split over several launches.  Lr above 5460 (the sweep's diagonals live in LDS) raises ``AsrHipError``."""
    dev = torch.device("cuda", torch.cuda.current_device())
    r, rl, Lr = _id_rows(ref, ref_len, dev)
    h, hl, Lh = _id_rows(hyp, hyp_len, dev)
    if r.shape[0] != h.shape[0]:
        raise ValueError("ref and hyp must have one row per pair")
    counts, rmap, hmap = _ops.edit_align(r, rl, h, hl, paths, ALIGN_WORKSPACE_BUDGET)
    if paths:
        rmap, hmap = rmap[:, :Lr], hmap[:, :Lh]
    return EditAlignment(counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3], rmap, hmap)


def error_counts(pred, pred_len, true, true_len):
    """Substitutions, deletions, insertions and reference length per utterance -> ``ErrorCounts`` of four (B) int32 device tensors:
    pred (B, L) / pred_len (B) collapsed hypotheses, true (B, L') / true_len (B) the transcripts they are aligned against
    (``edit_alignment``'s pinned path, no maps).  S + D + I is the Levenshtein distance ``compute_minibatch_error`` divides by the
    reference length."""
    a = edit_alignment(true, true_len, pred, pred_len, paths=False)
    dev = a.distance.device
    n_ref = _device_ids(true_len, dev).clamp(0, _device_ids(true, dev).shape[1])
    return ErrorCounts(a.substitutions, a.deletions, a.insertions, n_ref)


def compute_minibatch_error_counts(y_batch, t_batch, BLANK, vocab_token_to_id, vocab_id_to_token):
    """The arguments of ``compute_minibatch_error`` and the same collapse and retokenisation -> ``ErrorCounts`` of four Python
    ints, the totals over the minibatch: what a corpus-level error rate (S + D + I) / N_ref and its breakdown are summed from."""
    dev = torch.device("cuda", torch.cuda.current_device())
    y = _device_ids(y_batch, dev)
    t = _device_ids(t_batch, dev)
    pred, pred_len = _ops.ctc_collapse(y, None, BLANK, True)
    true, true_len = _ops.ctc_collapse(t, None, BLANK, False)
    pred, pred_len = _retokenised(pred, pred_len, BLANK, vocab_token_to_id, vocab_id_to_token)
    totals = torch.stack(error_counts(pred, pred_len, true, true_len)).sum(dim=1).cpu()
    _ops.gru_check_all()        # as in compute_minibatch_error: the ids came from a forward pass nobody else checks
    return ErrorCounts(*(int(v) for v in totals))


def mbr_decode(ids, lengths, scores, scale=1.0, confidence=True):
    """Minimum-Bayes-risk pick from an N-best list, the decode-side dual of ``asr.loss.mwer_loss``: ids (B, N, L) int32, lengths
    (B, N) int32 and scores (B, N) float exactly as ``beam_decode``, ``beam_decode_lm``, ``beam_decode_biased``, ``gram_beam_decode*``
    or a ``*Stream.result()`` return them (for the searches with more scores, pass the one to rank by).  A slot is used iff its
    score is finite; an empty hypothesis with a finite score is a hypothesis.  With post = softmax(scale * scores) over the used
    slots and dist the Levenshtein distance between slots,

        risk[b, i] = sum_j post[b, j] dist[b, i, j]   (+inf for an unused i),      index[b] = argmin_i risk[b, i]

    (ties to the lowest index; -1 where no slot is used): the hypothesis with the least expected number of errors under the
    list's own posterior.  -> ``MBR(ids (B, L), lengths (B), index (B) int32, risk (B, N) f64, posterior (B, N) f64, confidence
    (B, L) f32 or None)``; ids / lengths are the chosen slot's (slot 0's ids with length 0 where index is -1).  confidence[b, l]
    is the posterior mass of the hypotheses that, aligned against the chosen one by ``edit_alignment``'s rule, carry the same
    token at its position l (0 at and beyond its length): a token confidence over competing hypotheses, which ``ctc_align``'s
    acoustic log-probability is not.  For a Gram-CTC list the units are characters.

    Beam scores are lower bounds on log p(hypothesis | x): the beam drops paths.  ``asr.loss.ctc_nbest_logp`` /
    ``gram_ctc_nbest_logp`` give the exact ones, to be passed as `scores`.  The distances and the confidence are integer kernels
    (asr_nbest_pairwise_distance, asr_nbest_consensus, in launches of at most ``ALIGN_WORKSPACE_BUDGET`` workspace bytes); the
    (B, N) arithmetic is float64 torch on the device, as in ``mwer_parts``.  Nothing here synchronises with the host.  The
    consensus workspace grows with L squared: a caller who can afford one synchronisation cuts the T-wide ids of a search to the
    longest hypothesis first, as ``mwer_loss`` does (B = 32, N = 16: 0.55 ms instead of 1.16 ms at L = 1000)."""
    if ids.dim() != 3 or tuple(lengths.shape) != tuple(ids.shape[:2]) or tuple(scores.shape) != tuple(ids.shape[:2]):
        raise ValueError("ids must be (B, N, L), lengths and scores (B, N)")
    if ids.dtype != torch.int32 or lengths.dtype != torch.int32:
        raise TypeError("ids and lengths must be int32")
    B, N, L = ids.shape
    if N == 0:
        raise ValueError("the list has no slots")
    dev = ids.device
    if L == 0:
        ids = torch.zeros((B, N, 1), dtype=torch.int32, device=dev)
    ids = ids.contiguous()
    used = torch.isfinite(scores)
    lens = torch.where(used, lengths.clamp(0, L), torch.full_like(lengths, -1)).contiguous()
    dist = _ops.nbest_pairwise_distance(ids, lens)
    s = torch.where(used, float(scale) * scores.double(), torch.full_like(scores, float("-inf"), dtype=torch.float64))
    top = s.max(dim=1, keepdim=True).values
    e = torch.where(used, torch.exp(s - torch.where(torch.isfinite(top), top, torch.zeros_like(top))), torch.zeros_like(s))
    z = e.sum(dim=1, keepdim=True)
    post = e / torch.where(z > 0, z, torch.ones_like(z))
    risk = torch.where(used, (post[:, None, :] * dist.double()).sum(dim=2), torch.full_like(post, float("inf")))
    slot = torch.arange(N, device=dev)[None, :].expand(B, N)
    first = torch.where(risk == risk.min(dim=1, keepdim=True).values, slot, torch.full_like(slot, N)).min(dim=1).values
    index = torch.where(used.any(dim=1), first, torch.full_like(first, -1)).to(torch.int32)
    pick = index.clamp_min(0).long()
    out_ids = ids.gather(1, pick[:, None, None].expand(B, 1, ids.shape[2]))[:, 0, :L]
    out_len = torch.where(index >= 0, lens.gather(1, pick[:, None])[:, 0], torch.zeros_like(index))
    conf = None
    if confidence:
        conf = _ops.nbest_consensus(ids, lens, index.contiguous(), post.to(torch.float32).contiguous(), ALIGN_WORKSPACE_BUDGET)[:, :L]
    return MBR(out_ids, out_len, index, risk, post, conf)
