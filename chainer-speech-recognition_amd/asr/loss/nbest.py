"""Sequence-level criteria over a set of hypotheses per utterance, on the HIP path.

``ctc_nbest_logp`` gives the exact log p(h_n | x_b) of N labellings per utterance under CTC -- every path, not the lower
bound ``asr.error.beam_decode`` reports for what its beam kept -- and lets the gradient flow back into the logits.
``mwer_loss`` is the expected number of errors (minimum word error rate training, Prabhavalkar et al. 2018) over such a set.
The reference has neither; its only sequence criterion is the CTC / Gram-CTC loss.

The N hypotheses of an utterance share its logit rows: the kernels (csrc/ctc_nbest.hip) read the (T, B, V) logits once and
write one (T, B, V) gradient, whatever N is; only the lattices are per hypothesis.

``gram_ctc_nbest_logp`` and ``gram_mwer_loss`` are the same for a Gram-CTC model: the hypotheses are strings of characters (what
``asr.error.gram_beam_decode`` returns) and log p(string | x) sums every way of cutting the string into the unigram and bigram
tokens of the inventory.
"""
import collections

import numpy as np
import torch

from .. import _lib
from .ctc import _check_common


class _NbestFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xs, hyps, hyp_lengths, input_length, blank, gram):
        """gram None: CTC over labels; a checked (V, 2) int32 device table: Gram-CTC over characters"""
        lib = _lib.lib()
        if xs.dtype != torch.float32:
            raise TypeError("xs must be float32")
        for t in (hyps, hyp_lengths, input_length):
            if t is not None and t.dtype != torch.int32:
                raise TypeError("labels and lengths must be int32")
        xs = xs.contiguous()
        _lib.ptr(xs)                # raises on a CPU tensor: there is no CPU path
        T, B, V = xs.shape
        if hyps.dim() != 3 or hyps.shape[0] != B or tuple(hyp_lengths.shape) != tuple(hyps.shape[:2]):
            raise ValueError("hyps must be (B, N, L) and hyp_lengths (B, N)")
        if input_length is not None and tuple(input_length.shape) != (B,):
            raise ValueError("input_length must be (B,)")
        N, Lmax = int(hyps.shape[1]), int(hyps.shape[2])
        if Lmax == 0:               # only empty hypotheses: one column that no length reaches
            hyps, Lmax = torch.full((B, N, 1), int(blank), dtype=torch.int32, device=xs.device), 1
        hyps, hyp_lengths = hyps.contiguous(), hyp_lengths.contiguous()
        input_length = None if input_length is None else input_length.contiguous()
        query = lib.asr_ctc_nbest_workspace_bytes if gram is None else lib.asr_gram_ctc_nbest_workspace_bytes
        nbytes = query(T, B, V, N, Lmax)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=xs.device)
        logp = torch.empty((B, N), dtype=torch.float32, device=xs.device)
        if gram is None:
            rc = lib.asr_ctc_nbest_forward(_lib.stream(), _lib.ptr(xs), _lib.ptr(hyps), _lib.ptr(hyp_lengths), _lib.ptr(input_length),
                                           T, B, V, N, Lmax, int(blank), _lib.ptr(logp), _lib.ptr(ws), nbytes)
            _lib.check(rc, "asr_ctc_nbest_forward")
        else:
            rc = lib.asr_gram_ctc_nbest_forward(_lib.stream(), _lib.ptr(xs), _lib.ptr(hyps), _lib.ptr(hyp_lengths),
                                                _lib.ptr(input_length), _lib.ptr(gram), T, B, V, N, Lmax, int(blank), _lib.ptr(logp),
                                                _lib.ptr(ws), nbytes)
            _lib.check(rc, "asr_gram_ctc_nbest_forward")
        ctx.save_for_backward(xs, input_length, ws)
        ctx.dims = (T, B, V, N, Lmax, nbytes, gram is not None)
        return logp

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.lib()
        xs, input_length, ws = ctx.saved_tensors
        T, B, V, N, Lmax, nbytes, is_gram = ctx.dims
        gy = gy.contiguous().to(torch.float32)
        # an ordinary (T, B, V) gradient: logits that come straight out of a LayerNormalization receive it through autograd beside
        # the recipe a CTC loss on the same logits may have left there (functions._CtcBox), and the normalisation adds the two
        grad = torch.empty_like(xs)
        name = "asr_gram_ctc_nbest_backward" if is_gram else "asr_ctc_nbest_backward"
        rc = getattr(lib, name)(_lib.stream(), _lib.ptr(xs), _lib.ptr(input_length), T, B, V, N, Lmax, _lib.ptr(gy),
                                _lib.ptr(grad), _lib.ptr(ws), nbytes)
        _lib.check(rc, name)
        return grad, None, None, None, None, None


def ctc_nbest_logp(x, hyps, hyp_lengths, blank_symbol, input_length=None):
    """Exact CTC log-probabilities of N labellings per utterance: ``x`` as ``connectionist_temporal_classification`` takes it
    ((T, B, V) float32 logits or the tuple of T views), ``hyps`` (B, N, L) int32, ``hyp_lengths`` (B, N) int32 -> (B, N) float32
    log p(h_n | x_b), differentiable with respect to ``x``.  A negative length marks an unused slot (log p = -inf); length 0 is
    the empty labelling; a labelling that does not fit into the utterance's frames has log p = -inf.  Slots with -inf send no
    gradient, whatever gradient arrives for them.  For N = 1 this is minus the CTC loss with ``reduce="no"``.
    ``asr.error.beam_decode``'s ids and lengths (unused slots set to -1) can be passed as they come."""
    xs = _check_common(x, blank_symbol, "no")
    return _NbestFunction.apply(xs, hyps, hyp_lengths, input_length, blank_symbol, None)


def _checked_gram_table(xs, gram, blank_symbol):
    """`gram` through ``asr.error._gram_table`` (validated on the host, -> (V, 2) int32 on the logits' device) and one more
    check: every character a bigram row spells with has a unigram row.  A string over such a table never meets a character it
    cannot emit alone, which is the only lattice the kernels (and the float64 oracle) model."""
    from ..error import _gram_table
    table = _gram_table(gram, xs.shape[2], blank_symbol, xs.device)
    g = gram.cpu().numpy() if isinstance(gram, torch.Tensor) else np.asarray(gram)
    unigrams = g[(g[:, 0] >= 0) & (g[:, 1] < 0), 0]
    spelled = g[g[:, 1] >= 0].reshape(-1)
    missing = np.setdiff1d(spelled, unigrams)
    if len(missing):
        raise ValueError("gram has bigram rows that spell with %s, which no unigram row spells" % missing[:8].tolist())
    return table


def gram_ctc_nbest_logp(x, hyps, hyp_lengths, gram, blank_symbol, input_length=None):
    """Exact Gram-CTC log-probabilities of N strings per utterance: ``x`` and the hypotheses as ``ctc_nbest_logp`` takes them, with
    ``hyps`` (B, N, L) int32 in characters (unigram ids), and ``gram`` the (V, 2) table of ``asr.vocab.gram_table`` (NumPy or a
    device tensor, validated on the host as ``asr.error.gram_beam_decode`` validates it; every character a bigram row spells with
    must have a unigram row, else ValueError) -> (B, N) float32 log p(string_n | x_b), differentiable with respect to ``x``.
    log p sums every way of cutting the string into unigram and bigram tokens of the table: it is minus ``gram_ctc`` with
    label_unigram[i] = the token of (s[i]) and label_bigram[i] = the token of (s[i-1], s[i]) or -1, reduce="no".
    A negative length marks an unused slot (log p = -inf); length 0 is the empty string; a string that does not fit into the
    utterance's frames, or holds a character without a unigram token, has log p = -inf.  Slots with -inf send no gradient.
    ``asr.error.gram_beam_decode``'s / ``gram_beam_decode_lm``'s ids and lengths (unused slots set to -1) can be passed as they
    come.  There is no CPU path."""
    xs = _check_common(x, blank_symbol, "no")
    return _NbestFunction.apply(xs, hyps, hyp_lengths, input_length, blank_symbol, _checked_gram_table(xs, gram, blank_symbol))


MWER = collections.namedtuple("MWER", "loss logp errors posteriors hyps hyp_lengths")
MWER.__doc__ = """Result of ``mwer_loss``: loss (scalar, or (B) with reduce="no") carries the graph; the rest are detached device
tensors over the hypothesis slots: logp (B, N) f32 exact log p(h_n | x), errors (B, N) f32 edit distance to the transcript (divided
by its length with normalize), posteriors (B, N) f32 the distribution over the valid slots (0 elsewhere), hyps (B, N, L) /
hyp_lengths (B, N) int32 the set itself (-1: unused), ready to be passed back in.  sum(posteriors * errors, 1) is the expected error."""


class _MwerParts(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, errors):
        valid = logp > float("-inf")
        zero = torch.zeros_like(logp)
        m = torch.where(valid, logp, torch.full_like(logp, float("-inf"))).max(dim=1, keepdim=True).values
        m = torch.where(m > float("-inf"), m, torch.zeros_like(m))
        z = torch.where(valid, torch.exp(torch.where(valid, logp, m.expand_as(logp)) - m), zero)
        post = z / z.sum(dim=1, keepdim=True).clamp_min(1e-30)
        e = torch.where(valid, errors.to(logp.dtype), zero)
        ebar = e.sum(dim=1, keepdim=True) / valid.sum(dim=1, keepdim=True).clamp_min(1).to(logp.dtype)
        ctx.save_for_backward(post, e)
        ctx.mark_non_differentiable(post)
        return (post * torch.where(valid, e - ebar, zero)).sum(dim=1), post

    @staticmethod
    def backward(ctx, g_loss, _g_post):
        post, e = ctx.saved_tensors
        # P_n (e_n - sum_m P_m e_m) written as P_n sum_m P_m (e_n - e_m): when one hypothesis holds nearly all the mass the first form
        # subtracts two nearly equal numbers and loses the coefficient of exactly that hypothesis; the second has no cancellation
        coef = post * ((e[:, :, None] - e[:, None, :]) * post[:, None, :]).sum(dim=2)
        return g_loss[:, None] * coef, None


def mwer_parts(logp, errors):
    """The (B, N) arithmetic of ``mwer_loss`` on any device and float type: over the slots with a finite logp,
    posteriors = softmax(logp), loss_b = sum_n posteriors_n (errors_n - mean errors).  -> (loss_b (B), posteriors (B, N));
    d loss_b / d logp_n = P_n (e_n - sum_m P_m e_m) flows to ``logp``, the posteriors carry no graph.
    Slots with logp = -inf get posterior 0 and no gradient; a row without a valid slot gives loss 0.  Never NaN."""
    return _MwerParts.apply(logp, errors)


def mwer_loss(x, t, blank_symbol, input_length=None, label_length=None, beam_width=8, top_k=8, min_logp=None, hyps=None,
              hyp_lengths=None, add_reference=False, normalize=False, max_length=None, reduce="mean"):
    """Expected number of errors over an N-best list (MWER): with e_n the Levenshtein distance of hypothesis n to the
    transcript ``t`` (B, L) int32 / ``label_length`` (divided by max(1, len) with ``normalize``), over the slots S_b that are in
    use and have a path,

        P_n = softmax_{n in S_b}(log p(h_n | x_b)),   loss_b = sum_n P_n (e_n - mean_{S_b} e),

    so that d loss_b / d log p_n = P_n (e_n - sum_m P_m e_m); ``reduce`` "mean" averages over the batch, "no" returns (B).
    log p is exact (``ctc_nbest_logp``); its gradient reaches ``x`` in one (T, B, V) pass whatever N is.

    Without ``hyps`` the list is ``asr.error.beam_decode(x.detach(), beam_width, top_k, blank_symbol, input_length, min_logp)``;
    its unused slots become length -1 and its T-wide ids are cut to the longest hypothesis, which costs ONE host
    synchronisation; with ``max_length`` given there is none: ids are cut there and longer hypotheses are dropped (unused).
    With ``hyps`` (B, N, L) / ``hyp_lengths`` (B, N) int32 given (-1: unused) no search runs.
    ``add_reference`` appends the transcript as one more slot unless a slot in use already equals it (then the appended slot is
    unused: the reference's probability is never counted twice).
    Returns an ``MWER`` namedtuple.  The usual training criterion interpolates with the CTC loss on the same logits:

        mwer = mwer_loss(ys, t, 0, x_len, t_len, beam_width=8)
        loss = mwer.loss + lam * connectionist_temporal_classification(ys, t, 0, x_len, t_len)
    """
    from ..error import beam_decode
    xs = _check_common(x, blank_symbol, reduce)
    if hyps is None:
        ids, lens, scores = beam_decode(xs.detach(), beam_width, top_k, blank_symbol, input_length, min_logp)
        hyps, hyp_lengths = _cut_list(ids, lens, scores, max_length)
    return _mwer_over_list(xs, t, blank_symbol, input_length, label_length, hyps, hyp_lengths, add_reference, normalize, reduce,
                           ctc_nbest_logp)


def _cut_list(ids, lens, scores, max_length):
    """a beam's N-best as a hypothesis set: unused slots (score -inf) get length -1, the ids are cut to the longest hypothesis
    (ONE host synchronisation) or, with ``max_length``, there (none; longer hypotheses become unused)"""
    lens = torch.where(scores > float("-inf"), lens, torch.full_like(lens, -1))
    if max_length is None:
        width = max(1, int(lens.max().item()))          # the one host synchronisation
    else:
        width = max(1, min(int(max_length), ids.shape[2]))
        lens = torch.where(lens > width, torch.full_like(lens, -1), lens)
    return ids[:, :, :width].contiguous(), lens


def _mwer_over_list(xs, t, blank_symbol, input_length, label_length, hyps, hyp_lengths, add_reference, normalize, reduce, logp_fn):
    """what ``mwer_loss`` and ``gram_mwer_loss`` do once the hypothesis set is there; ``logp_fn(xs, hyps, hyp_lengths, blank_symbol,
    input_length)`` scores it"""
    from .. import _ops
    T, B, V = xs.shape
    dev = xs.device
    if t.dtype != torch.int32 or (label_length is not None and label_length.dtype != torch.int32):
        raise TypeError("labels and lengths must be int32")
    if t.dim() != 2 or t.shape[0] != B:
        raise ValueError("t must be (B, L)")
    if label_length is None:
        label_length = torch.full((B,), t.shape[1], dtype=torch.int32, device=dev)
    if hyp_lengths is None:
        raise ValueError("hyp_lengths must be given with hyps")
    if hyps.dtype != torch.int32 or hyp_lengths.dtype != torch.int32:
        raise TypeError("labels and lengths must be int32")
    if hyps.dim() != 3 or hyps.shape[0] != B or tuple(hyp_lengths.shape) != tuple(hyps.shape[:2]):
        raise ValueError("hyps must be (B, N, L) and hyp_lengths (B, N)")
    if hyps.shape[2] == 0:
        hyps = torch.full((B, hyps.shape[1], 1), int(blank_symbol), dtype=torch.int32, device=dev)
    N = hyps.shape[1]

    def distances(h, hl):           # (B, n, L), (B, n) -> (B, n) f32 Levenshtein distance to the transcript, on the device
        n = h.shape[1]
        ref = t.repeat_interleave(n, dim=0).contiguous()
        ref_len = label_length.repeat_interleave(n).contiguous()
        if ref.shape[1] == 0:
            ref = torch.full((B * n, 1), int(blank_symbol), dtype=torch.int32, device=dev)
        d = _ops.edit_distance(ref, ref_len, h.reshape(B * n, h.shape[2]).contiguous(), hl.clamp_min(0).reshape(B * n).contiguous())
        return d.reshape(B, n).to(torch.float32)

    errors = distances(hyps, hyp_lengths)
    if add_reference:
        listed = ((errors == 0) & (hyp_lengths >= 0)).any(dim=1)
        W = max(hyps.shape[2], t.shape[1])
        both = torch.full((B, N + 1, W), int(blank_symbol), dtype=torch.int32, device=dev)
        both[:, :N, :hyps.shape[2]] = hyps
        both[:, N, :t.shape[1]] = t
        hyps = both
        hyp_lengths = torch.cat([hyp_lengths, torch.where(listed, torch.full_like(label_length, -1), label_length)[:, None]], dim=1)
        errors = torch.cat([errors, torch.zeros((B, 1), dtype=torch.float32, device=dev)], dim=1)
    if normalize:
        errors = errors / label_length.clamp_min(1).to(torch.float32)[:, None]
    logp = logp_fn(xs, hyps, hyp_lengths, blank_symbol, input_length)
    # float64 for the (B, N) part: the coefficients are products of posteriors that differ by many orders of magnitude
    loss_b, post = mwer_parts(logp.double(), errors.double())
    loss_b = loss_b.to(torch.float32)
    loss = loss_b.mean() if reduce == "mean" else loss_b
    return MWER(loss, logp.detach(), errors, post.to(torch.float32), hyps, hyp_lengths)


def gram_mwer_loss(x, t, gram, blank_symbol, input_length=None, label_length=None, beam_width=8, top_k=8, min_logp=None, hyps=None,
                   hyp_lengths=None, add_reference=False, normalize=False, max_length=None, reduce="mean", lm=None, lm_weight=0.0,
                   length_bonus=0.0, use_eos=True):
    """``mwer_loss`` for a Gram-CTC model: the transcript ``t`` (B, L) int32 and the hypotheses are strings of characters (unigram
    ids), e_n is the Levenshtein distance over characters, and log p(string_n | x_b) is exact under Gram-CTC
    (``gram_ctc_nbest_logp`` with the table ``gram``).  Everything else -- P_n, loss_b, ``add_reference``, ``normalize``,
    ``reduce``, the returned ``MWER`` -- is ``mwer_loss``'s.

    Without ``hyps`` the list is ``asr.error.gram_beam_decode(x.detach(), gram, beam_width, top_k, blank_symbol, input_length,
    min_logp)``, or with ``lm`` (an ``asr.lm.NGramLM`` over the characters) ``gram_beam_decode_lm(..., lm, lm_weight, length_bonus,
    ..., use_eos)``: the language model chooses the list, the criterion stays the acoustic model's expected error.  Its 2T-wide
    ids are cut as ``mwer_loss`` cuts them (one host synchronisation, none with ``max_length``).  The usual training criterion:

        mwer = gram_mwer_loss(ys, t, gram, 0, x_len, t_len, beam_width=8)
        loss = mwer.loss + lam * gram_ctc(ys, label_unigram, label_bigram, 0, x_len, t_len)
    """
    from ..error import gram_beam_decode, gram_beam_decode_lm
    xs = _check_common(x, blank_symbol, reduce)
    table = _checked_gram_table(xs, gram, blank_symbol)
    if hyps is None:
        if lm is None:
            ids, lens, scores = gram_beam_decode(xs.detach(), gram, beam_width, top_k, blank_symbol, input_length, min_logp)
        else:
            ids, lens, scores = gram_beam_decode_lm(xs.detach(), gram, lm, lm_weight, length_bonus, beam_width, top_k, blank_symbol,
                                                    input_length, min_logp, use_eos)[:3]
        hyps, hyp_lengths = _cut_list(ids, lens, scores, max_length)

    def logp_fn(xs, hyps, hyp_lengths, blank_symbol, input_length):
        return _NbestFunction.apply(xs, hyps, hyp_lengths, input_length, blank_symbol, table)
    return _mwer_over_list(xs, t, blank_symbol, input_length, label_length, hyps, hyp_lengths, add_reference, normalize, reduce,
                           logp_fn)
