"""Sequence-level criteria over a set of hypotheses per utterance, on the HIP path.

``ctc_nbest_logp`` gives the exact log p(h_n | x_b) of N labellings per utterance under CTC -- every path, not the lower
bound ``asr.error.beam_decode`` reports for what its beam kept -- and lets the gradient flow back into the logits.
``mwer_loss`` is the expected number of errors (minimum word error rate training, Prabhavalkar et al. 2018) over such a set.
The reference has neither; its only sequence criterion is the CTC / Gram-CTC loss.

The N hypotheses of an utterance share its logit rows: the kernels (csrc/ctc_nbest.hip) read the (T, B, V) logits once and
write one (T, B, V) gradient, whatever N is; only the lattices are per hypothesis.
"""
import collections

import torch

from .. import _lib
from .ctc import _check_common


class _NbestFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xs, hyps, hyp_lengths, input_length, blank):
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
        nbytes = lib.asr_ctc_nbest_workspace_bytes(T, B, V, N, Lmax)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=xs.device)
        logp = torch.empty((B, N), dtype=torch.float32, device=xs.device)
        rc = lib.asr_ctc_nbest_forward(_lib.stream(), _lib.ptr(xs), _lib.ptr(hyps), _lib.ptr(hyp_lengths), _lib.ptr(input_length),
                                       T, B, V, N, Lmax, int(blank), _lib.ptr(logp), _lib.ptr(ws), nbytes)
        _lib.check(rc, "asr_ctc_nbest_forward")
        ctx.save_for_backward(xs, input_length, ws)
        ctx.dims = (T, B, V, N, Lmax, nbytes)
        return logp

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.lib()
        xs, input_length, ws = ctx.saved_tensors
        T, B, V, N, Lmax, nbytes = ctx.dims
        gy = gy.contiguous().to(torch.float32)
        # an ordinary (T, B, V) gradient: logits that come straight out of a LayerNormalization receive it through autograd beside
        # the recipe a CTC loss on the same logits may have left there (functions._CtcBox), and the normalisation adds the two
        grad = torch.empty_like(xs)
        rc = lib.asr_ctc_nbest_backward(_lib.stream(), _lib.ptr(xs), _lib.ptr(input_length), T, B, V, N, Lmax, _lib.ptr(gy),
                                        _lib.ptr(grad), _lib.ptr(ws), nbytes)
        _lib.check(rc, "asr_ctc_nbest_backward")
        return grad, None, None, None, None


def ctc_nbest_logp(x, hyps, hyp_lengths, blank_symbol, input_length=None):
    """Exact CTC log-probabilities of N labellings per utterance: ``x`` as ``connectionist_temporal_classification`` takes it
    ((T, B, V) float32 logits or the tuple of T views), ``hyps`` (B, N, L) int32, ``hyp_lengths`` (B, N) int32 -> (B, N) float32
    log p(h_n | x_b), differentiable with respect to ``x``.  A negative length marks an unused slot (log p = -inf); length 0 is
    the empty labelling; a labelling that does not fit into the utterance's frames has log p = -inf.  Slots with -inf send no
    gradient, whatever gradient arrives for them.  For N = 1 this is minus the CTC loss with ``reduce="no"``.
    ``asr.error.beam_decode``'s ids and lengths (unused slots set to -1) can be passed as they come."""
    xs = _check_common(x, blank_symbol, "no")
    return _NbestFunction.apply(xs, hyps, hyp_lengths, input_length, blank_symbol)


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
    from .. import _ops
    from ..error import beam_decode
    xs = _check_common(x, blank_symbol, reduce)
    T, B, V = xs.shape
    dev = xs.device
    if t.dtype != torch.int32 or (label_length is not None and label_length.dtype != torch.int32):
        raise TypeError("labels and lengths must be int32")
    if t.dim() != 2 or t.shape[0] != B:
        raise ValueError("t must be (B, L)")
    if label_length is None:
        label_length = torch.full((B,), t.shape[1], dtype=torch.int32, device=dev)
    if hyps is None:
        ids, lens, scores = beam_decode(xs.detach(), beam_width, top_k, blank_symbol, input_length, min_logp)
        lens = torch.where(scores > float("-inf"), lens, torch.full_like(lens, -1))
        if max_length is None:
            width = max(1, int(lens.max().item()))          # the one host synchronisation
        else:
            width = max(1, min(int(max_length), T))
            lens = torch.where(lens > width, torch.full_like(lens, -1), lens)
        hyps, hyp_lengths = ids[:, :, :width].contiguous(), lens
    else:
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
    logp = ctc_nbest_logp(xs, hyps, hyp_lengths, blank_symbol, input_length)
    # float64 for the (B, N) part: the coefficients are products of posteriors that differ by many orders of magnitude
    loss_b, post = mwer_parts(logp.double(), errors.double())
    loss_b = loss_b.to(torch.float32)
    loss = loss_b.mean() if reduce == "mean" else loss_b
    return MWER(loss, logp.detach(), errors, post.to(torch.float32), hyps, hyp_lengths)
