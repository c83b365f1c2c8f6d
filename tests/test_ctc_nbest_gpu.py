"""N-best CTC scoring (asr.loss.ctc_nbest_logp, csrc/ctc_nbest.hip) and the MWER loss (asr.loss.mwer_loss) on the device against
the float64 restatement tests/ctc_nbest_reference.py.

Tolerances are tests/test_ctc_gpu.py's: logp rtol 1e-4 (LOSS_RTOL); a gradient sum_n gy_n g_n element-wise within
    1e-5 sum_n |gy[b, n]| + 1e-4 sum_n |gy[b, n] g_n|
i.e. that file's per-hypothesis bound (GRAD_ATOL, GRAD_RTOL = 1e-5, 1e-4) summed over the hypotheses of the utterance."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_reference as beam_ref
import ctc_nbest_reference as ref

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4
GRAD_ATOL, GRAD_RTOL = 1e-5, 1e-4


def _dev(device, *arrays):
    return [None if a is None else torch.tensor(a, device=device) for a in arrays]


def _grad_bound(gy_abs_sum, mag):
    """gy_abs_sum (B): sum_n |gy[b, n]| over the live slots; mag (T, B, V): sum_n |gy[b, n] g_n|"""
    return GRAD_ATOL * gy_abs_sum[None, :, None] + GRAD_RTOL * mag


# ---------------------------------------------------------------------------------------------- 1. N = 1 is the loss
@pytest.mark.parametrize("T,B,V,L", [(50, 3, 7, 5), (64, 2, 8200, 9), (700, 1, 37, 600)])
def test_one_hypothesis_equals_the_ctc_loss(device, T, B, V, L):
    """against the device's own connectionist_temporal_classification(reduce="no"): logp = -loss, and the gradient with gy = -w
    is the loss's gradient with gy = w.  1e-5 relative as tests/test_ctc_gpu.py compares its own paths: the loss values
    element-wise, the gradients relative to the largest entry (both kernels scatter the occupancy with float atomics, whose order
    is not fixed, so entries where softmax and occupancy cancel have no element-wise relative bound even between two runs).
    L = 600: 1201 path nodes, the sweep with several nodes per thread as csrc/ctc_nbest.hip launches it (the loss's own long
    transcripts are compared with the oracle in tests/test_ctc_edges_gpu.py)"""
    from asr.loss import connectionist_temporal_classification, ctc_nbest_logp
    rs = np.random.RandomState(T + V)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    lab = rs.randint(1, min(V, 119), size=(B, L)).astype(np.int32)
    lab[:, 2] = lab[:, 1]
    tl = rs.randint(max(1, L // 2), L + 1, size=B).astype(np.int32)
    tl[0] = L
    xl = rs.randint(min(3 * L, T), T + 1, size=B).astype(np.int32)
    xl[0] = T
    w = rs.rand(B).astype(np.float32) + 0.5
    d_lab, d_tl, d_xl, d_w = _dev(device, lab, tl, xl, w)
    x1 = torch.tensor(xs, device=device, requires_grad=True)
    loss = connectionist_temporal_classification(x1, d_lab, 0, d_xl, d_tl, "no")
    loss.backward(d_w)
    x2 = torch.tensor(xs, device=device, requires_grad=True)
    logp = ctc_nbest_logp(x2, d_lab[:, None, :], d_tl[:, None], 0, d_xl)
    assert logp.shape == (B, 1) and logp.dtype == torch.float32
    logp.backward(-d_w[:, None])
    np.testing.assert_allclose(logp[:, 0].detach().cpu().numpy(), -loss.detach().cpu().numpy(), rtol=1e-5)
    g1, g2 = x1.grad.cpu().numpy(), x2.grad.cpu().numpy()
    print("N=1 (T,B,V,L)=%s: max |dgrad| / max |grad| = %.3g" % ((T, B, V, L), np.abs(g1 - g2).max() / np.abs(g1).max()))
    assert np.abs(g1 - g2).max() <= 1e-5 * np.abs(g1).max()


# ---------------------------------------------------------------------------------------------- 2. random cases
CASES = [(50, 3, 7, 3, 5), (120, 2, 119, 5, 20), (200, 2, 3001, 4, 33), (64, 2, 8200, 2, 9)]


@functools.lru_cache(maxsize=None)
def _case(T, B, V, N, L):
    """inputs and the float64 reference of one random case, computed once and shared (treat as read-only)"""
    xs, hyps, hyp_len, x_len, gy, dead = ref.random_case(T, B, V, N, L, seed=T + V + N)
    logp, grads = ref.nbest_logp_grad(xs, hyps, hyp_len, x_len)
    return xs, hyps, hyp_len, x_len, gy, dead, logp, grads


def _check_logp_and_grad(got_logp, got_grad, case, T, B, V, N, tag):
    xs, hyps, hyp_len, x_len, gy, dead, logp, grads = case
    assert np.array_equal(np.isneginf(got_logp), dead), (got_logp, dead)
    assert np.array_equal(~np.isfinite(logp), dead)
    np.testing.assert_allclose(got_logp[~dead], logp[~dead], rtol=LOSS_RTOL)
    assert np.isfinite(got_grad).all()
    for b in range(B):
        assert not got_grad[x_len[b]:, b].any()
    gy0 = np.where(dead, 0.0, gy).astype(np.float64)
    want, mag = ref.weighted_grad(grads, gy0, B, N, T, V)
    bound = _grad_bound(np.abs(gy0).sum(axis=1), mag)
    err = np.abs(got_grad - want)
    print("%s: worst |dlogp| / |logp| = %.3g, worst |dgrad| / bound = %.3g" %
          (tag, np.abs(got_logp[~dead] - logp[~dead]).max() / np.abs(logp[~dead]).min(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()


@pytest.mark.parametrize("T,B,V,N,L", CASES)
def test_random_cases_against_the_restatement(device, T, B, V, N, L):
    """ragged x_len and hyp_len, a repeat in every hypothesis, an empty, an unused and an infeasible slot, NaN in gy where logp
    is -inf: logp -inf exactly there, the gradient finite, exactly 0 beyond x_len, and inside the derived bound everywhere"""
    from asr.loss import ctc_nbest_logp
    case = _case(T, B, V, N, L)
    xs, hyps, hyp_len, x_len, gy = case[:5]
    d_h, d_hl, d_xl, d_gy = _dev(device, hyps, hyp_len, x_len, gy)
    x = torch.tensor(xs, device=device, requires_grad=True)
    logp = ctc_nbest_logp(x, d_h, d_hl, 0, d_xl)
    logp.backward(d_gy)
    _check_logp_and_grad(logp.detach().cpu().numpy(), x.grad.cpu().numpy(), case, T, B, V, N, "random %s" % ((T, B, V, N, L),))


# ---------------------------------------------------------------------------------------------- 3. tuple of views
def test_tuple_of_views_input(device):
    from asr.loss import ctc_nbest_logp
    T, B, V, N, L = CASES[0]
    xs, hyps, hyp_len, x_len, gy = _case(T, B, V, N, L)[:5]
    d_h, d_hl, d_xl, d_gy = _dev(device, hyps, hyp_len, x_len, gy)
    out = []
    for as_tuple in (False, True):
        x = torch.tensor(xs, device=device, requires_grad=True)
        logp = ctc_nbest_logp(tuple(x.unbind(0)) if as_tuple else x, d_h, d_hl, 0, d_xl)
        logp.backward(d_gy)
        out.append((logp.detach().cpu().numpy(), x.grad.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.abs(out[1][1] - out[0][1]).max() <= 1e-5 * np.abs(out[0][1]).max()      # (float atomics: the order of the adds is not fixed)


# ---------------------------------------------------------------------------------------------- 4. mwer_loss on given hypotheses
@pytest.mark.parametrize("reduce", ["mean", "no"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("T,B,V,N,L", CASES[:2])
def test_mwer_loss_with_given_hypotheses(device, T, B, V, N, L, normalize, reduce):
    """in three steps, so that the softmax's amplification of the logp error stays out of the tolerances: (a) the returned logp
    against the restatement; (b) with the device's own logp in float64, loss and posteriors against the float64 formula;
    (c) x.grad = sum_n c_n g_n with c_n from (b) and g_n from the restatement, inside the derived gradient bound"""
    from asr.loss import mwer_loss
    xs, hyps, hyp_len, x_len, _, dead, logp, grads = _case(T, B, V, N, L)
    rs = np.random.RandomState(N + L)
    t = rs.randint(1, min(V, 119), size=(B, L + 2)).astype(np.int32)
    t_len = rs.randint(1, L + 3, size=B).astype(np.int32)
    t[0, :L], t_len[0] = hyps[0, 0], L                 # one hypothesis is its utterance's transcript: e = 0
    d_h, d_hl, d_xl, d_t, d_tl = _dev(device, hyps, hyp_len, x_len, t, t_len)
    x = torch.tensor(xs, device=device, requires_grad=True)
    res = mwer_loss(x, d_t, 0, d_xl, d_tl, hyps=d_h, hyp_lengths=d_hl, normalize=normalize, reduce=reduce)
    w = np.ones(B) / B if reduce == "mean" else rs.rand(B) + 0.5
    if reduce == "mean":
        assert res.loss.shape == ()
        res.loss.backward()
    else:
        assert res.loss.shape == (B,)
        res.loss.backward(torch.tensor(w.astype(np.float32), device=device))
        w = w.astype(np.float32).astype(np.float64)
    assert torch.equal(res.hyps, d_h) and torch.equal(res.hyp_lengths, d_hl)
    # (a)
    got_logp = res.logp.cpu().numpy()
    assert np.array_equal(np.isneginf(got_logp), dead)
    np.testing.assert_allclose(got_logp[~dead], logp[~dead], rtol=LOSS_RTOL)
    # (b)
    e = ref.errors(hyps, hyp_len, t, t_len, normalize)
    np.testing.assert_allclose(res.errors.cpu().numpy(), e, rtol=1e-6)
    loss_b, post, coef, spread = ref.mwer(got_logp.astype(np.float64), e)
    got_loss = res.loss.detach().cpu().numpy().astype(np.float64)
    if reduce == "mean":
        assert abs(got_loss - loss_b.mean()) <= 1e-5 * spread.mean(), (got_loss, loss_b.mean())
    else:
        assert (np.abs(got_loss - loss_b) <= 1e-5 * spread).all(), (got_loss, loss_b)
    assert np.abs(res.posteriors.cpu().numpy() - post).max() <= 1e-5
    assert np.isfinite(got_loss).all()
    # (c)
    c = coef * w[:, None]
    want, mag = ref.weighted_grad(grads, c, B, N, T, V)
    bound = _grad_bound(np.abs(c).sum(axis=1), mag)
    gr = x.grad.cpu().numpy()
    assert np.isfinite(gr).all()
    err = np.abs(gr - want)
    print("mwer %s %s normalize=%s: worst |dgrad| / bound = %.3g" % ((T, B, V, N, L), reduce, normalize, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()


# ---------------------------------------------------------------------------------------------- 5. mwer_loss with its own beam
def _peaky_batch(T, B, V, seed):
    rs = np.random.RandomState(seed)
    xs = np.stack([beam_ref.peaky(rs, T, V) for _ in range(B)], axis=1)
    return xs.astype(np.float32)


def test_mwer_loss_end_to_end_with_its_own_beam(device):
    from asr.error import beam_decode
    from asr.loss import mwer_loss
    T, B, V, W = 60, 3, 30, 4
    xs = _peaky_batch(T, B, V, seed=7)
    x_len = np.array([T, T - 7, T - 19], np.int32)
    d_xl, = _dev(device, x_len)
    x0 = torch.tensor(xs, device=device)
    ids, lens, scores = beam_decode(x0, W, W, 0, d_xl)
    lens_h, ids_h = lens.cpu().numpy(), ids.cpu().numpy()
    # transcripts: utterance 0's is its best hypothesis (already listed), the others' are not in their lists
    Lt = int(lens_h.max()) + 2
    t = np.zeros((B, Lt), np.int32)
    t_len = np.zeros(B, np.int32)
    t[0, :lens_h[0, 0]], t_len[0] = ids_h[0, 0, :lens_h[0, 0]], lens_h[0, 0]
    for b in (1, 2):
        n = lens_h[b, 0]
        t[b, :n], t_len[b] = ids_h[b, 0, :n], n + 1
        t[b, n] = 1 + (ids_h[b, 0, max(n - 1, 0)] % (V - 2))         # one more token, different from its neighbour
    d_t, d_tl = _dev(device, t, t_len)

    def run(**kw):
        x = x0.clone().requires_grad_(True)
        r = mwer_loss(x, d_t, 0, d_xl, d_tl, beam_width=W, top_k=W, **kw)
        r.loss.sum().backward()
        return r, x.grad
    r1, g1 = run()
    width = max(1, int(lens_h.max()))
    want_len = np.where(np.isneginf(scores.cpu().numpy()), -1, lens_h)
    assert np.array_equal(r1.hyps.cpu().numpy(), ids_h[:, :, :width]) and np.array_equal(r1.hyp_lengths.cpu().numpy(), want_len)
    assert torch.isfinite(r1.loss) and torch.isfinite(g1).all()
    # exact log p cannot be below what the beam kept of it
    sc = scores.cpu().numpy()
    used = want_len >= 0
    assert (r1.logp.cpu().numpy()[used] >= sc[used] - 1e-4 * np.abs(sc[used])).all()
    r2, g2 = run(hyps=r1.hyps, hyp_lengths=r1.hyp_lengths)
    assert torch.equal(r1.logp, r2.logp) and abs(r1.loss.item() - r2.loss.item()) <= 1e-6 * abs(r1.loss.item()) + 1e-9
    assert float((g1 - g2).abs().max()) <= 1e-5 * float(g1.abs().max())
    # max_length: no synchronisation, longer hypotheses dropped
    r3, _ = run(max_length=width)
    assert torch.equal(r3.hyps, r1.hyps) and torch.equal(r3.hyp_lengths, r1.hyp_lengths)
    r4, _ = run(max_length=width - 1)
    assert r4.hyps.shape[2] == width - 1
    assert np.array_equal(r4.hyp_lengths.cpu().numpy(), np.where(want_len > width - 1, -1, want_len))
    # add_reference
    ra, ga = run(add_reference=True)
    la, ha = ra.hyp_lengths.cpu().numpy(), ra.hyps.cpu().numpy()
    h_ref, l_ref = ref.with_reference(ids_h[:, :, :width], want_len.astype(np.int32), t, t_len)
    assert l_ref[0, W] == -1 and (l_ref[1:, W] == t_len[1:]).all()          # (what this test's transcripts were made for)
    assert la.shape == (B, W + 1) and np.array_equal(la, l_ref)
    assert np.array_equal(la[:, :W], want_len) and np.array_equal(ha[:, :W, :width], ids_h[:, :, :width])
    for b in (1, 2):
        assert np.array_equal(ha[b, W, :t_len[b]], t[b, :t_len[b]])
    # utterance 0 lists its transcript: with and without the appended slot it is the same problem
    rn, gn = run(reduce="no")
    rna, gna = run(add_reference=True, reduce="no")
    assert abs(rn.loss[0].item() - rna.loss[0].item()) <= 1e-6 * abs(rn.loss[0].item()) + 1e-9
    assert rna.posteriors[0, W].item() == 0.0 and torch.isneginf(rna.logp[0, W])
    assert torch.equal(rn.logp[0], rna.logp[0, :W])
    # the others: the reference's slot is there and its posterior is the restatement's
    logp64 = ref.nbest_logp_grad(xs, h_ref, l_ref, x_len, want_grad=False)
    got = ra.logp.cpu().numpy()
    assert np.array_equal(np.isfinite(got), np.isfinite(logp64))
    np.testing.assert_allclose(got[np.isfinite(got)], logp64[np.isfinite(got)], rtol=LOSS_RTOL)
    _, post, _, _ = ref.mwer(got.astype(np.float64), ref.errors(h_ref, l_ref, t, t_len))
    assert np.abs(ra.posteriors.cpu().numpy() - post).max() <= 1e-5
    assert (post[1:, W] > 0).all() and (ra.posteriors[1:, W] > 0).all()
    assert (ra.errors.cpu().numpy()[1:, W] == 0).all()


# ---------------------------------------------------------------------------------------------- 6. LayerNorm interplay
def test_mwer_plus_ctc_on_layernorm_logits_fused_equals_unfused(device):
    """logits straight out of a per-frame LayerNormalization (tests/test_ctc_gpu.py: _ln_ctc_case): the CTC loss leaves its
    recipe at the normalisation, mwer_loss sends an ordinary gradient through autograd, and the normalisation adds the two;
    with FUSE_CTC_INTO_LAYERNORM off both arrive through autograd.  Same dx / dgamma, to the tolerances of
    test_layernorm_ctc_fusion_with_another_consumer_of_the_logits"""
    from asr import functions as F, _ops
    from asr.link import Parameter
    from asr.loss import connectionist_temporal_classification, mwer_loss
    rs = np.random.RandomState(11)
    T, B, V, L, N = 30, 2, 36, 4, 3
    x0 = torch.tensor((rs.randn(T * B, V) * 2.0 + 0.3).astype(np.float32)).to(device)
    g0 = torch.tensor(rs.uniform(0.5, 1.5, V).astype(np.float32))
    b0 = torch.tensor((rs.randn(V) * 0.2).astype(np.float32))
    uni, = _dev(device, rs.randint(1, V, size=(B, L)).astype(np.int32))
    hyps = rs.randint(1, V, size=(B, N, L)).astype(np.int32)
    hyps[:, 0] = uni.cpu().numpy()
    hyp_len = np.array([[L, L - 1, 0], [L, -1, L - 2]], np.int32)
    d_h, d_hl = _dev(device, hyps, hyp_len)

    def run(fused):
        F.FUSE_CTC_INTO_LAYERNORM[0] = fused
        try:
            x = x0.clone().requires_grad_(True)
            gamma, beta = Parameter(g0.clone().to(device)), Parameter(b0.clone().to(device))
            y = F.layer_normalization(x.reshape(T, B, 1, V).permute(1, 3, 2, 0), gamma, beta, out_f32=True)
            tbv = y.permute(3, 0, 2, 1).squeeze(2)
            before = _ops.CALLS.get("layernorm_ctc_bwd", 0)
            m = mwer_loss(tbv, uni, 0, hyps=d_h, hyp_lengths=d_hl)
            total = m.loss + 0.3 * connectionist_temporal_classification(tbv, uni, 0)
            total.backward()
            torch.cuda.synchronize()
            assert _ops.CALLS.get("layernorm_ctc_bwd", 0) - before == (1 if fused else 0)
            return total.item(), x.grad.clone(), gamma.grad.clone()
        finally:
            F.FUSE_CTC_INTO_LAYERNORM[0] = True
    (lf, dxf, dgf), (lu, dxu, dgu) = run(True), run(False)
    assert abs(lf - lu) <= 1e-5 * abs(lu)
    assert float(dxu.abs().max()) > 0
    assert float((dxf - dxu).abs().max()) <= 1e-4 * float(dxu.abs().max())
    assert float((dgf - dgu).abs().max()) <= 1e-4 * float(dgu.abs().max()) + 1e-6


# ---------------------------------------------------------------------------------------------- 7. full size, once
def test_full_size_once(device):
    """B = 32, T = 1000, V = 3000, N = 16, hypotheses from beam_decode on peaked logits: column 0 against the device's CTC loss on
    the same labels; one utterance's 16 logp and its gradient rows against the restatement; every logp at or above its beam score"""
    from asr.error import beam_decode
    from asr.loss import connectionist_temporal_classification, ctc_nbest_logp
    T, B, V, N = 1000, 32, 3000, 16
    xs = _peaky_batch(T, B, V, seed=3)
    rs = np.random.RandomState(4)
    x_len = rs.randint(600, T + 1, size=B).astype(np.int32)
    x_len[0] = T
    d_xl, = _dev(device, x_len)
    x = torch.tensor(xs, device=device, requires_grad=True)
    ids, lens, scores = beam_decode(x.detach(), N, 16, 0, d_xl)
    lens = torch.where(scores > float("-inf"), lens, torch.full_like(lens, -1))
    width = int(lens.max().item())
    hyps = ids[:, :, :width].contiguous()
    gy = torch.tensor(rs.randn(B, N).astype(np.float32), device=device)
    logp = ctc_nbest_logp(x, hyps, lens, 0, d_xl)
    logp.backward(gy)
    got, sc, lens_h = logp.detach().cpu().numpy(), scores.cpu().numpy(), lens.cpu().numpy()
    used = lens_h >= 0
    assert used[:, 0].all() and np.array_equal(np.isfinite(got), used)
    assert (got[used] >= sc[used] - 1e-4 * np.abs(sc[used])).all()
    loss = connectionist_temporal_classification(x.detach(), hyps[:, 0].contiguous(), 0, d_xl, lens[:, 0].contiguous(), "no")
    np.testing.assert_allclose(got[:, 0], -loss.cpu().numpy(), rtol=1e-5)
    gr = x.grad
    mask = (torch.arange(T)[:, None] < torch.tensor(x_len.astype(np.int64))[None, :])
    assert torch.isfinite(gr).all() and (gr.cpu()[~mask] == 0).all()
    b = 3
    hb, lb = hyps[b:b + 1].cpu().numpy(), lens_h[b:b + 1]
    logp64, grads = ref.nbest_logp_grad(xs[:, b:b + 1], hb, lb, x_len[b:b + 1])
    np.testing.assert_allclose(got[b][used[b]], logp64[0][used[b]], rtol=LOSS_RTOL)
    gyb = np.where(used[b], gy[b].cpu().numpy(), 0.0).astype(np.float64)[None, :]
    want, mag = ref.weighted_grad(grads, gyb, 1, N, T, V)
    err = np.abs(gr[:, b].cpu().numpy() - want[:, 0])
    bound = _grad_bound(np.abs(gyb).sum(axis=1), mag)[:, 0]
    print("full size: used slots %d of %d, width %d, worst |dgrad| / bound = %.3g" % (used.sum(), used.size, width, (err / bound).max()))
    assert (err <= bound).all(), (err / bound).max()


# ---------------------------------------------------------------------------------------------- 8. error codes
def test_error_codes(device):
    """N = 0, N = 129, a short workspace and a null pointer are refused before anything is launched (logp keeps its contents)"""
    from asr import _lib
    lib = _lib.lib()
    T, B, V, N, L = 20, 2, 9, 3, 4
    x = torch.randn(T, B, V, device=device)
    hyp = torch.ones((B, 129, L), dtype=torch.int32, device=device)
    hl = torch.full((B, 129), L, dtype=torch.int32, device=device)
    logp = torch.full((B, 129), 7.0, device=device)
    gy = torch.ones((B, 129), device=device)
    grad = torch.full((T, B, V), 7.0, device=device)
    nbytes = lib.asr_ctc_nbest_workspace_bytes(T, B, V, N, L)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    p, s = _lib.ptr, _lib.stream()
    BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3

    def fwd(n, xs=x, h=hyp, nb=nbytes, w=ws):
        return lib.asr_ctc_nbest_forward(s, p(xs), p(h), p(hl), None, T, B, V, n, L, 0, p(logp), p(w), nb)

    def bwd(n, g=gy, nb=nbytes, w=ws):
        return lib.asr_ctc_nbest_backward(s, p(x), None, T, B, V, n, L, p(g), p(grad), p(w), nb)
    assert fwd(0) == BAD_ARG and bwd(0) == BAD_ARG                      # not a count (as the beam refuses beam_width 0)
    assert fwd(129) == UNSUPPORTED and bwd(129) == UNSUPPORTED          # above the beam's limit
    assert fwd(N, nb=nbytes - 1) == WORKSPACE and bwd(N, nb=nbytes - 1) == WORKSPACE
    assert fwd(N, xs=None) == BAD_ARG and fwd(N, h=None) == BAD_ARG and fwd(N, w=None) == BAD_ARG
    assert bwd(N, g=None) == BAD_ARG and bwd(N, w=None) == BAD_ARG
    assert lib.asr_ctc_nbest_forward(s, p(x), p(hyp), p(hl), None, T, B, V, N, L, V, p(logp), p(ws), nbytes) == BAD_ARG   # blank
    assert lib.asr_ctc_nbest_forward(s, p(x), p(hyp), p(hl), None, T, B, V, N, 80000, 0, p(logp), p(ws), 1 << 62) == UNSUPPORTED  # LDS
    torch.cuda.synchronize()
    assert (logp == 7.0).all() and (grad == 7.0).all()
    with pytest.raises(TypeError):
        from asr.loss import ctc_nbest_logp
        ctc_nbest_logp(x, hyp[:, :N].long(), hl[:, :N], 0)
