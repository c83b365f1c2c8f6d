"""N-best Gram-CTC scoring (asr.loss.gram_ctc_nbest_logp, asr_gram_ctc_nbest_* in csrc/ctc_nbest.hip) and the string-level MWER
loss (asr.loss.gram_mwer_loss) on the device against the float64 restatement tests/gram_nbest_reference.py, the exhaustive
enumeration of tests/gram_beam_reference.py, the device's own Gram-CTC loss and the Gram-CTC beam search.

Tolerances are tests/test_ctc_nbest_gpu.py's (whose helpers this file uses): logp rtol 1e-4; a gradient sum_n gy_n g_n
element-wise within 1e-5 sum_n |gy[b, n]| + 1e-4 sum_n |gy[b, n] g_n|."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as lmref
import gram_beam_lm_reference as glm
import gram_beam_reference as gref
import gram_nbest_reference as ref
import test_gram_beam_gpu as gbase
from test_ctc_beam_gpu import tol
from test_ctc_nbest_gpu import LOSS_RTOL, _check_logp_and_grad, _dev, _grad_bound

pytestmark = pytest.mark.gpu


def _labels(chars, gram):
    """(B, L) characters -> gram_ctc's (label_unigram, label_bigram) with every bigram of the table offered"""
    uni = gref.unigram_ids(gram)
    lu = np.array([[uni[int(c)] for c in row] for row in chars], np.int32)
    lb = np.array([gref.label_bigrams([int(c) for c in row], gram) for row in chars], np.int32)
    return lu, lb


# ---------------------------------------------------------------------------------------------- 1. N = 1 is the loss
@pytest.mark.parametrize("T,B,U,G,L", [(50, 3, 3, 3, 5), (64, 2, 100, 8099, 9)])
def test_one_hypothesis_equals_the_gram_ctc_loss(device, T, B, U, G, L):
    """against the device's own gram_ctc(reduce="no") on the labels the string stands for, over a table whose unigram token ids
    differ from the characters they spell (the index is really used): logp = -loss to 1e-5, the gradients within 1e-5 of the
    largest entry (float atomics: tests/test_ctc_nbest_gpu.py::test_one_hypothesis_equals_the_ctc_loss)"""
    from asr.loss import gram_ctc, gram_ctc_nbest_logp
    gram = ref.shuffled_table(U, G, seed=T)
    V = len(gram)
    assert (T, B, V, L) in ((50, 3, 7, 5), (64, 2, 8200, 9))
    rs = np.random.RandomState(T + V)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    chars = rs.randint(1, U + 1, size=(B, L)).astype(np.int32)
    chars[:, 2] = chars[:, 1]
    chars[0, 3:5] = ref.table_pairs(gram)[0]
    lu, lb = _labels(chars, gram)
    assert (lb >= 0).any() and (lu != chars).any()
    tl = rs.randint(max(1, L // 2), L + 1, size=B).astype(np.int32)
    tl[0] = L
    xl = rs.randint(3 * L, T + 1, size=B).astype(np.int32)
    xl[0] = T
    w = rs.rand(B).astype(np.float32) + 0.5
    d_c, d_lu, d_lb, d_tl, d_xl, d_w = _dev(device, chars, lu, lb, tl, xl, w)
    x1 = torch.tensor(xs, device=device, requires_grad=True)
    loss = gram_ctc(x1, d_lu, d_lb, 0, d_xl, d_tl, "no")
    loss.backward(d_w)
    x2 = torch.tensor(xs, device=device, requires_grad=True)
    logp = gram_ctc_nbest_logp(x2, d_c[:, None, :], d_tl[:, None], gram, 0, d_xl)
    assert logp.shape == (B, 1) and logp.dtype == torch.float32
    logp.backward(-d_w[:, None])
    np.testing.assert_allclose(logp[:, 0].detach().cpu().numpy(), -loss.detach().cpu().numpy(), rtol=1e-5)
    g1, g2 = x1.grad.cpu().numpy(), x2.grad.cpu().numpy()
    print("N=1 (T,B,V,L)=%s: max |dgrad| / max |grad| = %.3g" % ((T, B, V, L), np.abs(g1 - g2).max() / np.abs(g1).max()))
    assert np.abs(g1 - g2).max() <= 1e-5 * np.abs(g1).max()


# ---------------------------------------------------------------------------------------------- 2. random cases
# (T, B, V, N, L): smallest; pruned_table(), Sp = 64; V not a multiple of 4, Sp = 128; V above the 8192-entry occupancy chunk;
# Sp = 320, wider than the 256 threads of the row kernels and not a power of two
CASES = [(50, 3, 7, 3, 5), (120, 2, 171, 5, 20), (200, 2, 3001, 4, 33), (64, 2, 8200, 2, 9), (200, 1, 171, 3, 90)]


@functools.lru_cache(maxsize=None)
def _table(V):
    gram = {7: lambda: ref.shuffled_table(3, 3, seed=7), 171: gref.pruned_table, 3001: lambda: ref.shuffled_table(60, 2940, seed=3001),
            8200: lambda: ref.shuffled_table(100, 8099, seed=8200)}[V]()
    assert len(gram) == V
    return gram


@functools.lru_cache(maxsize=None)
def _case(T, B, V, N, L):
    """inputs and the float64 reference of one random case, computed once and shared (treat as read-only); the layout of
    tests/test_ctc_nbest_gpu.py::_case, with NaN in gy wherever log p is -inf"""
    gram = _table(V)
    xs, hyps, hyp_len, x_len, gy = ref.random_case(T, B, N, L, gram, seed=T + V + N)
    logp, grads = ref.nbest_logp_grad(xs, hyps, hyp_len, gram, x_len)
    dead = ~np.isfinite(logp)
    assert np.isfinite(logp[0, 0]) and np.isfinite(logp[0, 1]) and dead.sum() >= (1 if B == 1 else 2 if N == 2 else 3)
    gy[dead] = np.nan
    return xs, hyps, hyp_len, x_len, gy, dead, logp, grads


@pytest.mark.parametrize("T,B,V,N,L", CASES)
def test_random_cases_against_the_restatement(device, T, B, V, N, L):
    """ragged x_len and hyp_len, a doubled character, an "abab" over a bigram of the table, a pair the table does not have, an
    empty, an unused and a too-long slot and one with a character outside the table (tests/gram_nbest_reference.py::random_case
    says which of them B * N has room for), NaN in gy where logp is -inf: logp -inf exactly there, the gradient finite, exactly 0
    beyond x_len, and inside the derived bound everywhere"""
    from asr.loss import gram_ctc_nbest_logp
    case = _case(T, B, V, N, L)
    xs, hyps, hyp_len, x_len, gy = case[:5]
    d_h, d_hl, d_xl, d_gy = _dev(device, hyps, hyp_len, x_len, gy)
    x = torch.tensor(xs, device=device, requires_grad=True)
    logp = gram_ctc_nbest_logp(x, d_h, d_hl, _table(V), 0, d_xl)
    logp.backward(d_gy)
    _check_logp_and_grad(logp.detach().cpu().numpy(), x.grad.cpu().numpy(), case, T, B, V, N, "gram random %s" % ((T, B, V, N, L),))


# ---------------------------------------------------------------------------------------------- 3. exhaustive
@pytest.mark.parametrize("case", gref.EXHAUSTIVE, ids=lambda c: "T%d_rows%d_s%d" % (c[0][0], len(c[0][1]), c[0][2]))
def test_exhaustive_against_the_enumeration(device, case):
    """every string with p > 0 (the empty one included) as the N <= 101 slots of one call"""
    from asr.loss import gram_ctc_nbest_logp
    (T, rows, seed), count = case
    gram = gref.table(rows)
    x = gref.exhaustive_logits(T, len(gram), seed)
    exact = gref.enumerate_strings(x, gram)
    strings = sorted(exact)
    assert len(strings) == count
    L = max(len(s) for s in strings)
    hyps = np.zeros((1, count, L), np.int32)
    lens = np.zeros((1, count), np.int32)
    for n, s in enumerate(strings):
        hyps[0, n, :len(s)], lens[0, n] = s, len(s)
    d_h, d_hl = _dev(device, hyps, lens)
    got = gram_ctc_nbest_logp(torch.tensor(x[:, None, :], device=device), d_h, d_hl, gram, 0).cpu().numpy()[0]
    want = np.array([exact[s] for s in strings])
    print("case", case, "worst |logp - exact| / |exact| =", (np.abs(got - want) / np.abs(want)).max())
    np.testing.assert_allclose(got, want, rtol=LOSS_RTOL)


# ---------------------------------------------------------------------------------------------- 4. with the beam
@pytest.mark.parametrize("run", ["full", "ragged"])
def test_exact_scores_of_the_beams_list(device, run):
    """gram_beam_decode at (16, 16) on the pruned inputs: ids and lengths pass straight in (unused slots -1); every used slot's
    exact log p is at or above the beam's lower bound (tests/test_gram_beam_gpu.py's tolerance) and equals that file's
    replicated-logits gram_ctc value to 1e-5"""
    from asr.loss import gram_ctc_nbest_logp
    gram, x, lengths = gref.pruned_inputs()
    ln = None if run == "full" else lengths
    ids, lens, scores = gbase.gbeam(device, x, gram, gref.W_P, gref.K_P, 0, ln)
    used = scores > -np.inf
    hl = np.where(used, lens, -1).astype(np.int32)
    width = int(hl.max())
    d_h, d_hl, d_ln = _dev(device, np.ascontiguousarray(ids[:, :, :width]), hl, ln)
    got = gram_ctc_nbest_logp(torch.tensor(x, device=device), d_h, d_hl, gram, 0, d_ln).cpu().numpy()
    assert np.array_equal(np.isfinite(got), used) and used[:, 0].all()
    assert (got[used] >= scores[used] - np.array([tol(s) for s in scores[used]])).all()
    worst = 0.0
    for b in range(x.shape[1]):
        slots = [n for n in range(gref.W_P) if used[b, n] and lens[b, n] > 0]
        strings = [tuple(int(c) for c in ids[b, n, :lens[b, n]]) for n in slots]
        want = gbase.gpu_gram_scores(device, x[:, b], gram, strings, None if ln is None else ln[b])
        np.testing.assert_allclose(got[b, slots], want, rtol=1e-5)
        worst = max(worst, (np.abs(got[b, slots] - want) / np.abs(want)).max())
    print("%s: %d used slots, largest exact - beam score %.3g, worst relative difference to the replicated route %.3g"
          % (run, used.sum(), (got[used] - scores[used]).max(), worst))


# ---------------------------------------------------------------------------------------------- 5. gram_mwer_loss
@pytest.mark.parametrize("reduce", ["mean", "no"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("T,B,V,N,L", CASES[:2])
def test_gram_mwer_loss_with_given_hypotheses(device, T, B, V, N, L, normalize, reduce):
    """the three steps of tests/test_ctc_nbest_gpu.py::test_mwer_loss_with_given_hypotheses, over characters"""
    from asr.loss import gram_mwer_loss
    xs, hyps, hyp_len, x_len, _, dead, logp, grads = _case(T, B, V, N, L)
    gram = _table(V)
    rs = np.random.RandomState(N + L)
    chars = sorted(gref.unigram_ids(gram))
    t = np.array(chars, np.int32)[rs.randint(len(chars), size=(B, L + 2))]
    t_len = rs.randint(1, L + 3, size=B).astype(np.int32)
    t[0, :L], t_len[0] = hyps[0, 0], L                 # one hypothesis is its utterance's transcript: e = 0
    d_h, d_hl, d_xl, d_t, d_tl = _dev(device, hyps, hyp_len, x_len, t, t_len)
    x = torch.tensor(xs, device=device, requires_grad=True)
    res = gram_mwer_loss(x, d_t, gram, 0, d_xl, d_tl, hyps=d_h, hyp_lengths=d_hl, normalize=normalize, reduce=reduce)
    w = np.ones(B) / B if reduce == "mean" else rs.rand(B) + 0.5
    if reduce == "mean":
        assert res.loss.shape == ()
        res.loss.backward()
    else:
        assert res.loss.shape == (B,)
        res.loss.backward(torch.tensor(w.astype(np.float32), device=device))
        w = w.astype(np.float32).astype(np.float64)
    assert torch.equal(res.hyps, d_h) and torch.equal(res.hyp_lengths, d_hl)
    # (a) the returned logp against the restatement
    got_logp = res.logp.cpu().numpy()
    assert np.array_equal(np.isneginf(got_logp), dead)
    np.testing.assert_allclose(got_logp[~dead], logp[~dead], rtol=LOSS_RTOL)
    # (b) with the device's own logp in float64, loss and posteriors against the float64 formula
    e = ref.errors(hyps, hyp_len, t, t_len, normalize)
    np.testing.assert_allclose(res.errors.cpu().numpy(), e, rtol=1e-6)
    assert e[0, 0] == 0
    loss_b, post, coef, spread = ref.mwer(got_logp.astype(np.float64), e)
    got_loss = res.loss.detach().cpu().numpy().astype(np.float64)
    if reduce == "mean":
        assert abs(got_loss - loss_b.mean()) <= 1e-5 * spread.mean(), (got_loss, loss_b.mean())
    else:
        assert (np.abs(got_loss - loss_b) <= 1e-5 * spread).all(), (got_loss, loss_b)
    assert np.abs(res.posteriors.cpu().numpy() - post).max() <= 1e-5
    assert np.isfinite(got_loss).all()
    # (c) x.grad = sum_n c_n g_n with c_n from (b) and g_n from the restatement, inside the derived gradient bound
    c = coef * w[:, None]
    want, mag = ref.weighted_grad(grads, c, B, N, T, V)
    bound = _grad_bound(np.abs(c).sum(axis=1), mag)
    gr = x.grad.cpu().numpy()
    assert np.isfinite(gr).all()
    err = np.abs(gr - want)
    print("gram mwer %s %s normalize=%s: worst |dgrad| / bound = %.3g" % ((T, B, V, N, L), reduce, normalize, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()


def _peaky_gram_batch(T, B, gram, seed):
    rs = np.random.RandomState(seed)
    return np.stack([gref.peaky_gram(rs, T, gram) for _ in range(B)], axis=1).astype(np.float32)


@pytest.mark.parametrize("with_lm", [False, True], ids=["acoustic", "lm"])
def test_gram_mwer_loss_end_to_end_with_its_own_beam(device, with_lm):
    """the list is the Gram-CTC beam's (with `lm`: the fused search's, an order-2 character model); loss, posteriors and errors
    equal the restatement evaluated on the list that is returned; the same list passed back in gives the same result"""
    from asr import error, lm as asr_lm
    from asr.loss import gram_mwer_loss
    gram = gref.pruned_table()
    V = len(gram)
    T, B, W = 60, 3, 4
    xs = _peaky_gram_batch(T, B, gram, seed=7)
    x_len = np.array([T, T - 7, T - 19], np.int32)
    d_xl, = _dev(device, x_len)
    x0 = torch.tensor(xs, device=device)
    kw = {}
    if with_lm:
        ng = lmref.random_model(np.random.RandomState(9), gref.U_P + 1, 2, [], n_random=300)
        model = asr_lm.NGramLM.from_ngrams(glm.relabel_marks(ng, gref.U_P + 1, V), V, V, V + 1)
        kw = dict(lm=model, lm_weight=0.5, length_bonus=1.0)
        ids, lens, scores = error.gram_beam_decode_lm(x0, gram, model, 0.5, 1.0, W, W, 0, d_xl)[:3]
    else:
        ids, lens, scores = error.gram_beam_decode(x0, gram, W, W, 0, d_xl)
    ids_h, lens_h, sc = ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()
    want_len = np.where(np.isneginf(sc), -1, lens_h).astype(np.int32)
    width = max(1, int(want_len.max()))
    assert width > 2 and (want_len[:, 0] > 0).all()
    # transcripts: utterance 0's is its best string (already listed), the others' are their best string plus one character
    t = np.zeros((B, width + 1), np.int32)
    t_len = np.zeros(B, np.int32)
    for b in range(B):
        n = lens_h[b, 0]
        t[b, :n], t_len[b] = ids_h[b, 0, :n], n + (b > 0)
        t[b, n] = 1 + (ids_h[b, 0, n - 1] % (gref.U_P - 1)) if b > 0 else 0
    d_t, d_tl = _dev(device, t, t_len)

    def run(**more):
        x = x0.clone().requires_grad_(True)
        r = gram_mwer_loss(x, d_t, gram, 0, d_xl, d_tl, beam_width=W, top_k=W, **kw, **more)
        r.loss.sum().backward()
        return r, x.grad
    r1, g1 = run(reduce="no")
    assert np.array_equal(r1.hyps.cpu().numpy(), ids_h[:, :, :width]) and np.array_equal(r1.hyp_lengths.cpu().numpy(), want_len)
    assert torch.isfinite(r1.loss).all() and torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    logp64 = ref.nbest_logp_grad(xs, ids_h[:, :, :width], want_len, gram, x_len, want_grad=False)
    got = r1.logp.cpu().numpy()
    assert np.array_equal(np.isfinite(got), want_len >= 0) and np.array_equal(np.isfinite(logp64), want_len >= 0)
    np.testing.assert_allclose(got[want_len >= 0], logp64[want_len >= 0], rtol=LOSS_RTOL)
    e = ref.errors(ids_h[:, :, :width], want_len, t, t_len)
    assert np.array_equal(r1.errors.cpu().numpy(), e) and e[0, 0] == 0 and (e[1:, 0] == 1).all()
    loss_b, post, _, spread = ref.mwer(got.astype(np.float64), e)
    assert (np.abs(r1.loss.detach().cpu().numpy() - loss_b) <= 1e-5 * spread).all()
    assert np.abs(r1.posteriors.cpu().numpy() - post).max() <= 1e-5
    r2, g2 = run(reduce="no", hyps=r1.hyps, hyp_lengths=r1.hyp_lengths)
    assert torch.equal(r1.logp, r2.logp) and torch.equal(r1.loss, r2.loss)
    assert float((g1 - g2).abs().max()) <= 1e-5 * float(g1.abs().max())
    # max_length: no synchronisation, longer strings dropped; the ids are 2 T wide
    r3, _ = run(max_length=width - 1)
    assert r3.hyps.shape[2] == width - 1
    assert np.array_equal(r3.hyp_lengths.cpu().numpy(), np.where(want_len > width - 1, -1, want_len))
    assert run(max_length=5 * T)[0].hyps.shape[2] == 2 * T
    # add_reference: utterance 0 lists its transcript (the appended slot stays unused), the others get it as slot W
    ra, _ = run(add_reference=True, reduce="no")
    h_ref, l_ref = ref.with_reference(ids_h[:, :, :width], want_len, t, t_len)
    assert l_ref[0, W] == -1 and (l_ref[1:, W] == t_len[1:]).all()
    assert np.array_equal(ra.hyp_lengths.cpu().numpy(), l_ref) and np.array_equal(ra.hyps.cpu().numpy(), h_ref)
    assert ra.posteriors[0, W].item() == 0.0 and torch.isneginf(ra.logp[0, W]) and (ra.posteriors[1:, W] > 0).all()
    assert abs(ra.loss[0].item() - r1.loss[0].item()) <= 1e-6 * abs(r1.loss[0].item()) + 1e-9
    la64 = ref.nbest_logp_grad(xs, h_ref, l_ref, gram, x_len, want_grad=False)
    ga = ra.logp.cpu().numpy()
    assert np.array_equal(np.isfinite(ga), np.isfinite(la64))
    np.testing.assert_allclose(ga[np.isfinite(ga)], la64[np.isfinite(ga)], rtol=LOSS_RTOL)
    _, post_a, _, _ = ref.mwer(ga.astype(np.float64), ref.errors(h_ref, l_ref, t, t_len))
    assert np.abs(ra.posteriors.cpu().numpy() - post_a).max() <= 1e-5


# ---------------------------------------------------------------------------------------------- 6. LayerNorm interplay
def test_gram_mwer_plus_gram_ctc_on_layernorm_logits_fused_equals_unfused(device):
    """tests/test_ctc_nbest_gpu.py::test_mwer_plus_ctc_on_layernorm_logits_fused_equals_unfused with the Gram-CTC pair: gram_ctc
    leaves its recipe at the normalisation, gram_mwer_loss sends an ordinary gradient through autograd, the normalisation adds
    the two.  Same dx / dgamma as with the fusion off, to that test's bound"""
    from asr import functions as F, _ops
    from asr.link import Parameter
    from asr.loss import gram_ctc, gram_mwer_loss
    rs = np.random.RandomState(11)
    T, B, L, N = 30, 2, 4, 3
    gram = ref.shuffled_table(8, 27, seed=36)
    V = len(gram)
    assert V == 36
    x0 = torch.tensor((rs.randn(T * B, V) * 2.0 + 0.3).astype(np.float32)).to(device)
    g0 = torch.tensor(rs.uniform(0.5, 1.5, V).astype(np.float32))
    b0 = torch.tensor((rs.randn(V) * 0.2).astype(np.float32))
    chars = rs.randint(1, 9, size=(B, L)).astype(np.int32)
    chars[0, 1:3] = ref.table_pairs(gram)[0]
    lu, lb = _labels(chars, gram)
    hyps = rs.randint(1, 9, size=(B, N, L)).astype(np.int32)
    hyps[:, 0] = chars
    hyp_len = np.array([[L, L - 1, 0], [L, -1, L - 2]], np.int32)
    d_c, d_lu, d_lb, d_h, d_hl = _dev(device, chars, lu, lb, hyps, hyp_len)

    def run(fused):
        F.FUSE_CTC_INTO_LAYERNORM[0] = fused
        try:
            x = x0.clone().requires_grad_(True)
            gamma, beta = Parameter(g0.clone().to(device)), Parameter(b0.clone().to(device))
            y = F.layer_normalization(x.reshape(T, B, 1, V).permute(1, 3, 2, 0), gamma, beta, out_f32=True)
            tbv = y.permute(3, 0, 2, 1).squeeze(2)
            before = _ops.CALLS.get("layernorm_ctc_bwd", 0)
            m = gram_mwer_loss(tbv, d_c, gram, 0, hyps=d_h, hyp_lengths=d_hl)
            total = m.loss + 0.3 * gram_ctc(tbv, d_lu, d_lb, 0)
            total.backward()
            torch.cuda.synchronize()
            assert _ops.CALLS.get("layernorm_ctc_bwd", 0) - before == (1 if fused else 0)
            return total.item(), x.grad.clone(), gamma.grad.clone()
        finally:
            F.FUSE_CTC_INTO_LAYERNORM[0] = True
    (lf, dxf, dgf), (lu_, dxu, dgu) = run(True), run(False)
    assert abs(lf - lu_) <= 1e-5 * abs(lu_)
    assert float(dxu.abs().max()) > 0
    assert float((dxf - dxu).abs().max()) <= 1e-4 * float(dxu.abs().max())
    assert float((dgf - dgu).abs().max()) <= 1e-4 * float(dgu.abs().max()) + 1e-6


# ---------------------------------------------------------------------------------------------- 7. tuple of views
def test_tuple_of_views_input(device):
    from asr.loss import gram_ctc_nbest_logp
    T, B, V, N, L = CASES[0]
    xs, hyps, hyp_len, x_len, gy = _case(T, B, V, N, L)[:5]
    d_h, d_hl, d_xl, d_gy = _dev(device, hyps, hyp_len, x_len, gy)
    out = []
    for as_tuple in (False, True):
        x = torch.tensor(xs, device=device, requires_grad=True)
        logp = gram_ctc_nbest_logp(tuple(x.unbind(0)) if as_tuple else x, d_h, d_hl, torch.from_numpy(_table(V)).to(device), 0, d_xl)
        logp.backward(d_gy)
        out.append((logp.detach().cpu().numpy(), x.grad.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.abs(out[1][1] - out[0][1]).max() <= 1e-5 * np.abs(out[0][1]).max()      # (float atomics: the order of the adds is not fixed)


# ---------------------------------------------------------------------------------------------- 8. error codes
def test_error_codes(device):
    """refused before anything is launched (logp and grad keep their contents)"""
    from asr import _lib
    lib = _lib.lib()
    T, B, V, N, L = 20, 2, 9, 3, 4
    x = torch.randn(T, B, V, device=device)
    gram = torch.tensor(ref.shuffled_table(3, 5, seed=1), device=device)
    hyp = torch.ones((B, 129, L), dtype=torch.int32, device=device)
    hl = torch.full((B, 129), L, dtype=torch.int32, device=device)
    logp = torch.full((B, 129), 7.0, device=device)
    gy = torch.ones((B, 129), device=device)
    grad = torch.full((T, B, V), 7.0, device=device)
    nbytes = lib.asr_gram_ctc_nbest_workspace_bytes(T, B, V, N, L)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    p, s = _lib.ptr, _lib.stream()
    BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -3

    def fwd(n, xs=x, h=hyp, g=gram, nb=nbytes, w=ws, b=B, lmax=L, blank=0):
        return lib.asr_gram_ctc_nbest_forward(s, p(xs), p(h), p(hl), None, p(g), T, b, V, n, lmax, blank, p(logp), p(w), nb)

    def bwd(n, g=gy, nb=nbytes, w=ws, b=B, lmax=L):
        return lib.asr_gram_ctc_nbest_backward(s, p(x), None, T, b, V, n, lmax, p(g), p(grad), p(w), nb)
    for n in (0, -1, 129):                                                                  # N outside [1, 128]
        assert fwd(n) == UNSUPPORTED and bwd(n) == UNSUPPORTED, n
    assert fwd(N, b=0) == BAD_ARG and bwd(N, b=0) == BAD_ARG
    assert fwd(N, nb=nbytes - 1) == WORKSPACE and bwd(N, nb=nbytes - 1) == WORKSPACE
    assert fwd(N, xs=None) == BAD_ARG and fwd(N, h=None) == BAD_ARG and fwd(N, w=None) == BAD_ARG
    assert fwd(N, g=None) == UNSUPPORTED                                                   # as the Gram-CTC beam entries
    assert bwd(N, g=None) == BAD_ARG and bwd(N, w=None) == BAD_ARG
    assert fwd(N, blank=V) == BAD_ARG and fwd(N, blank=-1) == BAD_ARG
    assert fwd(N, lmax=80000, nb=1 << 62) == UNSUPPORTED and bwd(N, lmax=80000, nb=1 << 62) == UNSUPPORTED      # the sweep's LDS
    assert fwd(128, b=1 << 20, nb=1 << 62) == UNSUPPORTED and bwd(128, b=1 << 20, nb=1 << 62) == UNSUPPORTED    # B N Sp > int32
    torch.cuda.synchronize()
    assert (logp == 7.0).all() and (grad == 7.0).all()
    from asr.loss import gram_ctc_nbest_logp
    with pytest.raises(TypeError):
        gram_ctc_nbest_logp(x, hyp[:, :N].long(), hl[:, :N], gram, 0)


# ---------------------------------------------------------------------------------------------- 9. full size, once
def test_full_size_once(device):
    """B = 32, T = 1000, V = 3000 (118 characters, 2881 bigrams, shuffled token ids), N = 16, the lists from gram_beam_decode:
    log p finite exactly for the used slots and at or above the beam's score, the gradient finite and 0 beyond x_len, and for 2
    sampled utterances log p and the gradient rows against the restatement"""
    from asr.error import gram_beam_decode
    from asr.loss import gram_ctc_nbest_logp
    T, B, N = 1000, 32, 16
    gram = ref.shuffled_table(118, 2881, seed=3000)
    V = len(gram)
    assert V == 3000
    xs = _peaky_gram_batch(T, B, gram, seed=3)
    rs = np.random.RandomState(4)
    x_len = rs.randint(600, T + 1, size=B).astype(np.int32)
    x_len[0] = T
    d_xl, = _dev(device, x_len)
    x = torch.tensor(xs, device=device, requires_grad=True)
    ids, lens, scores = gram_beam_decode(x.detach(), gram, N, 16, 0, d_xl)
    lens = torch.where(scores > float("-inf"), lens, torch.full_like(lens, -1))
    width = int(lens.max().item())
    hyps = ids[:, :, :width].contiguous()
    gy = torch.tensor(rs.randn(B, N).astype(np.float32), device=device)
    logp = gram_ctc_nbest_logp(x, hyps, lens, gram, 0, d_xl)
    logp.backward(gy)
    got, sc, lens_h = logp.detach().cpu().numpy(), scores.cpu().numpy(), lens.cpu().numpy()
    used = lens_h >= 0
    assert used[:, 0].all() and np.array_equal(np.isfinite(got), used)
    assert (got[used] >= sc[used] - 1e-4 * np.abs(sc[used])).all()
    gr = x.grad
    mask = (torch.arange(T)[:, None] < torch.tensor(x_len.astype(np.int64))[None, :])
    assert torch.isfinite(gr).all() and (gr.cpu()[~mask] == 0).all()
    for b in (3, 20):
        hb, lb = hyps[b:b + 1].cpu().numpy(), lens_h[b:b + 1]
        logp64, grads = ref.nbest_logp_grad(xs[:, b:b + 1], hb, lb, gram, x_len[b:b + 1])
        np.testing.assert_allclose(got[b][used[b]], logp64[0][used[b]], rtol=LOSS_RTOL)
        gyb = np.where(used[b], gy[b].cpu().numpy(), 0.0).astype(np.float64)[None, :]
        want, mag = ref.weighted_grad(grads, gyb, 1, N, T, V)
        err = np.abs(gr[:, b].cpu().numpy() - want[:, 0])
        bound = _grad_bound(np.abs(gyb).sum(axis=1), mag)[:, 0]
        print("full size, utterance %d: used slots %d of %d, width %d, worst |dgrad| / bound = %.3g"
              % (b, used.sum(), used.size, width, (err / bound).max()))
        assert (err <= bound).all(), (err / bound).max()
        del grads, want, mag
