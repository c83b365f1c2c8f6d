"""N-best CTC scoring and the MWER loss without a GPU: the float64 restatement (tests/ctc_nbest_reference.py) against torch's
own CTC with autograd, the (B, N) arithmetic of asr.loss.mwer_loss against float64 autograd, and the ABI."""
import os
import re

import numpy as np
import torch

import ctc_nbest_reference as ref
from conftest import PKG, ROOT

SYMBOLS = ("asr_ctc_nbest_workspace_bytes", "asr_ctc_nbest_forward", "asr_ctc_nbest_backward")


def test_restatement_against_torch_ctc_with_autograd():
    """logp and the gradient of sum gy logp over the feasible slots against torch.nn.functional.ctc_loss in float64 on logits
    replicated per slot (the route this change replaces), rtol 1e-9; the empty hypothesis, which torch also scores, included"""
    T, B, V, N, L = 40, 3, 9, 4, 5
    xs, hyps, hyp_len, x_len, gy, dead = ref.random_case(T, B, V, N, L, seed=5)
    logp, grads = ref.nbest_logp_grad(xs, hyps, hyp_len, x_len)
    assert np.array_equal(~np.isfinite(logp), dead)
    live = ~dead
    gy64 = np.where(live, gy, 0.0).astype(np.float64)
    x = torch.tensor(xs.astype(np.float64), requires_grad=True)
    rep = x.repeat_interleave(N, dim=1)                                  # (T, B * N, V)
    nll = torch.nn.functional.ctc_loss(torch.log_softmax(rep, dim=2), torch.tensor(hyps.reshape(B * N, L).astype(np.int64)),
                                       torch.tensor(np.repeat(x_len, N).astype(np.int64)),
                                       torch.tensor(np.maximum(hyp_len, 0).reshape(B * N).astype(np.int64)), blank=0,
                                       reduction="none", zero_infinity=True)
    want = -nll.reshape(B, N)
    mask = torch.tensor(live)
    np.testing.assert_allclose(logp[live], want.detach().numpy()[live], rtol=1e-9)
    (want * torch.tensor(gy64))[mask].sum().backward()
    got, _ = ref.weighted_grad(grads, gy64, B, N, T, V)
    np.testing.assert_allclose(got, x.grad.numpy(), rtol=1e-9, atol=1e-12)
    for b in range(B):                                                   # nothing beyond the utterance's frames
        assert not got[x_len[b]:, b].any()


def test_feasibility_is_length_plus_adjacent_repeats():
    assert ref.feasible([3, 3, 4], 3, 4) and not ref.feasible([3, 3, 4], 3, 3)
    assert ref.feasible([3, 4, 3], 3, 3) and ref.feasible([], 0, 1) and not ref.feasible([1], -1, 10)
    x = np.random.RandomState(0).randn(4, 5)
    assert ref.slot_logp_grad(x, [3, 3, 4], 3, 3)[0] == -np.inf
    assert np.isfinite(ref.slot_logp_grad(x, [3, 3, 4], 3, 4)[0])
    lp0, g0 = ref.slot_logp_grad(x, [0], 0, 3)
    np.testing.assert_allclose(lp0, ref.log_softmax64(x[:3])[:, 0].sum(), rtol=1e-12)
    assert not g0[3:].any() and np.abs(g0[:3].sum(axis=1)).max() < 1e-12


def _logp_errors(seed, B=4, N=6):
    rs = np.random.RandomState(seed)
    logp = -rs.uniform(1.0, 30.0, size=(B, N))
    e = rs.randint(0, 9, size=(B, N)).astype(np.float64)
    logp[0, 2] = -np.inf
    logp[1, :] = -np.inf                 # an utterance without a valid slot
    logp[2, 1:] = -np.inf                # a single valid slot
    return logp, e


def test_mwer_coefficients_against_float64_autograd():
    """d loss_b / d logp_n = P_n (e_n - sum_m P_m e_m): the restatement's closed form and asr.loss.mwer_parts (what mwer_loss
    runs on the device) against autograd of the float64 loss, 1e-12; -inf slots give no NaN anywhere"""
    from asr.loss import mwer_parts
    logp, e = _logp_errors(1)
    loss, post, coef, _ = ref.mwer(logp, e)
    lp = torch.tensor(logp, requires_grad=True)
    loss_t, post_t = mwer_parts(lp, torch.tensor(e))
    loss_t.sum().backward()
    assert torch.isfinite(loss_t).all() and torch.isfinite(post_t).all() and torch.isfinite(lp.grad).all()
    np.testing.assert_allclose(loss_t.detach().numpy(), loss, rtol=0, atol=1e-12)
    np.testing.assert_allclose(post_t.detach().numpy(), post, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lp.grad.numpy(), coef, rtol=0, atol=1e-12)
    # and the plain formula with torch.softmax over the valid slots of one row, by autograd
    b = 0
    S = np.nonzero(np.isfinite(logp[b]))[0]
    z = torch.tensor(logp[b, S], requires_grad=True)
    es = torch.tensor(e[b, S])
    (torch.softmax(z, 0) * (es - es.mean())).sum().backward()
    np.testing.assert_allclose(z.grad.numpy(), coef[b, S], rtol=0, atol=1e-12)
    assert loss[1] == 0 and not post[1].any() and abs(loss[2]) < 1e-15 and post[2, 0] == 1.0


def test_mwer_parts_in_float32_has_no_nan_for_far_apart_scores():
    from asr.loss import mwer_parts
    lp = torch.tensor([[-5000.0, -5200.0, float("-inf")], [float("-inf")] * 3], requires_grad=True)
    loss, post = mwer_parts(lp, torch.tensor([[1.0, 3.0, 2.0], [1.0, 2.0, 3.0]]))
    loss.sum().backward()
    assert torch.isfinite(loss).all() and torch.isfinite(post).all() and torch.isfinite(lp.grad).all()
    assert post[0, 0].item() == 1.0 and post[1].sum().item() == 0.0


def test_add_reference_never_counts_the_reference_twice():
    rs = np.random.RandomState(2)
    B, N, L = 3, 4, 5
    hyps = rs.randint(1, 8, size=(B, N, L)).astype(np.int32)
    hyp_len = rs.randint(1, L + 1, size=(B, N)).astype(np.int32)
    t = rs.randint(1, 8, size=(B, 7)).astype(np.int32)
    t_len = np.array([7, 3, 4], np.int32)
    hyps[1, 2, :3], hyp_len[1, 2] = t[1, :3], 3          # utterance 1 lists its transcript
    hyps[2, 1, :4], hyp_len[2, 1] = t[2, :4], -1         # utterance 2 holds it in an UNUSED slot: that does not count
    out, lens = ref.with_reference(hyps, hyp_len, t, t_len)
    assert out.shape == (B, N + 1, 7) and list(lens[:, N]) == [7, -1, 4]
    e = ref.errors(out, lens, t, t_len)
    for b in range(B):
        used = lens[b] >= 0
        assert int(((e[b] == 0) & used).sum()) == 1      # exactly one slot in use is the transcript
    assert (out[:, :N, :L] == hyps).all() and (lens[:, :N] == hyp_len).all()


def test_header_binding_and_library_have_the_nbest_symbols():
    import ctypes
    from asr import _lib
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    handle = _lib.lib()
    half = ctypes.CDLL(os.path.join(PKG, "libasr_hip_f16.so"))
    for name in SYMBOLS:
        assert hasattr(handle, name) and hasattr(half, name), name


def test_workspace_query_and_limits_on_the_host():
    from asr import _lib
    lib = _lib.lib()
    n1 = lib.asr_ctc_nbest_workspace_bytes(100, 4, 50, 1, 10)
    n4 = lib.asr_ctc_nbest_workspace_bytes(100, 4, 50, 4, 10)
    assert n1 > 4 * 100 * 64 * (8 + 8 + 4) and 3 * n1 < n4 < 4 * n1
    assert lib.asr_ctc_nbest_workspace_bytes(100, 4, 50, 0, 10) == 0
    assert lib.asr_ctc_nbest_workspace_bytes(100, 4, 50, 129, 10) == 0
    assert lib.asr_ctc_nbest_workspace_bytes(100, 4, 50, 128, 10) > 0
    # the headline size of profiles/ctc_nbest.txt with the loss's float64 layout: about 2.6 GB at Lmax = 120
    assert 2.5e9 < lib.asr_ctc_nbest_workspace_bytes(1000, 32, 3000, 16, 120) < 2.8e9


def test_no_cpu_path():
    import pytest
    from asr import _lib
    from asr.loss import ctc_nbest_logp
    with pytest.raises(_lib.AsrHipError):
        ctc_nbest_logp(torch.zeros(4, 2, 5), torch.ones(2, 3, 1, dtype=torch.int32), torch.ones(2, 3, dtype=torch.int32), 0)
