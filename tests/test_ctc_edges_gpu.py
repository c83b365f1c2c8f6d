"""The CTC / Gram-CTC loss lattice (csrc/ctc.hip, csrc/ctc_sweep.hpp, csrc/ctc_lattice.hpp, csrc/ctc_ln.hip) at its edges and on
long transcripts, through the public asr.loss functions against the float64 oracle (oracle/ctc.py).

tests/test_ctc_gpu.py runs the loss on comfortable inputs (x_len >= 3 L, L <= 171, logits 1.5 randn).  This module runs what
those never reach:

  a  empty / one-frame / exactly-feasible / infeasible / frameless utterances in one batch
  b  the same utterances behind a per-frame LayerNormalization (the fused backward of csrc/ctc_ln.hip)
  c  every residue of the one-node sweep's prefetch loops (x_len = 1 .. 11; whole blocks with and without a tail)
  d  both sides of the switch between the one-node and the strided sweep (more than 1024 path nodes), and the launch with more
     than 48 KB of LDS
  e  the largest transcript the sweep accepts (CTC 3807, Gram-CTC 2538 labels) and the first it refuses (3808, 2539)
  f  labels in the second and third occupancy chunk of the gradient kernels (V > 8192), loss and N-best scorer
  g  numerics: peaked and near-one-hot rows, equal rows, a large common offset, masked (-inf) vocabulary entries, a long run
     of one label
  h  labels outside the vocabulary

Tolerances are tests/test_ctc_gpu.py's LOSS_RTOL, GRAD_RTOL, GRAD_ATOL, imported.  Every comparison asserts besides: the
gradient is finite; it is bitwise zero for t >= x_len[b]; an utterance without a path reports exactly 1e10 and its gradient is
softmax * scale.  reduce="no" is driven with a per-utterance gy that holds a zero and a negative entry (|gy| <= 1, so that the
absolute tolerance of the gy = 1 comparisons applies as it stands).

g, the bound where float32 storage decides.  The device stores x[l] - lse in float32 (rows_kernel); with logits of magnitude
1e2 .. 1e4 that alone costs more than the fixed tolerances.  For the cases "x40", "offset 1e4" and "one-hot" the bound is
therefore built from the reference alone: the oracle runs a second time with its log-softmax rounded as the device rounds it
(oracle.ctc.log_softmax_f32), and the bound is the larger of the fixed tolerance and 4 x the distance between the two oracle
runs (maximum norm: over the batch for the loss, over the array for the unscaled gradient).  The factor 4 covers __expf / __logf
against numpy's, which the rounding-matched run does not model.  The other cases keep the fixed tolerances.

Measured on an MI355X (T = 40, B = 3, V = 11; worst error / bound over reduce="mean" and "no", CTC then Gram-CTC).  "fixed": the
imported tolerances alone, |dloss| <= 1e-4 |loss| and |dgrad| <= 1e-5 + 1e-4 |grad|.  A derived floor is absolute, 4 x the distance
between the two oracle runs, and counts where it is above the fixed bound:

    case         loss bound                        gradient bound              worst loss error / bound   worst gradient error / bound
    x8           fixed                             fixed                       2.8e-4, 5.7e-4             0.071, 0.071
    x40          fixed (floor 5.0e-5 < 0.098)      max(fixed, 1.51e-5)         2.4e-4, 2.4e-4             0.117, 0.107
    equal rows   fixed                             fixed                       1.6e-3, 1.6e-3             4.2e-3, 3.6e-3
    offset 1e4   max(fixed, 1.62e-2)               max(fixed, 8.35e-4)         0.25,   0.25               0.25,  0.25
    masked       fixed                             fixed                       4.1e-4, 3.6e-4             6.3e-3, 5.6e-3
    run of 20    fixed                             fixed                       2.3e-4, 1.7e-4             2.5e-3, 4.9e-3
    one-hot      fixed (floor 6.2e-6 < 0.015)      fixed (floor 1.75e-6)       5.2e-4, 6.2e-4             0.025, 0.019

"offset 1e4" at exactly a quarter of its bound: the device's error there IS the float32 rounding of lse = 1e4 + log(sum) (half an
ulp of 2^-10 per frame), which the rounding-matched oracle run reproduces digit for digit.  The gradient is what needs the derived
bound there: its error, 2.1e-4, is about twice what the fixed tolerance allows for an entry of magnitude one (1.1e-4) and twenty
times its absolute part; the loss error, 4.1e-3 at most, lies just inside the fixed 1e-4 relative (4.6e-3 for the smallest loss of the batch).
"""
import functools

import numpy as np
import pytest
import torch

import ctc_nbest_reference as nbest_ref
from oracle import ctc as octc
from test_ctc_gpu import GRAD_ATOL, GRAD_RTOL, LOSS_RTOL, _ln_ctc_oracle, _run
from test_ctc_nbest_gpu import _grad_bound as _nbest_grad_bound

pytestmark = pytest.mark.gpu

INFEASIBLE = 1e10
KINDS = pytest.mark.parametrize("gram", [False, True], ids=["ctc", "gram"])


# ---------------------------------------------------------------------------------------------- helpers
def _softmax64(xs):
    return np.exp(octc.log_softmax(xs, axis=2))


def _oracle_no(xs, uni, big, xl, tl, **kw):
    """per-utterance losses (B) and unscaled gradients (T, B, V): reduce="no" with gy = 1.  Every other reduction and gy is
    this gradient times a per-utterance factor, so the oracle runs once per case."""
    if big is None:
        return octc.ctc_loss_grad(xs, uni, 0, xl, tl, "no", None, **kw)
    return octc.gram_ctc_loss_grad(xs, uni, big, 0, xl, tl, "no", None, **kw)


def _gy(B):
    """per-utterance upstream gradient for reduce="no": |gy| <= 1, one negative entry and (B >= 2) one zero"""
    gy = np.random.RandomState(B).uniform(0.3, 1.0, B).astype(np.float32)
    gy[0 if B < 3 else 1] *= -1.0
    if B >= 2:
        gy[B - 1] = 0.0
    return gy


def _compare(device, xs, uni, big, xl, tl, want, tag, loss_abs=0.0, grad_abs=0.0, reduces=("mean", "no")):
    """device loss and gradient against want = (losses (B), unscaled gradients (T, B, V)) in both reductions, with the
    assertions the module docstring lists.  loss_abs / grad_abs: absolute floors of the bound (numerics cases only).
    -> worst error / bound (loss, gradient)"""
    lo, G = want
    T, B, V = xs.shape
    xlc = np.full(B, T) if xl is None else np.clip(xl, 0, T)
    dead = lo == INFEASIBLE
    y = _softmax64(xs)
    worst_l = worst_g = 0.0
    for reduce in reduces:
        gy = None if reduce == "mean" else _gy(B)
        l, g = _run(device, xs, uni, big, xl, tl, reduce, gy)
        scale = np.full(B, 1.0 / B) if reduce == "mean" else gy.astype(np.float64)
        assert np.isfinite(g).all(), tag
        for b in range(B):
            assert not np.ascontiguousarray(g[xlc[b]:, b]).view(np.uint32).any(), (tag, reduce, b)     # bitwise zero
        if reduce == "mean":
            err, bound = abs(float(l) - lo.mean()), LOSS_RTOL * abs(lo.mean()) + loss_abs
            assert err <= bound, (tag, reduce, float(l), lo.mean())
            worst_l = max(worst_l, err / bound)
        else:
            assert l.shape == (B,)
            assert np.array_equal(l == np.float32(INFEASIBLE), dead), (tag, l, lo)      # exactly 1e10, exactly there
            err, bound = np.abs(l - lo)[~dead], np.maximum(LOSS_RTOL * np.abs(lo), loss_abs)[~dead]
            assert (err <= bound).all(), (tag, reduce, l, lo)
            if err.size:
                worst_l = max(worst_l, float((err / np.maximum(bound, 1e-300)).max()))
        sc = scale[None, :, None]
        want_g = G * sc
        bound = np.maximum(GRAD_ATOL + GRAD_RTOL * np.abs(want_g), grad_abs * np.abs(sc))
        err = np.abs(g - want_g)
        assert (err <= bound).all(), (tag, reduce, float((err / bound).max()), np.unravel_index((err / bound).argmax(), err.shape))
        worst_g = max(worst_g, float((err / bound).max()))
        for b in np.nonzero(dead)[0]:               # no path: the occupancy is zero, softmax * scale is left
            np.testing.assert_allclose(g[:xlc[b], b], y[:xlc[b], b] * scale[b], rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=tag)
    print("%s: worst loss error / bound %.3g, worst gradient error / bound %.3g" % (tag, worst_l, worst_g))
    return worst_l, worst_g


def _labels(rs, B, L, lo, hi):
    """(B, L) ids in [lo, hi) whose neighbours differ, except one forced repeat at positions 1, 2"""
    lab = rs.randint(lo, hi, size=(B, L))
    for i in range(1, L):
        same = lab[:, i] == lab[:, i - 1]
        lab[same, i] = lo + (lab[same, i] - lo + 1) % (hi - lo)
    if L >= 3:
        lab[:, 2] = lab[:, 1]
        if L >= 4:
            same = lab[:, 3] == lab[:, 2]
            lab[same, 3] = lo + (lab[same, 3] - lo + 1) % (hi - lo)
    return lab.astype(np.int32)


def _bigrams(rs, B, L, lo, hi, p_absent=0.3):
    big = rs.randint(lo, hi, size=(B, L)).astype(np.int32)
    big[rs.rand(B, L) < p_absent] = -1
    big[:, 0] = -1
    return big


# ---------------------------------------------------------------------------------------------- a. edges in one batch
EDGE_T, EDGE_L = 12, 4
#          unigrams       bigrams            x_len  l_len
EDGES = [([1, 2, 3, 4], [-1, 6, 7, 8],       7,     0),    # 0  empty transcript: one blank node, final
         ([3, 1, 2, 4], [-1, 6, 7, 8],       1,     1),    # 1  one label in one frame: the backward sweep has no step
         ([1, 2, 3, 4], [-1, -1, -1, -1],    4,     4),    # 2  x_len == l_len, no repeats, no bigrams: exactly one path
         ([5, 5, 5, 5], [-1, -1, -1, -1],    7,     4),    # 3  four equal labels in 2 L - 1 frames: exactly one path
         ([5, 5, 5, 5], [-1, -1, -1, -1],    6,     4),    # 4  the same in 2 L - 2 frames: no path
         ([1, 2, 1, 3], [-1, 7, -1, 8],      1,     4),    # 5  x_len < l_len (and below the two bigrams Gram-CTC needs): no path
         ([2, 4, 1, 3], [-1, 6, -1, -1],     0,     2),    # 6  no frames
         ([3, 3, 5, 2], [-1, 6, 7, 8],       12,    4),    # 7  x_len = T, l_len = Lmax, a repeat, last bigram alive
         ([2, 2, 4, 1], [-1, -1, 7, 6],      4,     3),    # 8  x_len == l_len + repeats; last bigram of the row alive, one beyond l_len
         ([1, 2, 3, 1], [-1, -1, -1, -1],    9,     4),    # 9  Gram-CTC: a bigram row of all -1
         ([4, 1, 2, 3], [-1, -1, -1, 8],     4,     4)]    # 10 Gram-CTC: only the last bigram alive, x_len == l_len
ONE_PATH = 2


def _edge_batch(V, seed=9):
    rs = np.random.RandomState(seed)
    B = len(EDGES)
    xs = (rs.randn(EDGE_T, B, V) * 2.0).astype(np.float32)
    uni = np.array([e[0] for e in EDGES], np.int32)
    big = np.array([e[1] for e in EDGES], np.int32)
    xl = np.array([e[2] for e in EDGES], np.int32)
    tl = np.array([e[3] for e in EDGES], np.int32)
    return xs, uni, big, xl, tl


@KINDS
def test_edges_in_one_batch(device, gram):
    xs, uni, big, xl, tl = _edge_batch(9)
    big = big if gram else None
    lo, G = want = _oracle_no(xs, uni, big, xl, tl)
    assert np.array_equal(lo == INFEASIBLE, np.isin(np.arange(len(EDGES)), (4, 5, 6)))        # the batch is what its comments say
    # the utterance with exactly one path, in closed form: loss = -sum_t log softmax(x_t)[label_t], gradient = softmax - onehot
    b, n = ONE_PATH, xl[ONE_PATH]
    logy = octc.log_softmax(xs[:n, b], axis=1)
    onehot = np.zeros_like(logy)
    onehot[np.arange(n), uni[b, :n]] = 1.0
    assert abs(lo[b] + logy[np.arange(n), uni[b, :n]].sum()) <= 1e-12 * abs(lo[b])
    assert np.abs(G[:n, b] - (np.exp(logy) - onehot)).max() <= 1e-12
    _compare(device, xs, uni, big, xl, tl, want, "edges")
    l, g = _run(device, xs, uni, big, xl, tl, "no")
    np.testing.assert_allclose(l[b], -logy[np.arange(n), uni[b, :n]].sum(), rtol=LOSS_RTOL)
    np.testing.assert_allclose(g[:n, b], np.exp(logy) - onehot, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    # without the length arrays every utterance has T frames and Lmax labels
    _compare(device, xs, uni, big, None, None, _oracle_no(xs, uni, big, None, None), "edges, no lengths")


# ---------------------------------------------------------------------------------------------- b. behind a LayerNormalization
LN_V = 12       # the fused LayerNorm + loss backward takes rows of a multiple of four logits (asr/functions.py: per_frame)


@pytest.mark.parametrize("losses", [[("ctc", "mean")], [("ctc", "no")], [("gram", "mean")], [("gram", "no")],
                                    [("gram", "mean"), ("ctc", "mean")], [("gram", "no"), ("ctc", "mean")]],
                         ids=lambda ls: "+".join("%s_%s" % l for l in ls))
def test_edges_behind_a_layernormalization(device, losses):
    """the utterances of test_edges_in_one_batch on per-frame normalised logits (the construction of tests/test_ctc_gpu.py's
    _ln_ctc_case, the oracle chain and the tolerances of its fused-equals-unfused and float64-oracle tests): empty, infeasible and
    frameless utterances through the `tot != -inf` and `live[q]` guards of csrc/ctc_ln.hip.  fused == unfused == oracle for dx,
    dgamma, dbeta.  V = 12 instead of a's 9: the fused sweep only takes rows of a multiple of four logits."""
    from asr import functions as F, _ops
    from asr.link import Parameter
    from asr.loss import connectionist_temporal_classification, gram_ctc
    _, uni, big, xl, tl = _edge_batch(LN_V)
    T, B, V = EDGE_T, len(EDGES), LN_V
    rs = np.random.RandomState(21)
    x0 = (rs.randn(T * B, V) * 2.0 + 0.3).astype(np.float32)
    g0 = rs.uniform(0.5, 1.5, V).astype(np.float32)
    b0 = (rs.randn(V) * 0.2).astype(np.float32)
    gy_no = _gy(B)
    d = lambda a: torch.tensor(a, device=device)        # noqa: E731
    d_uni, d_big, d_xl, d_tl, d_gy = d(uni), d(big), d(xl), d(tl), d(gy_no)

    def run(fused):
        F.FUSE_CTC_INTO_LAYERNORM[0] = fused
        try:
            x = d(x0).requires_grad_(True)
            gamma, beta = Parameter(d(g0)), Parameter(d(b0))
            y = F.layer_normalization(x.reshape(T, B, 1, V).permute(1, 3, 2, 0), gamma, beta, out_f32=True)
            tbv = y.permute(3, 0, 2, 1).squeeze(2)
            total = None
            for kind, reduce in losses:
                if kind == "ctc":
                    l = connectionist_temporal_classification(tbv, d_uni, 0, d_xl, d_tl, reduce)
                else:
                    l = gram_ctc(tbv, d_uni, d_big, 0, d_xl, d_tl, reduce)
                l = l if reduce == "mean" else (l * d_gy).sum()
                total = l if total is None else total + l
            before = _ops.CALLS.get("layernorm_ctc_bwd", 0)
            total.backward()
            torch.cuda.synchronize()
            assert _ops.CALLS.get("layernorm_ctc_bwd", 0) - before == (1 if fused else 0)
            if fused:
                assert F.LAST_FUSED_RECIPES[0] == len(losses)
            return total.item(), x.grad.clone(), gamma.grad.clone(), beta.grad.clone()
        finally:
            F.FUSE_CTC_INTO_LAYERNORM[0] = True

    (lf, dxf, dgf, dbf), (lu, dxu, dgu, dbu) = run(True), run(False)
    # fused against unfused: test_layernorm_ctc_backward_fused_equals_unfused
    assert lf == lu
    assert torch.isfinite(dxf).all() and torch.isfinite(dxu).all()
    scale = float(dxu.abs().max()) + 1e-30
    assert float((dxf - dxu).abs().max()) <= 2e-5 * scale + 1e-9, float((dxf - dxu).abs().max()) / scale
    for a, r in ((dgf, dgu), (dbf, dbu)):
        assert float((a - r).abs().max()) <= 1e-4 * (float(r.abs().max()) + 1e-30) + 1e-7
    # both against the float64 chain: test_layernorm_ctc_backward_against_the_float64_oracle
    lo, dxo, dgo, dbo = _ln_ctc_oracle(x0, g0, b0, uni, big, xl, tl, losses, gy_no, T, B, V)
    for tag, (l, dx, dg, db) in (("fused", (lf, dxf, dgf, dbf)), ("unfused", (lu, dxu, dgu, dbu))):
        np.testing.assert_allclose(l, lo, rtol=LOSS_RTOL, err_msg=tag)
        dx = dx.cpu().numpy().astype(np.float64)
        assert np.abs(dx - dxo).max() <= 2e-4 * np.abs(dxo).max() + 1e-9, (tag, np.abs(dx - dxo).max() / np.abs(dxo).max())
        assert np.linalg.norm(dx - dxo) <= 1e-4 * np.linalg.norm(dxo), tag
        for got, want in ((dg.cpu().numpy(), dgo), (db.cpu().numpy(), dbo)):
            assert np.linalg.norm(got - want) <= 2e-4 * np.linalg.norm(want) + 1e-7, (tag, np.linalg.norm(got - want) / np.linalg.norm(want))
    # rows of frames beyond an utterance's length carry no gradient: dx there is exactly zero
    dx3 = dxf.reshape(T, B, V).cpu().numpy()
    for b in range(B):
        assert not dx3[xl[b]:, b].any()


# ---------------------------------------------------------------------------------------------- c. prefetch residues
def _residue_case(T, B, V, gram, xl, seed):
    rs = np.random.RandomState(seed)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    uni = _labels(rs, B, 2, 1, 7)
    big = _bigrams(rs, B, 2, 7, V, p_absent=0.5) if gram else None
    tl = np.minimum(2, xl).astype(np.int32)
    return xs, uni, big, xl.astype(np.int32), tl


@KINDS
def test_every_residue_of_the_prefetch_loops(device, gram):
    """the one-node sweep runs whole blocks of PF = 4 steps and a tail of x_len % 4 with clamped prefetch indices
    (min(t + PF, xl - 1), max(xl - 2 - j, 0)): x_len = 1 .. 11, one utterance each, l_len = min(2, x_len)"""
    T = B = 11
    case = _residue_case(T, B, 13, gram, np.arange(1, B + 1), seed=5)
    want = _oracle_no(*case)
    assert (want[0] < INFEASIBLE).all()
    _compare(device, *case, want, "residues 1..11")


@KINDS
@pytest.mark.parametrize("T", [4, 5, 8])
def test_whole_prefetch_blocks(device, gram, T):
    """x_len = T for every utterance: whole blocks and no tail (4, 8), one block and a tail of one (5)"""
    B = 11
    case = _residue_case(T, B, 13, gram, np.full(B, T), seed=6 + T)
    _compare(device, *case, _oracle_no(*case), "whole blocks T=%d" % T)


# ---------------------------------------------------------------------------------------------- d. more than 1024 path nodes
def _long_case(L, T, B, gram, seed):
    V = 37
    rs = np.random.RandomState(seed)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    uni = _labels(rs, B, L, 1, 20 if gram else V)
    big = _bigrams(rs, B, L, 20, V) if gram else None
    xl = np.full(B, T, np.int32)
    tl = np.full(B, L, np.int32)
    if B > 1:               # a short path in a wide padded lattice: the sweep runs over mostly dead nodes
        tl[1] = L // 2
        xl[1] = int(0.65 * T)
    return xs, uni, big, xl, tl


@pytest.mark.parametrize("L,gram", [(511, False), (512, False), (600, False), (341, True), (342, True), (400, True)])
def test_both_sides_of_the_one_node_strided_switch(device, L, gram):
    """lattice_kernel takes one node per thread up to 1024 padded path nodes (CTC L = 511, Gram-CTC L = 341: Sp = 1024) and
    several nodes per thread above (L = 512 / 342: Sp = 1088).  x_len[0] = T ~ 1.15 L leaves the alignment little room."""
    S = (3 if gram else 2) * L + 1
    Sp = (S + 63) // 64 * 64
    assert (Sp <= 1024) == (L in (511, 341))
    case = _long_case(L, int(round(1.15 * L)), 2, gram, seed=L)
    want = _oracle_no(*case)
    assert (want[0] < INFEASIBLE).all()
    _compare(device, *case, want, "L=%d %s" % (L, "gram" if gram else "ctc"))


def test_sweep_with_more_than_48_kb_of_lds(device):
    """CTC L = 1300: Sp = 2624, 16 (Sp + 16) + 4 (Sp + 8) = 52,768 B of LDS, above the 48 KB a launch gets without asking"""
    case = _long_case(1300, 1400, 1, False, seed=1300)
    want = _oracle_no(*case)
    assert (want[0] < INFEASIBLE).all()
    _compare(device, *case, want, "L=1300")


# ---------------------------------------------------------------------------------------------- e. the size bound
def _lds_bytes(L, gram):
    S = (3 if gram else 2) * L + 1
    Sp = (S + 63) // 64 * 64
    return 16 * (Sp + 16) + 4 * (Sp + 8)                 # asr_ctc_forward_lse: two double rows and the mask row, with their guards


def _bound_case(L, gram):
    T, B, V = 8, 1, 16
    rs = np.random.RandomState(L)
    xs = rs.randn(T, B, V).astype(np.float32)
    uni = _labels(rs, B, L, 1, 9)
    big = _bigrams(rs, B, L, 9, V) if gram else None
    return xs, uni, big, np.array([T], np.int32), np.array([L], np.int32)


@pytest.mark.parametrize("L,gram", [(3807, False), (2538, True)], ids=["ctc", "gram"])
def test_largest_transcript_is_accepted_and_the_next_refused(device, L, gram):
    """the sweep keeps its state in LDS and refuses what needs more than 150 KB.  The largest Lmax inside the bound launches
    (T = 8 frames: no path, so loss 1e10 and the softmax as gradient -- the 150 KB launch without a long sweep); one more label
    raises, through the public function and through the raw entry point, which then leaves its output alone."""
    from asr import _lib
    assert _lds_bytes(L, gram) <= 150 * 1024 < _lds_bytes(L + 1, gram)
    assert _lds_bytes(L, gram) == 152608 and _lds_bytes(L + 1, gram) == 153888
    case = _bound_case(L, gram)
    want = _oracle_no(*case)
    assert want[0][0] == INFEASIBLE
    _compare(device, *case, want, "Lmax=%d" % L)
    xs, uni, big, xl, tl = _bound_case(L + 1, gram)
    with pytest.raises(_lib.AsrHipError):
        _run(device, xs, uni, big, xl, tl, "no")
    # raw ABI: refused before anything is launched
    lib = _lib.lib()
    T, B, V = xs.shape
    d = lambda a: None if a is None else torch.tensor(a, device=device)         # noqa: E731
    x, u, g, dxl, dtl = d(xs), d(uni), d(big), d(xl), d(tl)
    nbytes = lib.asr_ctc_workspace_bytes(T, B, V, L + 1, int(gram))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    loss_b = torch.full((B,), 7.0, device=device)
    loss_m = torch.full((), 7.0, device=device)
    p = _lib.ptr
    rc = lib.asr_ctc_forward_lse(_lib.stream(), p(x), p(u), p(g), p(dxl), p(dtl), T, B, V, L + 1, 0, p(loss_b), p(loss_m), p(ws),
                                 nbytes, None)
    torch.cuda.synchronize()
    assert rc == -3                                     # ASR_ERR_UNSUPPORTED
    assert (loss_b == 7.0).all() and loss_m.item() == 7.0 and not ws.any()


# ---------------------------------------------------------------------------------------------- f. occupancy chunks
CHUNK_LABELS = {8200: [[8191, 8192, 8199, 3, 8192, 8192, 100, 8191], [8199, 8191, 7, 8192, 1, 8199, 8199, 2]],
                16390: [[8191, 8192, 16383, 16384, 16389, 16389, 3, 8199], [16384, 8191, 16389, 8192, 16383, 5, 16384, 8199]]}


@functools.lru_cache(maxsize=None)
def _chunk_case(V):
    T, B = 40, 2
    rs = np.random.RandomState(V)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    uni = np.array(CHUNK_LABELS[V], np.int32)
    return xs, uni, None, np.array([T, 33], np.int32), np.array([8, 7], np.int32)


@pytest.mark.parametrize("V", [8200, 16390])
def test_labels_in_every_occupancy_chunk(device, V):
    """grad_kernel scatters the occupancy in chunks of 8192 vocabulary entries: labels on both sides of every chunk border
    (8191 | 8192, 16383 | 16384), the last id of the vocabulary, a label repeated inside an utterance and shared between the
    two.  V = 8200 takes the float4 rows, V = 16390 the scalar ones."""
    case = _chunk_case(V)
    _compare(device, *case, _oracle_no(*case), "V=%d" % V)


def test_labels_beyond_the_first_chunk_in_the_nbest_scorer(device):
    """csrc/ctc_nbest.hip's grad_kernel has its own chunk loop; the hypotheses of tests/test_ctc_nbest_gpu.py stay below id 119"""
    from asr.loss import ctc_nbest_logp
    V = 8200
    xs, uni, _, xl, tl = _chunk_case(V)
    T, B, N = xs.shape[0], xs.shape[1], 2
    hyps = np.stack([uni, uni[::-1, ::-1]], axis=1).astype(np.int32)             # (B, N, L)
    hyp_len = np.array([[8, 6], [7, 8]], np.int32)
    gy = np.array([[0.8, -0.6], [-1.0, 0.5]], np.float32)
    logp64, grads = nbest_ref.nbest_logp_grad(xs, hyps, hyp_len, xl)
    assert np.isfinite(logp64).all()
    x = torch.tensor(xs, device=device, requires_grad=True)
    d = lambda a: torch.tensor(a, device=device)        # noqa: E731
    logp = ctc_nbest_logp(x, d(hyps), d(hyp_len), 0, d(xl))
    logp.backward(d(gy))
    np.testing.assert_allclose(logp.detach().cpu().numpy(), logp64, rtol=LOSS_RTOL)
    got = x.grad.cpu().numpy()
    assert np.isfinite(got).all() and not got[xl[1]:, 1].any()
    want, mag = nbest_ref.weighted_grad(grads, gy.astype(np.float64), B, N, T, V)
    bound = _nbest_grad_bound(np.abs(gy.astype(np.float64)).sum(axis=1), mag)
    err = np.abs(got - want)
    assert (err <= bound).all(), (err / bound).max()


# ---------------------------------------------------------------------------------------------- g. numerics
NUM_T, NUM_B, NUM_V, NUM_L = 40, 3, 11, 5
MASKED = (5, 9, 10)                      # vocabulary entries at -inf on every frame
DERIVED = ("x40", "offset 1e4", "one-hot")
NUMERICS = ("x8", "x40", "equal rows", "offset 1e4", "masked", "run of 20", "one-hot")


def _numerics_case(name, gram):
    T, B, V, L = NUM_T, NUM_B, NUM_V, NUM_L
    rs = np.random.RandomState(17 + NUMERICS.index(name))
    uni = _labels(rs, B, L, 1, 5)                         # ids 1 .. 4: none of MASKED
    big = np.array([[-1, 6, -1, 7, 8], [-1, -1, -1, -1, -1], [-1, 9, 6, -1, 7]], np.int32)      # (utterance 2: a masked bigram)
    xl = np.array([T, 31, 23], np.int32)
    tl = np.array([L, L, 4], np.int32)
    z = rs.randn(T, B, V)
    if name == "x8":
        xs = z * 8
    elif name == "x40":
        xs = z * 40
    elif name == "equal rows":
        xs = np.broadcast_to(rs.randn(T, B, 1) * 3, (T, B, V)).copy()
    elif name == "offset 1e4":
        xs = z + 1e4
    elif name == "masked":
        xs = z
        xs[:, :, list(MASKED)] = -np.inf
        uni[1, 2] = MASKED[0]                             # in utterance 1's transcript (no bigram bridges it): no path
    elif name == "run of 20":
        L = 20
        uni = np.array([[3] * L, [2] * L, [4] * L], np.int32)
        big = np.array([[-1] * L, [-1] + [7] * (L - 1), [-1] * L], np.int32)
        xl = np.array([2 * L - 1, T, 30], np.int32)      # exactly one path; a few; l_len = 10 in 30 frames
        tl = np.array([L, L, 10], np.int32)
        xs = z * 1.5
    else:                                                 # one-hot: every frame all but decided, mostly for the blank
        xs = z
        hot = np.where(rs.rand(T, B) < 0.6, 0, rs.randint(0, V, size=(T, B)))
        np.put_along_axis(xs, hot[:, :, None], 30.0, axis=2)
    return xs.astype(np.float32), uni, (big if gram else None), xl, tl


@KINDS
@pytest.mark.parametrize("name", NUMERICS)
def test_numerics(device, name, gram):
    case = _numerics_case(name, gram)
    lo, G = want = _oracle_no(*case)
    assert np.array_equal(lo == INFEASIBLE, np.arange(NUM_B) == (1 if name == "masked" else -1))
    loss_abs = grad_abs = 0.0
    if name in DERIVED:
        lo32, G32 = _oracle_no(*case, f32_logits=True)
        loss_abs, grad_abs = 4.0 * np.abs(lo - lo32).max(), 4.0 * np.abs(G - G32).max()
    wl, wg = _compare(device, *case, want, "numerics %s" % name, loss_abs, grad_abs)
    print("NUMERICS %-10s %-4s loss floor %.3g (fixed: %.3g)  gradient floor %.3g (fixed: %.3g)  worst loss %.3g  worst gradient %.3g"
          % (name, "gram" if gram else "ctc", loss_abs, LOSS_RTOL * np.abs(lo[lo < INFEASIBLE]).min(), grad_abs, GRAD_ATOL, wl, wg))


# ---------------------------------------------------------------------------------------------- h. labels outside the vocabulary
@KINDS
def test_labels_outside_the_vocabulary(device, gram):
    """an id outside [0, V) inside l_len makes its node dead (prep_kernel), so the utterance has no path: loss 1e10, gradient
    softmax * scale, and the other utterances are what the oracle gives without it.  An outside id among the bigrams is an
    absent bigram.  (A property: the oracle is not asked to index out of range.)"""
    T, B, V, L = 20, 4, 9, 4
    rs = np.random.RandomState(8)
    xs = (rs.randn(T, B, V) * 1.5).astype(np.float32)
    uni = _labels(rs, B, L, 1, 5)
    big = np.array([[-1, 6, 7, 8], [-1, -1, -1, -1], [-1, V + 2, 6, -7], [-1, -1, -1, 8]], np.int32)
    uni[1, 1], uni[3, 2] = -1, V
    xl = np.array([T, 15, 17, T], np.int32)
    tl = np.array([L, L, L, 3], np.int32)
    good, bad = [0, 2], [1, 3]
    big_clean = np.where((big < 0) | (big >= V), -1, big).astype(np.int32)
    lo_g, G_g = _oracle_no(xs[:, good], uni[good], big_clean[good] if gram else None, xl[good], tl[good])
    assert (lo_g < INFEASIBLE).all()
    lo = np.full(B, INFEASIBLE)
    G = _softmax64(xs)
    for b in bad:
        G[xl[b]:, b] = 0.0
    lo[good], G[:, good] = lo_g, G_g
    _compare(device, xs, uni, big if gram else None, xl, tl, (lo, G), "labels outside the vocabulary")
