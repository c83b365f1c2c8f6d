"""The CPU oracle against the reference's golden vectors (and torch CPU) -- no GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ctc as octc


def _load_gram_ctc(golden_dir):
    if golden_dir not in sys.path:
        sys.path.insert(0, golden_dir)
    import gram_ctc_fixture
    return gram_ctc_fixture.load(golden_dir)


def _cases(golden_dir):
    g = _load_gram_ctc(golden_dir)
    return g, [str(n) for n in g["names"]]


def _get(g, n):
    return [g["%s.%s" % (n, k)] for k in ("xs", "uni", "big", "xl", "tl", "loss", "gy", "gx")] + [str(g[n + ".reduce"])]


@pytest.mark.parametrize("name", ["ctc_small", "ctc_noreduce", "ctc_full", "ctc_v300", "ctc_v3000", "ctc_len1",
                                  "gram_mixed", "gram_all", "gram_repeat2", "gram_v3000", "gram_len1"])
def test_gram_oracle_matches_reference(golden_dir, name):
    g, names = _cases(golden_dir)
    assert name in names
    xs, uni, big, xl, tl, loss, gy, gx, red = _get(g, name)
    l, gr = octc.gram_ctc_loss_grad(xs, uni, big, 0, xl, tl, red, gy)
    np.testing.assert_allclose(l, loss, rtol=1e-5)
    # the reference accumulates in float32 (error grows with T and V); the oracle is float64
    np.testing.assert_allclose(gr, gx, rtol=2e-3, atol=2e-4)


@pytest.mark.parametrize("name", ["ctc_small", "ctc_noreduce", "ctc_full", "ctc_v300", "ctc_len1"])
def test_standard_ctc_is_gram_with_no_bigrams(golden_dir, name):
    g, _ = _cases(golden_dir)
    xs, uni, big, xl, tl, loss, gy, gx, red = _get(g, name)
    assert (big[:, :1] == -1).all()
    l, gr = octc.ctc_loss_grad(xs, uni, 0, xl, tl, red, gy)
    np.testing.assert_allclose(l, loss, rtol=1e-5)
    np.testing.assert_allclose(gr, gx, rtol=2e-3, atol=2e-4)


def test_standard_ctc_matches_torch_cpu():
    rs = np.random.RandomState(5)
    T, B, V, L = 40, 5, 17, 8
    xs = rs.randn(T, B, V).astype(np.float32) * 2
    lab = rs.randint(1, V, size=(B, L)).astype(np.int32)
    lab[:, 3] = lab[:, 2]
    tl = rs.randint(1, L + 1, size=B).astype(np.int32)
    xl = rs.randint(2 * L + 2, T + 1, size=B).astype(np.int32)
    loss, grad = octc.ctc_loss_grad(xs, lab, 0, xl, tl, "no")
    x = torch.tensor(xs, dtype=torch.float64, requires_grad=True)
    lt = torch.nn.functional.ctc_loss(torch.log_softmax(x, 2), torch.tensor(lab, dtype=torch.long), torch.tensor(xl, dtype=torch.long),
                                      torch.tensor(tl, dtype=torch.long), blank=0, reduction="none")
    lt.sum().backward()
    np.testing.assert_allclose(loss, lt.detach().numpy(), rtol=1e-9)
    np.testing.assert_allclose(grad, x.grad.numpy(), atol=1e-9)


def test_connection_matrices_match_reference(golden_dir):
    c = np.load(os.path.join(golden_dir, "gram_ctc_connection.npz"))
    for b in range(c["uni"].shape[0]):
        m = octc.gram_connection_matrix(c["uni"][b], c["big"][b], c["tl"][b], c["fwd"].shape[1])
        assert np.array_equal(m, c["fwd"][b])


def test_infeasible_alignment_is_flagged():
    xs = np.zeros((2, 1, 5), dtype=np.float32)          # T = 2 < 2 L + 1
    loss, grad = octc.ctc_loss_grad(xs, np.array([[1, 1, 2]], dtype=np.int32), 0, None, None, "no")
    assert loss[0] >= 1e9


# ---------------------------------------------------------------------------------------------- brute force over all labellings
def _collapse(path, blank=0):
    """CTC's many-to-one map: merge runs of one symbol, then drop the blanks"""
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def _decompositions(uni, big):
    """every token sequence that spells the transcript: position i is covered by uni[i] alone, or positions (i-1, i) by
    big[i] where it is not -1 (asr/loss/gram_ctc.py:24-32).  Unigram and bigram ids are disjoint in these cases, so two
    decompositions never give the same token sequence."""
    L = len(uni)
    out = []

    def rec(i, acc):
        if i == L:
            out.append(tuple(acc))
            return
        rec(i + 1, acc + [int(uni[i])])
        if i + 1 < L and big[i + 1] != -1:
            rec(i + 2, acc + [int(big[i + 1])])
    rec(0, [])
    return set(out)


def _brute_force_loss(xs, targets):
    """-log of the summed probability of all V^T frame labellings that collapse to one of ``targets``; xs (T, V) float64"""
    import itertools
    T, V = xs.shape
    assert T <= 6 and V <= 4
    p = np.exp(octc.log_softmax(xs, axis=1))
    total = 0.0
    for path in itertools.product(range(V), repeat=T):
        if _collapse(path) in targets:
            total += float(np.prod(p[np.arange(T), list(path)]))
    return -np.log(total) if total > 0.0 else 1e10


#              name                                T  uni           big              finite under (CTC, Gram-CTC)
BRUTE = [("empty transcript",                      3, [],           [],              (True, True)),
         ("one label, one frame",                  1, [1],          [-1],            (True, True)),
         ("T == L, no repeats",                    3, [1, 2, 1],    [-1, -1, -1],    (True, True)),
         ("T == L, a bigram alive",                3, [1, 2, 1],    [-1, 3, -1],     (True, True)),
         ("T == L - 1: only through the bigram",   2, [1, 2, 1],    [-1, 3, -1],     (False, True)),
         ("T == L - 2",                            1, [1, 2, 1],    [-1, 3, -1],     (False, False)),
         ("T == L + repeats",                      4, [1, 1, 2],    [-1, -1, -1],    (True, True)),
         ("T == L + repeats - 1",                  3, [1, 1, 2],    [-1, -1, -1],    (False, False)),
         ("all labels identical, T = 2L - 1",      5, [2, 2, 2],    [-1, -1, -1],    (True, True)),
         ("all labels identical, T = 2L - 2",      4, [2, 2, 2],    [-1, -1, -1],    (False, False)),
         ("identical labels, last bigram alive",   4, [1, 1, 1],    [-1, -1, 3],     (False, True)),
         ("identical labels and bigrams",          5, [1, 1, 1, 1], [-1, 3, -1, 3],  (False, True)),
         ("identical labels and bigrams, T = 6",   6, [1, 1, 1, 1], [-1, 3, 2, 3],   (False, True)),
         ("longer than needed",                    6, [1, 2],       [-1, 3],         (True, True))]


@pytest.mark.parametrize("name,T,uni,big,finite", BRUTE, ids=[c[0] for c in BRUTE])
def test_oracle_against_brute_force_enumeration(name, T, uni, big, finite):
    """The lattice (edges, final nodes, the empty path) against its definition: the sum over ALL V^T frame labellings (T <= 6,
    V <= 4) that collapse to the transcript under CTC, or to one of its decompositions under Gram-CTC.  Both sides are float64:
    1e-12 relative.  The edges: empty transcript, one label in one frame, exactly as many frames as the shortest path needs, one
    fewer (1e10), all labels identical."""
    V, L = 4, len(uni)
    rs = np.random.RandomState(T * 31 + L)
    xs = rs.randn(T, 1, V) * 2.0
    Lmax = max(L, 1)                     # (the label rows have at least one column; label_length says how much counts)
    u = np.zeros((1, Lmax), np.int32)
    g = np.full((1, Lmax), -1, np.int32)
    u[0, :L], g[0, :L] = uni, big
    tl = np.array([L], np.int32)
    want_ctc = _brute_force_loss(xs[:, 0], {tuple(uni)})
    want_gram = _brute_force_loss(xs[:, 0], _decompositions(uni, big))
    assert (want_ctc < 1e10, want_gram < 1e10) == finite           # the case is what its name says
    got_ctc, _ = octc.ctc_loss_grad(xs, u, 0, None, tl, "no")
    got_gram, _ = octc.gram_ctc_loss_grad(xs, u, g, 0, None, tl, "no")
    got_none, _ = octc.gram_ctc_loss_grad(xs, u, np.full_like(g, -1), 0, None, tl, "no")
    for got, want in ((got_ctc[0], want_ctc), (got_gram[0], want_gram), (got_none[0], want_ctc)):
        if want == 1e10:
            assert got == 1e10
        else:
            assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_oracle_accepts_an_utterance_without_frames():
    """input_length 0: infeasible, and there is no gradient row to fill; the other utterance is what it is alone"""
    rs = np.random.RandomState(2)
    xs = rs.randn(5, 2, 4)
    lab = np.array([[1, 2], [3, 1]], np.int32)
    for tl0 in (2, 0):
        xl, tl = np.array([0, 5], np.int32), np.array([tl0, 2], np.int32)
        gy = np.array([0.7, -1.3])
        for fn, args in ((octc.ctc_loss_grad, (lab,)), (octc.gram_ctc_loss_grad, (lab, np.full_like(lab, -1)))):
            loss, grad = fn(xs, *args, 0, xl, tl, "no", gy)
            assert loss[0] == 1e10 and not grad[:, 0].any()
            l1, g1 = fn(xs[:, 1:], *[a[1:] for a in args], 0, xl[1:], tl[1:], "no", gy[1:])
            assert loss[1] == l1[0] and np.array_equal(grad[:, 1], g1[:, 0])


def test_float32_logit_option_only_rounds():
    """f32_logits models the device's storage of x - lse: same results to float32's precision, and not the same bits"""
    rs = np.random.RandomState(3)
    xs = (rs.randn(12, 2, 6) + 1e4).astype(np.float32)
    lab = rs.randint(1, 6, size=(2, 3)).astype(np.int32)
    l64, g64 = octc.ctc_loss_grad(xs, lab, 0, None, None, "no")
    l32, g32 = octc.ctc_loss_grad(xs, lab, 0, None, None, "no", None, f32_logits=True)
    assert 0 < np.abs(l64 - l32).max() <= 12 * 2.0 ** -11          # 12 frames, half an ulp of a float32 near 1e4 each
    assert 0 < np.abs(g64 - g32).max() <= 1e-2
