"""CTC / Gram-CTC forced alignment, host side: the float64 restatement (tests/ctc_align_reference.py) against a brute-force search
over every path and against the CTC oracle, and the two C entries in both libraries (no GPU)."""
import ctypes
import os

import numpy as np
import pytest

import ctc_align_reference as ref
from conftest import PKG
from oracle import ctc as octc


def _check(x, uni, big, L, blank=0):
    got = ref.align_one(x, uni, big, None, L, blank)
    best, frames = ref.brute_force(x, uni, big, L, blank)
    if frames is None:
        assert got["score"] == -np.inf and got["n_tokens"] == 0 and np.all(got["frames"] == blank)
        return False
    assert np.array_equal(got["frames"], frames), (got["frames"], frames)
    assert abs(got["score"] - best) <= 1e-9
    # the outputs derived from the path are consistent with it
    n = got["n_tokens"]
    lp = octc.log_softmax(np.asarray(x, np.float64), axis=1)
    covered = np.zeros(len(frames), bool)
    for k in range(n):
        s, e = got["starts"][k], got["ends"][k]
        assert s < e and np.all(frames[s:e] == got["tokens"][k])
        assert abs(got["token_logp"][k] - lp[s:e, got["tokens"][k]].sum()) <= 1e-9
        covered[s:e] = True
    assert np.all(frames[~covered] == blank)
    assert np.all(got["tokens"][n:] == blank) and not got["ends"][n:].any()
    if big is None:
        assert n == L and list(got["tokens"][:n]) == list(uni[:L]) and list(got["positions"][:n]) == list(range(L))
    else:
        assert (L + 1) // 2 <= n <= L
        p = 0
        for k in range(n):              # the tokens spell the unigrams, position by position
            assert got["positions"][k] == p
            if got["tokens"][k] == uni[p]:
                p += 1
            else:
                assert got["tokens"][k] == big[p + 1]
                p += 2
        assert p == L
    # the best path is one of the paths the loss sums over
    if L > 0:
        if big is None:
            loss, _ = octc.ctc_loss_grad(x[:, None, :], uni[None, :], blank, None, np.array([L]), "no")
        else:
            loss, _ = octc.gram_ctc_loss_grad(x[:, None, :], uni[None, :], big[None, :], blank, None, np.array([L]), "no")
        assert got["score"] <= -loss[0] + 1e-9
    return True


def test_restatement_equals_brute_force_ctc():
    cases = ref.tiny_ctc_cases()
    feasible = sum(_check(x, u, None, L) for x, u, L in cases)
    assert 0 < feasible < len(cases)            # the infeasible case is among them


def test_restatement_equals_brute_force_gram():
    cases = ref.tiny_gram_cases()
    used_bigram = 0
    feasible = 0
    for x, u, g, L in cases:
        if _check(x, u, g, L):
            feasible += 1
            got = ref.align_one(x, u, g, None, L, 0)
            used_bigram += bool(np.any(got["tokens"][:got["n_tokens"]] >= 3))
    assert 0 < feasible < len(cases)
    assert used_bigram >= 3                     # the bigram branch of the lattice is exercised


def test_restatement_ragged_batch_and_empty_transcript():
    rs = np.random.RandomState(5)
    xs = rs.randn(6, 3, 4).astype(np.float32)
    uni = np.array([[1, 2, 3], [2, 2, 1], [3, 1, 1]], np.int32)
    out = ref.align_batch(xs, uni, None, np.array([6, 4, 0]), np.array([3, 0, 1]), 0)
    assert out["n_tokens"].tolist() == [3, 0, 0]
    lp = octc.log_softmax(xs[:4, 1].astype(np.float64), axis=1)
    assert abs(out["score"][1] - lp[:, 0].sum()) <= 1e-12 and np.all(out["frames"][1] == 0)      # L = 0: all blank
    assert out["score"][2] == -np.inf                                                             # no frames: infeasible
    best, frames = ref.brute_force(xs[:, 0], uni[0], None, 3, 0)
    assert np.array_equal(out["frames"][0], frames)


def test_tie_rule_of_the_restatement():
    """all-zero logits: every feasible path ties.  Smallest offset first means 'stay as long as possible': the path leaves the
    leading blank as late as it can; the largest final node is the trailing blank."""
    out = ref.align_one(np.zeros((6, 3), np.float32), np.array([1, 2], np.int32), None, None, 2, 0)
    assert out["frames"].tolist() == [1, 2, 0, 0, 0, 0]
    out = ref.align_one(np.zeros((6, 5), np.float32), np.array([1, 2], np.int32), np.array([-1, 3], np.int32), None, 2, 0)
    assert out["n_tokens"] >= 1 and out["score"] > -np.inf


@pytest.mark.parametrize("lib", ["libasr_hip.so", "libasr_hip_f16.so"])
def test_both_libraries_export_the_entries(lib):
    handle = ctypes.CDLL(os.path.join(PKG, lib))
    assert hasattr(handle, "asr_ctc_align") and hasattr(handle, "asr_ctc_align_workspace_bytes")
    q = handle.asr_ctc_align_workspace_bytes
    q.restype, q.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
    loss_q = handle.asr_ctc_workspace_bytes
    loss_q.restype, loss_q.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
    for gram in (0, 1):
        n = q(1000, 32, 3000, 120, gram)        # runs on the host, no device
        assert 0 < n < loss_q(1000, 32, 3000, 120, gram) // 3, (n, loss_q(1000, 32, 3000, 120, gram))
    assert q(0, 32, 3000, 120, 0) == 0


def test_binding_lists_the_entries():
    from asr import _lib
    assert "asr_ctc_align" in _lib.SIGNATURES and "asr_ctc_align_workspace_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["asr_ctc_align"][1]) == 21


def test_cpu_tensors_are_refused():
    import torch
    from asr import _lib, loss
    x = torch.zeros(4, 1, 3)
    t = torch.ones(1, 2, dtype=torch.int32)
    with pytest.raises(_lib.AsrHipError):
        loss.ctc_align(x, t, 0)
    with pytest.raises(_lib.AsrHipError):
        loss.gram_ctc_align(x, t, torch.full((1, 2), -1, dtype=torch.int32), 0)
    with pytest.raises(TypeError):
        loss.ctc_align(x, t.long(), 0)
    assert loss.Alignment._fields == ("frames", "tokens", "positions", "starts", "ends", "token_logp", "n_tokens", "score")
