"""CTC prefix beam search, host side: the float64 restatement (tests/ctc_beam_reference.py) against an exhaustive enumeration
of every path and against the CTC oracle, and the two C entries in both libraries (no GPU)."""
import ctypes
import os

import numpy as np

import ctc_beam_reference as ref
from conftest import PKG
from oracle import ctc as octc

EXHAUSTIVE, exhaustive_logits = ref.EXHAUSTIVE, ref.exhaustive_logits


def oracle_scores(x, labellings, blank=0):
    """-ctc_loss of every (non-empty: the oracle's lattice needs one label) labelling over the same logits (oracle/ctc.py,
    float64, reduce='no')"""
    n = len(labellings)
    L = max(1, max(len(lab) for lab in labellings))
    labels = np.zeros((n, L), np.int32)
    for i, lab in enumerate(labellings):
        labels[i, :len(lab)] = lab
    lens = np.array([len(lab) for lab in labellings], np.int32)
    xs = np.repeat(np.asarray(x, np.float32)[:, None, :], n, axis=1)
    loss, _ = octc.ctc_loss_grad(xs, labels, blank, None, lens, "no")
    return -np.asarray(loss, np.float64)


def test_restatement_is_exact_when_the_beam_holds_everything():
    """top_k = V - 1 and a beam wider than the number of feasible prefixes: the restatement returns exactly the feasible
    labellings, each with log p(labelling | x) -- the enumeration of all V^T paths and, for every non-empty labelling, minus
    the oracle's CTC loss, to 1e-12.  The empty labelling has one path, all blanks: its score is also that path's sum."""
    for (T, V, W, seed), count in EXHAUSTIVE:
        x = exhaustive_logits(T, V, seed)
        got = ref.beam_search(x, W, V - 1)
        exact = ref.enumerate_paths(x)
        labs = [lab for lab, _ in got]
        assert len(exact) == count, (T, V, seed, len(exact))
        assert len(got) == count and len(set(labs)) == count and set(labs) == set(exact), (T, V, seed)
        scores = np.array([s for _, s in got])
        assert np.all(np.isfinite(scores))
        assert np.all(np.diff(scores) <= 0)
        want = np.array([exact[lab] for lab in labs])
        assert np.max(np.abs(scores - want)) <= 1e-12, (T, V, seed, np.max(np.abs(scores - want)))
        nonempty = [i for i, lab in enumerate(labs) if lab]
        orc = oracle_scores(x, [labs[i] for i in nonempty])
        assert np.max(np.abs(scores[nonempty] - orc)) <= 1e-12, (T, V, seed, np.max(np.abs(scores[nonempty] - orc)))
        blank_path = float(ref.log_softmax64(x)[:, 0].sum())
        assert abs(scores[labs.index(())] - blank_path) <= 1e-12


def test_restatement_prunes_to_a_lower_bound():
    """with a narrow beam each kept score is a lower bound on the exact log-probability of its labelling"""
    for (T, V, _, seed), _ in EXHAUSTIVE[:4]:
        x = exhaustive_logits(T, V, seed)
        exact = ref.enumerate_paths(x)
        got = ref.beam_search(x, 3, 1)
        assert 1 <= len(got) <= 3
        for lab, s in got:
            assert s <= exact[lab] + 1e-12


def _entries(path):
    lib = ctypes.CDLL(path)
    for name in ("asr_ctc_beam_workspace_bytes", "asr_ctc_beam_search"):
        assert hasattr(lib, name), (path, name)
    q = lib.asr_ctc_beam_workspace_bytes
    q.restype = ctypes.c_size_t
    q.argtypes = [ctypes.c_int] * 5
    return q


def test_entries_exist_in_both_libraries():
    """both builds export the two entries; the workspace query runs on the host and covers the candidate table and the
    prefix table"""
    for so in ("libasr_hip.so", "libasr_hip_f16.so"):
        path = os.path.join(PKG, so)
        assert os.path.isfile(path), "run `make -C chainer-speech-recognition_amd`"
        q = _entries(path)
        T, B, V, W, K = 1000, 16, 3000, 16, 16
        n = q(T, B, V, W, K)
        assert n >= T * B * (3 * 4 + 2 * K * 4 + W * 8)
        assert q(T, B, V, W, 64) > n                         # the candidate table grows with top_k
        assert q(5, 1, 3, 4, 16) == q(5, 1, 3, 4, 2)         # top_k above V - 1 acts as V - 1
        assert q(0, B, V, W, K) == 0 and q(T, B, V, 0, K) == 0

