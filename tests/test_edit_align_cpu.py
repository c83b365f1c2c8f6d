"""CPU: the restatement of the edit alignment and of MBR decoding (tests/edit_align_reference.py) against definitions that do not
share its code, the ABI of the five new entries, and their workspace queries on the host.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np

import edit_align_reference as ref
from conftest import PKG, ROOT
from oracle import text as otext

ENTRIES = ["asr_edit_align_workspace_bytes", "asr_edit_align", "asr_nbest_pairwise_distance", "asr_nbest_consensus_workspace_bytes",
           "asr_nbest_consensus"]


def _short_strings(max_len=4, symbols=(1, 2)):
    for n in range(max_len + 1):
        for s in itertools.product(symbols, repeat=n):
            yield list(s)


def test_reference_distance_equals_the_oracle():
    rs = np.random.RandomState(0)
    for _ in range(60):
        n, m, v = rs.randint(0, 40), rs.randint(0, 40), rs.choice([2, 3, 50])
        r, h = rs.randint(1, v + 1, size=n).tolist(), rs.randint(1, v + 1, size=m).tolist()
        want = otext.levenshtein(r, h)
        assert ref.table(r, h)[-1, -1] == want
        assert ref.align(r, h)[0] == want


def test_reference_paths_exhaustively():
    """every pair of strings of length <= 4 over 2 symbols (31 x 31): the maps are a monotone alignment, its cost is the distance,
    H + S + D = n, H + S + I = m, S + D + I = distance -- and the counts carried forward with the table (what the kernel does
    without back-pointers) are the trace-back's"""
    strings = list(_short_strings())
    assert len(strings) == 31
    for r in strings:
        for h in strings:
            dist, S, D, I, r2h, h2r = ref.align(r, h)
            n, m = len(r), len(h)
            assert dist == otext.levenshtein(r, h) == S + D + I
            pairs = [(i, j) for i, j in enumerate(r2h) if j >= 0]
            assert pairs == sorted(pairs) and all(a[0] < b[0] and a[1] < b[1] for a, b in zip(pairs, pairs[1:]))      # monotone
            assert all(h2r[j] == i for i, j in pairs) and sum(v >= 0 for v in h2r) == len(pairs)                    # one map's inverse
            H = sum(r[i] == h[j] for i, j in pairs)
            assert S == len(pairs) - H and D == n - len(pairs) and I == m - len(pairs)
            assert H + S + D == n and H + S + I == m
            assert (len(pairs) - H) + (n - len(pairs)) + (m - len(pairs)) == dist                                  # the path's cost
            assert ref.carried_counts(r, h) == (dist, S, D, I)


def test_reference_pins_the_rule():
    """pairs with several optimal alignments: the rule prefers, walking back, match > substitution > deletion > insertion"""
    a, b = 1, 2
    # ab / ba: two substitutions, or keep either letter with a deletion and an insertion; the rule substitutes twice
    assert ref.align([a, b], [b, a]) == (2, 2, 0, 0, [0, 1], [0, 1])
    # aab / ab: the last a matches (walking back), the first is deleted -- not the other way round
    assert ref.align([a, a, b], [a, b]) == (1, 0, 1, 0, [-1, 0, 1], [1, 2])
    # ab / aab: likewise the insertion lands in front
    assert ref.align([a, b], [a, a, b]) == (1, 0, 0, 1, [1, 2], [-1, 0, 1])
    # ab / bab -> insertion in front; abc / ca: substitution is preferred to deletion where both are optimal
    assert ref.align([a, b], [b, a, b]) == (1, 0, 0, 1, [1, 2], [-1, 0, 1])
    dist, S, D, I, r2h, h2r = ref.align([1, 2, 3], [3, 1])
    assert (dist, S, D, I) == (3, 2, 1, 0) and r2h == [-1, 0, 1] and h2r == [1, 2]
    # empty sides
    assert ref.align([], [a, b]) == (2, 0, 0, 2, [], [-1, -1])
    assert ref.align([a, b], []) == (2, 0, 2, 0, [-1, -1], [])
    assert ref.align([], []) == (0, 0, 0, 0, [], [])


def test_reference_mbr_against_brute_force():
    ids, lens, scores, want = ref.hand_batch()
    for scale in (1.0, 0.5):
        got = ref.mbr(ids, lens, scores, scale)
        for b, (name, hyps, sc, _) in enumerate(ref.HAND_LISTS):
            index, risks = ref.brute_force_mbr(hyps, sc, scale)
            assert got["index"][b] == index, name
            for i, h in enumerate(hyps):
                if h is None:
                    assert got["risk"][b, i] == np.inf and got["posterior"][b, i] == 0.0
                else:
                    assert abs(got["risk"][b, i] - risks[i]) < 1e-12, name
            if index >= 0:
                assert abs(got["posterior"][b].sum() - 1.0) < 1e-12
    got = ref.mbr(ids, lens, scores, 1.0)
    assert list(got["index"]) == list(want)
    names = [name for name, _, _, _ in ref.HAND_LISTS]
    assert got["index"][names.index("runners_up")] != 0 and got["index"][names.index("all_unused")] == -1
    for b, (name, hyps, _, _) in enumerate(ref.HAND_LISTS):           # decisive gaps: the GPU test demands the exact index
        r = np.sort(got["risk"][b][np.isfinite(got["risk"][b])])
        assert len(r) < 2 or r[1] - r[0] > 0.05, name
    # padding of the unused slots of the batch (junk ids, positive lengths) has no say
    assert (got["dist"][names.index("all_unused")] == 0).all() and (got["conf"][names.index("all_unused")] == 0).all()
    # confidence by hand: runners_up picks [1, 5, 3, 6]; 1 and 3 are in every hypothesis, 5 in the two runners-up, 6 only in the pick
    np.testing.assert_allclose(got["conf"][names.index("runners_up")][:4], [1.0, 0.6, 1.0, 0.35], atol=1e-12)


def test_the_five_entries_are_declared_bound_and_exported():
    from asr import _lib
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        for so in ("libasr_hip.so", "libasr_hip_f16.so"):
            assert hasattr(ctypes.CDLL(os.path.join(PKG, so)), name), (so, name)
    from asr import _ops, error
    for fn in ("edit_align", "nbest_pairwise_distance", "nbest_consensus"):
        assert callable(getattr(_ops, fn))
    for fn in ("edit_alignment", "error_counts", "compute_minibatch_error_counts", "mbr_decode"):
        assert callable(getattr(error, fn))


def test_workspace_queries_run_on_the_host():
    from asr import _lib
    lib = _lib.lib()
    for query in (lib.asr_edit_align_workspace_bytes, lib.asr_nbest_consensus_workspace_bytes):
        base = query(7, 33, 65)
        assert base > 0
        assert query(8, 33, 65) > base and query(7, 34, 65) > base and query(7, 33, 66) > base          # grows with each argument
        for empty in ((0, 33, 65), (7, 0, 65), (7, 33, 0), (-1, 33, 65)):
            assert query(*empty) == 0
    assert lib.asr_edit_align_workspace_bytes(3, 2000, 2000) >= 3 * 2000 * 2000 // 4          # at least 2 bits per cell
    assert lib.asr_edit_align_workspace_bytes(70000, 300, 300) > 2 ** 32                       # size_t, not int


def test_null_and_empty_arguments_are_refused_before_any_launch():
    from asr import _lib
    lib = _lib.lib()
    assert lib.asr_edit_align(None, None, None, 4, None, None, 4, 1, None, None, None, None, 0) == -1
    assert lib.asr_nbest_pairwise_distance(None, None, None, 1, 1, 4, None) == -1
    assert lib.asr_nbest_consensus(None, None, None, None, None, 1, 1, 4, None, None, 0) == -1
