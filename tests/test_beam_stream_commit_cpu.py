"""Committing a prefix of a beam search, without a GPU: the properties of tests/beam_commit_reference.py that the device tests lean on,
the measurements behind DESIGN.md section 34, and the host-only size queries of the commit entries."""
import numpy as np
import pytest

import beam_commit_reference as cr
import ctc_beam_reference as ref
import gram_beam_reference as gref

RTOL = 1e-4                                       # tests/test_ctc_beam_gpu.py's


def tol(s):
    return RTOL * max(1.0, abs(s))


def joined(run):
    return [(run["done"] + tail, score) for tail, score in run["tails"]]


GRAM = gref.random_table(12, 4, 7)
CASES = [(120, 12, 8, 6, 1, None), (90, 6, 16, 5, 2, None), (60, 7, 1, 4, 3, None), (120, 12, 8, 6, 1, GRAM), (60, 12, 1, 6, 2, GRAM)]


def logits(T, V, seed):
    return ref.peaky(np.random.RandomState(seed), T, V) if V > 7 else (np.random.RandomState(seed).randn(T, V) * 4).astype(np.float32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T%d_V%d_W%d_K%d_s%d_%s" % (c[:5] + ("ctc" if c[5] is None else "gram",)))
def test_without_commits_it_is_the_restatement_and_auto_commits_change_nothing(case):
    T, V, W, K, seed, gram = case
    x = logits(T, V, seed)
    want = ref.beam_search(x, W, K) if gram is None else gref.beam_search(x, gram, W, K)
    plain = cr.search(x, W, K, (), 0, gram)
    assert plain["done"] == () and plain["tails"] == want and plain["log"] == []
    auto = cr.search(x, W, K, cr.every(T, 10, "auto"), 0, gram)
    assert joined(auto) == want                                  # the same strings with the same float64 scores, in order
    assert all(status == 1 for _, _, status, _, _ in auto["log"])
    assert sum(len(P) for _, P, _, _, _ in auto["log"]) == len(auto["done"])
    if W == 1:
        assert auto["tails"][0][0] == () and auto["done"] == want[0][0]      # one hypothesis: everything is common
    assert auto["longest"] <= plain["longest"]


def test_two_filters_in_a_row_are_the_filter_by_both_and_a_foreign_prefix_is_refused():
    T, V, W, K = 120, 12, 8, 6
    x = logits(T, V, 5)
    for gram in (None, GRAM):
        at60 = cr.search(x[:60], W, K, (), 0, gram)["tails"]
        best = at60[0][0]
        assert len(best) >= 4
        P1, P2 = best[:2], best[2:4]
        two = cr.search(x, W, K, [(60, P1), (60, P2)], 0, gram)
        one = cr.search(x, W, K, [(60, P1 + P2)], 0, gram)
        assert two["done"] == one["done"] == P1 + P2 and two["tails"] == one["tails"]
        assert [entry[2] for entry in two["log"]] == [1, 1]
        # pruning is lossy by design: what is left is the unrestricted beam's entries that start with P, or fewer
        bad = tuple(V - 1 - c for c in best[:3])
        assert all(tail[:3] != bad for tail, _ in at60)
        refused = cr.search(x, W, K, [(60, bad)], 0, gram)
        assert refused["log"][0][2] == 0 and refused["done"] == ()
        assert refused["tails"] == cr.search(x, W, K, (), 0, gram)["tails"]


def test_the_common_prefix_lags_by_almost_the_whole_utterance():
    """the measurement of DESIGN.md section 34: peaky(seed 1), T = 400, V = 40, beam 16, top_k 8.  (frames: tokens of the best
    hypothesis, tokens all 16 hypotheses share)"""
    x = ref.peaky(np.random.RandomState(1), 400, 40)
    run = cr.search(x, 16, 8, lag_at=tuple(range(40, 401, 40)))
    print(run["lag"])
    assert run["lag"] == {40: (6, 0), 80: (17, 0), 120: (25, 0), 160: (32, 0), 200: (36, 0), 240: (42, 1), 280: (51, 1),
                          320: (58, 1), 360: (69, 1), 400: (75, 1)}


def test_committing_the_best_minus_eight_keeps_the_tails_short():
    """the six runs of DESIGN.md section 34: the longest live tail under ("best", 8) every 20 frames, and whether the final best
    hypothesis is the unrestricted search's"""
    got = []
    for seed in (1, 2, 3):
        for T, V, W, K in ((400, 40, 16, 8), (600, 12, 8, 6)):
            x = ref.peaky(np.random.RandomState(seed), T, V)
            run = cr.search(x, W, K, cr.every(T, 20, ("best", 8)))
            got.append((run["longest"], joined(run)[0][0] == ref.beam_search(x, W, K)[0][0]))
    print(got)
    assert got == [(17, True), (17, True), (18, True), (16, False), (15, True), (18, True)]


@pytest.mark.parametrize("family", ["ctc", "gram"])
def test_the_long_runs_of_the_gpu_tests(family):
    """what tests/test_beam_stream_commit_gpu.py takes from here: the longest tails, which size its streams, no refusal, and no
    near-tie at a commit: the best hypothesis leads by more than 10 tolerances wherever a prefix is taken from it"""
    runs = cr.long_runs(family)
    longest = [run["longest"] for run in runs]
    print(longest)
    assert longest == ([18, 16, 16, 15] if family == "ctc" else [26, 22])
    for run in runs:
        assert len(run["log"]) == 30 and all(status == 1 for _, _, status, _, _ in run["log"])
        assert min(margin / tol(best) for _, _, _, margin, best in run["log"]) > 10.0
        assert len(run["done"]) > 50


def test_auto_commits_reach_tens_of_tokens_at_beam_16():
    """randn * 4 with V = 6: the minimum the GPU test asserts for its auto commits"""
    x = (np.random.RandomState(5).randn(120, 6) * 4).astype(np.float32)
    run = cr.search(x, 16, 5, cr.every(120, 20, "auto"))
    assert len(run["done"]) == 26


# ---------------------------------------------------------------------------------------------- the size queries (host only)
def align256(n):
    return (n + 255) // 256 * 256


def state_bytes(B, W, F, gram, with_lm, with_bias):
    """the state layout as it was before there was a commit: the header, the per-slot arrays, the table"""
    if gram:
        n4, n8, node = 10 + (1 if with_lm else 0) + (2 if with_bias else 0), 3, 16
    else:
        n4, n8, node = 6 + (4 if with_lm else 0) + (2 if with_bias else 0), 2, 8
    return align256(B * 32) + n4 * align256(B * W * 4) + n8 * align256(B * W * 8) + align256(B * W * F * node)


def test_the_state_keeps_its_size_and_the_workspace_grows_with_every_dimension():
    from asr import _ops
    for B, W, F in ((1, 1, 1), (3, 8, 20), (4, 128, 76), (32, 16, 1000), (2, 7, 33)):
        for with_lm in (False, True):
            for with_bias in (False, True):
                assert _ops.ctc_beam_stream_state_bytes(B, W, F, with_lm, with_bias) == state_bytes(B, W, F, False, with_lm, with_bias)
                assert (_ops.gram_ctc_beam_bias_stream_state_bytes(B, W, F, with_lm, with_bias)
                        == state_bytes(B, W, F, True, with_lm, with_bias))
            assert _ops.gram_ctc_beam_stream_state_bytes(B, W, F, with_lm) == state_bytes(B, W, F, True, with_lm, False)
        for per_frame in (1, 2):
            assert _ops.beam_stream_commit_workspace_bytes(B, W, F, per_frame) == align256(B * W * F * per_frame * 4)
    q = _ops.beam_stream_commit_workspace_bytes
    assert q(4, 16, 100, 1) < q(8, 16, 100, 1) and q(4, 16, 100, 1) < q(4, 32, 100, 1) and q(4, 16, 100, 1) < q(4, 16, 200, 1)
    assert q(4, 16, 100, 1) < q(4, 16, 100, 2)
    assert q(0, 16, 100, 1) == 0 and q(4, 129, 100, 1) == 0 and q(4, 16, 100, 3) == 0 and q(4, 16, 0, 2) == 0
