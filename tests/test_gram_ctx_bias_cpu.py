"""Gram-CTC beam search with contextual phrase biasing, host side (no GPU): the float64 restatement
(tests/gram_ctx_bias_reference.py) against the restatements it joins (gram_beam_reference.beam_search,
gram_beam_lm_reference.beam_search_lm, ctx_bias_reference.beam_search_bias), against brute-force occurrence counting on the
exhaustive cases and against its float32 twin on the pruned inputs of tests/test_gram_ctx_bias_gpu.py, and the C entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref
import ctx_bias_reference as cref
import gram_beam_lm_reference as glm
import gram_beam_reference as gref
import gram_ctx_bias_reference as gcb
from conftest import PKG, ROOT

ALPHA, BETA = 0.5, 1.0
SEED_P = 20261101                      # tests/test_gram_ctx_bias_gpu.py uses the same inputs
NEW = ("asr_gram_ctc_beam_bias_workspace_bytes", "asr_gram_ctc_beam_search_bias", "asr_gram_ctc_beam_bias_stream_state_bytes",
       "asr_gram_ctc_beam_bias_stream_reset", "asr_gram_ctc_beam_bias_stream_advance", "asr_gram_ctc_beam_bias_stream_result")


def make_lm(ng, V):
    from asr import lm
    return lm.NGramLM.from_ngrams(ng, V, V, V + 1)


def small_gram_case(seed, T=24, V=12, U=4):
    gram = gref.random_table(V, U, seed)
    x = (np.random.RandomState(seed).randn(T, V) * 2).astype(np.float32)
    rs = np.random.RandomState(1000 + seed)
    ng = lmref.random_model(rs, V, 3, [rs.randint(1, V, size=6).tolist() for _ in range(8)], n_random=300)
    return gram, x, lmref.DictLM.of(make_lm(ng, V))


# ------------------------------------------------------------------------------------------------ 1. empty graph
@pytest.mark.parametrize("seed", [31, 32, 33])
def test_an_empty_graph_gives_the_two_parents_exactly(seed):
    gram, x, d = small_gram_case(seed)
    empty = cref.DictGraph([], [])
    for W, K in ((8, 5), (3, 11)):
        plain = gref.beam_search(x, gram, W, K)
        got = gcb.beam_search_bias(x, gram, empty, None, 0.0, 0.0, W, K)
        assert [(s, sc) for s, sc, _, _, _ in got] == plain
        assert all(c == sc and l == 0.0 and bv == 0.0 for _, sc, c, l, bv in got)
        for use_eos in (True, False):
            fused = glm.beam_search_lm(x, gram, d, ALPHA, BETA, W, K, use_eos=use_eos)
            got = gcb.beam_search_bias(x, gram, empty, d, ALPHA, BETA, W, K, use_eos=use_eos)
            assert [e[:4] for e in got] == fused and all(e[4] == 0.0 for e in got)


def test_an_empty_graph_gives_the_parents_on_the_exhaustive_cases():
    empty = cref.DictGraph([], [])
    for (T, rows, seed), _ in gref.EXHAUSTIVE:
        gram = gref.table(rows)
        x = gref.exhaustive_logits(T, len(gram), seed)
        d = lmref.DictLM(lmref.exhaustive_model(3, seed), 3, 3, 4)
        assert [e[:2] for e in gcb.beam_search_bias(x, gram, empty, None, 0.0, 0.0, 128, len(gram) - 1)] \
            == gref.beam_search(x, gram, 128, len(gram) - 1)
        assert [e[:4] for e in gcb.beam_search_bias(x, gram, empty, d, 0.7, 0.4, 128, len(gram) - 1)] \
            == glm.beam_search_lm(x, gram, d, 0.7, 0.4, 128, len(gram) - 1)


# ------------------------------------------------------------------------------------------------ 2. bigram-free table
@pytest.mark.parametrize("seed", [41, 42])
def test_a_bigram_free_table_gives_the_token_level_biased_restatement_exactly(seed):
    T, V, W, K = 40, 14, 8, 6
    rs = np.random.RandomState(seed)
    x = ref.peaky(rs, T, V)
    gram = np.full((V, 2), -1, np.int32)
    gram[1:, 0] = np.arange(1, V)
    phrases, weights = cref.tricky_phrases(rs, range(1, V), 20, 4)
    for w in gcb.windows(lmref.greedy(x), 3)[::4]:           # and some that the decoded strings contain
        if w not in phrases:
            phrases.append(w)
            weights.append(1.5)
    d = cref.DictGraph(phrases, weights)
    ng = lmref.random_model(rs, V, 3, [lmref.greedy(x)], n_random=300)
    dl = lmref.DictLM.of(make_lm(ng, V))
    for lm, a, bt in ((None, 0.0, 0.0), (dl, ALPHA, BETA)):
        for length in (None, 17):
            want = cref.beam_search_bias(x, d, lm, a, bt, W, K, 0, length)
            got = gcb.beam_search_bias(x, gram, d, lm, a, bt, W, K, 0, length)
            assert got == want
            assert any(e[4] > 0 for e in got)


# ------------------------------------------------------------------------------------------------ 3. exhaustive
def test_the_exhaustive_phrase_sets_hold_the_cases_where_the_bigram_step_can_go_wrong():
    for (T, rows, seed), _ in gref.EXHAUSTIVE:
        phrases, weights = gcb.exhaustive_phrases(rows, seed)
        a, b = [r for r in rows if len(r) == 2][0]
        assert any(len(p) > 1 and p[-1] == a for p in phrases)           # ends on the bigram token's first character
        assert any(len(p) > 1 and p[0] == b for p in phrases)            # starts on its second
        assert any(p in ((a,), (b,)) for p in phrases)                   # one character inside it
        assert any(p != q and q[-len(p):] == p for p in phrases for q in phrases)      # a suffix of another phrase
        assert any(p != q and q[:len(p)] == p for p in phrases for q in phrases)       # nested: a prefix of another
        assert all(w * 2 == int(w * 2) for w in weights) and len(set(phrases)) == len(phrases)
    # the C1 merge: with the unigram tokens (a), (b) and the bigram token (a, b) among the candidates of a frame after the first,
    # the beam holds S and S + a, and S + a + b is reached both as (S + a) + b and as S + (a, b)
    merges = [(T, rows) for (T, rows, _), _ in gref.EXHAUSTIVE if T >= 2
              and any(len(r) == 2 and (r[0],) in rows and (r[1],) in rows for r in rows)]
    assert len(merges) >= 3


@pytest.mark.parametrize("case", gref.EXHAUSTIVE, ids=lambda c: "T%d_rows%d_s%d" % (c[0][0], len(c[0][1]), c[0][2]))
def test_memoised_bias_is_the_brute_force_count_for_every_string(case):
    """the beam holds every string: each appears once with the enumeration's probability, and bias_open + ret(state), however
    the string was cut, merged or re-created, is the sum of weight * length over the occurrences -- exactly, in float64 and in
    the float32 twin over the host image (the weights are multiples of 0.5).  Some string is reached in one frame both as
    (S + a) + b and as S + (a, b): the C1 merge."""
    from asr import bias
    (T, rows, seed), count = case
    gram = gref.table(rows)
    V = len(gram)
    x = gref.exhaustive_logits(T, V, seed)
    phrases, weights = gcb.exhaustive_phrases(rows, seed)
    d = cref.DictGraph(phrases, weights)
    tw = cref.Image32(bias.ContextGraph(phrases, V, weights).host_image())
    exact = gref.enumerate_strings(x, gram)
    assert len(exact) == count
    for graph, f32 in ((d, False), (tw, True)):
        memo = {}
        got = gcb.beam_search_bias(x, gram, graph, None, 0.0, 0.0, 128, V - 1, f32=f32, memo=memo)
        strings = [e[0] for e in got]
        assert len(got) == count and len(set(strings)) == count and set(strings) == set(exact)
        assert set(exact) <= set(memo)
        for s, sc, ctc, l, bv in got:
            want = cref.occurrences(s, phrases, weights)
            bo, st = memo[s]
            assert bv == want and bo + float(graph.ret(st)) == want, (s, bv, bo, want)
            assert abs(ctc - exact[s]) <= (1e-4 * max(1.0, abs(exact[s])) if f32 else 1e-9), (s, ctc, exact[s])
            assert abs(sc - (ctc + bv)) <= 1e-4 * max(1.0, abs(sc)) if f32 else sc == ctc + bv
        assert any(e[4] > 0 for e in got)


# ------------------------------------------------------------------------------------------------ 4. the pruned inputs' condition
def test_the_pruned_inputs_do_not_separate_the_two_precisions():
    """what tests/test_gram_ctx_bias_gpu.py's cap of 0 rests on: on pruned_inputs(SEED_P) the float32 twin (the device's bits per
    look-up, every addition rounded) and the float64 restatement return the same strings in the same order in 8 of 8 utterances,
    with and without the model, and the bias changes the top-1 of every utterance"""
    from asr import bias
    gram, x, lengths, phrases, weights, plain = gcb.pruned_inputs(SEED_P)
    assert len(phrases) >= 400
    g = bias.ContextGraph(phrases, gcb.V_P, weights)
    d, tw = cref.DictGraph(phrases, weights), cref.Image32(g.host_image())
    model = make_lm(gcb.pruned_ngrams(plain, SEED_P + 1), gcb.V_P)
    dl, img = lmref.DictLM.of(model), model.host_image()
    for lm, a, bt in ((None, 0.0, 0.0), (dl, ALPHA, BETA)):
        differ = changed = 0
        worst = 0.0
        for b in range(gcb.B_P):
            w64 = gcb.beam_search_bias(x[:, b], gram, d, lm, a, bt, gcb.W_P, gcb.K_P, 0, int(lengths[b]))
            w32 = gcb.beam_search_bias(x[:, b], gram, tw, lm, a, bt, gcb.W_P, gcb.K_P, 0, int(lengths[b]), f32=True, img=img)
            differ += [e[0] for e in w64] != [e[0] for e in w32]
            changed += w64[0][0] != plain[b][0][0]
            worst = max(worst, max(abs(p[1] - q[1]) / (1e-4 * max(1.0, abs(p[1]))) for p, q in zip(w64, w32)))
        print("model" if lm else "plain", "lists that differ:", differ, "top-1 changed:", changed, "worst score gap / tol", worst)
        assert differ == 0 and changed >= 1 and worst <= 0.5


# ------------------------------------------------------------------------------------------------ 5. the C entries
def test_entries_in_the_header_the_binding_and_both_libraries():
    from asr import _lib
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["asr_gram_ctc_beam_search_bias"][1]) == len(_lib.SIGNATURES["asr_gram_ctc_beam_search_lm"][1]) + 7
    assert len(_lib.SIGNATURES["asr_gram_ctc_beam_bias_stream_advance"][1]) \
        == len(_lib.SIGNATURES["asr_gram_ctc_beam_stream_advance"][1]) + 6
    assert len(_lib.SIGNATURES["asr_gram_ctc_beam_bias_stream_result"][1]) \
        == len(_lib.SIGNATURES["asr_gram_ctc_beam_stream_result"][1]) + 7
    for so in ("libasr_hip.so", "libasr_hip_f16.so"):
        path = os.path.join(PKG, so)
        assert os.path.isfile(path), "run `make -C chainer-speech-recognition_amd`"
        lib = ctypes.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (so, name)


def test_size_queries_run_on_the_host():
    from asr import _lib
    lib = _lib.lib()
    T, B, V, W, K = 1000, 16, 3000, 16, 16
    assert lib.asr_gram_ctc_beam_bias_workspace_bytes(T, B, V, W, K) == lib.asr_gram_ctc_beam_workspace_bytes(T, B, V, W, K) > 0
    assert lib.asr_gram_ctc_beam_bias_workspace_bytes(0, B, V, W, K) == 0
    for with_lm in (0, 1):
        old = lib.asr_gram_ctc_beam_stream_state_bytes(B, W, T, with_lm)
        none = lib.asr_gram_ctc_beam_bias_stream_state_bytes(B, W, T, with_lm, 0)
        with_bias = lib.asr_gram_ctc_beam_bias_stream_state_bytes(B, W, T, with_lm, 1)
        assert none == old > 0
        assert with_bias >= old + B * W * 8 and with_bias - old <= B * W * 8 + 2 * 256     # bias_open and the state per string
    assert lib.asr_gram_ctc_beam_bias_stream_state_bytes(0, W, T, 1, 1) == 0
    assert lib.asr_gram_ctc_beam_bias_stream_state_bytes(B, W, 0, 1, 1) == 0


def test_no_cpu_fallback_and_the_graph_must_fit_the_logits():
    import torch
    from asr import _lib, bias, error
    gram = gref.table([(1,), (2,), (1, 2)])
    g = bias.ContextGraph([(1, 2)], 4)
    with pytest.raises(_lib.AsrHipError):
        error.gram_beam_decode_biased(torch.zeros(5, 2, 4), gram, g)
    with pytest.raises(ValueError):
        error.gram_beam_decode_biased(torch.zeros(5, 2, 4), gram, bias.ContextGraph([(1, 2)], 5))
    with pytest.raises(ValueError):
        error.gram_beam_decode_biased(torch.zeros(5, 2, 4), gram, bias.ContextGraph([(1, 2)], 4, blank=3))
    with pytest.raises(ValueError):
        error.GramBeamStream(2, 4, 10, gram, graph=bias.ContextGraph([(1, 2)], 5), device="cpu")
