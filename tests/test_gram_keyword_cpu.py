"""CPU: the restatement of the Gram-CTC keyword search (tests/gram_keyword_reference.py) against a brute force over every span and
every label sequence, against the CTC restatement (tests/keyword_reference.py) on a bigram-free inventory and as the maximum over
all tokenisations, the image builder of asr.spot.GramKeywordSet, the ABI of the three new entries and their checks on the host.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import gram_keyword_reference as gref
import keyword_reference as ref
from conftest import PKG, ROOT

from asr import spot

ENTRIES = ["asr_gram_kws_state_bytes", "asr_gram_kws_state_reset", "asr_gram_kws_detect"]
ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -1, -2, -3
A, B = gref.A, gref.Bc


def test_restatement_equals_brute_force():
    """T <= 5, V = 6 (a, b, ab, aa, ba; every fifth case without the unigram b), L <= 4, 40 cases, every third with logits rounded
    to halves so that candidates tie: det[e] is the maximum over every start, every decomposition and every path, bit for bit
    (both sides add the same float64 costs left to right), and the reported start is a start that attains it"""
    seen = set()
    n_finite = 0
    for i, (x, p, g) in enumerate(gref.tiny_cases(40)):
        T = x.shape[0]
        det, start, _, _ = gref.detect(x, T, [p], g)
        best = gref.brute_force(x, p, g)
        seen.add(tuple(p))
        for e in range(T):
            want = best[:e + 1, e].max()
            assert np.float32(want) == det[0, e], (i, p, e, want, det[0, e])
            if np.isfinite(want):
                n_finite += 1
                assert 0 <= start[0, e] <= e and best[start[0, e], e] == want, (i, p, e)
                assert want <= 0.0
            else:
                assert start[0, e] == -1
    assert {(A, A, A, A), (A, B, A, B), (B, A, A, B)} <= seen and n_finite >= 40


def test_bigram_free_restatement_equals_the_ctc_restatement():
    """without bigrams every G node is absent and a -inf candidate never wins strictly: det and starts are those of
    keyword_reference.detect bit for bit, one shot and in the stream form"""
    V = 7
    x = ref.random_logits(23, 1, V, 5)[:, 0]
    x[::3] = np.round(x[::3])                                         # ties
    phrases = [(1,), (2, 2), (1, 2, 1), (3, 3, 3, 4), (), (5, 0), (6, 5, 4, 3, 2, 1), (9,)]
    want = ref.detect(x, 20, phrases)
    got = gref.detect(x, 20, phrases, gref.plain(V))
    for w, g in zip(want[:3], got[:3]):
        assert w.dtype == g.dtype and np.array_equal(w, g)
    state, parts = None, []
    for a, b in ((0, 1), (1, 8), (8, 8), (8, 23)):
        d, s, f, state = gref.detect(x[a:b], min(b, 20) - a, phrases, gref.plain(V), state=state)
        parts.append((d, s, f))
    for i in range(3):
        assert np.array_equal(np.concatenate([p[i] for p in parts], -1), want[i])


def test_det_is_the_maximum_over_all_tokenisations():
    """every path accumulates the same additions in the same order in either lattice, so det equals exactly the element-wise
    maximum of the CTC restatement over every way of cutting the phrase into tokens"""
    cases = [(gref.SMALL, [(A, B, A, B), (A, A, A, A, A), (B, A, A, B, A), (A,), (B, A)]),
             (gref.NO_B, [(A, B, A, B), (A, B, A, A), (A, A), (A, B)]),
             (gref.NINE, [(1, 2, 1, 2, 1), (3, 3, 3, 4), (4, 3, 3), (2, 1, 2)])]
    for n, (g, phrases) in enumerate(cases):
        V = g.shape[0]
        x = ref.random_logits(17, 1, V, 30 + n)[:, 0]
        x[::2] = np.round(x[::2] * 2) / 2
        det, start, _, _ = gref.detect(x, 17, phrases, g)
        for k, p in enumerate(phrases):
            toks = gref.tokenisations(p, g)
            assert len(toks) >= (2 if len(p) > 2 and g is not gref.NO_B else 1), (p, toks)
            each = ref.detect(x, 17, toks)[0]
            assert np.array_equal(det[k], each.max(axis=0)), (n, p)
            assert np.array_equal(start[k] < 0, np.isneginf(det[k]))
    assert sorted(gref.tokenisations((A, B, A), gref.SMALL)) == [(1, 2, 1), (1, 5), (3, 1)]
    assert gref.tokenisations((B, B), gref.NO_B) == [] and gref.tokenisations((A, B), gref.NO_B) == [(3,)]


def test_phrases_without_a_spelling_and_with_only_a_bigram_spelling():
    x = ref.peaked([0, 3, 3, 0, 1, 5, 0], 6)                          # ab, then a ba
    det, start, _, _ = gref.detect(x, 7, [(A, B), (B, B), (A, B, A), (B,)], gref.NO_B)
    assert list(det[0, 1:3]) == [0.0, 0.0] and list(start[0, 1:3]) == [1, 1]              # only spelling: the bigram ab
    assert np.all(np.isneginf(det[1])) and np.all(start[1] == -1)                          # b b: no token ends or starts it
    assert det[2, 5] == 0.0 and start[2, 5] == 4                                           # a + ba
    assert np.all(np.isneginf(det[3])) and np.all(start[3] == -1)                          # b alone has no token


def test_stream_form_of_the_restatement():
    x = ref.random_logits(11, 1, 6, 4)[:, 0]
    phrases = [(A, B, B, A), (A, A, A), (B,)]
    det, start, _, _ = gref.detect(x, 11, phrases, gref.SMALL)
    state, parts = None, []
    for a, b in ((0, 3), (3, 4), (4, 11)):
        d, s, _, state = gref.detect(x[a:b], b - a, phrases, gref.SMALL, state=state)
        parts.append((d, s))
    assert np.array_equal(np.concatenate([p[0] for p in parts], 1), det)
    assert np.array_equal(np.concatenate([p[1] for p in parts], 1), start)
    assert state["base"] == 11


def test_planted_generator_and_exact_zero():
    """whichever mix of tokens the planted path uses, the restatement scores the occurrence exactly 0.0 on its span"""
    phrases = [(1, 2, 1, 2), (3, 3, 4), (2, 1, 1)]
    mixes = set()
    for seed in range(6):
        path, spans, used = gref.planted(60, phrases, gref.NINE, seed)
        mixes |= {tuple(u) for u in used}
        det, start, _, _ = gref.detect(ref.peaked(path, 9, seed), 60, phrases, gref.NINE)
        for k, s, e in spans:
            assert det[k, e - 1] == 0.0 and start[k, e - 1] == s, (seed, k)
    assert len(mixes) >= 6                                            # unigram-only, bigram-only and mixed spellings all occurred


def test_image_builder():
    g = gref.NINE                                                     # a b c d = 1 2 3 4; ab 5, ba 6, cc 7, cd 8
    phrases = [(1, 2, 1), (3, 3, 4), (2, 2), (4,), (), (1, 0, 1), (1, 9), (1, 2, 1), (-1,)]
    kws = spot.GramKeywordSet(phrases, g)
    h = kws.host_image()
    assert kws.K == 9 and kws.Lmax == 3 and kws.V == 9 and kws.dead == [False] * 4 + [True] * 3 + [False, True]
    assert all(h[n].dtype == np.int32 for n in ("uniq", "node_uni", "node_big", "kw_len"))
    assert list(h["uniq"]) == [1, 2, 3, 4, 5, 6, 7, 8] and kws.U == 8                   # shared tokens once, dead phrases add none
    assert h["node_uni"].tolist() == [[0, 1, 0], [2, 2, 3], [1, 1, -1], [3, -1, -1]] + [[-1] * 3] * 3 + [[0, 1, 0], [-1] * 3]
    assert h["node_big"].tolist() == [[-1, 4, 5], [-1, 6, 7], [-1, -1, -1], [-1] * 3] + [[-1] * 3] * 3 + [[-1, 4, 5], [-1] * 3]
    assert list(h["kw_len"]) == [3, 3, 2, 1, 0, 3, 2, 3, 1]
    assert np.all(h["node_big"][:, 0] == -1)
    # a character without a unigram token is not dead: its U node is absent, the bigrams still cover it
    nob = spot.GramKeywordSet([(1, 2, 1), (2, 2)], gref.NO_B)
    h = nob.host_image()
    assert nob.dead == [False, False] and list(h["uniq"]) == [1, 3, 5]
    assert h["node_uni"].tolist() == [[0, -1, 0], [-1, -1, -1]] and h["node_big"].tolist() == [[-1, 1, 2], [-1, -1, -1]]
    # only tokens that a live phrase can use are gathered
    assert list(spot.GramKeywordSet([(4, 4)], g).host_image()["uniq"]) == [4]
    only_dead = spot.GramKeywordSet([(), (99,)], g).host_image()
    assert only_dead["uniq"].shape == (1,) and np.all(only_dead["node_uni"] == -1) and np.all(only_dead["node_big"] == -1)
    assert spot.GramKeywordSet([[1] * 64], g).Lmax == 64
    with pytest.raises(ValueError):
        spot.GramKeywordSet([[1] * 65], g)
    with pytest.raises(ValueError):
        spot.GramKeywordSet([], g)
    bad = g.copy()
    bad[0] = (1, -1)
    with pytest.raises(ValueError):
        spot.GramKeywordSet([(1,)], bad)                              # asr.error.check_gram_table: the blank row
    assert spot.GRAM_SWEEP_TILE >= 1 and spot.MAX_LEN == 64


def test_from_text():
    from asr import vocab
    ids, _ = vocab.get_unigram_ids()
    ids = dict(ids)
    a, b = vocab.UNIGRAM_TOKENS[0], vocab.UNIGRAM_TOKENS[1]
    ids[a + b] = len(ids)
    kws = spot.GramKeywordSet.from_text([a + b + a, "", "  ", b, "\x00" + a], ids)
    assert kws.K == 2 and kws.dropped == 1 and kws.V == len(ids)
    assert kws.phrases == [(ids[a], ids[b], ids[a]), (ids[b],)]
    h = kws.host_image()
    assert list(h["uniq"]) == [ids[a], ids[b], ids[a + b]]
    assert h["node_uni"].tolist() == [[0, 1, 0], [1, -1, -1]] and h["node_big"].tolist() == [[-1, 2, -1], [-1, -1, -1]]


def test_the_three_entries_are_declared_bound_and_exported():
    from asr import _lib, _ops
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        for so in ("libasr_hip.so", "libasr_hip_f16.so"):
            assert hasattr(ctypes.CDLL(os.path.join(PKG, so)), name), (so, name)
    for fn in ("gram_kws_state", "gram_kws_state_reset", "gram_kws_detect"):
        assert callable(getattr(_ops, fn))
    assert hasattr(spot, "GramKeywordSet") and callable(spot.GramKeywordSet.from_text)


def test_state_query_runs_on_the_host():
    from asr import _lib
    lib = _lib.lib()
    query = lib.asr_gram_kws_state_bytes
    base = query(7, 3, 5)
    assert base == 36 * 7 * 3 * 5 + 4 * 7                             # three nodes per position, 12 bytes each; a counter per b
    assert query(8, 3, 5) > base and query(7, 4, 5) > base and query(7, 3, 6) > base                  # grows with each argument
    for empty in ((0, 3, 5), (7, 0, 5), (7, 3, 0), (-1, 3, 5)):
        assert query(*empty) == 0
    assert query(32, 64, 64) == 36 * 32 * 64 * 64 + 128 and query(4096, 4096, 64) > 2 ** 32           # size_t, not int
    assert query(7, 3, 5) > lib.asr_kws_state_bytes(7, 3, 5)


def test_bad_arguments_are_refused_before_any_launch():
    """the entry checks need no GPU: the pointers below are never followed"""
    from asr import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    good = dict(stream=None, logits=p, lengths=None, T=4, B=1, V=5, blank=0, uniq=p, U=2, node_uni=p, node_big=p, kw_len=p, K=1,
                Lmax=2, state=None, det=p, det_start=p, fill=p, ws=p, ws_bytes=1 << 20)

    def detect(**over):
        return lib.asr_gram_kws_detect(*dict(good, **over).values())

    for name in ("logits", "uniq", "node_uni", "node_big", "kw_len", "det", "det_start", "fill", "ws"):
        assert detect(**{name: None}) == ASR_ERR_BAD_ARG, name
    for name in ("T", "B", "V", "U", "K", "Lmax"):
        for bad in (0, -1):
            assert detect(**{name: bad}) == ASR_ERR_BAD_ARG, name
    assert detect(blank=-1) == ASR_ERR_BAD_ARG and detect(blank=5) == ASR_ERR_BAD_ARG
    assert detect(Lmax=65) == ASR_ERR_UNSUPPORTED
    assert detect(ws_bytes=8) == ASR_ERR_WORKSPACE
    assert detect(ws_bytes=lib.asr_kws_workspace_bytes(4, 1, 2) - 1) == ASR_ERR_WORKSPACE

    assert lib.asr_gram_kws_state_reset(None, None, 1, 1, 2, None) == ASR_ERR_BAD_ARG
    for bad in ((0, 1, 2), (1, 0, 2), (1, 1, 0)):
        assert lib.asr_gram_kws_state_reset(None, p, *bad, None) == ASR_ERR_BAD_ARG
    assert lib.asr_gram_kws_state_reset(None, p, 1, 1, 65, None) == ASR_ERR_UNSUPPORTED
