"""CPU: the restatement of the CTC keyword search (tests/keyword_reference.py) against a brute force over every span and every path,
hand cases of its tie rules, the keyword image builder of asr/spot.py, the ABI of the five new entries and their checks on the host.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import keyword_reference as ref
from conftest import PKG, ROOT

from asr import spot

ENTRIES = ["asr_kws_workspace_bytes", "asr_kws_state_bytes", "asr_kws_state_reset", "asr_kws_detect", "asr_kws_hits"]
ASR_ERR_BAD_ARG, ASR_ERR_UNSUPPORTED = -1, -3


def test_restatement_equals_brute_force():
    """T <= 5, V = 3, L <= 3, 30 random cases: det[e] is the maximum over every start and every path, bit for bit (both sides add
    the same float64 costs left to right), and the reported start is a start that attains it"""
    seen_repeat = False
    for i, (x, p) in enumerate(ref.tiny_cases(30)):
        T = x.shape[0]
        det, start, _, _ = ref.detect(x, T, [p])
        best = ref.brute_force(x, p)
        seen_repeat |= tuple(p) == (1, 1)
        for e in range(T):
            want = best[:e + 1, e].max()
            assert np.float32(want) == det[0, e], (i, p, e, want, det[0, e])
            if np.isfinite(want):
                assert 0 <= start[0, e] <= e and best[start[0, e], e] == want, (i, p, e)
                assert want <= 0.0
            else:
                assert start[0, e] == -1
    assert seen_repeat


def test_restatement_is_vectorised_consistently():
    """K phrases at once equal each phrase on its own; a dead phrase beside live ones is -inf / -1 everywhere; lengths cut"""
    x = ref.random_logits(9, 1, 6, 3)[:, 0]
    phrases = [(1, 2), (7, 1), (3,), (), (2, 2, 4), (1, 0)]
    det, start, fill, _ = ref.detect(x, 7, phrases)
    for k, p in enumerate(phrases):
        d1, s1, f1, _ = ref.detect(x, 7, [p])
        assert np.array_equal(d1[0], det[k]) and np.array_equal(s1[0], start[k]) and np.array_equal(f1, fill)
    for k in (1, 3, 5):
        assert np.all(np.isneginf(det[k])) and np.all(start[k] == -1)
    assert np.all(np.isneginf(det[:, 7:])) and np.all(start[:, 7:] == -1) and np.all(fill[7:] == 0) and np.all(fill[:7] < 0)


def test_stream_form_of_the_restatement():
    x = ref.random_logits(11, 1, 5, 4)[:, 0]
    phrases = [(1, 2, 2), (3,)]
    det, start, _, _ = ref.detect(x, 11, phrases)
    state, parts = None, []
    for a, b in ((0, 3), (3, 4), (4, 11)):
        d, s, _, state = ref.detect(x[a:b], b - a, phrases, state=state)
        parts.append((d, s))
    assert np.array_equal(np.concatenate([p[0] for p in parts], 1), det)
    assert np.array_equal(np.concatenate([p[1] for p in parts], 1), start)


def test_tie_rules_by_hand():
    """peaked path 0 1 1 0 2 2 2 0 0 1 2 0, keyword (1, 2): hits [1, 7) and [9, 11), both exactly 0.0, the earlier one first"""
    path = [0, 1, 1, 0, 2, 2, 2, 0, 0, 1, 2, 0]
    x = ref.peaked(path, 4)
    det, start, fill, _ = ref.detect(x, len(path), [(1, 2)])
    # the run of the first token belongs to the occurrence from its first frame; the run of the last token is covered to its end
    assert list(det[0, 4:7]) == [0.0, 0.0, 0.0] and list(start[0, 4:7]) == [1, 1, 1]
    assert det[0, 10] == 0.0 and start[0, 10] == 9
    # without a threshold every finite score is a candidate: what is left beside the two occurrences scores far below them
    hs, he, sc, lp, n = ref.hits(det[0], start[0], fill, len(path), max_hits=4)
    assert n >= 2 and list(hs[:2]) == [1, 9] and list(he[:2]) == [7, 11] and list(sc[:2]) == [0.0, 0.0] and np.all(sc[2:] < -5.0)
    hs, he, sc, lp, n = ref.hits(det[0], start[0], fill, len(path), max_hits=4, min_score=-1.0)
    assert n == 2 and list(hs) == [1, 9, -1, -1] and list(he) == [7, 11, -1, -1]
    assert list(sc[:2]) == [0.0, 0.0] and np.all(np.isneginf(sc[2:])) and np.all(np.isneginf(lp[2:]))
    assert abs(lp[0] - fill[1:7].astype(np.float64).sum()) < 1e-6
    # max_hits = 1 keeps the earlier of the two equally good occurrences; a threshold above every score keeps nothing
    assert ref.hits(det[0], start[0], fill, len(path), max_hits=1)[0][0] == 1
    assert ref.hits(det[0], start[0], fill, len(path), max_hits=4, min_score=1.0)[4] == 0
    # a repeated token needs its blank: on 1 1 0 1 the keyword (1, 1) ends at frame 3 and starts at frame 0
    det, start, _, _ = ref.detect(ref.peaked([1, 1, 0, 1], 3), 4, [(1, 1)])
    assert det[0, 3] == 0.0 and start[0, 3] == 0 and np.all(det[0, :2] < -5.0)


def test_image_builder():
    kws = spot.KeywordSet([(5, 9, 2), (9, 5), (7, 7), (3, 40), (), (4, 0, 4), (5, 9, 2)], V=40, blank=0)
    h = kws.host_image()
    assert kws.K == 7 and kws.Lmax == 3 and kws.dead == [False, False, False, True, True, True, False]
    assert h["uniq"].dtype == h["node_tok"].dtype == h["kw_len"].dtype == np.int32
    assert list(h["uniq"]) == [2, 5, 7, 9] and kws.U == 4                   # shared tokens: one entry each, dead phrases add none
    assert h["node_tok"].tolist() == [[1, 3, 0], [3, 1, -1], [2, 2, -1], [-1] * 3, [-1] * 3, [-1] * 3, [1, 3, 0]]
    assert list(h["kw_len"]) == [3, 2, 2, 2, 0, 3, 3]
    assert spot.KeywordSet([range(1, 65)], V=100).Lmax == 64
    with pytest.raises(ValueError):
        spot.KeywordSet([range(1, 66)], V=100)
    only_dead = spot.KeywordSet([(), (99,)], V=10).host_image()
    assert only_dead["uniq"].shape == (1,) and np.all(only_dead["node_tok"] == -1)
    assert spot.SWEEP_GROUP >= 1 and spot.SWEEP_TILE >= 1 and spot.MAX_LEN == 64


def test_the_five_entries_are_declared_bound_and_exported():
    from asr import _lib, _ops
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        for so in ("libasr_hip.so", "libasr_hip_f16.so"):
            assert hasattr(ctypes.CDLL(os.path.join(PKG, so)), name), (so, name)
    for fn in ("kws_state", "kws_state_reset", "kws_detect", "kws_hits"):
        assert callable(getattr(_ops, fn))
    for fn in ("KeywordSet", "keyword_detect", "keyword_hits", "keyword_search", "KeywordStream", "Detection", "Hits"):
        assert hasattr(spot, fn)
    assert spot.Detection._fields == ("score", "start", "fill") and spot.Hits._fields == ("start", "end", "score", "logp", "count")


def test_queries_run_on_the_host():
    from asr import _lib
    lib = _lib.lib()
    for query in (lib.asr_kws_workspace_bytes, lib.asr_kws_state_bytes):
        base = query(7, 3, 5)
        assert base > 0
        assert query(8, 3, 5) > base and query(7, 4, 5) > base and query(7, 3, 6) > base              # grows with each argument
        for empty in ((0, 3, 5), (7, 0, 5), (7, 3, 0), (-1, 3, 5)):
            assert query(*empty) == 0
    assert lib.asr_kws_workspace_bytes(1000, 32, 600) >= 1000 * 32 * 601 * 4                          # U + 1 values per frame
    assert lib.asr_kws_workspace_bytes(100000, 64, 4000) > 2 ** 32                                    # size_t, not int
    assert lib.asr_kws_state_bytes(32, 64, 16) >= 32 * 64 * (2 * 16 - 1) * 12 + 32 * 4                # value and start per node


def test_bad_arguments_are_refused_before_any_launch():
    """the entry checks need no GPU: the pointers below are never followed"""
    from asr import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    good = dict(stream=None, logits=p, lengths=None, T=4, B=1, V=5, blank=0, uniq=p, U=2, node_tok=p, kw_len=p, K=1, Lmax=2,
                state=None, det=p, det_start=p, fill=p, ws=p, ws_bytes=1 << 20)

    def detect(**over):
        return lib.asr_kws_detect(*dict(good, **over).values())

    for name in ("logits", "uniq", "node_tok", "kw_len", "det", "det_start", "fill", "ws"):
        assert detect(**{name: None}) == ASR_ERR_BAD_ARG, name
    for name in ("T", "B", "V", "U", "K", "Lmax"):
        for bad in (0, -1):
            assert detect(**{name: bad}) == ASR_ERR_BAD_ARG, name
    assert detect(blank=-1) == ASR_ERR_BAD_ARG and detect(blank=5) == ASR_ERR_BAD_ARG
    assert detect(Lmax=65) == ASR_ERR_UNSUPPORTED
    assert detect(ws_bytes=8) == -2

    hits = dict(stream=None, det=p, det_start=p, fill=p, lengths=None, B=1, K=1, T=4, max_hits=2, min_score=0.0, hs=p, he=p, sc=p,
                lp=p, n=p)
    for name in ("det", "det_start", "fill", "hs", "he", "sc", "lp", "n"):
        assert lib.asr_kws_hits(*dict(hits, **{name: None}).values()) == ASR_ERR_BAD_ARG, name
    for name in ("B", "K", "T", "max_hits"):
        assert lib.asr_kws_hits(*dict(hits, **{name: 0}).values()) == ASR_ERR_BAD_ARG, name
    assert lib.asr_kws_hits(*dict(hits, max_hits=4097).values()) == ASR_ERR_UNSUPPORTED

    assert lib.asr_kws_state_reset(None, None, 1, 1, 2, None) == ASR_ERR_BAD_ARG
    for bad in ((0, 1, 2), (1, 0, 2), (1, 1, 0)):
        assert lib.asr_kws_state_reset(None, p, *bad, None) == ASR_ERR_BAD_ARG
    assert lib.asr_kws_state_reset(None, p, 1, 1, 65, None) == ASR_ERR_UNSUPPORTED
