"""Gram-CTC beam search fused with a character n-gram language model, host side (no GPU): the float64 restatement
(tests/gram_beam_lm_reference.py) against an exhaustive enumeration of every path, against the two restatements it joins
(gram_beam_reference.beam_search, ctc_beam_lm_reference.beam_search_lm) and against its float32 twin, and the C entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import ctc_beam_lm_reference as lmref
import gram_beam_lm_reference as glm
import gram_beam_reference as gref
from conftest import PKG, ROOT

ALPHA, BETA = 0.5, 1.0
SEED_P = 20261019


def tol(s):
    return 1e-4 * max(1.0, abs(s))


# ------------------------------------------------------------------------------------------------ 1. exhaustive
def test_restatement_is_exact_when_the_beam_holds_everything():
    alpha, beta = 0.7, 0.4
    worst = 0.0
    for (T, rows, seed), count in gref.EXHAUSTIVE:
        gram = gref.table(rows)
        V = len(gram)
        x = gref.exhaustive_logits(T, V, seed)
        d = lmref.DictLM(lmref.exhaustive_model(3, seed), 3, 3, 4)
        exact = gref.enumerate_strings(x, gram)
        got = glm.beam_search_lm(x, gram, d, alpha, beta, 128, V - 1)
        strings = [e[0] for e in got]
        assert len(got) == count and len(set(strings)) == count and set(strings) == set(exact)
        for s, score, ctc, l in got:
            dev = max(abs(ctc - exact[s]), abs(l - d.score(s)), abs(score - (exact[s] + alpha * d.score(s) + beta * len(s))))
            worst = max(worst, dev)
            assert dev <= 1e-9, (T, rows, seed, s, dev)
        sc = [e[1] for e in got]
        assert all(a >= b for a, b in zip(sc, sc[1:]))
    print("worst deviation from the enumeration:", worst)


# ------------------------------------------------------------------------------------------------ 2. neutral weights
@pytest.fixture(scope="module")
def pruned():
    """the pruned inputs, the unfused restatement's N-best (full and ragged) and the model of test 4 with <s> / </s> as the ids
    V and V + 1 (the values are those of the ids U_P + 1 / U_P + 2 it is made with)"""
    gram, x, lengths = gref.pruned_inputs()
    out = {"gram": gram, "x": x, "lengths": lengths}
    for name, ln in (("full", None), ("ragged", lengths)):
        out[name] = [gref.beam_search(x[:, b], gram, gref.W_P, gref.K_P, 0, None if ln is None else ln[b])
                     for b in range(gref.B_P)]
    out["model"] = pruned_model(out["full"], len(gram))
    out["d"] = lmref.DictLM.of(out["model"])
    return out


def pruned_model(unfused_full, V, seed=SEED_P):
    from asr import lm
    ng = lmref.random_model(np.random.RandomState(seed), gref.U_P + 1, 3, [w[0][0] for w in unfused_full], n_random=300)
    return lm.NGramLM.from_ngrams(glm.relabel_marks(ng, gref.U_P + 1, V), V, V, V + 1)


def test_neutral_weights_and_no_eos_give_the_unfused_restatement(pruned):
    gram = pruned["gram"]
    for name, ln in (("full", None), ("ragged", pruned["lengths"])):
        for b in range(gref.B_P):
            got = glm.beam_search_lm(pruned["x"][:, b], gram, pruned["d"], 0.0, 0.0, gref.W_P, gref.K_P, 0,
                                     None if ln is None else ln[b], use_eos=False)
            assert [(e[0], e[1]) for e in got] == pruned[name][b]           # == on float64
            assert [e[2] for e in got] == [w[1] for w in pruned[name][b]]


# ------------------------------------------------------------------------------------------------ 3. bigram-free table
def test_a_bigram_free_table_gives_the_token_level_fused_search():
    for T, V, W, K, blank, seed in ((12, 6, 8, 5, 0, 1), (20, 9, 4, 3, 2, 2), (30, 40, 16, 16, 0, 4)):
        rs = np.random.RandomState(seed)
        x = (rs.randn(T, V) * 2).astype(np.float32)
        gram = np.full((V, 2), -1, np.int32)
        gram[:, 0] = np.arange(V)
        gram[blank] = -1
        ng = lmref.random_model(rs, V, 4, [rs.randint(0, V, size=6).tolist() for _ in range(8)], n_random=300)
        d = lmref.DictLM(ng, 4, V, V + 1)
        want = lmref.beam_search_lm(x, d, ALPHA, BETA, W, K, blank)
        got = glm.beam_search_lm(x, gram, d, ALPHA, BETA, W, K, blank)
        assert [e[0] for e in got] == [e[0] for e in want]
        diff = max(abs(a - b) for g, w in zip(got, want) for a, b in zip(g[1:], w[1:]))
        assert diff == 0.0, (T, V, W, K, blank, diff)


# ------------------------------------------------------------------------------------------------ 4. behind the GPU cap
def test_pruned_inputs_do_not_separate_float32_from_float64(pruned):
    """the condition behind the cap of tests/test_gram_beam_lm_gpu.py::test_pruned_search_against_restatement: on these inputs
    the float32 twin returns the float64 run's strings in the same order in 8 of 8 utterances, full and ragged, and the model
    changes every top-1 string"""
    gram, x, d = pruned["gram"], pruned["x"], pruned["d"]
    img = pruned["model"].host_image()
    for name, ln in (("full", None), ("ragged", pruned["lengths"])):
        worst, changed = 0.0, 0
        for b in range(gref.B_P):
            length = None if ln is None else ln[b]
            w64 = glm.beam_search_lm(x[:, b], gram, d, ALPHA, BETA, gref.W_P, gref.K_P, 0, length)
            w32 = glm.beam_search_lm(x[:, b], gram, d, ALPHA, BETA, gref.W_P, gref.K_P, 0, length, f32=True, img=img)
            assert [e[0] for e in w32] == [e[0] for e in w64], (name, b)
            worst = max([worst] + [abs(a[1] - c[1]) / tol(c[1]) for a, c in zip(w32, w64)])
            changed += w64[0][0] != pruned[name][b][0][0]
        print("%s: worst float32 / float64 score gap %.4f tol, top-1 differs from the unfused search's in %d of %d"
              % (name, worst, changed, gref.B_P))
        # a float32 sum of T = 160 frames of O(10) terms: well inside a tenth of the tolerance
        assert worst <= 0.1
        assert changed == gref.B_P


# ------------------------------------------------------------------------------------------------ 5. plumbing
def test_entries_in_the_header_the_binding_and_both_libraries():
    from asr import _lib
    header = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in ("asr_gram_ctc_beam_lm_workspace_bytes", "asr_gram_ctc_beam_search_lm"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["asr_gram_ctc_beam_search_lm"][1]) == 29
    for so in ("libasr_hip.so", "libasr_hip_f16.so"):
        path = os.path.join(PKG, so)
        assert os.path.isfile(path), "run `make -C chainer-speech-recognition_amd`"
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "asr_gram_ctc_beam_search_lm")
        q, p = lib.asr_gram_ctc_beam_lm_workspace_bytes, lib.asr_gram_ctc_beam_workspace_bytes
        for f in (q, p):
            f.restype = ctypes.c_size_t
            f.argtypes = [ctypes.c_int] * 5
        T, B, V, W, K = 1000, 16, 3000, 16, 16
        assert q(T, B, V, W, K) >= p(T, B, V, W, K) > 0
        assert q(5, 1, 3, 4, 16) == q(5, 1, 3, 4, 2)       # top_k above V - 1 acts as V - 1
        for dims in ((0, B, V, W, K), (T, 0, V, W, K), (T, B, 0, W, K), (T, B, V, 0, K), (T, B, V, W, 0), (-1, B, V, W, K)):
            assert q(*dims) == 0, dims


def test_gram_beam_decode_lm_value_errors():
    import torch
    from asr import error, lm
    x = torch.zeros((3, 1, 4), dtype=torch.float32)
    good = gref.table(((1,), (2,), (1, 2)))
    model = lm.NGramLM.from_ngrams({(i,): (-1.0, 0.0) for i in range(6)}, 4, 4, 5)
    bad = []
    bad.append(good[:3])                                   # wrong shape
    bad.append(good.astype(np.float32))                    # not integers
    g = good.copy(); g[0] = (1, -1); bad.append(g)         # the blank row spells something
    g = good.copy(); g[3] = (1, 4); bad.append(g)          # id outside [0, V)
    g = good.copy(); g[3] = (-1, 2); bad.append(g)         # a bigram without its first unigram
    g = good.copy(); g[2] = (1, -1); bad.append(g)         # two tokens, one spelling
    g = good.copy(); g[3] = (-2, -1); bad.append(g)
    for g in bad:
        with pytest.raises(ValueError):
            error.gram_beam_decode_lm(x, g, model, 0.5, 1.0, 4, 3)
    with pytest.raises(ValueError):
        error.gram_beam_decode_lm(x, good, model, 0.5, 1.0, 4, 3, 1)       # blank row must be (-1, -1)
    small = lm.NGramLM.from_ngrams({(i,): (-1.0, 0.0) for i in range(3)}, 3)
    assert small.vlm == 3
    with pytest.raises(ValueError):
        error.gram_beam_decode_lm(x, good, small, 0.5, 1.0, 4, 3)          # the model covers fewer ids than the logits
