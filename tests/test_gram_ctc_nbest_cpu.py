"""N-best Gram-CTC scoring and the string-level MWER loss without a GPU: the float64 restatement
(tests/gram_nbest_reference.py) against the enumeration of every path, its explicit decisions, the ABI and the host-side checks
of asr.loss.gram_ctc_nbest_logp / gram_mwer_loss."""
import os
import re

import numpy as np
import pytest
import torch

import gram_beam_reference as gref
import gram_nbest_reference as ref
from conftest import PKG, ROOT

SYMBOLS = ("asr_gram_ctc_nbest_workspace_bytes", "asr_gram_ctc_nbest_forward", "asr_gram_ctc_nbest_backward")


@pytest.mark.parametrize("case", gref.EXHAUSTIVE, ids=lambda c: "T%d_rows%d_s%d" % (c[0][0], len(c[0][1]), c[0][2]))
def test_restatement_equals_the_enumeration_of_every_path(case):
    """every string with p > 0 of the six exhaustive inventories, the empty one included, to 1e-9; and the gradient of the
    restatement sums to zero over every frame's inventory (it is occupancy - softmax)"""
    (T, rows, seed), count = case
    gram = gref.table(rows)
    x = gref.exhaustive_logits(T, len(gram), seed)
    exact = gref.enumerate_strings(x, gram)
    assert len(exact) == count and () in exact
    strings = sorted(exact)
    L = max(len(s) for s in strings)
    hyps = np.zeros((1, count, L), np.int32)
    lens = np.zeros((1, count), np.int32)
    for n, s in enumerate(strings):
        hyps[0, n, :len(s)], lens[0, n] = s, len(s)
    logp, grads = ref.nbest_logp_grad(x[:, None, :], hyps, lens, gram)
    want = np.array([exact[s] for s in strings])
    print("worst |restatement - enumeration| =", np.abs(logp[0] - want).max())
    assert np.abs(logp[0] - want).max() <= 1e-9
    assert abs(np.logaddexp.reduce(logp[0])) <= 1e-9            # the strings with p > 0 are all there is
    for g in grads[0]:
        assert np.abs(g.sum(axis=1)).max() <= 1e-12


def test_a_string_longer_than_two_characters_per_frame_has_no_path():
    gram = gref.table(((1,), (2,), (1, 2), (2, 1)))
    x = gref.exhaustive_logits(3, len(gram), 0)
    six, seven = [1, 2, 2, 1, 1, 2], [1, 2, 2, 1, 1, 2, 1]
    assert np.isfinite(ref.slot_logp_grad(x, six, 6, 3, gram)[0])           # 2 T characters: the bigram tokens (1, 2) (2, 1) (1, 2)
    lp, g = ref.slot_logp_grad(x, seven, 7, 3, gram)
    assert lp == -np.inf and not g.any()
    assert ref.slot_logp_grad(x, six, 6, 2, gram)[0] == -np.inf             # the same string on 2 of the 3 frames
    assert ref.slot_logp_grad(x, six, -1, 3, gram)[0] == -np.inf            # unused
    assert ref.slot_logp_grad(x, six, 6, 0, gram)[0] == -np.inf             # no frames


def test_a_character_without_a_unigram_token_scores_minus_infinity():
    gram = gref.table(((1,), (2,), (1, 2)))
    x = gref.exhaustive_logits(4, len(gram), 1)
    assert np.isfinite(ref.slot_logp_grad(x, [1, 2], 2, 4, gram)[0])
    for s in ([1, 3], [3], [1, -1], [1, 7], [0, 1]):                        # 3 is the bigram TOKEN, not a character; 0 the blank
        lp, g = ref.slot_logp_grad(x, s, len(s), 4, gram)
        assert lp == -np.inf and not g.any(), s
    # a bigram spelled with a character that has no unigram row: strings with that character are refused, whatever the bigram
    only_pair = gref.table(((1,), (1, 2)))
    assert ref.slot_logp_grad(gref.exhaustive_logits(4, 3, 2), [1, 2], 2, 4, only_pair)[0] == -np.inf


def test_random_case_has_every_kind_of_slot():
    """the generator of the GPU cases at its smallest shape: -inf exactly at the slots made for it (and at what else does not fit
    into the last utterance's two frames), finite at the slots with the doubled character, "abab" and the missing pair"""
    T, B, V, N, L = 50, 3, 7, 3, 5
    gram = ref.shuffled_table(3, 3, seed=V)
    xs, hyps, hyp_len, x_len, gy = ref.random_case(T, B, N, L, gram, seed=1)
    logp = ref.nbest_logp_grad(xs, hyps, hyp_len, gram, x_len, want_grad=False)
    assert np.isfinite(logp[0, 0]) and np.isfinite(logp[0, 1]) and np.isfinite(logp[1]).all()
    assert logp[0, 2] == -np.inf and logp[B - 1, 0] == -np.inf and logp[B - 1, N - 1] == -np.inf
    a, b = hyps[0, 0, 0], hyps[0, 0, 1]
    assert (a, b) in ref.table_pairs(gram) and list(hyps[0, 0, :4]) == [a, b, a, b]
    assert tuple(hyps[1, 0, L - 2:L]) not in ref.table_pairs(gram) and hyps[1, 1, 1] == hyps[1, 1, 2]
    assert hyp_len[0, 1] == 0 and hyp_len[B - 1, N - 1] == -1 and 2 * x_len[B - 1] < L


def test_header_binding_and_library_have_the_gram_nbest_symbols():
    import ctypes
    from asr import _lib
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    handle = _lib.lib()
    half = ctypes.CDLL(os.path.join(PKG, "libasr_hip_f16.so"))
    for name in SYMBOLS:
        assert hasattr(handle, name) and hasattr(half, name), name


def test_workspace_query_and_limits_on_the_host():
    from asr import _lib
    lib = _lib.lib()
    q = lib.asr_gram_ctc_nbest_workspace_bytes
    n1, n4 = q(100, 4, 50, 1, 10), q(100, 4, 50, 4, 10)
    assert n1 > 4 * 100 * 64 * (8 + 8 + 4) and 3 * n1 < n4 < 4 * n1        # 3 * 10 + 1 nodes pad to 64
    assert q(100, 4, 50, 4, 40) > 1.9 * n4                                  # 3 * 40 + 1 nodes pad to 128
    assert q(100, 4, 50, 4, 10) > lib.asr_ctc_nbest_workspace_bytes(100, 4, 50, 4, 10)     # label rows and the index on top
    assert q(100, 4, 50000, 4, 10) - n4 == 12 * (131072 - 128)               # the index: 12 bytes per slot, 2^17 / 2^7 >= 2 V slots
    assert q(100, 4, 50, 0, 10) == 0 and q(100, 4, 50, 129, 10) == 0 and q(100, 4, 50, 128, 10) > 0
    assert q(0, 4, 50, 4, 10) == 0 and q(100, 4, 50, 4, 0) == 0
    assert q(100, 4, 50, 4, 80000) == 0                                     # the sweep's LDS bound
    assert q(100, 1 << 20, 50, 128, 10) == 0                                # B * N * Sp beyond int32
    # the headline size of profiles/gram_ctc_nbest.txt is of this order: 3 L + 1 nodes instead of 2 L + 1
    assert 3.8e9 < q(1000, 32, 3000, 16, 120) < 4.1e9


def test_no_cpu_path():
    from asr import _lib
    from asr.loss import gram_ctc_nbest_logp
    gram = gref.table(((1,), (2,), (1, 2)))
    with pytest.raises(_lib.AsrHipError):
        gram_ctc_nbest_logp(torch.zeros(4, 2, 4), torch.ones(2, 3, 1, dtype=torch.int32), torch.ones(2, 3, dtype=torch.int32), gram, 0)


def test_table_checks_on_the_host():
    """asr.error's validation, and on top of it: every character a bigram row spells with has a unigram row"""
    from asr.loss import gram_ctc_nbest_logp, gram_mwer_loss
    x = torch.zeros(4, 2, 3)
    h, hl = torch.ones(2, 3, 1, dtype=torch.int32), torch.ones(2, 3, dtype=torch.int32)
    t = torch.ones(2, 2, dtype=torch.int32)
    bad = gref.table(((1,), (1, 2)))
    for table in (bad, torch.from_numpy(bad)):
        with pytest.raises(ValueError, match="unigram"):
            gram_ctc_nbest_logp(x, h, hl, table, 0)
        with pytest.raises(ValueError, match="unigram"):
            gram_mwer_loss(x, t, table, 0, hyps=h, hyp_lengths=hl)
    twice = gref.table(((1,), (1,)))
    with pytest.raises(ValueError, match="same spelling"):
        gram_ctc_nbest_logp(x, h, hl, twice, 0)
    with pytest.raises(ValueError):
        gram_ctc_nbest_logp(x, h, hl, gref.table(((1,), (2,), (1, 2))), 0)       # (4, 2) for V = 3


def test_add_reference_never_counts_the_transcript_twice():
    """the host-side logic gram_mwer_loss shares with mwer_loss, on strings of characters: exactly one slot in use equals the
    transcript, and mwer_parts gives the appended slot of an utterance that lists its transcript no mass"""
    from asr.loss import mwer_parts
    rs = np.random.RandomState(3)
    B, N, L = 3, 4, 6
    hyps = rs.randint(1, 5, size=(B, N, L)).astype(np.int32)
    hyp_len = rs.randint(1, L + 1, size=(B, N)).astype(np.int32)
    t = rs.randint(1, 5, size=(B, 8)).astype(np.int32)
    t_len = np.array([8, 3, 5], np.int32)
    hyps[1, 2, :3], hyp_len[1, 2] = t[1, :3], 3          # utterance 1 lists its transcript
    hyps[2, 1, :5], hyp_len[2, 1] = t[2, :5], -1         # utterance 2 holds it in an UNUSED slot: that does not count
    out, lens = ref.with_reference(hyps, hyp_len, t, t_len)
    assert out.shape == (B, N + 1, 8) and list(lens[:, N]) == [8, -1, 5]
    e = ref.errors(out, lens, t, t_len)
    for b in range(B):
        used = lens[b] >= 0
        assert int(((e[b] == 0) & used).sum()) == 1
    logp = -rs.uniform(1.0, 20.0, size=(B, N + 1))
    logp[lens < 0] = -np.inf
    loss, post = mwer_parts(torch.tensor(logp), torch.tensor(e))
    want_loss, want_post, _, _ = ref.mwer(logp, e)
    np.testing.assert_allclose(loss.numpy(), want_loss, rtol=0, atol=1e-12)
    np.testing.assert_allclose(post.numpy(), want_post, rtol=0, atol=1e-12)
    assert post[1, N].item() == 0.0 and post[0, N].item() > 0 and post[2, N].item() > 0 and post[2, 1].item() == 0.0
