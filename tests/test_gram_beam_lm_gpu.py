"""Gram-CTC beam search fused with a character n-gram language model on the GPU (asr_gram_ctc_beam_search_lm through
asr.error.gram_beam_decode_lm) against an exhaustive enumeration of every path, the float64 restatement of
tests/gram_beam_lm_reference.py, the project's GPU Gram-CTC loss and asr_ngram_score, the unfused string search and the
token-level fused search.

Tolerance: 1e-4 * max(1, |score|), `tol` of tests/test_ctc_beam_gpu.py (whose helpers, and those of tests/test_gram_beam_gpu.py and
tests/test_ctc_beam_lm_gpu.py, this file uses).
"""
import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as lmref
import gram_beam_lm_reference as glm
import gram_beam_reference as gref
import test_ctc_beam_gpu as base
import test_ctc_beam_lm_gpu as lmbase
import test_gram_beam_gpu as gbase
from test_ctc_beam_gpu import check_padding, compare_nbest, tol
from test_ctc_beam_lm_gpu import hyps4

pytestmark = pytest.mark.gpu

T_P, B_P, W_P, K_P = gref.T_P, gref.B_P, gref.W_P, gref.K_P
ALPHA, BETA = 0.5, 1.0
SEED_P = 20261019
ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -1, -2, -3


def make_lm(ng, V, marks=True):
    from asr import lm
    return lm.NGramLM.from_ngrams(ng, V, V if marks else None, V + 1 if marks else None)


def gfused(device, x, gram, model, alpha, beta, W, K, blank=0, lengths=None, min_logp=None, use_eos=True):
    """x (T, B, V) numpy -> numpy (ids (B, W, 2T), lens, scores, ctc, lm)"""
    from asr import error
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(device)
    out = error.gram_beam_decode_lm(xt, gram, model, alpha, beta, W, K, blank, lt, min_logp, use_eos)
    torch.cuda.synchronize()
    assert out[0].shape == (x.shape[1], W, 2 * x.shape[0])
    return tuple(o.cpu().numpy() for o in out)


def unused_slots_are_empty(out):
    unused = out[2] == -np.inf
    assert np.all(out[3][unused] == -np.inf) and np.all(out[4][unused] == 0.0) and np.all(out[1][unused] == 0)
    assert np.all(np.isfinite(out[3][~unused])) and np.all(np.isfinite(out[4][~unused]))


# ------------------------------------------------------------------------------------------------ 1. exhaustive
@pytest.mark.parametrize("case", gref.EXHAUSTIVE, ids=lambda c: "T%d_rows%d_s%d" % (c[0][0], len(c[0][1]), c[0][2]))
def test_exhaustive_fused_objective(device, case):
    (T, rows, seed), count = case
    alpha, beta = 0.7, 0.4
    gram = gref.table(rows)
    V = len(gram)
    x = gref.exhaustive_logits(T, V, seed)
    model = make_lm(glm.relabel_marks(lmref.exhaustive_model(3, seed), 3, V), V)      # characters 1 and 2
    d = lmref.DictLM.of(model)
    exact = gref.enumerate_strings(x, gram)
    assert len(exact) == count
    want = {s: (exact[s] + alpha * d.score(s) + beta * len(s), exact[s], d.score(s)) for s in exact}
    out = gfused(device, x[:, None, :], gram, model, alpha, beta, 128, V - 1)
    check_padding(out[0], out[1], out[2], 0)
    unused_slots_are_empty(out)
    got = hyps4(out, 0)
    strings = [g[0] for g in got]
    assert len(got) == count and len(set(strings)) == count and set(strings) == set(exact)
    assert np.all(out[2][0, count:] == -np.inf) and np.all(out[1][0, count:] == 0)
    worst = 0.0
    for s, sc, c, l in got:
        ws, wc, wl = want[s]
        worst = max(worst, abs(sc - ws) / tol(ws), abs(c - wc) / tol(wc), abs(l - wl) / tol(wl))
        assert abs(sc - ws) <= tol(ws) and abs(c - wc) <= tol(wc) and abs(l - wl) <= tol(wl), (s, sc, ws, c, wc, l, wl)
    print("case", case, "worst |score, ctc, lm - exact| / tol", worst)
    pos = {s: k for k, s in enumerate(strings)}
    order = sorted(want, key=lambda s: -want[s][0])
    for a, b in zip(order, order[1:]):
        if want[a][0] - want[b][0] > 2 * tol(want[b][0]):
            assert pos[a] < pos[b], (a, b, want[a][0], want[b][0])
    nonempty = [g for g in got if g[0]]
    loss = gbase.gpu_gram_scores(device, x, gram, [g[0] for g in nonempty])
    for (s, _, c, _), w in zip(nonempty, loss):
        assert abs(c - w) <= tol(w), (s, c, w)


# ------------------------------------------------------------------------------------------------ 2. pruned
@pytest.fixture(scope="module")
def pruned():
    """the pruned inputs of tests/test_gram_beam_gpu.py, the model built around the unfused restatement's top-1 strings of the
    full run (<s> / </s> relabelled from U_P + 1 / U_P + 2 to V / V + 1), and the fused restatement's N-best of the full and
    the ragged run (computed once)"""
    gram, x, lengths = gref.pruned_inputs()
    V = len(gram)
    top1 = [gref.beam_search(x[:, b], gram, W_P, K_P)[0][0] for b in range(B_P)]
    ng = lmref.random_model(np.random.RandomState(SEED_P), gref.U_P + 1, 3, top1, n_random=300)
    model = make_lm(glm.relabel_marks(ng, gref.U_P + 1, V), V)
    d = lmref.DictLM.of(model)
    out = {"gram": gram, "x": x, "lengths": lengths, "model": model, "d": d}
    for name, ln in (("full", None), ("ragged", lengths)):
        out[name] = [glm.beam_search_lm(x[:, b], gram, d, ALPHA, BETA, W_P, K_P, 0, None if ln is None else ln[b])
                     for b in range(B_P)]
    return out


@pytest.fixture(scope="module")
def decoded(device, pruned):
    """the GPU N-best of both runs (one launch each)"""
    return {run: gfused(device, pruned["x"], pruned["gram"], pruned["model"], ALPHA, BETA, W_P, K_P, 0,
                        None if run == "full" else pruned["lengths"]) for run in ("full", "ragged")}


@pytest.mark.parametrize("run", ["full", "ragged"])
def test_pruned_search_against_restatement(device, pruned, decoded, run):
    """compare_nbest's conditions with the cap B / 8 = 1; the restatement alone needs 0: its float32 twin
    (beam_search_lm(f32=True)) returns the float64 run's strings in the same order in 8 of 8 utterances, full and ragged, with a
    worst score gap of 0.0042 tol (full) and 0.0030 tol (ragged), and all 8 top-1 strings differ from the unfused search's
    (model seed 20261019; tests/test_gram_beam_lm_cpu.py asserts it)."""
    out = decoded[run]
    x, gram, model = pruned["x"], pruned["gram"], pruned["model"]
    ln = None if run == "full" else pruned["lengths"]
    check_padding(out[0], out[1], out[2], 0)
    unused_slots_are_empty(out)
    gpu = [hyps4(out, b) for b in range(B_P)]
    compare_nbest([[(g[0], g[1]) for g in hb] for hb in gpu], [[(w[0], w[1]) for w in wb] for wb in pruned[run]], B_P // 8)
    lm_dev = lmbase.device_lm_scores(device, model, out[0], out[1], True)
    img = model.host_image()
    worst = [0.0, 0.0, -np.inf]
    for b in range(B_P):
        assert len({g[0] for g in gpu[b]}) == len(gpu[b]), b                   # no string twice
        for i, (s, sc, c, l) in enumerate(gpu[b]):
            f = c + ALPHA * l + BETA * len(s)
            worst[0] = max(worst[0], abs(sc - f) / tol(f))
            assert abs(sc - f) <= tol(f), (b, s, sc, f)
            worst[1] = max(worst[1], abs(l - lm_dev[b, i]) / tol(lm_dev[b, i]))
            assert abs(l - lm_dev[b, i]) <= tol(lm_dev[b, i]), (b, s, l, lm_dev[b, i])
            # route independence: lm is the left-to-right float32 sum of the string's steps, then the eos step, bit for bit
            acc, ctx = np.float32(0.0), (model.bos,)
            for ch in s + (model.eos,):
                acc = np.float32(acc + lmref.step32(img, ctx, ch))
                ctx = (ctx + (ch,))[-3:]
            assert np.float32(out[4][b, i]).view(np.uint32) == acc.view(np.uint32), (b, s, out[4][b, i], acc)
        hb = [g for g in gpu[b] if g[0]]
        loss = gbase.gpu_gram_scores(device, x[:, b], gram, [g[0] for g in hb], None if ln is None else ln[b])
        for (s, _, c, _), w in zip(hb, loss):
            worst[2] = max(worst[2], (c - w) / tol(w))
            assert c <= w + tol(w), (b, s, c, w)
    print("worst |score - formula| / tol %.3g, |lm - ngram_score| / tol %.3g, largest (ctc - log p) / tol %.3g" % tuple(worst))
    plain = gbase.gbeam(device, x, gram, W_P, K_P, 0, ln)
    changed = sum(1 for b in range(B_P) if gpu[b][0][0] != base.hyps(*plain, b)[0][0])
    print("top-1 differs from gram_beam_decode's in %d of %d utterances" % (changed, B_P))
    assert changed >= 1


# ------------------------------------------------------------------------------------------------ 3. neutral weights
def check_neutral(device, x, gram, model, W, K, blank, lengths):
    a = gbase.gbeam(device, x, gram, W, K, blank, lengths)
    out = gfused(device, x, gram, model, 0.0, 0.0, W, K, blank, lengths, None, False)
    for u, v in zip(a, out[:3]):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    assert out[3].tobytes() == out[2].tobytes()
    unused_slots_are_empty(out)


@pytest.mark.parametrize("run", ["full", "ragged"])
def test_neutral_weights_reproduce_the_unfused_search_pruned_inputs(device, pruned, run):
    check_neutral(device, pruned["x"], pruned["gram"], pruned["model"], W_P, K_P, 0, None if run == "full" else pruned["lengths"])


@pytest.mark.parametrize("T,B,V,U,W,K,blank,seed", [
    (1, 3, 8, 3, 8, 4, 0, 11), (20, 3, 9, 3, 1, 5, 0, 12), (20, 3, 9, 3, 4, 1, 0, 13), (15, 3, 9, 3, 8, 5, 3, 14),
    (12, 2, 9, 3, 8, 64, 0, 16), (30, 2, 80, 10, 128, 32, 0, 17), (30, 2, 80, 10, 64, 64, 0, 18), (30, 2, 80, 10, 128, 1, 0, 19),
    (30, 2, 80, 10, 1, 64, 0, 20),
])
def test_neutral_weights_reproduce_the_unfused_search_edge_cases(device, T, B, V, U, W, K, blank, seed):
    check_neutral(device, base.small(T, B, V, seed), gref.random_table(V, U, seed, blank), edge_model(V, 4, seed), W, K, blank, None)


# ------------------------------------------------------------------------------------------------ 4. bigram-free table
def test_a_bigram_free_table_gives_beam_decode_lm(device, pruned):
    x = pruned["x"]
    T, _, V = x.shape
    gram = np.full((V, 2), -1, np.int32)
    gram[1:, 0] = np.arange(1, V)
    rs = np.random.RandomState(4)
    tr = [lmref.greedy(x[:, b]) for b in range(B_P)]
    model = make_lm(lmref.random_model(rs, V, 3, tr, n_random=3000), V)
    for ln in (None, pruned["lengths"]):
        got = gfused(device, x, gram, model, ALPHA, BETA, W_P, K_P, 0, ln)
        want = lmbase.fused(device, x, model, ALPHA, BETA, W_P, K_P, 0, ln)
        assert np.array_equal(got[0][..., :T], want[0]) and np.array_equal(got[1], want[1])
        assert np.all(got[0][..., T:] == 0)
        used = want[2] > -np.inf
        for g, w in zip(got[2:], want[2:]):
            assert np.array_equal(g[~used], w[~used])
            for u, v in zip(g[used], w[used]):
                assert abs(u - v) <= tol(v), (u, v)
        print("bitwise equal score, ctc, lm:", [g.tobytes() == w.tobytes() for g, w in zip(got[2:], want[2:])])


# ------------------------------------------------------------------------------------------------ 5. edge cases
def edge_model(V, order, seed, marks=True):
    """a random model of the given order over the ids 1 .. V - 1 (every unigram id of a table over V tokens)"""
    rs = np.random.RandomState(1000 + seed)
    ng = lmref.random_model(rs, V, order, [rs.randint(1, V, size=6).tolist() for _ in range(8)], n_random=300, bos=marks)
    return make_lm(ng, V, marks)


def against_restatement(device, x, gram, model, W, K, blank=0, lengths=None, use_eos=True):
    """slot by slot, with the rules of tests/test_gram_beam_gpu.py::against_restatement applied to the combined score"""
    out = gfused(device, x, gram, model, ALPHA, BETA, W, K, blank, lengths, None, use_eos)
    check_padding(out[0], out[1], out[2], blank)
    unused_slots_are_empty(out)
    d = lmref.DictLM.of(model)
    for b in range(x.shape[1]):
        want = glm.beam_search_lm(x[:, b], gram, d, ALPHA, BETA, W, K, blank, None if lengths is None else lengths[b],
                                  use_eos=use_eos)
        got = hyps4(out, b)
        assert len(got) == len(want), (b, len(got), len(want))
        assert len({g[0] for g in got}) == len(got), b
        for g, w in zip(got, want):
            assert abs(g[1] - w[1]) <= tol(w[1]), (b, g, w)
        gs, ws = {g[0]: g for g in got}, {w[0]: w for w in want}
        for s in set(gs) & set(ws):
            for k in (1, 2, 3):                            # score, ctc, lm
                assert abs(gs[s][k] - ws[s][k]) <= tol(ws[s][k]), (b, s, k, gs[s], ws[s])
        for s in set(gs) - set(ws):
            assert gs[s][1] <= want[-1][1] + tol(want[-1][1]), (b, s)
        for s in set(ws) - set(gs):
            assert ws[s][1] <= got[-1][1] + tol(got[-1][1]), (b, s)
        print("utterance %d: %d hypotheses, %d on one side only, longest %d"
              % (b, len(got), len(set(gs) ^ set(ws)), out[1][b].max()))
    return out


@pytest.mark.parametrize("T,B,V,U,W,K,blank,seed,order,marks,use_eos", [
    (1, 3, 8, 3, 8, 4, 0, 11, 4, True, True),            # T = 1
    (20, 3, 9, 3, 1, 5, 0, 12, 1, True, True),           # beam_width = 1; unigrams only: no hash table
    (20, 3, 9, 3, 4, 1, 0, 13, 2, True, True),           # top_k = 1
    (15, 3, 9, 3, 8, 5, 3, 14, 4, False, True),          # blank id other than 0; a model without <s> / </s>
    (12, 2, 9, 3, 8, 64, 0, 16, 2, True, False),         # top_k above V - 1; no end term
    (30, 2, 80, 10, 128, 32, 0, 17, 4, True, True),      # the largest accepted shapes
    (30, 2, 80, 10, 64, 64, 0, 18, 4, True, True),
])
def test_edge_cases_against_restatement(device, T, B, V, U, W, K, blank, seed, order, marks, use_eos):
    model = edge_model(V, order, seed, marks)
    assert (model.host_image()["slots"] == 0) == (order == 1)
    against_restatement(device, base.small(T, B, V, seed), gref.random_table(V, U, seed, blank), model, W, K, blank, None, use_eos)


def test_an_inventory_without_unigram_rows(device):
    """every extension takes two steps"""
    gram = gref.random_table(10, 3, 21, all_bigram=True)
    assert not np.any((gram[:, 0] >= 0) & (gram[:, 1] < 0)) and np.sum(gram[:, 1] >= 0) == 9
    out = against_restatement(device, base.small(14, 2, 10, 21), gram, edge_model(10, 4, 21), 16, 9)
    assert np.all(out[1] % 2 == 0)


def test_rows_that_spell_nothing_among_the_top_candidates(device):
    gram = gref.random_table(12, 3, 22, dead=3)
    dead = [v for v in range(1, 12) if gram[v, 0] < 0]
    assert len(dead) == 3
    x = base.small(16, 2, 12, 22)
    x[:, :, dead] += 3.0
    against_restatement(device, x, gram, edge_model(12, 3, 22), 8, 4)


def test_a_length_zero_utterance_in_a_ragged_batch(device):
    gram = gref.random_table(9, 3, 23)
    model = edge_model(9, 3, 23)
    lengths = np.array([0, 13, 6], np.int32)
    out = against_restatement(device, base.small(13, 3, 9, 23), gram, model, 8, 5, 0, lengths)
    end = lmref.step32(model.host_image(), (model.bos,), model.eos)
    assert out[1][0, 0] == 0 and out[3][0, 0] == 0.0 and np.all(out[2][0, 1:] == -np.inf) and np.all(out[0][0] == 0)
    assert out[4][0, 0] == end and abs(out[2][0, 0] - ALPHA * float(end)) <= tol(ALPHA * float(end))
    plain = gfused(device, base.small(13, 3, 9, 23), gram, model, ALPHA, BETA, 8, 5, 0, lengths, None, False)
    assert plain[4][0, 0] == 0.0 and plain[2][0, 0] == 0.0 and plain[3][0, 0] == 0.0


def test_a_hypothesis_longer_than_the_number_of_frames(device):
    gram = gref.random_table(30, 5, 24)
    x = np.stack([gref.bigram_run(12, gram, 24 + b) for b in range(2)], axis=1)
    out = against_restatement(device, x, gram, edge_model(30, 4, 24), 16, 8)
    assert np.all(out[1][:, 0] == 24)                      # T = 12 frames, a bigram token on every one


# ------------------------------------------------------------------------------------------------ 6. padding, repeat
def test_padding_frames_are_never_read_and_launches_repeat_bitwise(device, pruned, decoded):
    x, lengths, gram, model = pruned["x"], pruned["lengths"], pruned["gram"], pruned["model"]
    a = decoded["ragged"]
    a2 = gfused(device, x, gram, model, ALPHA, BETA, W_P, K_P, 0, lengths)
    rs = np.random.RandomState(7)
    y = x.copy()
    for b in range(B_P):
        y[lengths[b]:, b] = (rs.randn(T_P - lengths[b], x.shape[2]) * 20).astype(np.float32)
    c = gfused(device, y, gram, model, ALPHA, BETA, W_P, K_P, 0, lengths)
    for u, v, w in zip(a, a2, c):
        assert u.tobytes() == v.tobytes() == w.tobytes()


# ------------------------------------------------------------------------------------------------ 7. limits
def _raw_call(device, model, T, B, V, W, K, nbytes=None, with_gram=True, order=None, slots=None, max_probe=None, vlm=None,
              bos=None):
    from asr import _lib
    lib = _lib.lib()
    model.to(device)
    img = model.image
    x = torch.zeros((T, B, V), dtype=torch.float32, device=device)
    gram = torch.full((V, 2), -1, dtype=torch.int32, device=device)
    gram[1:, 0] = torch.arange(1, V, dtype=torch.int32, device=device)
    need = lib.asr_gram_ctc_beam_lm_workspace_bytes(T, B, V, W, K)
    assert need >= lib.asr_gram_ctc_beam_workspace_bytes(T, B, V, W, K)
    nbytes = need if nbytes is None else nbytes(need)
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=device)
    ids = torch.empty((B, W, 2 * T), dtype=torch.int32, device=device)
    ln = torch.empty((B, W), dtype=torch.int32, device=device)
    sc, cc, lc = (torch.empty((B, W), dtype=torch.float32, device=device) for _ in range(3))
    rc = lib.asr_gram_ctc_beam_search_lm(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"),
                                         _lib.ptr(gram) if with_gram else None, _lib.ptr(img["uni"]),
                                         img["uni"].shape[0] if vlm is None else vlm, _lib.ptr(img["keys"]), _lib.ptr(img["vals"]),
                                         img["slots"] if slots is None else slots,
                                         img["max_probe"] if max_probe is None else max_probe,
                                         img["order"] if order is None else order, model.bos_id if bos is None else bos,
                                         model.eos_id, 0.5, 1.0, _lib.ptr(ws), nbytes, _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc),
                                         _lib.ptr(cc), _lib.ptr(lc))
    torch.cuda.synchronize()
    return rc


def test_limits_workspace_and_model_arguments(device):
    V = 100
    model = make_lm(lmref.random_model(np.random.RandomState(3), V, 3, n_random=500), V)
    for W, K in ((129, 1), (1, 65), (65, 64), (128, 33), (128, 64)):
        assert _raw_call(device, model, 4, 1, V, W, K) == ASR_ERR_UNSUPPORTED, (W, K)
    assert _raw_call(device, model, 4, 1, V, 16, 16, lambda n: n - 1) == ASR_ERR_WORKSPACE
    assert _raw_call(device, model, 4, 1, V, 16, 16, with_gram=False) == ASR_ERR_UNSUPPORTED
    assert _raw_call(device, model, 4, 1, V, 128, 32) == 0 and _raw_call(device, model, 4, 1, V, 64, 64) == 0
    assert _raw_call(device, model, 4, 1, V, 16, 16, order=5) == ASR_ERR_UNSUPPORTED
    assert _raw_call(device, model, 4, 1, V, 16, 16, slots=12) == ASR_ERR_BAD_ARG
    assert _raw_call(device, model, 4, 1, V, 16, 16, max_probe=0) == ASR_ERR_BAD_ARG
    assert _raw_call(device, model, 4, 1, V, 16, 16, vlm=V - 1) == ASR_ERR_BAD_ARG
    assert _raw_call(device, model, 4, 1, V, 16, 16, bos=V + 2) == ASR_ERR_BAD_ARG
    assert _raw_call(device, model, 4, 1, V, 16, 16) == 0


# ------------------------------------------------------------------------------------------------ 8. known strings
def test_known_strings_decode_with_error_rate_zero(device, pruned):
    from asr import error
    gram = pruned["gram"]
    V = len(gram)
    x, strings = gref.known_strings(4, 60, gram, 9)
    ng = lmref.random_model(np.random.RandomState(9), gref.U_P + 1, 3, strings, n_random=300)
    model = make_lm(glm.relabel_marks(ng, gref.U_P + 1, V), V)
    out = gfused(device, x, gram, model, ALPHA, BETA, 8, 8)
    for b, s in enumerate(strings):
        assert tuple(out[0][b, 0, :out[1][b, 0]]) == s
    t = np.zeros((4, max(len(s) for s in strings)), np.int32)
    for b, s in enumerate(strings):
        t[b, :len(s)] = s
    assert error.compute_sequence_error(out[0][:, 0], out[1][:, 0], t, 0, None, None) == 0.0
