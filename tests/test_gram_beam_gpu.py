"""Gram-CTC beam search over spelled strings on the GPU (asr_gram_ctc_beam_search through asr.error.gram_beam_decode) against
an exhaustive enumeration of every path, the project's own GPU Gram-CTC loss, the float64 restatement of
tests/gram_beam_reference.py and the token-level decoder.

Tolerance: 1e-4 * max(1, |score|), the project's CTC loss tolerance, as in tests/test_ctc_beam_gpu.py (whose helpers this file
uses): a score here is a Gram-CTC log-probability.
"""
import numpy as np
import pytest
import torch

import gram_beam_reference as gref
import test_ctc_beam_gpu as base
from test_ctc_beam_gpu import check_padding, compare_nbest, hyps, tol

pytestmark = pytest.mark.gpu

T_P, B_P, W_P, K_P = gref.T_P, gref.B_P, gref.W_P, gref.K_P
ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -2, -3


def gbeam(device, x, gram, W, K, blank=0, lengths=None, min_logp=None):
    """x (T, B, V) f32 numpy -> numpy (ids (B, W, 2T), lens (B, W), scores (B, W))"""
    from asr import error
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(device)
    ids, lens, scores = error.gram_beam_decode(xt, gram, W, K, blank, lt, min_logp)
    torch.cuda.synchronize()
    assert ids.shape == (x.shape[1], W, 2 * x.shape[0])
    return ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()


def gpu_gram_scores(device, x, gram, strings, length=None):
    """-(the project's GPU Gram-CTC loss) of every (non-empty) string over one utterance's logits x (T, V), as one batch, with
    every bigram of the table offered: label_bigram[i] = the id of (u[i-1], u[i]) or -1"""
    from asr.loss import gram_ctc
    uni = gref.unigram_ids(gram)
    n = len(strings)
    L = max(len(s) for s in strings)
    lu = np.zeros((n, L), np.int32)
    lb = np.full((n, L), -1, np.int32)
    for i, s in enumerate(strings):
        lu[i, :len(s)] = [uni[u] for u in s]
        lb[i, :len(s)] = gref.label_bigrams(s, gram)
    xs = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)[:, None, :].expand(-1, n, -1).contiguous()
    xl = None if length is None else torch.full((n,), int(length), dtype=torch.int32, device=device)
    ll = torch.tensor([len(s) for s in strings], dtype=torch.int32, device=device)
    with torch.no_grad():
        loss = gram_ctc(xs, torch.from_numpy(lu).to(device), torch.from_numpy(lb).to(device), 0, xl, ll, "no")
    return -loss.double().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. exhaustive
@pytest.mark.parametrize("case", gref.EXHAUSTIVE, ids=lambda c: "T%d_rows%d_s%d" % (c[0][0], len(c[0][1]), c[0][2]))
def test_exhaustive_against_enumeration_and_gram_ctc_loss(device, case):
    (T, rows, seed), count = case
    gram = gref.table(rows)
    V = len(gram)
    x = gref.exhaustive_logits(T, V, seed)
    exact = gref.enumerate_strings(x, gram)
    assert len(exact) == count
    ids, lens, scores = gbeam(device, x[:, None, :], gram, 128, V - 1)
    check_padding(ids, lens, scores, 0)
    got = hyps(ids, lens, scores, 0)
    strings = [s for s, _ in got]
    sc = np.array([v for _, v in got])
    print("case", case, "returned", len(got), "worst |score - exact| / tol",
          max(abs(v - exact[s]) / tol(exact[s]) for s, v in got if s in exact))
    assert len(got) == count and len(set(strings)) == count and set(strings) == set(exact)
    assert np.all(np.isfinite(sc))
    assert np.all(scores[0, count:] == -np.inf) and np.all(lens[0, count:] == 0)
    for s, v in got:
        assert abs(v - exact[s]) <= tol(exact[s]), (s, v, exact[s])
    order = sorted(exact, key=lambda s: -exact[s])
    pos = {s: k for k, s in enumerate(strings)}
    for a, b in zip(order, order[1:]):
        if exact[a] - exact[b] > 2 * tol(exact[b]):
            assert pos[a] < pos[b], (a, b, exact[a], exact[b])
    nonempty = [s for s in strings if s]
    loss = gpu_gram_scores(device, x, gram, nonempty)
    for s, c in zip(nonempty, loss):
        v = sc[strings.index(s)]
        assert abs(v - c) <= tol(c), (s, v, c)


# ------------------------------------------------------------------------------------------------ 2. pruned
@pytest.fixture(scope="module")
def pruned():
    """the inputs of tests 2, 3, 4, 7 and 8 and the restatement's N-best of the full and the ragged run (computed once)"""
    gram, x, lengths = gref.pruned_inputs()
    out = {"gram": gram, "x": x, "lengths": lengths}
    for name, ln in (("full", None), ("ragged", lengths)):
        out[name] = [gref.beam_search(x[:, b], gram, W_P, K_P, 0, None if ln is None else ln[b]) for b in range(B_P)]
    return out


@pytest.fixture(scope="module")
def decoded(device, pruned):
    """the GPU N-best of both runs (one launch each)"""
    return {run: gbeam(device, pruned["x"], pruned["gram"], W_P, K_P, 0, None if run == "full" else pruned["lengths"])
            for run in ("full", "ragged")}


@pytest.mark.parametrize("run", ["full", "ragged"])
def test_pruned_search_against_restatement(pruned, decoded, run):
    """compare_nbest's conditions with the cap B / 8 = 1.  A float32-accumulating run of the restatement
    (beam_search(f32=True)) differs from the float64 one in 0 of the 8 utterances on these inputs, full and ragged; the worst
    score gap between the two is 0.0043 tol."""
    ids, lens, scores = decoded[run]
    check_padding(ids, lens, scores, 0)
    gpu = [hyps(ids, lens, scores, b) for b in range(B_P)]
    compare_nbest(gpu, pruned[run], B_P // 8)


# ------------------------------------------------------------------------------------------------ 3. lower bound
@pytest.mark.parametrize("run", ["full", "ragged"])
def test_scores_are_lower_bounds_of_the_gram_ctc_loss(device, pruned, decoded, run):
    ids, lens, scores = decoded[run]
    ln = None if run == "full" else pruned["lengths"]
    worst = -np.inf
    for b in range(B_P):
        hb = [(s, v) for s, v in hyps(ids, lens, scores, b) if s]
        loss = gpu_gram_scores(device, pruned["x"][:, b], pruned["gram"], [s for s, _ in hb], None if ln is None else ln[b])
        for (s, v), c in zip(hb, loss):
            worst = max(worst, (v - c) / tol(c))
            assert v <= c + tol(c), (b, s, v, c)
    print("largest (score - log p) / tol:", worst)


# ------------------------------------------------------------------------------------------------ 4. merging is real
@pytest.mark.parametrize("run", ["full", "ragged"])
def test_top1_is_at_least_the_token_level_nbest_summed_per_string(device, pruned, decoded, run):
    ids, lens, scores = decoded[run]
    ln = None if run == "full" else pruned["lengths"]
    tid, tlen, tsc = base.beam(device, pruned["x"], W_P, K_P, 0, ln)
    gains = []
    for b in range(B_P):
        got = hyps(ids, lens, scores, b)
        assert len({s for s, _ in got}) == len(got), b                   # no string twice
        agg = gref.token_nbest_by_string(hyps(tid, tlen, tsc, b), pruned["gram"])
        best = max(agg.values())
        gains.append(got[0][1] - best)
        assert got[0][1] >= best - tol(best), (b, got[0][1], best)
    print("top-1 score minus the best of the token-level N-best summed per string:", np.round(gains, 4))


# ------------------------------------------------------------------------------------------------ 5. bigram-free table
def test_a_bigram_free_table_gives_beam_decode(device, pruned):
    x = pruned["x"]
    T, _, V = x.shape
    gram = np.full((V, 2), -1, np.int32)
    gram[1:, 0] = np.arange(1, V)
    for ln in (None, pruned["lengths"]):
        ids, lens, scores = gbeam(device, x, gram, W_P, K_P, 0, ln)
        tid, tlen, tsc = base.beam(device, x, W_P, K_P, 0, ln)
        assert np.array_equal(ids[..., :T], tid) and np.array_equal(lens, tlen)
        assert np.all(ids[..., T:] == 0)
        used = tsc > -np.inf
        assert np.array_equal(scores > -np.inf, used)
        for g, w in zip(scores[used], tsc[used]):
            assert abs(g - w) <= tol(w)
        print("bitwise equal scores:", scores.tobytes() == tsc.tobytes())


# ------------------------------------------------------------------------------------------------ 6. edge cases
def against_restatement(device, x, gram, W, K, blank=0, lengths=None):
    """slot by slot, as tests/test_ctc_beam_gpu.py::test_edge_cases_against_restatement"""
    ids, lens, scores = gbeam(device, x, gram, W, K, blank, lengths)
    check_padding(ids, lens, scores, blank)
    for b in range(x.shape[1]):
        want = gref.beam_search(x[:, b], gram, W, K, blank, None if lengths is None else lengths[b])
        got = hyps(ids, lens, scores, b)
        assert len(got) == len(want), (b, len(got), len(want))
        assert len({s for s, _ in got}) == len(got), b
        for (_, g), (_, w) in zip(got, want):
            assert abs(g - w) <= tol(w), (b, g, w)
        gs, ws = dict(got), dict(want)
        for s in set(gs) & set(ws):
            assert abs(gs[s] - ws[s]) <= tol(ws[s]), (b, s)
        for s in set(gs) - set(ws):
            assert gs[s] <= want[-1][1] + tol(want[-1][1]), (b, s)
        for s in set(ws) - set(gs):
            assert ws[s] <= got[-1][1] + tol(got[-1][1]), (b, s)
        print("utterance %d: %d hypotheses, %d on one side only, longest %d" % (b, len(got), len(set(gs) ^ set(ws)), lens[b].max()))
    return ids, lens, scores


@pytest.mark.parametrize("T,B,V,U,W,K,blank,seed", [
    (1, 3, 8, 3, 8, 4, 0, 11),           # T = 1
    (20, 3, 9, 3, 1, 5, 0, 12),          # beam_width = 1
    (20, 3, 9, 3, 4, 1, 0, 13),          # top_k = 1
    (15, 3, 9, 3, 8, 5, 3, 14),          # blank id other than 0
    (12, 2, 9, 3, 8, 64, 0, 16),         # top_k above V - 1
    (30, 2, 80, 10, 128, 32, 0, 17),      # the largest accepted shapes
    (30, 2, 80, 10, 64, 64, 0, 18),
    (30, 2, 80, 10, 128, 1, 0, 19),
    (30, 2, 80, 10, 1, 64, 0, 20),
])
def test_edge_cases_against_restatement(device, T, B, V, U, W, K, blank, seed):
    against_restatement(device, base.small(T, B, V, seed), gref.random_table(V, U, seed, blank), W, K, blank)


def test_an_inventory_without_unigram_rows(device):
    gram = gref.random_table(10, 3, 21, all_bigram=True)
    assert not np.any((gram[:, 0] >= 0) & (gram[:, 1] < 0)) and np.sum(gram[:, 1] >= 0) == 9
    _, lens, _ = against_restatement(device, base.small(14, 2, 10, 21), gram, 16, 9)
    assert np.all(lens % 2 == 0)


def test_rows_that_spell_nothing_among_the_top_candidates(device):
    gram = gref.random_table(12, 3, 22, dead=3)
    dead = [v for v in range(1, 12) if gram[v, 0] < 0]
    assert len(dead) == 3
    x = base.small(16, 2, 12, 22)
    x[:, :, dead] += 3.0
    against_restatement(device, x, gram, 8, 4)


def test_a_length_zero_utterance_in_a_ragged_batch(device):
    gram = gref.random_table(9, 3, 23)
    lengths = np.array([0, 13, 6], np.int32)
    ids, lens, scores = against_restatement(device, base.small(13, 3, 9, 23), gram, 8, 5, 0, lengths)
    assert lens[0, 0] == 0 and scores[0, 0] == 0.0 and np.all(scores[0, 1:] == -np.inf) and np.all(ids[0] == 0)


def test_a_hypothesis_longer_than_the_number_of_frames(device):
    gram = gref.random_table(30, 5, 24)
    x = np.stack([gref.bigram_run(12, gram, 24 + b) for b in range(2)], axis=1)
    _, lens, _ = against_restatement(device, x, gram, 16, 8)
    assert np.all(lens[:, 0] == 24)                      # T = 12 frames, a bigram token on every one


def _raw_call(device, T, B, V, W, K, nbytes=None, with_gram=True):
    from asr import _lib
    lib = _lib.lib()
    x = torch.zeros((T, B, V), dtype=torch.float32, device=device)
    gram = torch.full((V, 2), -1, dtype=torch.int32, device=device)
    gram[1:, 0] = torch.arange(1, V, dtype=torch.int32, device=device)
    need = lib.asr_gram_ctc_beam_workspace_bytes(T, B, V, W, K)
    nbytes = need if nbytes is None else nbytes(need)
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=device)
    ids = torch.empty((B, W, 2 * T), dtype=torch.int32, device=device)
    ln = torch.empty((B, W), dtype=torch.int32, device=device)
    sc = torch.empty((B, W), dtype=torch.float32, device=device)
    rc = lib.asr_gram_ctc_beam_search(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"),
                                      _lib.ptr(gram) if with_gram else None, _lib.ptr(ws), nbytes, _lib.ptr(ids), _lib.ptr(ln),
                                      _lib.ptr(sc))
    torch.cuda.synchronize()
    return rc


def test_limits_and_workspace(device):
    for W, K in ((129, 1), (1, 65), (65, 64), (128, 33), (128, 64)):
        assert _raw_call(device, 4, 1, 100, W, K) == ASR_ERR_UNSUPPORTED, (W, K)
    assert _raw_call(device, 4, 1, 100, 16, 16, lambda n: n - 1) == ASR_ERR_WORKSPACE
    assert _raw_call(device, 4, 1, 100, 16, 16, with_gram=False) == ASR_ERR_UNSUPPORTED
    assert _raw_call(device, 4, 1, 100, 128, 32) == 0 and _raw_call(device, 4, 1, 100, 64, 64) == 0


def test_table_validation(device):
    from asr import error
    x = torch.zeros((3, 1, 4), dtype=torch.float32, device=device)
    good = gref.table(((1,), (2,), (1, 2)))
    error.gram_beam_decode(x, good, 4, 3)
    error.gram_beam_decode(x, torch.from_numpy(good).to(device), 4, 3)
    for row, value in ((0, (1, -1)), (3, (1, 4)), (3, (-1, 2)), (2, (1, -1))):
        bad = good.copy()
        bad[row] = value
        with pytest.raises(ValueError):
            error.gram_beam_decode(x, bad, 4, 3)
        with pytest.raises(ValueError):
            error.gram_beam_decode(x, torch.from_numpy(bad).to(device), 4, 3)
    with pytest.raises(ValueError):
        error.gram_beam_decode(x, good[:3], 4, 3)


# ------------------------------------------------------------------------------------------------ 7. padding, repeat
def test_padding_frames_are_never_read_and_launches_repeat_bitwise(device, pruned, decoded):
    x, lengths, gram = pruned["x"], pruned["lengths"], pruned["gram"]
    a = decoded["ragged"]
    a2 = gbeam(device, x, gram, W_P, K_P, 0, lengths)
    rs = np.random.RandomState(7)
    y = x.copy()
    for b in range(B_P):
        y[lengths[b]:, b] = (rs.randn(T_P - lengths[b], x.shape[2]) * 20).astype(np.float32)
    c = gbeam(device, y, gram, W_P, K_P, 0, lengths)
    for u, v, w in zip(a, a2, c):
        assert u.tobytes() == v.tobytes() == w.tobytes()


# ------------------------------------------------------------------------------------------------ 8. error rate
def levenshtein(r, h):
    d = list(range(len(h) + 1))
    for i, a in enumerate(r, 1):
        prev, d[0] = d[0], i
        for j, b in enumerate(h, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (a != b))
    return d[len(h)]


def test_slot_0_goes_straight_into_compute_sequence_error(device, pruned, decoded):
    from asr import error
    ids, lens, _ = decoded["full"]
    rs = np.random.RandomState(8)
    labels = []
    for b in range(B_P):                                  # the restatement's best string with a few edits
        s = list(pruned["full"][b][0][0])
        for _ in range(3):
            s[rs.randint(len(s))] = int(rs.randint(1, gref.U_P + 1))
        del s[rs.randint(len(s))]
        labels.append(s)
    t = np.zeros((B_P, max(len(s) for s in labels)), np.int32)
    for b, s in enumerate(labels):
        t[b, :len(s)] = s
    want = np.mean([levenshtein(s, list(ids[b, 0, :lens[b, 0]])) / len(s) for b, s in enumerate(labels)])
    got = error.compute_sequence_error(ids[:, 0], lens[:, 0], t, 0, None, None)
    assert want > 0 and abs(got - want) <= 1e-12, (got, want)


def test_known_strings_decode_with_error_rate_zero(device, pruned):
    from asr import error
    x, strings = gref.known_strings(4, 60, pruned["gram"], 9)
    ids, lens, scores = gbeam(device, x, pruned["gram"], 8, 8)
    for b, s in enumerate(strings):
        assert tuple(ids[b, 0, :lens[b, 0]]) == s
    t = np.zeros((4, max(len(s) for s in strings)), np.int32)
    for b, s in enumerate(strings):
        t[b, :len(s)] = s
    assert error.compute_sequence_error(ids[:, 0], lens[:, 0], t, 0, None, None) == 0.0
