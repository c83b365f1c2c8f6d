"""The n-gram language model and the fused beam search on the GPU (csrc/ngram.hpp, csrc/ctc_beam.hip through asr.lm.NGramLM and
asr.error.beam_decode_lm) against the restatements of tests/ctc_beam_lm_reference.py, the unfused decoder and the project's
own GPU CTC loss.

Tolerance: 1e-4 * max(1, |score|), as in tests/test_ctc_beam_gpu.py (whose helpers this file uses).
"""
import json
import os

import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref
import test_ctc_beam_gpu as base
from test_ctc_beam_gpu import tol

pytestmark = pytest.mark.gpu

T_FULL, B_FULL, V_FULL, W_FULL, K_FULL = lmref.T_FULL, lmref.B_FULL, lmref.V_FULL, 16, 16
ALPHA, BETA = 0.5, 1.0
ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -1, -2, -3


def make_lm(ng, V, bos=True):
    from asr import lm
    return lm.NGramLM.from_ngrams(ng, V, V if bos else None, V + 1 if bos else None)


def fused(device, x, model, alpha, beta, W, K, blank=0, lengths=None, min_logp=None, use_eos=True):
    """x (T, B, V) numpy -> numpy (ids, lens, scores, ctc, lm)"""
    from asr import error
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(device)
    out = error.beam_decode_lm(xt, model, alpha, beta, W, K, blank, lt, min_logp, use_eos)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def hyps4(out, b):
    """the used slots of utterance b: [(labels, score, ctc, lm)] in slot order"""
    ids, lens, scores, ctc, lm = out
    return [(tuple(int(c) for c in ids[b, i, :lens[b, i]]), float(scores[b, i]), float(ctc[b, i]), float(lm[b, i]))
            for i in range(ids.shape[1]) if scores[b, i] > -np.inf]


def device_lm_scores(device, model, ids, lens, use_eos):
    """asr_ngram_score of every slot: ids (B, W, T), lens (B, W) -> (B, W) float64"""
    B, W, T = ids.shape
    it = torch.from_numpy(np.ascontiguousarray(ids.reshape(B * W, T))).to(device)
    lt = torch.from_numpy(np.ascontiguousarray(lens.reshape(B * W))).to(device)
    _, total = model.score(it, lt, True, use_eos)
    return total.double().cpu().numpy().reshape(B, W)


# ------------------------------------------------------------------------------------------------ 1. ngram_score
def mixed_sequences(rs, ng, V, N, Lmax):
    """sequences that chain n-grams of the model and random tokens, some empty"""
    high = [k for k in ng if len(k) > 1 and max(k) < V]
    seqs = []
    for i in range(N):
        L = 0 if i % 9 == 4 else int(rs.randint(1, Lmax + 1))
        s = []
        while len(s) < L:
            if high and rs.rand() < 0.6:
                s += list(high[rs.randint(len(high))])
            else:
                s.append(int(rs.randint(1, V)))
        seqs.append(s[:L])
    return seqs


@pytest.mark.parametrize("order", [1, 3, 4])
@pytest.mark.parametrize("marks", [True, False], ids=["bos_eos", "plain"])
def test_ngram_score_bits_and_sums(device, order, marks):
    V, N, Lmax = 3000, 40, 200
    rs = np.random.RandomState(40 + order)
    tr = [rs.randint(1, V, size=30).tolist() for _ in range(20)]
    ng = lmref.random_model(rs, V, order, tr, n_random=60000)
    model = make_lm(ng, V)
    img = model.host_image()
    assert (img["slots"] == 0) == (order == 1)                # order 1: all unigrams, no hash table
    d = lmref.DictLM.of(model)
    seqs = mixed_sequences(rs, ng, V, N, Lmax)
    ids = np.zeros((N, Lmax), np.int32)
    lens = np.array([len(s) for s in seqs], np.int32)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = s
        ids[i, len(s):] = rs.randint(1, V, size=Lmax - len(s))     # past the length: never scored
    tok, total = model.score(torch.from_numpy(ids).to(device), torch.from_numpy(lens).to(device), marks, marks)
    torch.cuda.synchronize()
    tok, total = tok.cpu().numpy(), total.cpu().numpy()
    worst = 0.0
    for i, s in enumerate(seqs):
        want = np.array(lmref.score32(img, s, model.bos if marks else None), np.float32)
        assert np.array_equal(tok[i, :len(s)].view(np.uint32), want.view(np.uint32)), i
        assert np.all(tok[i, len(s):] == 0.0)
        exact = d.score(s, marks, marks)
        worst = max(worst, abs(float(total[i]) - exact) / tol(exact))
        assert abs(float(total[i]) - exact) <= tol(exact), (i, total[i], exact)
    hits = sum(1 for s in seqs for j in range(1, len(s)) if tuple(s[j - 1:j + 1]) in ng)
    print("order %d marks %s: %d tokens bit-identical, %d bigram hits, worst |sum - float64| / tol %.3g"
          % (order, marks, int(lens.sum()), hits, worst))
    assert order == 1 or hits > 200


# ------------------------------------------------------------------------------------------------ shared full-size inputs
@pytest.fixture(scope="module")
def fullm():
    x, lengths, ng = lmref.full_inputs()
    model = make_lm(ng, V_FULL)
    d = lmref.DictLM.of(model)
    want = [lmref.beam_search_lm(x[:, b], d, ALPHA, BETA, W_FULL, K_FULL, 0, int(lengths[b])) for b in range(B_FULL)]
    return dict(x=x, lengths=lengths, model=model, d=d, want=want)


# ------------------------------------------------------------------------------------------------ 2. neutral weights
def check_neutral(device, x, model, W, K, blank, lengths):
    a = base.beam(device, x, W, K, blank, lengths)
    out = fused(device, x, model, 0.0, 0.0, W, K, blank, lengths, None, False)
    for u, v in zip(a, out[:3]):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    assert out[3].tobytes() == out[2].tobytes()
    lm_dev = device_lm_scores(device, model, out[0], out[1], False)
    used = out[2] > -np.inf
    worst = 0.0
    for b, i in zip(*np.nonzero(used)):
        worst = max(worst, abs(out[4][b, i] - lm_dev[b, i]) / tol(lm_dev[b, i]))
        assert abs(out[4][b, i] - lm_dev[b, i]) <= tol(lm_dev[b, i]), (b, i, out[4][b, i], lm_dev[b, i])
    assert np.all(out[4][~used] == 0.0)
    return worst


@pytest.mark.parametrize("run", ["full", "ragged"])
def test_neutral_weights_reproduce_the_unfused_decoder_full_size(device, fullm, run):
    worst = check_neutral(device, fullm["x"], fullm["model"], W_FULL, K_FULL, 0, None if run == "full" else fullm["lengths"])
    print("neutral %s: bitwise equal to beam_decode; worst |lm - ngram_score| / tol %.3g" % (run, worst))


@pytest.mark.parametrize("T,B,V,W,K,blank,seed", [
    (1, 3, 5, 8, 4, 0, 11), (20, 3, 6, 1, 5, 0, 12), (20, 3, 6, 4, 1, 0, 13), (15, 3, 6, 8, 5, 3, 14), (2, 2, 3, 16, 2, 0, 15),
    (12, 2, 9, 8, 64, 0, 16), (30, 2, 80, 128, 32, 0, 17), (30, 2, 80, 64, 64, 0, 18), (30, 2, 80, 128, 1, 0, 19),
    (30, 2, 80, 1, 64, 0, 20),
])
def test_neutral_weights_reproduce_the_unfused_decoder_edge_cases(device, T, B, V, W, K, blank, seed):
    rs = np.random.RandomState(seed)
    ng = lmref.random_model(rs, V, 4, [rs.randint(0, V, size=6).tolist() for _ in range(8)], n_random=300)
    check_neutral(device, base.small(T, B, V, seed), make_lm(ng, V), W, K, blank, None)


# ------------------------------------------------------------------------------------------------ 3. exhaustive
@pytest.mark.parametrize("case", ref.EXHAUSTIVE, ids=lambda c: "T%d_V%d_W%d_s%d" % c[0])
def test_exhaustive_fused_objective(device, case):
    (T, V, W, seed), count = case
    alpha, beta = 0.7, 0.4
    x = ref.exhaustive_logits(T, V, seed)
    model = make_lm(lmref.exhaustive_model(V, seed), V)
    d = lmref.DictLM.of(model)
    exact = ref.enumerate_paths(x)
    want = {lab: (exact[lab] + alpha * d.score(lab) + beta * len(lab), exact[lab], d.score(lab)) for lab in exact}
    out = fused(device, x[:, None, :], model, alpha, beta, W, V - 1)
    base.check_padding(out[0], out[1], out[2], 0)
    got = hyps4(out, 0)
    labs = [g[0] for g in got]
    assert len(got) == count and set(labs) == set(exact) and len(set(labs)) == count
    assert np.all(out[2][0, count:] == -np.inf) and np.all(out[1][0, count:] == 0)
    worst = 0.0
    for lab, s, c, l in got:
        ws, wc, wl = want[lab]
        worst = max(worst, abs(s - ws) / tol(ws), abs(c - wc) / tol(wc), abs(l - wl) / tol(wl))
        assert abs(s - ws) <= tol(ws) and abs(c - wc) <= tol(wc) and abs(l - wl) <= tol(wl), (lab, s, ws, c, wc, l, wl)
    print("case", case, "worst |score, ctc, lm - exact| / tol", worst)
    pos = {lab: k for k, lab in enumerate(labs)}
    order = sorted(want, key=lambda lab: -want[lab][0])
    for a, b in zip(order, order[1:]):
        if want[a][0] - want[b][0] > 2 * tol(want[b][0]):
            assert pos[a] < pos[b], (a, b)


# ------------------------------------------------------------------------------------------------ 4. full size
def test_full_size_against_restatement(device, fullm):
    """B = 16, T = 1000, V = 3000, beam 16, top_k 16, alpha 0.5, beta 1.0, odd utterances ragged (lmref.full_inputs;
    403,899 n-grams).  The cap on differing N-best sets is a condition on the inputs: the float32-rounded twin
    of the restatement (beam_search_lm(f32=True)) differs from the float64 one in 0 of the 16 utterances on these inputs, the
    worst float32 / float64 score difference is 0.0103 of the tolerance, and all 16 top-1 hypotheses differ from the unfused
    restatement's."""
    x, lengths, model, want = fullm["x"], fullm["lengths"], fullm["model"], fullm["want"]
    out = fused(device, x, model, ALPHA, BETA, W_FULL, K_FULL, 0, lengths)
    base.check_padding(out[0], out[1], out[2], 0)
    gpu = [hyps4(out, b) for b in range(B_FULL)]
    base.compare_nbest([[(g[0], g[1]) for g in hb] for hb in gpu], [[(w[0], w[1]) for w in wb] for wb in want], B_FULL // 8)
    lm_dev = device_lm_scores(device, model, out[0], out[1], True)
    worst = [0.0, 0.0, -np.inf]
    for b in range(B_FULL):
        for i, (lab, s, c, l) in enumerate(gpu[b]):
            f = c + ALPHA * l + BETA * len(lab)
            worst[0] = max(worst[0], abs(s - f) / tol(f))
            assert abs(s - f) <= tol(f), (b, lab, s, f)
            worst[1] = max(worst[1], abs(l - lm_dev[b, i]) / tol(lm_dev[b, i]))
            assert abs(l - lm_dev[b, i]) <= tol(lm_dev[b, i]), (b, lab, l, lm_dev[b, i])
        hb = [g for g in gpu[b] if g[0]]
        ctc = base.gpu_ctc_scores(device, x[:, b], [g[0] for g in hb], lengths[b])
        for (lab, s, c, l), cc in zip(hb, ctc):
            worst[2] = max(worst[2], (c - cc) / tol(cc))
            assert c <= cc + tol(cc), (b, lab, c, cc)
    print("worst |score - formula| / tol %.3g, |lm - ngram_score| / tol %.3g, largest (ctc - log p) / tol %.3g" % tuple(worst))
    plain = base.beam(device, x, W_FULL, K_FULL, 0, lengths)
    changed = sum(1 for b in range(B_FULL) if gpu[b][0][0] != base.hyps(*plain, b)[0][0])
    print("top-1 differs from beam_decode's in %d of %d utterances" % (changed, B_FULL))
    assert changed >= 1


# ------------------------------------------------------------------------------------------------ 5. robustness
def test_padding_is_never_read_launches_repeat_and_empty_utterances(device, fullm):
    x, lengths, model = fullm["x"], fullm["lengths"].copy(), fullm["model"]
    lengths[3] = 0
    a = fused(device, x, model, ALPHA, BETA, W_FULL, K_FULL, 0, lengths)
    a2 = fused(device, x, model, ALPHA, BETA, W_FULL, K_FULL, 0, lengths)
    y = x.copy()
    for b in range(B_FULL):
        y[lengths[b]:, b] = np.nan
    c = fused(device, y, model, ALPHA, BETA, W_FULL, K_FULL, 0, lengths)
    for u, v, w in zip(a, a2, c):
        assert u.tobytes() == v.tobytes() == w.tobytes()
    # no frames: the empty hypothesis alone, its lm the end term only
    end = lmref.step32(model.host_image(), (model.bos,), model.eos)
    assert a[1][3, 0] == 0 and a[3][3, 0] == 0.0 and np.all(a[2][3, 1:] == -np.inf) and np.all(a[0][3] == 0)
    assert a[4][3, 0] == end and abs(a[2][3, 0] - ALPHA * float(end)) <= tol(ALPHA * float(end))
    assert abs(float(end) - fullm["d"].step((model.bos,), model.eos)) <= tol(float(end))


def _raw_call(device, model, T, B, V, W, K, nbytes=None, order=None, slots=None, max_probe=None):
    from asr import _lib
    lib = _lib.lib()
    model.to(device)
    img = model.image
    x = torch.zeros((T, B, V), dtype=torch.float32, device=device)
    need = lib.asr_ctc_beam_lm_workspace_bytes(T, B, V, W, K)
    assert need == lib.asr_ctc_beam_workspace_bytes(T, B, V, W, K)
    nbytes = need if nbytes is None else nbytes(need)
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=device)
    ids = torch.empty((B, W, T), dtype=torch.int32, device=device)
    ln = torch.empty((B, W), dtype=torch.int32, device=device)
    sc, cc, lc = (torch.empty((B, W), dtype=torch.float32, device=device) for _ in range(3))
    rc = lib.asr_ctc_beam_search_lm(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), _lib.ptr(img["uni"]),
                                    img["uni"].shape[0], _lib.ptr(img["keys"]), _lib.ptr(img["vals"]),
                                    img["slots"] if slots is None else slots, img["max_probe"] if max_probe is None else max_probe,
                                    img["order"] if order is None else order, model.bos_id, model.eos_id, 0.5, 1.0, _lib.ptr(ws),
                                    nbytes, _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(cc), _lib.ptr(lc))
    torch.cuda.synchronize()
    return rc


def test_limits_workspace_and_model_arguments(device):
    V = 100
    rs = np.random.RandomState(3)
    model = make_lm(lmref.random_model(rs, V, 3, n_random=500), V)
    for W, K in ((129, 1), (1, 65), (65, 64), (128, 33), (128, 64)):
        assert _raw_call(device, model, 4, 1, V, W, K) == ASR_ERR_UNSUPPORTED, (W, K)
    assert _raw_call(device, model, 4, 1, V, 16, 16, lambda n: n - 1) == ASR_ERR_WORKSPACE
    assert _raw_call(device, model, 4, 1, V, 128, 32) == 0 and _raw_call(device, model, 4, 1, V, 64, 64) == 0
    assert _raw_call(device, model, 4, 1, V, 16, 16, order=5) == ASR_ERR_UNSUPPORTED
    assert _raw_call(device, model, 4, 1, V, 16, 16, slots=12) == ASR_ERR_BAD_ARG
    assert _raw_call(device, model, 4, 1, V, 16, 16, max_probe=0) == ASR_ERR_BAD_ARG
    assert _raw_call(device, model, 4, 1, V, 16, 16) == 0


# ------------------------------------------------------------------------------------------------ 6. error-rate flow
def test_beam_decode_lm_then_sequence_error(device, fullm):
    from asr import error
    x = fullm["x"][:, :4]
    out = fused(device, x, fullm["model"], ALPHA, BETA, W_FULL, K_FULL, 0, fullm["lengths"][:4])
    top1 = [fullm["want"][b][0][0] for b in range(4)]
    t = np.zeros((4, max(len(lab) for lab in top1)), np.int32)
    for b, lab in enumerate(top1):
        t[b, :len(lab)] = lab
    assert error.compute_sequence_error(out[0][:, 0], out[1][:, 0], t, 0, None, None) == 0.0


def test_beam_decode_lm_feeds_sequence_error_on_golden_pairs(device, golden_dir):
    """frames that spell the golden per-frame ids, decoded under a flat unigram model: the top hypothesis is their collapse, and
    its error rate against the golden transcripts is that of compute_minibatch_error on the frames"""
    from asr import error, vocab
    with open(os.path.join(golden_dir, "text.json")) as f:
        g = json.load(f)
    tok, inv = vocab.get_unigram_ids()
    V = max(inv) + 1
    y, t = np.asarray(g["y"]), np.asarray(g["t"])
    B, T = y.shape
    x = np.zeros((T, B, V), np.float32)
    for b in range(B):
        x[np.arange(T), b, y[b]] = 30.0
    model = make_lm({(i,): (-float(np.log(V)), 0.0) for i in range(V + 2)}, V)
    out = fused(device, x, model, 0.3, 0.0, 8, 8)
    want = error.compute_minibatch_error(y, t, 0, tok, inv)
    assert error.compute_sequence_error(out[0][:, 0], out[1][:, 0], t, 0, tok, inv) == want
