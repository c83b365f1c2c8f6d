"""CTC prefix beam search on the GPU (csrc/ctc_beam.hip through asr.error.beam_decode) against an exhaustive enumeration of
every path, the project's own GPU CTC loss, and the float64 restatement of tests/ctc_beam_reference.py.

Tolerance: 1e-4 * max(1, |score|), the project's CTC loss tolerance (tests/test_ctc_gpu.py, from BASELINE.json): a beam score is
a CTC log-probability.
"""
import numpy as np
import pytest
import torch

import ctc_beam_reference as ref
from ctc_beam_reference import EXHAUSTIVE, exhaustive_logits

pytestmark = pytest.mark.gpu

RTOL = 1e-4
T_FULL, B_FULL, V_FULL, W_FULL, K_FULL = 1000, 16, 3000, 16, 16
ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -2, -3


def tol(s):
    return RTOL * max(1.0, abs(s))


def beam(device, x, W, K, blank=0, lengths=None, min_logp=None):
    """x (T, B, V) f32 numpy -> numpy (ids (B, W, T), lens (B, W), scores (B, W))"""
    from asr import error
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(device)
    ids, lens, scores = error.beam_decode(xt, W, K, blank, lt, min_logp)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy()


def hyps(ids, lens, scores, b):
    """the used slots of utterance b: [(labels tuple, score)] in slot order"""
    return [(tuple(int(c) for c in ids[b, i, :lens[b, i]]), float(scores[b, i])) for i in range(ids.shape[1])
            if scores[b, i] > -np.inf]


def check_padding(ids, lens, scores, blank):
    B, W, T = ids.shape
    for b in range(B):
        for i in range(W):
            assert np.all(ids[b, i, lens[b, i]:] == blank)
            if scores[b, i] == -np.inf:
                assert lens[b, i] == 0
        used = scores[b] > -np.inf
        assert np.all(used[:used.sum()])                  # used slots first
        assert np.all(np.diff(scores[b][used]) <= 0)      # best first


def gpu_ctc_scores(device, x, labellings, length=None):
    """-(the project's GPU CTC loss) of every labelling (non-empty) over one utterance's logits x (T, V), as one batch"""
    from asr.loss import connectionist_temporal_classification
    n = len(labellings)
    L = max(len(lab) for lab in labellings)
    labels = np.zeros((n, L), np.int32)
    for i, lab in enumerate(labellings):
        labels[i, :len(lab)] = lab
    xs = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)[:, None, :].expand(-1, n, -1).contiguous()
    xl = None if length is None else torch.full((n,), int(length), dtype=torch.int32, device=device)
    ll = torch.tensor([len(lab) for lab in labellings], dtype=torch.int32, device=device)
    with torch.no_grad():
        loss = connectionist_temporal_classification(xs, torch.from_numpy(labels).to(device), 0, xl, ll, "no")
    return -loss.double().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. exhaustive
@pytest.mark.parametrize("case", EXHAUSTIVE, ids=lambda c: "T%d_V%d_W%d_s%d" % c[0])
def test_exhaustive_against_enumeration_and_ctc_loss(device, case):
    (T, V, W, seed), count = case
    x = exhaustive_logits(T, V, seed)
    exact = ref.enumerate_paths(x)
    assert len(exact) == count
    ids, lens, scores = beam(device, x[:, None, :], W, V - 1)
    check_padding(ids, lens, scores, 0)
    got = hyps(ids, lens, scores, 0)
    labs = [lab for lab, _ in got]
    s = np.array([sc for _, sc in got])
    print("case", case, "returned", len(got), "worst |score - exact| / tol",
          max(abs(sc - exact[lab]) / tol(exact[lab]) for lab, sc in got))
    assert len(got) == count and len(set(labs)) == count and set(labs) == set(exact)
    assert np.all(np.isfinite(s))
    assert np.all(scores[0, count:] == -np.inf) and np.all(lens[0, count:] == 0)
    for lab, sc in got:
        assert abs(sc - exact[lab]) <= tol(exact[lab]), (lab, sc, exact[lab])
    nonempty = [lab for lab in labs if lab]
    ctc = gpu_ctc_scores(device, x, nonempty)
    for lab, c in zip(nonempty, ctc):
        sc = s[labs.index(lab)]
        assert abs(sc - c) <= tol(c), (lab, sc, c)
    assert np.all(np.diff(s) <= 0)
    order = sorted(exact, key=lambda lab: -exact[lab])
    pos = {lab: k for k, lab in enumerate(labs)}
    for a, b in zip(order, order[1:]):
        if exact[a] - exact[b] > 2 * tol(exact[b]):
            assert pos[a] < pos[b], (a, b, exact[a], exact[b])


# ------------------------------------------------------------------------------------------------ 2. full size
def full_inputs():
    rs = np.random.RandomState(20261016)
    x = np.stack([ref.peaky(rs, T_FULL, V_FULL) for _ in range(B_FULL)], axis=1)
    lengths = np.random.RandomState(1016).randint(T_FULL // 2, T_FULL + 1, size=B_FULL).astype(np.int32)
    return x, lengths


@pytest.fixture(scope="module")
def full():
    """the inputs of test 2, the GPU N-best of the full and the ragged run, and the restatement's (computed once)"""
    x, lengths = full_inputs()
    out = {"x": x, "lengths": lengths}
    for name, ln in (("full", None), ("ragged", lengths)):
        out[name] = [ref.beam_search(x[:, b], W_FULL, K_FULL, 0, None if ln is None else ln[b]) for b in range(B_FULL)]
    return out


def compare_nbest(gpu, want, cap):
    """the test-2 conditions: equal N-best sets in all but `cap` utterances, matching scores for every hypothesis in both
    lists, and any GPU hypothesis missing from the restatement's list scores at most its last kept score (+ tolerance)"""
    differ = 0
    for b, (g, w) in enumerate(zip(gpu, want)):
        gs, ws = dict(g), dict(w)
        worst = max([abs(gs[lab] - ws[lab]) / tol(ws[lab]) for lab in gs if lab in ws] + [0.0])
        print("utterance %d: %d / %d in both, top-1 %s, worst |score diff| / tol %.3g"
              % (b, len(set(gs) & set(ws)), len(ws), g[0][0] == w[0][0], worst))
        for lab in set(gs) & set(ws):
            assert abs(gs[lab] - ws[lab]) <= tol(ws[lab]), (b, lab, gs[lab], ws[lab])
        if set(gs) != set(ws):
            differ += 1
            last = w[-1][1]
            for lab in set(gs) - set(ws):
                assert gs[lab] <= last + tol(last), (b, lab, gs[lab], last)
    print("utterances whose N-best sets differ: %d (at most %d)" % (differ, cap))
    assert differ <= cap


@pytest.mark.parametrize("run", ["full", "ragged"])
def test_full_size_against_restatement(device, full, run):
    x, lengths = full["x"], full["lengths"]
    ids, lens, scores = beam(device, x, W_FULL, K_FULL, 0, None if run == "full" else lengths)
    check_padding(ids, lens, scores, 0)
    gpu = [hyps(ids, lens, scores, b) for b in range(B_FULL)]
    compare_nbest(gpu, full[run], B_FULL // 8)


# ------------------------------------------------------------------------------------------------ 3. lower bound
@pytest.mark.parametrize("run", ["full", "ragged"])
def test_scores_are_lower_bounds_of_the_ctc_loss(device, full, run):
    x, lengths = full["x"], full["lengths"]
    ln = None if run == "full" else lengths
    ids, lens, scores = beam(device, x, W_FULL, K_FULL, 0, ln)
    worst = -np.inf
    for b in range(B_FULL):
        hb = [(lab, sc) for lab, sc in hyps(ids, lens, scores, b) if lab]
        ctc = gpu_ctc_scores(device, x[:, b], [lab for lab, _ in hb], None if ln is None else ln[b])
        for (lab, sc), c in zip(hb, ctc):
            worst = max(worst, (sc - c) / tol(c))
            assert sc <= c + tol(c), (b, lab, sc, c)
    print("largest (score - log p) / tol:", worst)


# ------------------------------------------------------------------------------------------------ 4. ragged, padding, repeat
def test_padding_frames_are_never_read_and_launches_repeat_bitwise(device):
    x, lengths = full_inputs()
    a = beam(device, x, W_FULL, K_FULL, 0, lengths)
    a2 = beam(device, x, W_FULL, K_FULL, 0, lengths)
    rs = np.random.RandomState(7)
    y = x.copy()
    for b in range(B_FULL):
        y[lengths[b]:, b] = (rs.randn(T_FULL - lengths[b], V_FULL) * 20).astype(np.float32)
    c = beam(device, y, W_FULL, K_FULL, 0, lengths)
    for u, v, w in zip(a, a2, c):
        assert np.array_equal(u, v) and np.array_equal(u, w)
        assert u.tobytes() == v.tobytes() == w.tobytes()


# ------------------------------------------------------------------------------------------------ 5. min_logp
def test_min_logp_against_restatement(device, full):
    thr = float(np.log(1e-3))
    x = full["x"][:, :8]
    for b in range(x.shape[1]):
        lp, cands = ref.candidates(x[:, b], 0, K_FULL)
        near = min(np.min(np.abs(lp[t, c] - thr)) for t, c in enumerate(cands) if c)
        assert near > 1e-5, ("a candidate's lp lies within 1e-5 of the threshold: the inputs do not separate it", b, near)
    ids, lens, scores = beam(device, x, W_FULL, K_FULL, 0, None, thr)
    check_padding(ids, lens, scores, 0)
    want = [ref.beam_search(x[:, b], W_FULL, K_FULL, 0, None, thr) for b in range(x.shape[1])]
    compare_nbest([hyps(ids, lens, scores, b) for b in range(x.shape[1])], want, x.shape[1] // 8)


# ------------------------------------------------------------------------------------------------ 6. edge cases
def small(T, B, V, seed, scale=2.0):
    return (np.random.RandomState(seed).randn(T, B, V) * scale).astype(np.float32)


@pytest.mark.parametrize("T,B,V,W,K,blank,seed", [
    (1, 3, 5, 8, 4, 0, 11),          # T = 1
    (20, 3, 6, 1, 5, 0, 12),         # beam_width = 1
    (20, 3, 6, 4, 1, 0, 13),         # top_k = 1
    (15, 3, 6, 8, 5, 3, 14),         # blank id other than 0
    (2, 2, 3, 16, 2, 0, 15),         # fewer feasible prefixes (5) than slots
    (12, 2, 9, 8, 64, 0, 16),        # top_k above V - 1
    (30, 2, 80, 128, 32, 0, 17),     # the largest accepted shapes
    (30, 2, 80, 64, 64, 0, 18),
    (30, 2, 80, 128, 1, 0, 19),
    (30, 2, 80, 1, 64, 0, 20),
])
def test_edge_cases_against_restatement(device, T, B, V, W, K, blank, seed):
    x = small(T, B, V, seed)
    ids, lens, scores = beam(device, x, W, K, blank)
    check_padding(ids, lens, scores, blank)
    for b in range(B):
        want = ref.beam_search(x[:, b], W, K, blank)
        got = hyps(ids, lens, scores, b)
        assert len(got) == len(want), b
        # slot by slot the scores agree; a labelling kept by one side only sits at the other's cut within the tolerance
        # (an f32 / float64 near-tie at the beam boundary), and every labelling on both sides has the same score
        for (_, g), (_, w) in zip(got, want):
            assert abs(g - w) <= tol(w), (b, g, w)
        gs, ws = dict(got), dict(want)
        for lab in set(gs) & set(ws):
            assert abs(gs[lab] - ws[lab]) <= tol(ws[lab]), (b, lab)
        for lab in set(gs) - set(ws):
            assert gs[lab] <= want[-1][1] + tol(want[-1][1]), (b, lab)
        for lab in set(ws) - set(gs):
            assert ws[lab] <= got[-1][1] + tol(got[-1][1]), (b, lab)
        print("T%d B%d V%d W%d K%d blank %d utterance %d: %d hypotheses, %d on one side only"
              % (T, B, V, W, K, blank, b, len(got), len(set(gs) ^ set(ws))))
        if T == 2 and V == 3:
            assert len(got) == 5 and np.all(scores[b, 5:] == -np.inf) and np.all(lens[b, 5:] == 0)
            assert np.all(ids[b, 5:] == blank)


def _raw_call(device, T, B, V, W, K, nbytes=None):
    from asr import _lib
    lib = _lib.lib()
    x = torch.zeros((T, B, V), dtype=torch.float32, device=device)
    need = lib.asr_ctc_beam_workspace_bytes(T, B, V, W, K)
    nbytes = need if nbytes is None else nbytes(need)
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=device)
    ids = torch.empty((B, W, T), dtype=torch.int32, device=device)
    ln = torch.empty((B, W), dtype=torch.int32, device=device)
    sc = torch.empty((B, W), dtype=torch.float32, device=device)
    rc = lib.asr_ctc_beam_search(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), _lib.ptr(ws), nbytes,
                                 _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc))
    torch.cuda.synchronize()
    return rc


def test_limits_and_workspace(device):
    for W, K in ((129, 1), (1, 65), (65, 64), (128, 33), (128, 64)):
        assert _raw_call(device, 4, 1, 100, W, K) == ASR_ERR_UNSUPPORTED, (W, K)
    assert _raw_call(device, 4, 1, 100, 16, 16, lambda n: n - 1) == ASR_ERR_WORKSPACE
    assert _raw_call(device, 4, 1, 100, 128, 32) == 0 and _raw_call(device, 4, 1, 100, 64, 64) == 0


# ------------------------------------------------------------------------------------------------ 7. Python layer
def test_beam_decode_then_sequence_error(device, full):
    from asr import error
    x = full["x"][:, :4]
    ids, lens, _ = beam(device, x, W_FULL, K_FULL)
    top1 = [full["full"][b][0][0] for b in range(4)]
    t = np.zeros((4, max(len(lab) for lab in top1)), np.int32)
    for b, lab in enumerate(top1):
        t[b, :len(lab)] = lab
    assert error.compute_sequence_error(ids[:, 0], lens[:, 0], t, 0, None, None) == 0.0


def test_sequence_error_equals_minibatch_error_on_golden_pairs(device, golden_dir):
    import json
    import os
    from asr import error, vocab
    with open(os.path.join(golden_dir, "text.json")) as f:
        g = json.load(f)
    tok, inv = vocab.get_unigram_ids()
    y, t = np.asarray(g["y"]), np.asarray(g["t"])
    pred = np.zeros_like(y)
    plen = np.zeros(len(y), np.int32)
    for b in range(len(y)):                      # collapsed on the host: blanks and repeats dropped
        prev, row = 0, []
        for c in y[b]:
            if c != 0 and c != prev:
                row.append(int(c))
            prev = c
        pred[b, :len(row)] = row
        plen[b] = len(row)
    assert error.compute_sequence_error(pred, plen, t, 0, tok, inv) == error.compute_minibatch_error(y, t, 0, tok, inv)
    for b in range(len(y)):
        assert error.compute_sequence_error(pred[b:b + 1], plen[b:b + 1], t[b:b + 1], 0, tok, inv) == \
            error.compute_minibatch_error(y[b:b + 1], t[b:b + 1], 0, tok, inv)
