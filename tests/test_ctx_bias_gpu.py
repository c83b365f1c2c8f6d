"""Contextual phrase biasing on the GPU (csrc/ctxgraph.hpp, csrc/ctc_beam.hip through asr.bias.ContextGraph and
asr.error.beam_decode_biased) against the restatements of tests/ctx_bias_reference.py, brute-force occurrence counting, the two
parent decoders and the project's own GPU CTC loss.

Tolerance: 1e-4 * max(1, |score|), as in tests/test_ctc_beam_gpu.py and tests/test_ctc_beam_lm_gpu.py (whose helpers this file
uses).
"""
import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref
import ctx_bias_reference as cref
import test_ctc_beam_gpu as base
import test_ctc_beam_lm_gpu as lmbase
from test_ctc_beam_gpu import tol

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.5, 1.0
ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -1, -2, -3
T_P, B_P, V_P, W_P, K_P = 160, 8, 300, 16, 8


def make_graph(phrases, V, weights=None, blank=0):
    from asr import bias
    return bias.ContextGraph(phrases, V, weights, blank=blank)


def biased(device, x, graph, model, alpha, beta, W, K, blank=0, lengths=None, min_logp=None, use_eos=True):
    """x (T, B, V) numpy -> numpy (ids, lens, scores, ctc, lm, bias)"""
    from asr import error
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(device)
    out = error.beam_decode_biased(xt, graph, model, alpha, beta, W, K, blank, lt, min_logp, use_eos)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def hyps5(out, b):
    """the used slots of utterance b: [(labels, score, ctc, lm, bias)] in slot order"""
    ids, lens, scores, ctc, lm, bias = out
    return [(tuple(int(c) for c in ids[b, i, :lens[b, i]]), float(scores[b, i]), float(ctc[b, i]), float(lm[b, i]),
             float(bias[b, i])) for i in range(ids.shape[1]) if scores[b, i] > -np.inf]


# ------------------------------------------------------------------------------------------------ 1. ctx_score
def score_case(name):
    if name == "A":                              # V = 50, 30 phrases with the nested / suffix / overlap cases first
        V, N, L = 50, 64, 40
        rs = np.random.RandomState(61)
        phrases, weights = cref.tricky_phrases(rs, range(1, 12), 30, 4)
    else:                                        # V = 3000, 2000 random phrases of 1-6 tokens: a table with probe chains
        V, N, L = 3000, 64, 40
        rs = np.random.RandomState(62)
        phrases = cref.random_phrases(rs, V, 2000, 1, 6)
        weights = rs.choice([0.5, 1.0, 2.0], size=len(phrases)).tolist()
    seqs = []
    for i in range(N):
        n = 0 if i % 9 == 4 else int(rs.randint(1, L + 1))
        s = []
        while len(s) < n:
            if i % 2 == 0:                       # stitched from phrases
                s += list(phrases[rs.randint(len(phrases))])
            else:
                s.append(int(rs.randint(1, 12 if name == "A" else V)))
        seqs.append(s[:n])
    return V, L, phrases, weights, seqs, rs


@pytest.mark.parametrize("name", ["A", "B"])
def test_ctx_score_bits_sums_and_occurrence_counting(device, name):
    V, L, phrases, weights, seqs, rs = score_case(name)
    N = len(seqs)
    g = make_graph(phrases, V, weights)
    img = g.host_image()
    tw = cref.Image32(img)
    ids = np.zeros((N, L), np.int32)
    lens = np.array([len(s) for s in seqs], np.int32)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = s
        ids[i, len(s):] = rs.randint(1, V, size=L - len(s))          # past the length: never scored
    it, lt = torch.from_numpy(ids).to(device), torch.from_numpy(lens).to(device)
    tok, final = g.score(it, lt, True)
    tok2, opened = g.score(it, lt, False)
    torch.cuda.synchronize()
    tok, final, tok2, opened = tok.cpu().numpy(), final.cpu().numpy(), tok2.cpu().numpy(), opened.cpu().numpy()
    assert tok.tobytes() == tok2.tobytes()
    worst, longest, hits = 0.0, 0, 0
    for i, s in enumerate(seqs):
        want, state = tw.tokens(s)
        want = np.array(want, np.float32).reshape(-1)
        assert np.array_equal(tok[i, :len(s)].view(np.uint32), want.view(np.uint32)), i
        assert np.all(tok[i, len(s):] == 0.0)
        acc = np.float32(0.0)
        for d in want:
            acc = np.float32(acc + d)
        assert opened[i] == acc and final[i] == np.float32(acc + tw.ret(state)), i
        exact = cref.occurrences(s, phrases, weights)
        hits += exact > 0
        worst = max(worst, abs(float(final[i]) - exact) / max(1.0, abs(exact)))
        assert abs(float(final[i]) - exact) <= 1e-4 * max(1.0, abs(exact)), (i, final[i], exact)
        assert opened[i] >= final[i] >= 0.0
        t = 0
        for c in s:
            longest = max(longest, cref.probes_needed(img, t, c), cref.probes_needed(img, 0, c))
            t = tw.step(t, c)[0]
    print("case %s: %d tokens bit-identical, %d sequences with a phrase, longest probe chain walked %d (max_probe %d), "
          "worst |sum - counting| / max(1, |s|) %.3g" % (name, int(lens.sum()), hits, longest, img["max_probe"], worst))
    assert hits >= N // 3 and (name == "A" or longest >= 2)
    # ids outside [0, V): NaN for that token, the rest of the row as if the match started over
    bad = ids.copy()
    r0, r1 = [i for i in range(N) if lens[i] >= 4][:2]
    bad[r0, 1], bad[r1, 0] = V, -1
    tokb, _ = g.score(torch.from_numpy(bad).to(device), lt, True)
    tokb = tokb.cpu().numpy()
    assert np.isnan(tokb[r0, 1]) and np.isnan(tokb[r1, 0]) and np.isnan(tokb).sum() == 2
    rest = np.array(tw.tokens(seqs[r0][2:])[0], np.float32).reshape(-1)
    assert np.array_equal(tokb[r0, 2:lens[r0]].view(np.uint32), rest.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. neutral graph
def check_neutral(device, x, V, W, K, blank, lengths, seed):
    g = make_graph([], V, blank=blank)
    assert g.n_states == 1 and g.host_image()["slots"] == 0
    a = base.beam(device, x, W, K, blank, lengths)
    out = biased(device, x, g, None, 0.0, 0.0, W, K, blank, lengths)
    for u, v in zip(a, out[:3]):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    assert out[3].tobytes() == out[2].tobytes() and np.all(out[4] == 0.0) and np.all(out[5] == 0.0)
    rs = np.random.RandomState(seed)
    ng = lmref.random_model(rs, V, 4, [rs.randint(0, V, size=6).tolist() for _ in range(8)], n_random=300)
    model = lmbase.make_lm(ng, V)
    a = lmbase.fused(device, x, model, ALPHA, BETA, W, K, blank, lengths)
    out = biased(device, x, g, model, ALPHA, BETA, W, K, blank, lengths)
    for u, v in zip(a, out[:5]):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    assert np.all(out[5] == 0.0)
    return out


@pytest.mark.parametrize("T,B,V,W,K,blank,seed", [
    (1, 3, 5, 8, 4, 0, 11), (20, 3, 6, 1, 5, 0, 12), (20, 3, 6, 4, 1, 0, 13), (15, 3, 6, 8, 5, 3, 14), (2, 2, 3, 16, 2, 0, 15),
    (12, 2, 9, 8, 64, 0, 16), (30, 2, 80, 128, 32, 0, 17), (30, 2, 80, 64, 64, 0, 18),
])
def test_neutral_graph_reproduces_both_parents(device, T, B, V, W, K, blank, seed):
    check_neutral(device, base.small(T, B, V, seed), V, W, K, blank, None, seed)


def test_neutral_graph_ragged_batch_with_an_empty_utterance(device):
    x = base.small(24, 4, 12, 21)
    out = check_neutral(device, x, 12, 8, 6, 0, np.array([24, 0, 13, 1], np.int32), 21)
    assert out[1][1, 0] == 0 and out[3][1, 0] == 0.0 and np.all(out[2][1, 1:] == -np.inf)


# ------------------------------------------------------------------------------------------------ 3. exhaustive
@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
@pytest.mark.parametrize("case", ref.EXHAUSTIVE, ids=lambda c: "T%d_V%d_W%d_s%d" % c[0])
def test_exhaustive_biased_objective(device, case, with_lm):
    (T, V, W, seed), count = case
    alpha, beta = (0.7, 0.4) if with_lm else (0.0, 0.0)
    x = ref.exhaustive_logits(T, V, seed)
    rs = np.random.RandomState(200 + seed)
    phrases, weights = cref.tricky_phrases(rs, range(1, V), 3 + seed % 3, 3)
    g = make_graph(phrases, V, weights)
    model = lmbase.make_lm(lmref.exhaustive_model(V, seed), V) if with_lm else None
    d = lmref.DictLM.of(model) if with_lm else None
    exact = ref.enumerate_paths(x)
    want = {}
    for lab in exact:
        l = d.score(lab) if with_lm else 0.0
        bv = cref.occurrences(lab, phrases, weights)
        want[lab] = ((exact[lab] + (alpha * l + beta * len(lab) if with_lm else 0.0)) + bv, exact[lab], l, bv)
    out = biased(device, x[:, None, :], g, model, alpha, beta, W, V - 1)
    base.check_padding(out[0], out[1], out[2], 0)
    got = hyps5(out, 0)
    labs = [h[0] for h in got]
    assert len(got) == count and set(labs) == set(exact) and len(set(labs)) == count
    assert np.all(out[2][0, count:] == -np.inf) and np.all(out[1][0, count:] == 0) and np.all(out[5][0, count:] == 0.0)
    worst = 0.0
    for lab, s, c, l, bv in got:
        ws, wc, wl, wb = want[lab]
        worst = max(worst, abs(s - ws) / tol(ws), abs(c - wc) / tol(wc), abs(l - wl) / tol(wl), abs(bv - wb) / tol(wb))
        assert abs(c - wc) <= tol(wc) and abs(l - wl) <= tol(wl) and abs(bv - wb) <= tol(wb), (lab, c, wc, l, wl, bv, wb)
        assert abs(s - ws) <= tol(ws), (lab, s, ws)
        f = (c + (alpha * l + beta * len(lab))) + bv if with_lm else c + bv
        assert abs(s - f) <= tol(f), (lab, s, f)
    print("case", case, "lm" if with_lm else "plain", "%d of %d labellings biased," % (sum(w[3] > 0 for w in want.values()), count),
          "worst |score, ctc, lm, bias - exact| / tol", worst)
    assert any(w[3] > 0 for w in want.values())
    pos = {lab: k for k, lab in enumerate(labs)}
    order = sorted(want, key=lambda lab: -want[lab][0])
    for a, b in zip(order, order[1:]):
        if want[a][0] - want[b][0] > 2 * tol(want[b][0]):
            assert pos[a] < pos[b], (a, b)


# ------------------------------------------------------------------------------------------------ 4. pruned search
def windows(lab, n):
    return [tuple(lab[i:i + n]) for i in range(len(lab) - n + 1)]


def pruned_inputs():
    """T = 160, B = 8, V = 300 peaky logits, odd utterances ragged, and 400 phrases: the 3-token windows of the unbiased
    restatement's hypotheses ranked 2-6 that its top-1 lacks (weight 1.5), 2-5-token spans of the top-1 and random phrases
    (weights from {0.5, 1, 2}) -> (x, lengths, phrases, weights, the unbiased restatement's lists)"""
    rs = np.random.RandomState(20261020)
    x = np.stack([ref.peaky(rs, T_P, V_P) for _ in range(B_P)], axis=1)
    lengths = np.full(B_P, T_P, np.int32)
    lengths[1::2] = rs.randint(T_P // 2, T_P + 1, size=B_P)[1::2]
    plain = [ref.beam_search(x[:, b], W_P, K_P, 0, int(lengths[b])) for b in range(B_P)]
    table = {}
    for b in range(B_P):
        top = plain[b][0][0]
        have = set(windows(top, 3))
        for lab, _ in plain[b][1:6]:
            for w in windows(lab, 3):
                if w not in have:
                    table.setdefault(w, 1.5)
    for b in range(B_P):
        top = plain[b][0][0]
        for _ in range(8):
            n = int(rs.randint(2, 6))
            i = int(rs.randint(0, max(1, len(top) - n + 1)))
            if len(top[i:i + n]) == n:
                table.setdefault(tuple(top[i:i + n]), float(rs.choice([0.5, 1.0, 2.0])))
    for p in cref.random_phrases(rs, V_P, 400 - len(table), 2, 4, table):
        table[p] = float(rs.choice([0.5, 1.0, 2.0]))
    assert len(table) == 400
    return x, lengths, list(table), list(table.values()), plain


@pytest.fixture(scope="module")
def pruned():
    x, lengths, phrases, weights, plain = pruned_inputs()
    g = make_graph(phrases, V_P, weights)
    tr = [p[0][0] for p in plain]
    model = lmbase.make_lm(lmref.random_model(np.random.RandomState(20261021), V_P, 3, tr, n_random=20000), V_P)
    d, dl = cref.DictGraph(phrases, weights), lmref.DictLM.of(model)
    want = {}
    for name, lm, a, bt in (("plain", None, 0.0, 0.0), ("lm", dl, ALPHA, BETA)):
        want[name] = [cref.beam_search_bias(x[:, b], d, lm, a, bt, W_P, K_P, 0, int(lengths[b])) for b in range(B_P)]
    return dict(x=x, lengths=lengths, phrases=phrases, weights=weights, plain=plain, graph=g, model=model, want=want)


@pytest.mark.parametrize("run", ["plain", "lm"])
def test_pruned_search_against_restatement(device, pruned, run):
    """The cap on differing N-best sets is a condition on the inputs: on pruned_inputs() the float32-rounded twin of the
    restatement (beam_search_bias(f32=True) over the host image) and the float64 one give identical ordered lists in 8 of 8
    utterances in both runs, the worst float32 / float64 score difference is 0.007 (without a model) / 0.16 (with it) of the
    tolerance, and all 8 top-1 hypotheses differ from the unbiased restatement's (checked on the CPU)."""
    x, lengths, g = pruned["x"], pruned["lengths"], pruned["graph"]
    model, alpha, beta = (pruned["model"], ALPHA, BETA) if run == "lm" else (None, 0.0, 0.0)
    want = pruned["want"][run]
    out = biased(device, x, g, model, alpha, beta, W_P, K_P, 0, lengths)
    base.check_padding(out[0], out[1], out[2], 0)
    gpu = [hyps5(out, b) for b in range(B_P)]
    base.compare_nbest([[(h[0], h[1]) for h in hb] for hb in gpu], [[(w[0], w[1]) for w in wb] for wb in want], B_P // 8)
    B, W, T = out[0].shape
    _, dev_bias = g.score(torch.from_numpy(np.ascontiguousarray(out[0].reshape(B * W, T))).to(device),
                          torch.from_numpy(np.ascontiguousarray(out[1].reshape(B * W))).to(device), True)
    dev_bias = dev_bias.double().cpu().numpy().reshape(B, W)
    worst = [0.0, 0.0, -np.inf]
    for b in range(B_P):
        for i, (lab, s, c, l, bv) in enumerate(gpu[b]):
            f = (c + (alpha * l + beta * len(lab))) + bv if run == "lm" else c + bv
            worst[0] = max(worst[0], abs(s - f) / tol(f))
            assert abs(s - f) <= tol(f), (b, lab, s, f)
            worst[1] = max(worst[1], abs(bv - dev_bias[b, i]) / tol(dev_bias[b, i]))
            assert abs(bv - dev_bias[b, i]) <= tol(dev_bias[b, i]), (b, lab, bv, dev_bias[b, i])
            exact = cref.occurrences(lab, pruned["phrases"], pruned["weights"])
            assert abs(bv - exact) <= tol(exact), (b, lab, bv, exact)
        hb = [h for h in gpu[b] if h[0]]
        ctc = base.gpu_ctc_scores(device, x[:, b], [h[0] for h in hb], lengths[b])
        for h, cc in zip(hb, ctc):
            worst[2] = max(worst[2], (h[2] - cc) / tol(cc))
            assert h[2] <= cc + tol(cc), (b, h[0], h[2], cc)
    print("worst |score - formula| / tol %.3g, |bias - ctx_score| / tol %.3g, largest (ctc - log p) / tol %.3g" % tuple(worst))
    changed = sum(1 for b in range(B_P) if gpu[b][0][0] != pruned["plain"][b][0][0])
    print("top-1 differs from the unbiased search's in %d of %d utterances" % (changed, B_P))
    assert changed >= 1


# ------------------------------------------------------------------------------------------------ 5. largest shapes
@pytest.mark.parametrize("T,B,V,W,K,seed", [(30, 2, 80, 128, 32, 17), (30, 2, 80, 64, 64, 18)])
def test_largest_shapes_with_model_and_graph(device, T, B, V, W, K, seed):
    """more than one look-up per thread (up to 4096 extensions on 256 threads) and the full LDS footprint, under the edge-case
    conditions of tests/test_ctc_beam_gpu.py"""
    x = base.small(T, B, V, seed)
    rs = np.random.RandomState(seed)
    ng = lmref.random_model(rs, V, 4, [rs.randint(0, V, size=6).tolist() for _ in range(8)], n_random=300)
    model = lmbase.make_lm(ng, V)
    phrases = cref.random_phrases(rs, V, 60, 1, 3)
    weights = rs.choice([0.5, 1.0, 2.0], size=len(phrases)).tolist()
    g = make_graph(phrases, V, weights)
    d, dl = cref.DictGraph(phrases, weights), lmref.DictLM.of(model)
    out = biased(device, x, g, model, ALPHA, BETA, W, K)
    base.check_padding(out[0], out[1], out[2], 0)
    for b in range(B):
        want = [(w[0], w[1]) for w in cref.beam_search_bias(x[:, b], d, dl, ALPHA, BETA, W, K)]
        got = [(h[0], h[1]) for h in hyps5(out, b)]
        assert len(got) == len(want), b
        for (_, gs_), (_, ws_) in zip(got, want):
            assert abs(gs_ - ws_) <= tol(ws_), (b, gs_, ws_)
        gs, ws = dict(got), dict(want)
        for lab in set(gs) & set(ws):
            assert abs(gs[lab] - ws[lab]) <= tol(ws[lab]), (b, lab)
        for lab in set(gs) - set(ws):
            assert gs[lab] <= want[-1][1] + tol(want[-1][1]), (b, lab)
        for lab in set(ws) - set(gs):
            assert ws[lab] <= got[-1][1] + tol(got[-1][1]), (b, lab)
        biased_n = sum(1 for h in hyps5(out, b) if h[4] > 0)
        print("T%d V%d W%d K%d utterance %d: %d hypotheses, %d with a phrase, %d on one side only"
              % (T, V, W, K, b, len(got), biased_n, len(set(gs) ^ set(ws))))
        assert biased_n >= 1


# ------------------------------------------------------------------------------------------------ 6. robustness
def test_launches_repeat_padding_is_never_read_and_empty_utterances(device, pruned):
    x, lengths, g, model = pruned["x"], pruned["lengths"].copy(), pruned["graph"], pruned["model"]
    lengths[3] = 0
    a = biased(device, x, g, model, ALPHA, BETA, W_P, K_P, 0, lengths)
    a2 = biased(device, x, g, model, ALPHA, BETA, W_P, K_P, 0, lengths)
    y = x.copy()
    for b in range(B_P):
        y[lengths[b]:, b] = np.nan
    c = biased(device, y, g, model, ALPHA, BETA, W_P, K_P, 0, lengths)
    for u, v, w in zip(a, a2, c):
        assert u.tobytes() == v.tobytes() == w.tobytes()
    assert a[1][3, 0] == 0 and a[3][3, 0] == 0.0 and a[5][3, 0] == 0.0 and np.all(a[2][3, 1:] == -np.inf) and np.all(a[0][3] == 0)
    assert np.all(a[5][3] == 0.0)
    p = biased(device, x, g, None, 0.0, 0.0, W_P, K_P, 0, lengths)
    assert p[1][3, 0] == 0 and p[2][3, 0] == 0.0 and p[5][3, 0] == 0.0 and np.all(p[4] == 0.0)


def _raw_call(device, graph, T, B, V, W, K, nbytes=None, model=None, n_states=None, slots=None, max_probe=None, ret=True,
              vals=None, x=None):
    from asr import _lib, _ops
    lib = _lib.lib()
    graph.to(device)
    img = graph.image
    x = torch.zeros((T, B, V), dtype=torch.float32, device=device) if x is None else x
    need = lib.asr_ctc_beam_bias_workspace_bytes(T, B, V, W, K)
    assert need == lib.asr_ctc_beam_workspace_bytes(T, B, V, W, K)
    nbytes = need if nbytes is None else nbytes(need)
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=device)
    ids = torch.full((B, W, T), -7, dtype=torch.int32, device=device)
    ln = torch.empty((B, W), dtype=torch.int32, device=device)
    sc, cc, lc, bc = (torch.empty((B, W), dtype=torch.float32, device=device) for _ in range(4))
    if model is None:
        lm_args, bos, eos = (None, 0, None, None, 0, 0, 0), -1, -1
    else:
        model.to(device)
        lm_args, bos, eos = _ops._lm_args(model.image), model.bos_id, model.eos_id
    rc = lib.asr_ctc_beam_search_bias(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), *lm_args, bos, eos, 0.5,
                                      1.0, _lib.ptr(ws), nbytes, _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(cc),
                                      _lib.ptr(lc), _lib.ptr(img["keys"]), _lib.ptr(img["vals"] if vals is None else vals),
                                      img["slots"] if slots is None else slots,
                                      img["max_probe"] if max_probe is None else max_probe, _lib.ptr(img["ret"]) if ret else None,
                                      img["n_states"] if n_states is None else n_states, _lib.ptr(bc))
    torch.cuda.synchronize()
    return rc, ids.cpu().numpy(), ln.cpu().numpy()


def test_limits_workspace_and_graph_arguments(device):
    V = 100
    rs = np.random.RandomState(3)
    g = make_graph(cref.random_phrases(rs, V, 50, 1, 4), V)
    model = lmbase.make_lm(lmref.random_model(rs, V, 3, n_random=500), V)
    for m in (None, model):
        for W, K in ((129, 1), (1, 65), (65, 64), (128, 33), (128, 64)):
            assert _raw_call(device, g, 4, 1, V, W, K, model=m)[0] == ASR_ERR_UNSUPPORTED, (W, K)
        assert _raw_call(device, g, 4, 1, V, 16, 16, lambda n: n - 1, model=m)[0] == ASR_ERR_WORKSPACE
        assert _raw_call(device, g, 4, 1, V, 128, 32, model=m)[0] == 0 and _raw_call(device, g, 4, 1, V, 64, 64, model=m)[0] == 0
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, n_states=0)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, ret=False)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, slots=12)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, max_probe=0)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m)[0] == 0


def test_a_table_with_damaged_next_fields_stays_in_range(device, pruned):
    """every `next` of the table overwritten on the host with out-of-range values: the call returns 0, reads nothing out of
    range (such a `next` counts as the root) and every id it writes is a token id"""
    g = pruned["graph"]
    vals = g.host_image()["vals"].copy()
    vals[:, 0] = np.where(np.arange(len(vals)) % 2 == 0, 0x7fffffff, -5)
    x = torch.from_numpy(np.ascontiguousarray(pruned["x"][:40])).to(device)
    rc, ids, ln = _raw_call(device, g, 40, B_P, V_P, W_P, K_P, vals=torch.from_numpy(vals).to(device), x=x)
    assert rc == 0 and ids.min() >= 0 and ids.max() < V_P and ln.min() >= 0 and ln.max() <= 40
