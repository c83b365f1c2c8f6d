"""Gram-CTC beam search with contextual phrase biasing on the GPU (asr_gram_ctc_beam_search_bias and
asr_gram_ctc_beam_bias_stream_* of csrc/ctc_beam.hip through asr.error.gram_beam_decode_biased and GramBeamStream(graph=...))
against the float64 restatement of tests/gram_ctx_bias_reference.py, an exhaustive enumeration of every path with brute-force
occurrence counting, the two parent string searches, the token-level biased search and asr_ctx_score.

Tolerance: 1e-4 * max(1, |score|), `tol` of tests/test_ctc_beam_gpu.py (whose helpers, and those of the Gram-CTC, language-model,
biasing and streaming GPU tests, this file uses).  Comparisons with the parents and between launches are on bytes.
"""
import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref
import ctx_bias_reference as cref
import gram_beam_reference as gref
import gram_ctx_bias_reference as gcb
import test_ctc_beam_gpu as base
import test_ctx_bias_gpu as bbase
from test_ctc_beam_gpu import check_padding, compare_nbest, tol
from test_ctc_beam_stream_gpu import cuttings, feed, fetch, same
from test_ctx_bias_gpu import hyps5, make_graph
from test_gram_beam_gpu import gbeam
from test_gram_beam_lm_gpu import edge_model, gfused, make_lm

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.5, 1.0
ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -1, -2, -3
SEED_P = 20261101                      # tests/test_gram_ctx_bias_cpu.py asserts what the cap of 0 rests on
T_P, B_P, V_P, W_P, K_P = gcb.T_P, gcb.B_P, gcb.V_P, gcb.W_P, gcb.K_P
VARIANTS = ["plain", "lm"]


def gbiased(device, x, gram, graph, model, alpha, beta, W, K, blank=0, lengths=None, min_logp=None, use_eos=True):
    """x (T, B, V) numpy -> numpy (ids (B, W, 2T), lens, scores, ctc, lm, bias)"""
    from asr import error
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(device)
    out = error.gram_beam_decode_biased(xt, gram, graph, model, alpha, beta, W, K, blank, lt, min_logp, use_eos)
    torch.cuda.synchronize()
    assert out[0].shape == (x.shape[1], W, 2 * x.shape[0])
    return tuple(o.cpu().numpy() for o in out)


def unused_slots_are_empty(out):
    unused = out[2] == -np.inf
    assert np.all(out[3][unused] == -np.inf) and np.all(out[4][unused] == 0.0) and np.all(out[5][unused] == 0.0)
    assert np.all(out[1][unused] == 0)
    assert np.all(np.isfinite(out[3][~unused])) and np.all(np.isfinite(out[4][~unused])) and np.all(np.isfinite(out[5][~unused]))


def char_phrases(rs, chars, count, min_len=1, max_len=3):
    """`count` different random phrases over the characters `chars`, weights from {0.5, 1, 2}"""
    chars = list(chars)
    count = min(count, sum(len(chars) ** n for n in range(min_len, max_len + 1)) // 2)
    seen = []
    while len(seen) < count:
        p = tuple(int(chars[i]) for i in rs.randint(0, len(chars), size=rs.randint(min_len, max_len + 1)))
        if p not in seen:
            seen.append(p)
    return seen, rs.choice([0.5, 1.0, 2.0], size=len(seen)).tolist()


def chars_of(gram):
    return sorted({int(c) for c in np.asarray(gram).reshape(-1) if c >= 0})


# ------------------------------------------------------------------------------------------------ 1. neutral graph
def check_neutral(device, x, gram, model, W, K, blank, lengths):
    V = x.shape[2]
    g = make_graph([], V, blank=blank)
    assert g.n_states == 1 and g.host_image()["slots"] == 0
    a = gbeam(device, x, gram, W, K, blank, lengths)
    out = gbiased(device, x, gram, g, None, 0.0, 0.0, W, K, blank, lengths)
    for u, v in zip(a, out[:3]):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    assert out[3].tobytes() == out[2].tobytes() and np.all(out[4] == 0.0) and np.all(out[5] == 0.0)
    for alpha, beta in ((0.7, 0.4), (ALPHA, BETA)):         # weights whose products round, and the exact ones
        a = gfused(device, x, gram, model, alpha, beta, W, K, blank, lengths)
        out = gbiased(device, x, gram, g, model, alpha, beta, W, K, blank, lengths)
        for u, v in zip(a, out[:5]):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
        assert np.all(out[5] == 0.0)
    return out


@pytest.mark.parametrize("T,B,V,U,W,K,blank,seed", [
    (1, 3, 8, 3, 8, 4, 0, 11), (20, 3, 9, 3, 1, 5, 0, 12), (20, 3, 9, 3, 4, 1, 0, 13), (15, 3, 9, 3, 8, 5, 3, 14),
    (12, 2, 9, 3, 8, 64, 0, 16), (30, 2, 80, 10, 128, 32, 0, 17), (30, 2, 80, 10, 64, 64, 0, 18), (30, 2, 80, 10, 128, 1, 0, 19),
    (30, 2, 80, 10, 1, 64, 0, 20),
])
def test_neutral_graph_reproduces_both_parents_on_the_edge_shapes(device, T, B, V, U, W, K, blank, seed):
    check_neutral(device, base.small(T, B, V, seed), gref.random_table(V, U, seed, blank), edge_model(V, 4, seed), W, K, blank, None)


def test_neutral_graph_ragged_batch_with_a_frameless_utterance(device):
    out = check_neutral(device, base.small(24, 4, 12, 21), gref.random_table(12, 4, 21), edge_model(12, 3, 21), 8, 6, 0,
                        np.array([24, 0, 13, 1], np.int32))
    assert out[1][1, 0] == 0 and out[3][1, 0] == 0.0 and np.all(out[2][1, 1:] == -np.inf) and np.all(out[0][1] == 0)


# ------------------------------------------------------------------------------------------------ 2. bigram-free table
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_bigram_free_table_gives_beam_decode_biased(device, variant):
    """unigram ids = token ids, no bigram row: the first T id columns, the lengths and the four scores are the token-level biased
    search's, bit for bit"""
    T, B, V, W, K = 60, 4, 40, 16, 8
    rs = np.random.RandomState(51)
    x = np.stack([ref.peaky(rs, T, V) for _ in range(B)], axis=1)
    gram = np.full((V, 2), -1, np.int32)
    gram[1:, 0] = np.arange(1, V)
    tr = [lmref.greedy(x[:, b]) for b in range(B)]
    phrases, weights = cref.tricky_phrases(rs, range(1, V), 40, 4)
    for t in tr:
        for w in gcb.windows(t, 3)[::3]:
            if w not in phrases:
                phrases.append(w)
                weights.append(1.5)
    g = make_graph(phrases, V, weights)
    model = make_lm(lmref.random_model(rs, V, 3, tr, n_random=3000), V) if variant == "lm" else None
    a, bt = (ALPHA, BETA) if variant == "lm" else (0.0, 0.0)
    for ln in (None, np.array([60, 0, 31, 45], np.int32)):
        got = gbiased(device, x, gram, g, model, a, bt, W, K, 0, ln)
        want = bbase.biased(device, x, g, model, a, bt, W, K, 0, ln)
        assert np.array_equal(got[0][..., :T], want[0]) and np.all(got[0][..., T:] == 0)
        for u, v in zip(got[1:], want[1:]):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
        assert np.any(got[5] > 0)


# ------------------------------------------------------------------------------------------------ 3. exhaustive
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", gref.EXHAUSTIVE, ids=lambda c: "T%d_rows%d_s%d" % (c[0][0], len(c[0][1]), c[0][2]))
def test_exhaustive_biased_objective(device, case, variant):
    """the beam holds every string: each appears once, ctc is the enumeration's log-probability, bias is the brute-force count
    (exactly: the weights are multiples of 0.5) however the string was cut into tokens, merged or re-created, and lm and score are
    the float64 values.  The phrase sets are gram_ctx_bias_reference.exhaustive_phrases (tests/test_gram_ctx_bias_cpu.py asserts
    that they hold the cases of the bigram step)."""
    (T, rows, seed), count = case
    with_lm = variant == "lm"
    alpha, beta = (0.7, 0.4) if with_lm else (0.0, 0.0)
    gram = gref.table(rows)
    V = len(gram)
    x = gref.exhaustive_logits(T, V, seed)
    phrases, weights = gcb.exhaustive_phrases(rows, seed)
    g = make_graph(phrases, V, weights)
    import gram_beam_lm_reference as glm
    model = make_lm(glm.relabel_marks(lmref.exhaustive_model(3, seed), 3, V), V) if with_lm else None
    d = lmref.DictLM.of(model) if with_lm else None
    exact = gref.enumerate_strings(x, gram)
    assert len(exact) == count
    out = gbiased(device, x[:, None, :], gram, g, model, alpha, beta, 128, V - 1)
    check_padding(out[0], out[1], out[2], 0)
    unused_slots_are_empty(out)
    got = hyps5(out, 0)
    strings = [h[0] for h in got]
    assert len(got) == count and len(set(strings)) == count and set(strings) == set(exact)
    assert np.all(out[2][0, count:] == -np.inf) and np.all(out[1][0, count:] == 0) and np.all(out[5][0, count:] == 0.0)
    want, worst = {}, 0.0
    for s, sc, c, l, bv in got:
        wl = d.score(s) if with_lm else 0.0
        wb = cref.occurrences(s, phrases, weights)
        ws = (exact[s] + (alpha * wl + beta * len(s) if with_lm else 0.0)) + wb
        want[s] = ws
        print(s, sc, ws, c, exact[s], l, wl, bv, wb)
        worst = max(worst, abs(sc - ws) / tol(ws), abs(c - exact[s]) / tol(exact[s]), abs(l - wl) / tol(wl))
        assert bv == wb, (s, bv, wb)
        assert abs(c - exact[s]) <= tol(exact[s]) and abs(l - wl) <= tol(wl), (s, c, exact[s], l, wl)
        assert abs(sc - ws) <= tol(ws), (s, sc, ws)
    print("case", case, variant, "%d of %d strings biased," % (sum(h[4] > 0 for h in got), count), "worst |score, ctc, lm - exact| / tol",
          worst)
    assert any(h[4] > 0 for h in got)
    pos = {s: k for k, s in enumerate(strings)}
    order = sorted(want, key=lambda s: -want[s])
    for a, b in zip(order, order[1:]):
        if want[a] - want[b] > 2 * tol(want[b]):
            assert pos[a] < pos[b], (a, b)


# ------------------------------------------------------------------------------------------------ 4. pruned search
@pytest.fixture(scope="module")
def pruned():
    """gram_ctx_bias_reference.pruned_inputs(SEED_P), the graph, the trigram character model, and the float64 restatement's N-best
    without and with the model (computed once)"""
    gram, x, lengths, phrases, weights, plain = gcb.pruned_inputs(SEED_P)
    g = make_graph(phrases, V_P, weights)
    model = make_lm(gcb.pruned_ngrams(plain, SEED_P + 1), V_P)
    d, dl = cref.DictGraph(phrases, weights), lmref.DictLM.of(model)
    want = {}
    for name, lm, a, bt in (("plain", None, 0.0, 0.0), ("lm", dl, ALPHA, BETA)):
        want[name] = [gcb.beam_search_bias(x[:, b], gram, d, lm, a, bt, W_P, K_P, 0, int(lengths[b])) for b in range(B_P)]
    return dict(gram=gram, x=x, lengths=lengths, phrases=phrases, weights=weights, plain=plain, graph=g, model=model, want=want)


def run_args(pruned, variant):
    return (pruned["model"], ALPHA, BETA) if variant == "lm" else (None, 0.0, 0.0)


@pytest.fixture(scope="module")
def decoded(device, pruned):
    """the GPU N-best of both variants (one launch each)"""
    return {v: gbiased(device, pruned["x"], pruned["gram"], pruned["graph"], *run_args(pruned, v), W_P, K_P, 0, pruned["lengths"])
            for v in VARIANTS}


@pytest.mark.parametrize("variant", VARIANTS)
def test_pruned_search_against_restatement(device, pruned, decoded, variant):
    """T = 160, B = 8 (odd utterances ragged), V = 300 (24 unigrams, 275 bigrams), beam 16, top_k 8, 400 phrases planted by the
    3-character windows of the unbiased restatement's strings.  compare_nbest's conditions with the cap 0: on these inputs (seed
    20261101) the float32 twin of the restatement (the device's bits per look-up, every addition rounded) and the float64
    restatement return identical ordered lists in 8 of 8 utterances, with and without the model, the worst float32 / float64 score
    gap being 0.005 (without the model) / 0.023 (with it) of the tolerance, and the bias changes all 8 top-1 strings
    (tests/test_gram_ctx_bias_cpu.py asserts it)."""
    out = decoded[variant]
    model, alpha, beta = run_args(pruned, variant)
    x, gram, lengths, g = pruned["x"], pruned["gram"], pruned["lengths"], pruned["graph"]
    check_padding(out[0], out[1], out[2], 0)
    unused_slots_are_empty(out)
    gpu = [hyps5(out, b) for b in range(B_P)]
    compare_nbest([[(h[0], h[1]) for h in hb] for hb in gpu], [[(w[0], w[1]) for w in wb] for wb in pruned["want"][variant]], 0)
    worst = [0.0, 0.0]
    for b in range(B_P):
        assert len({h[0] for h in gpu[b]}) == len(gpu[b]), b                   # no string twice
        for s, sc, c, l, bv in gpu[b]:
            f = (c + (alpha * l + beta * len(s))) + bv if variant == "lm" else c + bv
            worst[0] = max(worst[0], abs(sc - f) / tol(f))
            assert abs(sc - f) <= tol(f), (b, s, sc, f)
            exact = cref.occurrences(s, pruned["phrases"], pruned["weights"])
            worst[1] = max(worst[1], abs(bv - exact) / tol(exact))
            assert abs(bv - exact) <= tol(exact), (b, s, bv, exact)
    print("worst |score - formula| / tol %.3g, |bias - counting| / tol %.3g" % tuple(worst))
    plain = gbeam(device, x, gram, W_P, K_P, 0, lengths)
    changed = sum(1 for b in range(B_P) if gpu[b][0][0] != base.hyps(*plain, b)[0][0])
    print("top-1 differs from gram_beam_decode's in %d of %d utterances" % (changed, B_P))
    assert changed >= 1


# ------------------------------------------------------------------------------------------------ 5. scores and sizes
@pytest.mark.parametrize("variant", VARIANTS)
def test_ctx_score_over_the_decoded_strings_gives_out_bias_bit_for_bit(device, pruned, decoded, variant):
    out = decoded[variant]
    B, W, L = out[0].shape
    _, dev_bias = pruned["graph"].score(torch.from_numpy(np.ascontiguousarray(out[0].reshape(B * W, L))).to(device),
                                        torch.from_numpy(np.ascontiguousarray(out[1].reshape(B * W))).to(device), True)
    dev_bias = dev_bias.cpu().numpy().reshape(B, W)
    assert dev_bias.dtype == out[5].dtype and dev_bias.tobytes() == out[5].tobytes()
    assert np.sum(out[5] > 0) >= B


@pytest.mark.parametrize("T,B,V,U,W,K,seed", [(30, 2, 80, 10, 128, 32, 17), (30, 2, 80, 10, 64, 64, 18)])
def test_largest_shapes_with_model_and_graph(device, T, B, V, U, W, K, seed):
    """more than one look-up per thread (up to 4096 extensions on 256 threads) and the full LDS footprint, under the edge-case
    conditions of tests/test_gram_beam_lm_gpu.py"""
    x = base.small(T, B, V, seed)
    gram = gref.random_table(V, U, seed)
    model = edge_model(V, 4, seed)
    rs = np.random.RandomState(seed)
    phrases, weights = char_phrases(rs, chars_of(gram), 60, 1, 3)
    g = make_graph(phrases, V, weights)
    d, dl = cref.DictGraph(phrases, weights), lmref.DictLM.of(model)
    out = gbiased(device, x, gram, g, model, ALPHA, BETA, W, K)
    check_padding(out[0], out[1], out[2], 0)
    unused_slots_are_empty(out)
    for b in range(B):
        want = [(w[0], w[1]) for w in gcb.beam_search_bias(x[:, b], gram, d, dl, ALPHA, BETA, W, K)]
        got = [(h[0], h[1]) for h in hyps5(out, b)]
        assert len(got) == len(want), b
        assert len({h[0] for h in got}) == len(got), b
        for (_, gs_), (_, ws_) in zip(got, want):
            assert abs(gs_ - ws_) <= tol(ws_), (b, gs_, ws_)
        gs, ws = dict(got), dict(want)
        for s in set(gs) & set(ws):
            assert abs(gs[s] - ws[s]) <= tol(ws[s]), (b, s)
        for s in set(gs) - set(ws):
            assert gs[s] <= want[-1][1] + tol(want[-1][1]), (b, s)
        for s in set(ws) - set(gs):
            assert ws[s] <= got[-1][1] + tol(got[-1][1]), (b, s)
        for s, _, _, _, bv in hyps5(out, b):
            assert bv == cref.occurrences(s, phrases, weights), (b, s, bv)        # multiples of 0.5: exact
        biased_n = sum(1 for h in hyps5(out, b) if h[4] > 0)
        print("T%d V%d W%d K%d utterance %d: %d strings, %d with a phrase, %d on one side only"
              % (T, V, W, K, b, len(got), biased_n, len(set(gs) ^ set(ws))))
        assert biased_n >= 1


# ------------------------------------------------------------------------------------------------ 6. robustness
def test_launches_repeat_and_padding_is_never_read(device, pruned, decoded):
    x, lengths, gram, g, model = pruned["x"], pruned["lengths"], pruned["gram"], pruned["graph"], pruned["model"]
    a = decoded["lm"]
    a2 = gbiased(device, x, gram, g, model, ALPHA, BETA, W_P, K_P, 0, lengths)
    y = x.copy()
    for b in range(B_P):
        y[lengths[b]:, b] = np.nan
    c = gbiased(device, y, gram, g, model, ALPHA, BETA, W_P, K_P, 0, lengths)
    for u, v, w in zip(a, a2, c):
        assert u.tobytes() == v.tobytes() == w.tobytes()
    p = decoded["plain"]
    p2 = gbiased(device, y, gram, g, None, 0.0, 0.0, W_P, K_P, 0, lengths)
    for u, v in zip(p, p2):
        assert u.tobytes() == v.tobytes()
    assert np.all(p[4] == 0.0)


def _raw_call(device, graph, T, B, V, W, K, nbytes=None, model=None, n_states=None, slots=None, max_probe=None, ret=True,
              vals=None, x=None, gram=None, with_gram=True, out_bias=True, **lm_over):
    from asr import _lib, _ops
    lib = _lib.lib()
    graph.to(device)
    img = graph.image
    x = torch.zeros((T, B, V), dtype=torch.float32, device=device) if x is None else x
    if gram is None:
        gram = np.full((V, 2), -1, np.int32)
        gram[1:, 0] = np.arange(1, V)
    gt = torch.from_numpy(np.ascontiguousarray(gram, np.int32)).to(device)
    need = lib.asr_gram_ctc_beam_bias_workspace_bytes(T, B, V, W, K)
    assert need == lib.asr_gram_ctc_beam_workspace_bytes(T, B, V, W, K)
    nbytes = need if nbytes is None else nbytes(need)
    ws = torch.empty(max(1, need), dtype=torch.uint8, device=device)
    ids = torch.full((B, W, 2 * T), -7, dtype=torch.int32, device=device)
    ln = torch.full((B, W), -7, dtype=torch.int32, device=device)
    sc, cc, lc, bc = (torch.full((B, W), 7.0, dtype=torch.float32, device=device) for _ in range(4))
    if model is None:
        lm_args, bos, eos = [None, 0, None, None, 0, 0, 0], -1, -1
    else:
        model.to(device)
        lm_args, bos, eos = list(_ops._lm_args(model.image)), model.bos_id, model.eos_id
        for k, name in enumerate(("uni", "vlm", "keys", "vals", "slots", "max_probe", "order")):
            if "lm_" + name in lm_over:
                lm_args[k] = lm_over["lm_" + name]
        bos = lm_over.get("bos", bos)
    rc = lib.asr_gram_ctc_beam_search_bias(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"),
                                           _lib.ptr(gt) if with_gram else None, *lm_args, bos, eos, 0.5, 1.0, _lib.ptr(ws), nbytes,
                                           _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(cc), _lib.ptr(lc),
                                           _lib.ptr(img["keys"]), _lib.ptr(img["vals"] if vals is None else vals),
                                           img["slots"] if slots is None else slots,
                                           img["max_probe"] if max_probe is None else max_probe,
                                           _lib.ptr(img["ret"]) if ret else None, img["n_states"] if n_states is None else n_states,
                                           _lib.ptr(bc) if out_bias else None)
    torch.cuda.synchronize()
    return rc, ids.cpu().numpy(), ln.cpu().numpy(), [t.cpu().numpy() for t in (sc, cc, lc, bc)]


def test_limits_workspace_model_and_graph_arguments(device):
    V = 100
    rs = np.random.RandomState(3)
    g = make_graph(cref.random_phrases(rs, V, 50, 1, 4), V)
    model = make_lm(lmref.random_model(rs, V, 3, n_random=500), V)
    for m in (None, model):
        for W, K in ((129, 1), (1, 65), (65, 64), (128, 33), (128, 64)):
            assert _raw_call(device, g, 4, 1, V, W, K, model=m)[0] == ASR_ERR_UNSUPPORTED, (W, K)
        assert _raw_call(device, g, 4, 1, V, 16, 16, lambda n: n - 1, model=m)[0] == ASR_ERR_WORKSPACE
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, with_gram=False)[0] == ASR_ERR_UNSUPPORTED
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, n_states=0)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, ret=False)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, slots=12)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, max_probe=0)[0] == ASR_ERR_BAD_ARG
        assert _raw_call(device, g, 4, 1, V, 16, 16, model=m, out_bias=False)[0] == ASR_ERR_BAD_ARG
        # every element of every output is written: 4 frames of zeros, 16 slots
        rc, ids, ln, scores = _raw_call(device, g, 4, 1, V, 16, 16, model=m)
        assert rc == 0 and ids.min() >= 0 and ln.min() >= 0 and all(np.all(s != 7.0) for s in scores)
    assert _raw_call(device, g, 4, 1, V, 16, 16, model=model, lm_order=5)[0] == ASR_ERR_UNSUPPORTED
    assert _raw_call(device, g, 4, 1, V, 16, 16, model=model, lm_order=0)[0] == ASR_ERR_BAD_ARG
    assert _raw_call(device, g, 4, 1, V, 16, 16, model=model, lm_slots=12)[0] == ASR_ERR_BAD_ARG
    assert _raw_call(device, g, 4, 1, V, 16, 16, model=model, lm_max_probe=0)[0] == ASR_ERR_BAD_ARG
    assert _raw_call(device, g, 4, 1, V, 16, 16, model=model, lm_vlm=V - 1)[0] == ASR_ERR_BAD_ARG
    assert _raw_call(device, g, 4, 1, V, 16, 16, model=model, bos=V + 2)[0] == ASR_ERR_BAD_ARG
    # the largest accepted shapes
    assert _raw_call(device, g, 4, 1, V, 128, 32, model=model)[0] == 0 and _raw_call(device, g, 4, 1, V, 64, 64, model=model)[0] == 0


def test_a_table_with_damaged_next_fields_stays_in_range(device, pruned):
    """every `next` of the table overwritten on the host with out-of-range values: the call returns 0, reads nothing out of range
    (such a `next` counts as the root) and every id it writes is a character of the table"""
    g, gram = pruned["graph"], pruned["gram"]
    vals = g.host_image()["vals"].copy()
    vals[:, 0] = np.where(np.arange(len(vals)) % 2 == 0, 0x7fffffff, -5)
    x = torch.from_numpy(np.ascontiguousarray(pruned["x"][:40])).to(device)
    for m in (None, pruned["model"]):
        rc, ids, ln, scores = _raw_call(device, g, 40, B_P, V_P, W_P, K_P, vals=torch.from_numpy(vals).to(device), x=x, gram=gram,
                                        model=m)
        assert rc == 0 and ids.min() >= 0 and ids.max() <= gcb.U_P and ln.min() >= 0 and ln.max() <= 80
        assert np.all(np.isfinite(scores[3]))


# ------------------------------------------------------------------------------------------------ 7. streaming
def open_stream(device, B, V, F, gram, W, K, blank, model, graph):
    from asr import error
    a, b = (ALPHA, BETA) if model is not None else (0.0, 0.0)
    return error.GramBeamStream(B, V, F, gram, W, K, blank, None, model, a, b, device, graph=graph)


def stream_setup(T, B, V, U, seed, blank=0):
    gram = gref.random_table(V, U, seed, blank)
    rs = np.random.RandomState(seed)
    phrases, weights = char_phrases(rs, chars_of(gram), 30, 1, 4)
    return base.small(T, B, V, seed), gram, edge_model(V, 4, seed), make_graph(phrases, V, weights, blank=blank)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T,B,V,U,W,K,blank,seed", [(1, 3, 8, 3, 8, 4, 0, 11), (20, 3, 9, 3, 4, 5, 0, 41), (15, 3, 9, 3, 8, 5, 3, 14),
                                                     (30, 2, 80, 10, 64, 64, 0, 18)])
def test_chunking_invariance(device, T, B, V, U, W, K, blank, seed, variant):
    """one chunk, one frame per chunk and two uneven cuttings: result() is the one-shot entry's output, bytes for bytes"""
    x, gram, model, g = stream_setup(T, B, V, U, seed, blank)
    model = model if variant == "lm" else None
    a, bt = (ALPHA, BETA) if model is not None else (0.0, 0.0)
    want = gbiased(device, x, gram, g, model, a, bt, W, K, blank)
    assert np.any(want[5] > 0) or T == 1
    for cuts in cuttings(T, seed):
        s = open_stream(device, B, V, T, gram, W, K, blank, model, g)
        assert feed(s, device, x, cuts) == T
        got = fetch(s)
        assert len(got) == 6 and got[0].shape == (B, W, 2 * T)
        same(got, want)
        assert s.frames.cpu().tolist() == [T] * B


@pytest.mark.parametrize("variant", VARIANTS)
def test_result_after_every_chunk_lengths_with_zeros_and_a_partial_reset(device, variant):
    """chunks of 3 frames with per-utterance lengths (utterance 1 gets nothing in every other chunk), result() after every chunk
    against the one-shot entry on the frames so far; utterance 2 is reset in the middle and goes on from there"""
    T, B, V, U, W, K = 21, 3, 9, 3, 8, 5
    x, gram, model, g = stream_setup(T, B, V, U, 43)
    model = model if variant == "lm" else None
    a, bt = (ALPHA, BETA) if model is not None else (0.0, 0.0)
    xt = torch.from_numpy(x).to(device)
    s = open_stream(device, B, V, T, gram, W, K, 0, model, g)
    seen = [np.zeros((0, V), np.float32) for _ in range(B)]          # the frames every utterance has consumed since its reset
    for k, t0 in enumerate(range(0, T, 3)):
        lens = np.array([3, 0 if k % 2 else 2, 3], np.int32)
        if t0 == 9:
            s.reset(mask=[0, 0, 1])
            seen[2] = np.zeros((0, V), np.float32)
        s.advance(xt[t0:t0 + 3], torch.from_numpy(lens).to(device))
        for b in range(B):
            seen[b] = np.concatenate([seen[b], x[t0:t0 + lens[b], b]])
        got = fetch(s)
        same(fetch(s), got)                                  # result does not change the state
        assert len(got) == 6 and got[0].shape == (B, W, 2 * (t0 + 3))
        assert s.frames.cpu().tolist() == [len(f) for f in seen]
        for b in range(B):
            n = len(seen[b])
            want = gbiased(device, np.zeros((1, 1, V), np.float32) if n == 0 else seen[b][:, None, :], gram, g, model, a, bt, W, K,
                           0, np.array([n], np.int32))
            same(tuple(o[b:b + 1] for o in got), want, T=min(2 * max(n, 1), got[0].shape[2]))
            assert np.all(got[0][b, :, 2 * n:] == 0)


class Raw:
    """the asr_gram_ctc_beam_bias_stream_* entries (and, with bias=None, the asr_gram_ctc_beam_stream_* ones) through the raw
    ABI over a state with a canary tail"""
    CANARY, TAIL = 0xA5, 4096

    def __init__(self, device, B, V, F, W, K, gram, model, graph):
        from asr import _lib, _ops
        self.lib, self._lib, self._ops = _lib.lib(), _lib, _ops
        self.device, self.B, self.V, self.F, self.W, self.K = device, B, V, F, W, K
        self.gram = torch.from_numpy(np.ascontiguousarray(gram, np.int32)).to(device)
        self.model = None if model is None else model.to(device)
        self.graph = graph.to(device)
        self.st_bytes = self.lib.asr_gram_ctc_beam_bias_stream_state_bytes(B, W, F, model is not None, 1)
        self.ws_bytes = self.lib.asr_gram_ctc_beam_stream_workspace_bytes(F, B, V, W, K)
        self.st = torch.full((self.st_bytes + self.TAIL,), self.CANARY, dtype=torch.uint8, device=device)
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=device)

    def lm_args(self):
        return [None, 0, None, None, 0, 0, 0] if self.model is None else list(self._ops._lm_args(self.model.image))

    def g_args(self, bias, **over):
        if not bias:
            return [None, None, 0, 0, None, 0]
        a = list(self._ops._graph_args(self.graph.image))
        for k, name in enumerate(("keys", "vals", "slots", "max_probe", "ret", "n_states")):
            if name in over:
                a[k] = over[name]
        return a

    def bos(self):
        return -1 if self.model is None else self.model.bos_id

    def fill(self):
        self.st.fill_(self.CANARY)

    def reset(self, bias):
        """bias None: the entry of the family without a graph"""
        p, with_lm = self._lib.ptr, int(self.model is not None)
        if bias is None:
            return self.lib.asr_gram_ctc_beam_stream_reset(self._lib.stream(), p(self.st), self.st_bytes, self.B, self.W, self.F, with_lm,
                                                           None)
        return self.lib.asr_gram_ctc_beam_bias_stream_reset(self._lib.stream(), p(self.st), self.st_bytes, self.B, self.W, self.F,
                                                            with_lm, int(bias), None)

    def advance(self, x, fb, bias, **over):
        p = self._lib.ptr
        head = (self._lib.stream(), p(x), None, x.shape[0], self.B, self.V, 0, self.W, self.K, float("-inf"), p(self.gram),
                *self.lm_args(), self.bos())
        tail = (ALPHA, BETA, fb, self.F, p(self.st), self.st_bytes, p(self.ws), self.ws_bytes)
        if bias is None:
            rc = self.lib.asr_gram_ctc_beam_stream_advance(*head, *tail)
        else:
            rc = self.lib.asr_gram_ctc_beam_bias_stream_advance(*head, *self.g_args(bias, **over), *tail)
        torch.cuda.synchronize()
        return rc

    def result(self, Lcap, bias, out_bias=True, **over):
        p, B, W = self._lib.ptr, self.B, self.W
        ids = torch.full((B, W, Lcap), -7, dtype=torch.int32, device=self.device)
        ln = torch.full((B, W), -7, dtype=torch.int32, device=self.device)
        sc, cc, lc, bc = (torch.full((B, W), 7.0, dtype=torch.float32, device=self.device) for _ in range(4))
        fr = torch.full((B,), -7, dtype=torch.int32, device=self.device)
        extra = self.model is not None or bool(bias)
        head = (self._lib.stream(), *self.lm_args(), self.bos(), -1)
        mid = (ALPHA, BETA, B, W, self.F, 0, Lcap, p(self.st), self.st_bytes, p(ids), p(ln), p(sc), p(cc) if extra else None,
               p(lc) if extra else None)
        if bias is None:
            rc = self.lib.asr_gram_ctc_beam_stream_result(*head, *mid, p(fr))
        else:
            rc = self.lib.asr_gram_ctc_beam_bias_stream_result(*head, *self.g_args(bias, **over), *mid,
                                                               p(bc) if bias and out_bias else None, p(fr))
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy() for t in (ids, ln, sc, cc, lc, bc)], fr.cpu().numpy()

    def state_bytes(self):
        return self.st.cpu().numpy().tobytes()

    def canary_intact(self):
        return bool((self.st[self.st_bytes:] == self.CANARY).all().item())


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_two_stream_families_share_states_without_a_graph_and_refuse_a_variant_mismatch(device, variant):
    T, B, V, U, W, K = 8, 2, 30, 5, 16, 8
    x, gram, model, g = stream_setup(T, B, V, U, 61)
    model = model if variant == "lm" else None
    xt = torch.from_numpy(x).to(device)
    r = Raw(device, B, V, T, W, K, gram, model, g)
    # with_bias == 0: the new entries and the old ones write identical state bytes, and each reads the other's state
    images = []
    for fam in (None, False):
        r.fill()
        assert r.reset(fam) == 0 and r.advance(xt[:4], 0, fam) == 0
        images.append(r.state_bytes())
    assert images[0] == images[1]
    assert r.advance(xt[4:], 4, None) == 0                       # the state the new family wrote, advanced by the old one
    mixed = r.result(2 * T, False)
    r.fill()
    assert r.reset(None) == 0 and r.advance(xt, 0, None) == 0
    old = r.result(2 * T, None)
    assert mixed[0] == 0 and old[0] == 0 and old[2].tolist() == [T] * B and mixed[2].tolist() == [T] * B
    for u, v in zip(mixed[1][:3], old[1][:3]):
        assert u.tobytes() == v.tobytes()
    want = gbeam(device, x, gram, W, K) if model is None else gfused(device, x, gram, model, ALPHA, BETA, W, K, 0, None, None, False)
    for u, v in zip(old[1], want):
        assert u.tobytes() == v.tobytes()
    # a state reset without the bias bit, given to calls with a graph: left alone, reported with out_frames -1
    before = r.state_bytes()
    assert r.advance(xt[:1], 0, True) == 0
    assert r.state_bytes() == before
    rc, out, fr = r.result(2 * T, True)
    assert rc == 0 and fr.tolist() == [-1] * B
    assert np.all(out[0] == 0) and np.all(out[1] == 0) and np.all(out[2] == -np.inf) and np.all(out[3] == -np.inf)
    assert np.all(out[4] == 0.0) and np.all(out[5] == 0.0)
    assert r.state_bytes() == before
    # and the reverse: a state with the bias bit given to calls without a graph
    r.fill()
    assert r.reset(True) == 0 and r.advance(xt[:4], 0, True) == 0
    before = r.state_bytes()
    assert before != images[0]
    for fam in (None, False):
        assert r.advance(xt[4:], 4, fam) == 0
        assert r.state_bytes() == before
        assert r.result(2 * T, fam)[2].tolist() == [-1] * B
    assert r.advance(xt[4:], 4, True) == 0 and r.state_bytes() != before
    rc, out, fr = r.result(2 * T, True)
    a, bt = (ALPHA, BETA) if model is not None else (0.0, 0.0)
    want = gbiased(device, x, gram, g, model, a, bt, W, K, 0, None, None, False)
    assert rc == 0 and fr.tolist() == [T] * B
    for u, v in zip(out, want):
        assert u.tobytes() == v.tobytes()
    # the graph-argument checks, all before the first launch
    before = r.state_bytes()
    assert r.advance(xt[:1], 0, True, n_states=0) == ASR_ERR_BAD_ARG
    assert r.advance(xt[:1], 0, True, slots=12) == ASR_ERR_BAD_ARG
    assert r.advance(xt[:1], 0, True, max_probe=0) == ASR_ERR_BAD_ARG
    assert r.advance(xt[:1], 0, True, ret=None) == ASR_ERR_BAD_ARG             # a graph without its ret is not "no graph"
    assert r.result(2 * T, True, slots=12)[0] == ASR_ERR_BAD_ARG
    assert r.result(2 * T, True, out_bias=False)[0] == ASR_ERR_BAD_ARG
    assert r.advance(xt[:1], T, True) == ASR_ERR_UNSUPPORTED                   # frames_before + Tc > max_frames
    assert r.state_bytes() == before and r.canary_intact()


def test_the_class_validates_the_graph_and_the_tuple_goes_into_mbr_decode(device):
    from asr import error
    V = 9
    gram = gref.random_table(V, 3, 1)
    with pytest.raises(ValueError):
        error.GramBeamStream(2, V, 10, gram, graph=make_graph([(1, 2)], V + 1), device=device)
    with pytest.raises(ValueError):
        error.GramBeamStream(2, V, 10, gram, graph=make_graph([(1, 2)], V, blank=3), device=device)
    x = torch.from_numpy(base.small(6, 2, V, 1)).to(device)
    with pytest.raises(ValueError):
        error.gram_beam_decode_biased(x, gram, make_graph([(1, 2)], V + 1))
    chars = chars_of(gram)
    g = make_graph([(chars[0], chars[1]), (chars[2],)], V, [1.0, 0.5])
    s = error.GramBeamStream(2, V, 10, gram, 4, 4, device=device, graph=g)
    s.advance(x)
    out = s.result()
    assert len(out) == 6 and out[0].shape == (2, 4, 12)
    one = error.gram_beam_decode_biased(x, gram, g, None, 0.0, 0.0, 4, 4)
    same(tuple(o.cpu().numpy() for o in out), tuple(o.cpu().numpy() for o in one))
    picked = error.mbr_decode(*one[:3])                    # ids, lengths and the combined score, as they come
    torch.cuda.synchronize()
    index = picked.index.cpu().numpy()
    assert np.all(index >= 0) and np.all(np.isfinite(one[2].cpu().numpy()[np.arange(2), index]))
