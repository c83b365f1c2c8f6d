"""Contextual phrase biasing, host side (no GPU): the automaton compiler and the table builder of asr/bias.py against brute-force
occurrence counting and the dictionary automaton of tests/ctx_bias_reference.py, the constructor's checks, and the restatement
of the biased search against the two restatements it extends."""
import numpy as np
import pytest

import ctc_beam_lm_reference as lmref
import ctc_beam_reference as ref
import ctx_bias_reference as cref


def graph_of(phrases, V, weights=None, **kw):
    from asr import bias
    return bias.ContextGraph(phrases, V, weights, **kw)


def random_sets():
    """(seed, V, phrases, weights): 60 phrase sets over 3-5 symbols with nested prefixes, proper suffixes and overlaps"""
    for seed in range(60):
        rs = np.random.RandomState(seed)
        nsym = 3 + seed % 3
        phrases, weights = cref.tricky_phrases(rs, range(1, nsym + 1), int(rs.randint(3, 9)), 4)
        yield seed, nsym + 1, phrases, weights, rs


# ------------------------------------------------------------------------------------------------ 1. compiler
def test_finalised_score_is_occurrence_counting_and_open_bounds_it():
    worst, strings = 0.0, 0
    for seed, V, phrases, weights, rs in random_sets():
        d = cref.DictGraph(phrases, weights)
        tw = cref.Image32(graph_of(phrases, V, weights).host_image())
        for _ in range(50):
            h = rs.randint(1, V, size=rs.randint(0, 13)).tolist()
            exact = cref.occurrences(h, phrases, weights)
            assert abs(d.score(h) - exact) <= 1e-9, (seed, h)
            toks, s = tw.tokens(h)
            opened = float(np.sum(np.array(toks, np.float64)))
            final = opened + float(tw.ret(s))
            worst = max(worst, abs(final - exact))
            assert abs(final - exact) <= 1e-4 * max(1.0, exact), (seed, h, final, exact)
            assert opened >= final - 1e-5 and final >= -1e-5, (seed, h, opened, final)
            assert d.score(h, False) >= d.score(h) - 1e-12 >= -1e-12
            strings += 1
    print("%d strings: worst |image sum - occurrence counting| %.3g" % (strings, worst))


def test_sparse_image_reproduces_the_dense_automaton():
    """state by state: the image's integer state stands for the dictionary automaton's string on every prefix of every string,
    and every delta is the float64 one rounded (a fallback adds two rounded terms: 1 ulp of the largest)"""
    for seed, V, phrases, weights, rs in random_sets():
        d = cref.DictGraph(phrases, weights)
        g = graph_of(phrases, V, weights)
        tw = cref.Image32(g.host_image())
        name = {0: ()}                            # image state -> dictionary state
        for _ in range(50):
            h = rs.randint(1, V, size=rs.randint(1, 13)).tolist()
            s, t = 0, ()
            for c in h:
                s, dv = tw.step(s, c)
                t, want = d.step(t, c)
                assert name.setdefault(s, t) == t, (seed, h)
                assert abs(float(dv) - want) <= 1e-6 * max(1.0, abs(want)), (seed, h, c, dv, want)
                assert abs(float(tw.ret(s)) - d.ret(t)) <= 1e-6 * max(1.0, abs(d.ret(t)))
        assert len(set(name.values())) == len(name) <= g.n_states == len(d.edge) + 1


def test_the_issue_s_example_sizes():
    """400 phrases of 2-5 tokens over V = 300: the sparse table stays near two transitions per state"""
    rs = np.random.RandomState(5)
    phrases = cref.random_phrases(rs, 300, 400, 2, 5)
    g = graph_of(phrases, 300)
    img = g.host_image()
    stored = int((img["keys"][:, 0] >= 0).sum())
    print("400 phrases over 300 ids: %d states, %d stored transitions, %d slots, max_probe %d"
          % (g.n_states, stored, img["slots"], img["max_probe"]))
    assert g.n_states - 1 <= stored <= 4 * g.n_states


# ------------------------------------------------------------------------------------------------ 2. table invariants
def test_table_invariants():
    rs = np.random.RandomState(9)
    phrases = cref.random_phrases(rs, 3000, 2000, 1, 6)
    g = graph_of(phrases, 3000, rs.choice([0.5, 1.0, 2.0], size=len(phrases)).tolist())
    img = g.host_image()
    S = img["slots"]
    used = img["keys"][:, 0] >= 0
    assert S & (S - 1) == 0 and 2 * used.sum() <= S
    assert np.all(img["keys"][~used] == -1)
    assert np.all((img["vals"][used, 0] >= 0) & (img["vals"][used, 0] < g.n_states))
    assert img["ret"].shape == (g.n_states,) and img["ret"][0] == 0.0 and np.all(img["ret"] <= 0.0)
    longest = 0
    for s, c in img["keys"][used].tolist():
        assert cref.probe(img, s, c) is not None, (s, c)
        longest = max(longest, cref.probes_needed(img, s, c))
    assert longest == img["max_probe"]
    # an empty graph: one state, no table
    e = graph_of([], 10).host_image()
    assert e["n_states"] == 1 and e["slots"] == 0 and e["max_probe"] == 0 and e["ret"].tolist() == [0.0]


# ------------------------------------------------------------------------------------------------ 3. constructor
@pytest.mark.parametrize("phrases,weights", [
    ([[1, 2], []], None),                        # an empty phrase
    ([[1, 5]], None),                            # an id outside [0, V)
    ([[-1]], None),
    ([[1, 0, 2]], None),                         # the blank
    ([[1, 2], [3], [1, 2]], None),               # a duplicate
    ([[1, 2]], [0.0]),                           # weights that are not finite and positive
    ([[1, 2]], [-1.0]),
    ([[1, 2]], [float("inf")]),
    ([[1, 2]], [float("nan")]),
    ([[1, 2]], [1.0, 2.0]),                      # one weight too many
])
def test_constructor_rejects_bad_input(phrases, weights):
    with pytest.raises(ValueError):
        graph_of(phrases, 5, weights)


def test_constructor_rejects_a_table_above_the_limit(monkeypatch):
    from asr import bias
    monkeypatch.setattr(bias, "MAX_TRANSITIONS", 5)
    with pytest.raises(ValueError):
        bias.ContextGraph([[1, 2, 3], [2, 3, 4]], 5)
    assert bias.ContextGraph([[1, 2, 3], [4]], 5).n_states == 5


def test_boost_scales_every_weight_and_the_blank_may_move():
    g = graph_of([[0, 1], [2]], 4, [1.0, 3.0], boost=0.5, blank=3)
    assert g.weights == [0.5, 1.5]
    with pytest.raises(ValueError):
        graph_of([[0, 3]], 4, blank=3)
    with pytest.raises(ValueError):
        graph_of([[1]], 4, boost=0.0)


# ------------------------------------------------------------------------------------------------ 4. from_text
def test_from_text_counts_dropped_phrases():
    from asr import bias
    tok = {"_": 0, "a": 1, "b": 2, "c": 3}
    g = bias.ContextGraph.from_text(["abc", "", "bq", "ca", "zz"], tok, weights=[1.0, 9.0, 2.0, 3.0, 4.0], boost=2.0)
    assert g.phrases == [(1, 2, 3), (3, 1)] and g.weights == [2.0, 6.0] and g.dropped == 2 and g.V == 4
    d = cref.DictGraph.of(g)
    assert d.score([1, 2, 3, 1]) == 2.0 * 3 + 6.0 * 2


# ------------------------------------------------------------------------------------------------ 5. restatement
@pytest.mark.parametrize("f32", [False, True])
def test_empty_graph_restates_the_parent_searches(f32):
    """no phrases: labels and scores of ctc_beam_reference.beam_search and ctc_beam_lm_reference.beam_search_lm, exactly"""
    V = 7
    rs = np.random.RandomState(3)
    x = (rs.randn(25, V) * 2).astype(np.float32)
    ng = lmref.random_model(rs, V, 3, [rs.randint(1, V, size=5).tolist() for _ in range(6)], n_random=60)
    lm = lmref.DictLM(ng, 3, V, V + 1)
    empty = cref.Image32(graph_of([], V).host_image()) if f32 else cref.DictGraph([], [])
    for W, K in ((4, 3), (16, 6)):
        got = cref.beam_search_bias(x, empty, lm, 0.6, 0.3, W, K, f32=f32)
        want = lmref.beam_search_lm(x, lm, 0.6, 0.3, W, K, f32=f32)
        assert [g[:4] for g in got] == want and all(g[4] == 0.0 for g in got)
        if not f32:
            got = cref.beam_search_bias(x, empty, None, 0.0, 0.0, W, K)
            assert [(g[0], g[1]) for g in got] == ref.beam_search(x, W, K)
            assert all(g[2] == g[1] and g[3] == 0.0 and g[4] == 0.0 for g in got)


def test_biased_restatement_ranks_by_the_exact_objective_when_nothing_is_pruned():
    (T, V, W, seed), count = ref.EXHAUSTIVE[0]
    x = ref.exhaustive_logits(T, V, seed)
    exact = ref.enumerate_paths(x)
    phrases, weights = [(1, 2), (2,), (2, 1, 1)], [1.0, 0.5, 2.0]
    d = cref.DictGraph(phrases, weights)
    got = cref.beam_search_bias(x, d, None, 0.0, 0.0, W, V - 1)
    assert len(got) == count and {g[0] for g in got} == set(exact)
    for lab, sc, ctc, _, b in got:
        assert abs(ctc - exact[lab]) <= 1e-9 and abs(b - cref.occurrences(lab, phrases, weights)) <= 1e-9
        assert abs(sc - (ctc + b)) <= 1e-12
    assert [g[1] for g in got] == sorted((g[1] for g in got), reverse=True)
