"""Gram-CTC keyword spotting on the GPU (csrc/ctc_kws.hip: asr_gram_kws_detect through asr.spot) against the float64 restatement of
tests/gram_keyword_reference.py, against the CTC keyword kernel (bit for bit on a bigram-free inventory; as the maximum over every
tokenisation of a phrase) and against the project's own Gram-CTC aligner.

det (after the cast to f32), every det_start, every hit start / end / count and hit_score must equal the restatement exactly: both
sides run the same IEEE float64 max and one addition per step on the same f32 logits.  fill and hit_logp contain the row's
log-sum-exp (f32 on the device): 1e-4 * max(1, |value|), the tolerance of tests/test_keyword_gpu.py.  Every test prints its worst
error / tolerance.
"""
import numpy as np
import pytest
import torch

import gram_keyword_reference as gref
import keyword_reference as ref

from asr import spot

pytestmark = pytest.mark.gpu

RTOL = 1e-4
EXACT = ("det", "start", "hit_start", "hit_end", "n_hits", "hit_score")
POISON_I, POISON_F = 0x5A5A5A5A, 12345.5
G, TILE = spot.SWEEP_GROUP, spot.GRAM_SWEEP_TILE
A, B_ = gref.A, gref.Bc


def _t(device, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def ratio(got, want):
    """worst |got - want| / tolerance over two float arrays; -inf must match -inf"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf) and not np.isnan(got).any()
    if inf.all():
        return 0.0
    return float((np.abs(got[~inf] - want[~inf]) / (RTOL * np.maximum(1.0, np.abs(want[~inf])))).max())


def run(device, xs, lengths, kws, max_hits=4, min_score=None):
    """numpy in -> dict of numpy arrays named as keyword_reference.search names them, through the public functions"""
    h = None if lengths is None else _t(device, lengths, np.int32)
    d = spot.keyword_detect(_t(device, xs, np.float32), kws, h)
    hits = spot.keyword_hits(d, h, max_hits, min_score)
    torch.cuda.synchronize()
    out = dict(det=d.score, start=d.start, fill=d.fill, hit_start=hits.start, hit_end=hits.end, hit_score=hits.score,
               hit_logp=hits.logp, n_hits=hits.count)
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(got, want, what):
    for k in EXACT:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(~((g == w) | (np.isnan(g.astype(np.float64)) & np.isnan(w.astype(np.float64)))))
        assert bad.size == 0, "%s: %s differs from the restatement, first at %s (%d elements): %r != %r" % (
            what, k, bad[0], len(bad), g[tuple(bad[0])], w[tuple(bad[0])])
    r = max(ratio(got["fill"], want["fill"]), ratio(got["hit_logp"], want["hit_logp"]))
    print("%s: worst error / tolerance of fill and hit_logp = %.3g" % (what, r))
    assert r <= 1.0, (what, r)
    return r


def check(device, xs, lengths, phrases, gram, what, max_hits=4, min_score=None):
    want = gref.search(xs, lengths, phrases, gram, 0, max_hits, -np.inf if min_score is None else min_score)
    got = run(device, xs, lengths, spot.GramKeywordSet(phrases, gram), max_hits, min_score)
    compare(got, want, what)
    return got, want


def found(got, b, k, s, e):
    """the planted span [s, e) of keyword k in utterance b is among the hits, with score exactly 0.0"""
    n = got["n_hits"][b, k]
    spans = list(zip(got["hit_start"][b, k, :n].tolist(), got["hit_end"][b, k, :n].tolist(), got["hit_score"][b, k, :n].tolist()))
    return (s, e, 0.0) in spans


# ------------------------------------------------------------------------------------------------ 1. shapes and dispatch edges
@pytest.mark.parametrize("L", [1, 2, 3, 4, 63, 64])
def test_phrase_lengths(device, L):
    """an inventory of 300 tokens (20 characters, 279 bigrams): one phrase planted in a peaked path with a random mix of unigram and
    bigram tokens and found with score exactly 0.0, beside its prefix and random logits.  L = 1: no G and no B at all; L = 2: the
    fresh start of G_2; L = 3: G_3 has no G_1; L = 63, 64: the last lanes"""
    gram = gref.big_table(20, 300, seed=1)
    V, T = 300, 300
    p = tuple(1 + (i * 7 + i // 20) % 20 for i in range(L))
    path, spans, used = gref.planted(T, [p], gram, seed=L)
    xs = np.stack([ref.peaked(path, V, seed=1), ref.random_logits(T, 1, V, 2)[:, 0]], 1)
    got, _ = check(device, xs, None, [p, p[:max(1, L // 2)]], gram, "L = %d" % L, max_hits=2, min_score=-0.5)
    (_, s, e), = spans
    assert got["n_hits"][0, 0] == 1 and found(got, 0, 0, s, e), (used, s, e, got["hit_start"][0, 0], got["hit_end"][0, 0])
    if L >= 63:
        assert any(v > 20 for v in used[0]) and any(v <= 20 for v in used[0])      # the path mixes bigram and unigram tokens


@pytest.mark.parametrize("K", [1, G, G + 1, 2 * G + 1])
def test_keywords_per_workgroup(device, K):
    xs = ref.random_logits(TILE + 5, 2, 6, 10 + K)
    check(device, xs, [TILE + 5, 9], gref.random_strings(K, 2, 1, 6, K), gref.SMALL, "K = %d" % K)


@pytest.mark.parametrize("T", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_frames_around_the_tile(device, T):
    """V = 9: repeated characters (cc), g_i = g_{i-2} (ababa), a phrase of every length up to 10"""
    xs = ref.random_logits(T, 3, 9, 20 + T)
    xs[::2] = np.round(xs[::2])                                      # ties between the candidates of a node
    phrases = [(1,), (2, 1), (3, 3), (3, 3, 4), (1, 2, 1, 2, 1), (3, 3, 3, 3), (1, 2, 3, 4, 1, 2, 3, 3, 4, 1)]
    check(device, xs, None, phrases, gref.NINE, "T = %d" % T)
    check(device, xs, [T, max(T - 1, 0), T // 2], phrases, gref.NINE, "T = %d, ragged" % T)


@pytest.mark.parametrize("gram", [gref.SMALL, gref.NO_B], ids=["ab", "without-b"])
@pytest.mark.parametrize("B", [1, 3])
def test_small_inventories_and_lengths(device, gram, B):
    """V = 6; lengths 0, 1 and T.  Without the unigram b: (a, b) is spelled by the bigram ab alone, (b, b) and (b) have no spelling
    at all (live rows whose every path is -inf), absent U nodes sit inside live phrases.  Dead and duplicate rows beside them."""
    T = 13
    xs = ref.random_logits(T, B, 6, 7 * B + int(gram[2, 0]))
    phrases = [(A, B_), (B_, B_), (B_,), (A, B_, A, B_), (), (A, 0), (A, A, A, A), (B_, A, A, B_), (A, B_), (7,), (A, B_, B_, A)]
    lengths = [T] if B == 1 else [0, 1, T]
    got, _ = check(device, xs, lengths, phrases, gram, "V = 6, B = %d" % B)
    for k in (4, 5, 9) + ((1, 2) if gram is gref.NO_B else ()):
        assert np.all(np.isneginf(got["det"][:, k])) and np.all(got["start"][:, k] == -1) and np.all(got["n_hits"][:, k] == 0)
    assert np.all(np.isfinite(got["det"][-1, 0, :])) and np.all(np.isfinite(got["det"][-1, 3, 2:]))
    for name in got:
        if name != "fill":
            assert np.array_equal(got[name][:, 0], got[name][:, 8]), name
    if B == 3:
        assert np.all(np.isneginf(got["det"][0])) and np.all(got["fill"][0] == 0) and np.all(got["n_hits"][0] == 0)
        assert np.all(np.isneginf(got["det"][1, :, 1:])) and np.all(got["start"][1, :, 1:] == -1)


def _raw(device, xs, lengths, kws, max_hits, min_score):
    """both entries with every output pre-filled with a poison value -> dict of numpy outputs"""
    from asr import _lib
    lib = _lib.lib()
    T, B, V = xs.shape
    kws.to(device)
    img = kws.image
    K, H = kws.K, max_hits
    x = _t(device, xs, np.float32)
    h = _t(device, lengths, np.int32)
    fi = lambda *s: torch.full(s, POISON_I, dtype=torch.int32, device=device)
    ff = lambda *s: torch.full(s, POISON_F, dtype=torch.float32, device=device)
    o = dict(det=ff(B, K, T), start=fi(B, K, T), fill=ff(B, T), hit_start=fi(B, K, H), hit_end=fi(B, K, H), hit_score=ff(B, K, H),
             hit_logp=ff(B, K, H), n_hits=fi(B, K))
    n = lib.asr_kws_workspace_bytes(T, B, kws.U)
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device=device)
    p = _lib.ptr
    rc = lib.asr_gram_kws_detect(_lib.stream(), p(x), p(h), T, B, V, kws.blank, p(img["uniq"]), kws.U, p(img["node_uni"]),
                                 p(img["node_big"]), p(img["kw_len"]), K, kws.Lmax, None, p(o["det"]), p(o["start"]), p(o["fill"]),
                                 p(ws), n)
    assert rc == 0
    rc = lib.asr_kws_hits(_lib.stream(), p(o["det"]), p(o["start"]), p(o["fill"]), p(h), B, K, T, H, min_score, p(o["hit_start"]),
                          p(o["hit_end"]), p(o["hit_score"]), p(o["hit_logp"]), p(o["n_hits"]))
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_poisoned_outputs_are_overwritten(device):
    T, B, V = TILE + 3, 4, 9
    xs = ref.random_logits(T, B, V, 41)
    lengths = [0, 1, T, TILE]
    phrases = [(1, 2), (), (3,), (9, 1), (4, 3, 3, 4, 1, 2, 1), (2, 2)]
    got = _raw(device, xs, lengths, spot.GramKeywordSet(phrases, gref.NINE), 3, -np.inf)
    compare(got, gref.search(xs, lengths, phrases, gref.NINE, 0, 3), "poisoned outputs")
    for name, a in got.items():
        assert not np.any(a == (POISON_I if a.dtype == np.int32 else np.float32(POISON_F))), name


# ------------------------------------------------------------------------------------------------ 2. against the CTC keyword kernel
def _detect(device, xs, lengths, kws):
    d = spot.keyword_detect(_t(device, xs, np.float32), kws, None if lengths is None else _t(device, lengths, np.int32))
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in d]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_bigram_free_inventory_equals_the_ctc_kernel_bit_for_bit(device):
    """without bigrams every G node is absent, and a -inf candidate never wins strictly: the outputs are those of asr_kws_detect"""
    V, T = 12, 2 * TILE + 3
    xs = ref.random_logits(T, 3, V, 90)
    xs[1::2] = np.round(xs[1::2])
    phrases = ref.random_phrases(6, V, 1, 9, 3) + [(3, 3, 3), (), (4, V), (5, 0), tuple(1 + i % 11 for i in range(64))]
    lengths = [T, 0, TILE + 1]
    want = _detect(device, xs, lengths, spot.KeywordSet(phrases, V))
    got = _detect(device, xs, lengths, spot.GramKeywordSet(phrases, gref.plain(V)))
    for name, g, w in zip(spot.Detection._fields, got, want):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), name
    assert np.isfinite(want[0][0, :6, 20:]).all()


@pytest.mark.parametrize("gram", [gref.SMALL, gref.NO_B, gref.NINE], ids=["ab", "without-b", "abcd"])
def test_det_is_the_maximum_of_the_ctc_kernel_over_all_tokenisations(device, gram):
    """the existing kernel as the yardstick: every tokenisation of every phrase as a keyword of its own"""
    V, T = gram.shape[0], TILE + 9
    n_chars = 2 if V == 6 else 4
    xs = ref.random_logits(T, 2, V, 95 + V)
    xs[::3] = np.round(xs[::3] * 2) / 2
    phrases = [p for p in gref.random_strings(12, n_chars, 1, 7, V) + [(1, 2, 1, 2, 1, 2), (1, 1, 1, 1, 1)] if gref.tokenisations(p, gram)]
    toks = [gref.tokenisations(p, gram) for p in phrases]
    assert len(phrases) >= 4 and max(len(t) for t in toks) >= (2 if gram is gref.NO_B else 8)
    each = _detect(device, xs, None, spot.KeywordSet([t for ts in toks for t in ts], V))[0]
    got = _detect(device, xs, None, spot.GramKeywordSet(phrases, gram))[0]
    row = 0
    for k, ts in enumerate(toks):
        want = each[:, row:row + len(ts)].max(axis=1)
        row += len(ts)
        assert np.array_equal(_bits(got[:, k]), _bits(want)), (k, phrases[k])


# ------------------------------------------------------------------------------------------------ 3. planted phrases, the aligner
def test_planted_phrases_are_found_whichever_tokens_spell_them(device):
    """six utterances, each a peaked path that spells the same three phrases with another random mix of unigram and bigram tokens"""
    phrases = [(1, 2, 1, 2), (3, 3, 4), (2, 1, 1)]
    T, V = 60, 9
    plants = [gref.planted(T, phrases, gref.NINE, seed) for seed in range(6)]
    xs = np.stack([ref.peaked(path, V, seed=i) for i, (path, _, _) in enumerate(plants)], 1)
    got, _ = check(device, xs, None, phrases, gref.NINE, "planted phrases", max_hits=3, min_score=-1.0)
    assert len({tuple(u) for _, _, used in plants for u in used}) >= 6
    for b, (_, spans, used) in enumerate(plants):
        for k, s, e in spans:
            assert found(got, b, k, s, e), (b, k, s, e, used[k])


def test_hits_against_the_gram_aligner(device):
    """for every hit, the Gram-CTC forced alignment of the phrase on logits[start:end] is compared with hit_logp.  The aligner also
    allows leading and trailing blanks, so its score is never below hit_logp.  For the first hit of a (b, k), and for every hit of
    score 0.0, it cannot be above either (tests/test_keyword_gpu.py gives the argument): there the two agree within the tolerance."""
    from asr.loss import gram_ctc_align
    gram = gref.NINE
    uni, big = gref.token_maps(gram)
    V, T = 9, 70
    phrases = [(1, 2, 1), (3, 3, 4), (4,), (2, 1, 2, 1)]
    path, _, _ = gref.planted(T, [phrases[0], phrases[1], phrases[2], phrases[3], phrases[0]], gram, seed=11)
    xs = np.stack([ref.peaked(path, V, seed=3, peak=4.0), ref.random_logits(T, 1, V, 4, scale=1.5)[:, 0]], 1)
    got, _ = check(device, xs, None, phrases, gram, "aligner cross-check: the search itself", max_hits=3)
    segs, labels, want, tight = [], [], [], []
    for b in range(2):
        for k, p in enumerate(phrases):
            for h in range(got["n_hits"][b, k]):
                s, e = got["hit_start"][b, k, h], got["hit_end"][b, k, h]
                segs.append(xs[s:e, b])
                labels.append(p)
                want.append(got["hit_logp"][b, k, h])
                tight.append(h == 0 or got["hit_score"][b, k, h] == 0.0)
    assert len(segs) >= 8 and sum(tight) >= 8
    Lmax = max(len(p) for p in labels)
    x = np.zeros((max(len(s) for s in segs), len(segs), V), np.float32)
    lu = np.zeros((len(segs), Lmax), np.int32)
    lb = np.full((len(segs), Lmax), -1, np.int32)
    for i, (seg, p) in enumerate(zip(segs, labels)):
        x[:len(seg), i] = seg
        lu[i, :len(p)] = [uni[c] for c in p]
        lb[i, 1:len(p)] = [big.get(cc, -1) for cc in zip(p, p[1:])]
    a = gram_ctc_align(_t(device, x), _t(device, lu), _t(device, lb), 0, _t(device, [len(s) for s in segs], np.int32),
                       _t(device, [len(p) for p in labels], np.int32))
    torch.cuda.synchronize()
    score, want, tight = a.score.cpu().numpy().astype(np.float64), np.asarray(want, np.float64), np.asarray(tight)
    tol = RTOL * np.maximum(1.0, np.abs(want))
    r = float((np.abs(score - want) / tol)[tight].max())
    low = float(((want - score) / tol).max())
    print("hit_logp against gram_ctc_align on the hit's frames, %d hits (%d tight): worst error / tolerance = %.3g, worst shortfall "
          "of the aligner / tolerance = %.3g" % (len(segs), tight.sum(), r, low))
    assert r <= 1.0 and low <= 1.0


# ------------------------------------------------------------------------------------------------ 4. streaming
STREAM_PHRASES = [(1, 2), (3, 3), (4,), (1, 2, 1, 2, 1), (2, 1, 1), (3, 3, 4, 3, 3)]


@pytest.mark.parametrize("chunk", [1, 7, TILE - 1, TILE, TILE + 1])
def test_stream_equals_one_shot(device, chunk):
    """full-length chunks: the chunk outputs concatenated along T are bit for bit the one-shot result and go into keyword_hits"""
    T, B, V = 2 * TILE + 9, 2, 9
    xs = ref.random_logits(T, B, V, 50 + chunk)
    kws = spot.GramKeywordSet(STREAM_PHRASES, gref.NINE)
    want = _detect(device, xs, None, kws)
    s = spot.KeywordStream(B, V, kws, device)
    parts = [s.advance(_t(device, xs[a:a + chunk])) for a in range(0, T, chunk)]
    got = [torch.cat([p[i] for p in parts], -1) for i in range(3)]
    for name, g, w in zip(spot.Detection._fields, got, want):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w)), name
    hits = spot.keyword_hits(spot.Detection(*got), None, 3)
    full = spot.keyword_hits(spot.Detection(*[_t(device, w) for w in want]), None, 3)
    for a, b in zip(hits, full):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    compare(run(device, xs, None, kws, 3), gref.search(xs, None, STREAM_PHRASES, gref.NINE, 0, 3),
            "stream, chunks of %d: the one-shot side" % chunk)


def test_stream_ragged_chunks_and_reset(device):
    """ragged lengths including 0: each utterance's outputs over its valid frames, in order, are the one-shot result of the frames
    it was fed; frames past a chunk's length hold -inf / -1 / 0; reset(mask) restarts only the masked utterances"""
    B, V, Tc = 3, 9, TILE + 2
    kws = spot.GramKeywordSet(STREAM_PHRASES, gref.NINE)
    rs = np.random.RandomState(9)
    chunks = [ref.random_logits(Tc, B, V, 60 + i) for i in range(4)]
    lens = [np.array([Tc, 0, 5]), np.array([0, Tc, 1]), np.array([TILE - 1, 3, 0]), rs.randint(0, Tc + 1, size=B)]
    s = spot.KeywordStream(B, V, kws, device)

    def feed(chunks, lens):
        outs = [[v.cpu().numpy() for v in s.advance(_t(device, c), _t(device, l, np.int32))] for c, l in zip(chunks, lens)]
        for (d, st, f), l in zip(outs, lens):
            for b in range(B):
                assert np.all(np.isneginf(d[b, :, l[b]:])) and np.all(st[b, :, l[b]:] == -1) and np.all(f[b, l[b]:] == 0)
        return outs

    def expect(b, chunks, lens, outs):
        fed = np.concatenate([c[:l[b], b] for c, l in zip(chunks, lens)], 0)
        if len(fed) == 0:
            return
        want = _detect(device, fed[:, None, :], None, kws)
        for i, name in enumerate(spot.Detection._fields):
            got = np.concatenate([o[i][b][..., :l[b]] for o, l in zip(outs, lens)], -1)
            assert np.array_equal(_bits(got), _bits(want[i][0])), (b, name)

    outs = feed(chunks, lens)
    for b in range(B):
        expect(b, chunks, lens, outs)
    s.reset(torch.tensor([1, 0, 1]))
    more = [ref.random_logits(Tc, B, V, 70 + i) for i in range(2)]
    mlens = [np.array([4, 2, Tc]), np.array([Tc, Tc, 7])]
    mouts = feed(more, mlens)
    expect(0, more, mlens, mouts)
    expect(2, more, mlens, mouts)
    expect(1, chunks + more, lens + mlens, outs + mouts)
    s.reset()
    outs = feed(chunks[:1], lens[:1])
    expect(0, chunks[:1], lens[:1], outs)


@pytest.mark.parametrize("B,K,L", [(1, 64, 16), (3, 6, 7), (2, 5, 7)])
def test_stream_state_is_large_enough_and_not_overrun(device, B, K, L):
    """the state is 36 B K Lmax + 4 B bytes: for odd B and even K Lmax not a whole number of 8-byte words (the first two cases), and
    the frame counters are its last words.  (a) KeywordStream allocates at least the bytes the library names; (b) reset and
    advance, given exactly those bytes inside a poisoned buffer, touch nothing behind them; (c) the stream equals one shot."""
    from asr import _lib
    lib = _lib.lib()
    gram = gref.big_table(20, 300, seed=2)
    V, T = 300, TILE + 3
    phrases = gref.random_strings(K - 1, 20, 1, L, B * 100 + K) + [tuple(range(1, L + 1))]
    kws = spot.GramKeywordSet(phrases, gram).to(device)
    assert (kws.K, kws.Lmax) == (K, L)
    nbytes = lib.asr_gram_kws_state_bytes(B, K, L)
    assert nbytes == 36 * B * K * L + 4 * B
    assert nbytes % 8 == (4 if B % 2 else 0)
    s = spot.KeywordStream(B, V, kws, device)
    assert s.state.numel() * s.state.element_size() >= nbytes, (s.state.numel(), nbytes)
    xs = ref.random_logits(T, B, V, 80 + B)
    want = _detect(device, xs, None, kws)
    parts = [s.advance(_t(device, xs[a:a + 5])) for a in range(0, T, 5)]
    for i, name in enumerate(spot.Detection._fields):
        got = torch.cat([p[i] for p in parts], -1).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want[i])), name
    # (b) through the C ABI, the state at the front of a poisoned buffer (torch allocations are 256-byte aligned)
    guard = 1024
    buf = torch.full((nbytes + guard,), 0x5A, dtype=torch.uint8, device=device)
    img, p = kws.image, _lib.ptr
    x = _t(device, xs[:7])
    det = torch.empty((B, K, 7), dtype=torch.float32, device=device)
    st = torch.empty((B, K, 7), dtype=torch.int32, device=device)
    fill = torch.empty((B, 7), dtype=torch.float32, device=device)
    n = lib.asr_kws_workspace_bytes(7, B, kws.U)
    ws = torch.empty(n, dtype=torch.uint8, device=device)
    assert lib.asr_gram_kws_state_reset(_lib.stream(), p(buf), B, K, L, None) == 0
    for _ in range(2):
        assert lib.asr_gram_kws_detect(_lib.stream(), p(x), None, 7, B, V, 0, p(img["uniq"]), kws.U, p(img["node_uni"]),
                                       p(img["node_big"]), p(img["kw_len"]), K, L, p(buf), p(det), p(st), p(fill), p(ws), n) == 0
    torch.cuda.synchronize()
    tail = buf[nbytes:].cpu().numpy()
    assert np.all(tail == 0x5A), "%d bytes behind the state were written" % int((tail != 0x5A).sum())
    counters = buf[nbytes - 4 * B:nbytes].cpu().numpy().view(np.int32)
    assert list(counters) == [14] * B                                # the frame counters are the last words of the state


# ------------------------------------------------------------------------------------------------ 5. full size
def test_full_size(device):
    """B = 4, T = 1000, V = 3000 (118 characters, 2881 bigrams), K = 64 phrases of 2 to 16 characters: two utterances of random
    logits, two peaked with planted phrases in a random mix of tokens"""
    B, T, V, K = 4, 1000, 3000, 64
    gram = gref.big_table(118, V, seed=3)
    phrases = gref.random_strings(K, 118, 2, 16, 1)
    xs = ref.random_logits(T, B, V, 2, scale=2.0)
    plants = []
    for b in (2, 3):
        ks = list(range(b, K, 4))
        path, spans, _ = gref.planted(T, [phrases[k] for k in ks], gram, seed=b)
        xs[:, b] = ref.peaked(path, V, seed=b)
        plants.append([(ks[i], s, e) for i, s, e in spans])
    lengths = [T, 777, T, 900]
    got, _ = check(device, xs, lengths, phrases, gram, "full size", max_hits=4)
    for b, spans in zip((2, 3), plants):
        for k, s, e in spans:
            if e <= lengths[b]:
                assert got["hit_score"][b, k, 0] == 0.0 and got["hit_start"][b, k, 0] == s and got["hit_end"][b, k, 0] == e, (b, k)
