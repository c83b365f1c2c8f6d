"""CTC keyword spotting on the GPU (csrc/ctc_kws.hip through asr.spot) against the float64 restatement of tests/keyword_reference.py
and the project's own aligner.

det (after the cast to f32), every det_start, every hit start / end / count and hit_score must equal the restatement exactly: both
sides run the same IEEE float64 max and one addition per step on the same f32 logits.  fill and hit_logp contain the row's
log-sum-exp (f32 on the device): 1e-4 * max(1, |value|), the project's CTC tolerance as tests/test_ctc_align_gpu.py uses it.  Every
test prints its worst error / tolerance.
"""
import numpy as np
import pytest
import torch

import keyword_reference as ref

from asr import spot

pytestmark = pytest.mark.gpu

RTOL = 1e-4
EXACT = ("det", "start", "hit_start", "hit_end", "n_hits", "hit_score")
POISON_I, POISON_F = 0x5A5A5A5A, 12345.5
G, TILE = spot.SWEEP_GROUP, spot.SWEEP_TILE


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


def run(device, xs, lengths, phrases, max_hits=4, min_score=None, blank=0):
    """numpy in -> dict of numpy arrays named as tests/keyword_reference.py: search names them, through the public functions"""
    kws = spot.KeywordSet(phrases, xs.shape[2], blank)
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


def check(device, xs, lengths, phrases, what, max_hits=4, min_score=None):
    want = ref.search(xs, lengths, phrases, 0, max_hits, -np.inf if min_score is None else min_score)
    got = run(device, xs, lengths, phrases, max_hits, min_score)
    compare(got, want, what)
    return got, want


# ------------------------------------------------------------------------------------------------ 1. shapes and dispatch edges
@pytest.mark.parametrize("L", [1, 2, 63, 64])
def test_keyword_lengths(device, L):
    """one long phrase planted in a peaked path and found with score exactly 0.0, beside its prefix and random logits"""
    V, T = 80, 300
    p = tuple(1 + (i * 7) % (V - 1) for i in range(L))
    path, spans = ref.planted(T, V, [p], seed=L)
    xs = np.stack([ref.peaked(path, V, seed=1), ref.random_logits(T, 1, V, 2)[:, 0]], 1)
    got, _ = check(device, xs, None, [p, p[:max(1, L // 2)]], "L = %d" % L, max_hits=2, min_score=-0.5)
    (_, s, e), = spans
    assert got["n_hits"][0, 0] == 1 and got["hit_start"][0, 0, 0] == s and got["hit_end"][0, 0, 0] == e
    assert got["hit_score"][0, 0, 0] == 0.0


@pytest.mark.parametrize("K", [1, G, G + 1, 2 * G + 1])
def test_keywords_per_workgroup(device, K):
    xs = ref.random_logits(TILE + 5, 2, 12, 10 + K)
    check(device, xs, [TILE + 5, 9], ref.random_phrases(K, 12, 1, 5, K), "K = %d" % K)


@pytest.mark.parametrize("T", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_frames_around_the_tile(device, T):
    xs = ref.random_logits(T, 3, 7, 20 + T)
    phrases = [(1,), (2, 3), (4, 4), (5, 6, 1), (1, 2, 3, 4, 5, 6, 1, 2, 3, 4)]
    check(device, xs, None, phrases, "T = %d" % T)
    check(device, xs, [T, max(T - 1, 0), T // 2], phrases, "T = %d, ragged" % T)


def test_keyword_longer_than_the_utterance(device):
    xs = ref.random_logits(12, 2, 9, 31)
    got, _ = check(device, xs, [5, 12], [(1, 2, 3, 4, 5, 6, 7, 8), (1, 2)], "keyword longer than xl")
    assert np.all(np.isneginf(got["det"][0, 0])) and got["n_hits"][0, 0] == 0 and got["n_hits"][1, 0] >= 1


@pytest.mark.parametrize("U", [63, 64, 65, 255, 256, 257])
def test_distinct_tokens(device, U):
    V = 300
    toks = list(range(1, U + 1))
    phrases = [tuple(toks[i:i + 8]) for i in range(0, U, 8)] + [(toks[-1], toks[0]), (toks[0], toks[-1], toks[U // 2])]
    assert spot.KeywordSet(phrases, V).U == U
    check(device, ref.random_logits(10, 2, V, U), None, phrases, "U = %d" % U)


@pytest.mark.parametrize("V", [3, 8, 9])
@pytest.mark.parametrize("B", [1, 3])
def test_row_paths_and_lengths(device, V, B):
    """V = 3 and 9: the scalar row loop, V = 8: float4; lengths 0, 1 and T"""
    T = 11
    xs = ref.random_logits(T, B, V, V * 10 + B)
    phrases = [(1, 2), (2,), (1, 1), (2, 1, 2)]
    lengths = [T] if B == 1 else [0, 1, T]
    got, _ = check(device, xs, lengths, phrases, "V = %d, B = %d" % (V, B))
    if B == 3:
        assert np.all(np.isneginf(got["det"][0])) and np.all(got["fill"][0] == 0) and np.all(got["n_hits"][0] == 0)
        assert np.all(np.isneginf(got["det"][1, :, 1:])) and np.all(got["start"][1, :, 1:] == -1)


def test_repeats_dead_duplicates_and_prefixes(device):
    """repeated tokens, dead keywords beside live ones, the same phrase twice (identical rows), one phrase a prefix of another"""
    V, T = 10, 40
    phrases = [(3, 3), (3, 3, 3), (1, 2, 3), (1, 2), (1, 2, 3), (), (4, V), (5, 0, 5), (-1,), (2, 2, 1, 1)]
    path, _ = ref.planted(T, V, [(3, 3, 3), (1, 2, 3), (2, 2, 1, 1)], seed=5)
    xs = np.stack([ref.peaked(path, V, seed=2), ref.random_logits(T, 1, V, 3)[:, 0]], 1)
    got, _ = check(device, xs, None, phrases, "repeats / dead / duplicates / prefixes")
    for k in (5, 6, 7, 8):
        assert np.all(np.isneginf(got["det"][:, k])) and np.all(got["start"][:, k] == -1) and np.all(got["n_hits"][:, k] == 0)
    for name in got:
        if name != "fill":
            assert np.array_equal(got[name][:, 2], got[name][:, 4]), name


# ------------------------------------------------------------------------------------------------ 2. hits
def planted_case(seed=7):
    V, T = 20, 120
    phrases = [(1, 2, 3), (4, 4), (5,), (6, 7, 8, 9), (1, 2)]
    order = [0, 1, 2, 0, 3, 1, 0]
    path, spans = ref.planted(T, V, [phrases[k] for k in order], seed)
    return V, T, phrases, [(order[i], s, e) for i, s, e in spans], ref.peaked(path, V, seed=seed)[:, None, :]


def test_planted_phrases_are_found_exactly(device):
    V, T, phrases, spans, xs = planted_case()
    got, _ = check(device, xs, None, phrases, "planted phrases", max_hits=5, min_score=-1.0)
    for k in range(4):
        mine = sorted((s, e) for kk, s, e in spans if kk == k)
        n = got["n_hits"][0, k]
        assert n == len(mine), (k, n, mine)
        found = sorted(zip(got["hit_start"][0, k, :n].tolist(), got["hit_end"][0, k, :n].tolist()))
        assert found == mine, (k, found, mine)
        assert np.all(got["hit_score"][0, k, :n] == 0.0)
        assert got["hit_start"][0, k, 0] == mine[0][0]               # equally good occurrences: the earlier first
    assert got["n_hits"][0, 4] == 3 and np.all(got["hit_score"][0, 4, :3] == 0.0)       # the prefix (1, 2) of every (1, 2, 3)


@pytest.mark.parametrize("max_hits,min_score", [(1, None), (2, -1.0), (8, -1.0), (8, None), (3, -30.0), (4, 1.0)])
def test_max_hits_and_min_score(device, max_hits, min_score):
    """max_hits = 1, max_hits above the occurrences (unused slots -1 / -inf), thresholds that cut the list or leave nothing"""
    V, T, phrases, spans, xs = planted_case()
    got, _ = check(device, xs, None, phrases, "max_hits = %d, min_score = %s" % (max_hits, min_score), max_hits, min_score)
    if min_score == -1.0 and max_hits == 8:
        assert list(got["n_hits"][0]) == [3, 2, 1, 1, 3]
        assert np.all(got["hit_start"][0, 2, 1:] == -1) and np.all(np.isneginf(got["hit_logp"][0, 2, 1:]))
    if min_score == 1.0:
        assert np.all(got["n_hits"] == 0)


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
    rc = lib.asr_kws_detect(_lib.stream(), p(x), p(h), T, B, V, kws.blank, p(img["uniq"]), kws.U, p(img["node_tok"]), p(img["kw_len"]),
                            K, kws.Lmax, None, p(o["det"]), p(o["start"]), p(o["fill"]), p(ws), n)
    assert rc == 0
    rc = lib.asr_kws_hits(_lib.stream(), p(o["det"]), p(o["start"]), p(o["fill"]), p(h), B, K, T, H, min_score, p(o["hit_start"]),
                          p(o["hit_end"]), p(o["hit_score"]), p(o["hit_logp"]), p(o["n_hits"]))
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_poisoned_outputs_are_overwritten(device):
    T, B, V = TILE + 3, 4, 8
    xs = ref.random_logits(T, B, V, 41)
    lengths = [0, 1, T, TILE]
    phrases = [(1, 2), (), (3,), (9, 1), (4, 5, 6, 7, 1, 2, 3)]
    got = _raw(device, xs, lengths, spot.KeywordSet(phrases, V), 3, -np.inf)
    compare(got, ref.search(xs, lengths, phrases, 0, 3), "poisoned outputs")
    for name, a in got.items():
        assert not np.any(a == (POISON_I if a.dtype == np.int32 else np.float32(POISON_F))), name


# ------------------------------------------------------------------------------------------------ 3. against existing code
def test_hits_against_the_aligner(device):
    """for every hit, the forced alignment of the keyword on logits[start:end] is compared with hit_logp.  The aligner also allows
    leading and trailing blanks, so its score is never below hit_logp.  For the first hit of a (b, k), and for every hit of score
    0.0, it cannot be above either: a path blank^a + (a tight path on [s + a, e - b]) + blank^b is worth at most det[e - b] <= det[e],
    the maximum over every end and start.  There the two must agree within the tolerance."""
    from asr.loss import ctc_align
    V, T = 16, 70
    phrases = [(1, 2, 3), (4, 4), (5,), (2, 3)]
    path, _ = ref.planted(T, V, [phrases[0], phrases[1], phrases[2], phrases[0]], seed=11)
    xs = np.stack([ref.peaked(path, V, seed=3, peak=4.0), ref.random_logits(T, 1, V, 4, scale=1.5)[:, 0]], 1)
    got, _ = check(device, xs, None, phrases, "aligner cross-check: the search itself", max_hits=3)
    segs, labels, lens, want, tight = [], [], [], [], []
    for b in range(2):
        for k, p in enumerate(phrases):
            for h in range(got["n_hits"][b, k]):
                s, e = got["hit_start"][b, k, h], got["hit_end"][b, k, h]
                segs.append(xs[s:e, b])
                labels.append(p)
                lens.append(e - s)
                want.append(got["hit_logp"][b, k, h])
                tight.append(h == 0 or got["hit_score"][b, k, h] == 0.0)
    assert len(segs) >= 8 and sum(tight) >= 8
    x = np.zeros((max(lens), len(segs), V), np.float32)
    t = np.zeros((len(segs), 3), np.int32)
    for i, (seg, p) in enumerate(zip(segs, labels)):
        x[:len(seg), i] = seg
        t[i, :len(p)] = p
    a = ctc_align(_t(device, x), _t(device, t), 0, _t(device, lens, np.int32), _t(device, [len(p) for p in labels], np.int32))
    torch.cuda.synchronize()
    score, want, tight = a.score.cpu().numpy().astype(np.float64), np.asarray(want, np.float64), np.asarray(tight)
    tol = RTOL * np.maximum(1.0, np.abs(want))
    r = float((np.abs(score - want) / tol)[tight].max())
    low = float(((want - score) / tol).max())
    print("hit_logp against ctc_align on the hit's frames, %d hits (%d tight): worst error / tolerance = %.3g, worst shortfall of "
          "the aligner / tolerance = %.3g" % (len(segs), tight.sum(), r, low))
    assert r <= 1.0 and low <= 1.0


# ------------------------------------------------------------------------------------------------ 4. streaming
def _one_shot(device, xs, lengths, kws):
    d = spot.keyword_detect(_t(device, xs, np.float32), kws, None if lengths is None else _t(device, lengths, np.int32))
    return [v.cpu().numpy() for v in d]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("chunk", [1, 7, TILE - 1, TILE, TILE + 1])
def test_stream_equals_one_shot(device, chunk):
    """full-length chunks: the chunk outputs concatenated along T are bit for bit the one-shot result and go into keyword_hits"""
    T, B, V = 2 * TILE + 9, 2, 9
    xs = ref.random_logits(T, B, V, 50 + chunk)
    phrases = [(1, 2), (3, 3), (4,), (5, 6, 7, 8, 1), (2, 1)]
    kws = spot.KeywordSet(phrases, V)
    want = _one_shot(device, xs, None, kws)
    s = spot.KeywordStream(B, V, kws, device)
    parts = [s.advance(_t(device, xs[a:a + chunk])) for a in range(0, T, chunk)]
    got = [torch.cat([p[i] for p in parts], -1) for i in range(3)]
    for name, g, w in zip(spot.Detection._fields, got, want):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w)), name
    hits = spot.keyword_hits(spot.Detection(*got), None, 3)
    full = spot.keyword_hits(spot.Detection(*[_t(device, w) for w in want]), None, 3)
    for a, b in zip(hits, full):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    compare(run(device, xs, None, phrases, 3), ref.search(xs, None, phrases, 0, 3), "stream, chunks of %d: the one-shot side" % chunk)


def test_stream_ragged_chunks_and_reset(device):
    """ragged lengths including 0: each utterance's outputs over its valid frames, in order, are the one-shot result of the frames
    it was fed; frames past a chunk's length hold -inf / -1 / 0; reset(mask) restarts only the masked utterances"""
    B, V, Tc = 3, 9, TILE + 2
    phrases = [(1, 2), (3, 3), (4,), (5, 6, 7), (2, 1, 2, 1)]
    kws = spot.KeywordSet(phrases, V)
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
        want = _one_shot(device, fed[:, None, :], None, kws)
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


@pytest.mark.parametrize("B,K,L", [(1, 64, 16), (3, 5, 7), (2, 5, 7)])
def test_stream_state_is_large_enough_and_not_overrun(device, B, K, L):
    """the state is 24 B K Lmax + 4 B bytes: for odd B not a whole number of 8-byte words, and the frame counters are its last
    words.  B = 1, K = 64, Lmax = 16 is 24580 bytes: cut to whole words it would be 24576 = 48 * 512, and the only frame counter
    would lie in whatever the allocator placed next.  (a) KeywordStream allocates at least the bytes the library names; (b) reset
    and advance, given exactly those bytes inside a poisoned buffer, touch nothing behind them; (c) the stream equals one shot."""
    from asr import _lib
    lib = _lib.lib()
    V, T = 40, TILE + 3
    phrases = ref.random_phrases(K - 1, V, 1, L, B * 100 + K) + [tuple(range(1, L + 1))]
    kws = spot.KeywordSet(phrases, V).to(device)
    assert (kws.K, kws.Lmax) == (K, L)
    nbytes = lib.asr_kws_state_bytes(B, K, L)
    assert nbytes == 24 * B * K * L + 4 * B
    if (B, K, L) == (1, 64, 16):
        assert nbytes % 8 == 4 and (nbytes // 8 * 8) % 512 == 0
    s = spot.KeywordStream(B, V, kws, device)
    assert s.state.numel() * s.state.element_size() >= nbytes, (s.state.numel(), nbytes)
    xs = ref.random_logits(T, B, V, 80 + B)
    want = _one_shot(device, xs, None, kws)
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
    assert lib.asr_kws_state_reset(_lib.stream(), p(buf), B, K, L, None) == 0
    for _ in range(2):
        assert lib.asr_kws_detect(_lib.stream(), p(x), None, 7, B, V, 0, p(img["uniq"]), kws.U, p(img["node_tok"]), p(img["kw_len"]),
                                  K, L, p(buf), p(det), p(st), p(fill), p(ws), n) == 0
    torch.cuda.synchronize()
    tail = buf[nbytes:].cpu().numpy()
    assert np.all(tail == 0x5A), "%d bytes behind the state were written" % int((tail != 0x5A).sum())
    counters = buf[nbytes - 4 * B:nbytes].cpu().numpy().view(np.int32)
    assert list(counters) == [14] * B                                # the frame counters are the last words of the state


# ------------------------------------------------------------------------------------------------ 5. full size
def test_full_size(device):
    """B = 4, T = 1000, V = 3000, K = 64 phrases of 2 to 16 tokens: two utterances of random logits, two peaked with planted phrases"""
    B, T, V, K = 4, 1000, 3000, 64
    phrases = ref.random_phrases(K, V, 2, 16, 1)
    xs = ref.random_logits(T, B, V, 2, scale=2.0)
    planted = []
    for b in (2, 3):
        path, spans = ref.planted(T, V, [phrases[k] for k in range(b, K, 4)], seed=b)
        xs[:, b] = ref.peaked(path, V, seed=b)
        planted.append([(range(b, K, 4)[i], s, e) for i, s, e in spans])
    lengths = [T, 777, T, 900]
    got, _ = check(device, xs, lengths, phrases, "full size", max_hits=4)
    for b, spans in zip((2, 3), planted):
        for k, s, e in spans:
            if e <= lengths[b]:
                assert got["hit_score"][b, k, 0] == 0.0 and got["hit_start"][b, k, 0] == s and got["hit_end"][b, k, 0] == e, (b, k)
