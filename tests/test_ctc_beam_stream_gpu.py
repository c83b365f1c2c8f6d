"""Streaming CTC beam search on the GPU (asr.error.BeamStream, asr_ctc_beam_stream_* of csrc/ctc_beam.hip) against the one-shot
entries asr.error.beam_decode / beam_decode_lm / beam_decode_biased, which the existing tests hold to their float64 restatements.

Every comparison is on bytes, dtype included: the stream runs the same f32 operations in the same order as the one-shot kernel,
so for any cutting of the frames into chunks the outputs are identical, and a difference is a bug in the carry-over.  The helpers
are those of tests/test_ctc_beam_gpu.py, tests/test_ctc_beam_lm_gpu.py and tests/test_ctx_bias_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as lmref
import ctx_bias_reference as cref
import test_ctc_beam_gpu as base
import test_ctc_beam_lm_gpu as lmbase
import test_ctx_bias_gpu as bbase
from test_ctx_bias_gpu import ALPHA, BETA, ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

VARIANTS = ["plain", "lm", "graph", "lm_graph"]
SHAPES = [(1, 3, 5, 8, 4, 0, 11), (20, 3, 6, 1, 5, 0, 12), (20, 3, 6, 4, 1, 0, 13), (15, 3, 6, 8, 5, 3, 14), (2, 2, 3, 16, 2, 0, 15),
          (12, 2, 9, 8, 64, 0, 16), (30, 2, 80, 128, 32, 0, 17), (30, 2, 80, 64, 64, 0, 18)]


def pick(variant, model, graph):
    return (model if "lm" in variant else None), (graph if "graph" in variant else None)


def oneshot(device, x, model, graph, W, K, blank=0, lengths=None, use_eos=True):
    """the one-shot function of the variant -> its tuple of numpy arrays"""
    if graph is not None:
        a, b = (ALPHA, BETA) if model is not None else (0.0, 0.0)
        return bbase.biased(device, x, graph, model, a, b, W, K, blank, lengths, None, use_eos)
    if model is not None:
        return lmbase.fused(device, x, model, ALPHA, BETA, W, K, blank, lengths, None, use_eos)
    return base.beam(device, x, W, K, blank, lengths)


def open_stream(device, B, V, F, W, K, blank, model, graph):
    from asr import error
    a, b = (ALPHA, BETA) if model is not None else (0.0, 0.0)
    return error.BeamStream(B, V, F, W, K, blank, None, model, a, b, graph, device)


def fetch(s, use_eos=True):
    out = s.result(use_eos)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def same(got, want, T=None, rows=None):
    """the stream's tuple against the one-shot tuple, byte for byte, the stream's ids cut to the one-shot width T"""
    assert len(got) == len(want)
    for k, (u, v) in enumerate(zip(got, want)):
        if k == 0:
            u = u[:, :, :v.shape[2] if T is None else T]
        if rows is not None:
            u, v = u[rows], v[rows]
        u = np.ascontiguousarray(u)
        v = np.ascontiguousarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape, (k, u.dtype, v.dtype, u.shape, v.shape)
        assert u.tobytes() == v.tobytes(), (k, u, v)


def cuttings(T, seed):
    """one chunk; one frame per chunk; two seeded random cuttings"""
    out = [[T], [1] * T]
    for s in (seed, seed + 1000):
        rs = np.random.RandomState(s)
        cuts = sorted(set(rs.randint(1, T, size=max(1, T // 4)).tolist())) if T > 1 else []
        edges = [0] + cuts + [T]
        out.append([b - a for a, b in zip(edges, edges[1:])])
    assert all(sum(c) == T and min(c) >= 1 for c in out)
    return out


def feed(s, device, x, cuts, totals=None):
    """x (T, B, V) numpy into the stream in chunks of cuts[k] frames; totals (B): the frames of every utterance (None: all)"""
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    t = 0
    for c in cuts:
        lt = None
        if totals is not None:
            lt = torch.from_numpy(np.clip(np.asarray(totals) - t, 0, c).astype(np.int32)).to(device)
        s.advance(xt[t:t + c], lt)
        t += c
    return t


@functools.lru_cache(maxsize=None)
def setup(T, B, V, W, K, blank, seed):
    """logits, a random order-4 model as check_neutral builds it, and a graph of random phrases of 2-4 tokens"""
    x = base.small(T, B, V, seed)
    rs = np.random.RandomState(seed)
    ng = lmref.random_model(rs, V, 4, [rs.randint(0, V, size=6).tolist() for _ in range(8)], n_random=300)
    model = lmbase.make_lm(ng, V)
    n = V - 1
    phrases = cref.random_phrases(rs, V, min(30, (n ** 2 + n ** 3 + n ** 4) // 2), 2, 4, blank=blank)
    weights = rs.choice([0.5, 1.0, 2.0], size=len(phrases)).tolist()
    return x, model, bbase.make_graph(phrases, V, weights, blank=blank)


# ------------------------------------------------------------------------------------------------ 1. chunking invariance
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_B%d_V%d_W%d_K%d_b%d" % s[:6])
def test_chunking_invariance_on_the_edge_shapes(device, shape, variant):
    T, B, V, W, K, blank, seed = shape
    x, model, graph = setup(*shape)
    model, graph = pick(variant, model, graph)
    want = oneshot(device, x, model, graph, W, K, blank)
    for cuts in cuttings(T, seed):
        s = open_stream(device, B, V, T, W, K, blank, model, graph)
        assert feed(s, device, x, cuts) == T
        got = fetch(s)
        assert got[0].shape == (B, W, T)
        same(got, want)
        assert s.frames.cpu().tolist() == [T] * B


# ------------------------------------------------------------------------------------------------ 2. prefix property
@pytest.mark.parametrize("variant", VARIANTS)
def test_result_after_every_chunk_is_the_decode_of_the_frames_so_far(device, variant):
    shape = (20, 3, 6, 4, 5, 0, 41)
    T, B, V, W, K, blank, _ = shape
    x, model, graph = setup(*shape)
    model, graph = pick(variant, model, graph)
    xt = torch.from_numpy(x).to(device)
    s = open_stream(device, B, V, T, W, K, blank, model, graph)
    for t0 in range(0, T, 3):
        t1 = min(T, t0 + 3)
        s.advance(xt[t0:t1])
        for use_eos in (True, False):
            got = fetch(s, use_eos)
            again = fetch(s, use_eos)                     # result does not change the state
            same(again, got)
            assert got[0].shape == (B, W, t1)
            same(got, oneshot(device, x[:t1], model, graph, W, K, blank, None, use_eos))
    same(fetch(s), oneshot(device, x, model, graph, W, K, blank))


# ------------------------------------------------------------------------------------------------ 3. ragged batches
def gather_chunks(x, totals, delay, size):
    """chunks of `size` frames in which utterance b's frames start `delay[b]` chunks late: [(chunk (Tc, B, V), lengths (B))],
    every chunk assembled by a gather from x and filled with NaN past its lengths"""
    T, B, V = x.shape
    n = max(int(np.ceil(totals[b] / size)) + delay[b] for b in range(B))
    out = []
    for k in range(n):
        start = np.array([(k - delay[b]) * size for b in range(B)])
        lens = np.array([0 if k < delay[b] else np.clip(totals[b] - start[b], 0, size) for b in range(B)], np.int32)
        Tc = max(1, int(lens.max()))
        idx = np.clip(start[None, :] + np.arange(Tc)[:, None], 0, T - 1)          # (Tc, B)
        chunk = x[idx, np.arange(B)[None, :]].copy()
        chunk[np.arange(Tc)[:, None] >= lens[None, :]] = np.nan
        out.append((chunk, lens))
    return out


@pytest.mark.parametrize("delay", [(0, 0, 0, 0), (0, 0, 1, 0)], ids=["aligned", "staggered"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_ragged_batches_and_padding_is_never_read(device, variant, delay):
    T, B, V, W, K = 24, 4, 12, 8, 6
    x, model, graph = setup(T, B, V, W, K, 0, 21)
    assert np.array_equal(x, base.small(24, 4, 12, 21))
    model, graph = pick(variant, model, graph)
    totals = np.array([24, 0, 13, 1], np.int32)
    want = oneshot(device, x, model, graph, W, K, 0, totals)
    chunks = gather_chunks(x, totals, delay, 5)
    assert len(chunks) == 5 and (delay[2] == 0 or chunks[0][1][2] == 0)
    s = open_stream(device, B, V, sum(c.shape[0] for c, _ in chunks), W, K, 0, model, graph)
    for chunk, lens in chunks:
        s.advance(torch.from_numpy(chunk).to(device), torch.from_numpy(lens).to(device))
    got = fetch(s)
    same(got, want, T)
    assert np.all(got[0][:, :, T:] == 0)
    assert got[1][1, 0] == 0 and got[2][1, 0] == want[2][1, 0] and np.all(got[2][1, 1:] == -np.inf)
    assert s.frames.cpu().tolist() == totals.tolist()


# ------------------------------------------------------------------------------------------------ 4. pruned search
@pytest.fixture(scope="module")
def pruned():
    x, lengths, phrases, weights, plain = bbase.pruned_inputs()
    g = bbase.make_graph(phrases, bbase.V_P, weights)
    tr = [p[0][0] for p in plain]
    model = lmbase.make_lm(lmref.random_model(np.random.RandomState(20261021), bbase.V_P, 3, tr, n_random=20000), bbase.V_P)
    return dict(x=x, lengths=lengths, graph=g, model=model)


@pytest.mark.parametrize("variant", VARIANTS)
def test_pruned_search_across_chunk_boundaries(device, pruned, variant):
    """T = 160, V = 300, 400 phrases, an order-3 model, odd utterances ragged: beam entries are pruned and recreated across the
    boundaries, and the automaton and the model contexts are in mid-phrase at a boundary"""
    T, B, V, W, K = bbase.T_P, bbase.B_P, bbase.V_P, bbase.W_P, bbase.K_P
    x, lengths = pruned["x"], pruned["lengths"]
    model, graph = pick(variant, pruned["model"], pruned["graph"])
    want = oneshot(device, x, model, graph, W, K, 0, lengths)
    sevens = [7] * (T // 7) + ([T % 7] if T % 7 else [])
    for cuts in ([1] * T, sevens, [T], cuttings(T, 5)[2]):
        s = open_stream(device, B, V, T, W, K, 0, model, graph)
        feed(s, device, x, cuts, lengths)
        same(fetch(s), want)
        assert s.frames.cpu().tolist() == lengths.tolist()


# ------------------------------------------------------------------------------------------------ 5. slot reuse
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_partial_reset_starts_one_slot_over(device, variant):
    T, B, V, W, K = 20, 3, 8, 8, 5
    x, model, graph = setup(T, B, V, W, K, 0, 31)
    model, graph = pick(variant, model, graph)
    xt = torch.from_numpy(x).to(device)
    s = open_stream(device, B, V, T, W, K, 0, model, graph)
    s.advance(xt[:10])
    s.reset(mask=[0, 1, 0])
    s.advance(xt[10:])
    got = fetch(s)
    same(got, oneshot(device, x, model, graph, W, K, 0), rows=[0, 2])
    same(got, oneshot(device, x[10:], model, graph, W, K, 0), T=10, rows=[1])
    assert np.all(got[0][1, :, 10:] == 0)
    assert s.frames.cpu().tolist() == [20, 10, 20]


# ------------------------------------------------------------------------------------------------ 6. repeatability and bounds
def test_the_same_chunks_give_the_same_state_and_max_frames_does_not_matter(device):
    T, B, V, W, K = 20, 3, 8, 8, 5
    x, model, graph = setup(T, B, V, W, K, 0, 31)
    runs = []
    for F in (T, T, 2 * T):
        s = open_stream(device, B, V, F, W, K, 0, model, graph)
        feed(s, device, x, cuttings(T, 3)[2])
        out = fetch(s)
        runs.append((s.state.cpu().numpy().tobytes(), out))
    assert runs[0][0] == runs[1][0]
    same(runs[1][1], runs[0][1])
    same(runs[2][1], runs[0][1])
    same(runs[0][1], oneshot(device, x, model, graph, W, K, 0))


class Raw:
    """the stream entries through the raw ABI over buffers with a canary tail"""
    CANARY, TAIL = 0xA5, 4096

    def __init__(self, device, B, V, F, W, K, model=None, graph=None, alloc_W=None, alloc_Tc=None):
        from asr import _lib, _ops
        self.lib, self._lib, self._ops = _lib.lib(), _lib, _ops
        self.device, self.B, self.V, self.F, self.W, self.K = device, B, V, F, W, K
        self.model = None if model is None else model.to(device)
        self.graph = None if graph is None else graph.to(device)
        self.st_bytes = self.lib.asr_ctc_beam_stream_state_bytes(B, alloc_W or W, F, model is not None, graph is not None)
        self.ws_bytes = self.lib.asr_ctc_beam_stream_workspace_bytes(alloc_Tc or F, B, V, alloc_W or W, 64)
        assert self.st_bytes > 0 and self.ws_bytes > 0
        self.st = torch.full((self.st_bytes + self.TAIL,), self.CANARY, dtype=torch.uint8, device=device)
        self.ws = torch.full((self.ws_bytes + self.TAIL,), self.CANARY, dtype=torch.uint8, device=device)

    def lm_args(self, **over):
        if self.model is None:
            return [None, 0, None, None, 0, 0, 0]
        a = list(self._ops._lm_args(self.model.image))
        for k, name in enumerate(("uni", "vlm", "keys", "vals", "slots", "max_probe", "order")):
            if name in over:
                a[k] = over[name]
        return a

    def g_args(self, **over):
        if self.graph is None:
            return [None, None, 0, 0, None, 0]
        a = list(self._ops._graph_args(self.graph.image))
        for k, name in enumerate(("g_keys", "g_vals", "g_slots", "g_max_probe", "g_ret", "g_n_states")):
            if name in over:
                a[k] = over[name]
        return a

    def reset(self, W=None, mask=None):
        bos = -1 if self.model is None else self.model.bos_id
        return self.lib.asr_ctc_beam_stream_reset(self._lib.stream(), self._lib.ptr(self.st), self.st_bytes, self.B, W or self.W, self.F,
                                                  int(self.model is not None), int(self.graph is not None), bos, mask)

    def advance(self, x, fb, W=None, K=None, st_bytes=None, ws_bytes=None, logits=True, state=True, **over):
        Tc = x.shape[0]
        p = self._lib.ptr
        rc = self.lib.asr_ctc_beam_stream_advance(self._lib.stream(), p(x) if logits else None, None, Tc, self.B, self.V, 0, W or self.W,
                                                  K or self.K, float("-inf"), *self.lm_args(**over), *self.g_args(**over), ALPHA, BETA,
                                                  fb, self.F, p(self.st) if state else None,
                                                  self.st_bytes if st_bytes is None else st_bytes, p(self.ws),
                                                  self.ws_bytes if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        return rc

    def result(self, Lcap, W=None, st_bytes=None, eos=-1):
        W = W or self.W
        p = self._lib.ptr
        ids = torch.full((self.B * W * Lcap + 64,), -7, dtype=torch.int32, device=self.device)
        ln = torch.full((self.B, W), -7, dtype=torch.int32, device=self.device)
        sc, cc, lc, bc = (torch.full((self.B, W), 7.0, dtype=torch.float32, device=self.device) for _ in range(4))
        fr = torch.full((self.B,), -7, dtype=torch.int32, device=self.device)
        with_any = self.model is not None or self.graph is not None
        rc = self.lib.asr_ctc_beam_stream_result(self._lib.stream(), *self.lm_args(), *self.g_args(), ALPHA, BETA, eos, self.B, W,
                                                 self.F, 0, Lcap, p(self.st), self.st_bytes if st_bytes is None else st_bytes, p(ids),
                                                 p(ln), p(sc), p(cc) if with_any else None, p(lc) if with_any else None,
                                                 p(bc) if self.graph is not None else None, p(fr))
        torch.cuda.synchronize()
        ids = ids.cpu().numpy()
        assert np.all(ids[self.B * W * Lcap:] == -7)
        return rc, ids[:self.B * W * Lcap].reshape(self.B, W, Lcap), ln.cpu().numpy(), sc.cpu().numpy(), fr.cpu().numpy()

    def state_bytes(self):
        return self.st.cpu().numpy().tobytes()

    def canaries_intact(self):
        return bool((self.st[self.st_bytes:] == self.CANARY).all().item() and (self.ws[self.ws_bytes:] == self.CANARY).all().item())


@pytest.mark.parametrize("variant", ["plain", "lm_graph"])
def test_nothing_is_written_beyond_the_state_the_workspace_or_a_short_ids_row(device, variant):
    """exactly max_frames frames; the workspace is the size the query names for the chunk, the state the size it names for the
    stream, both followed by a canary; then a result with Lcap = 2 < the hypotheses' lengths"""
    T, B, V, W, K = 20, 3, 8, 8, 5
    x, model, graph = setup(T, B, V, W, K, 0, 31)
    model, graph = pick(variant, model, graph)
    xt = torch.from_numpy(x).to(device)
    r = Raw(device, B, V, T, W, K, model, graph, alloc_Tc=5)
    r.ws_bytes = r.lib.asr_ctc_beam_stream_workspace_bytes(5, B, V, W, K)
    r.ws = torch.full((r.ws_bytes + r.TAIL,), r.CANARY, dtype=torch.uint8, device=device)
    assert r.reset() == 0
    for t in range(0, T, 5):
        assert r.advance(xt[t:t + 5], t) == 0
    assert r.advance(xt[:1], T) == ASR_ERR_UNSUPPORTED
    want = oneshot(device, x, model, graph, W, K, 0, None, False)
    rc, ids, ln, sc, fr = r.result(T)
    assert rc == 0 and ids.tobytes() == want[0].tobytes() and ln.tobytes() == want[1].tobytes() and sc.tobytes() == want[2].tobytes()
    assert fr.tolist() == [T] * B and ln.max() > 2
    rc, ids2, ln2, sc2, _ = r.result(2)
    assert rc == 0 and np.array_equal(ids2, want[0][:, :, :2]) and ln2.tobytes() == want[1].tobytes() and sc2.tobytes() == sc.tobytes()
    assert r.canaries_intact()


# ------------------------------------------------------------------------------------------------ 7. limits and errors
def test_limits_errors_and_a_state_of_other_dimensions(device):
    V, B, F = 100, 2, 8
    rs = np.random.RandomState(3)
    g = bbase.make_graph(cref.random_phrases(rs, V, 50, 1, 4), V)
    model = lmbase.make_lm(lmref.random_model(rs, V, 3, n_random=500), V)
    x = torch.from_numpy(base.small(4, B, V, 5)).to(device)
    for m, gr in ((None, None), (model, None), (None, g), (model, g)):
        r = Raw(device, B, V, F, 16, 16, m, gr, alloc_W=129)
        assert r.reset() == 0 and r.advance(x, 0) == 0
        before = r.state_bytes()
        need = r.lib.asr_ctc_beam_stream_state_bytes(B, 16, F, int(m is not None), int(gr is not None))
        need_ws = r.lib.asr_ctc_beam_stream_workspace_bytes(4, B, V, 16, 16)
        assert r.advance(x, 4, st_bytes=need - 1) == ASR_ERR_WORKSPACE
        assert r.advance(x, 4, ws_bytes=need_ws - 1) == ASR_ERR_WORKSPACE
        assert r.result(8, st_bytes=need - 1)[0] == ASR_ERR_WORKSPACE
        assert r.advance(x, 5) == ASR_ERR_UNSUPPORTED                  # 5 + 4 > 8
        for W, K in ((129, 1), (1, 65), (65, 64), (128, 33)):
            assert r.advance(x, 4, W=W, K=K) == ASR_ERR_UNSUPPORTED, (W, K)
        assert r.advance(x, 4, logits=False) == ASR_ERR_BAD_ARG
        assert r.advance(x, 4, state=False) == ASR_ERR_BAD_ARG
        if gr is not None:
            assert r.advance(x, 4, g_n_states=0) == ASR_ERR_BAD_ARG
            assert r.advance(x, 4, g_ret=None) == ASR_ERR_BAD_ARG
            assert r.advance(x, 4, g_slots=12) == ASR_ERR_BAD_ARG
            assert r.advance(x, 4, g_max_probe=0) == ASR_ERR_BAD_ARG
        if m is not None:
            assert r.advance(x, 4, order=0) == ASR_ERR_BAD_ARG
            assert r.advance(x, 4, order=5) == ASR_ERR_UNSUPPORTED
            assert r.advance(x, 4, slots=12) == ASR_ERR_BAD_ARG
            assert r.advance(x, 4, max_probe=0) == ASR_ERR_BAD_ARG
            assert r.advance(x, 4, vlm=V - 1) == ASR_ERR_BAD_ARG
        assert r.state_bytes() == before and r.canaries_intact()
        assert r.advance(x, 4) == 0 and r.state_bytes() != before
        assert r.result(8)[4].tolist() == [8] * B
        # a state reset for beam_width 8, opened with beam_width 16 inside the same allocation
        assert r.reset(W=8) == 0
        before = r.state_bytes()
        assert r.advance(x, 0, W=16) == 0
        assert r.state_bytes() == before
        rc, ids, ln, sc, fr = r.result(8, W=16)
        assert rc == 0 and fr.tolist() == [-1] * B and np.all(ids == 0) and np.all(ln == 0) and np.all(sc == -np.inf)
        assert r.state_bytes() == before and r.canaries_intact()
        assert r.advance(x, 0, W=8, K=8) == 0 and r.result(8, W=8)[4].tolist() == [4] * B


# ------------------------------------------------------------------------------------------------ 8. the Python class
def test_the_class_refuses_wrong_chunks_graphs_and_overfeeding(device):
    from asr import error
    V = 9
    g = bbase.make_graph([(1, 2), (3, 4, 5)], V)
    with pytest.raises(ValueError):
        error.BeamStream(2, V + 1, 10, graph=g, device=device)
    with pytest.raises(ValueError):
        error.BeamStream(2, V, 10, blank=1, graph=g, device=device)
    s = error.BeamStream(2, V, 10, 4, 4, graph=g, device=device)
    x = torch.from_numpy(base.small(6, 2, V, 1)).to(device)
    with pytest.raises(ValueError):
        s.advance(x[:, :, :V - 1].contiguous())
    with pytest.raises(ValueError):
        s.advance(x[:, :1].contiguous())
    with pytest.raises(ValueError):
        s.advance(x, lengths=[1, 2, 3])
    with pytest.raises(ValueError):
        s.reset(mask=[1])
    s.advance(x)
    with pytest.raises(ValueError):
        s.advance(x)                                  # 6 + 6 > 10
    s.reset(mask=[1, 0])                              # a partial reset does not lower the host's count
    with pytest.raises(ValueError):
        s.advance(x)
    s.advance(x[:4])
    out = fetch(s)
    assert len(out) == 6 and out[0].shape == (2, 4, 10) and s.frames.cpu().tolist() == [4, 10]
    s.reset()
    assert s.fed == 0 and fetch(s)[0].shape == (2, 4, 0) and s.frames.cpu().tolist() == [0, 0]
    s.advance(x)
    same(fetch(s), bbase.biased(device, x.cpu().numpy(), g, None, 0.0, 0.0, 4, 4))
