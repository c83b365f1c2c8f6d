"""Streaming Gram-CTC beam search on the GPU (asr.error.GramBeamStream, asr_gram_ctc_beam_stream_* of csrc/ctc_beam.hip) against the
one-shot entries asr.error.gram_beam_decode / gram_beam_decode_lm, which tests/test_gram_beam_gpu.py and
tests/test_gram_beam_lm_gpu.py hold to their float64 restatements.

Every comparison is on bytes, dtype included: the stream runs the same f32 operations in the same order as the one-shot kernel,
so for any cutting of the frames into chunks the outputs are identical, and a difference is a bug in the carry-over.  The helpers
are those of the one-shot tests and of tests/test_ctc_beam_stream_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as lmref
import gram_beam_lm_reference as glm
import gram_beam_reference as gref
import test_ctc_beam_gpu as base
from test_ctc_beam_stream_gpu import cuttings, feed, fetch, gather_chunks, same
from test_gram_beam_gpu import gbeam
from test_gram_beam_lm_gpu import ALPHA, BETA, ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED, SEED_P, edge_model, gfused, make_lm

pytestmark = pytest.mark.gpu

VARIANTS = ["plain", "lm"]
# T, B, V, U, W, K, blank, seed: the nine of tests/test_gram_beam_gpu.py::test_edge_cases_against_restatement
SHAPES = [(1, 3, 8, 3, 8, 4, 0, 11), (20, 3, 9, 3, 1, 5, 0, 12), (20, 3, 9, 3, 4, 1, 0, 13), (15, 3, 9, 3, 8, 5, 3, 14),
          (12, 2, 9, 3, 8, 64, 0, 16), (30, 2, 80, 10, 128, 32, 0, 17), (30, 2, 80, 10, 64, 64, 0, 18), (30, 2, 80, 10, 128, 1, 0, 19),
          (30, 2, 80, 10, 1, 64, 0, 20)]


def oneshot(device, x, gram, model, W, K, blank=0, lengths=None, use_eos=True):
    """the one-shot function of the variant -> its tuple of numpy arrays"""
    if model is not None:
        return gfused(device, x, gram, model, ALPHA, BETA, W, K, blank, lengths, None, use_eos)
    return gbeam(device, x, gram, W, K, blank, lengths)


def open_stream(device, B, V, F, gram, W, K, blank, model):
    from asr import error
    a, b = (ALPHA, BETA) if model is not None else (0.0, 0.0)
    return error.GramBeamStream(B, V, F, gram, W, K, blank, None, model, a, b, device)


@functools.lru_cache(maxsize=None)
def setup(T, B, V, U, W, K, blank, seed):
    """logits, a random table with U unigrams and a random order-4 character model over the ids of V tokens"""
    return base.small(T, B, V, seed), gref.random_table(V, U, seed, blank), edge_model(V, 4, seed)


def both_ways(device, x, gram, model, W, K, blank=0):
    """x fed as a whole and frame by frame -> the one-shot tuple, which both equal"""
    T, B, V = x.shape
    want = oneshot(device, x, gram, model, W, K, blank)
    for cuts in ([T], [1] * T):
        s = open_stream(device, B, V, T, gram, W, K, blank, model)
        assert feed(s, device, x, cuts) == T
        got = fetch(s)
        assert got[0].shape == (B, W, 2 * T)
        same(got, want)
        assert s.frames.cpu().tolist() == [T] * B
    return want


# ------------------------------------------------------------------------------------------------ 1. chunking invariance
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_B%d_V%d_U%d_W%d_K%d_b%d" % s[:7])
def test_chunking_invariance_on_the_edge_shapes(device, shape, variant):
    T, B, V, U, W, K, blank, seed = shape
    x, gram, model = setup(*shape)
    model = model if variant == "lm" else None
    want = oneshot(device, x, gram, model, W, K, blank)
    for cuts in cuttings(T, seed):
        s = open_stream(device, B, V, T, gram, W, K, blank, model)
        assert feed(s, device, x, cuts) == T
        got = fetch(s)
        assert got[0].shape == (B, W, 2 * T)
        same(got, want)
        assert s.frames.cpu().tolist() == [T] * B


# ------------------------------------------------------------------------------------------------ 2. prefix property
@pytest.mark.parametrize("variant", VARIANTS)
def test_result_after_every_chunk_is_the_decode_of_the_frames_so_far(device, variant):
    shape = (20, 3, 9, 3, 4, 5, 0, 41)
    T, B, V, U, W, K, blank, _ = shape
    x, gram, model = setup(*shape)
    model = model if variant == "lm" else None
    xt = torch.from_numpy(x).to(device)
    s = open_stream(device, B, V, T, gram, W, K, blank, model)
    for t0 in range(0, T, 3):
        t1 = min(T, t0 + 3)
        s.advance(xt[t0:t1])
        for use_eos in (True, False):
            got = fetch(s, use_eos)
            again = fetch(s, use_eos)                     # result does not change the state
            same(again, got)
            assert got[0].shape == (B, W, 2 * t1)
            same(got, oneshot(device, x[:t1], gram, model, W, K, blank, None, use_eos))
    same(fetch(s), oneshot(device, x, gram, model, W, K, blank))


# ------------------------------------------------------------------------------------------------ 3. ragged batches
@pytest.mark.parametrize("delay", [(0, 0, 0, 0), (0, 0, 1, 0)], ids=["aligned", "staggered"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_ragged_batches_and_padding_is_never_read(device, variant, delay):
    T, B, V, U, W, K = 24, 4, 12, 4, 8, 6
    x, gram, model = setup(T, B, V, U, W, K, 0, 21)
    model = model if variant == "lm" else None
    totals = np.array([24, 0, 13, 1], np.int32)
    want = oneshot(device, x, gram, model, W, K, 0, totals)
    chunks = gather_chunks(x, totals, delay, 5)
    assert len(chunks) == 5 and (delay[2] == 0 or chunks[0][1][2] == 0)
    assert all(np.isnan(c[n:, b]).all() for c, ln in chunks for b, n in enumerate(ln))
    F = sum(c.shape[0] for c, _ in chunks)
    s = open_stream(device, B, V, F, gram, W, K, 0, model)
    for chunk, lens in chunks:
        s.advance(torch.from_numpy(chunk).to(device), torch.from_numpy(lens).to(device))
    got = fetch(s)
    assert got[0].shape == (B, W, 2 * F)
    same(got, want, 2 * T)
    assert np.all(got[0][:, :, 2 * T:] == 0)
    assert got[1][1, 0] == 0 and got[2][1, 0] == want[2][1, 0] and np.all(got[2][1, 1:] == -np.inf)
    assert s.frames.cpu().tolist() == totals.tolist()


# ------------------------------------------------------------------------------------------------ 4. pruned search
@pytest.fixture(scope="module")
def pruned():
    """gref.pruned_inputs() and the order-3 model of tests/test_gram_beam_lm_gpu.py::pruned, built the same way"""
    gram, x, lengths = gref.pruned_inputs()
    V = len(gram)
    top1 = [gref.beam_search(x[:, b], gram, gref.W_P, gref.K_P)[0][0] for b in range(gref.B_P)]
    ng = lmref.random_model(np.random.RandomState(SEED_P), gref.U_P + 1, 3, top1, n_random=300)
    return dict(gram=gram, x=x, lengths=lengths, model=make_lm(glm.relabel_marks(ng, gref.U_P + 1, V), V))


@pytest.mark.parametrize("variant", VARIANTS)
def test_pruned_search_across_chunk_boundaries(device, pruned, variant):
    """T = 160, B = 8, V = 171 (20 unigrams, 150 bigrams), beam 16, top_k 16: strings are pruned, recreated and merged across
    the boundaries, a frame's pair of extensions that spell one string (mt[]) meets a string carried over the boundary, and the
    model contexts are the carried strings' last characters.  The full run in four cuttings, the ragged one in sevens."""
    T, B, W, K = gref.T_P, gref.B_P, gref.W_P, gref.K_P
    gram, x, lengths = pruned["gram"], pruned["x"], pruned["lengths"]
    V = len(gram)
    assert x.shape == (160, 8, 171) and (W, K) == (16, 16)
    model = pruned["model"] if variant == "lm" else None
    want = oneshot(device, x, gram, model, W, K, 0)
    assert want[1][:, 0].min() > 2                       # real strings; some of them cut into bigram tokens
    sevens = [7] * (T // 7) + ([T % 7] if T % 7 else [])
    for cuts in ([1] * T, sevens, [T], cuttings(T, 5)[2]):
        s = open_stream(device, B, V, T, gram, W, K, 0, model)
        feed(s, device, x, cuts)
        same(fetch(s), want)
        assert s.frames.cpu().tolist() == [T] * B
    s = open_stream(device, B, V, T, gram, W, K, 0, model)
    feed(s, device, x, sevens, lengths)
    same(fetch(s), oneshot(device, x, gram, model, W, K, 0, lengths))
    assert s.frames.cpu().tolist() == lengths.tolist()


# ------------------------------------------------------------------------------------------------ 5. what only Gram-CTC has
class Raw:
    """the stream entries through the raw ABI over buffers with a canary tail"""
    CANARY, TAIL = 0xA5, 4096

    def __init__(self, device, B, V, F, W, K, gram, model=None, alloc_W=None, alloc_Tc=None):
        from asr import _lib, _ops
        self.lib, self._lib, self._ops = _lib.lib(), _lib, _ops
        self.device, self.B, self.V, self.F, self.W, self.K = device, B, V, F, W, K
        self.gram = torch.from_numpy(np.ascontiguousarray(gram, np.int32)).to(device)
        self.model = None if model is None else model.to(device)
        self.st_bytes = self.lib.asr_gram_ctc_beam_stream_state_bytes(B, alloc_W or W, F, model is not None)
        self.ws_bytes = self.lib.asr_gram_ctc_beam_stream_workspace_bytes(alloc_Tc or F, B, V, W, K if alloc_Tc else 64)
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

    def bos(self):
        return -1 if self.model is None else self.model.bos_id

    def reset(self, W=None, mask=None):
        return self.lib.asr_gram_ctc_beam_stream_reset(self._lib.stream(), self._lib.ptr(self.st), self.st_bytes, self.B, W or self.W,
                                                       self.F, int(self.model is not None), mask)

    def advance(self, x, fb, W=None, K=None, st_bytes=None, ws_bytes=None, logits=True, state=True, gram=True, bos=None, **over):
        Tc = x.shape[0]
        p = self._lib.ptr
        rc = self.lib.asr_gram_ctc_beam_stream_advance(self._lib.stream(), p(x) if logits else None, None, Tc, self.B, self.V, 0,
                                                       W or self.W, K or self.K, float("-inf"), p(self.gram) if gram else None,
                                                       *self.lm_args(**over), self.bos() if bos is None else bos, ALPHA, BETA, fb,
                                                       self.F, p(self.st) if state else None,
                                                       self.st_bytes if st_bytes is None else st_bytes, p(self.ws),
                                                       self.ws_bytes if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        return rc

    def result(self, Lcap, W=None, st_bytes=None, eos=-1):
        W = W or self.W
        p = self._lib.ptr
        ids = torch.full((self.B * W * Lcap + 64,), -7, dtype=torch.int32, device=self.device)
        ln = torch.full((self.B, W), -7, dtype=torch.int32, device=self.device)
        sc, cc, lc = (torch.full((self.B, W), 7.0, dtype=torch.float32, device=self.device) for _ in range(3))
        fr = torch.full((self.B,), -7, dtype=torch.int32, device=self.device)
        with_lm = self.model is not None
        rc = self.lib.asr_gram_ctc_beam_stream_result(self._lib.stream(), *self.lm_args(), self.bos(), eos, ALPHA, BETA, self.B, W,
                                                      self.F, 0, Lcap, p(self.st), self.st_bytes if st_bytes is None else st_bytes,
                                                      p(ids), p(ln), p(sc), p(cc) if with_lm else None, p(lc) if with_lm else None,
                                                      p(fr))
        torch.cuda.synchronize()
        ids = ids.cpu().numpy()
        assert np.all(ids[self.B * W * Lcap:] == -7)
        return rc, ids[:self.B * W * Lcap].reshape(self.B, W, Lcap), ln.cpu().numpy(), sc.cpu().numpy(), fr.cpu().numpy()

    # the CTC stream's entries of the same variant on the same buffers
    def ctc_reset(self, W=None):
        return self.lib.asr_ctc_beam_stream_reset(self._lib.stream(), self._lib.ptr(self.st), self.st_bytes, self.B, W or self.W, self.F,
                                                  int(self.model is not None), 0, self.bos(), None)

    def ctc_advance(self, x, fb):
        p = self._lib.ptr
        rc = self.lib.asr_ctc_beam_stream_advance(self._lib.stream(), p(x), None, x.shape[0], self.B, self.V, 0, self.W, self.K,
                                                  float("-inf"), *self.lm_args(), None, None, 0, 0, None, 0, ALPHA, BETA, fb, self.F,
                                                  p(self.st), self.st_bytes, p(self.ws), self.ws_bytes)
        torch.cuda.synchronize()
        return rc

    def ctc_result(self, Lcap):
        p = self._lib.ptr
        ids = torch.full((self.B, self.W, Lcap), -7, dtype=torch.int32, device=self.device)
        ln = torch.full((self.B, self.W), -7, dtype=torch.int32, device=self.device)
        sc, cc, lc = (torch.full((self.B, self.W), 7.0, dtype=torch.float32, device=self.device) for _ in range(3))
        fr = torch.full((self.B,), -7, dtype=torch.int32, device=self.device)
        with_lm = self.model is not None
        rc = self.lib.asr_ctc_beam_stream_result(self._lib.stream(), *self.lm_args(), None, None, 0, 0, None, 0, ALPHA, BETA, -1, self.B,
                                                 self.W, self.F, 0, Lcap, p(self.st), self.st_bytes, p(ids), p(ln), p(sc),
                                                 p(cc) if with_lm else None, p(lc) if with_lm else None, None, p(fr))
        torch.cuda.synchronize()
        return rc, ids.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy(), fr.cpu().numpy()

    def state_bytes(self):
        return self.st.cpu().numpy().tobytes()

    def canaries_intact(self):
        return bool((self.st[self.st_bytes:] == self.CANARY).all().item() and (self.ws[self.ws_bytes:] == self.CANARY).all().item())


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_bigram_on_every_frame_fills_the_table_and_a_short_ids_row_is_cut(device, variant):
    """T = 12 frames, a bigram token on every one: the best string has 2T characters and every extension of it writes two nodes.
    One frame per chunk with max_frames exactly T, the state and the workspace exactly the sizes the queries name, each followed
    by a canary; then a result with Lcap = 5 < 2T"""
    T, B, V, W, K = 12, 2, 30, 16, 8
    gram = gref.random_table(V, 5, 24)
    x = np.stack([gref.bigram_run(T, gram, 24 + b) for b in range(B)], axis=1)
    model = edge_model(V, 4, 24) if variant == "lm" else None
    want = both_ways(device, x, gram, model, W, K)
    assert np.all(want[1][:, 0] == 2 * T)
    want = oneshot(device, x, gram, model, W, K, 0, None, False)
    xt = torch.from_numpy(x).to(device)
    r = Raw(device, B, V, T, W, K, gram, model, alloc_Tc=1)
    assert r.reset() == 0
    for t in range(T):
        assert r.advance(xt[t:t + 1], t) == 0
    assert r.advance(xt[:1], T) == ASR_ERR_UNSUPPORTED
    rc, ids, ln, sc, fr = r.result(2 * T)
    assert rc == 0 and ids.tobytes() == want[0].tobytes() and ln.tobytes() == want[1].tobytes() and sc.tobytes() == want[2].tobytes()
    assert fr.tolist() == [T] * B
    rc, ids2, ln2, sc2, _ = r.result(5)
    assert rc == 0 and np.array_equal(ids2, want[0][:, :, :5]) and ln2.tobytes() == want[1].tobytes() and sc2.tobytes() == sc.tobytes()
    assert np.all(ln2[:, 0] == 2 * T)                    # the full length, although the row holds 5 ids
    assert r.canaries_intact()


@pytest.mark.parametrize("variant", VARIANTS)
def test_an_inventory_without_unigram_rows(device, variant):
    gram = gref.random_table(10, 3, 21, all_bigram=True)
    assert not np.any((gram[:, 0] >= 0) & (gram[:, 1] < 0)) and np.sum(gram[:, 1] >= 0) == 9
    want = both_ways(device, base.small(14, 2, 10, 21), gram, edge_model(10, 4, 21) if variant == "lm" else None, 16, 9)
    assert np.all(want[1] % 2 == 0) and want[1].max() > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_that_spell_nothing_among_the_top_candidates(device, variant):
    gram = gref.random_table(12, 3, 22, dead=3)
    dead = [v for v in range(1, 12) if gram[v, 0] < 0]
    assert len(dead) == 3
    x = base.small(16, 2, 12, 22)
    x[:, :, dead] += 3.0
    both_ways(device, x, gram, edge_model(12, 3, 22) if variant == "lm" else None, 8, 4)


# ------------------------------------------------------------------------------------------------ 6. slot reuse
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_partial_reset_starts_one_slot_over(device, variant):
    shape = (20, 3, 9, 3, 8, 5, 0, 31)
    T, B, V, U, W, K, _, _ = shape
    x, gram, model = setup(*shape)
    model = model if variant == "lm" else None
    xt = torch.from_numpy(x).to(device)
    s = open_stream(device, B, V, T, gram, W, K, 0, model)
    s.advance(xt[:10])
    s.reset(mask=[0, 1, 0])
    s.advance(xt[10:])
    got = fetch(s)
    same(got, oneshot(device, x, gram, model, W, K, 0), rows=[0, 2])
    same(got, oneshot(device, x[10:], gram, model, W, K, 0), T=20, rows=[1])
    assert np.all(got[0][1, :, 20:] == 0)
    assert s.frames.cpu().tolist() == [20, 10, 20]


# ------------------------------------------------------------------------------------------------ 7. state hygiene
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_same_chunks_give_the_same_state_and_max_frames_does_not_matter(device, variant):
    shape = (20, 3, 9, 3, 8, 5, 0, 31)
    T, B, V, U, W, K, _, _ = shape
    x, gram, model = setup(*shape)
    model = model if variant == "lm" else None
    runs = []
    for F in (T, T, 2 * T):
        s = open_stream(device, B, V, F, gram, W, K, 0, model)
        feed(s, device, x, cuttings(T, 3)[2])
        out = fetch(s)
        runs.append((s.state.cpu().numpy().tobytes(), out))
    assert runs[0][0] == runs[1][0]
    same(runs[1][1], runs[0][1])
    same(runs[2][1], runs[0][1])
    same(runs[0][1], oneshot(device, x, gram, model, W, K, 0))


def unused(out, B):
    rc, ids, ln, sc, fr = out
    return rc == 0 and fr.tolist() == [-1] * B and bool(np.all(ids == 0) and np.all(ln == 0) and np.all(sc == -np.inf))


@pytest.mark.parametrize("variant", VARIANTS)
def test_errors_and_foreign_states_leave_the_state_alone(device, variant):
    V, B, F = 100, 2, 8
    gram = gref.random_table(V, 10, 3)
    model = make_lm(lmref.random_model(np.random.RandomState(3), V, 3, n_random=500), V) if variant == "lm" else None
    x = torch.from_numpy(base.small(4, B, V, 5)).to(device)
    r = Raw(device, B, V, F, 16, 16, gram, model, alloc_W=129)
    assert r.reset() == 0 and r.advance(x, 0) == 0
    before = r.state_bytes()
    need = r.lib.asr_gram_ctc_beam_stream_state_bytes(B, 16, F, int(model is not None))
    need_ws = r.lib.asr_gram_ctc_beam_stream_workspace_bytes(4, B, V, 16, 16)
    assert r.advance(x, 4, st_bytes=need - 1) == ASR_ERR_WORKSPACE
    assert r.advance(x, 4, ws_bytes=need_ws - 1) == ASR_ERR_WORKSPACE
    assert r.result(16, st_bytes=need - 1)[0] == ASR_ERR_WORKSPACE
    assert r.advance(x, 5) == ASR_ERR_UNSUPPORTED                  # 5 + 4 > 8
    for W, K in ((129, 1), (1, 65), (65, 64), (128, 33)):
        assert r.advance(x, 4, W=W, K=K) == ASR_ERR_UNSUPPORTED, (W, K)
    assert r.advance(x, 4, gram=False) == ASR_ERR_UNSUPPORTED
    assert r.advance(x, 4, logits=False) == ASR_ERR_BAD_ARG
    assert r.advance(x, 4, state=False) == ASR_ERR_BAD_ARG
    assert r.advance(x, -1) == ASR_ERR_BAD_ARG
    assert r.result(0)[0] == ASR_ERR_BAD_ARG
    if model is not None:
        assert r.advance(x, 4, order=0) == ASR_ERR_BAD_ARG
        assert r.advance(x, 4, order=5) == ASR_ERR_UNSUPPORTED
        assert r.advance(x, 4, slots=12) == ASR_ERR_BAD_ARG
        assert r.advance(x, 4, max_probe=0) == ASR_ERR_BAD_ARG
        assert r.advance(x, 4, vlm=V - 1) == ASR_ERR_BAD_ARG
        assert r.advance(x, 4, bos=V + 2) == ASR_ERR_BAD_ARG
        assert r.result(16, eos=V + 2)[0] == ASR_ERR_BAD_ARG
    assert r.state_bytes() == before and r.canaries_intact()
    assert r.advance(x, 4) == 0 and r.state_bytes() != before
    assert r.result(16)[4].tolist() == [8] * B
    # a state reset for beam_width 8, opened with beam_width 16 inside the same allocation
    assert r.reset(W=8) == 0
    before = r.state_bytes()
    assert r.advance(x, 0, W=16) == 0
    assert r.state_bytes() == before
    assert unused(r.result(16, W=16), B)
    assert r.state_bytes() == before and r.canaries_intact()
    assert r.advance(x, 0, W=8, K=8) == 0 and r.result(16, W=8)[4].tolist() == [4] * B
    # a state of the CTC stream given to the Gram entries
    assert r.ctc_reset() == 0 and r.ctc_advance(x, 0) == 0
    assert r.ctc_result(8)[4].tolist() == [4] * B
    before = r.state_bytes()
    assert r.advance(x, 4) == 0
    assert r.state_bytes() == before
    assert unused(r.result(16), B)
    assert r.state_bytes() == before and r.ctc_result(8)[4].tolist() == [4] * B
    # a Gram state given to the CTC stream's entries
    assert r.reset() == 0 and r.advance(x, 0) == 0
    before = r.state_bytes()
    assert r.ctc_advance(x, 4) == 0
    assert r.state_bytes() == before
    assert unused(r.ctc_result(8), B)
    assert r.state_bytes() == before and r.result(16)[4].tolist() == [4] * B and r.canaries_intact()


# ------------------------------------------------------------------------------------------------ 8. the Python class
def test_the_class_validates_the_table_the_model_the_chunks_and_overfeeding(device):
    from asr import error
    V = 9
    gram = gref.random_table(V, 3, 1)
    bad = gram.copy()
    bad[0] = (1, -1)                                     # the blank row spells something
    with pytest.raises(ValueError):
        error.GramBeamStream(2, V, 10, bad, device=device)
    with pytest.raises(ValueError):
        error.GramBeamStream(2, V, 10, torch.from_numpy(bad).to(device), device=device)
    with pytest.raises(ValueError):
        error.GramBeamStream(2, V + 1, 10, gram, device=device)
    with pytest.raises(ValueError):
        error.GramBeamStream(2, V, 10, gram, lm=edge_model(V - 3, 2, 1), device=device)      # lm.vlm < V
    with pytest.raises(ValueError):
        error.GramBeamStream(2, V, 0, gram, device=device)
    s = error.GramBeamStream(2, V, 10, torch.from_numpy(gram).to(device), 4, 4, device=device)
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
    assert len(out) == 3 and out[0].shape == (2, 4, 20) and s.frames.cpu().tolist() == [4, 10]
    s.reset()
    assert s.fed == 0 and fetch(s)[0].shape == (2, 4, 0) and s.frames.cpu().tolist() == [0, 0]
    s.advance(x)
    same(fetch(s), gbeam(device, x.cpu().numpy(), gram, 4, 4))
    assert len(fetch(error.GramBeamStream(2, V, 10, gram, 4, 4, lm=edge_model(V, 2, 1), device=device))) == 5
