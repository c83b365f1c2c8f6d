"""Committing a prefix of a streaming beam search on the GPU (asr.error.BeamStream / GramBeamStream .commit, the
asr_*_beam_stream_commit entries of csrc/ctc_beam.hip).

Comparisons between two device runs are on bytes: a commit moves entries and renumbers table nodes, it computes nothing, so
whatever the stream returns after a commit of the common prefix is the uncommitted stream's output.  Against the float64
restatement with commits (tests/beam_commit_reference.py) the conditions are tests/test_ctc_beam_gpu.py::compare_nbest's.
"""
import functools

import numpy as np
import pytest
import torch

import beam_commit_reference as cr
import ctc_beam_reference as ref
import test_ctc_beam_gpu as base
import test_ctc_beam_stream_gpu as sbase
import test_ctx_bias_gpu as bbase
import test_gram_ctx_bias_gpu as gcbase
from test_beam_stream_commit_cpu import align256, joined
from test_ctc_beam_gpu import compare_nbest

pytestmark = pytest.mark.gpu

ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE, ASR_ERR_UNSUPPORTED = -1, -2, -3
FAMILIES = [("ctc", v) for v in ("plain", "lm", "graph", "lm_graph")] + [("gram", v) for v in ("plain", "lm", "graph")]
IDS = ["%s-%s" % f for f in FAMILIES]


def per_frame(family):
    return 2 if family == "gram" else 1


@functools.lru_cache(maxsize=None)
def extras(family, V, seed):
    """(gram table or None, model, graph) for logits over V ids"""
    if family == "ctc":
        _, model, graph = sbase.setup(4, 1, V, 4, 4, 0, seed)
        return None, model, graph
    _, gram, model, graph = gcbase.stream_setup(4, 1, V, {9: 3, 12: cr.GRAM_U, 80: 10}[V], seed)
    return gram, model, graph


def opener(device, family, variant, V, W, K, seed=7, neutral=False):
    """-> (open(B, F) -> a stream of the variant, oneshot(x) -> the one-shot tuple of numpy arrays, the gram table or None).
    `neutral`: a model with weights 0 and a graph without phrases, which rank as the plain search does."""
    gram, model, graph = extras(family, V, seed)
    model = model if "lm" in variant else None
    graph = graph if "graph" in variant else None
    if neutral and graph is not None:
        graph = bbase.make_graph([], V)
    from asr import error
    a, b = (sbase.ALPHA, sbase.BETA) if model is not None and not neutral else (0.0, 0.0)

    def open_stream(B, F):
        if family == "ctc":
            return error.BeamStream(B, V, F, W, K, 0, None, model, a, b, graph, device)
        return error.GramBeamStream(B, V, F, gram, W, K, 0, None, model, a, b, device, graph=graph)

    def oneshot(x):
        if family == "ctc":
            return sbase.oneshot(device, x, model, graph, W, K)
        if graph is not None:
            return gcbase.gbiased(device, x, gram, graph, model, a, b, W, K)
        if model is not None:
            return gcbase.gfused(device, x, gram, model, a, b, W, K)
        return gcbase.gbeam(device, x, gram, W, K)

    return open_stream, oneshot, gram


def numpy_of(out):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def equal_tuples(got, want):
    """two result tuples, byte for byte; the ids are compared over the wider of the two widths, padded with blank (0)"""
    assert len(got) == len(want)
    for k, (u, v) in enumerate(zip(got, want)):
        if k == 0:
            width = max(u.shape[2], v.shape[2])
            u = np.pad(u, ((0, 0), (0, 0), (0, width - u.shape[2])))
            v = np.pad(v, ((0, 0), (0, 0), (0, width - v.shape[2])))
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert u.dtype == v.dtype and u.shape == v.shape, (k, u.dtype, v.dtype, u.shape, v.shape)
        assert u.tobytes() == v.tobytes(), (k, u, v)


def pad_to(a, width):
    return np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, max(0, width - a.shape[-1]))])


def state_of(s):
    torch.cuda.synchronize()
    return s.state.cpu().numpy().tobytes()


def header(s):
    return s.state[:s.B * 32].view(torch.int32).view(s.B, 8).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. auto commit is free
def randn4(T, B, V, seed):
    return np.stack([(np.random.RandomState(seed + b).randn(T, V) * 4).astype(np.float32) for b in range(B)], axis=1)


# (name, T, B, V, W, K, logits): beams 1, 4, 16 and 128; V = 6 for CTC, the Gram-CTC tables need 9
def auto_cases(family):
    V = 6 if family == "ctc" else 9
    return [("beam1", 40, 2, V, 1, 5, randn4(40, 2, V, 5)), ("beam4", 60, 3, V, 4, 5, randn4(60, 3, V, 5)),
            ("beam16", 120, 2, V, 16, 5, randn4(120, 2, V, 5)), ("beam128", 30, 2, 80, 128, 32, base.small(30, 2, 80, 17)),
            ("peaky", 100, 2, 12, 8, 6, np.stack([ref.peaky(np.random.RandomState(s), 100, 12) for s in (1, 2)], axis=1))]


@pytest.mark.parametrize("family,variant", FAMILIES, ids=IDS)
def test_auto_commit_is_free(device, family, variant):
    """after every chunk of 10 frames: committed + tail, with every score, is the uncommitted stream's result and the one-shot
    decode of the frames so far, on bytes"""
    for name, T, B, V, W, K, x in auto_cases(family):
        open_stream, oneshot, _ = opener(device, family, variant, V, W, K)
        s, u = open_stream(B, T), open_stream(B, T)
        xt = torch.from_numpy(x).to(device)
        total = np.zeros(B, np.int64)
        for t0 in range(0, T, 10):
            s.advance(xt[t0:t0 + 10])
            u.advance(xt[t0:t0 + 10])
            tokens, counts, status = numpy_of(s.commit())
            assert status.tolist() == [1] * B, (name, t0, status)
            total += counts
            got = numpy_of(s.full_result())
            equal_tuples(got, numpy_of(u.result()))
            equal_tuples(got, oneshot(x[:t0 + 10]))
            assert s.frames.cpu().tolist() == [t0 + 10] * B
            assert header(s)[:, 7].tolist() == total.tolist() == [len(c) for c in s.committed]
        tails = numpy_of(s.result())
        print(family, variant, name, "committed", total.tolist(), "longest tail", int(tails[1].max()), "rows", header(s)[:, 6].tolist())
        if W == 1:
            assert tails[1].max() == 0 and (total > 0).all()        # one hypothesis: everything is common
        if name == "beam16" and (family, variant) == ("ctc", "plain"):
            # tests/test_beam_stream_commit_cpu.py::test_auto_commits_reach_tens_of_tokens_at_beam_16: 26 in float64
            assert total[0] >= 20


# ------------------------------------------------------------------------------------------------ 2./3. unbounded; pruning
def long_inputs(family):
    if family == "ctc":
        return cr.long_ctc_logits(), cr.LONG_CTC
    return cr.long_gram_inputs()[0], cr.LONG_GRAM


def small_table(family):
    """max_frames of the unbounded runs: twice (the rows of the longest tail the reference recorded + a chunk)"""
    longest = max(run["longest"] for run in cr.long_runs(family))
    return 2 * (-(-longest // per_frame(family)) + cr.CHUNK)


@functools.lru_cache(maxsize=None)
def replay(device, family, variant, F):
    """the long inputs through a stream of `max_frames` F with the reference's prefixes committed every CHUNK frames ->
    (per commit (tokens, counts, status), final tails tuple, final frames, committed lists)"""
    x, (T, V, W, K, seeds) = long_inputs(family)
    B = len(seeds)
    open_stream, _, _ = opener(device, family, variant, V, W, K, neutral=True)
    if family == "gram":
        assert np.array_equal(opener(device, family, variant, V, W, K)[2], cr.long_gram_inputs()[1])
    runs = cr.long_runs(family)
    s = open_stream(B, F)
    xt = torch.from_numpy(x).to(device)
    commits = []
    for k, t0 in enumerate(range(0, T, cr.CHUNK)):
        s.advance(xt[t0:t0 + cr.CHUNK])
        Ps = [run["log"][k][1] for run in runs]
        assert all(run["log"][k][0] == t0 + cr.CHUNK for run in runs)
        n = max(1, max(len(P) for P in Ps))
        prefix = np.zeros((B, n), np.int32)
        for b, P in enumerate(Ps):
            prefix[b, :len(P)] = P
        commits.append(numpy_of(s.commit(prefix, [len(P) for P in Ps])))
        assert s.fed <= F - cr.CHUNK or t0 + cr.CHUNK == T
    out = numpy_of(s.result())
    return commits, out, s.frames.cpu().tolist(), [list(c) for c in s.committed]


@pytest.mark.parametrize("family,variant", FAMILIES, ids=IDS)
def test_600_frames_through_a_table_of_a_few_dozen_rows(device, family, variant):
    x, (T, V, W, K, seeds) = long_inputs(family)
    F = small_table(family)
    assert F < T // 4
    commits, out, frames, committed = replay(device, family, variant, F)
    assert frames == [T] * len(seeds)
    assert all(status.tolist() == [1] * len(seeds) for _, _, status in commits)         # no call is refused
    assert out[0].shape[2] <= per_frame(family) * F
    print(family, variant, "max_frames", F, "committed", [len(c) for c in committed], "longest final tail", int(out[1].max()))


@pytest.mark.parametrize("family,variant", FAMILIES, ids=IDS)
def test_pruning_matches_the_restatement(device, family, variant):
    """the reference's schedule of prefixes against the float64 search that filters its beam list the same way, under
    compare_nbest's conditions; an utterance with a refused commit counts among those that may differ (B // 8 = 0 here: the
    seeds are chosen for their margins).  The model and the graph are neutral, so every variant ranks as the restatement does."""
    x, (T, V, W, K, seeds) = long_inputs(family)
    B = len(seeds)
    commits, out, _, committed = replay(device, family, variant, small_table(family))
    runs = cr.long_runs(family)
    refused = {b for _, _, status in commits for b in range(B) if status[b] != 1}
    gpu, want = [], []
    for b in range(B):
        hyps = base.hyps(out[0], out[1], out[2], b)
        gpu.append([(tuple(committed[b]) + h, sc) for h, sc in hyps])
        want.append(joined(runs[b]))
        if b not in refused:
            assert tuple(committed[b]) == runs[b]["done"]
    compare_nbest(gpu, want, B // 8 - len(refused))


@pytest.mark.parametrize("family,variant", [f for f in FAMILIES if f[1] != "plain"], ids=[i for i in IDS if "plain" not in i])
def test_unbounded_with_the_models_own_ranking(device, family, variant):
    """with a model and a graph that do rank: commit_best(8) every 20 frames, the prefix coming from the stream itself"""
    x, (T, V, W, K, seeds) = long_inputs(family)
    B, F = len(seeds), small_table(family) + 16
    open_stream, _, _ = opener(device, family, variant, V, W, K)
    s = open_stream(B, F)
    xt = torch.from_numpy(x).to(device)
    for t0 in range(0, T, cr.CHUNK):
        s.advance(xt[t0:t0 + cr.CHUNK])
        _, _, status = numpy_of(s.commit_best(cr.HOLD))
        assert status.tolist() == [1] * B
    out = numpy_of(s.result())
    assert s.frames.cpu().tolist() == [T] * B and out[1].max() <= per_frame(family) * F
    assert min(len(c) for c in s.committed) > 40


# ------------------------------------------------------------------------------------------------ 4. exact device-only properties
@pytest.mark.parametrize("family,variant", [("ctc", "lm_graph"), ("gram", "lm")], ids=["ctc", "gram"])
def test_the_table_size_does_not_matter(device, family, variant):
    F = small_table(family)
    a = replay(device, family, variant, F)
    b = replay(device, family, variant, 4 * F)
    for (ta, ca, sa), (tb, cb, sb) in zip(a[0], b[0]):
        assert ca.tobytes() == cb.tobytes() and sa.tobytes() == sb.tobytes()
        n = min(ta.shape[1], tb.shape[1])
        assert np.array_equal(ta[:, :n], tb[:, :n]) and not ta[:, n:].any() and not tb[:, n:].any()
    equal_tuples(a[1], b[1])
    assert a[2:] == b[2:]


@pytest.mark.parametrize("family,variant", [("ctc", "lm_graph"), ("gram", "graph")], ids=["ctc", "gram"])
def test_two_commits_are_one_peeking_writes_nothing_and_runs_repeat(device, family, variant):
    x, (T, V, W, K, seeds) = long_inputs(family)
    B = len(seeds)
    open_stream, _, _ = opener(device, family, variant, V, W, K)
    xt = torch.from_numpy(x).to(device)

    def fed():
        s = open_stream(B, 80)
        s.advance(xt[:40])
        s.advance(xt[40:60])
        return s
    s = fed()
    before = state_of(s)
    best = numpy_of(s.result())
    assert best[1][:, 0].min() >= 4
    P = best[0][:, 0, :4].astype(np.int32)
    peek = numpy_of(s.commit(P, None, compact=False))
    assert state_of(s) == before and s.committed == [[] for _ in range(B)] and s.fed == 60
    one = numpy_of(s.commit(P))
    assert peek[2].tolist() == one[2].tolist() == [1] * B
    assert np.array_equal(peek[0][:, :4], P) and np.array_equal(one[0][:, :4], P) and peek[1].tolist() == one[1].tolist() == [4] * B
    after = state_of(s)
    assert after != before
    two = fed()
    two.commit(P[:, :2])
    two.commit(P[:, 2:])
    assert state_of(two) == after and two.committed == s.committed == [row.tolist() for row in P]
    again = fed()
    again.commit(P)
    assert state_of(again) == after
    # and the search goes on from either state alike
    for stream in (s, two):
        stream.advance(xt[60:80])
    assert state_of(s) == state_of(two)
    equal_tuples(numpy_of(s.result()), numpy_of(two.result()))


# ------------------------------------------------------------------------------------------------ 5. refusals and guards
class RawCommit:
    """a fed stream's state copied in front of a canary, and the commit entry through the raw ABI"""
    CANARY, TAIL = 0xA5, 4096

    def __init__(self, device, family, s):
        from asr import _lib
        self._lib, self.lib, self.family, self.s, self.device = _lib, _lib.lib(), family, s, device
        self.st_bytes = s.state.numel()
        self.st = torch.full((self.st_bytes + self.TAIL,), self.CANARY, dtype=torch.uint8, device=device)
        self.st[:self.st_bytes] = s.state
        self.ws_bytes = self.lib.asr_beam_stream_commit_workspace_bytes(s.B, s.beam_width, s.max_frames, per_frame(family))
        assert self.ws_bytes > 0
        self.ws = torch.full((self.ws_bytes + self.TAIL,), self.CANARY, dtype=torch.uint8, device=device)

    def __call__(self, prefix, lens, W=None, compact=1, max_rows=None, ws_bytes=None, st_bytes=None, out_pitch=1, **null):
        s, p = self.s, self._lib.ptr
        B = s.B
        self.out = torch.full((B * out_pitch + 64,), -7, dtype=torch.int32, device=self.device)
        outs = [torch.full((B,), -7, dtype=torch.int32, device=self.device) for _ in range(4)]
        pre = None if prefix is None else torch.tensor(prefix, dtype=torch.int32, device=self.device).reshape(B, -1)
        ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=self.device)
        fn = self.lib.asr_gram_ctc_beam_stream_commit if self.family == "gram" else self.lib.asr_ctc_beam_stream_commit
        args = dict(state=p(self.st), workspace=p(self.ws), out_ids=p(self.out), out_len=p(outs[0]), out_committed=p(outs[1]),
                    out_rows=p(outs[2]), out_status=p(outs[3]))
        for k in null:
            args[k] = None
        rc = fn(self._lib.stream(), args["state"], self.st_bytes if st_bytes is None else st_bytes, B, W or s.beam_width, s.max_frames,
                int(s.lm is not None), int(s.graph is not None), p(pre), 0 if pre is None else pre.shape[1], p(ln), compact,
                s.max_frames if max_rows is None else max_rows, args["workspace"], self.ws_bytes if ws_bytes is None else ws_bytes,
                args["out_ids"], out_pitch, args["out_len"], args["out_committed"], args["out_rows"], args["out_status"])
        torch.cuda.synchronize()
        return rc, [o.cpu().tolist() for o in outs]

    def state_bytes(self):
        return self.st.cpu().numpy().tobytes()

    def canaries_intact(self, out_pitch=1):
        return bool((self.st[self.st_bytes:] == self.CANARY).all().item() and (self.ws[self.ws_bytes:] == self.CANARY).all().item()
                    and (self.out[self.s.B * out_pitch:] == -7).all().item())


@pytest.mark.parametrize("family,variant", [("ctc", "lm_graph"), ("gram", "lm")], ids=["ctc", "gram"])
def test_refusals_and_guards_leave_the_state_alone(device, family, variant):
    x, (T, V, W, K, seeds) = long_inputs(family)
    B = len(seeds)
    open_stream, _, _ = opener(device, family, variant, V, W, K)
    s = open_stream(B, 60)
    s.advance(torch.from_numpy(x[:40]).to(device))
    best = numpy_of(s.result())
    P = best[0][:, 0, :3].astype(np.int32)
    assert best[1][:, 0].min() >= 3 and best[1].max() > 3
    r = RawCommit(device, family, s)
    before = r.state_bytes()
    rows = header(s)[:, 6].tolist()
    # a prefix no hypothesis starts with (the blank is in no hypothesis), in one utterance only: the others are applied in a peek
    bad = P.copy()
    bad[0, 1] = 0
    rc, (n, c, rw, st) = r(bad, [3] * B, compact=0)
    assert rc == 0 and st == [0] + [1] * (B - 1) and n == [0] + [3] * (B - 1) and c == [0] + [3] * (B - 1) and rw[0] == rows[0]
    rc, (n, c, rw, st) = r(bad[:1].repeat(B, axis=0) * 0, [3] * B)
    assert rc == 0 and st == [0] * B and c == [0] * B and rw == rows
    rc, (n, c, rw, st) = r(P, [4] * B)                                   # a prefix longer than its row
    assert rc == 0 and st == [0] * B
    rc, (n, c, rw, st) = r(P, [3] * B, max_rows=0)                       # the kept tails need rows
    assert rc == 0 and st == [0] * B and rw == rows
    rc, (n, c, rw, st) = r(P, [3] * B, W=W // 2)                         # a state reset for another beam width
    assert rc == 0 and st == [-1] * B and c == [-1] * B and rw == [-1] * B
    assert r(P, [3] * B, ws_bytes=r.ws_bytes - 1)[0] == ASR_ERR_WORKSPACE
    assert r(P, [3] * B, st_bytes=r.st_bytes - 1)[0] == ASR_ERR_WORKSPACE
    for name in ("state", "workspace", "out_ids", "out_len", "out_committed", "out_rows", "out_status"):
        assert r(P, [3] * B, **{name: None})[0] == ASR_ERR_BAD_ARG, name
    assert r(P, None)[0] == ASR_ERR_BAD_ARG and r(P, [3] * B, out_pitch=0)[0] == ASR_ERR_BAD_ARG
    assert r(P, [3] * B, max_rows=-1)[0] == ASR_ERR_BAD_ARG and r(P, [3] * B, W=129)[0] == ASR_ERR_UNSUPPORTED
    assert r.state_bytes() == before
    # applied, with an out_ids row of one token: the row is cut, the count is whole, nothing is written behind anything
    rc, (n, c, rw, st) = r(P, [3] * B, out_pitch=1)
    assert rc == 0 and st == [1] * B and n == [3] * B and c == [3] * B and max(rw) < max(rows)
    assert r.out[:B].cpu().tolist() == P[:, 0].tolist() and r.canaries_intact()
    assert r.state_bytes() != before


def test_a_masked_reset_and_a_resting_slot(device):
    """reset(mask) starts one slot's committed count over while the others keep theirs; a slot with lengths == 0 in later chunks
    keeps its commit"""
    x, (T, V, W, K, seeds) = long_inputs("ctc")
    B = len(seeds)
    open_stream, oneshot, _ = opener(device, "ctc", "plain", V, W, K)
    xt = torch.from_numpy(x).to(device)
    s = open_stream(B, 70)
    s.advance(xt[:40])
    s.commit_best(4)
    mid = numpy_of(s.full_result())
    done = [list(c) for c in s.committed]
    assert min(len(c) for c in done) > 0 and header(s)[:, 7].tolist() == [len(c) for c in done]
    s.reset(mask=[0, 1] + [0] * (B - 2))
    assert header(s)[:, 7].tolist() == [len(done[0]), 0] + [len(c) for c in done[2:]]
    assert s.committed == [done[0], []] + done[2:]
    rest = torch.tensor([20, 20, 0] + [20] * (B - 3), dtype=torch.int32)
    s.advance(xt[40:60], rest)
    s.commit()
    full = numpy_of(s.full_result())
    assert s.frames.cpu().tolist() == [60, 20, 40] + [60] * (B - 3)
    assert s.committed[2][:len(done[2])] == done[2]
    want = oneshot(x[40:60])                                             # slot 1 has seen these 20 frames only
    for k in range(1, 3):
        assert full[k][1].tobytes() == want[k][1].tobytes()
    assert np.array_equal(pad_to(full[0][1], 60)[:, :20], want[0][1]) and not pad_to(full[0][1], 60)[:, 20:].any()
    for k in range(1, 3):                                                # slot 2 rests where the first commit left it
        assert full[k][2].tobytes() == mid[k][2].tobytes()
    assert np.array_equal(pad_to(full[0][2], 60), pad_to(mid[0][2], 60)) and mid[1][2].max() > len(done[2])


@pytest.mark.parametrize("on_device", [False, True], ids=["host_mask", "device_mask"])
def test_a_masked_reset_after_a_commit_of_no_tokens(device, on_device):
    """commit_best with a hold longer than every hypothesis commits nothing and still compacts the table, so the rows in use fall
    below the frames consumed; a masked reset right after it starts that slot's frame count at 0 like everything else of it"""
    x, (T, V, W, K, seeds) = long_inputs("ctc")
    B = len(seeds)
    open_stream, oneshot, _ = opener(device, "ctc", "plain", V, W, K)
    xt = torch.from_numpy(x).to(device)
    s = open_stream(B, 70)
    s.advance(xt[:20])
    _, counts, status = numpy_of(s.commit_best(1000))
    assert status.tolist() == [1] * B and counts.tolist() == [0] * B and s.committed == [[] for _ in range(B)]
    rows = header(s)[:, 6]
    assert rows.max() < 20 and s.fed == rows.max()                       # compacted: fewer rows than frames, in every slot
    numpy_of(s.result())
    assert s.frames.cpu().tolist() == [20] * B
    mask = [0, 1] + [0] * (B - 2)
    s.reset(mask=torch.tensor(mask, dtype=torch.int32, device=device) if on_device else mask)
    s.advance(xt[20:40])
    got = numpy_of(s.result())
    assert s.frames.cpu().tolist() == [40, 20] + [40] * (B - 2)
    s.commit()
    full = numpy_of(s.full_result())
    assert s.frames.cpu().tolist() == [40, 20] + [40] * (B - 2)
    want, fresh = oneshot(x[:40]), oneshot(x[20:40])
    for b in range(B):
        w = fresh if b == 1 else want
        for k in range(1, 3):
            assert got[k][b].tobytes() == w[k][b].tobytes() == full[k][b].tobytes()
        assert np.array_equal(pad_to(got[0][b], 40), pad_to(w[0][b], 40)) and np.array_equal(pad_to(full[0][b], 40), pad_to(w[0][b], 40))


# ------------------------------------------------------------------------------------------------ 5b. pruning with real weights
UNUSED = (0, 0, -np.inf, -np.inf, 0.0, 0.0)                            # ids, lengths, scores, ctc, lm, bias of an unused slot


@pytest.mark.parametrize("family,variant", FAMILIES, ids=IDS)
def test_a_pruning_commit_keeps_exactly_the_rows_that_start_with_the_prefix(device, family, variant):
    """with the variant's real weights, before any further advance: committed + tail with every part of every score is, on
    bytes, the uncommitted stream's rows that start with the prefix (the best hypothesis without its last token), in their
    order, then unused slots.  This is the check that
    sees every per-slot array of the variant (model contexts, automaton states) move with its hypothesis."""
    x, (T, V, W, K, seeds) = long_inputs(family)
    B = len(seeds)
    open_stream, _, _ = opener(device, family, variant, V, W, K)
    xt = torch.from_numpy(x).to(device)
    s, u = open_stream(B, 80), open_stream(B, 80)
    for stream in (s, u):
        stream.advance(xt[:40])
        stream.advance(xt[40:60])
    dropped = 0
    for use_eos in (True, False):
        whole = numpy_of(u.result(use_eos))
        if use_eos:
            n = whole[1][:, 0] - 1                                       # the best hypothesis without its last token
            assert n.min() >= 4
            P = whole[0][:, 0, :n.max()].astype(np.int32)
            _, counts, status = numpy_of(s.commit(P, n))
            assert status.tolist() == [1] * B and counts.tolist() == n.tolist()
        want = [np.empty_like(a) for a in whole]
        for b in range(B):
            rows = [i for i in range(W) if whole[2][b, i] > -np.inf and whole[1][b, i] >= n[b]
                    and np.array_equal(whole[0][b, i, :n[b]], P[b, :n[b]])]
            dropped += int((whole[2][b] > -np.inf).sum()) - len(rows)
            assert rows and (rows[0] == 0 or not use_eos)
            for k, a in enumerate(whole):
                want[k][b] = UNUSED[k]
                want[k][b, :len(rows)] = a[b, rows]
        equal_tuples(numpy_of(s.full_result(use_eos)), tuple(want))
    assert dropped > 0                                                   # something was pruned
    assert header(s)[:, 5].tolist() == [int((w > -np.inf).sum()) for w in want[2]]


# ------------------------------------------------------------------------------------------------ 6. the kernel's edges
@pytest.mark.parametrize("family", ["ctc", "gram"])
def test_one_commit_at_the_kernels_edges(device, family):
    """a state written by hand (plain variant): utterance 0 has m = W = 128 hypotheses of 1 .. 5 tokens whose first token
    alternates, so that the commit of that token keeps every other entry, with tails of 0 tokens and of exactly per_frame x rows
    tokens among them; utterance 1 is the root alone (m = 1) and commits nothing; the batch is ragged.  Every byte of the state
    after the commit is predicted."""
    from asr import _lib, _ops
    per, B, W, F = per_frame(family), 2, 128, 6
    if family == "ctc":
        nbytes = _ops.ctc_beam_stream_state_bytes(B, W, F, False, False)
        state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _ops.ctc_beam_stream_reset(state, B, W, F, False, False)
        sizes = [4, 4, 8, 8, 4, 4, 4, 4]                          # pb pnb hash phash len last plast node
        len_k, node_k = 4, 7
    else:
        nbytes = _ops.gram_ctc_beam_stream_state_bytes(B, W, F, False)
        state = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _ops.gram_ctc_beam_stream_reset(state, B, W, F, False)
        sizes = [4, 4, 4, 8, 8, 8, 4, 4, 4, 4, 4, 4, 4]           # pb pu pg h0 h1 h2 len c1 c2 c3 utok gtok node
        len_k, node_k = 6, 12
    torch.cuda.synchronize()
    img = state.cpu().numpy().copy()
    offs, off = [], align256(B * 32)
    for sz in sizes:
        offs.append(off)
        off += align256(B * W * sz)
    table_off = off
    assert off + align256(B * W * F * per * 8) == nbytes
    hdr = img[:B * 32].view(np.int32).reshape(B, 8)
    arrays = [img[o:o + B * W * sz].view(np.int32 if sz == 4 else np.uint64).reshape(B, W) for o, sz in zip(offs, sizes)]
    table = img[table_off:table_off + B * W * F * per * 8].view(np.int32).reshape(B, F * per * W, 2)
    root = [a[1, 0].copy() for a in arrays]
    rows0 = 5 if per == 1 else 3                                  # 5 tokens need 5 rows, or 3 of two characters
    toks = [[3 if i % 2 == 0 else 5] + [(i + j) % 7 + 1 for j in range(i % 5)] for i in range(W)]
    for k, a in enumerate(arrays):
        if k not in (len_k, node_k):
            a[0] = (np.arange(W) * 16 + k + 1).astype(a.dtype)     # recognisable values: a commit only moves them
    arrays[len_k][0] = [len(t) for t in toks]
    arrays[node_k][0] = [(len(t) - 1) * W + i for i, t in enumerate(toks)]
    for i, t in enumerate(toks):
        for j, c in enumerate(t):
            table[0, j * W + i] = ((j - 1) * W + i if j else -1, c)
    hdr[0, 5], hdr[0, 6] = W, rows0
    state.copy_(torch.from_numpy(img).to(device))
    want = img.copy()
    w_hdr = want[:B * 32].view(np.int32).reshape(B, 8)
    w_arrays = [want[o:o + B * W * sz].view(np.int32 if sz == 4 else np.uint64).reshape(B, W) for o, sz in zip(offs, sizes)]
    w_table = want[table_off:table_off + B * W * F * per * 8].view(np.int32).reshape(B, F * per * W, 2)
    kept = list(range(0, W, 2))
    for k, a in enumerate(w_arrays):
        a[0, :len(kept)] = arrays[k][0, kept]
        a[0, len(kept):] = 0
    w_table[0, :rows0 * per * W] = 0
    tails = [toks[i][1:] for i in kept]
    assert min(len(t) for t in tails) == 0 and max(len(t) for t in tails) == 4
    rows = -(-4 // per)
    assert max(len(t) for t in tails) == per * rows
    for q, t in enumerate(tails):
        w_arrays[node_k][0, q] = (len(t) - 1) * W + q if t else -1
        for j, c in enumerate(t):
            w_table[0, j * W + q] = ((j - 1) * W + q if j else -1, c)
    w_hdr[0, 5], w_hdr[0, 6], w_hdr[0, 7] = len(kept), rows, 1
    prefix = torch.tensor([[3], [0]], dtype=torch.int32, device=device)
    lens = torch.tensor([1, 0], dtype=torch.int32, device=device)
    tokens, counts, committed, rows_out, status = _ops.beam_stream_commit(state, family == "gram", B, W, F, False, False, prefix, lens,
                                                                         True, None, 2)
    torch.cuda.synchronize()
    assert status.tolist() == [1, 1] and counts.tolist() == [1, 0] and committed.tolist() == [1, 0] and rows_out.tolist() == [rows, 0]
    assert tokens.cpu().tolist() == [[3, 0], [0, 0]]
    got = state.cpu().numpy()
    for k, a in enumerate(arrays):
        assert np.array_equal(a[1, 0], root[k])
    assert got.tobytes() == want.tobytes()
    # the same state through the auto mode: utterance 0's live hypotheses share nothing more (a tail is empty)
    tokens, counts, committed, rows_out, status = _ops.beam_stream_commit(state, family == "gram", B, W, F, False, False, None, None,
                                                                         True, None, 2)
    torch.cuda.synchronize()
    assert status.tolist() == [1, 1] and counts.tolist() == [0, 0] and committed.tolist() == [1, 0]
    assert state.cpu().numpy().tobytes() == want.tobytes()
