"""CTC / Gram-CTC forced alignment on the GPU (csrc/ctc_align.hip through asr.loss.ctc_align / gram_ctc_align) against a brute-force
search over every path, the float64 restatement of tests/ctc_align_reference.py and the project's own loss and decoders.

Integer outputs (frames, tokens, positions, starts, ends, n_tokens) must equal the restatement exactly: both sides run the same
IEEE float64 max and one addition per step on the same f32 logits.  Tolerance for score / token_logp: 1e-4 * max(1, |value|), the
project's CTC loss tolerance (tests/test_ctc_gpu.py, from BASELINE.json): they are sums of the per-frame log-softmax terms the
loss is made of.  Every test prints its worst error / tolerance.
"""
import functools
import sys

import numpy as np
import pytest
import torch

import ctc_align_reference as ref
from ctc_beam_reference import peaky
from oracle import ctc as octc

pytestmark = pytest.mark.gpu

RTOL = 1e-4
INTS = ("frames", "tokens", "positions", "starts", "ends", "n_tokens")
ASR_ERR_BAD_ARG, ASR_ERR_WORKSPACE = -1, -2
POISON_I, POISON_F = 0x5A5A5A5A, 12345.5


def _t(device, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def run(device, xs, uni, big, xl, tl, blank=0, as_tuple=False):
    """numpy in -> dict of numpy arrays named as the fields of asr.loss.Alignment, through the public functions"""
    from asr.loss import ctc_align, gram_ctc_align
    x = _t(device, xs, np.float32)
    if as_tuple:
        x = tuple(x.unbind(0))
    if big is None:
        a = ctc_align(x, _t(device, uni, np.int32), blank, _t(device, xl, np.int32), _t(device, tl, np.int32))
    else:
        a = gram_ctc_align(x, _t(device, uni, np.int32), _t(device, big, np.int32), blank, _t(device, xl, np.int32),
                           _t(device, tl, np.int32))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in a._asdict().items()}


def ratio(got, want):
    """worst |got - want| / tolerance over two float arrays; -inf must match -inf"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf) and not np.isnan(got).any()
    if inf.all():
        return 0.0
    d = np.abs(got[~inf] - want[~inf]) / (RTOL * np.maximum(1.0, np.abs(want[~inf])))
    return float(d.max())


def compare(got, want, what):
    for k in INTS:
        bad = np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))
        assert bad.size == 0, "%s: %s differs from the restatement, first at %s (%d elements)" % (what, k, bad[0], len(bad))
    r = max(ratio(got["score"], want["score"]), ratio(got["token_logp"], want["token_logp"]))
    print("%s: worst error / tolerance of score and token_logp = %.3g" % (what, r))
    assert r <= 1.0, (what, r)
    return r


# ------------------------------------------------------------------------------------------------ 1. brute force
def test_tiny_ctc_against_brute_force(device):
    worst = 0.0
    for i, (x, u, L) in enumerate(ref.tiny_ctc_cases()):
        got = run(device, x[:, None, :], u[None, :], None, None, np.array([L]))
        best, frames = ref.brute_force(x, u, None, L, 0)
        if frames is None:
            assert got["score"][0] == -np.inf and got["n_tokens"][0] == 0 and np.all(got["frames"] == 0), i
            continue
        assert np.array_equal(got["frames"][0], frames), (i, got["frames"][0], frames)
        worst = max(worst, ratio(got["score"], [best]))
    print("tiny CTC: worst error / tolerance of score = %.3g" % worst)
    assert worst <= 1.0


def test_tiny_gram_against_brute_force(device):
    worst = 0.0
    for i, (x, u, g, L) in enumerate(ref.tiny_gram_cases()):
        got = run(device, x[:, None, :], u[None, :], g[None, :], None, np.array([L]))
        best, frames = ref.brute_force(x, u, g, L, 0)
        if frames is None:
            assert got["score"][0] == -np.inf and got["n_tokens"][0] == 0 and np.all(got["frames"] == 0), i
            continue
        assert np.array_equal(got["frames"][0], frames), (i, got["frames"][0], frames)
        worst = max(worst, ratio(got["score"], [best]))
    print("tiny Gram-CTC: worst error / tolerance of score = %.3g" % worst)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 2. the goldens' label sets
GOLDEN = ["ctc_small", "ctc_noreduce", "ctc_full", "ctc_v300", "ctc_v3000", "ctc_len1",
          "gram_mixed", "gram_all", "gram_repeat2", "gram_v3000", "gram_len1"]


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_label_sets(device, golden_dir, name):
    if golden_dir not in sys.path:
        sys.path.insert(0, golden_dir)
    import gram_ctc_fixture
    g = gram_ctc_fixture.load(golden_dir)
    xs, uni, big, xl, tl = [g["%s.%s" % (name, k)] for k in ("xs", "uni", "big", "xl", "tl")]
    xs, uni, big = np.asarray(xs, np.float32), np.asarray(uni, np.int32), np.asarray(big, np.int32)
    compare(run(device, xs, uni, big, xl, tl), ref.align_batch(xs, uni, big, xl, tl, 0), name + " (Gram-CTC lattice)")
    if name.startswith("ctc"):
        compare(run(device, xs, uni, None, xl, tl), ref.align_batch(xs, uni, None, xl, tl, 0), name + " (CTC lattice)")


# ------------------------------------------------------------------------------------------------ 3. full size
@functools.lru_cache(maxsize=None)
def full(kind, gram):
    case = ref.full_case(kind, gram, seed=20 + 2 * (kind == "peaky") + gram)
    return case, ref.align_batch(*case, 0)


FULL = [("randn", False), ("peaky", False), ("randn", True), ("peaky", True)]
FULL_IDS = ["randn-ctc", "peaky-ctc", "randn-gram", "peaky-gram"]


@pytest.mark.parametrize("kind,gram", FULL, ids=FULL_IDS)
def test_full_size_equals_restatement(device, kind, gram):
    """B = 32, T = 1000, V = 3000, L ~ U{40..120}, x_len ~ U{600..1000}: all 32 utterances, every integer output exact"""
    (xs, uni, big, xl, tl), want = full(kind, gram)
    got = run(device, xs, uni, big, xl, tl)
    assert np.all(np.isfinite(want["score"])) and np.all(want["n_tokens"] > 0)
    if gram:
        n_big = int((want["tokens"] >= 119).sum())
        print("bigram tokens on the best paths: %d of %d tokens" % (n_big, int(want["n_tokens"].sum())))
        assert n_big > 0
    if kind == "peaky":       # the transcript was perturbed: the alignment has to disagree with the per-frame argmax somewhere
        arg = xs.argmax(axis=2).T
        assert any(np.any(want["frames"][b, :xl[b]] != arg[b, :xl[b]]) for b in range(xs.shape[1]))
    compare(got, want, "full size %s %s" % (kind, "Gram-CTC" if gram else "CTC"))


# ------------------------------------------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("gram", [False, True], ids=["ctc", "gram"])
@pytest.mark.parametrize("kind", ["zeros", "small-int"])
def test_ties_follow_the_rule(device, kind, gram):
    rs = np.random.RandomState(3)
    T, B, V, L = 40, 6, 9, 6
    xs = np.zeros((T, B, V), np.float32) if kind == "zeros" else rs.randint(0, 3, size=(T, B, V)).astype(np.float32)
    uni = rs.randint(1, 4, size=(B, L)).astype(np.int32)
    big = None
    if gram:
        big = np.where(rs.rand(B, L) < 0.3, -1, rs.randint(4, V, size=(B, L))).astype(np.int32)
        big[:, 0] = -1
    xl = np.array([40, 33, 12, 40, 25, 13], np.int32)
    tl = np.array([6, 6, 6, 3, 1, 5], np.int32)
    compare(run(device, xs, uni, big, xl, tl), ref.align_batch(xs, uni, big, xl, tl, 0), "ties %s" % kind)


# ------------------------------------------------------------------------------------------------ 5. consistency
@pytest.mark.parametrize("kind,gram", FULL, ids=FULL_IDS)
def test_score_below_the_loss_and_parts_add_up(device, kind, gram):
    from asr.loss import connectionist_temporal_classification, gram_ctc
    (xs, uni, big, xl, tl), _ = full(kind, gram)
    got = run(device, xs, uni, big, xl, tl)
    x = _t(device, xs)
    with torch.no_grad():
        if gram:
            loss = gram_ctc(x, _t(device, uni), _t(device, big), 0, _t(device, xl), _t(device, tl), "no")
        else:
            loss = connectionist_temporal_classification(x, _t(device, uni), 0, _t(device, xl), _t(device, tl), "no")
    loss = loss.double().cpu().numpy()
    worst = 0.0
    for b in range(xs.shape[1]):
        s = float(got["score"][b])
        assert np.isfinite(s) and s <= -loss[b] + RTOL * max(1.0, abs(loss[b])), (b, s, -loss[b])
        lp = octc.log_softmax(xs[:xl[b], b].astype(np.float64), axis=1)
        fr = got["frames"][b, :xl[b]]
        n = got["n_tokens"][b]
        tok_frames = np.zeros(xl[b], bool)
        for k in range(n):
            tok_frames[got["starts"][b, k]:got["ends"][b, k]] = True
        parts = float(got["token_logp"][b, :n].astype(np.float64).sum() + lp[~tok_frames, 0].sum())
        assert np.all(fr[~tok_frames] == 0)
        worst = max(worst, abs(parts - s) / (RTOL * max(1.0, abs(s))))
    print("%s %s: worst |sum of parts - score| / tolerance = %.3g" % (kind, "gram" if gram else "ctc", worst))
    assert worst <= 1.0


@pytest.mark.parametrize("kind", ["randn", "peaky"])
def test_greedy_round_trip(device, kind):
    """the greedy labelling aligned back gives the greedy path: labels of length up to T, i.e. 2 T + 1 lattice nodes"""
    from asr import _ops, error
    from asr.loss import ctc_align
    rs = np.random.RandomState(8)
    T, B, V = 1000, 4, 3000
    xs = rs.randn(T, B, V).astype(np.float32) if kind == "randn" else np.stack([peaky(rs, T, V) for _ in range(B)], axis=1)
    top2 = np.sort(xs, axis=2)[:, :, -2:]
    assert np.all(top2[:, :, 1] > top2[:, :, 0])              # no row has a tied maximum
    xl = np.array([1000, 777, 950, 3], np.int32)
    x = _t(device, xs)
    lengths = _t(device, xl)
    ids, lens = error.greedy_decode(x, 0, lengths)
    a = ctc_align(x, ids, 0, lengths, lens)
    arg = _ops.argmax_rows(x)
    torch.cuda.synchronize()
    frames, arg = a.frames.cpu().numpy(), arg.cpu().numpy()
    assert np.array_equal(a.n_tokens.cpu().numpy(), lens.cpu().numpy())
    for b in range(B):
        assert np.array_equal(frames[b, :xl[b]], arg[b, :xl[b]]), b
        assert np.all(frames[b, xl[b]:] == 0)
    lp = octc.log_softmax(xs.astype(np.float64), axis=2)
    want = [lp[:xl[b], b].max(axis=1).sum() for b in range(B)]
    r = ratio(a.score.cpu().numpy(), want)
    print("greedy round trip %s: worst error / tolerance of score = %.3g" % (kind, r))
    assert r <= 1.0


def test_beam_hypothesis_gets_time_stamps(device):
    from asr import error
    from asr.loss import connectionist_temporal_classification, ctc_align
    rs = np.random.RandomState(9)
    T, B, V = 1000, 4, 3000
    xs = np.stack([peaky(rs, T, V) for _ in range(B)], axis=1)
    xl = np.array([1000, 640, 901, 820], np.int32)
    x, lengths = _t(device, xs), _t(device, xl)
    ids, lens, _ = error.beam_decode(x, 16, 16, 0, lengths)
    a = ctc_align(x, ids[:, 0], 0, lengths, lens[:, 0])             # the slot as it comes
    with torch.no_grad():
        loss = connectionist_temporal_classification(x, ids[:, 0].contiguous(), 0, lengths, lens[:, 0].contiguous(), "no")
    torch.cuda.synchronize()
    n, s, loss = a.n_tokens.cpu().numpy(), a.score.double().cpu().numpy(), loss.double().cpu().numpy()
    assert np.array_equal(n, lens[:, 0].cpu().numpy()) and np.all(n > 0)
    for b in range(B):
        assert np.isfinite(s[b]) and s[b] <= -loss[b] + RTOL * max(1.0, abs(loss[b])), (b, s[b], -loss[b])
    tokens, hyp = a.tokens.cpu().numpy(), ids[:, 0].cpu().numpy()
    for b in range(B):
        assert np.array_equal(tokens[b, :n[b]], hyp[b, :n[b]])


# ------------------------------------------------------------------------------------------------ 6. edges
def edge_batch(gram):
    rs = np.random.RandomState(4)
    T, B, V, L = 30, 6, 7, 4                    # V is not a multiple of 4: the scalar row path
    xs = (rs.randn(T, B, V) * 2).astype(np.float32)
    uni = np.array([[1, 2, 2, 1], [1, 1, 1, 1], [2, 1, 2, 1], [1, 2, 1, 2], [1, V + 3, 2, 1], [2, 2, 1, 1]], np.int32)
    xl = np.array([30, 5, 30, 0, 30, 17], np.int32)      # 1: 4 equal labels need 7 frames (CTC)    3: no frames
    tl = np.array([4, 4, 0, 2, 4, 3], np.int32)          # 2: empty transcript    4: an id outside [0, V)
    big = None
    if gram:
        big = np.array([[-1, 3, -1, 4], [-1, -1, -1, -1], [-1, 5, 5, 5], [-1, 3, 3, 3], [-1, -1, 6, -1], [-1, 4, 4, 4]], np.int32)
    return xs, uni, big, xl, tl


@pytest.mark.parametrize("gram", [False, True], ids=["ctc", "gram"])
def test_edges_in_one_batch(device, gram):
    xs, uni, big, xl, tl = edge_batch(gram)
    want = ref.align_batch(xs, uni, big, xl, tl, 0)
    assert want["score"][1] == -np.inf and want["score"][3] == -np.inf and np.isfinite(want["score"][[0, 2, 5]]).all()
    assert np.isfinite(want["score"][4]) == gram          # only the bigram (1 .. 2) bridges the bad unigram
    assert want["n_tokens"][2] == 0
    got = run(device, xs, uni, big, xl, tl)
    compare(got, want, "edges")
    for b in range(xs.shape[1]):
        assert np.all(got["frames"][b, max(xl[b], 0):] == 0)
    compare(run(device, xs, uni, big, xl, tl, as_tuple=True), want, "edges, tuple of views")
    want_none = ref.align_batch(xs, uni, big, None, None, 0)
    compare(run(device, xs, uni, big, None, None), want_none, "edges, no lengths")


def test_other_blank_symbol(device):
    rs = np.random.RandomState(10)
    xs = (rs.randn(25, 3, 6) * 2).astype(np.float32)
    uni = np.array([[0, 1, 3, 3], [5, 4, 0, 1], [3, 0, 3, 0]], np.int32)
    xl, tl = np.array([25, 9, 20], np.int32), np.array([4, 3, 4], np.int32)
    want = ref.align_batch(xs, uni, None, xl, tl, 2)
    assert np.isfinite(want["score"]).all()
    got = run(device, xs, uni, None, xl, tl, blank=2)
    compare(got, want, "blank = 2")
    assert np.all(got["frames"][1, 9:] == 2) and np.all(got["tokens"][1, 3:] == 2)


def raw(device, xs, uni, big, xl, tl, blank=0, ws_bytes=None, bad=None):
    """asr_ctc_align with every output pre-filled with a poison value -> (rc, dict of numpy outputs); `bad` replaces arguments"""
    from asr import _lib
    lib = _lib.lib()
    T, B, V = xs.shape
    Lmax = uni.shape[1]
    x, u, g, l1, l2 = _t(device, xs), _t(device, uni), _t(device, big), _t(device, xl), _t(device, tl)
    n = lib.asr_ctc_align_workspace_bytes(T, B, V, Lmax, int(big is not None))
    ws = torch.zeros(n, dtype=torch.uint8, device=device)
    out = dict(frames=torch.full((B, T), POISON_I, dtype=torch.int32, device=device))
    for k in ("tokens", "positions", "starts", "ends"):
        out[k] = torch.full((B, Lmax), POISON_I, dtype=torch.int32, device=device)
    out["token_logp"] = torch.full((B, Lmax), POISON_F, dtype=torch.float32, device=device)
    out["n_tokens"] = torch.full((B,), POISON_I, dtype=torch.int32, device=device)
    out["score"] = torch.full((B,), POISON_F, dtype=torch.float32, device=device)
    p = _lib.ptr
    args = dict(xs=p(x), T=T, B=B, V=V, Lmax=Lmax, blank=blank, frames=p(out["frames"]), ws=p(ws))
    args.update(bad or {})
    rc = lib.asr_ctc_align(_lib.stream(), args["xs"], p(u), p(g), p(l1), p(l2), args["T"], args["B"], args["V"], args["Lmax"],
                           args["blank"], args["frames"], p(out["tokens"]), p(out["positions"]), p(out["starts"]), p(out["ends"]),
                           p(out["token_logp"]), p(out["n_tokens"]), p(out["score"]), args["ws"], n if ws_bytes is None else ws_bytes)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def untouched(out):
    return all(np.all(out[k] == POISON_I) for k in INTS) and np.all(out["token_logp"] == POISON_F) and np.all(out["score"] == POISON_F)


@pytest.mark.parametrize("gram", [False, True], ids=["ctc", "gram"])
def test_every_output_element_is_written(device, gram):
    xs, uni, big, xl, tl = edge_batch(gram)
    rc, got = raw(device, xs, uni, big, xl, tl)
    assert rc == 0
    compare(got, ref.align_batch(xs, uni, big, xl, tl, 0), "poisoned outputs")      # no poison survives anywhere


# ------------------------------------------------------------------------------------------------ 7. raw ABI
def test_raw_abi_errors_leave_the_outputs_alone(device):
    from asr import _lib
    xs, uni, big, xl, tl = edge_batch(True)
    n = _lib.lib().asr_ctc_align_workspace_bytes(xs.shape[0], xs.shape[1], xs.shape[2], uni.shape[1], 1)
    rc, out = raw(device, xs, uni, big, xl, tl, ws_bytes=n - 1)
    assert rc == ASR_ERR_WORKSPACE and untouched(out)
    for bad in (dict(xs=None), dict(frames=None), dict(ws=None), dict(T=0), dict(B=-1), dict(V=0), dict(Lmax=0), dict(blank=-1),
                dict(blank=xs.shape[2])):
        rc, out = raw(device, xs, uni, big, xl, tl, bad=bad)
        assert rc == ASR_ERR_BAD_ARG and untouched(out), bad


@pytest.mark.parametrize("gram", [False, True], ids=["ctc", "gram"])
def test_long_input_and_two_launches(device, gram):
    """more frames than one block of back-pointers holds in LDS (the spill path), against the restatement; a second launch
    gives bit-identical outputs"""
    rs = np.random.RandomState(6)
    T, B, V, L = (1500 if gram else 2600), 3, 200, 120      # one block holds 1088 (Gram-CTC) / 2486 (CTC) frames at this Lmax
    xs = rs.randn(T, B, V).astype(np.float32)
    uni = rs.randint(1, 60, size=(B, L)).astype(np.int32)
    big = None
    if gram:
        big = np.where(rs.rand(B, L) < 0.3, -1, rs.randint(60, V, size=(B, L))).astype(np.int32)
        big[:, 0] = -1
    xl = np.array([T, T - 389, 400], np.int32)
    tl = np.array([120, 77, 101], np.int32)
    rc, one = raw(device, xs, uni, big, xl, tl)
    rc2, two = raw(device, xs, uni, big, xl, tl)
    assert rc == 0 and rc2 == 0
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k
    compare(one, ref.align_batch(xs, uni, big, xl, tl, 0), "long input")
