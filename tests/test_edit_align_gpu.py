"""GPU: edit alignment (asr_edit_align), the pairwise distances of an N-best list (asr_nbest_pairwise_distance) and MBR decoding with
token confidence (asr_nbest_consensus) against tests/edit_align_reference.py.  Integer outputs are compared exactly; the float
caps are the ones DESIGN.md section 29 derives:

    posterior   float64 on the device: 1e-12 of the float64 reference
    risk[i]     float64 on the device: (N 1e-12 + (N + 8) 2^-53) max_j dist[i, j]   (the posterior's cap times the distances, plus the
                roundings of N products and N - 1 additions; far inside the float32 cap (N + 8) 2^-24 max_j dist[i, j])
    conf        float32 in the kernel: (N + 1) 2^-24   (N posteriors rounded to float32, relative 2^-24 of terms that sum to at most 1,
                and N - 1 additions of partial sums <= 1, each within 2^-24; second-order terms and the posterior's 1e-12 fit
                in the one extra 2^-24)"""
import json
import os

import numpy as np
import pytest
import torch

import ctc_beam_reference as beam_ref
import edit_align_reference as ref
import gram_beam_reference as gram_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JUNK = 77                                               # what the padding holds: an id that occurs in no string below
LENGTHS = (0, 1, 2, 63, 64, 65, 129)                    # around the 64-lane stride of the sweep


def _dev(a, device, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device, dtype)


def _check_alignment(pairs, device, ref_pitch=None, hyp_pitch=None, ref_len=None, hyp_len=None):
    """`pairs`: [(r, h)] as lists.  Pads with JUNK to the pitches, runs edit_alignment with and without paths (with `ref_len` /
    `hyp_len` in place of the true lengths if given) and compares everything with the reference, the distance also with
    _ops.edit_distance.  -> the EditAlignment with paths"""
    from asr import _ops
    from asr.error import edit_alignment
    R, rl = ref.pack([r for r, _ in pairs], ref_pitch, JUNK)
    H, hl = ref.pack([h for _, h in pairs], hyp_pitch, JUNK)
    Rd, Hd = _dev(R, device), _dev(H, device)
    rld, hld = _dev(rl if ref_len is None else ref_len, device), _dev(hl if hyp_len is None else hyp_len, device)
    got = edit_alignment(Rd, rld, Hd, hld)
    bare = edit_alignment(Rd, rld, Hd, hld, paths=False)
    assert bare.ref_to_hyp is None and bare.hyp_to_ref is None
    want = [ref.align(r, h) for r, h in pairs]
    for k, name in enumerate(("distance", "substitutions", "deletions", "insertions")):
        w = np.asarray([x[k] for x in want])
        np.testing.assert_array_equal(getattr(got, name).cpu().numpy(), w, err_msg=name)
        np.testing.assert_array_equal(getattr(bare, name).cpu().numpy(), w, err_msg=name + " without paths")
    assert got.distance.dtype == torch.int32 and got.ref_to_hyp.dtype == torch.int32
    r2h, h2r = got.ref_to_hyp.cpu().numpy(), got.hyp_to_ref.cpu().numpy()
    assert r2h.shape == R.shape and h2r.shape == H.shape
    for p, (_, _, _, _, wr, wh) in enumerate(want):
        assert list(r2h[p, :len(wr)]) == wr and (r2h[p, len(wr):] == -1).all(), p
        assert list(h2r[p, :len(wh)]) == wh and (h2r[p, len(wh):] == -1).all(), p
    old = _ops.edit_distance(Rd, _dev(rl, device), Hd, _dev(hl, device)).cpu().numpy()
    np.testing.assert_array_equal(got.distance.cpu().numpy(), old)
    return got


def _strings(rs, n, m, alphabet):
    """alphabet: a number of symbols, or "distinct": no symbol twice in a string (both drawn from the same 300 ids)"""
    if alphabet == "distinct":
        return (rs.permutation(300)[:n] + 100).tolist(), (rs.permutation(300)[:m] + 100).tolist()
    return rs.randint(1, alphabet + 1, size=n).tolist(), rs.randint(1, alphabet + 1, size=m).tolist()


@pytest.mark.parametrize("alphabet", [2, 50, "distinct"])
def test_lengths_around_the_lane_stride(device, alphabet):
    rs = np.random.RandomState(11)
    _check_alignment([_strings(rs, n, m, alphabet) for n in LENGTHS for m in LENGTHS], device)


def test_long_pairs(device):
    rs = np.random.RandomState(12)
    _check_alignment([_strings(rs, 300, 5, 3)], device)
    _check_alignment([_strings(rs, 5, 300, 3)], device)
    got = _check_alignment([_strings(rs, 2000, 2000, 3)], device)
    assert 0 < int(got.distance[0]) < 2000


def test_identical_and_disjoint_pairs(device):
    rs = np.random.RandomState(13)
    same = [rs.randint(1, 5, size=n).tolist() for n in (1, 64, 130)]
    got = _check_alignment([(s, list(s)) for s in same], device)
    assert (got.distance == 0).all()
    for p, s in enumerate(same):
        assert list(got.ref_to_hyp[p, :len(s)].cpu().numpy()) == list(range(len(s)))
    disjoint = [(rs.randint(1, 5, size=n).tolist(), rs.randint(10, 15, size=m).tolist()) for n, m in ((1, 1), (70, 64), (3, 90), (129, 2))]
    got = _check_alignment(disjoint, device)
    assert list(got.distance.cpu().numpy()) == [max(len(r), len(h)) for r, h in disjoint]
    assert list(got.substitutions.cpu().numpy()) == [min(len(r), len(h)) for r, h in disjoint]


def test_padding_junk_and_length_clamping(device):
    rs = np.random.RandomState(14)
    pairs = [_strings(rs, n, m, 3) for n, m in ((5, 9), (0, 4), (17, 0), (40, 40))]
    tight = _check_alignment(pairs, device)
    wide = _check_alignment(pairs, device, ref_pitch=100, hyp_pitch=70)              # junk ids in the padding
    np.testing.assert_array_equal(wide.ref_to_hyp[:, :40].cpu().numpy(), tight.ref_to_hyp.cpu().numpy())
    assert (wide.ref_to_hyp[:, 40:] == -1).all() and (wide.hyp_to_ref[:, 40:] == -1).all()
    # lengths beyond the pitch are clamped to it, negative lengths are 0
    full = [(r + [JUNK] * (12 - len(r)), h + [JUNK] * (11 - len(h))) for r, h in (_strings(rs, 12, 11, 3), _strings(rs, 7, 11, 3))]
    _check_alignment(full, device, ref_pitch=12, hyp_pitch=11, ref_len=[99, 12], hyp_len=[11, 2 ** 30])
    empty = [([], h) for _, h in pairs]
    _check_alignment(empty, device, ref_pitch=6, ref_len=[-1, -5, 0, -2 ** 31])
    _check_alignment([(r, []) for r, _ in pairs], device, hyp_pitch=3, hyp_len=[-1, 0, -7, -1])
    # a matrix without a column: every reference is empty whatever its length says
    from asr.error import edit_alignment
    H, hl = ref.pack([h for _, h in pairs])
    none = edit_alignment(torch.zeros((4, 0), dtype=torch.int32, device=device), _dev([3, 0, 1, 9], device), _dev(H, device), _dev(hl, device))
    assert list(none.insertions.cpu().numpy()) == list(hl) == list(none.distance.cpu().numpy())
    assert tuple(none.ref_to_hyp.shape) == (4, 0) and (none.hyp_to_ref == -1).all()


def _mixed_pairs():
    rs = np.random.RandomState(15)
    return [_strings(rs, rs.randint(0, 50), rs.randint(0, 45), rs.choice([2, 6])) for _ in range(257)]


def test_many_pairs_in_one_call(device):
    _check_alignment(_mixed_pairs(), device)


def test_budget_split_gives_the_unsplit_result(device, monkeypatch):
    from asr import _lib, error
    pairs = _mixed_pairs()
    whole = _check_alignment(pairs, device)
    R, _ = ref.pack([r for r, _ in pairs])
    H, _ = ref.pack([h for _, h in pairs])
    one = _lib.lib().asr_edit_align_workspace_bytes(1, R.shape[1], H.shape[1])
    assert 0 < 257 * one < error.ALIGN_WORKSPACE_BUDGET                                # the call above was one launch
    monkeypatch.setattr(error, "ALIGN_WORKSPACE_BUDGET", 10 * one + 5)                 # 10 pairs per launch: 26 launches
    split = _check_alignment(pairs, device)
    for a, b in zip(whole, split):
        assert torch.equal(a, b)
    monkeypatch.setattr(error, "ALIGN_WORKSPACE_BUDGET", 1)                            # below one pair: a launch per pair
    _check_alignment(pairs[:9], device)


def test_the_longest_reference_and_the_refusal_beyond(device):
    from asr._lib import AsrHipError
    from asr.error import edit_alignment
    rs = np.random.RandomState(16)
    _check_alignment([_strings(rs, 5460, 3, 3)], device)                   # three diagonals of 5461 ints: 65,532 B of LDS
    zero = torch.zeros((1, 5461), dtype=torch.int32, device=device)
    one = torch.ones((1,), dtype=torch.int32, device=device)
    with pytest.raises(AsrHipError):
        edit_alignment(zero, one, zero[:, :4].contiguous(), one)
    with pytest.raises(AsrHipError):
        edit_alignment(zero, one, zero[:, :4].contiguous(), one, paths=False)


# ------------------------------------------------------------------------------------------------------ pairwise distances
def _ragged_list(rs, B, N, L, symbols=4):
    ids = rs.randint(1, symbols + 1, size=(B, N, L)).astype(np.int32)
    lens = rs.randint(0, L + 1, size=(B, N)).astype(np.int32)
    for b in range(B):
        base = ids[b, 0].copy()                         # near-duplicates of slot 0: small distances among large ones
        for k in range(1, N, 2):
            ids[b, k] = base
            ids[b, k, rs.randint(0, L, size=2)] = rs.randint(1, symbols + 1, size=2)
    lens.flat[rs.choice(B * N, size=max(1, B * N // 5), replace=False)] = 0
    lens.flat[rs.choice(B * N, size=B * N // 4, replace=False)] = rs.choice([-1, -3], size=B * N // 4)
    return ids, lens


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 5, 16])
def test_pairwise_distance(device, B, N):
    from asr import _ops
    rs = np.random.RandomState(100 * B + N)
    L = 37
    ids, lens = _ragged_list(rs, B, N, L)
    idd, lnd = _dev(ids, device), _dev(lens, device)
    got = _ops.nbest_pairwise_distance(idd, lnd)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, N, N)
    g = got.cpu().numpy()
    np.testing.assert_array_equal(g, ref.pairwise(ids, lens))
    np.testing.assert_array_equal(g, g.transpose(0, 2, 1))
    assert (g[:, np.arange(N), np.arange(N)] == 0).all()
    unused = lens < 0
    assert (g[unused] == 0).all() and (g.transpose(0, 2, 1)[unused] == 0).all()
    # the parent commit's route: every ordered pair replicated, one asr_edit_distance pair per copy
    left = idd.repeat_interleave(N, dim=1).reshape(B * N * N, L).contiguous()
    right = idd.repeat(1, N, 1).reshape(B * N * N, L).contiguous()
    ll, rl = lnd.repeat_interleave(N, dim=1).reshape(-1), lnd.repeat(1, N).reshape(-1)
    old = _ops.edit_distance(left, ll.clamp_min(0).contiguous(), right, rl.clamp_min(0).contiguous()).reshape(B, N, N)
    old = torch.where((ll.reshape(B, N, N) < 0) | (rl.reshape(B, N, N) < 0), torch.zeros_like(old), old)
    assert torch.equal(got, old)


# ---------------------------------------------------------------------------------------------------------------- mbr_decode
def _check_mbr(ids, lens, scores, scale, device, exact_index=None, score_dtype=torch.float32):
    """runs mbr_decode on the device and checks every field against the float64 reference -> the MBR tuple"""
    from asr.error import mbr_decode
    ids, lens = np.asarray(ids, np.int32), np.asarray(lens, np.int32)
    sd = torch.from_numpy(np.asarray(scores, np.float64)).to(device, score_dtype)
    got = mbr_decode(_dev(ids, device), _dev(lens, device), sd, scale=scale)
    B, N, L = ids.shape
    want = ref.mbr(ids, lens, sd.double().cpu().numpy(), scale)         # the scores as the device holds them
    used = want["lens"] >= 0
    post, risk, index = got.posterior.cpu().numpy(), got.risk.cpu().numpy(), got.index.cpu().numpy()
    assert got.posterior.dtype == torch.float64 and got.risk.dtype == torch.float64 and got.index.dtype == torch.int32
    assert got.confidence.dtype == torch.float32 and tuple(got.confidence.shape) == (B, L) and tuple(got.ids.shape) == (B, L)
    assert (post[~used] == 0).all() and np.abs(post - want["posterior"]).max() <= 1e-12
    sums = post.sum(axis=1)
    assert (np.abs(sums[used.any(axis=1)] - 1.0) <= N * 2.0 ** -52).all() and (sums[~used.any(axis=1)] == 0).all()
    assert (risk[~used] == np.inf).all()
    cap = (N * 1e-12 + (N + 8) * 2.0 ** -53) * want["dist"].max(axis=2)               # (B, N): per hypothesis i
    assert (np.abs(risk[used] - want["risk"][used]) <= cap[used]).all()
    conf = got.confidence.cpu().numpy()
    out_ids, out_len = got.ids.cpu().numpy(), got.lengths.cpu().numpy()
    for b in range(B):
        if not used[b].any():
            assert index[b] == -1 and out_len[b] == 0 and (conf[b] == 0).all()
            continue
        i = int(index[b])
        assert used[b, i] and want["risk"][b, i] - want["risk"][b][used[b]].min() <= cap[b, i], (b, i)
        assert out_len[b] == want["lens"][b, i] and (out_ids[b] == ids[b, i]).all()
        wc = ref.confidence(ids, want["lens"], want["posterior"], b, i)               # for the pivot the device chose
        assert np.abs(conf[b] - wc).max() <= (N + 1) * 2.0 ** -24, (b, np.abs(conf[b] - wc).max())
        assert (conf[b, out_len[b]:] == 0).all()
    if exact_index is not None:
        assert list(index) == list(exact_index)
    return got


def test_mbr_on_the_hand_made_lists(device):
    ids, lens, scores, want = ref.hand_batch()
    got = _check_mbr(ids, lens, scores, 1.0, device, exact_index=want, score_dtype=torch.float64)
    assert int(got.index[0]) != 0                                    # the runners-up outweigh slot 0
    _check_mbr(ids, lens, scores, 1.0, device, exact_index=want)     # float32 scores, as a search returns them
    from asr.error import mbr_decode
    bare = mbr_decode(_dev(ids, device), _dev(lens, device), torch.from_numpy(scores).to(device), confidence=False)
    assert bare.confidence is None and torch.equal(bare.index, got.index) and torch.equal(bare.risk, got.risk)


def _random_list(N, seed):
    rs = np.random.RandomState(seed)
    B, L = 4, 40
    ids, lens = _ragged_list(rs, B, N, L)
    lens = np.abs(lens)                                              # only the scores say which slots are unused
    scores = rs.randn(B, N) * 2.0
    scores[rs.rand(B, N) < 0.25] = -np.inf
    scores[0, 0], scores[0, 1:] = 0.3, -np.inf                       # one used slot
    if N > 2:
        scores[1] = -np.inf                                          # none
    return ids, lens, scores


@pytest.mark.parametrize("N", [2, 8, 16])
@pytest.mark.parametrize("scale", [0.5, 1.0, 3.0])
def test_mbr_on_random_lists(device, N, scale):
    ids, lens, scores = _random_list(N, 1000 + N)
    _check_mbr(ids, lens, scores, scale, device)


def test_confidence_is_bit_identical_from_run_to_run(device):
    from asr.error import mbr_decode
    ids, lens, scores = _random_list(16, 1016)
    args = (_dev(ids, device), _dev(lens, device), torch.from_numpy(scores).to(device, torch.float32))
    a, b = mbr_decode(*args), mbr_decode(*args)
    assert torch.equal(a.confidence, b.confidence) and torch.equal(a.index, b.index) and torch.equal(a.risk, b.risk)
    assert float(a.confidence.max()) > 0


def test_mbr_on_beam_search_lists(device):
    from asr.error import beam_decode, gram_beam_decode
    T, V, B, W = 40, 8, 3, 8
    rs = np.random.RandomState(21)
    x = np.stack([beam_ref.peaky(rs, T, V) for _ in range(B)], axis=1).astype(np.float32)
    ids, lens, scores = beam_decode(torch.from_numpy(x).to(device), W, V - 1)
    assert tuple(ids.shape) == (B, W, T) and int(torch.isfinite(scores).sum()) > B
    _check_mbr(ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy(), 1.0, device)
    gram = gram_ref.table([(1,), (2,), (3,), (1, 2), (2, 3), (3, 1), (1, 1)])
    assert gram.shape[0] == V
    xg = np.stack([gram_ref.peaky_gram(rs, T, gram) for _ in range(B)], axis=1).astype(np.float32)
    ids, lens, scores = gram_beam_decode(torch.from_numpy(xg).to(device), gram, W, V - 1)
    assert tuple(ids.shape) == (B, W, 2 * T) and int(torch.isfinite(scores).sum()) > B
    _check_mbr(ids.cpu().numpy(), lens.cpu().numpy(), scores.cpu().numpy(), 1.0, device)


# ------------------------------------------------------------------------------------------------------------ error counts
def test_error_counts_reproduce_the_minibatch_error(device):
    from asr import _ops, error, vocab
    with open(os.path.join(GOLD, "text.json"), encoding="utf-8") as f:
        g = json.load(f)
    tok, inv = vocab.get_unigram_ids()
    y, t = np.asarray(g["y"]), np.asarray(g["t"])
    pred, pred_len = _ops.ctc_collapse(_dev(y, device), None, 0, True)
    true, true_len = _ops.ctc_collapse(_dev(t, device), None, 0, False)
    c = error.error_counts(pred, pred_len, true, true_len)
    assert all(v.dtype == torch.int32 and tuple(v.shape) == (len(y),) for v in c)
    dist = _ops.edit_distance(true, true_len, pred, pred_len)
    assert torch.equal(c.substitutions + c.deletions + c.insertions, dist)
    assert torch.equal(c.reference_length, true_len)
    assert torch.equal(c.reference_length - c.deletions + c.insertions, pred_len)
    n = c.reference_length.double()
    per = torch.where(n > 0, dist.double() / n.clamp_min(1), dist.double())
    rate = error.compute_minibatch_error(y, t, 0, tok, inv)
    assert abs(float(per.mean()) - rate) < 1e-12 and abs(rate - g["cer_mean"]) < 1e-12
    totals = error.compute_minibatch_error_counts(y, t, 0, tok, inv)
    assert tuple(totals) == tuple(int(v.sum()) for v in c) and all(isinstance(v, int) for v in totals)
    assert totals.substitutions + totals.deletions + totals.insertions == int(dist.sum()) > 0
