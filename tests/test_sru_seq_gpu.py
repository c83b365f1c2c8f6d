"""asr_sru_seq_fwd / asr_sru_seq_bwd (csrc/sru_seq.hip) against the float64 restatement (tests/sru_seq_reference.py) on the device's own
rounded inputs, element by element, at the smallest shapes that reach every form the dispatch has: one chunk (T < 32) / chunked
(T = 32, 33, a ragged last chunk, the maximal chunk count), two features per lane / one (odd D, operands off their alignment), the
64-lane workgroup width (D = 126 / 128 / 130 with two features per lane, D = 2), the 4-row workgroup height (B = 1, 3, 4, 5).

Caps.  A value's cap is  slack x (error shape) + half a unit of the format it is stored in.  The error shapes are derived in
tests/sru_seq_reference.py (what float32 arithmetic of the kernels' form costs, carried along the recurrence); `slack` is MEASURED, in
this session, on the parent's own kernels: asr_sru_fwd / asr_sru_bwd on the same kind of inputs at ndir = 1, k = 3, full length, where
both layers exist -- the largest ratio (distance to the float64 restatement) / (error shape) over the calibration shapes -- and the new
kernels get twice that (one factor for a different chunk partition).  The fixture prints what it measured and asserts the shapes are
bounds of the parent at all (ratio <= 1).  The cases with saturated gates get a slack of their own, measured the same way on saturated
inputs: the exp's argument scaling, the term that grows with |a|, makes the shapes tighter there, and a sigmoid whose value is a
float32 subnormal may come out as 0 (the shapes say so).  y, gU and gxh are 16-bit: their caps add half a unit of that format at the rounding points
include/asr_hip.h names (one rounding of the float32 sum over directions).  C, cy, dcx and the bias sums are float32 values never
rounded beyond the arithmetic itself.
Measured on an MI355X: see DESIGN.md section 42."""
import ctypes

import numpy as np
import pytest
import torch

import sru_seq_reference as R

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64


def chunks(T, B, D):
    """csrc/sru_seq.hip's seq_chunks"""
    if T < 32:
        return 1
    waves = (B * ((D + 1) // 2) + 63) // 64
    nc = min((2048 + waves - 1) // waves, 32, T // 16)
    if nc < 2:
        return 1
    Tc = (T + nc - 1) // nc
    return (T + Tc - 1) // Tc


class Arena(object):
    """buffers with NaN on both sides (and NaN inside, where the kernels are to write), `misalign` elements off a 256-byte boundary"""

    def __init__(self, device, misalign):
        self.device, self.misalign, self.bufs = device, misalign, []

    def new(self, shape, dtype=F32, init=None):
        n = int(np.prod(shape))
        lead = GUARD + self.misalign
        whole = torch.full((lead + n + GUARD,), float("nan"), dtype=dtype, device=self.device)
        t = whole[lead:lead + n].view(*shape)
        assert whole.data_ptr() % 256 == 0 and t.is_contiguous()
        if init is not None:
            t.copy_(torch.as_tensor(init).to(dtype))
        self.bufs.append((whole, lead, n))
        return t

    def check(self):
        torch.cuda.synchronize()
        for whole, lead, n in self.bufs:
            assert bool(torch.isnan(whole[:lead]).all()) and bool(torch.isnan(whole[lead + n:]).all()), "a write outside a buffer"


def _lib():
    from asr import _lib
    return _lib


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _inputs(seed, T, B, D, k, ndir, saturate=False):
    rs = np.random.RandomState(seed)
    U = rs.randn(T, B, ndir, k, D)
    U[:, :, :, 1:3] *= 0.9
    if saturate:            # |U_f| up to ~200: f is exactly 0 or 1 on most frames, in float32 as in float64 to 2^-53
        U[:, :, :, 1] *= 60.0
    return dict(U=U.astype(np.float32), x=rs.randn(T, B, D), bias=(0.3 * rs.randn(ndir, 2 * D)).astype(np.float32),
                cx=rs.randn(ndir, B, D).astype(np.float32), gy=rs.randn(T, B, D), dcy=rs.randn(ndir, B, D).astype(np.float32),
                gb0=rs.randn(ndir, 2 * D).astype(np.float32))


def _call_fwd(A, dev, inp, T, B, D, k, ndir, x_len, use_tanh, with_cx, ws_bytes=None):
    L = _lib()
    p = L.ptr
    need = int(L.lib().asr_sru_seq_ws_bytes(T, B, D, ndir))
    assert need == (2 * ndir * chunks(T, B, D) * B * D * 4 if chunks(T, B, D) > 1 else 0)
    t = dict(U=A.new((T * B, ndir * k * D), F32, inp["U"].reshape(T * B, -1)), bias=A.new((ndir, 2 * D), F32, inp["bias"]),
             x=A.new((T, B, D), BF16, inp["x"]) if k == 3 else None, cx=A.new((ndir, B, D), F32, inp["cx"]) if with_cx else None,
             y=A.new((T, B, D), BF16), C=A.new((ndir, T, B, D), F32), cy=A.new((ndir, B, D), F32),
             ws=A.new((max(need, 4) // 4,), F32), n=None if x_len is None else torch.tensor(x_len, dtype=torch.int32, device=dev))
    rc = L.lib().asr_sru_seq_fwd(L.stream(), p(t["x"]), p(t["U"]), p(t["bias"]), p(t["cx"]), p(t["n"]), p(t["y"]), p(t["C"]), p(t["cy"]),
                                 T, B, D, k, ndir, int(use_tanh), p(t["ws"]), need if ws_bytes is None else ws_bytes)
    return rc, t


def _call_bwd(A, dev, inp, t, T, B, D, k, ndir, use_tanh, with_dcy):
    L = _lib()
    p = L.ptr
    need = int(L.lib().asr_sru_seq_ws_bytes(T, B, D, ndir))
    t.update(gy=A.new((T, B, D), BF16, inp["gy"]), dcy=A.new((ndir, B, D), F32, inp["dcy"]) if with_dcy else None,
             gU=A.new((T * B, ndir * k * D), BF16), gxh=A.new((T, B, D), BF16) if k == 3 else None,
             gb=A.new((ndir, 2 * D), F32, inp["gb0"]), dcx=A.new((ndir, B, D), F32))
    rc = L.lib().asr_sru_seq_bwd(L.stream(), p(t["x"]), p(t["U"]), p(t["bias"]), p(t["C"]), p(t["cx"]), p(t["n"]), p(t["gy"]), p(t["dcy"]),
                                 p(t["gU"]), p(t["gxh"]), p(t["gb"]), p(t["dcx"]), T, B, D, k, ndir, int(use_tanh), p(t["ws"]), need)
    return rc


def _inside(got, want, cap, what):
    bad = ~(np.abs(got - want) <= cap)
    assert not bad.any(), "%s: %d of %d outside, worst %.3g caps at %s" % (
        what, bad.sum(), bad.size, np.nanmax(np.abs(got - want) / cap), np.unravel_index(np.nanargmax(np.abs(got - want) / cap), got.shape))


# ------------------------------------------------------------------------------------------------ the slack, from the parent's kernels
@pytest.fixture(scope="module")
def slack(device):
    """{saturated gates?: (forward, backward)} = twice the parent kernels' own largest distance to the restatement, in units of the error
    shapes, on the two kinds of inputs the cases use"""
    from asr import _ops
    worst = {False: [0.0, 0.0], True: [0.0, 0.0]}
    shapes = [(64, 4, 128), (33, 3, 130), (200, 2, 64), (31, 5, 126), (5, 4, 512), (50, 3, 7)]
    # The first three once more with saturated gates (|U_f| up to ~200), as the saturated cases have them, for a slack of their own: the
    # exp's argument scaling, the term that grows with |a|, makes the shapes tighter there.  These are the shapes the parent serves with
    # its chunked kernels, whose sigmoid is the new kernels' rcp(1 + __expf(-a)); its one-thread-per-column kernels (T < 32, odd D) form
    # it as tanhf(a / 2) / 2 + 1 / 2, which cancels in the tails (an absolute 2^-24 where f ~ 1e-9) and is no yardstick for the shapes there.
    for seed, (T, B, D) in enumerate(shapes + shapes[:3]):
        for use_tanh in (True, False):
            saturate = seed >= len(shapes)
            inp = _inputs(100 + seed, T, B, D, 3, 1, saturate)
            x = torch.tensor(inp["x"], device=device).to(BF16)
            U = torch.tensor(inp["U"].reshape(T * B, 3 * D), device=device)
            bias, c0 = torch.tensor(inp["bias"][0], device=device), torch.tensor(inp["cx"][0], device=device)
            gy, gcT = torch.tensor(inp["gy"], device=device).to(BF16), torch.tensor(inp["dcy"][0], device=device)
            gb = torch.tensor(inp["gb0"][0], device=device)
            H, C, cT = _ops.sru_fwd(x, U, bias, c0, None, use_tanh)
            gU, gxh, gc0 = _ops.sru_bwd(x, U, bias, C, c0, None, gy, gcT, gb, use_tanh)
            torch.cuda.synchronize()
            args = (inp["U"].astype(np.float64), _np(x), inp["bias"], inp["cx"][:1])
            y, Cr, cy, (Ey, EC, Ecy) = R.scan_fwd(*args, None, use_tanh, bounds=True)

            def ratio(got, want, E, bits=7):
                """the distance beyond the stored format's half unit, in units of the error shape: what `slack` multiplies in a cap"""
                return ((np.abs(got - want) - R.half_unit(np.abs(want) + E, bits)) / (E + 2.0 ** -140)).max()
            f = max(ratio(_np(C), Cr[0], EC[0], 23), ratio(_np(cT), cy[0], Ecy[0], 23), ratio(_np(H), y, Ey))
            gUr, gxr, gbr, dcr, (EgU, Egx, Egb, Edc) = R.scan_bwd(*args[:3], _np(C)[None], args[3], None, _np(gy), inp["dcy"][:1], use_tanh,
                                                                  bounds=True)
            gUd = _np(gU).reshape(T, B, 1, 3, D)
            b = max(ratio(gUd, gUr, EgU), ratio(_np(gxh), gxr, Egx), ratio(_np(gc0), dcr[0], Edc[0], 23),
                    ratio(_np(gb) - inp["gb0"][0], gbr[0], Egb[0] + 2 * R.half_unit(_np(gb), 23), 23))
            print("parent asr_sru_fwd / asr_sru_bwd at T=%d B=%d D=%d tanh=%d saturated=%d: %.3f / %.3f of the error shapes"
                  % (T, B, D, use_tanh, saturate, f, b))
            worst[saturate] = [max(worst[saturate][0], f), max(worst[saturate][1], b)]
    for saturate, (f, b) in worst.items():
        print("slack (twice the parent's), saturated=%d: forward %.3f, backward %.3f" % (saturate, 2 * f, 2 * b))
        assert 0 < f <= 1 and 0 < b <= 1
    return {saturate: (2 * f, 2 * b) for saturate, (f, b) in worst.items()}


# ------------------------------------------------------------------------------------------------ one case, every output
def _run(device, slack, seed, T, B, D, k, ndir, x_len, use_tanh=True, with_cx=True, misalign=0, saturate=False, with_dcy=True):
    sf, sb = slack[bool(saturate)]
    A = Arena(device, misalign)
    inp = _inputs(seed, T, B, D, k, ndir, saturate)
    rc, t = _call_fwd(A, device, inp, T, B, D, k, ndir, x_len, use_tanh, with_cx)
    assert rc == 0
    A.check()
    x64 = _np(t["x"]) if k == 3 else None
    cx = inp["cx"] if with_cx else None
    y, C, cy, (Ey, EC, Ecy) = R.scan_fwd(inp["U"], x64, inp["bias"], cx, x_len, use_tanh, bounds=True)
    n = R.lengths(x_len, T, B)
    live = np.arange(T)[:, None] < n[None, :]                           # (T, B)
    Cd, yd = _np(t["C"]), _np(t["y"])
    assert np.isnan(Cd[:, ~live]).all(), "C is not written in the padding"
    assert (t["y"].view(torch.int16).cpu().numpy()[~live] == 0).all(), "the padding of y is exactly zero"
    _inside(Cd[:, live], C[:, live], sf * EC[:, live] + R.half_unit(C[:, live], 23), "C")
    _inside(_np(t["cy"]), cy, sf * Ecy + R.half_unit(cy, 23), "cy")
    _inside(yd[live], y[live], sf * Ey[live] + R.half_unit(np.abs(y[live]) + sf * Ey[live]), "y")
    for b in np.nonzero(n == 0)[0]:                                     # x_len = 0: cy = cx on bits
        want = t["cx"][:, b] if with_cx else torch.zeros_like(t["cy"][:, b])
        assert torch.equal(t["cy"][:, b].view(torch.int32), want.view(torch.int32))
    # backward, from the device's own saved states
    rc = _call_bwd(A, device, inp, t, T, B, D, k, ndir, use_tanh, with_dcy)
    assert rc == 0
    A.check()
    gyd = _np(t["gy"])
    gU, gxh, gb, dcx, (EgU, Egx, Egb, Edc) = R.scan_bwd(inp["U"], x64, inp["bias"], Cd, cx, x_len, gyd, inp["dcy"] if with_dcy else None,
                                                        use_tanh, bounds=True)
    gUd = _np(t["gU"]).reshape(T, B, ndir, k, D)
    assert (t["gU"].view(torch.int16).cpu().numpy().reshape(T, B, -1)[~live] == 0).all(), "gU is exactly zero in the padding"
    _inside(gUd[live], gU[live], sb * EgU[live] + R.half_unit(np.abs(gU[live]) + sb * EgU[live]), "gU")
    if k == 3:
        assert (t["gxh"].view(torch.int16).cpu().numpy()[~live] == 0).all(), "gxh is exactly zero in the padding"
        _inside(_np(t["gxh"])[live], gxh[live], sb * Egx[live] + R.half_unit(np.abs(gxh[live]) + sb * Egx[live]), "gxh")
    _inside(_np(t["dcx"]), dcx, sb * Edc + R.half_unit(dcx, 23), "dcx")
    _inside(_np(t["gb"]) - inp["gb0"], gb, sb * Egb + 2 * R.half_unit(_np(t["gb"]), 23) + R.half_unit(inp["gb0"], 23), "gbias")
    for b in np.nonzero(n == 0)[0]:                                     # and dcx = dcy
        want = t["dcy"][:, b] if with_dcy else torch.zeros_like(t["dcx"][:, b])
        assert torch.equal(t["dcx"][:, b].view(torch.int32), want.view(torch.int32))
    return t


def _length_kinds(T, B, D):
    """None, the edges, ragged around the first chunk boundary, entries outside 0 .. T (clamped)"""
    nc = chunks(T, B, D)
    Tc = (T + nc - 1) // nc
    edge = [0, 1, T - 1, T, T // 2]
    ragged = [Tc - 1, Tc, Tc + 1, 2 * Tc, 0]
    beyond = [T + 3, -2, T, 1, T - 1]
    fit = lambda v: [min(max(e, 0), T) for e in (v * 2)[:B]]
    return [None, fit(edge), fit(ragged), (beyond * 2)[:B]]


SHAPES = [(1, 1, 2), (2, 3, 126), (3, 4, 128), (4, 5, 130), (5, 3, 7), (31, 4, 128), (32, 3, 126), (33, 5, 130), (50, 4, 128), (50, 3, 7),
          (512, 1, 2), (40, 2, 512), (33, 1, 512)]


@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-B%d-D%d" % s)
def test_every_output_against_the_restatement(device, slack, shape, k, ndir):
    T, B, D = shape
    for i, x_len in enumerate(_length_kinds(T, B, D)):
        _run(device, slack, 7 * i + k + ndir, T, B, D, k, ndir, x_len, use_tanh=(i + k) % 2 == 0, with_cx=(i + ndir) % 2 == 0,
             with_dcy=i % 2 == 0)


@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("shape", [(5, 3, 126), (50, 5, 130), (33, 4, 128)], ids=lambda s: "T%d-B%d-D%d" % s)
def test_two_alignments_and_saturated_gates(device, slack, shape, misalign, k, ndir):
    """operands one element off their boundary run one feature per lane; |U_f| up to ~200 puts f at exactly 0 or 1"""
    T, B, D = shape
    kinds = _length_kinds(T, B, D)
    for i, saturate in enumerate((False, True)):
        _run(device, slack, 31 + i, T, B, D, k, ndir, kinds[2 - i], use_tanh=True, with_cx=True, misalign=misalign, saturate=saturate)
        _run(device, slack, 41 + i, T, B, D, k, ndir, kinds[i], use_tanh=False, with_cx=bool(i), misalign=misalign, saturate=saturate)


def test_a_state_of_negative_zero_and_subnormals_is_handed_on(device, slack):
    T, B, D, ndir = 40, 3, 128, 2
    inp = _inputs(3, T, B, D, 3, ndir)
    inp["cx"][:, 0, :4] = [-0.0, 1e-41, -1e-41, 0.0]
    A = Arena(device, 0)
    rc, t = _call_fwd(A, device, inp, T, B, D, 3, ndir, [0, T, 5], True, True)
    assert rc == 0
    A.check()
    assert torch.equal(t["cy"][:, 0].view(torch.int32), t["cx"][:, 0].view(torch.int32))


# ------------------------------------------------------------------------------------------------ the carried state
def _pieces(device, T, B, D, k, ndir, cuts, x_len):
    inp = _inputs(17, T, B, D, k, 1)
    A = Arena(device, 0)
    rc, whole = _call_fwd(A, device, inp, T, B, D, k, 1, x_len, True, True)
    assert rc == 0
    state, ys = inp["cx"], []
    for lo, hi in zip((0,) + cuts, cuts + (T,)):
        part = dict(inp, U=inp["U"][lo:hi], x=inp["x"][lo:hi], cx=state)
        n = [min(max(v - lo, 0), hi - lo) for v in x_len]
        rc, t = _call_fwd(A, device, part, hi - lo, B, D, k, 1, n, True, True)
        assert rc == 0
        state = t["cy"].cpu().numpy()
        ys.append(t["y"])
    A.check()
    return whole, torch.cat(ys), torch.tensor(state, device=device), inp


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("T, cuts", [(5, (1, 2)), (31, (7, 8, 20))])
def test_pieces_with_the_state_carried_equal_the_whole_on_bits(device, T, cuts, k):
    """below 32 frames the whole and every piece are one chunk each: the same arithmetic in the same order (what a stream's chunks are)"""
    x_len = [T, 3, 0, T - 1]
    whole, y, cy, _ = _pieces(device, T, 4, 130, k, 1, cuts, x_len)
    assert torch.equal(y.view(torch.int16), whole["y"].view(torch.int16))
    assert torch.equal(cy.view(torch.int32), whole["cy"].view(torch.int32))


def test_pieces_against_a_chunked_whole(device, slack):
    """T = 64 runs as 4 chunks whose entry states are folded summaries (P c + S), pieces of 16 run as one chunk each: another order of
    roundings, so not equal on bits -- both within their caps of the restatement, and the distance between them is printed
    (measured on an MI355X: 19 of 512 elements of cy differ, by at most 1.19e-7 = 0.45 caps)"""
    T, B, D = 64, 4, 128
    assert chunks(T, B, D) == 4
    x_len = [T, 17, 0, 47]
    whole, y, cy, inp = _pieces(device, T, B, D, 3, 1, (16, 32, 48), x_len)
    _, _, ref, (_, _, Ecy) = R.scan_fwd(inp["U"], _np(whole["x"]), inp["bias"], inp["cx"], x_len, True, bounds=True)
    cap = slack[False][0] * Ecy + R.half_unit(ref, 23)
    _inside(_np(cy), ref, cap, "cy of the pieces")
    _inside(_np(whole["cy"]), ref, cap, "cy of the whole")
    d = np.abs(_np(cy) - _np(whole["cy"]))
    print("pieces vs chunked whole, cy: max %.3g (%.2f caps), %d of %d elements differ" % (d.max(), (d / cap).max(), (d > 0).sum(), d.size))
    assert (y.view(torch.int16) != whole["y"].view(torch.int16)).float().mean().item() < 0.05       # (16-bit y: a rounding flip is rare)


# ------------------------------------------------------------------------------------------------ autograd: functions.sru_seq, the links
@pytest.mark.parametrize("I, D, ndir, T", [(64, 64, 1, 20), (64, 64, 2, 40), (40, 64, 1, 40), (40, 64, 2, 20)])
def test_autograd_through_the_links(device, slack, I, D, ndir, T):
    """The link's output is, on bits, the kernel's on the projection the link forms; its gradients are the restatement's scan from the
    device's own U and C followed by the two products, each 16-bit gU element worth half a unit: |gW - ref| <= 2^-8 |gU|^T |x| (+ the
    scan's own caps through the same product), gx likewise through |W| plus the roundings of its 16-bit terms."""
    from asr import _ops, nn
    B = 3
    k = 3 if I == D else 4
    torch.manual_seed(5)
    link = (nn.BiSeqSRU if ndir == 2 else nn.SeqSRU)(D).to(device)
    x = torch.randn(B, I, T, device=device).to(BF16).requires_grad_(True)
    hx = torch.randn(ndir, B, D, device=device).requires_grad_(True)
    x_len = torch.tensor([T, 0, T - 3], dtype=torch.int32, device=device)
    y, hy = link(x, x_len, hx)
    assert link.k == k and tuple(link.W.shape) == (ndir, k * D, I) and tuple(y.shape) == (B, D, T) and tuple(hy.shape) == (ndir, B, D)
    with torch.no_grad():
        link.B.copy_(0.3 * torch.randn_like(link.B))
    y, hy = link(x, x_len, hx)
    gy = torch.randn(B, D, T, device=device).to(BF16)
    dcy = torch.randn(ndir, B, D, device=device)
    ((y.float() * gy.float()).sum() + (hy * dcy).sum()).backward()
    # the same projection and scan, called directly
    xp = x.detach().permute(2, 0, 1).contiguous()
    w16 = _ops.cast_bf16(link.W.detach().reshape(-1, I))
    U = _ops.gemm_nt(xp.reshape(T * B, I), w16, None, F32)
    yk, Ck, cyk = _ops.sru_seq_fwd(xp if k == 3 else None, U, link.B.detach(), hx.detach(), x_len, T, B, D, k, ndir, True)
    assert torch.equal(y.detach().permute(2, 0, 1).contiguous().view(torch.int16), yk.view(torch.int16))
    assert torch.equal(hy.detach().view(torch.int32), cyk.view(torch.int32))
    U64, x64, W64 = _np(U).reshape(T, B, ndir, k, D), _np(xp), _np(w16).reshape(ndir * k * D, I)
    exact = x64.reshape(T * B, I) @ W64.T
    assert np.all(np.abs(_np(U) - exact) <= (I + 8) * 2.0 ** -24 * (np.abs(x64.reshape(T * B, I)) @ np.abs(W64.T)) + 2.0 ** -126)
    n = x_len.cpu().numpy()
    gyp = _np(gy.permute(2, 0, 1))
    gU, gxh, gb, dcx, (EgU, Egx, Egb, Edc) = R.scan_bwd(U64, x64 if k == 3 else None, _np(link.B), _np(Ck), _np(hx), n, gyp, _np(dcy), True,
                                                        bounds=True)
    sb = slack[False][1]
    g2, e2 = gU.reshape(T * B, -1), (2.0 ** -8 * np.abs(gU) + sb * EgU).reshape(T * B, -1)
    x2 = x64.reshape(T * B, I)
    roundoff = (T * B + 8) * 2.0 ** -24
    _inside(_np(link.W.grad).reshape(-1, I), g2.T @ x2, e2.T @ np.abs(x2) + roundoff * (np.abs(g2).T @ np.abs(x2)) + 2.0 ** -126, "gW")
    _inside(_np(link.B.grad), gb, sb * Egb + 2 * R.half_unit(gb, 23) + 2.0 ** -126, "gB")
    _inside(_np(hx.grad), dcx, sb * Edc + R.half_unit(dcx, 23), "dcx")
    gproj = g2 @ W64
    cap = e2 @ np.abs(W64) + roundoff * (np.abs(g2) @ np.abs(W64)) + 2.0 ** -8 * np.abs(gproj)
    want = gproj
    if k == 3:
        want = gproj + gxh.reshape(T * B, D)
        cap = cap + (2.0 ** -8 * np.abs(gxh) + sb * Egx).reshape(T * B, D) + 2.0 ** -8 * np.abs(want)
    got = _np(x.grad.permute(2, 0, 1)).reshape(T * B, I)
    _inside(got, want, cap + 2.0 ** -126, "gx")
    assert (got.reshape(T, B, I)[:, 1] == 0).all() and (got.reshape(T, B, I)[T - 3:, 2] == 0).all()      # the padding passes no gradient
    # without hx the call returns y alone, from a zero state
    y0 = link(x.detach(), x_len)
    yz, _ = link(x.detach(), x_len, torch.zeros_like(hx))
    assert torch.equal(y0.view(torch.int16), yz.view(torch.int16))


def test_functions_sru_seq_refuses_wrong_shapes(device):
    from asr import functions, nn
    link = nn.SeqSRU(48, 64).to(device)
    x = torch.zeros(2, 48, 6, device=device).to(BF16)
    with pytest.raises(ValueError, match="cx must have shape"):
        link(x, None, torch.zeros(2, 2, 64, device=device))
    with pytest.raises(ValueError, match="k = 4"):              # 48 -> 64 units takes the projected highway: four blocks
        functions.sru_seq(x, torch.nn.Parameter(link.W[:, :192].detach().clone()), link.B, link, 1)
    with pytest.raises(ValueError, match="W must be"):
        functions.sru_seq(torch.zeros(2, 64, 6, device=device).to(BF16), link.W, link.B, link, 1)
    with pytest.raises(ValueError, match="W must be"):
        functions.sru_seq(x, link.W, link.B, link, 2)
    # x_length as the GRU links take it: (B) int32 on the device, or refused before anything is launched
    for bad in (torch.tensor([6, 3], device=device), torch.tensor([6], dtype=torch.int32, device=device),
                torch.tensor([6, 3, 1], dtype=torch.int32, device=device), torch.tensor([6, 3], dtype=torch.int32)):
        with pytest.raises(ValueError, match="x_length must be"):
            link(x, bad)
        with pytest.raises(ValueError, match="x_length must be"):
            link(x, bad, torch.zeros(1, 2, 64, device=device))
    y = link(x, torch.tensor([6, 3], dtype=torch.int32, device=device))
    assert tuple(y.shape) == (2, 64, 6) and bool((y[1, :, 3:] == 0).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(device):
    L = _lib()
    T, B, D = 40, 2, 64
    assert chunks(T, B, D) > 1
    inp = _inputs(1, T, B, D, 3, 1)
    A = Arena(device, 0)
    rc, t = _call_fwd(A, device, inp, T, B, D, 3, 1, None, True, True)
    assert rc == 0
    p, lib, st = L.ptr, L.lib(), L.stream()
    need = int(lib.asr_sru_seq_ws_bytes(T, B, D, 1))
    assert need > 0 and lib.asr_sru_seq_ws_bytes(0, B, D, 1) == 0 and lib.asr_sru_seq_ws_bytes(T, B, D, 3) == 0

    def fwd(T=T, B=B, D=D, k=3, ndir=1, ws=t["ws"], ws_bytes=need, **none):
        a = {name: (None if name in none else p(t[name])) for name in ("x", "U", "bias", "cx", "y", "C", "cy")}
        return lib.asr_sru_seq_fwd(st, a["x"], a["U"], a["bias"], a["cx"], None, a["y"], a["C"], a["cy"], T, B, D, k, ndir, 1,
                                   None if ws is None else p(ws), ws_bytes)
    for kw in (dict(T=0), dict(B=0), dict(D=-1), dict(k=2), dict(k=5), dict(ndir=0), dict(ndir=3), dict(U=1), dict(bias=1), dict(y=1),
               dict(C=1), dict(cy=1), dict(x=1)):
        assert fwd(**kw) == -1, kw
    assert fwd(ws=None) == -2 and fwd(ws_bytes=need - 1) == -2
    assert fwd(cx=1) == 0                                   # (cx is optional; x is not read for k = 4)
    rc = _call_bwd(A, device, inp, t, T, B, D, 3, 1, True, True)
    assert rc == 0

    def bwd(T=T, k=3, ndir=1, ws_bytes=need, **none):
        a = {name: (None if name in none else p(t[name])) for name in ("x", "U", "bias", "C", "cx", "gy", "dcy", "gU", "gxh", "gb", "dcx")}
        return lib.asr_sru_seq_bwd(st, a["x"], a["U"], a["bias"], a["C"], a["cx"], None, a["gy"], a["dcy"], a["gU"], a["gxh"], a["gb"],
                                   a["dcx"], T, B, D, k, ndir, 1, p(t["ws"]), ws_bytes)
    for kw in (dict(T=0), dict(k=6), dict(ndir=3), dict(U=1), dict(bias=1), dict(C=1), dict(gy=1), dict(gU=1), dict(gb=1), dict(x=1), dict(gxh=1)):
        assert bwd(**kw) == -1, kw
    assert bwd(ws_bytes=8) == -2
    A.check()


def test_the_half_build_refuses():
    import os
    from conftest import PKG
    half = ctypes.CDLL(os.path.join(PKG, "libasr_hip_f16.so"))
    half.asr_sru_seq_fwd.restype = half.asr_sru_seq_bwd.restype = ctypes.c_int
    assert half.asr_sru_seq_fwd(*([None] * 9), 4, 1, 2, 3, 1, 1, None, ctypes.c_size_t(0)) == -3
    assert half.asr_sru_seq_bwd(*([None] * 13), 4, 1, 2, 3, 1, 1, None, ctypes.c_size_t(0)) == -3
