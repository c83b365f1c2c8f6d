"""oracle/gru_step.py pinned before it judges a kernel -- CPU only.

1. The steps chained free-running with no rounding point are torch's GRU in float64 (output and every gradient), with lengths they are
   pack_padded_sequence's semantics (oracle.bf16.gru_f32), with the rounding points on they are oracle.bf16.GRUMatched.
2. The caps can tell right from wrong ON THE INPUTS OF EVERY CASE of tests/test_gru_edges_gpu.py: the same step evaluated in float32
   stays within a quarter of the cap for every element, and a kernel that dropped one 32-wide K slice -- any one, for any
   (direction, 16-unit workgroup slice) -- lands outside the cap in at least one compared output of that slice.
   The device tensors a GPU run would hand to the reference (states, gates, dgh) are stood in for by the rounding-matched chain."""
import numpy as np
import pytest
import torch

import gru_edge_cases as E
from oracle import bf16 as Q
from oracle import gru_step as S

F64 = torch.float64


def _problem(T, B, I, H, ndir, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(H)
    P = dict(w_ih=torch.empty(ndir, 3 * H, I, dtype=F64).uniform_(-k, k, generator=g), w_hh=torch.empty(ndir, 3 * H, H, dtype=F64).uniform_(-k, k, generator=g),
             b_ih=torch.empty(ndir, 3 * H, dtype=F64).uniform_(-k, k, generator=g), b_hh=torch.empty(ndir, 3 * H, dtype=F64).uniform_(-k, k, generator=g))
    x = torch.randn(T, B, I, dtype=F64, generator=g)
    dy = torch.randn(T, B, H, dtype=F64, generator=g)
    return P, x, dy


def _chain(P, x, dy, T, B, I, H, ndir, **kw):
    gi = torch.cat([x.reshape(T * B, I) @ P["w_ih"][d].t() + P["b_ih"][d] for d in range(ndir)], dim=1)
    res = S.free_run(gi, P["w_hh"], P["b_hh"].reshape(-1), dy.reshape(T * B, H), T, B, H, ndir, **kw)
    dgi = res["dgi"].reshape(T * B, ndir, 3 * H)
    dgh = res["dgh"].reshape(T, B, ndir, 3 * H)
    hs = res["hseq"].reshape(T, B, ndir, H)
    out = dict(y=res["y"].reshape(T, B, H), dx=sum(dgi[:, d] @ P["w_ih"][d] for d in range(ndir)).reshape(T, B, I),
               w_ih=torch.stack([dgi[:, d].t() @ x.reshape(T * B, I) for d in range(ndir)]), b_ih=res["db_ih"].reshape(ndir, 3 * H),
               b_hh=res["db_hh"].reshape(ndir, 3 * H))
    whh = []
    for d in range(ndir):       # h_{t-1} pairs with step t (direction 1: h_{t+1})
        a, hb = (dgh[1:, :, d], hs[:-1, :, d]) if d == 0 else (dgh[:-1, :, d], hs[1:, :, d])
        whh.append(a.reshape(-1, 3 * H).t() @ hb.reshape(-1, H))
    out["w_hh"] = torch.stack(whh)
    return out


@pytest.mark.parametrize("T,B,I,H,ndir", [(7, 3, 24, 32, 1), (6, 4, 16, 96, 2), (1, 2, 8, 32, 2)])
def test_free_running_steps_are_torchs_gru_in_float64(T, B, I, H, ndir):
    """cap: every output is a sum of at most T (H + I + 16) float64 products of O(1) values, each operation good to 2^-53: 64 x that
    count x 2^-53 x the largest magnitude (the factor 64 covers exp / tanh in two libraries and a different summation order)"""
    P, x, dy = _problem(T, B, I, H, ndir, seed=T * H + ndir)
    got = _chain(P, x, dy, T, B, I, H, ndir)
    ref = torch.nn.GRU(I, H, bidirectional=ndir == 2).double()
    sufs = ["", "_reverse"][:ndir]
    with torch.no_grad():
        for d, s in enumerate(sufs):
            for n, v in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
                getattr(ref, n + s).copy_(P[v][d])
    xr = x.clone().requires_grad_(True)
    yr, _ = ref(xr)
    yr = yr if ndir == 1 else yr[..., :H] + yr[..., H:]
    yr.backward(dy)
    want = dict(y=yr.detach(), dx=xr.grad)
    for n, v in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
        want[v] = torch.stack([getattr(ref, n + s).grad for s in sufs])
    for name in want:
        cap = 64 * T * (H + I + 16) * 2.0 ** -53 * max(1.0, float(want[name].abs().max()))
        err = float((got[name] - want[name]).abs().max())
        assert err <= cap, (name, err, cap)


@pytest.mark.parametrize("ndir", [1, 2])
def test_lengths_are_packed_sequence_semantics(ndir):
    """against oracle.bf16.gru_f32 (float32 pack_padded_sequence): outputs zero beyond the length, the reverse direction starting from a
    zero state at x_len - 1, no gradient into the padding; an utterance with x_len = 0 (which pack_padded_sequence refuses) is all
    padding: zero output, zero gradient, and the others as if it were not there.  cap: float32 rounding of the comparison side,
    T (H + I + 16) operations x 2^-24 x 8"""
    T, B, I, H = 7, 5, 16, 32
    P, x, dy = _problem(T, B, I, H, ndir, seed=77 + ndir)
    x_len = torch.tensor([7, 1, 0, 4, 6], dtype=torch.int32)
    got = _chain(P, x, dy, T, B, I, H, ndir, x_len=x_len)
    rows = [0, 1, 3, 4]
    p32 = {k: v.float().requires_grad_(True) for k, v in P.items()}
    xr = x[:, rows].float().requires_grad_(True)
    yr = Q.gru_f32(xr, p32["w_ih"], p32["w_hh"], p32["b_ih"], p32["b_hh"], x_len[rows])
    yr.backward(dy[:, rows].float())
    cap = 8 * T * (H + I + 16) * 2.0 ** -24
    assert float((got["y"][:, rows] - yr.detach()).abs().max()) <= cap
    assert float((got["dx"][:, rows] - xr.grad).abs().max()) <= cap * max(1.0, float(xr.grad.abs().max()))
    for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
        assert float((got[name] - p32[name].grad).abs().max()) <= cap * max(1.0, float(p32[name].grad.abs().max())), name
    assert float(got["y"][:, 2].abs().max()) == 0.0 and float(got["dx"][:, 2].abs().max()) == 0.0
    live = (torch.arange(T).reshape(T, 1) < x_len.reshape(1, B)).unsqueeze(2)
    assert float(got["y"][~live.expand_as(got["y"])].abs().max()) == 0.0
    assert float(got["dx"][~live.expand(T, B, I)].abs().max()) == 0.0


@pytest.mark.parametrize("gi_bf16,gates_f16,ps,lens", [(False, False, 0, None), (True, True, 32, None), (True, False, 32, [6, 1, 3, 0, 5]),
                                                       (False, True, 0, [6, 6, 2, 1, 4])])
def test_rounding_points_reproduce_the_matched_oracle(gi_bf16, gates_f16, ps, lens):
    """GRUMatched computes in float32, the chain in float64 between the same rounding points: they agree to float32 rounding except
    where a value sat within that of a bf16 tie and rounded the other way -- one bf16 unit of that element (2^-8 relative), whose
    consequences downstream are of the same size.  cap: one bf16 unit at the summed magnitudes per element, and 99 % of all elements
    within 2^-16 of them (float32 rounding of a T (H + I)-term chain)"""
    T, B, I, H, ndir = 6, 5, 32, 128, 2
    P, x, dy = _problem(T, B, I, H, ndir, seed=5)
    rnd = lambda t: t.float().to(torch.bfloat16).to(F64)
    x, dy = rnd(x), rnd(dy)
    P["w_hh"], P["w_ih"] = rnd(P["w_hh"]), rnd(P["w_ih"])
    P = {k: v.float().double() for k, v in P.items()}
    x_len = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    gi = torch.cat([(x.reshape(T * B, I).float() @ P["w_ih"][d].float().t() + P["b_ih"][d].float()) for d in range(ndir)], dim=1)
    if gi_bf16:
        gi = gi.to(torch.bfloat16).float()
    res = S.free_run(gi, P["w_hh"], P["b_hh"].reshape(-1), dy.reshape(T * B, H), T, B, H, ndir, x_len=x_len, rounding=True,
                     gates_fmt="f16" if gates_f16 else "f32", ps_units=ps, gi_bf16=gi_bf16)
    p32 = {k: v.float().requires_grad_(True) for k, v in P.items()}
    xr = x.float().requires_grad_(True)
    ym = Q.GRUMatched.apply(xr, p32["w_ih"], p32["w_hh"], p32["b_ih"], p32["b_hh"], gi_bf16, ps, x_len, gates_f16)
    ym.backward(dy.float())
    # dgi and dgh -- what the GPU file judges -- through everything GRUMatched forms from them: dx, dW_ih, dW_hh and the bias sums
    dgi, dgh = res["dgi"].reshape(T * B, ndir, 3 * H), res["dgh"].reshape(T, B, ndir, 3 * H)
    hs, x2 = res["hseq"].reshape(T, B, ndir, H), x.reshape(T * B, I)
    dx = S.bf16r(sum(dgi[:, d] @ P["w_ih"][d] for d in range(ndir)))
    dx_mag = sum(dgi[:, d].abs() @ P["w_ih"][d].abs() for d in range(ndir))
    w_ih = torch.stack([dgi[:, d].t() @ x2 for d in range(ndir)])
    w_ih_mag = torch.stack([dgi[:, d].abs().t() @ x2.abs() for d in range(ndir)])
    w_hh, w_hh_mag = [], []
    for d in range(ndir):       # h_{t-1} (direction 1: h_{t+1}), in its bf16 operand copy, pairs with step t
        a, hb = (dgh[1:, :, d], hs[:-1, :, d]) if d == 0 else (dgh[:-1, :, d], hs[1:, :, d])
        a, hb = a.reshape(-1, 3 * H), S.bf16r(hb.reshape(-1, H))
        w_hh.append(a.t() @ hb)
        w_hh_mag.append(a.abs().t() @ hb.abs())
    mags = dict(y=res["hseq"].reshape(T, B, ndir, H).abs().sum(dim=2), b_ih=res["dgi"].abs().sum(dim=0).reshape(ndir, -1),
                b_hh=res["dgh"].abs().sum(dim=0).reshape(ndir, -1), dx=dx_mag, w_ih=w_ih_mag, w_hh=torch.stack(w_hh_mag))
    for name, a, b in (("y", res["y"].reshape(T, B, H), ym.detach()), ("b_ih", res["db_ih"].reshape(ndir, -1), p32["b_ih"].grad),
                       ("b_hh", res["db_hh"].reshape(ndir, -1), p32["b_hh"].grad), ("dx", dx, xr.grad.reshape(T * B, I)),
                       ("w_ih", w_ih, p32["w_ih"].grad), ("w_hh", torch.stack(w_hh), p32["w_hh"].grad)):
        d = (a - b.double()).abs()
        unit = 2.0 * S.half_spacing(mags[name], "bf16")         # (of the magnitudes that were summed: y = hf + hb may cancel)
        assert bool((d <= unit).all()), (name, float((d / unit).max()))
        close = d <= 2.0 ** -16 * torch.maximum(mags[name], torch.full_like(a, 1e-3))
        assert float(close.double().mean()) >= 0.99, (name, float(close.double().mean()))


# --------------------------------------------------------------------------------------- the caps on the GPU file's own inputs
def _forms(c):
    """(gi in bf16, gates in half, producer units of the partial-sum backward): which forms serve a case depends on the device
    (CU count), so the conditions are checked under the tightest and the loosest caps a case can meet"""
    forms = [(False, False, 0), (True, True, 32 if c.H % 128 == 0 else 0)]
    if c.H % 128 == 0:
        forms.append((False, False, 32))
    return forms


_SETS = {}
for _c in E.CASES:
    _SETS.setdefault(E.input_key(_c), _c)


def _stand_in(c, form):
    gi16, g16, ps = form
    inp = E.make_inputs(c)
    T, B, H, ndir = c.T, c.B, c.H, c.ndir
    gi = inp["gi"].to(torch.bfloat16).float() if gi16 else inp["gi"]
    dev = S.free_run(gi, inp["whh"], inp["bhh"], inp["dy"], T, B, H, ndir, x_len=inp["x_len"], rounding=True, gates_fmt="f16" if g16 else "f32",
                     ps_units=ps, gi_bf16=gi16)
    gi_read = S.pin_gi(gi, inp["x_len"], T, B, H, ndir, gi16)
    return inp, gi_read, dev["hseq"].float(), dev["gates"].float(), dev["dgh"].float(), dev


@pytest.mark.parametrize("key", list(_SETS), ids=[E.case_id(c) for c in _SETS.values()])
def test_caps_hold_the_float32_step_and_catch_a_dropped_k_slice(key):
    c = _SETS[key]
    T, B, H, ndir = c.T, c.B, c.H, c.ndir
    for form in _forms(c):
        gi16, g16, ps = form
        fmt = "f16" if g16 else "f32"
        inp, gi, hseq, gates, dgh, dev = _stand_in(c, form)
        ref, cap = S.teacher_forward(gi, hseq, inp["whh"], inp["bhh"], T, B, H, ndir, fmt)
        r32, _ = S.teacher_forward(gi, hseq, inp["whh"], inp["bhh"], T, B, H, ndir, fmt, dtype=torch.float32)
        gates_t = gates.reshape(T, B, ndir, 4, H)
        for i, k in enumerate(("r", "z", "n", "q")):
            # the stand-in is the same function of the same inputs, stored in the gate format: inside by construction -- a self-check
            # (the caps only: the stand-in is float64 arithmetic, which does not saturate where float32 does, so the exact demands are not its)
            assert float(S.outside(k, gates_t[:, :, :, i], ref, cap)[1].max()) <= 1.0, (form, k)
        # (the state: against the cap only -- the stand-in forms z in float64, where a saturated z is not 1 and h not bit for bit h')
        assert bool(((hseq.reshape(T, B, ndir, H).double() - ref["h"]).abs() <= cap["h"]).all()), (form, "h")
        for k in ("r", "z", "n", "q", "h"):
            # a quarter of the cap -- for r, z, n, h beside two float32 units of the value (h: and of its gates) and, for the gates, the
            # float32 rounding of their own argument (2^-24 |x| through the gate's slope: at |x| ~ 70 that alone is a third of a cap made of
            # the same term and the exp's argument scaling): where the arithmetic part of a cap is the
            # gate function's own few units (saturated gates, the first step of a narrow layer), the CPU's float32 exp, sum, quotient
            # and final rounding are no better than the device's exp and reciprocal, and a quarter of that cap cannot hold them
            # (DESIGN.md 25.3 says so; measured without the allowance: <= 0.5 of the cap).  q and the backward quantities: plain.
            own = 0.0 if k == "q" else 4.0 * S.half_spacing(ref[k], "f32")
            if k in "rz":
                own = own + ref[k] * (1.0 - ref[k]) * S.U * ref["x" + k].abs()
            if k == "n":
                own = own + (1.0 - ref[k] ** 2) * S.U * ref["xn"].abs()
            if k == "h":        # (... and of the gates it is formed from: z within half a spacing of 1 IS 1 in float32, whatever evaluates it)
                hp = torch.stack([S.prev_state(hseq, T, B, H, ndir, d) for d in range(ndir)], dim=2).double()
                own = own + (ref["n"] - hp).abs() * 4.0 * S.half_spacing(ref["z"], "f32") + (1.0 - ref["z"]) * 4.0 * S.half_spacing(ref["n"], "f32")
            excess = (r32[k].double() - ref[k]).abs() - own
            ratio = float((excess / cap[k]).max())
            assert ratio <= 0.25, (form, "float32 forward", k, ratio)
        if not c.fwd_only:
            bref, bcap = S.teacher_backward(inp["dy"], gates, hseq, dgh, inp["whh"], T, B, H, ndir, inp["x_len"], ps)
            b32, _ = S.teacher_backward(inp["dy"], gates, hseq, dgh, inp["whh"], T, B, H, ndir, inp["x_len"], ps, dtype=torch.float32)
            for k in bref:
                ratio = float(((b32[k].double() - bref[k]).abs() / bcap[k]).max())
                assert ratio <= 0.25, (form, "float32 backward", k, ratio)
                assert bool(((dev[k].reshape(T, B, ndir, 3 * H) - bref[k]).abs() <= bcap[k]).all()), (form, k)
        if c.group not in "abcd" or T < 2:
            continue        # (T = 1: the first step of a direction multiplies nothing -- there is no K slice to drop)
        drops = S.teacher_forward(gi, hseq, inp["whh"], inp["bhh"], T, B, H, ndir, fmt, drop=True)
        for d in range(ndir):
            moved = torch.zeros(H // 32, H, dtype=torch.bool)
            for k in ("r", "z", "n", "q", "h"):
                moved |= ((drops[d][k] - ref[k][:, :, d]).abs() > cap[k][:, :, d]).reshape(H // 32, T * B, H).any(dim=1)
            seen = moved.reshape(H // 32, H // 16, 16).any(dim=2)
            assert bool(seen.all()), (form, "forward: dropped K slice unseen (ks, unit slice)", d, (~seen).nonzero().tolist()[:8])
        if c.fwd_only:
            continue
        bdrop, _ = S.teacher_backward(inp["dy"], gates, hseq, dgh, inp["whh"], T, B, H, ndir, inp["x_len"], ps, rec_drop=True)
        nk = 3 * H // 32
        for d in range(ndir):
            moved = torch.zeros(nk, H, dtype=torch.bool)
            for k in ("dgi", "dgh"):
                m = ((bdrop[k][..., d, :] - bref[k][:, :, d]).abs() > bcap[k][:, :, d]).reshape(nk, T * B, 3, H).any(dim=1).any(dim=1)
                moved |= m
            seen = moved.reshape(nk, H // 16, 16).any(dim=2)
            assert bool(seen.all()), (form, "backward: dropped K slice unseen (ks, unit slice)", d, (~seen).nonzero().tolist()[:8])


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_saturated_limits_are_demanded_exactly(fmt):
    """a gate whose arithmetic can only give its limit must BE the limit in every storage format: one unit below 1 (and above -1), and
    the smallest non-zero value at the 0 end, are outside -- by the exact demand and, at 1 once the bound is below a quarter unit
    (|x| >= 20), by the numeric cap as well (the store's half unit is that of the values below 1).  Where the quotient is a subnormal a device may flush: its correctly rounded value and exactly
    0 are inside, the smallest normal number is not."""
    H = 32
    unit1 = 2.0 ** -24 if fmt == "f32" else 2.0 ** -11
    tiny = 2.0 ** -149 if fmt == "f32" else 2.0 ** -24
    zeros = torch.zeros(3 * H, H)
    for x in (17.4, 18.0, 20.0, 40.0, 90.0, 200.0):
        for sign in (1.0, -1.0):
            gi = torch.full((4, 3 * H), sign * x, dtype=F64)
            ev = S.fwd_eval(gi, torch.full((4, H), 0.25, dtype=F64), zeros, torch.zeros(3 * H))
            cap = S.fwd_caps(ev, H, fmt)
            one = torch.ones(4, H, dtype=F64)
            if sign > 0:
                for k in ("r", "z"):
                    assert bool((cap[k + "_exact"] == 1.0).all()), (x, k)
                    assert not bool(S.outside(k, one, ev, cap)[0].any())
                    bad, ratio = S.outside(k, one - unit1, ev, cap)
                    assert bool(bad.all()) and (x < 20.0 or float(ratio.min()) > 1.0), (x, k, float(ratio.min()))
                # with z == 1.0f the state is handed on bit for bit
                assert bool((cap["h_exact"] == 0.25).all()) and bool(S.outside("h", one * 0.25 * (1 + 2.0 ** -23), ev, cap)[0].all())
            elif x >= 90.0:
                for k in ("r", "z"):
                    assert bool((cap[k + "_exact"] == 0.0).all()), (x, k)
                    assert not bool(S.outside(k, one * 0.0, ev, cap)[0].any())
                    assert bool(S.outside(k, one * tiny, ev, cap)[0].all()), (x, k)
            assert bool((cap["n_exact"] == sign).all()), (x, "n")
            assert not bool(S.outside("n", one * sign, ev, cap)[0].any())
            bad, ratio = S.outside("n", one * sign * (1.0 - unit1), ev, cap)
            assert bool(bad.all()) and (x < 20.0 or float(ratio.min()) > 1.0), (x, "n", float(ratio.min()))
    # a subnormal quotient (x = -88: e^88 does not overflow, 1 / e^88 = 6e-39): the value itself and a flushed 0 pass, 2^-126 does not
    gi = torch.full((1, 3 * H), -88.0, dtype=F64)
    ev = S.fwd_eval(gi, torch.zeros(1, H, dtype=F64), zeros, torch.zeros(3 * H))
    cap = S.fwd_caps(ev, H, "f32")
    assert bool(torch.isnan(cap["r_exact"]).all()) and bool(cap["r_zero_ok"].all())
    for v, want in ((ev["r"].float().double(), False), (torch.zeros(1, H, dtype=F64), False), (torch.full((1, H), 2.0 ** -126, dtype=F64), True)):
        assert bool(S.outside("r", v, ev, cap)[0].all()) == want and bool(S.outside("r", v, ev, cap)[0].any()) == want
