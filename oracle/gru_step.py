"""Teacher-forced float64 statement of ONE step of the (Bi)GRU recurrence, with a derived error cap for every element.
TEST INFRASTRUCTURE -- see oracle/__init__.py.

The recurrence (csrc/gru.hip, cuDNN gate convention) is a pure function of the previous state:

    gh = bf16(h') W_hh^T + b_hh        r = s(gi_r + gh_r)   z = s(gi_z + gh_z)   n = tanh(gi_n + r gh_n)   q = gh_n
    h  = (1 - z) n + z h'

and the kernels save everything that function needs (the float32 state of every step, the gates).  So every step of a device run can
be judged on its own from the device's saved inputs: no accumulation over time, no bf16 rounding flip that propagates.  The backward
step is judged the same way from the saved gates, the states and the device's own bf16 dgh of the neighbouring step; only the carry
dh_t = dy_t + dh_{t+-1} z_{t+-1} + dgh_{t+-1} W_hh is chained here (in float64: the device keeps it in registers and saves nothing).

Everything is torch on the CPU.  `dtype` is float64 for the reference; the same functions run in float32 to show that a float32
evaluation of the step sits well inside the caps (tests/test_oracle_gru.py).  The caps are DERIVED, from
float32 accumulation, the documented accuracy of v_exp_f32 / v_rcp_f32 and the storage formats -- never from what a kernel returned.
"""
import torch

F64 = torch.float64
U = 2.0 ** -24                  # float32 unit roundoff (round to nearest)
ULP1 = 2.0 ** -23               # one float32 unit in the last place, relative: the documented accuracy of v_exp_f32 and v_rcp_f32
NOISE = 2.0 ** -50              # the float64 reference's own rounding, relative to the magnitudes involved
PIN = 1.0e4                     # pin_update_gate_kernel's update-gate input beyond an utterance's length


def bf16r(x):
    """round to nearest-even bfloat16, back in x's dtype (x holds float32 values: the first conversion is exact)"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def f16r(x):
    return x.to(torch.float32).to(torch.float16).to(x.dtype)


def _exponent(v):
    """floor(log2 |v|) as float64 (|v| = 0 -> a very small exponent)"""
    _, e = torch.frexp(v.abs().to(F64))
    return torch.where(v == 0, torch.full_like(e, -2000), e - 1).to(F64)


def half_spacing(v, fmt):
    """half a unit in the last place of `fmt` at |v| (the most a round-to-nearest store can move the value): 'f32' (flushing:
    nothing below the smallest normal number is trusted), 'f32g' (a float32 gate: the caps carry the flush of a subnormal quotient
    themselves, so the spacing goes all the way down), 'f16' (IEEE half with subnormals), 'bf16'"""
    e = _exponent(v)
    if fmt == "f32g":
        return torch.maximum(torch.pow(2.0, e - 24), torch.full_like(e, 2.0 ** -150))
    if fmt == "f32":
        return torch.maximum(torch.pow(2.0, e - 24), torch.full_like(e, 2.0 ** -126))
    if fmt == "f16":
        return torch.pow(2.0, torch.clamp(e, min=-14.0) - 11)
    if fmt == "bf16":
        return torch.maximum(torch.pow(2.0, e - 8), torch.full_like(e, 2.0 ** -133))
    raise ValueError(fmt)


# ------------------------------------------------------------------------------------------------------------------ gate functions
def sigmoid_cap(x, ex):
    """bound on |rcp(1 + __expf(-x')) - s(x)| for a float32 x' within ex of x (float64 tensors).
    __expf(-x) = v_exp_f32(-x log2e): the scaled argument is rounded (relative 2^-24 of |x| log2e, twice: the constant and the product),
    i.e. a RELATIVE error |x| 2^-23 of the result, plus one ulp of v_exp_f32: e' = e (1 + d), |d| <= 2^-23 (1 + |x|).  ds/de = -s^2, so
    that costs s (1 - s) d.  The sum 1 + e' rounds (2^-24) and v_rcp_f32 is good to one ulp: 1.5 2^-23 s.  The argument's own error
    goes through s' = s (1 - s) <= 1/4 (second-order term: |s''| <= s (1 - s)).
    Saturation.  e' <= 2^-25: 1 + e' IS 1.0f and rcp(1.0f) is exactly 1, the error is 1 - s = e / (1 + e) -- below half the spacing
    under 1 in every format, so the comparison there is exact equality with 1.  At the other end e' overflows (x < -88.7: 1 + inf,
    rcp -> +0: exactly 0 is demanded once the overflow is certain) or the quotient is subnormal and may be flushed: besides a value
    within the cap, exactly 0 is then accepted -- nothing else, so the smallest normal number is outside.
    -> cap, exact, zero_ok: exact holds 1.0 / 0.0 where the arithmetic leaves no other float32 result, NaN elsewhere; zero_ok marks
    the elements whose quotient may be flushed to 0."""
    s = torch.sigmoid(x)
    e = torch.exp(-x)
    d = ULP1 * (1.0 + x.abs())
    ds = s * (1.0 - s)
    general = ds * (1.001 * ex + d + ex * ex) + 1.5 * ULP1 * s
    sat1 = (torch.exp(-(x - ex)) * (1.0 + d)) <= 2.0 ** -25
    out = torch.where(sat1, torch.sigmoid(-x), general)
    sat0 = (torch.exp(-(x + ex)) * (1.0 - d)) >= 2.0 ** 128 * (1.0 + ULP1)          # v_exp_f32 returns +inf
    nan = torch.full_like(s, float("nan"))
    exact = torch.where(sat1, torch.ones_like(s), torch.where(sat0, torch.zeros_like(s), nan))
    return out, exact, s < 2.0 ** -125


def tanh_cap(x, ex):
    """bound on the kernel's tanh, t = 1 - 2 e rcp(1 + e) with e = __expf(-2 |x|) (sign copied), for x' within ex of x.
    e' = e (1 + d), |d| <= 2^-23 (1 + 2 |x|); dt/de = -2 / (1 + e)^2; the quotient 2 e / (1 + e) carries the rounding of the sum, one ulp
    of the reciprocal and one product rounding (2^-22 relative in all; 2 e is exact); the final subtraction rounds once.  For small
    |x| the subtraction cancels: the error stays ABSOLUTE, ~2^-22, which is what the cap says.  Saturation: e' <= 2^-26 gives
    1 - 2 e' = 1.0f exactly, the error is 1 - |tanh x| = 2 e / (1 + e).
    -> cap, exact: exact holds +-1.0 where nothing else can come out, NaN elsewhere."""
    a = x.abs()
    e = torch.exp(-2.0 * a)
    n = torch.tanh(x)
    d = ULP1 * (1.0 + 2.0 * a)
    general = (1.0 - n * n) * (1.001 * ex + ex * ex) + 2.0 * e / (1.0 + e) ** 2 * d + 2.0 * e / (1.0 + e) * (2.0 * ULP1) + U * n.abs()
    sat = (torch.exp(-2.0 * torch.clamp(a - ex, min=0.0)) * (1.0 + d)) <= 2.0 ** -26
    exact = torch.where(sat, torch.sign(x), torch.full_like(x, float("nan")))
    return torch.where(sat, 2.0 * e / (1.0 + e), general), exact


# ------------------------------------------------------------------------------------------------------------------ forward step
def fwd_eval(gi, hprev, whh, bhh, dtype=F64, round_h=True, gh_delta=None):
    """one step for rows (.., 3H) / (.., H): gi as the kernel read it, hprev the float32 state in front of the step (zeros at the
    first step of a direction), whh (3H, H) bf16-valued, bhh (3H).  gh_delta (broadcastable to (.., 3H)) is subtracted from gh: the
    share of one K slice, to model a kernel that dropped it.  -> dict of r, z, n, q, h and the magnitudes the caps need."""
    gi, hprev, whh, bhh = (a.to(dtype) for a in (gi, hprev, whh, bhh))
    H = hprev.shape[-1]
    hb = bf16r(hprev) if round_h else hprev
    gh = hb @ whh.t() + bhh
    if gh_delta is not None:
        gh = gh - gh_delta.to(dtype)
    S = hb.abs() @ whh.abs().t() + bhh.abs()
    xr, xz = gi[..., :H] + gh[..., :H], gi[..., H:2 * H] + gh[..., H:2 * H]
    r, z = torch.sigmoid(xr), torch.sigmoid(xz)
    q = gh[..., 2 * H:]
    xn = gi[..., 2 * H:] + r * q
    n = torch.tanh(xn)
    h = (1.0 - z) * n + z * hprev
    return dict(r=r, z=z, n=n, q=q, h=h, xr=xr, xz=xz, xn=xn, S=S, hprev=hprev)


def fwd_caps(ev, H, gate_fmt):
    """per-element caps for the outputs of fwd_eval(dtype=float64) against a kernel's float32 arithmetic.
    gate_fmt: 'f32' or 'f16', the format the gates were saved in; the state is float32."""
    S = ev["S"]
    # float32 accumulation of H exact bf16 x bf16 products (H / 32 MFMA steps), the four waves' partial sums and the bias: recursive
    # summation of H + 5 terms, |error| <= (H + 8) 2^-24 (sum |a| |w| + |b|) whatever the order
    egh = (H + 8) * U * S
    er_x = egh[..., :H] + U * ev["xr"].abs()
    ez_x = egh[..., H:2 * H] + U * ev["xz"].abs()
    (er, r_exact, r_zero), (ez, z_exact, z_zero) = sigmoid_cap(ev["xr"], er_x), sigmoid_cap(ev["xz"], ez_x)
    q, r, z, n, hp = ev["q"], ev["r"], ev["z"], ev["n"], ev["hprev"]
    eq = egh[..., 2 * H:]
    flush_r, flush_z = torch.where(r_zero, r, torch.zeros_like(r)), torch.where(z_zero, z, torch.zeros_like(z))     # (a flushed quotient, downstream)
    en_x = q.abs() * (er + flush_r) + r * eq + er * eq + U * ((r * q).abs() + ev["xn"].abs())
    en, n_exact = tanh_cap(ev["xn"], en_x)
    eh = (n - hp).abs() * (ez + flush_z) + (1.0 - z) * en + ez * en + U * (3.0 * ((1.0 - z) * n).abs() + 2.0 * (z * hp).abs() + ev["h"].abs())
    # the reference's own float64 rounding (2^-50 of the magnitudes involved: 1 - z cancels when z is within 2^-53 of 1)
    er, ez, en, eq = er + NOISE * r, ez + NOISE * z, en + NOISE * n.abs(), eq + NOISE * S[..., 2 * H:]
    eh = eh + NOISE * (n.abs() + hp.abs())
    # the store's half unit.  r, z and |n| cannot exceed 1, so the unit is that of the values BELOW 1 even where the reference (or
    # reference + bound) reaches 1: with the spacing of [1, 2) a result one unit short of a saturated limit would pass.
    gfmt = "f32g" if gate_fmt == "f32" else gate_fmt
    below1 = 1.0 - 2.0 ** -30
    # exact demands: a saturated gate IS its limit, and with z == 1.0f the state is handed on bit for bit (0 n + 1 h' = h')
    h_exact = torch.where(z_exact == 1.0, hp, torch.full_like(hp, float("nan")))
    return dict(r=er + half_spacing(torch.clamp(r + er, max=below1), gfmt), z=ez + half_spacing(torch.clamp(z + ez, max=below1), gfmt),
                n=en + half_spacing(torch.clamp(n.abs() + en, max=below1), gfmt),
                q=eq + half_spacing(q.abs() + eq, gate_fmt), h=eh + half_spacing(ev["h"].abs() + eh, "f32"),
                r_exact=r_exact, z_exact=z_exact, n_exact=n_exact, h_exact=h_exact, r_zero_ok=r_zero, z_zero_ok=z_zero)


def k_slice_shares(a, w):
    """(nks, .., N): the share of every 32-wide K slice in a @ w.t() (a (.., K), w (N, K)) -- what a kernel that masked that slice
    would lose"""
    K = a.shape[-1]
    nks = K // 32
    a4 = a.reshape(a.shape[:-1] + (nks, 32))
    w4 = w.reshape(w.shape[0], nks, 32)
    out = torch.einsum("...kc,nkc->k...n", a4, w4)
    return out


def prev_state(hseq, T, B, H, ndir, d):
    """(T, B, H): the state in front of every step of direction d, from the saved float32 sequence hseq (T*B, ndir*H)"""
    hs = hseq.reshape(T, B, ndir, H)[:, :, d]
    z = torch.zeros_like(hs[:1])
    return torch.cat([z, hs[:-1]]) if d == 0 else torch.cat([hs[1:], z])


def teacher_forward(gi, hseq, whh, bhh, T, B, H, ndir, gate_fmt="f32", dtype=F64, drop=False):
    """every step of every direction from the saved states.  gi (T*B, ndir*3H) as the kernel read it (after the length pinning),
    hseq (T*B, ndir*H) float32, whh (ndir, 3H, H), bhh (ndir*3H).  -> ref, cap: dicts of (T, B, ndir, H) tensors for r, z, n, q, h;
    cap also holds r_exact, z_exact, n_exact, h_exact: the value that MUST come out where the arithmetic leaves no other (saturated
    gates; the state under z == 1.0f), NaN elsewhere, and r_zero_ok, z_zero_ok: where a subnormal quotient may have been flushed, so that
    exactly 0 is accepted beside the cap.  outside() applies all three.
    drop=True: -> per direction a dict of (nks, T, B, H) outputs with K slice ks removed from gh instead."""
    gi = gi.to(torch.float32).reshape(T, B, ndir, 3 * H)
    whh = whh.to(torch.float32)
    bhh = bhh.reshape(ndir, 3 * H)
    refs, caps, drops = [], [], []
    for d in range(ndir):
        hp = prev_state(hseq.to(torch.float32), T, B, H, ndir, d)
        if drop:
            shares = k_slice_shares(bf16r(hp.to(dtype)), whh[d].to(dtype))
            drops.append(fwd_eval(gi[:, :, d].unsqueeze(0), hp.unsqueeze(0), whh[d], bhh[d], dtype, gh_delta=shares))
            continue
        ev = fwd_eval(gi[:, :, d], hp, whh[d], bhh[d], dtype)
        refs.append(ev)
        if dtype == F64:
            caps.append(fwd_caps(ev, H, gate_fmt))
    if drop:
        return drops
    names = ("r", "z", "n", "q", "h")
    ref = {k: torch.stack([e[k] for e in refs], dim=2) for k in names + ("xr", "xz", "xn")}      # (x*: the gates' arguments)
    extra = tuple(k + "_exact" for k in "rznh") + ("r_zero_ok", "z_zero_ok")
    cap = {k: torch.stack([c[k] for c in caps], dim=2) for k in names + extra} if caps else None
    return ref, cap


def outside(name, dev, ref, cap):
    """-> (bool tensor: elements of quantity `name` that fail, error / cap with the accepted flushes at 0): beyond the cap -- unless a
    flushed subnormal quotient is allowed there and the value is exactly 0 -- or different from the value demanded exactly"""
    dev = dev.to(F64)
    ratio = (dev - ref[name]).abs() / cap[name]
    zero_ok = cap.get(name + "_zero_ok")
    if zero_ok is not None:
        ratio = torch.where(zero_ok & (dev == 0), torch.zeros_like(ratio), ratio)
    bad = ~(ratio <= 1.0)
    exact = cap.get(name + "_exact")
    if exact is not None:
        bad = bad | (~torch.isnan(exact) & (dev != exact))
    return bad, ratio


# ------------------------------------------------------------------------------------------------------------------ backward step
def bwd_dir(dy, r, z, n, q, hp, dgh_nb, whh, order, ps_units=0, dtype=F64, rec_drop=False):
    """the backward sweep of one direction.  dy (T, B, H) masked as the kernel masks it; r, z, n, q the saved gates as stored and hp
    the state in front of each step, (T, B, H); dgh_nb (T, B, 3H) the DEVICE's bf16 dgh (step order[s] reads row order[s - 1]);
    whh (3H, H); order: time indices in sweep order.  ps_units: 32 when every 32-unit producer publishes its share of dgh . W_hh
    rounded to bf16 (bwd_ps_kernel), else 0.
    rec_drop: a leading axis of 3H / 32 variants, variant ks with that K slice removed from dgh . W_hh.
    -> ref dict (dar, daz, dan, dq: (T, B, H)) and cap dict (same keys; float64 only)."""
    dy, r, z, n, q, hp, dgh_nb, whh = (a.to(dtype) for a in (dy, r, z, n, q, hp, dgh_nb, whh))
    T, B, H = dy.shape
    K = 3 * H
    lead = (K // 32,) if rec_drop else ()
    out = {k: torch.zeros(lead + (T, B, H), dtype=dtype) for k in ("dar", "daz", "dan", "dq")}
    cap = {k: torch.zeros(lead + (T, B, H), dtype=dtype) for k in ("dar", "daz", "dan", "dq")}
    dh_prev = E_prev = None
    for s, t in enumerate(order):
        if s == 0:
            dh = dy[t].expand(lead + (B, H)).clone()
            E = torch.zeros_like(dh)
        else:
            tn = order[s - 1]
            g = dgh_nb[tn]
            rec = g @ whh
            Srec = g.abs() @ whh.abs()
            if ps_units:
                # producer p: units [p ps, (p + 1) ps) of all three gates; its share is published rounded to bf16 and the consumer adds the
                # shares in float32.  The reference keeps the exact sum and pays one bf16 unit per share (it cannot know which way the
                # device rounded a share whose float32 value sat near a tie), plus the float32 sum of a 3 ps-term share and of the shares
                P = H // ps_units
                gp = g.reshape(B, 3, P, ps_units)
                wp = whh.reshape(3, P, ps_units, H)
                part = torch.einsum("bgpu,gpuh->pbh", gp, wp)
                Sp = torch.einsum("bgpu,gpuh->pbh", gp.abs(), wp.abs())
                e_part = (3 * ps_units + 8) * U * Sp
                erec = (e_part + 2.0 * half_spacing(part.abs() + e_part, "bf16")).sum(dim=0) + (P + 4) * U * part.abs().sum(dim=0)
            else:
                erec = (K + 8) * U * Srec          # float32 accumulation of 3H exact products and the waves' partial sums, any order
            carry = dh_prev * z[tn]
            if rec_drop:
                rec = rec - k_slice_shares(g, whh.t())
            dh = dy[t] + carry + rec
            E = E_prev * z[tn] + U * carry.abs() + erec + 3.0 * U * (dy[t].abs() + carry.abs() + rec.abs())
        zt, nt, rt, qt, hpt = z[t], n[t], r[t], q[t], hp[t]
        A_an = (1.0 - zt) * (1.0 - nt * nt)
        eA_an = U * (1.0 - nt * nt).abs() + (1.0 - zt) * 2.0 * U + U * A_an.abs()
        dan = dh * A_an
        e_dan = E * A_an.abs() + dh.abs() * eA_an + E * eA_an + 3.0 * U * dan.abs()
        A_az = (hpt - nt) * zt * (1.0 - zt)
        eA_az = 2.0 * U * ((hpt - nt) * zt).abs() + 3.0 * U * A_az.abs()
        daz = dh * A_az
        e_daz = E * A_az.abs() + dh.abs() * eA_az + E * eA_az + 3.0 * U * daz.abs()
        dq = dan * rt
        e_dq = e_dan * rt + U * dq.abs()
        Bf = qt * rt * (1.0 - rt)
        eB = U * (qt * rt).abs() + 3.0 * U * Bf.abs()
        dar = dan * Bf
        e_dar = e_dan * Bf.abs() + dan.abs() * eB + 2.0 * U * dar.abs()
        for k, v, e in (("dar", dar, e_dar), ("daz", daz, e_daz), ("dan", dan, e_dan), ("dq", dq, e_dq)):
            out[k][..., t, :, :] = v
            if dtype == F64:
                cap[k][..., t, :, :] = e + half_spacing(v.abs() + e, "bf16")
        dh_prev, E_prev = dh, E
    return out, (cap if dtype == F64 else None)


def teacher_backward(dy, gates, hseq, dgh_dev, whh, T, B, H, ndir, x_len=None, ps_units=0, dtype=F64, rec_drop=False):
    """dy (T*B, H) bf16-valued as handed to the kernel (masked here), gates (T*B, ndir, 4, H) decoded to float32 exactly as stored,
    hseq (T*B, ndir*H), dgh_dev (T*B, ndir*3H) the device's own dgh.  -> ref, cap: dicts dgi, dgh of (T, B, ndir, 3H)
    (with rec_drop a leading variant axis)."""
    dy = dy.to(torch.float32).reshape(T, B, H)
    if x_len is not None:
        live = (torch.arange(T).reshape(T, 1) < x_len.reshape(1, B).long()).reshape(T, B, 1)
        dy = dy * live
    g = gates.to(torch.float32).reshape(T, B, ndir, 4, H)
    dg = dgh_dev.to(torch.float32).reshape(T, B, ndir, 3 * H)
    refs, caps = {"dgi": [], "dgh": []}, {"dgi": [], "dgh": []}
    for d in range(ndir):
        hp = prev_state(hseq.to(torch.float32), T, B, H, ndir, d)
        order = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        o, c = bwd_dir(dy, g[:, :, d, 0], g[:, :, d, 1], g[:, :, d, 2], g[:, :, d, 3], hp, dg[:, :, d], whh[d].to(torch.float32), order,
                       ps_units, dtype, rec_drop)
        refs["dgi"].append(torch.cat([o["dar"], o["daz"], o["dan"]], dim=-1))
        refs["dgh"].append(torch.cat([o["dar"], o["daz"], o["dq"]], dim=-1))
        if c is not None:
            caps["dgi"].append(torch.cat([c["dar"], c["daz"], c["dan"]], dim=-1))
            caps["dgh"].append(torch.cat([c["dar"], c["daz"], c["dq"]], dim=-1))
    ref = {k: torch.stack(v, dim=-2) for k, v in refs.items()}
    cap = {k: torch.stack(v, dim=-2) for k, v in caps.items()} if caps["dgi"] else None
    return ref, cap


def bias_grad_cap(rows, init):
    """the bias gradients are the column sums of the bf16 rows (every path sums the ROUNDED values: the persistent kernels in registers
    and with float atomics, the per-step path with asr_colsum_acc), added to the caller's buffer: float32 summation of n + 1 terms in
    any order.  rows (n, C) float64, init (C).  -> expected (C), cap (C)"""
    n = rows.shape[0]
    mag = rows.abs().sum(dim=0) + init.abs()
    return rows.sum(dim=0) + init, (n + 4) * U * mag + half_spacing(mag, "f32")


# ------------------------------------------------------------------------------------------------------------------ free-running chain
def pin_gi(gi, x_len, T, B, H, ndir, gi_bf16):
    """what asr_gru_fwd does to gi in place: the update-gate columns of rows beyond an utterance's length become +10^4 (bf16(10^4) in a
    bf16 gi)"""
    if x_len is None:
        return gi
    g = gi.clone().reshape(T, B, ndir, 3 * H)
    dead = (torch.arange(T).reshape(T, 1) >= x_len.reshape(1, B).long())
    pin = float(bf16r(torch.tensor(PIN, dtype=torch.float32))) if gi_bf16 else PIN
    g[..., H:2 * H] = torch.where(dead.reshape(T, B, 1, 1), torch.full_like(g[..., H:2 * H], pin), g[..., H:2 * H])
    return g.reshape(gi.shape)


def free_run(gi, whh, bhh, dy, T, B, H, ndir, x_len=None, rounding=False, gates_fmt="f32", ps_units=0, dtype=F64, gi_bf16=False):
    """the whole layer as a chain of the step functions above.  rounding=False: no rounding point at all (pure float64: equals
    torch's GRU); rounding=True: the device's rounding points -- bf16 operand copy of h, gates saved in `gates_fmt`, bf16 dgi / dgh
    and, with ps_units, bf16 producer shares -- i.e. oracle.bf16.GRUMatched.  gi (T*B, ndir*3H) BEFORE pinning, whh (ndir, 3H, H),
    bhh (ndir*3H), dy (T*B, H) or None.  -> dict y, hseq (T*B, ndir*H), gates (T*B, ndir, 4, H), dgi, dgh (T*B, ndir*3H), db_ih, db_hh"""
    gi = pin_gi(gi.to(dtype), x_len, T, B, H, ndir, gi_bf16).reshape(T, B, ndir, 3 * H)
    whh, bhh = whh.to(dtype), bhh.to(dtype).reshape(ndir, 3 * H)
    hseq = torch.zeros(T, B, ndir, H, dtype=dtype)
    gates = torch.zeros(T, B, ndir, 4, H, dtype=dtype)
    for d in range(ndir):
        h = torch.zeros(B, H, dtype=dtype)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            ev = fwd_eval(gi[t, :, d], h, whh[d], bhh[d], dtype, round_h=rounding)
            h = ev["h"].to(torch.float32).to(dtype) if rounding else ev["h"]          # (the device's state is float32)
            hseq[t, :, d] = h
            gates[t, :, d] = torch.stack([ev["r"], ev["z"], ev["n"], ev["q"]], dim=1)
    if rounding:
        gates = f16r(gates) if gates_fmt == "f16" else gates.to(torch.float32).to(dtype)
    live = None
    if x_len is not None:
        live = (torch.arange(T).reshape(T, 1) < x_len.reshape(1, B).long()).reshape(T, B, 1)
    y = hseq.sum(dim=2)
    if rounding:
        y = bf16r(y)
    if live is not None:
        y = y * live
    res = dict(y=y.reshape(T * B, H), hseq=hseq.reshape(T * B, ndir * H), gates=gates.reshape(T * B, ndir, 4, H))
    if dy is None:
        return res
    dyt = dy.to(dtype).reshape(T, B, H)
    if live is not None:
        dyt = dyt * live
    dgi = torch.zeros(T, B, ndir, 3 * H, dtype=dtype)
    dgh = torch.zeros(T, B, ndir, 3 * H, dtype=dtype)
    rnd = bf16r if rounding else (lambda v: v)
    for d in range(ndir):
        hs = hseq[:, :, d]
        zero = torch.zeros_like(hs[:1])
        hp = torch.cat([zero, hs[:-1]]) if d == 0 else torch.cat([hs[1:], zero])
        order = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        dh_prev = None
        for s, t in enumerate(order):
            r, z, n, q = (gates[t, :, d, k] for k in range(4))
            dh = dyt[t]
            if s > 0:
                tn = order[s - 1]
                g = dgh[tn, :, d]
                if rounding and ps_units:
                    P = H // ps_units
                    rec = rnd(torch.einsum("bgpu,gpuh->pbh", g.reshape(B, 3, P, ps_units), whh[d].reshape(3, P, ps_units, H))).sum(dim=0)
                else:
                    rec = g @ whh[d]
                dh = dyt[t] + dh_prev * gates[tn, :, d, 1] + rec
            dan = dh * ((1.0 - z) * (1.0 - n * n))
            daz = dh * ((hp[t] - n) * z * (1.0 - z))
            dq = dan * r
            dar = dan * (q * r * (1.0 - r))
            dgi[t, :, d] = rnd(torch.cat([dar, daz, dan], dim=1))
            dgh[t, :, d] = rnd(torch.cat([dar, daz, dq], dim=1))
            dh_prev = dh
    res.update(dgi=dgi.reshape(T * B, ndir * 3 * H), dgh=dgh.reshape(T * B, ndir * 3 * H),
               db_ih=dgi.reshape(T * B, -1).sum(dim=0), db_hh=dgh.reshape(T * B, -1).sum(dim=0))
    return res
