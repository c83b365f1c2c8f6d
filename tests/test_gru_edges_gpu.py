"""The GRU recurrences step by step at their dispatch edges (csrc/gru.hip), element by element against the teacher-forced float64
step reference (oracle/gru_step.py) with DERIVED caps, plus the bit-exact identities between the outputs.

Every case runs _ops.gru_fwd / _ops.gru_bwd on the inputs of tests/gru_edge_cases.py; every step of every direction is then recomputed
in float64 from the device's own saved inputs (the gi it read, its float32 states, its gates as stored, its bf16 dgh), so nothing
accumulates and no bf16 rounding flip propagates: one wrong 16-unit slice at one time step is outside the cap.  Nothing is skipped.
tests/test_oracle_gru.py shows on the CPU, for these very inputs, that a float32 evaluation sits inside the caps and a kernel that
dropped one 32-wide K slice does not.

Kernel instances reached on a 256-CU device (from asr_gru_fwd / asr_gru_bwd; fewer CUs turn the persistent forms of the widest
shapes into per-step launches -- the forms are asked of asr_gru_fwd_accepts_bf16_gi / asr_gru_gates_f16_ok, never assumed):

  group (a), T=7, B=5        forward                                            backward
  H     nks  3H/32   mode 0            1      2                    4 / 7         mode 0 / 4 / 7 / 9 / 10     1         2
  32    1    3       io<1> flags       step<1> io<1> placement-free io<1> flags   step<2> (modes >= 2: UNSUPPORTED)  step<2>   UNSUPPORTED
  96    3    9       io<1> flags       step<1> io<1> placement-free io<1>         wide<2>                     step<6>   wide<2> p.-free
  160   5    15      io<2> ring        step<2> wide_fwd<1>          io<2>         wide<2>                     step<6>   wide<2>
  224   7    21      io<2> ring        step<2> wide_fwd<1>          io<2>         wide<3>                     step<6>   wide<3>
  320   10   30      io<4> ring        step<4> wide_fwd<2>          io<4>         wide<4>                     step<12>  wide<4>
  352   11   33      io<4> ring        step<4> wide_fwd<2>          io<4>         wide<5>                     step<12>  wide<5>
  448   14   42      io<4> ring        step<4> wide_fwd<2>          io<4>         wide<6>                     step<12>  wide<6>
  (io = fwd_persistent_io_kernel<KSW>, step = fwd_step_kernel<KSW> / bwd_step_kernel<KSW>, wide = bwd_wide_kernel<KS8>,
   wide_fwd = fwd_wide_kernel<KS8>.  H = 96: 3 K slices over 4 waves x 1; 160: 5 over 4 x 2 -- wave 2 holds one live and one dead
   slice; 224: 7 over 4 x 2; 320: 10 over 4 x 4; backward 9 / 15 / 21 / 30 / 33 / 42 slices over 5 waves' 8-slice groups.
   Modes 9 and 10 in group (a), H = 160 and 320: H % 128 != 0, so they do NOT select bwd_ps_kernel there -- the forward pass is mode 0's
   (io ring) and the backward falls through to bwd_wide_kernel<.., LOCAL = false>, mode 2's; what these rows pin is that fall-through.
   The partial-sum kernel under 9 / 10 runs in groups (c) and (d).)
  group (b)  H = 544, 1024: fwd_step_kernel<8> (no persistent grid of these widths fits 256 CUs); backward UNSUPPORTED above H = 512.
  group (c)  H=64 B=5 mode 0: io<1> with flags + bwd_wide<2>;  H=256 B=20: io<2> ring, bf16 gi, half gates + bwd_ps<2, G16>, and with both
             switches off io<2> ring float32 + bwd_ps<2>;  H=128: io<1> + bwd_ps<1>;  H=192: io<2> ring + bwd_wide<3>;  mode 1: step<1> /
             step<2>;  mode 2, H=128: fwd_wide<1> + bwd_wide<2>, both placement-free;  mode 9, H=128: io<1> + bwd_ps<1> asked for;
             mode 10, H=256 B=20: io<2> ring, half gates + bwd_ps<2, G16> with a forged split placement (its placement-free stores).
  group (d)  H=128: io<1> + bwd_ps<1> (B = 1 .. 32: 1 .. 4 eight-row, 1 .. 8 four-row recurrences);  H=160: io<2> ring + bwd_wide<2>;
             B = 33, 65 at H=256: slabs of 32 + a one-row remainder through io<2> ring + bwd_ps<2, G16>;  B = 33 at H=160: per-step
             (no slabs without the partial-sum backward), the loop over 32-row passes with one row in the second;  mode 10 at H=128,
             B = 1, 5, 17, 32: bwd_ps<1> with the forged placement.
"""
import numpy as np
import pytest
import torch

import gru_edge_cases as E
from oracle import gru_step as S

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32

_WORST = {}          # (group, quantity) -> (device error / cap, case id): printed when the module is done (DESIGN.md 25.4 quotes a run)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nGRU edges: worst device error / cap per group and quantity")
        for k in sorted(_WORST):
            print("  (%s) %-16s %.3f  %s" % (k[0], k[1], _WORST[k][0], _WORST[k][1]))


def _note(c, name, dev, ref, cap, q=None):
    """q: the quantity's name in the step reference's dicts -- then ref and cap are those dicts, and the exact demands at saturated limits
    and the accepted flush of a subnormal quotient apply (oracle.gru_step.outside)"""
    if q is None:
        ratio = (dev.double() - ref).abs() / cap
        bad = ~(ratio <= 1.0)
    else:
        bad, ratio = S.outside(q, dev, ref, cap)
        ref, cap = ref[q], cap[q]
    worst = float(ratio.max())
    key = (c.group, name)
    if worst > _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (worst, E.case_id(c))
    if bool(bad.any()):
        i = int(torch.where(bad, torch.nan_to_num(ratio, nan=float("inf")) + 1.0, torch.zeros_like(ratio)).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
        raise AssertionError("%s %s: device %r reference %r cap %.3e (error / cap %.3f) at (t, b, dir, unit) %r; %d of %d elements outside"
                             % (E.case_id(c), name, float(dev[idx]), float(ref[idx]), float(cap[idx]), worst, idx,
                                int(bad.sum()), ratio.numel()))


def _persist_ok(c):
    """whether a persistent grid of this shape fits the device (can_persist): the flag-signalled form of the 16-unit x 8-row kernel
    (mode 4) takes bf16 input projections exactly then"""
    from asr import _lib
    return c.B <= 32 and _lib.lib().asr_gru_fwd_accepts_bf16_gi(c.T, c.B, c.H, c.ndir, 4) == 1


def _predict(c):
    """-> (forward refuses, backward refuses, producer units of the partial-sum backward) from the dispatch rules and the device's answers.
    A HAND COPY of csrc/gru.hip's host dispatch -- can_persist (asked of the device through _persist_ok), slab_rows, bwd_ps_form and the
    order of the branches of asr_gru_bwd (slab / partial-sum, then wide: H >= 64, ks8 <= 6, then per-step: ksw <= 12): change it with
    them.  What a stale copy costs: ps = 32 for a shape the wide kernel serves WIDENS the backward caps by one bf16 unit per producer
    (tests/test_oracle_gru.py shows a dropped K slice is still outside under those caps); ps = 0 where the partial-sum kernel serves
    narrows them and fails loudly.  The library does not say which backward form it took."""
    from asr import _lib
    T, B, H, ndir, mode = c.T, c.B, c.H, c.ndir, c.mode
    persist = _persist_ok(c)
    slab = B > 32 and mode == 0 and _lib.lib().asr_gru_fwd_accepts_bf16_gi(T, B, H, ndir, 0) == 1
    ksw = (3 * H // 32 + 3) // 4
    ps = (slab or (persist and ksw <= 12 and mode in (0, 9, 10) and ndir * ((B + 3) // 4) <= 16)) and H % 128 == 0 and H // 128 in (1, 2, 3, 4, 8)
    wide = persist and ksw <= 12 and H >= 64 and ndir * ((B + 3) // 4) <= 16 and (3 * H // 32 + 7) // 8 <= 6
    fwd_no = H > 1024 or (mode >= 2 and not persist)
    bwd_no = ksw > 12 or (mode >= 2 and not (ps or wide))
    return fwd_no, bwd_no, 32 if ps else 0


class _Forms:
    def __init__(self, c, mode=None):
        self.vals = (c.mode if mode is None else mode, c.gi16, c.g16)

    def __enter__(self):
        from asr import _ops
        self.old = (_ops.GRU_MODE[0], _ops.GRU_GI_BF16[0], _ops.GRU_GATES_F16[0])
        _ops.GRU_MODE[0], _ops.GRU_GI_BF16[0], _ops.GRU_GATES_F16[0] = self.vals

    def __exit__(self, *a):
        from asr import _ops
        _ops.GRU_MODE[0], _ops.GRU_GI_BF16[0], _ops.GRU_GATES_F16[0] = self.old


def _abort_word(device, c):
    from asr import _ops, _lib
    return int(_ops._sync_buffer(device, _lib.lib().asr_gru_sync_bytes(c.B, c.H, c.ndir))[1023:1024].cpu()[0])


def _device_inputs(device, c, inp, rows=None, T=None):
    T0, B, H, ndir = c.T, c.B, c.H, c.ndir
    T = T0 if T is None else T
    gi = inp["gi"].reshape(T0, B, -1)[:T]
    dy = inp["dy"].reshape(T0, B, -1)[:T]
    if rows is not None:
        gi, dy = gi[:, rows], dy[:, rows]
    n = gi.shape[1]
    return gi.reshape(T * n, -1).contiguous(), dy.reshape(T * n, H).contiguous(), n


def _run(device, c, inp, x_len="case", rows=None, T=None, mode=None, check=True):
    """forward + backward of case c (optionally a slice of its batch / its first T steps / another mode) -> dict of CPU tensors.
    check: every element against the step reference, and the identities."""
    from asr import _ops, _lib
    H, ndir = c.H, c.ndir
    gi_f, dy_f, B = _device_inputs(device, c, inp, rows, T)
    T = c.T if T is None else T
    cc = c._replace(T=T, B=B, mode=c.mode if mode is None else mode)
    xl = inp["x_len"] if isinstance(x_len, str) else x_len
    if xl is not None and rows is not None:
        xl = xl[rows]
    whh16 = inp["whh"].to(device, BF16).contiguous()
    whhT16 = inp["whh"].transpose(1, 2).contiguous().to(device, BF16)
    bhh = inp["bhh"].to(device)
    out = dict(c=cc, x_len=xl)
    with _Forms(cc):
        fwd_no, bwd_no, ps = _predict(cc)
        gi = gi_f.to(device, _ops.gru_gi_dtype(T, B, H, ndir)).clone()          # (the call pins the update gate of dead rows in place)
        xld = None if xl is None else xl.to(device)
        if fwd_no:
            with pytest.raises(_lib.AsrHipError, match="unsupported shape"):
                _ops.gru_fwd(gi, whh16, bhh, T, B, H, ndir, xld)
            torch.cuda.synchronize()
            assert _abort_word(device, cc) == 0
            out["fwd_refused"] = True
            return out
        y, hseq, hseq16, gates = _ops.gru_fwd(gi, whh16, bhh, T, B, H, ndir, xld)
        _ops.gru_check_sync()
        out.update(gi=gi.float().cpu(), y=y.float().cpu(), hseq=hseq.cpu(), hseq16=hseq16.float().cpu(), fmt="f16" if gates.dtype == torch.float16 else "f32",
                   gates=_ops.gru_gates_standard(gates, H).cpu(), ps=ps)
        g = torch.Generator().manual_seed(B + H)
        init = torch.empty(2, ndir * 3 * H).uniform_(-1.0, 1.0, generator=g)      # (the caller's accumulate semantics: a non-zero buffer)
        dyd = dy_f.to(device, BF16)
        if bwd_no or c.fwd_only:
            dbi, dbh = init[0].to(device), init[1].to(device)
            with pytest.raises(_lib.AsrHipError, match="unsupported shape"):
                _ops.gru_bwd(dyd, gates, hseq, whhT16, T, B, H, ndir, dbi, dbh, xld)
            torch.cuda.synchronize()
            assert _abort_word(device, cc) == 0
            assert torch.equal(dbi.cpu(), init[0]) and torch.equal(dbh.cpu(), init[1])
            out["bwd_refused"] = True
    if out.get("bwd_refused") and not c.fwd_only:
        # the refusal left nothing behind: the next default-mode call on the same buffers is correct
        cc = cc._replace(mode=0)
        out["c"] = cc
        with _Forms(cc):
            _, bwd_no, ps = _predict(cc)
            assert not bwd_no
            out["ps"] = ps
    if not c.fwd_only:
        with _Forms(cc):
            dbi, dbh = init[0].to(device), init[1].to(device)
            dgi, dgh = _ops.gru_bwd(dyd, gates, hseq, whhT16, T, B, H, ndir, dbi, dbh, xld)
            _ops.gru_check_sync()
            out.update(dgi=dgi.float().cpu(), dgh=dgh.float().cpu(), dbi=dbi.cpu(), dbh=dbh.cpu(), init=init)
            if xl is not None:          # dx through the projection's backward-data GEMM: zero rows stay zero
                wih = torch.empty(ndir * 3 * H, 32).uniform_(-0.1, 0.1, generator=g).to(device, BF16)
                out["dx"] = _ops.gemm_nt(dgi, wih.t().contiguous(), None, F32).cpu()
    if check:
        _check(out, inp, dy_f)
    return out


def _check(o, inp, dy):
    c, xl = o["c"], o["x_len"]
    T, B, H, ndir = c.T, c.B, c.H, c.ndir
    hs = o["hseq"].reshape(T, B, ndir, H)
    gates = o["gates"].reshape(T, B, ndir, 4, H)
    for name, t in (("hseq", o["hseq"]), ("gates", o["gates"]), ("y", o["y"])):
        assert bool(torch.isfinite(t).all()), (E.case_id(c), name, "not finite")
    r, z, n = gates[:, :, :, 0], gates[:, :, :, 1], gates[:, :, :, 2]
    assert float(r.min()) >= 0.0 and float(r.max()) <= 1.0 and float(z.min()) >= 0.0 and float(z.max()) <= 1.0 and float(n.abs().max()) <= 1.0
    # ---- every step against the float64 step reference
    ref, cap = S.teacher_forward(o["gi"], o["hseq"], inp["whh"], inp["bhh"], T, B, H, ndir, o["fmt"])
    for i, k in enumerate(("r", "z", "n", "q")):
        _note(c, "%s %s" % (k, o["fmt"]), gates[:, :, :, i], ref, cap, q=k)
    _note(c, "h f32", hs, ref, cap, q="h")
    o["cap"] = cap
    # ---- identities, bit for bit
    h16 = o["hseq16"].reshape(T, B, ndir, H)
    want16 = o["hseq"].to(BF16).float().reshape(T, B, ndir, H)
    # (the operand copy of h: the LAST step of a direction is never read -- nor written by the ring form)
    assert torch.equal(h16[:-1, :, 0], want16[:-1, :, 0]), (E.case_id(c), "hseq16 != bf16(hseq), direction 0")
    if ndir == 2:
        assert torch.equal(h16[1:, :, 1], want16[1:, :, 1]), (E.case_id(c), "hseq16 != bf16(hseq), direction 1")
    ysum = hs[:, :, 0] if ndir == 1 else hs[:, :, 0] + hs[:, :, 1]
    live = torch.ones(T, B, 1, dtype=torch.bool)
    if xl is not None:
        live = (torch.arange(T).reshape(T, 1) < xl.reshape(1, B).long()).reshape(T, B, 1)
    want_y = torch.where(live, ysum.to(BF16).float(), torch.zeros(()))
    assert torch.equal(o["y"].reshape(T, B, H), want_y), (E.case_id(c), "y != bf16(hseq_fwd + hseq_bwd) / zero beyond the length")
    if xl is not None:
        for b in range(B):
            L = int(xl[b])
            if L < T:
                frozen = hs[L - 1, b, 0] if L > 0 else torch.zeros(H)
                assert torch.equal(hs[L:, b, 0], frozen.expand(T - L, H)), (E.case_id(c), "forward state not frozen beyond the length", b)
                if ndir == 2:
                    assert float(hs[L:, b, 1].abs().max()) == 0.0, (E.case_id(c), "reverse state not zero beyond the length", b)
    if "dgi" not in o:
        return
    dgi, dgh = o["dgi"].reshape(T, B, ndir, 3 * H), o["dgh"].reshape(T, B, ndir, 3 * H)
    assert bool(torch.isfinite(dgi).all()) and bool(torch.isfinite(dgh).all()), (E.case_id(c), "gradient not finite")
    bref, bcap = S.teacher_backward(dy, o["gates"], o["hseq"], o["dgh"], inp["whh"], T, B, H, ndir, xl, o["ps"])
    form = " partial-sum" if o["ps"] else ""
    _note(c, "dgi" + form, dgi, bref["dgi"], bcap["dgi"])
    _note(c, "dgh" + form, dgh, bref["dgh"], bcap["dgh"])
    if xl is not None:
        dead = ~live.reshape(T, B)
        if bool(dead.any()):
            assert float(dgi[dead].abs().max()) == 0.0 and float(dgh[dead].abs().max()) == 0.0, (E.case_id(c), "gate gradient on a dead row")
            assert float(o["dx"].reshape(T, B, -1)[dead].abs().max()) == 0.0, (E.case_id(c), "dx on a dead row")
    # bias gradients: every path sums the bf16 ROWS (the persistent kernels in registers, the per-step path with asr_colsum_acc), on
    # top of what the caller's buffer held
    for name, rows, got, init in (("db_ih", o["dgi"], o["dbi"], o["init"][0]), ("db_hh", o["dgh"], o["dbh"], o["init"][1])):
        want, bc = S.bias_grad_cap(rows.double().reshape(T * B, -1), init.double())
        _note(c, name, got, want, bc)


def _ids(group):
    cs = [c for c in E.CASES if c.group == group]
    return dict(argvalues=cs, ids=[E.case_id(c) for c in cs])


@pytest.mark.parametrize("c", **_ids("a"))
def test_ragged_k_splits_and_untested_instances(device, c):
    """(a): widths whose K split leaves one wave partly filled, H = 32 on the persistent forward and the per-step backward,
    bwd_wide_kernel<4>; a mode >= 2 that no kernel serves raises UNSUPPORTED, leaves the abort word zero and the caller's bias buffers
    untouched, and the default-mode call that follows on the same buffers is correct (the table in the module docstring)"""
    o = _run(device, c, E.make_inputs(c))
    assert not o.get("fwd_refused") or not _persist_ok(c)
    if o.get("fwd_refused"):
        _run(device, c._replace(mode=0), E.make_inputs(c))
    if c.H == 32 and c.mode >= 2:
        assert o.get("bwd_refused")


@pytest.mark.parametrize("c", **_ids("b"))
def test_forward_beyond_512_units_and_the_backward_refusal(device, c):
    """(b): the forward pass serves H <= 1024 (fwd_step_kernel<8> at 544 and 1024), the backward pass stops at 512 and says so"""
    o = _run(device, c, E.make_inputs(c))
    assert o.get("bwd_refused") and "dgi" not in o


@pytest.mark.parametrize("c", **_ids("c"))
def test_sequences_shorter_than_the_pipelines(device, c):
    """(c): T = 1 .. 5 -- no steady state of the four-step prefetch and the four-slot ring, only prologue and epilogue"""
    _run(device, c, E.make_inputs(c))


@pytest.mark.parametrize("c", **_ids("d"))
def test_batch_borders(device, c):
    """(d): one row, the 4- and 8-row recurrence borders, 16 | 17, 31 | 32, and beyond 32 rows a remainder of ONE row (slabs at H = 256,
    the per-step loop at H = 160): remainder rows equal the same utterances run alone -- bit for bit where the same kernels serve
    (> 16 rows), to rounding otherwise (test_gru_batches_beyond_the_resident_limit_run_as_slabs's rule)"""
    inp = E.make_inputs(c)
    whole = _run(device, c, inp)
    if c.B <= 32:
        return
    T, B, H, ndir = c.T, c.B, c.H, c.ndir
    for b0 in range(32, B, 32):
        rows = slice(b0, min(B, b0 + 32))
        n = rows.stop - rows.start
        part = _run(device, c, inp, rows=rows)
        same_kernels = n > 16 and c.H % 128 == 0
        for name in ("y", "hseq", "hseq16", "gates", "dgi", "dgh"):
            a = whole[name].reshape(T, B, -1)[:, rows]
            b = part[name].reshape(T, n, -1)
            if name == "hseq16":
                a = torch.cat([a[:-1, :, :H], a[1:, :, H:]], dim=2)
                b = torch.cat([b[:-1, :, :H], b[1:, :, H:]], dim=2)
            if same_kernels:
                assert torch.equal(a, b), (name, b0)
            else:
                rel = float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
                assert rel < 2e-2, (name, b0, rel)


@pytest.mark.parametrize("c", **_ids("e"))
def test_lengths_zero_one_and_full(device, c):
    """(e): x_len[b] = 0 (a dead utterance between live ones, and in front), x_len all 1, x_len all T; gi holds a non-zero bias and dy
    non-zero values on the dead rows.  Utterances are independent and a pinned update gate is exact, so a call with lengths equals
    the no-length call BIT FOR BIT wherever that one computes the same thing: every row of full length (all T; T next to a dead
    row), and the first frame of x_len all 1 against the no-length call with T = 1"""
    inp = E.make_inputs(c)
    T, B = c.T, c.B
    o = _run(device, c, inp)
    lens = list(c.lens)
    names = ("y", "hseq", "gates", "dgi", "dgh")
    if all(v in (0, T) for v in lens):
        plain = _run(device, c, inp, x_len=None)
        rows = [b for b in range(B) if lens[b] == T]
        for name in names:
            assert torch.equal(o[name].reshape(T, B, -1)[:, rows], plain[name].reshape(T, B, -1)[:, rows]), name
    elif all(v == 1 for v in lens):
        plain = _run(device, c, inp, x_len=None, T=1)
        for name in names:
            assert torch.equal(o[name].reshape(T, B, -1)[0], plain[name].reshape(1, B, -1)[0]), name


@pytest.mark.parametrize("c", **_ids("f"))
def test_saturated_gates(device, c):
    """(f): |gi + gh| up to ~14 (r, z below the half format's normal range), ~20, ~90 (__expf overflows to inf) and ~200, mixed signs,
    one row with r, z, n all at their limits: everything finite, r, z in [0, 1], |n| <= 1 (asserted for every case of this file), and
    the step reference's caps.  Where float32 arithmetic can only give the limit (e' <= 2^-25 in the sigmoid, 2^-26 in tanh; __expf
    overflowing at the other end) the reference DEMANDS the limit bit for bit -- r, z exactly 1 or 0, n exactly +-1, and under z == 1
    the state handed on unchanged -- in float32 and in half storage alike; one unit short of a limit fails (tests/test_oracle_gru.py
    shows that on the CPU for both formats)"""
    inp = E.make_inputs(c)
    o = _run(device, c, inp)
    gates = o["gates"].reshape(c.T, c.B, c.ndir, 4, c.H)
    if c.sat >= 20:         # the all-saturated row really is: r, z in {0, 1} and n = +-1 to within 2^-20
        r0 = gates[:, 0, :, :2]
        assert float(torch.minimum(r0, 1.0 - r0).max()) <= 2.0 ** -20 and float((1.0 - gates[:, 0, :, 2].abs()).max()) <= 2.0 ** -20
    if c.sat >= 200:        # ... and there the exact demands cover the whole row (at ~20 only the part with |x| > 17.4; at ~90 a negative
        for k in ("r_exact", "z_exact", "n_exact"):     # argument may sit in (-88.8, -87.3), where the quotient is a subnormal and nothing is demanded)
            assert not bool(torch.isnan(o["cap"][k][:, 0]).any()), k
    if c.sat >= 90:
        assert int((o["cap"]["r_exact"] == 0.0).sum()) > 100 and int((o["cap"]["r_exact"] == 1.0).sum()) > 100
    if c.sat == 14.0 and o["fmt"] == "f16":
        tiny = gates[:, 1, :, :2]
        assert int(((tiny > 0.0) & (tiny < 2.0 ** -14)).sum()) > 100             # half subnormals are there, and kept (the caps judge their values)
