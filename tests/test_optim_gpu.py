"""csrc/optim.hip and asr/optimizers.py against the float64 references of oracle/nn.py: every update rule (Adam, SGD, MomentumSGD,
NesterovAG) through both families of entry points, the step control's ctl[0..6], the argument guards, and the Optimizer classes on a
four-parameter link.

Sizes: the update kernels launch at most 2048 x 256 = 524288 threads and stride over the rest, the squared norm is folded from one
partial sum per workgroup by 256 threads.  SIZES gives 1, 2, 256, 257 and 2048 partial sums and one, two and three trips of the
grid-stride loops, the last of them ragged.

Bounds: every buffer a kernel sees is the middle of a larger allocation with 64 sentinel floats on either side, once starting on a
256-byte boundary and once one float later (the ABI promises float alignment only); the sentinels are compared bit for bit after every
launch.  A sentinel that changed is an out-of-bounds write: read the index arithmetic of the kernel that ran last.

Hyperparameters are float32 values widened to float64 on the oracle's side, like the data: the ABI takes them as float.
"""
import numpy as np
import pytest
import torch

from oracle import nn as onn

pytestmark = pytest.mark.gpu

SIZES = (1, 257, 65536, 65537, 524288, 524289, 1048653)
PARTIALS = {1: 1, 257: 2, 65536: 256, 65537: 257, 524288: 2048, 524289: 2048, 1048653: 2048}
GUARD = 64
SENTINEL_BITS = 0x4B5EA71E          # a finite float32 (about 1.46e7) no test value comes near
BAD_ARG = -1


def f32(x):
    return float(np.float32(x))


ALPHA, BETA1, BETA2, EPS = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
LR, MU = f32(0.1), f32(0.9)         # a step large enough that one element left out of a loop's tail shows in p at TOL_P
DECAY, CLIP, GS = f32(1e-5), 1.0, 0.5
RULES = ("adam", 0, 1, 2)           # Adam, or the kind of asr_sgd_ctl / asr_clip_decay_sgd
TOL_P = dict(rtol=1e-5, atol=1e-6)          # the bars of test_clip_decay_adam (tests/test_kernels_gpu.py)
TOL_M = dict(rtol=1e-4, atol=1e-7)          # first moment / velocity
TOL_V = dict(rtol=1e-4, atol=1e-9)          # Adam's second moment

_BASE = {}


def _randn(seed, n):
    """the first n of one cached float32 normal sequence per seed (read-only: callers copy)"""
    if seed not in _BASE:
        _BASE[seed] = np.random.RandomState(seed).randn(max(SIZES)).astype(np.float32)
        _BASE[seed].setflags(write=False)
    return _BASE[seed][:n]


def _grad(seed, n, target, grad_scale=GS):
    """float32 gradient whose norm times |grad_scale| is `target` (up to its float32 rounding)"""
    g = _randn(seed, n).astype(np.float64)
    g *= target / (np.sqrt((g ** 2).sum()) * abs(grad_scale))
    return g.astype(np.float32)


def _assert_clip_is_decided(g, clip=CLIP, grad_scale=GS):
    """float32 and float64 must not disagree about whether this step is clipped"""
    norm = np.sqrt((g.astype(np.float64) ** 2).sum())
    assert abs(clip / (norm * abs(grad_scale)) - 1.0) > 1e-3


class Arena(object):
    """hands out guarded buffers and checks all their sentinels at once"""

    def __init__(self, device, misalign):
        self.device, self.misalign, self.bufs = device, misalign, []

    def new(self, n, init=None, dtype=torch.float32, name=""):
        lead = GUARD + self.misalign
        whole = torch.empty(lead + n + GUARD, dtype=dtype, device=self.device)
        whole.view(torch.int32).fill_(SENTINEL_BITS)
        t = whole[lead:lead + n]
        assert whole.data_ptr() % 256 == 0 and (t.data_ptr() % 256 == 0) == (self.misalign == 0) and t.is_contiguous()
        if isinstance(init, np.ndarray):
            t.copy_(torch.from_numpy(np.array(init)))
        elif init is not None:
            t.fill_(init)
        self.bufs.append((name or "buffer %d" % len(self.bufs), whole, lead, n))
        return t

    def check(self, after):
        torch.cuda.synchronize()
        for name, whole, lead, n in self.bufs:
            w = whole.view(torch.int32)
            ok = bool((w[:lead] == SENTINEL_BITS).all()) and bool((w[lead + n:] == SENTINEL_BITS).all())
            assert ok, "out-of-bounds write next to %s (%d elements) after %s" % (name, n, after)

    def snapshot(self):
        return [whole.clone() for _, whole, _, _ in self.bufs]

    def assert_unchanged(self, snap, after):
        torch.cuda.synchronize()
        for (name, whole, _, _), s in zip(self.bufs, snap):
            assert torch.equal(whole.view(torch.int32), s.view(torch.int32)), "%s changed after %s" % (name, after)


def _host(t):
    return t.cpu().numpy().astype(np.float64)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _oracle_step(rule, p, g, state, step, lr, mu, decay, clip, grad_scale, alpha=ALPHA, beta1=BETA1):
    """one float64 step from float32 state; state = (m, v) for Adam, (vel,) for the SGD kinds.  Returns (p, state)"""
    g = g.astype(np.float64)
    if rule == "adam":
        p, m, v = onn.clip_decay_adam(p, g, state[0], state[1], step, alpha=alpha, beta1=beta1, beta2=BETA2, eps=EPS, decay=decay,
                                      clip=clip, grad_scale=grad_scale)
        return p, (m, v)
    p, vel = onn.clip_decay_sgd(p, g, state[0], rule, lr, mu, decay, clip, grad_scale)
    return p, (vel,)


def _compare(rule, p_dev, state_dev, p_want, state_want, what):
    np.testing.assert_allclose(p_dev.cpu().numpy(), p_want, err_msg="p, " + what, **TOL_P)
    np.testing.assert_allclose(state_dev[0].cpu().numpy(), state_want[0], err_msg="m / velocity, " + what, **TOL_M)
    if rule == "adam":
        np.testing.assert_allclose(state_dev[1].cpu().numpy(), state_want[1], err_msg="v, " + what, **TOL_V)


def _run_rule(device, n, misalign, rule, entry, targets=(0.3, 30.0, 0.3), decay=DECAY, clip=CLIP):
    """three consecutive steps of one rule; entry "ctl": asr_step_control + asr_adam_ctl / asr_sgd_ctl sharing one ctl / applied
    pair, "old": asr_sqnorm_acc + asr_clip_decay_adam / asr_clip_decay_sgd.  targets: ||g|| |grad_scale| per step (None: g = 0);
    with clip = 1 the default is not clipped, clipped hard, not clipped.  Every step is compared with the float64 reference of
    ONE step started from the device's float32 state before it."""
    from asr import _ops
    A = Arena(device, misalign)
    p = A.new(n, _randn(0, n), name="p")
    g = A.new(n, 0.0, name="g")
    if rule == "adam":
        state = (A.new(n, 0.0, name="m"), A.new(n, 0.0, name="v"))
    else:
        state = (A.new(n, 0.0 if rule else 0.25, name="velocity"),)
    ctl = A.new(8, 0.0, name="ctl")
    applied = A.new(1, 0, dtype=torch.int32, name="applied")
    no_abort = A.new(1, 0, dtype=torch.int32, name="abort word")
    partials = A.new(_ops.sqnorm_partials_count(n), 0.0, name="partials")
    sq = A.new(1, 0.0, name="sqnorm")
    p_host, state_host = _host(p), tuple(_host(s) for s in state)
    for step, target in enumerate(targets, 1):
        what = "%s, n = %d, step %d" % (rule, n, step)
        g_np = np.zeros(n, np.float32) if target is None else _grad(step, n, target)
        if clip > 0 and target is not None:
            _assert_clip_is_decided(g_np, clip)
        g.copy_(torch.from_numpy(g_np))
        if entry == "ctl":
            _ops.step_control(g, partials, clip, GS, ALPHA, BETA1, BETA2, applied, ctl, no_abort)
            A.check("asr_step_control, " + what)
            if rule == "adam":
                _ops.adam_ctl(p, g, state[0], state[1], BETA1, BETA2, EPS, decay, ctl)
            else:       # kind 0 takes v = NULL, and leaves a velocity buffer alone that is passed all the same (step 2)
                vel = state[0] if rule or step == 2 else None
                _ops.sgd_ctl(p, g, vel, rule, LR, MU, decay, ctl)
        else:
            sq.zero_()
            _ops.sqnorm_acc(g, sq)
            if rule == "adam":
                _ops.clip_decay_adam(p, g, state[0], state[1], ALPHA, BETA1, BETA2, EPS, decay, clip, GS, sq, step)
            else:
                _ops.clip_decay_sgd(p, g, state[0] if rule or step == 2 else None, rule, LR, MU, decay, clip, GS, sq)
        A.check("the update kernel, " + what)
        p_want, state_want = _oracle_step(rule, p_host, g_np, state_host, step, LR, MU, decay, clip, GS)
        assert np.isfinite(p_want).all()
        if rule == 0:
            assert bool((state[0] == 0.25).all()), "kind 0 wrote to the velocity buffer, " + what
            np.testing.assert_allclose(p.cpu().numpy(), p_want, err_msg="p, " + what, **TOL_P)
        else:
            _compare(rule, p, state, p_want, state_want, what)
        assert torch.equal(g.cpu(), torch.from_numpy(g_np)), "the gradient changed, " + what
        p_host, state_host = _host(p), tuple(_host(s) for s in state)       # re-seeded: errors do not compound
    if entry == "ctl":
        assert int(applied.cpu()[0]) == len(targets) and float(ctl.cpu()[3]) == float(len(targets))
    return p_host, state_host, ctl.cpu().tolist()


# ------------------------------------------------------------------------------------------------ update rules
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_update_rules_follow_float64(device, n, misalign, rule):
    """asr_adam_ctl and asr_sgd_ctl kinds 0, 1, 2 driven by asr_step_control: not clipped, clipped hard, not clipped; clip 1,
    decay 1e-5, grad_scale 0.5"""
    _run_rule(device, n, misalign, rule, "ctl")


@pytest.mark.parametrize("rule", RULES)
def test_old_entry_points_follow_float64(device, rule):
    """asr_clip_decay_adam / asr_clip_decay_sgd (still exported) with grad_scale 0.5: the same reference, two loop trips"""
    _run_rule(device, 524289, 1, rule, "old")


@pytest.mark.parametrize("entry", ("ctl", "old"))
@pytest.mark.parametrize("rule", RULES)
def test_update_rules_without_hooks(device, rule, entry):
    """decay = 0 and clip = 0: a gradient of norm 60 goes through unclipped"""
    _run_rule(device, 65537, 1, rule, entry, decay=0.0, clip=0.0)


@pytest.mark.parametrize("entry", ("ctl", "old"))
@pytest.mark.parametrize("rule", RULES)
def test_decay_is_added_after_the_clip(device, rule, entry):
    """WeightDecay follows GradientClipping: the clip factor must not reach the decay term.  With the 1e-5 of the recipes that
    term is below TOL_P for plain SGD; at 1e-2 a clipped step (factor 1 / 30) that scaled it would be off by 1e-3 |p|"""
    _run_rule(device, 65537, 1, rule, entry, decay=f32(1e-2))


@pytest.mark.parametrize("entry", ("ctl", "old"))
@pytest.mark.parametrize("rule", RULES)
def test_update_rules_on_a_zero_gradient(device, rule, entry):
    """norm 0: clip / 0 neither clips nor makes a NaN; SGD's parameters move by the decay alone, Adam stays finite.  The zero step
    comes second, so the velocity and the moments it meets are not zero."""
    n = 65537
    p1, _, _ = _run_rule(device, n, 1, rule, entry, targets=(0.3,))
    p2, state, ctl = _run_rule(device, n, 1, rule, entry, targets=(0.3, None))
    assert np.isfinite(p2).all() and all(np.isfinite(s).all() for s in state)
    if entry == "ctl":
        assert ctl[0] == 0.0 and ctl[1] == GS and ctl[4] == 0.0
    if rule == 0:
        np.testing.assert_allclose(p2, p1 * (1.0 - LR * DECAY), **TOL_P)


# ------------------------------------------------------------------------------------------------ step control
def _assert_ctl(got, applied, want, applied_want, what):
    for i in (0, 3, 5, 6):
        assert got[i] == want[i], (what, i, got, want)
    assert applied == applied_want, (what, applied, applied_want)
    assert got[7] == 0.0, (what, got)
    if np.isfinite(want[4]):
        np.testing.assert_allclose(got[4], want[4], rtol=1e-5, err_msg=what)      # the bar of test_clip_decay_adam's sqnorm_acc
    else:
        assert not np.isfinite(got[4]), (what, got)
    for i in (1, 2):
        assert abs(got[i] - want[i]) <= 1e-6 * abs(want[i]), (what, i, got[i], want[i])


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_step_control_values(device, n, misalign):
    """ctl[0..6] and the applied count over apply, apply (clipped), drop (an inf in the LAST element: the tail of the last loop
    trip sees it), apply: t and alpha_t after the drop are those of the third applied step, and the update kernels launched on the
    dropped control leave parameters and state bit-identical"""
    from asr import _ops
    assert _ops.sqnorm_partials_count(n) == PARTIALS[n]
    A = Arena(device, misalign)
    g = A.new(n, 0.0, name="g")
    p, m, v, vel = (A.new(n, _randn(20 + i, n) * (1.0 if i == 0 else 0.01), name=s) for i, s in enumerate(("p", "m", "v", "velocity")))
    v.abs_()
    ctl = A.new(8, 0.0, name="ctl")
    applied = A.new(1, 0, dtype=torch.int32, name="applied")
    no_abort = A.new(1, 0, dtype=torch.int32, name="abort word")
    partials = A.new(PARTIALS[n], 0.0, name="partials")
    state = (0, 0.0)
    for i, (target, plant) in enumerate(((0.3, False), (30.0, False), (0.3, True), (0.3, False))):
        what = "n = %d, step %d" % (n, i + 1)
        g_np = _grad(10 + i, n, target)
        _assert_clip_is_decided(g_np)
        if plant:
            g_np[-1] = np.inf
        g.copy_(torch.from_numpy(g_np))
        _ops.step_control(g, partials, CLIP, GS, ALPHA, BETA1, BETA2, applied, ctl, no_abort)
        A.check("asr_step_control, " + what)
        want, applied_want, _ = onn.step_control(g_np, state, CLIP, GS, ALPHA, BETA1, BETA2)
        _assert_ctl(ctl.cpu().tolist(), int(applied.cpu()[0]), want, applied_want, what)
        assert want[0] == (1.0 if plant else 0.0)
        if plant:
            snap = A.snapshot()
            _ops.adam_ctl(p, g, m, v, BETA1, BETA2, EPS, DECAY, ctl)
            _ops.sgd_ctl(p, g, vel, 2, LR, MU, DECAY, ctl)
            _ops.sgd_ctl(p, g, None, 0, LR, MU, DECAY, ctl)
            A.assert_unchanged(snap, "the update kernels of a dropped step, " + what)
        state = (applied_want, want[6])
    got = ctl.cpu().tolist()
    assert got[3] == 3.0 and int(applied.cpu()[0]) == 3
    alpha_3 = ALPHA * np.sqrt(1.0 - BETA2 ** 3) / (1.0 - BETA1 ** 3)
    assert abs(got[2] - alpha_3) <= 1e-6 * alpha_3


def test_squared_norm_is_bit_identical_from_launch_to_launch(device):
    """include/asr_hip.h: the partial sums are added in a fixed order, so every data-parallel rank derives the same clipping factor.
    Ten launches on one gradient, a 64 MB fill in between to change which workgroup arrives when"""
    from asr import _ops
    n = 1048653
    A = Arena(device, 1)
    g = A.new(n, _grad(5, n, 30.0), name="g")
    ctl = A.new(8, 0.0, name="ctl")
    applied = A.new(1, 0, dtype=torch.int32, name="applied")
    no_abort = A.new(1, 0, dtype=torch.int32, name="abort word")
    partials = A.new(PARTIALS[n], 0.0, name="partials")
    scratch = torch.empty(16 * 1024 * 1024, dtype=torch.float32, device=device)
    seen = set()
    for i in range(10):
        _ops.fill_(scratch, float(i))
        _ops.step_control(g, partials, CLIP, GS, ALPHA, BETA1, BETA2, applied, ctl, no_abort)
        b = _bits(ctl)
        seen.add((int(b[4]), int(b[1])))
    A.check("ten asr_step_control launches")
    assert len(seen) == 1, seen
    assert float(ctl.cpu()[1]) < GS and int(applied.cpu()[0]) == 10


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_sqnorm_acc_adds_onto_out(device, n, misalign):
    from asr import _ops
    A = Arena(device, misalign)
    g_np = _grad(6, n, 1.5, 1.0)
    g = A.new(n, g_np, name="g")
    out = A.new(1, 3.5, name="out")
    _ops.sqnorm_acc(g, out)
    A.check("asr_sqnorm_acc, n = %d" % n)
    np.testing.assert_allclose(float(out.cpu()[0]), 3.5 + (g_np.astype(np.float64) ** 2).sum(), rtol=1e-5)


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_fill(device, n, misalign):
    from asr import _ops
    A = Arena(device, misalign)
    t = A.new(n, _randn(7, n), name="t")
    _ops.fill_(t, 1.25)
    A.check("asr_fill_f32, n = %d" % n)
    assert bool((t == 1.25).all())
    _ops.fill_(t, 0.0)
    A.check("asr_fill_f32, n = %d" % n)
    assert bool((_bits(t) == 0).all())


# ------------------------------------------------------------------------------------------------ paths asr._ops never takes
def _control_call(fn, g, partials, abort0, abort1, applied, ctl, reserved_index, *loss_scale):
    from asr import _lib
    P = _lib.ptr
    rc = fn(_lib.stream(), P(g), g.numel(), P(partials), P(abort0), P(abort1), CLIP, GS, ALPHA, BETA1, BETA2, P(applied), P(ctl),
            int(reserved_index), *[P(x) for x in loss_scale])
    assert rc == 0
    torch.cuda.synchronize()
    return ctl.cpu().tolist(), int(applied.cpu()[0])


def test_unscaled_entry_second_abort_word_and_reserved_element(device):
    from asr import _lib
    L = _lib.lib()
    n = 65537
    A = Arena(device, 1)
    g_np = _grad(8, n, 30.0)
    g = A.new(n, g_np, name="g")
    partials = A.new(PARTIALS[n], 0.0, name="partials")
    clear = A.new(1, 0, dtype=torch.int32, name="clear abort word")
    raised = A.new(1, 1, dtype=torch.int32, name="raised abort word")

    def fresh():
        return A.new(8, 0.0, name="ctl"), A.new(1, 0, dtype=torch.int32, name="applied")

    # asr_step_control = asr_step_control_scaled with loss_scale = NULL
    ctl_a, app_a = fresh()
    ctl_b, app_b = fresh()
    got_a = _control_call(L.asr_step_control, g, partials, clear, None, app_a, ctl_a, -1)
    got_b = _control_call(L.asr_step_control_scaled, g, partials, clear, None, app_b, ctl_b, -1, None)
    assert torch.equal(_bits(ctl_a), _bits(ctl_b)) and got_a[1] == got_b[1] == 1
    want, applied_want, _ = onn.step_control(g_np, (0, 0.0), CLIP, GS, ALPHA, BETA1, BETA2)
    _assert_ctl(got_a[0], got_a[1], want, applied_want, "asr_step_control")
    # reserved_index = 0 on a finite g[0]: as reserved_index = -1
    ctl_c, app_c = fresh()
    _control_call(L.asr_step_control, g, partials, clear, None, app_c, ctl_c, 0)
    assert torch.equal(_bits(ctl_c), _bits(ctl_a)) and int(app_c.cpu()[0]) == 1
    # abort1 raised, abort0 clear or NULL: dropped because a recurrence gave up
    for abort0 in (clear, None):
        ctl_d, app_d = fresh()
        got, app = _control_call(L.asr_step_control, g, partials, abort0, raised, app_d, ctl_d, -1)
        want, applied_want, _ = onn.step_control(g_np, (0, 0.0), CLIP, GS, ALPHA, BETA1, BETA2, abort=True)
        _assert_ctl(got, app, want, applied_want, "abort1 raised")
        assert got[0] == 1.0 and got[5] == 1.0 and got[6] == 1.0 and app == 0
    # reserved_index = 0 with a NaN in g[0] (a peer gave up): dropped, counted in ctl[6], the loss scale untouched
    bad_np = g_np.copy()
    bad_np[0] = np.nan
    bad = A.new(n, bad_np, name="g with a NaN in front")
    ls = A.new(4, np.array([1024.0, 1.0, 3.0, 0.0], np.float32), name="loss scale")
    ctl_e, app_e = fresh()
    ctl_e[6] = 2.0
    got, app = _control_call(L.asr_step_control_scaled, bad, partials, clear, clear, app_e, ctl_e, 0, ls)
    want, applied_want, ls_want = onn.step_control(bad_np, (0, 2.0), CLIP, GS, ALPHA, BETA1, BETA2, reserved_index=0,
                                                   loss_scale=[1024.0, 1.0, 3.0, 0.0])
    for i in (0, 3, 5, 6):
        assert got[i] == want[i], (i, got, want)
    assert got[0] == 1.0 and got[5] == 1.0 and got[6] == 3.0 and app == applied_want == 0
    assert got[1] == want[1] == GS / 1024.0                         # the factor still carries 1 / S
    assert ls.cpu().tolist() == ls_want == [1024.0, 1.0, 3.0, 0.0]
    # the same NaN with no reserved element: an overflow -- not a give-up, and the scale is halved
    ctl_f, app_f = fresh()
    got, app = _control_call(L.asr_step_control_scaled, bad, partials, clear, clear, app_f, ctl_f, -1, ls)
    assert got[0] == 1.0 and got[5] == 0.0 and got[6] == 0.0 and app == 0 and ls.cpu().tolist() == [512.0, 0.0, 3.0, 1.0]
    A.check("the direct asr_step_control calls")


def test_gather_abort(device):
    from asr import _lib
    L, P = _lib.lib(), _lib.ptr
    A = Arena(device, 1)
    words = [A.new(1, 0, dtype=torch.int32, name="abort word %d" % i) for i in range(3)]
    any_word = A.new(1, 7, dtype=torch.int32, name="any_word")
    poison = A.new(1, 1.5, name="poison")

    def gather(table, count, out=any_word, mark=poison):
        t = None if table is None else torch.tensor(table, dtype=torch.int64).to(device)
        assert L.asr_gather_abort(_lib.stream(), P(t), count, P(out), P(mark)) == 0
        A.check("asr_gather_abort")
        return int(any_word.cpu()[0]), float(poison.cpu()[0])

    table = [w.data_ptr() for w in words]
    assert gather(table, 3) == (0, 1.5)                             # none raised: word 0, poison untouched
    words[1].fill_(1)
    got = gather(table, 3)
    assert got[0] == 1 and np.isnan(got[1])                         # one raised: word 1, a NaN planted
    poison.fill_(1.5)
    assert gather([table[0], 0, table[2]], 3) == (0, 1.5)           # a NULL entry is skipped
    got = gather([0, table[1], 0], 3)
    assert got[0] == 1 and np.isnan(got[1])
    poison.fill_(1.5)
    any_word.fill_(7)
    assert gather(table, 1) == (0, 1.5)                             # only the first `n` entries count
    any_word.fill_(7)
    assert gather(None, 0) == (0, 1.5)                              # n = 0: accepted, nothing raised
    words[0].fill_(-5)                                              # any non-zero value raises; either output may be NULL
    any_word.fill_(7)
    assert gather(table, 3, mark=None) == (1, 1.5)
    any_word.fill_(7)
    got = gather(table, 3, out=None)
    assert got[0] == 7 and np.isnan(got[1])


def test_bad_arguments_are_refused_before_any_launch(device):
    """ASR_ERR_BAD_ARG, and no buffer touched: the sentinels and the payloads are what they were"""
    from asr import _lib
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream()
    n = 257
    A = Arena(device, 1)
    p, g, m, v = (A.new(n, _randn(30 + i, n), name=s) for i, s in enumerate(("p", "g", "m", "v")))
    ctl = A.new(8, 0.5, name="ctl")
    applied = A.new(1, 3, dtype=torch.int32, name="applied")
    word = A.new(1, 1, dtype=torch.int32, name="abort word")
    partials = A.new(2, 0.25, name="partials")
    sq = A.new(1, 1.0, name="sqnorm")
    ls = A.new(4, np.array([64.0, 1.0, 3.0, 0.0], np.float32), name="loss scale")
    table = A.new(2, 0, dtype=torch.int32, name="pointer table")       # one int64 slot, never read
    snap = A.snapshot()
    p_, g_, m_, v_, ctl_, app_, w_, part_, sq_, ls_ = (P(x) for x in (p, g, m, v, ctl, applied, word, partials, sq, ls))
    adam = (ALPHA, BETA1, BETA2, EPS, DECAY, CLIP, GS)
    sgd = (LR, MU, DECAY, CLIP, GS)
    control = (CLIP, GS, ALPHA, BETA1, BETA2)
    calls = {
        "fill n = 0": lambda: L.asr_fill_f32(S, p_, 0, 1.0),
        "fill n < 0": lambda: L.asr_fill_f32(S, p_, -1, 1.0),
        "fill NULL": lambda: L.asr_fill_f32(S, None, n, 1.0),
        "sqnorm n = 0": lambda: L.asr_sqnorm_acc(S, g_, 0, sq_),
        "sqnorm NULL out": lambda: L.asr_sqnorm_acc(S, g_, n, None),
        "clip_decay_adam n = 0": lambda: L.asr_clip_decay_adam(S, p_, g_, m_, v_, 0, *adam, sq_, 1),
        "clip_decay_adam step = 0": lambda: L.asr_clip_decay_adam(S, p_, g_, m_, v_, n, *adam, sq_, 0),
        "clip_decay_adam NULL m": lambda: L.asr_clip_decay_adam(S, p_, g_, None, v_, n, *adam, sq_, 1),
        "clip_decay_sgd n = 0": lambda: L.asr_clip_decay_sgd(S, p_, g_, v_, 0, 1, *sgd, sq_),
        "clip_decay_sgd kind = 3": lambda: L.asr_clip_decay_sgd(S, p_, g_, v_, n, 3, *sgd, sq_),
        "clip_decay_sgd kind = -1": lambda: L.asr_clip_decay_sgd(S, p_, g_, v_, n, -1, *sgd, sq_),
        "clip_decay_sgd kind = 1, v = NULL": lambda: L.asr_clip_decay_sgd(S, p_, g_, None, n, 1, *sgd, sq_),
        "clip_decay_sgd kind = 2, v = NULL": lambda: L.asr_clip_decay_sgd(S, p_, g_, None, n, 2, *sgd, sq_),
        "step_control n = 0": lambda: L.asr_step_control(S, g_, 0, part_, w_, None, *control, app_, ctl_, -1),
        "step_control reserved_index = n": lambda: L.asr_step_control(S, g_, n, part_, w_, None, *control, app_, ctl_, n),
        "step_control NULL ctl": lambda: L.asr_step_control(S, g_, n, part_, w_, None, *control, app_, None, -1),
        "step_control NULL partials": lambda: L.asr_step_control(S, g_, n, None, w_, None, *control, app_, ctl_, -1),
        "step_control NULL applied": lambda: L.asr_step_control(S, g_, n, part_, w_, None, *control, None, ctl_, -1),
        "step_control_scaled n = 0": lambda: L.asr_step_control_scaled(S, g_, 0, part_, w_, None, *control, app_, ctl_, -1, ls_),
        "step_control_scaled reserved_index = n": lambda: L.asr_step_control_scaled(S, g_, n, part_, w_, None, *control, app_, ctl_, n, ls_),
        "step_control_scaled NULL ctl": lambda: L.asr_step_control_scaled(S, g_, n, part_, w_, None, *control, app_, None, -1, ls_),
        "adam_ctl n = 0": lambda: L.asr_adam_ctl(S, p_, g_, m_, v_, 0, BETA1, BETA2, EPS, DECAY, ctl_),
        "adam_ctl NULL ctl": lambda: L.asr_adam_ctl(S, p_, g_, m_, v_, n, BETA1, BETA2, EPS, DECAY, None),
        "adam_ctl NULL v": lambda: L.asr_adam_ctl(S, p_, g_, m_, None, n, BETA1, BETA2, EPS, DECAY, ctl_),
        "sgd_ctl n = 0": lambda: L.asr_sgd_ctl(S, p_, g_, v_, 0, 1, LR, MU, DECAY, ctl_),
        "sgd_ctl kind = 3": lambda: L.asr_sgd_ctl(S, p_, g_, v_, n, 3, LR, MU, DECAY, ctl_),
        "sgd_ctl kind = -1": lambda: L.asr_sgd_ctl(S, p_, g_, v_, n, -1, LR, MU, DECAY, ctl_),
        "sgd_ctl kind = 1, v = NULL": lambda: L.asr_sgd_ctl(S, p_, g_, None, n, 1, LR, MU, DECAY, ctl_),
        "sgd_ctl kind = 2, v = NULL": lambda: L.asr_sgd_ctl(S, p_, g_, None, n, 2, LR, MU, DECAY, ctl_),
        "sgd_ctl NULL ctl": lambda: L.asr_sgd_ctl(S, p_, g_, v_, n, 1, LR, MU, DECAY, None),
        "gather_abort n < 0": lambda: L.asr_gather_abort(S, P(table), -1, w_, sq_),
        "gather_abort NULL table": lambda: L.asr_gather_abort(S, None, 1, w_, sq_),
        "gather_abort no output": lambda: L.asr_gather_abort(S, P(table), 1, None, None),
    }
    for what, call in calls.items():
        assert call() == BAD_ARG, what
        A.assert_unchanged(snap, what)


# ------------------------------------------------------------------------------------------------ the Optimizer classes
SHAPES = ((70, 45), (29,), (1,), (64,))         # two padded to 64 floats, a single element, one that fills its slot exactly
OFFSETS = (64, 64 + 3200, 64 + 3264, 64 + 3328)
TOTAL = 64 + 3200 + 64 + 64 + 64
NREAL = 70 * 45 + 29 + 1 + 64


def _four_parameter_link(device, seed):
    from asr.link import Link, Parameter

    class Four(Link):
        def __init__(self):
            super().__init__()
            gen = torch.Generator().manual_seed(seed)
            with self.init_scope():
                self.a = Parameter(torch.randn(SHAPES[0], generator=gen))
                self.b = Parameter(torch.randn(SHAPES[1], generator=gen))
                self.c = Parameter(torch.randn(SHAPES[2], generator=gen))
                self.d = Parameter(torch.randn(SHAPES[3], generator=gen))

    return Four().to_gpu(device.index)


def _real_mask():
    mask = np.zeros(TOTAL, bool)
    for o, s in zip(OFFSETS, SHAPES):
        mask[o:o + int(np.prod(s))] = True
    return mask


class ClassHarness(object):
    """steps an Optimizer of asr.optimizers on the four-parameter link beside the float64 oracle, which sees the concatenated real
    elements (one joint norm) and keeps its own learning rate, momentum and applied-step count"""

    def __init__(self, device, name, hooks, seed=0):
        from asr import optimizers as O
        self.O, self.name, self.device = O, name, device
        self.link = _four_parameter_link(device, seed)
        self.opt = O.get_optimizer(name, 0.05, 0.8)
        self.opt.setup(self.link)
        self.clip, self.decay = (1.0, f32(1e-3)) if hooks else (0.0, 0.0)
        if hooks:
            self.opt.add_hook(O.GradientClipping(1.0))
            self.opt.add_hook(O.WeightDecay(1e-3))
        self.opt.cleargrads()
        self.rule = "adam" if name == "adam" else {"sgd": 0, "msgd": 1, "nesterov": 2}[name]
        self.lr, self.mu, self.applied = 0.05, 0.8, 0
        self.mask = torch.from_numpy(_real_mask()).to(device)
        assert tuple(self.opt._flat["offsets"]) == OFFSETS and self.opt.flat_parameters().numel() == TOTAL
        self.check_layout()

    def params(self):
        return [self.link.a, self.link.b, self.link.c, self.link.d]

    def state(self):
        if self.rule == "adam":
            return (self.opt.m, self.opt.v)
        return (self.opt.vel,) if self.rule else ()

    def real(self, flat):
        return flat[self.mask].cpu().numpy().astype(np.float64)

    def check_layout(self):
        """p.data / p.grad are views into the flat buffers; reserved and padding elements are exactly 0 everywhere"""
        P, G = self.opt.flat_parameters(), self.opt.flat_gradients()
        for p, o in zip(self.params(), OFFSETS):
            assert p.grad is not None and p.grad.data_ptr() == G.data_ptr() + 4 * o and p.grad.shape == p.shape
            assert p.data_ptr() == P.data_ptr() + 4 * o
        for buf in (P,) + self.state():
            assert buf.numel() == TOTAL and bool((buf[~self.mask] == 0).all())
        if self.rule == 0:
            assert self.opt.vel is None and [b for b in self.opt._state_buffers() if b is not None] == []

    def write_grad(self, g_np):
        o = 0
        for p in self.params():
            p.grad.copy_(torch.from_numpy(g_np[o:o + p.numel()].reshape(p.shape)))
            o += p.numel()
        assert o == NREAL

    def step(self, seed, target, what, nan_at=None):
        g_np = _grad(seed, NREAL, target, 1.0)
        if nan_at is not None:
            g_np[nan_at] = np.nan
        elif self.clip > 0:
            _assert_clip_is_decided(g_np, self.clip, 1.0)
        p0 = self.real(self.opt.flat_parameters())
        s0 = tuple(self.real(s) for s in self.state())
        snap = [t.clone() for t in (self.opt.flat_parameters(),) + self.state()]
        self.write_grad(g_np)
        self.opt.update()
        torch.cuda.synchronize()
        self.check_layout()
        if nan_at is not None:
            for a, b in zip(snap, (self.opt.flat_parameters(),) + self.state()):
                assert torch.equal(_bits(a), _bits(b)), what
            assert self.opt.applied_steps() == self.applied, what
            return
        self.applied += 1
        lr, mu = f32(self.lr), f32(self.mu)
        p_want, s_want = _oracle_step(self.rule, p0, g_np, s0 if s0 else (None,), self.applied, lr, mu, self.decay, self.clip, 1.0,
                                      alpha=lr, beta1=mu)
        got_p = self.real(self.opt.flat_parameters())
        assert np.isfinite(got_p).all()
        np.testing.assert_allclose(got_p, p_want, err_msg="p, " + what, **TOL_P)
        if self.rule != 0:
            np.testing.assert_allclose(self.real(self.state()[0]), s_want[0], err_msg="m / velocity, " + what, **TOL_M)
        if self.rule == "adam":
            np.testing.assert_allclose(self.real(self.state()[1]), s_want[1], err_msg="v, " + what, **TOL_V)
            assert float(self.opt._flat["ctl"][3]) == float(self.applied), what
        assert self.opt.applied_steps() == self.applied, what


@pytest.mark.parametrize("hooks", (True, False), ids=("hooks", "no_hooks"))
@pytest.mark.parametrize("name", ("sgd", "msgd", "nesterov", "adam"))
def test_optimizer_classes_follow_float64(device, name, hooks):
    """six update() calls without a lossfun on gradients written into p.grad: learning rate and momentum change after step 2, the
    learning rate decays after step 4, step 5 carries a NaN and is dropped, step 6 is the fifth applied one (Adam's t = 5)"""
    from asr import optimizers as O
    h = ClassHarness(device, name, hooks)
    tag = "%s, %s, step " % (name, "hooks" if hooks else "no hooks")
    h.step(41, 0.3, tag + "1")
    h.step(42, 30.0, tag + "2")
    O.set_learning_rate(h.opt, 0.01)
    O.set_momentum(h.opt, 0.5)
    h.lr, h.mu = 0.01, 0.5
    assert O.get_learning_rate(h.opt) == 0.01
    h.step(43, 0.5, tag + "3")
    h.step(44, 5.0, tag + "4")
    assert O.decay_learning_rate(h.opt, 0.5, 1e-6) is None and O.get_learning_rate(h.opt) == 0.005
    h.lr = 0.005
    h.step(45, 0.4, tag + "5 (NaN)", nan_at=3150 + 7)
    assert h.applied == 4 and h.opt.applied_steps() == 4 and h.opt.t == 5
    h.step(46, 0.4, tag + "6")
    assert h.applied == 5 and h.opt.applied_steps() == 5


@pytest.mark.parametrize("name", ("msgd", "nesterov"))
def test_momentum_survives_a_reflatten(device, name):
    """as test_optimiser_state_survives_a_reflatten (tests/test_model_gpu.py) does it for Adam's moments: one parameter moves to
    fresh storage, the flat buffers are rebuilt, and velocity, parameters and the applied count come along bit for bit"""
    h = ClassHarness(device, name, True, seed=1)
    h.step(51, 0.3, name + ", step 1")
    h.step(52, 30.0, name + ", step 2")
    old_vel = h.opt.vel
    vel_before = [_bits(h.opt.vel[o:o + p.numel()]) for p, o in zip(h.params(), OFFSETS)]
    w_before = [_bits(p.detach()) for p in h.params()]
    assert float(h.opt.vel.abs().sum()) > 0
    p0 = h.params()[1]
    p0.data = p0.data.clone()
    h.opt._ensure_flat()
    assert h.opt.vel is not old_vel and h.opt.applied_steps() == 2
    for p, o, vb, wb in zip(h.params(), OFFSETS, vel_before, w_before):
        assert torch.equal(_bits(h.opt.vel[o:o + p.numel()]), vb)
        assert torch.equal(_bits(p.detach()), wb)
    h.check_layout()
    h.step(53, 0.5, name + ", the step after the re-flatten")
