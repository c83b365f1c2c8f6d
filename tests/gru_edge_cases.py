"""The cases of tests/test_gru_edges_gpu.py and their inputs -- shared with tests/test_oracle_gru.py, which checks on the CPU that
the caps of oracle/gru_step.py can tell a right kernel from a wrong one on exactly these inputs."""
import collections

import numpy as np
import torch

Case = collections.namedtuple("Case", "group T B H ndir mode gi16 g16 lens sat fwd_only")


def _case(group, T, B, H, ndir=2, mode=0, gi16=True, g16=True, lens=None, sat=0.0, fwd_only=False):
    return Case(group, T, B, H, ndir, mode, gi16, g16, None if lens is None else tuple(int(v) for v in lens), float(sat), fwd_only)


def case_id(c):
    s = "%s-T%d-B%d-H%d-d%d-m%d" % (c.group, c.T, c.B, c.H, c.ndir, c.mode)
    if not (c.gi16 and c.g16):
        s += "-f32forms"
    if c.lens is not None:
        s += "-len" + "".join(str(min(v, 9)) for v in c.lens[:8])
    if c.sat:
        s += "-sat%g" % c.sat
    return s


def mixed_lengths(T, B):
    """1, T and values between, cycled over the batch"""
    pat = [T, 1, max(1, T // 2), T, min(T, 2), max(1, T - 1)]
    return [pat[b % len(pat)] for b in range(B)]


def _cases():
    out = []
    # (a) widths that leave a wave of the K split partly filled, and the template instances no other test reaches
    for H in (32, 96, 160, 224, 320, 352, 448):
        for mode in (0, 1, 2, 4, 7):
            out.append(_case("a", 7, 5, H, 2, mode))
    for H in (96, 320):
        for mode in (0, 1, 2, 4, 7):
            out.append(_case("a", 7, 5, H, 1, mode))
    for H in (160, 320):
        for mode in (9, 10):
            out.append(_case("a", 7, 5, H, 2, mode))
    # (b) forward only beyond H = 512
    for H in (544, 1024):
        for mode in (0, 1):
            out.append(_case("b", 3, 3, H, 2, mode, fwd_only=True))
    # (c) sequences shorter than the pipelines, through each family
    fams = [dict(H=64, B=5, mode=0), dict(H=256, B=20, mode=0), dict(H=256, B=20, mode=0, gi16=False, g16=False), dict(H=128, B=5, mode=0),
            dict(H=192, B=5, mode=0), dict(H=64, B=5, mode=1), dict(H=128, B=5, mode=2),
            # modes 9 / 10 where they select what they exist for: the partial-sum backward asked for, and with a forged split placement
            # (its placement-free stores); the forward pass of these modes is mode 0's
            dict(H=128, B=5, mode=9), dict(H=256, B=20, mode=10)]
    for f in fams:
        for T in (1, 2, 3, 4, 5):
            out.append(_case("c", T, ndir=2, **f))
            out.append(_case("c", T, ndir=2, lens=mixed_lengths(T, f["B"]), **f))
    # (d) batch borders
    for H in (128, 160):
        for B in (1, 4, 5, 8, 9, 16, 17, 31, 32):
            out.append(_case("d", 6, B, H))
    out += [_case("d", 6, 33, 256), _case("d", 6, 65, 256), _case("d", 6, 33, 160)]
    out += [_case("d", 6, B, 128, mode=10) for B in (1, 5, 17, 32)]        # (the forged placement of the partial-sum backward at the borders)
    # (e) lengths: a dead utterance (x_len = 0) between live ones, all 1, all T
    for f in (dict(H=128, B=5, mode=0), dict(H=256, B=20, mode=0), dict(H=96, B=5, mode=1), dict(H=160, B=5, mode=2)):
        T, B = 6, f["B"]
        dead_mid = [T if b % 2 == 0 else 3 for b in range(B)]
        dead_mid[B // 2] = 0
        for lens in (dead_mid, [1] * B, [T] * B, [0] + [T] * (B - 1)):
            out.append(_case("e", T, ndir=2, lens=lens, **f))
    # (f) saturated gates: |gi + gh| up to ~20, ~90 (__expf overflows), ~200; 14: r, z below the half format's normal range
    for sat in (14.0, 20.0, 90.0, 200.0):
        out.append(_case("f", 4, 20, 256, 2, 0, sat=sat))
        out.append(_case("f", 4, 5, 96, 2, 1, sat=sat))
    return out


CASES = _cases()


def input_key(c):
    """cases that differ only in the kernel form asked for share their inputs"""
    return (c.T, c.B, c.H, c.ndir, c.lens, c.sat)


_INPUTS = {}


def make_inputs(c):
    """-> dict: gi (T*B, ndir*3H) float32 (the caller rounds it to bf16 where the kernel takes that), whh (ndir, 3H, H) bf16-valued
    float32, bhh (ndir*3H), dy (T*B, H) bf16-valued, x_len (B) int32 or None.
    Scales: |w| ~ U(-2 / sqrt(H), 2 / sqrt(H)) and a non-zero b_hh keep |h| ~ 0.5 and the share of one 32-wide K slice
    in gh at ~0.3 -- three orders above the caps; gi ~ 0.7 N(0, 1) keeps the gates of groups (a) to (e) away from saturation."""
    key = input_key(c)
    if key in _INPUTS:
        return _INPUTS[key]
    T, B, H, ndir = c.T, c.B, c.H, c.ndir
    g = torch.Generator().manual_seed(1000003 * T + 1009 * B + 7 * H + ndir + (0 if c.lens is None else 31 + sum(c.lens)))
    k = 2.0 / np.sqrt(H)
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    whh = bf(torch.empty(ndir, 3 * H, H).uniform_(-k, k, generator=g))
    bhh = torch.empty(ndir * 3 * H).uniform_(-0.5, 0.5, generator=g)
    gi = 0.7 * torch.randn(T, B, ndir, 3, H, generator=g) + torch.empty(ndir, 3, H).uniform_(-0.3, 0.3, generator=g)    # (a non-zero b_ih inside)
    dy = bf(torch.randn(T * B, H, generator=g))
    if c.sat:
        s = c.sat
        gi = torch.randn(T, B, ndir, 3, H, generator=g) * (s / 3.0)
        sign = torch.where(torch.rand(T, ndir, 3, H, generator=g) < 0.5, -1.0, 1.0)
        gi[:, 0] = s * sign                                     # a row whose r, z, n all sit at their limits, every sign pattern
        if B > 1:                                               # a row with r, z tiny but not zero (below the half normal range at s = 14)
            gi[:, 1, :, :2] = -s * (0.75 + 0.25 * torch.rand(T, ndir, 2, H, generator=g))
    x_len = None if c.lens is None else torch.tensor(c.lens, dtype=torch.int32)
    res = dict(gi=gi.reshape(T * B, ndir * 3 * H).contiguous(), whh=whh, bhh=bhh, dy=dy, x_len=x_len)
    if len(_INPUTS) > 64:
        _INPUTS.clear()
    _INPUTS[key] = res
    return res
