"""The two dispatch queries of csrc/gru.hip -- asr_gru_gates_f16_ok and asr_gru_fwd_accepts_bf16_gi, on whose word asr/_ops.py allocates
half-precision gates and bf16 input projections -- against their answers frozen from the library BEFORE the dispatch became one plan
(DESIGN.md section 28): tests/golden/gru_dispatch.npz holds the five axes and both answers as packed bits, in (T, B, H, ndir, mode) order.

The table was taken on a host without a device, where the compute-unit bound of can_persist is inactive (device_cus() == 0).  With a
device the bound refuses the persistent forms whose largest grid exceeds its CUs, and both answers are then 0: the test applies that one
rule to the table.  The table is for the default flags (ASR_DEBUG is read once per process)."""
import os

import numpy as np
import pytest

from conftest import ROOT


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 0


def _grid_need(B, H, ndir):
    """workgroups of the largest persistent grid of can_persist, for the batch or for a slab of 32 rows"""
    Be = np.minimum(B, 32)
    rec8, rec4 = (ndir * ((Be + 7) // 8) + 7) & ~7, (ndir * ((Be + 3) // 4) + 7) & ~7
    return np.maximum(rec8 * (H // 16), rec4 * ((H + 31) // 32))


@pytest.fixture(scope="module")
def answers():
    if any(k in os.environ.get("ASR_DEBUG", "") for k in ("fwd_ring", "gru_fwd_rows")):
        pytest.skip("the table is for the default flags")
    from asr import _lib
    lib = _lib.lib()
    tab = np.load(os.path.join(ROOT, "tests", "golden", "gru_dispatch.npz"))
    axes = [tab[k].tolist() for k in ("T", "B", "H", "ndir", "mode")]
    shape = tuple(len(a) for a in axes)
    n = int(np.prod(shape))
    want = {k: np.unpackbits(tab[k])[:n].reshape(shape) for k in ("gates_f16_ok", "fwd_accepts_bf16_gi")}
    fg, fa = lib.asr_gru_gates_f16_ok, lib.asr_gru_fwd_accepts_bf16_gi
    got = {k: np.zeros(shape, np.uint8) for k in want}
    g, a = got["gates_f16_ok"], got["fwd_accepts_bf16_gi"]
    for it, T in enumerate(axes[0]):
        for ib, B in enumerate(axes[1]):
            for ih, H in enumerate(axes[2]):
                for id_, nd in enumerate(axes[3]):
                    for im, m in enumerate(axes[4]):
                        g[it, ib, ih, id_, im] = fg(T, B, H, nd, m)
                        a[it, ib, ih, id_, im] = fa(T, B, H, nd, m)
    return axes, want, got


def test_the_grid_is_the_one_asked_for(answers):
    (Ts, Bs, Hs, ndirs, modes), _, _ = answers
    assert set(Bs) >= set(range(1, 35)) | {48, 63, 64, 65, 66, 128, 129}
    assert set(Hs) >= set(range(16, 1041, 16)) and len([H for H in Hs if H <= 0 or H % 16]) >= 2
    assert ndirs == [1, 2] and modes == list(range(-1, 12))
    # T * B * ndir * 3H * 2 = 2^31 at (B, H) = (32, 512) lies between 10922 and 10923 (ndir 2), 21845 and 21846 (ndir 1)
    assert set(Ts) >= {1, 1000, 10922, 10923, 21845, 21846}
    assert 10922 * 32 * 2 * 3 * 512 * 2 < 2 ** 31 <= 10923 * 32 * 2 * 3 * 512 * 2 and 21845 * 32 * 3 * 512 * 2 < 2 ** 31 <= 21846 * 32 * 3 * 512 * 2


def test_queries_answer_as_before_the_plan(answers):
    (Ts, Bs, Hs, ndirs, modes), want, got = answers
    cus = _cus()
    B, H, nd = np.array(Bs)[:, None, None], np.array(Hs)[None, :, None], np.array(ndirs)[None, None, :]
    fits = (cus == 0) | (_grid_need(B, H, nd) <= cus)                 # (B, H, ndir)
    for k in want:
        w = want[k] * fits[None, :, :, :, None].astype(np.uint8)
        bad = np.argwhere(w != got[k])
        assert len(bad) == 0, (k, len(bad), [(Ts[i], Bs[j], Hs[l], ndirs[m], modes[n]) for i, j, l, m, n in bad[:5]])
    assert want["gates_f16_ok"].sum() > 1000 and want["fwd_accepts_bf16_gi"].sum() > 10000        # (the table is not empty)


def test_half_gates_imply_bf16_projections(answers):
    """asr/_ops.py allocates bf16 input projections wherever it allocates half gates; asr_gru_fwd_accepts_bf16_gi maps modes 9 / 10 to
    the forward pass's mode 0 itself, as the launch entry does"""
    _, _, got = answers
    assert not np.any((got["gates_f16_ok"] == 1) & (got["fwd_accepts_bf16_gi"] == 0))


def test_refused_sizes_answer_no(answers):
    (Ts, Bs, Hs, ndirs, modes), _, got = answers
    refused = np.array([H <= 0 or H % 32 != 0 for H in Hs])
    assert refused.sum() >= 2
    for k in got:
        assert not got[k][:, :, refused].any(), k
    from asr import _lib
    lib = _lib.lib()
    for T, B, H, nd in ((0, 4, 128, 2), (-1, 4, 128, 2), (3, 0, 128, 2), (3, -4, 128, 2), (3, 4, 0, 2), (3, 4, -128, 2), (3, 4, 128, 0), (3, 4, 128, 3),
                        (3, 4, 144, 2), (3, 4, 520, 1)):
        for m in modes:
            assert lib.asr_gru_gates_f16_ok(T, B, H, nd, m) == 0 and lib.asr_gru_fwd_accepts_bf16_gi(T, B, H, nd, m) == 0, (T, B, H, nd, m)
