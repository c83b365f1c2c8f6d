"""The host side of the streaming CTC beam search (asr_ctc_beam_stream_*: include/asr_hip.h): the two size
queries, and that every entry is declared, bound and exported by both builds.  No GPU."""
import ctypes
import os

from conftest import PKG
from test_abi import _header_functions

ENTRIES = ["asr_ctc_beam_stream_state_bytes", "asr_ctc_beam_stream_workspace_bytes", "asr_ctc_beam_stream_reset",
           "asr_ctc_beam_stream_advance", "asr_ctc_beam_stream_result"]


def test_every_stream_entry_is_declared_bound_and_exported_in_both_builds():
    from asr import _lib
    declared = _header_functions()
    half = ctypes.CDLL(os.path.join(PKG, "libasr_hip_f16.so"))
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
        assert hasattr(half, name), name
    from asr import _ops, error
    assert callable(error.BeamStream)
    for name in ENTRIES:
        assert callable(getattr(_ops, name[len("asr_"):])), name


def test_state_query_runs_on_the_host_and_grows_with_every_argument():
    from asr import _lib
    q = _lib.lib().asr_ctc_beam_stream_state_bytes
    for bad in ((0, 16, 100, 0, 0), (4, 0, 100, 1, 1), (4, 16, 0, 0, 0), (-1, 16, 100, 0, 0), (4, -2, 100, 0, 0), (4, 16, -3, 1, 0)):
        assert q(*bad) == 0, bad
    B, W, F = 4, 16, 100
    for lm in (0, 1):
        for bias in (0, 1):
            n = q(B, W, F, lm, bias)
            # the prefix table alone is B * F * W int2 nodes; the beam's fields are 40 bytes per slot, + 16 with a model, + 8 with a graph
            assert n >= B * F * W * 8 + B * W * (40 + 16 * lm + 8 * bias)
            assert n % 256 == 0
            assert q(2 * B, W, F, lm, bias) > n and q(B, 2 * W, F, lm, bias) > n and q(B, W, 2 * F, lm, bias) > n
            assert q(B + 1, W, F, lm, bias) >= n and q(B, W + 1, F, lm, bias) >= n and q(B, W, F + 1, lm, bias) >= n
    assert q(B, W, F, 1, 0) > q(B, W, F, 0, 0) and q(B, W, F, 0, 1) > q(B, W, F, 0, 0)
    assert q(B, W, F, 1, 1) > q(B, W, F, 1, 0) and q(B, W, F, 1, 1) > q(B, W, F, 0, 1)
    assert q(1, 1, 1, 0, 0) >= 8
    assert q(32, 128, 1000, 1, 1) >= 32 * 1000 * 128 * 8


def test_workspace_query_runs_on_the_host_and_grows_with_every_argument():
    from asr import _lib
    q = _lib.lib().asr_ctc_beam_stream_workspace_bytes
    for bad in ((0, 4, 50, 16, 16), (10, 0, 50, 16, 16), (10, 4, 0, 16, 16), (10, 4, 50, 0, 16), (10, 4, 50, 16, 0), (-1, 4, 50, 16, 16)):
        assert q(*bad) == 0, bad
    Tc, B, V, W, K = 100, 4, 50, 16, 16
    n = q(Tc, B, V, W, K)
    # per row: log-sum-exp, lp[blank], the count, and top_k (id, lp) pairs
    assert n >= Tc * B * (12 + 8 * K) and n % 256 == 0
    assert q(2 * Tc, B, V, W, K) > n and q(Tc, 2 * B, V, W, K) > n and q(Tc, B, V, W, 2 * K) > n
    assert q(Tc, B, 8, W, K) < n                       # top_k acts as V - 1 where V is small
    assert q(Tc, B, 2 * V, W, K) >= n and q(Tc, B, V, 2 * W, K) >= n
    # the chunk's scratch holds no prefix table: that is the state's
    assert n < _lib.lib().asr_ctc_beam_workspace_bytes(Tc, B, V, W, K)
    assert q(Tc, B, V, 2 * W, K) == n
