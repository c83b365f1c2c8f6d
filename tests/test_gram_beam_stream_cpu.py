"""The host side of the streaming Gram-CTC beam search (asr_gram_ctc_beam_stream_*: include/asr_hip.h): the
two size queries, and that every entry is declared, bound and exported by both builds.  No GPU."""
import ctypes
import os

from conftest import PKG
from test_abi import _header_functions

ENTRIES = ["asr_gram_ctc_beam_stream_state_bytes", "asr_gram_ctc_beam_stream_workspace_bytes", "asr_gram_ctc_beam_stream_reset",
           "asr_gram_ctc_beam_stream_advance", "asr_gram_ctc_beam_stream_result"]


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
    assert callable(error.GramBeamStream)
    for name in ENTRIES:
        assert callable(getattr(_ops, name[len("asr_"):])), name


def test_state_query_runs_on_the_host_and_grows_with_every_argument():
    from asr import _lib
    q = _lib.lib().asr_gram_ctc_beam_stream_state_bytes
    for bad in ((0, 16, 100, 0), (4, 0, 100, 1), (4, 16, 0, 0), (-1, 16, 100, 0), (4, -2, 100, 0), (4, 16, -3, 1)):
        assert q(*bad) == 0, bad
    B, W, F = 4, 16, 100
    for lm in (0, 1):
        n = q(B, W, F, lm)
        # the prefix table alone is 2 * B * F * W int2 nodes; the beam's fields are 3 masses, 3 hashes and 7 ints: 64 bytes per
        # slot, + 4 with a model
        assert n >= 2 * B * F * W * 8 + B * W * (64 + 4 * lm)
        assert n % 256 == 0
        assert q(2 * B, W, F, lm) > n and q(B, 2 * W, F, lm) > n and q(B, W, 2 * F, lm) > n
        assert q(B + 1, W, F, lm) >= n and q(B, W + 1, F, lm) >= n and q(B, W, F + 1, lm) >= n
    assert q(B, W, F, 1) > q(B, W, F, 0)
    assert q(1, 1, 1, 0) >= 16
    assert q(32, 128, 1000, 1) >= 2 * 32 * 1000 * 128 * 8
    # two characters per frame: the table is twice the CTC stream's
    assert q(B, W, F, 0) > _lib.lib().asr_ctc_beam_stream_state_bytes(B, W, F, 0, 0)


def test_workspace_query_runs_on_the_host_and_does_not_grow_with_the_beam():
    from asr import _lib
    q = _lib.lib().asr_gram_ctc_beam_stream_workspace_bytes
    for bad in ((0, 4, 50, 16, 16), (10, 0, 50, 16, 16), (10, 4, 0, 16, 16), (10, 4, 50, 0, 16), (10, 4, 50, 16, 0), (-1, 4, 50, 16, 16)):
        assert q(*bad) == 0, bad
    Tc, B, V, W, K = 100, 4, 50, 16, 16
    n = q(Tc, B, V, W, K)
    # per row: log-sum-exp, lp[blank], the count, top_k (id, lp) pairs and their top_k spellings
    assert n >= Tc * B * (12 + 16 * K) and n % 256 == 0
    assert q(2 * Tc, B, V, W, K) > n and q(Tc, 2 * B, V, W, K) > n and q(Tc, B, V, W, 2 * K) > n
    assert q(Tc, B, 8, W, K) < n                       # top_k acts as V - 1 where V is small
    assert q(Tc, B, 2 * V, W, K) >= n
    # the chunk's scratch holds no prefix table: that is the state's
    assert q(Tc, B, V, 2 * W, K) == n and q(Tc, B, V, 128, K) == n and q(Tc, B, V, 1, K) == n
    assert n < _lib.lib().asr_gram_ctc_beam_workspace_bytes(Tc, B, V, W, K)
    assert n > _lib.lib().asr_ctc_beam_stream_workspace_bytes(Tc, B, V, W, K)
