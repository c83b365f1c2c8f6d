"""The push semantics (tests/stream_push_reference.py) do what a stream needs: however a sequence is cut -- chunks of 0 rows, fewer
than K, more than K -- running a K-tap layer on every window and keeping the rows it may emit gives the layer run on the whole
sequence.  Both modes, restarts of single slots in the middle."""
import numpy as np
import pytest

import stream_push_reference as sp


def _taps(window_rows, weights):
    """a K + 1 tap layer on consecutive rows: out[i] = sum_k weights[k] * rows[i + k], for every i with all taps inside"""
    K = len(weights) - 1
    n = window_rows.shape[0] - K
    if n <= 0:
        return np.zeros((0,) + window_rows.shape[1:])
    return sum(weights[k] * window_rows[k:k + n] for k in range(K + 1))


def _whole(seq, weights, mode):
    """the layer over a whole utterance: causal (K zero rows in front) in context mode, lookahead (K zero rows behind) otherwise"""
    K = len(weights) - 1
    pad = np.zeros((K,) + seq.shape[1:])
    rows = np.concatenate([pad, seq] if mode == sp.CONTEXT else [seq, pad], axis=0)
    return _taps(rows, weights)


@pytest.mark.parametrize("mode", [sp.CONTEXT, sp.LOOKAHEAD])
@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_any_cut_gives_the_whole_sequence(mode, K, seed):
    rng = np.random.default_rng(100 * K + seed + 7 * mode)
    B, R, max_chunk = 4, 3, 2 * K + 3
    weights = rng.standard_normal(K + 1)
    line = sp.Line(K, B, R, mode, dtype=np.float64)
    fed = [[] for _ in range(B)]            # the current utterance of every slot: rows fed, rows emitted
    got = [[] for _ in range(B)]
    done = []                               # finished utterances: (rows fed, rows emitted)

    def finish(b):
        done.append((fed[b], got[b]))
        fed[b], got[b] = [], []

    sizes = [0, 1, max(K - 1, 0), K, K + 1, max_chunk]
    for step in range(40):
        Tc = int(rng.choice(sizes[1:]))
        n = np.array([min(int(rng.choice(sizes)), Tc) for _ in range(B)])
        chunk = rng.standard_normal((Tc, B, R))
        before = (line.state.copy(), line.m.copy())
        window, wlen, emit = line.push(chunk, n)
        for b in range(B):
            if n[b] == 0:
                assert np.array_equal(line.state[:, b], before[0][:, b]) and line.m[b] == before[1][b] and emit[b] == 0
            assert np.all(window[wlen[b]:, b] == 0)
            fed[b].append(chunk[:n[b], b])
            out = _taps(window[:wlen[b], b], weights)
            assert out.shape[0] == emit[b]
            got[b].append(out)
        if step % 7 == 3:                   # a slot ends its utterance and starts a new one while the others go on
            b = step % B
            if mode == sp.LOOKAHEAD:
                flush = np.zeros(B, dtype=np.int32)
                flush[b] = 1
                others = (line.state.copy(), line.m.copy())
                window, wlen, emit = line.push(None, None, flush)
                tail = np.concatenate([window[:wlen[b], b], np.zeros((K, R))], axis=0)      # the pending rows and a zero future
                out = _taps(tail, weights)
                assert out.shape[0] == emit[b] and all(emit[o] == 0 for o in range(B) if o != b)
                got[b].append(out)
                for o in range(B):
                    if o != b:
                        assert np.array_equal(line.state[:, o], others[0][:, o]) and line.m[o] == others[1][o]
                assert line.m[b] == 0 and np.all(line.state[:, b] == 0)
            else:
                mask = np.zeros(B, dtype=np.int32)
                mask[b] = 1
                line.reset(mask)
            finish(b)
    if mode == sp.LOOKAHEAD:
        window, wlen, emit = line.push(None, None, np.ones(B, dtype=np.int32))
        for b in range(B):
            got[b].append(_taps(np.concatenate([window[:wlen[b], b], np.zeros((K, R))], axis=0), weights))
    for b in range(B):
        finish(b)
    assert len(done) > B
    for rows, outs in done:
        seq = np.concatenate(rows, axis=0)
        out = np.concatenate(outs, axis=0)
        assert out.shape == seq.shape
        np.testing.assert_allclose(out, _whole(seq, weights, mode), rtol=0, atol=1e-12)


def test_reset_in_lookahead_mode_drops_the_pending_rows():
    line = sp.Line(3, 2, 1, sp.LOOKAHEAD, dtype=np.float64)
    line.push(np.ones((2, 2, 1)))
    assert line.m.tolist() == [2, 2]
    line.reset([0, 1])
    assert line.m.tolist() == [2, 0] and np.all(line.state[:, 1] == 0) and np.all(line.state[:2, 0] == 1)
    _, wlen, emit = line.push(np.ones((2, 2, 1)))
    assert wlen.tolist() == [4, 2] and emit.tolist() == [1, 0]
