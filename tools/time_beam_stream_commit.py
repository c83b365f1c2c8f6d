"""Time the commit of a streaming beam search (asr_ctc_beam_stream_commit, csrc/ctc_beam.hip: commit_kernel) on section 15's inputs:
B = 32, T = 1000, V = 3000 peaky logits (tests/ctc_beam_lm_reference.py full_inputs), (beam_width, top_k) = (16, 16), no model,
chunks of --chunk frames, everything through the C ABI with state, workspace and outputs allocated once and device events on the
launch stream, alternating in one process:

  advance        reset, T / chunk advances, one result: the "chunk 20" line of profiles/ctc_beam_stream.txt again
  commit_best    the same with, after every chunk, what asr.error.BeamStream.commit_best(hold) does on the device: a result, the
                 best hypothesis' length minus `hold` (one elementwise launch), a commit of that prefix read in place from the
                 result's ids.  Nothing waits for the host; the table keeps max_frames = T rows so that no host count is needed.
  class          asr.error.BeamStream with max_frames = --small and commit_best(hold) after every chunk, which reads the
                 committed tokens back after every commit (the method synchronises)
  commit alone   one commit on a saved state, as a peek (compact = 0: chain walk and comparison) and in full (the state is
                 restored before every run; the restore alone is timed and subtracted), for the state after T frames without
                 any commit (tails of ~170 tokens, the worst case of the chain walk) and for a steady state under commit_best
                 (tails of at most ~20 tokens)

One JSON line per measurement.
usage: python tools/time_beam_stream_commit.py [--iters 5] [--warmup 1] [--repeats 3] [--chunk 20] [--hold 8] [--small 96]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from time_ctc_beam import timed  # noqa: E402
from time_ctc_beam_stream import enqueue_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--hold", type=int, default=8)
    ap.add_argument("--small", type=int, default=96)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import ctc_beam_lm_reference as lmref
    from asr import _lib, error
    dev = torch.device("cuda:0")
    B, T, V, W, K, C = 32, 1000, 3000, 16, 16, a.chunk
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream
    xh, _, _ = lmref.full_inputs(B, T, V, 3)
    x = torch.from_numpy(xh).to(dev)
    parts = [(t, x[t:t + C]) for t in range(0, T, C)]
    no_lm, no_graph = (None, 0, None, None, 0, 0, 0), (None, None, 0, 0, None, 0)
    nws = lib.asr_ctc_beam_stream_workspace_bytes(C, B, V, W, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    nst = lib.asr_ctc_beam_stream_state_bytes(B, W, T, 0, 0)
    state = torch.zeros(nst, dtype=torch.uint8, device=dev)
    ncw = lib.asr_beam_stream_commit_workspace_bytes(B, W, T, 1)
    cws = torch.empty(ncw, dtype=torch.uint8, device=dev)
    ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
    ln = torch.empty((B, W), dtype=torch.int32, device=dev)
    sc = torch.empty((B, W), dtype=torch.float32, device=dev)
    fr = torch.empty((B,), dtype=torch.int32, device=dev)
    plen = torch.empty((B,), dtype=torch.int32, device=dev)
    out = torch.zeros((B, T), dtype=torch.int32, device=dev)
    o_n, o_c, o_r, o_s = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(4))

    def reset():
        assert lib.asr_ctc_beam_stream_reset(st(), p(state), nst, B, W, T, 0, 0, -1, None) == 0

    def advance(t, xc):
        rc = lib.asr_ctc_beam_stream_advance(st(), p(xc), None, xc.shape[0], B, V, 0, W, K, float("-inf"), *no_lm, *no_graph, 0.0, 0.0,
                                             t, T, p(state), nst, p(ws), nws)
        assert rc == 0, rc

    def result(Lcap):
        rc = lib.asr_ctc_beam_stream_result(st(), *no_lm, *no_graph, 0.0, 0.0, -1, B, W, T, 0, Lcap, p(state), nst, p(ids), p(ln), p(sc),
                                            None, None, None, p(fr))
        assert rc == 0, rc

    def commit(Lcap, compact=1):
        """the prefix is row 0 of every utterance's ids, read where result wrote it"""
        rc = lib.asr_ctc_beam_stream_commit(st(), p(state), nst, B, W, T, 0, 0, p(ids), W * Lcap, p(plen), compact, T, p(cws), ncw,
                                            p(out), T, p(o_n), p(o_c), p(o_r), p(o_s))
        assert rc == 0, rc

    def best_minus_hold():
        torch.clamp(ln[:, 0] - a.hold, min=0, out=plen)

    def run_advance():
        reset()
        for t, xc in parts:
            advance(t, xc)
        result(T)

    def run_commit_best():
        reset()
        for t, xc in parts:
            advance(t, xc)
            result(T)
            best_minus_hold()
            commit(T)
        result(T)

    stream = error.BeamStream(B, V, a.small, W, K, device=dev)

    def run_class():
        stream.reset()
        for _, xc in parts:
            stream.advance(xc)
            stream.commit_best(a.hold)
        stream.result()

    run_commit_best()
    torch.cuda.synchronize()
    assert o_s.cpu().tolist() == [1] * B
    steady_tail = int(ln.max().item())
    runs = {"advance": run_advance, "commit_best": run_commit_best, "class": run_class}
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, f in runs.items():
            ms[k].append(round(timed(f, a.warmup, a.iters), 4))
    host = {k: round(enqueue_ms(f, a.iters), 4) for k, f in runs.items()}
    n = len(parts)
    base = min(ms["advance"])
    for k in runs:
        print(json.dumps(dict(op=k, chunk=C, advances=n, hold=a.hold, ms=ms[k], spread_ms=round(max(ms[k]) - min(ms[k]), 4),
                              host_enqueue_ms=host[k], extra_us_per_chunk=round((min(ms[k]) - base) * 1e3 / n, 3),
                              max_frames=a.small if k == "class" else T)))
    # one commit alone, on two saved states
    saved = {}
    run_advance()
    best_minus_hold()
    torch.cuda.synchronize()
    saved["after %d frames, no commit before" % T] = (state.clone(), plen.clone(), int(ln.max().item()))
    reset()
    for t, xc in parts[:len(parts) // 2]:
        advance(t, xc)
        result(T)
        best_minus_hold()
        commit(T)
    advance(*parts[len(parts) // 2])
    result(T)
    best_minus_hold()
    torch.cuda.synchronize()
    saved["steady state under commit_best"] = (state.clone(), plen.clone(), int(ln.max().item()))
    for name, (snap, lens, longest) in saved.items():
        state.copy_(snap)
        plen.copy_(lens)
        result(T)                                               # the prefix rows that commit reads

        def restore():
            state.copy_(snap)

        def full():
            state.copy_(snap)
            commit(T)

        def peek():
            commit(T, 0)
        t_restore = min(timed(restore, a.warmup, 20) for _ in range(a.repeats))
        t_full = min(timed(full, a.warmup, 20) for _ in range(a.repeats))
        state.copy_(snap)
        t_peek = min(timed(peek, a.warmup, 20) for _ in range(a.repeats))
        print(json.dumps(dict(op="commit alone", state=name, longest_tail=longest, mean_prefix=round(float(lens.float().mean()), 1),
                              peek_us=round(t_peek * 1e3, 2), restore_us=round(t_restore * 1e3, 2),
                              restore_and_commit_us=round(t_full * 1e3, 2), commit_us=round((t_full - t_restore) * 1e3, 2))))
    print(json.dumps(dict(op="note", steady_longest_tail_after_last_commit=steady_tail)))


if __name__ == "__main__":
    main()
