"""Time the streaming beam search (asr_ctc_beam_stream_reset / _advance / _result) against the one-shot entry on the same frames,
alternating in one process: asr_ctc_beam_search and asr_ctc_beam_search_lm (section 17's order-3 model) on B = 32, T = 1000,
V = 3000 peaky logits (tests/ctc_beam_lm_reference.py full_inputs), (beam_width, top_k) = (16, 16), and the stream fed the same
frames in chunks of --chunks frames (reset, T / chunk advances, one result).  State, workspace and outputs are allocated once;
device events on the launch stream; --repeats rounds of --iters runs each.  The figure of interest is the extra time per advance
call over the one-shot decode, (t_stream - t_oneshot) / number of chunks, from the best round of each.  The host's time to
enqueue one run is printed beside it: where it exceeds the device time the stream is bound by the launches, not by the kernels.
Every stream run's outputs are compared with the one-shot entry's, byte for byte, before anything is timed.  One JSON line per
measurement.

usage: python tools/time_ctc_beam_stream.py [--iters 5] [--warmup 1] [--repeats 3] [--chunks 1000,100,20,4] [--config 16x16]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from time_ctc_beam import timed  # noqa: E402


def enqueue_ms(fn, iters):
    """host time to enqueue one run (the device is idle at the start and is not waited for)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunks", default="1000,100,20,4")
    ap.add_argument("--config", default="16x16")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import ctc_beam_lm_reference as lmref
    from asr import _lib, _ops, lm
    dev = torch.device("cuda:0")
    B, T, V = 32, 1000, 3000
    W, K = (int(v) for v in a.config.split("x"))
    chunks = [int(c) for c in a.chunks.split(",")]
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream
    xh, _, ng = lmref.full_inputs(B, T, V, 3)
    x = torch.from_numpy(xh).to(dev)
    model = lm.NGramLM.from_ngrams(ng, V, V, V + 1).to(dev)
    no_lm, no_graph = (None, 0, None, None, 0, 0, 0), (None, None, 0, 0, None, 0)
    n1 = lib.asr_ctc_beam_workspace_bytes(T, B, V, W, K)
    ws1 = torch.empty(n1, dtype=torch.uint8, device=dev)
    nws = lib.asr_ctc_beam_stream_workspace_bytes(max(chunks), B, V, W, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)

    def outputs():
        return dict(ids=torch.empty((B, W, T), dtype=torch.int32, device=dev), ln=torch.empty((B, W), dtype=torch.int32, device=dev),
                    sc=torch.empty((B, W), dtype=torch.float32, device=dev), cc=torch.empty((B, W), dtype=torch.float32, device=dev),
                    lc=torch.empty((B, W), dtype=torch.float32, device=dev))
    fr = torch.empty((B,), dtype=torch.int32, device=dev)
    for name, with_lm in (("ctc_beam_search", False), ("ctc_beam_search_lm", True)):
        lm_args = _ops._lm_args(model.image) if with_lm else no_lm
        bos, eos = (model.bos_id, model.eos_id) if with_lm else (-1, -1)
        nst = lib.asr_ctc_beam_stream_state_bytes(B, W, T, int(with_lm), 0)
        state = torch.zeros(nst, dtype=torch.uint8, device=dev)
        o1, o2 = outputs(), outputs()

        def oneshot():
            if with_lm:
                rc = lib.asr_ctc_beam_search_lm(st(), p(x), None, T, B, V, 0, W, K, float("-inf"), *lm_args, bos, eos, 0.5, 1.0, p(ws1),
                                                n1, p(o1["ids"]), p(o1["ln"]), p(o1["sc"]), p(o1["cc"]), p(o1["lc"]))
            else:
                rc = lib.asr_ctc_beam_search(st(), p(x), None, T, B, V, 0, W, K, float("-inf"), p(ws1), n1, p(o1["ids"]), p(o1["ln"]),
                                             p(o1["sc"]))
            assert rc == 0, rc

        def streamed(c):
            parts = [(t, x[t:t + c]) for t in range(0, T, c)]

            def run():
                rc = lib.asr_ctc_beam_stream_reset(st(), p(state), nst, B, W, T, int(with_lm), 0, bos, None)
                assert rc == 0, rc
                for t, xc in parts:
                    rc = lib.asr_ctc_beam_stream_advance(st(), p(xc), None, xc.shape[0], B, V, 0, W, K, float("-inf"), *lm_args,
                                                         *no_graph, 0.5, 1.0, t, T, p(state), nst, p(ws), nws)
                    assert rc == 0, rc
                rc = lib.asr_ctc_beam_stream_result(st(), *lm_args, *no_graph, 0.5, 1.0, eos, B, W, T, 0, T, p(state), nst, p(o2["ids"]),
                                                    p(o2["ln"]), p(o2["sc"]), p(o2["cc"]) if with_lm else None,
                                                    p(o2["lc"]) if with_lm else None, None, p(fr))
                assert rc == 0, rc
            return run
        runs = {"oneshot": oneshot}
        runs.update({c: streamed(c) for c in chunks})
        oneshot()
        for c in chunks:
            for v in o2.values():
                v.fill_(-3)
            runs[c]()
            torch.cuda.synchronize()
            for k in ("ids", "ln", "sc") + (("cc", "lc") if with_lm else ()):
                assert o1[k].cpu().numpy().tobytes() == o2[k].cpu().numpy().tobytes(), (name, c, k)
            assert fr.cpu().tolist() == [T] * B
        ms = {k: [] for k in runs}
        for _ in range(a.repeats):
            for k, f in runs.items():
                ms[k].append(round(timed(f, a.warmup, a.iters), 4))
        host = {k: round(enqueue_ms(f, a.iters), 4) for k, f in runs.items()}
        base = min(ms["oneshot"])
        print(json.dumps(dict(op="oneshot", entry=name, beam_width=W, top_k=K, B=B, T=T, V=V, ms=ms["oneshot"],
                              spread_ms=round(max(ms["oneshot"]) - base, 4), host_enqueue_ms=host["oneshot"])))
        for c in chunks:
            n = (T + c - 1) // c
            print(json.dumps(dict(op="stream", entry=name, chunk=c, advances=n, ms=ms[c], spread_ms=round(max(ms[c]) - min(ms[c]), 4),
                                  host_enqueue_ms=host[c], extra_us_per_advance=round((min(ms[c]) - base) * 1e3 / n, 3),
                                  state_bytes=nst, beam_bytes_per_utterance=(nst - B * T * W * 8) // B)))


if __name__ == "__main__":
    main()
