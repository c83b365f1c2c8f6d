"""Time the streaming Gram-CTC beam search (asr_gram_ctc_beam_stream_reset / _advance / _result) against the one-shot entry on the
same frames, alternating in one process: asr_gram_ctc_beam_search and asr_gram_ctc_beam_search_lm on the inputs of
tools/time_gram_beam.py and tools/time_gram_beam_lm.py (B = 32, T = 1000, V = 3000: blank, 118 unigrams, 2881 bigrams; the
order-3 character model around the unfused top-1 strings), (beam_width, top_k) = (16, 16), and the stream fed the same frames in
chunks of --chunks frames (reset, T / chunk advances, one result).  State, workspace and outputs are allocated once; device
events on the launch stream; --repeats rounds of --iters runs each.  The figure of interest is the extra time per advance call
over the one-shot decode, (t_stream - t_oneshot) / number of chunks, from the best round of each.  The host's time to enqueue one
run is printed beside it.  Every stream run's outputs are compared with the one-shot entry's, byte for byte, before anything is
timed.  One JSON line per measurement.

usage: python tools/time_gram_beam_stream.py [--iters 5] [--warmup 1] [--repeats 3] [--chunks 1000,100,20,4] [--config 16x16]
For the split between the passes run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from time_ctc_beam import timed  # noqa: E402
from time_ctc_beam_stream import enqueue_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunks", default="1000,100,20,4")
    ap.add_argument("--config", default="16x16")
    ap.add_argument("--order", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import ctc_beam_lm_reference as lmref
    import gram_beam_reference as gref
    from asr import _lib, _ops, error, lm
    dev = torch.device("cuda:0")
    B, T, V, U = 32, 1000, 3000, 118
    W, K = (int(v) for v in a.config.split("x"))
    chunks = [int(c) for c in a.chunks.split(",")]
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream
    table = gref.uni_bigram_table(U, V - 1 - U, 1)
    error.check_gram_table(table, V, 0)
    rs = np.random.RandomState(20261017)
    x = torch.from_numpy(np.stack([gref.peaky_gram(rs, T, table) for _ in range(B)], axis=1)).to(dev)
    gram = torch.from_numpy(table).to(dev)
    ids0, len0, _ = error.gram_beam_decode(x, gram, 16, 16)
    ids0, len0 = ids0[:, 0].cpu().numpy(), len0[:, 0].cpu().numpy()
    ng = lmref.random_model(np.random.RandomState(20261018), U + 1, a.order, [ids0[b, :len0[b]].tolist() for b in range(B)])
    move = {U + 1: V, U + 2: V + 1}                       # <s> / </s> above every token id; the values do not change
    model = lm.NGramLM.from_ngrams({tuple(move.get(c, c) for c in k): v for k, v in ng.items()}, V, V, V + 1).to(dev)
    no_lm = (None, 0, None, None, 0, 0, 0)
    n1 = lib.asr_gram_ctc_beam_workspace_bytes(T, B, V, W, K)
    ws1 = torch.empty(n1, dtype=torch.uint8, device=dev)
    nws = lib.asr_gram_ctc_beam_stream_workspace_bytes(max(chunks), B, V, W, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)

    def outputs():
        return dict(ids=torch.empty((B, W, 2 * T), dtype=torch.int32, device=dev), ln=torch.empty((B, W), dtype=torch.int32, device=dev),
                    sc=torch.empty((B, W), dtype=torch.float32, device=dev), cc=torch.empty((B, W), dtype=torch.float32, device=dev),
                    lc=torch.empty((B, W), dtype=torch.float32, device=dev))
    fr = torch.empty((B,), dtype=torch.int32, device=dev)
    for name, with_lm in (("gram_ctc_beam_search", False), ("gram_ctc_beam_search_lm", True)):
        lm_args = _ops._lm_args(model.image) if with_lm else no_lm
        bos, eos = (model.bos_id, model.eos_id) if with_lm else (-1, -1)
        nst = lib.asr_gram_ctc_beam_stream_state_bytes(B, W, T, int(with_lm))
        state = torch.zeros(nst, dtype=torch.uint8, device=dev)
        o1, o2 = outputs(), outputs()

        def oneshot():
            if with_lm:
                rc = lib.asr_gram_ctc_beam_search_lm(st(), p(x), None, T, B, V, 0, W, K, float("-inf"), p(gram), *lm_args, bos, eos,
                                                     0.5, 1.0, p(ws1), n1, p(o1["ids"]), p(o1["ln"]), p(o1["sc"]), p(o1["cc"]),
                                                     p(o1["lc"]))
            else:
                rc = lib.asr_gram_ctc_beam_search(st(), p(x), None, T, B, V, 0, W, K, float("-inf"), p(gram), p(ws1), n1, p(o1["ids"]),
                                                  p(o1["ln"]), p(o1["sc"]))
            assert rc == 0, rc

        def streamed(c):
            parts = [(t, x[t:t + c]) for t in range(0, T, c)]

            def run():
                rc = lib.asr_gram_ctc_beam_stream_reset(st(), p(state), nst, B, W, T, int(with_lm), None)
                assert rc == 0, rc
                for t, xc in parts:
                    rc = lib.asr_gram_ctc_beam_stream_advance(st(), p(xc), None, xc.shape[0], B, V, 0, W, K, float("-inf"), p(gram),
                                                              *lm_args, bos, 0.5, 1.0, t, T, p(state), nst, p(ws), nws)
                    assert rc == 0, rc
                rc = lib.asr_gram_ctc_beam_stream_result(st(), *lm_args, bos, eos, 0.5, 1.0, B, W, T, 0, 2 * T, p(state), nst,
                                                         p(o2["ids"]), p(o2["ln"]), p(o2["sc"]), p(o2["cc"]) if with_lm else None,
                                                         p(o2["lc"]) if with_lm else None, p(fr))
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
                              spread_ms=round(max(ms["oneshot"]) - base, 4), host_enqueue_ms=host["oneshot"],
                              top1_chars_mean=float(o1["ln"][:, 0].float().mean().item()))))
        for c in chunks:
            n = (T + c - 1) // c
            print(json.dumps(dict(op="stream", entry=name, chunk=c, advances=n, ms=ms[c], spread_ms=round(max(ms[c]) - min(ms[c]), 4),
                                  host_enqueue_ms=host[c], extra_us_per_advance=round((min(ms[c]) - base) * 1e3 / n, 3),
                                  state_bytes=nst, beam_bytes_per_utterance=(nst - 2 * B * T * W * 8) // B)))


if __name__ == "__main__":
    main()
