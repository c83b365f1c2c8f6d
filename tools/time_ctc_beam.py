"""Time the CTC prefix beam search (asr_ctc_beam_search) and, for context, the greedy decode (asr_argmax_rows + asr_ctc_collapse)
with device events on the launch stream: B = 32, T = 1000, V = 3000 peaky logits (tests/ctc_beam_reference.py), (beam_width,
top_k) in (8, 8), (16, 16), (64, 32); warm-up, then --iters timed launches.  One JSON line per measurement.

usage: python tools/time_ctc_beam.py [--what beam,greedy] [--iters 20] [--warmup 3] [--root DIR] [--configs 8x8,16x16,64x32]
  --root DIR  import the asr package of another checkout (e.g. the parent commit's, built in place), whose library may not
              have the beam entries: time --what greedy there.
For the split between the two passes run it under rocprofv3 --kernel-trace --stats (cand_kernel, beam_kernel)."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def logits(B, T, V, seed=20261016):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import ctc_beam_reference as ref
    rs = np.random.RandomState(seed)
    return np.stack([ref.peaky(rs, T, V) for _ in range(B)], axis=1)


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="beam,greedy")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--configs", default="8x8,16x16,64x32")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "chainer-speech-recognition_amd"))
    import torch
    from asr import _lib, _ops
    dev = torch.device("cuda:0")
    B, T, V = 32, 1000, 3000
    x = torch.from_numpy(logits(B, T, V)).to(dev)
    bytes_read = T * B * V * 4
    what = a.what.split(",")
    if "greedy" in what:
        ms = timed(lambda: _ops.argmax_rows(x), a.warmup, a.iters)
        print(json.dumps(dict(op="argmax_rows", root=a.root, B=B, T=T, V=V, ms=round(ms, 4), GBps=round(bytes_read / ms / 1e6, 1))))
        ms = timed(lambda: _ops.ctc_collapse(_ops.argmax_rows(x), None, 0, True), a.warmup, a.iters)
        print(json.dumps(dict(op="greedy_decode", root=a.root, B=B, T=T, V=V, ms=round(ms, 4))))
    if "beam" in what:
        lib = _lib.lib()
        for cfg in a.configs.split(","):
            W, K = (int(v) for v in cfg.split("x"))
            n = lib.asr_ctc_beam_workspace_bytes(T, B, V, W, K)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
            ln = torch.empty((B, W), dtype=torch.int32, device=dev)
            sc = torch.empty((B, W), dtype=torch.float32, device=dev)

            def run():
                rc = lib.asr_ctc_beam_search(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), _lib.ptr(ws), n,
                                             _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc))
                assert rc == 0, rc
            ms = timed(run, a.warmup, a.iters)
            print(json.dumps(dict(op="ctc_beam_search", beam_width=W, top_k=K, B=B, T=T, V=V, ms=round(ms, 4),
                                  top1_len_mean=float(ln[:, 0].float().mean().item()), top1_score_mean=float(sc[:, 0].mean().item()))))


if __name__ == "__main__":
    main()
