"""Time the beam search fused with an n-gram language model (asr_ctc_beam_search_lm) against the unfused asr_ctc_beam_search on
the same inputs, alternating in one process, and asr_ngram_score: device events on the launch stream.  B = 32, T = 1000,
V = 3000 peaky logits with the model recipe of tests/ctc_beam_lm_reference.py (full_inputs), orders 3 and 4, (beam_width, top_k)
in (8, 8), (16, 16), (64, 32), alpha = 0.5, beta = 1.0; --repeats rounds of --iters launches each.  One JSON line per measurement.

usage: python tools/time_ctc_beam_lm.py [--iters 10] [--warmup 2] [--repeats 3] [--orders 3,4] [--configs 8x8,16x16,64x32]
For the split between the passes run it under rocprofv3 --kernel-trace --stats (cand_kernel, beam_kernel<false>, beam_kernel<true>,
ngram_score_kernel)."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from time_ctc_beam import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--orders", default="3,4")
    ap.add_argument("--configs", default="8x8,16x16,64x32")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import ctc_beam_lm_reference as lmref
    from asr import _lib, _ops, lm
    dev = torch.device("cuda:0")
    B, T, V = 32, 1000, 3000
    lib = _lib.lib()
    for order in (int(o) for o in a.orders.split(",")):
        xh, _, ng = lmref.full_inputs(B, T, V, order)
        x = torch.from_numpy(xh).to(dev)
        model = lm.NGramLM.from_ngrams(ng, V, V, V + 1).to(dev)
        img = model.image
        print(json.dumps(dict(op="model", order=order, ngrams=len(ng), slots=img["slots"], max_probe=img["max_probe"])))
        for cfg in a.configs.split(","):
            W, K = (int(v) for v in cfg.split("x"))
            n = lib.asr_ctc_beam_workspace_bytes(T, B, V, W, K)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
            ln = torch.empty((B, W), dtype=torch.int32, device=dev)
            sc, cc, lc = (torch.empty((B, W), dtype=torch.float32, device=dev) for _ in range(3))

            def plain():
                rc = lib.asr_ctc_beam_search(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), _lib.ptr(ws), n,
                                             _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc))
                assert rc == 0, rc

            def fused():
                rc = lib.asr_ctc_beam_search_lm(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), *_ops._lm_args(img),
                                                model.bos_id, model.eos_id, 0.5, 1.0, _lib.ptr(ws), n, _lib.ptr(ids), _lib.ptr(ln),
                                                _lib.ptr(sc), _lib.ptr(cc), _lib.ptr(lc))
                assert rc == 0, rc
            ms = {"plain": [], "fused": []}
            for _ in range(a.repeats):
                ms["plain"].append(round(timed(plain, a.warmup, a.iters), 4))
                ms["fused"].append(round(timed(fused, a.warmup, a.iters), 4))
            p, f = min(ms["plain"]), min(ms["fused"])
            print(json.dumps(dict(op="ctc_beam_search_lm", order=order, beam_width=W, top_k=K, B=B, T=T, V=V, plain_ms=ms["plain"],
                                  fused_ms=ms["fused"], extra_us_per_frame=round((f - p) * 1e3 / T, 3),
                                  top1_len_mean=float(ln[:, 0].float().mean().item()))))
        N, L = 512, 150
        seq = torch.from_numpy(np.random.RandomState(1).randint(1, V, size=(N, L)).astype(np.int32)).to(dev)
        ms = [round(timed(lambda: _ops.ngram_score(img, seq, None, model.bos_id, model.eos_id), a.warmup, a.iters), 4)
              for _ in range(a.repeats)]
        print(json.dumps(dict(op="ngram_score", order=order, N=N, L=L, ms=ms, Mtok_per_s=round(N * L / min(ms) / 1e3, 1))))


if __name__ == "__main__":
    main()
