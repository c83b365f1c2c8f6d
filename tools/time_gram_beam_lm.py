"""Time the Gram-CTC beam search fused with a character n-gram language model (asr_gram_ctc_beam_search_lm) against the unfused
string search asr_gram_ctc_beam_search on the same logits, alternating in one process: device events on the launch stream.  The
logits and the table of tools/time_gram_beam.py: B = 32, T = 1000, V = 3000 (blank, 118 unigrams, 2881 bigrams).  The model is
over the 118 unigram ids, built with the recipe of tests/ctc_beam_lm_reference.py (random_model, as full_inputs does) around the
unfused search's top-1 strings at (16, 16), orders 3 and 4, <s> / </s> = V / V + 1; (beam_width, top_k) in (8, 8), (16, 16),
(64, 32), alpha = 0.5, beta = 1.0; --repeats rounds of --iters launches each.  One JSON line per setting: the times of every
round, the ratio of the best ones and the extra cost per frame.

usage: python tools/time_gram_beam_lm.py [--iters 10] [--warmup 2] [--repeats 3] [--orders 3,4] [--configs 8x8,16x16,64x32]
For the split between the passes run it under rocprofv3 --kernel-trace --stats (cand_kernel, gram_rows_kernel,
gram_beam_kernel<false>, gram_beam_kernel<true>)."""
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
    import gram_beam_reference as gref
    from asr import _lib, _ops, error, lm
    dev = torch.device("cuda:0")
    B, T, V, U = 32, 1000, 3000, 118
    table = gref.uni_bigram_table(U, V - 1 - U, 1)
    error.check_gram_table(table, V, 0)
    rs = np.random.RandomState(20261017)
    x = torch.from_numpy(np.stack([gref.peaky_gram(rs, T, table) for _ in range(B)], axis=1)).to(dev)
    gram = torch.from_numpy(table).to(dev)
    lib = _lib.lib()
    ids0, len0, _ = error.gram_beam_decode(x, gram, 16, 16)
    ids0, len0 = ids0[:, 0].cpu().numpy(), len0[:, 0].cpu().numpy()
    top1 = [ids0[b, :len0[b]].tolist() for b in range(B)]
    for order in (int(o) for o in a.orders.split(",")):
        ng = lmref.random_model(np.random.RandomState(20261018), U + 1, order, top1)
        move = {U + 1: V, U + 2: V + 1}                   # <s> / </s> above every token id; the values do not change
        ng = {tuple(move.get(c, c) for c in k): v for k, v in ng.items()}
        model = lm.NGramLM.from_ngrams(ng, V, V, V + 1).to(dev)
        img = model.image
        print(json.dumps(dict(op="model", order=order, ngrams=len(ng), slots=img["slots"], max_probe=img["max_probe"])))
        for cfg in a.configs.split(","):
            W, K = (int(v) for v in cfg.split("x"))
            n = lib.asr_gram_ctc_beam_lm_workspace_bytes(T, B, V, W, K)
            assert n >= lib.asr_gram_ctc_beam_workspace_bytes(T, B, V, W, K)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            ids, fids = (torch.empty((B, W, 2 * T), dtype=torch.int32, device=dev) for _ in range(2))
            ln, fln = (torch.empty((B, W), dtype=torch.int32, device=dev) for _ in range(2))
            sc, fsc, cc, lc = (torch.empty((B, W), dtype=torch.float32, device=dev) for _ in range(4))

            def plain():
                rc = lib.asr_gram_ctc_beam_search(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), _lib.ptr(gram),
                                                  _lib.ptr(ws), n, _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc))
                assert rc == 0, rc

            def fused():
                rc = lib.asr_gram_ctc_beam_search_lm(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"),
                                                     _lib.ptr(gram), *_ops._lm_args(img), model.bos_id, model.eos_id, 0.5, 1.0,
                                                     _lib.ptr(ws), n, _lib.ptr(fids), _lib.ptr(fln), _lib.ptr(fsc), _lib.ptr(cc),
                                                     _lib.ptr(lc))
                assert rc == 0, rc
            ms = {"plain": [], "fused": []}
            for _ in range(a.repeats):
                ms["plain"].append(round(timed(plain, a.warmup, a.iters), 4))
                ms["fused"].append(round(timed(fused, a.warmup, a.iters), 4))
            p, f = min(ms["plain"]), min(ms["fused"])
            changed = int(((ln[:, 0] != fln[:, 0]) | (ids[:, 0] != fids[:, 0]).any(dim=1)).sum().item())
            print(json.dumps(dict(op="gram_ctc_beam_search_lm", order=order, beam_width=W, top_k=K, B=B, T=T, V=V, unigrams=U,
                                  plain_ms=ms["plain"], fused_ms=ms["fused"], ratio=round(f / p, 3),
                                  extra_us_per_frame=round((f - p) * 1e3 / T, 3),
                                  top1_chars_mean=float(fln[:, 0].float().mean().item()), top1_changed=changed)))


if __name__ == "__main__":
    main()
