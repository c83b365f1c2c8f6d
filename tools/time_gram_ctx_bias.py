"""Time the Gram-CTC beam search with contextual phrase biasing (asr_gram_ctc_beam_search_bias) against its two parents on the
same inputs, alternating in one process: asr_gram_ctc_beam_search against the biased entry without a model, and
asr_gram_ctc_beam_search_lm against the biased entry with the model, each with an empty graph and with a graph of --phrases
phrases.  Device events on the launch stream.  The inputs of tools/time_gram_beam_lm.py: B = 32, T = 1000, V = 3000 (blank, 118
unigrams, 2881 bigrams), the order-3 character model around the unfused search's top-1 strings; the phrases are 2-5-character
spans of those strings (a quarter) and random phrases of 2-5 characters; (beam_width, top_k) in (8, 8), (16, 16), (64, 32),
alpha = 0.5, beta = 1.0; --repeats rounds of --iters launches each.  One JSON line per measurement, with the extra cost per
frame over the parent entry.

--parent-lib PATH: a libasr_hip.so built from the commit before this entry existed.  Its two parent entries are then timed in the
same rounds, and every line says whether this library's unbiased entries lie within that library's own run-to-run spread
(min - spread .. max + spread, spread = max - min over its rounds; and, one-sided, whether they are no slower than max + spread):
the six gram_beam_kernel instantiations without a graph are meant to be the code as it stood.

usage: python tools/time_gram_ctx_bias.py [--iters 10] [--warmup 2] [--repeats 5] [--phrases 1000] [--configs 8x8,16x16,64x32]
                                          [--parent-lib PATH]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from time_ctc_beam import timed  # noqa: E402


def make_phrases(rs, strings, U, count):
    table = {}
    while len(table) < count // 4:
        s = strings[rs.randint(len(strings))]
        n = int(rs.randint(2, 6))
        i = int(rs.randint(0, len(s) - n + 1))
        table.setdefault(tuple(int(c) for c in s[i:i + n]), float(rs.choice([0.5, 1.0, 2.0])))
    while len(table) < count:
        p = tuple(int(c) for c in rs.randint(1, U + 1, size=rs.randint(2, 6)))
        table.setdefault(p, float(rs.choice([0.5, 1.0, 2.0])))
    return list(table), list(table.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--configs", default="8x8,16x16,64x32")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import ctc_beam_lm_reference as lmref
    import gram_beam_reference as gref
    from asr import _lib, _ops, bias, error, lm
    dev = torch.device("cuda:0")
    B, T, V, U = 32, 1000, 3000, 118
    table = gref.uni_bigram_table(U, V - 1 - U, 1)
    error.check_gram_table(table, V, 0)
    rs = np.random.RandomState(20261017)
    x = torch.from_numpy(np.stack([gref.peaky_gram(rs, T, table) for _ in range(B)], axis=1)).to(dev)
    gram = torch.from_numpy(table).to(dev)
    lib = _lib.lib()
    old = None
    if a.parent_lib:
        old = ctypes.CDLL(a.parent_lib)
        for name in ("asr_gram_ctc_beam_search", "asr_gram_ctc_beam_search_lm"):
            getattr(old, name).restype, getattr(old, name).argtypes = _lib.SIGNATURES[name]
        assert not hasattr(old, "asr_gram_ctc_beam_search_bias"), "--parent-lib already has the biased entry"
    ids0, len0, _ = error.gram_beam_decode(x, gram, 16, 16)
    ids0, len0 = ids0[:, 0].cpu().numpy(), len0[:, 0].cpu().numpy()
    top1 = [ids0[b, :len0[b]].tolist() for b in range(B)]
    ng = lmref.random_model(np.random.RandomState(20261018), U + 1, 3, top1)
    move = {U + 1: V, U + 2: V + 1}                   # <s> / </s> above every token id; the values do not change
    ng = {tuple(move.get(c, c) for c in k): v for k, v in ng.items()}
    model = lm.NGramLM.from_ngrams(ng, V, V, V + 1).to(dev)
    img = model.image
    phrases, weights = make_phrases(np.random.RandomState(22), top1, U, a.phrases)
    graphs = {"empty": bias.ContextGraph([], V).to(dev), "phrases": bias.ContextGraph(phrases, V, weights).to(dev)}
    h = graphs["phrases"].host_image()
    print(json.dumps(dict(op="graph", phrases=len(phrases), states=h["n_states"], stored=int((h["keys"][:, 0] >= 0).sum()),
                          slots=h["slots"], max_probe=h["max_probe"])))
    no_lm = (None, 0, None, None, 0, 0, 0)
    for cfg in a.configs.split(","):
        W, K = (int(v) for v in cfg.split("x"))
        n = lib.asr_gram_ctc_beam_bias_workspace_bytes(T, B, V, W, K)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        ids = torch.empty((B, W, 2 * T), dtype=torch.int32, device=dev)
        ln = torch.empty((B, W), dtype=torch.int32, device=dev)
        sc, cc, lc, bc = (torch.empty((B, W), dtype=torch.float32, device=dev) for _ in range(4))

        def plain(which):
            def run():
                rc = which.asr_gram_ctc_beam_search(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), _lib.ptr(gram),
                                                    _lib.ptr(ws), n, _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc))
                assert rc == 0, rc
            return run

        def fused(which):
            def run():
                rc = which.asr_gram_ctc_beam_search_lm(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"),
                                                       _lib.ptr(gram), *_ops._lm_args(img), model.bos_id, model.eos_id, 0.5, 1.0,
                                                       _lib.ptr(ws), n, _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(cc),
                                                       _lib.ptr(lc))
                assert rc == 0, rc
            return run

        def biased(graph, with_lm):
            def run():
                lm_args, bos, eos = (_ops._lm_args(img), model.bos_id, model.eos_id) if with_lm else (no_lm, -1, -1)
                rc = lib.asr_gram_ctc_beam_search_bias(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"),
                                                       _lib.ptr(gram), *lm_args, bos, eos, 0.5, 1.0, _lib.ptr(ws), n, _lib.ptr(ids),
                                                       _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(cc), _lib.ptr(lc),
                                                       *_ops._graph_args(graph.image), _lib.ptr(bc))
                assert rc == 0, rc
            return run
        for parent, fn, with_lm in (("gram_ctc_beam_search", plain, False), ("gram_ctc_beam_search_lm", fused, True)):
            runs = {}
            if old is not None:
                runs["parent_lib"] = fn(old)
            runs.update({"parent": fn(lib), "empty": biased(graphs["empty"], with_lm), "phrases": biased(graphs["phrases"], with_lm)})
            ms = {k: [] for k in runs}
            for _ in range(a.repeats):
                for k, f in runs.items():
                    ms[k].append(round(timed(f, a.warmup, a.iters), 4))
            p = min(ms["parent"])
            line = dict(op="gram_ctc_beam_search_bias", parent=parent, beam_width=W, top_k=K, B=B, T=T, V=V, unigrams=U,
                        parent_ms=ms["parent"], empty_graph_ms=ms["empty"], phrases_ms=ms["phrases"],
                        empty_extra_us_per_frame=round((min(ms["empty"]) - p) * 1e3 / T, 3),
                        phrases_extra_us_per_frame=round((min(ms["phrases"]) - p) * 1e3 / T, 3),
                        top1_bias_mean=float(bc[:, 0].mean().item()))
            if old is not None:
                lo, hi = min(ms["parent_lib"]), max(ms["parent_lib"])
                line.update(parent_lib_ms=ms["parent_lib"], parent_lib_spread_ms=round(hi - lo, 4),
                            unbiased_no_slower_than_parent_spread=bool(max(ms["parent"]) <= hi + (hi - lo)),
                            unbiased_within_parent_spread=bool(lo - (hi - lo) <= min(ms["parent"]) and max(ms["parent"]) <= hi + (hi - lo)))
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
