"""Time the beam search with contextual phrase biasing (asr_ctc_beam_search_bias) against its two parents on the same inputs,
alternating in one process: asr_ctc_beam_search against the biased entry without a model, and asr_ctc_beam_search_lm against the
biased entry with the model, each with an empty graph and with a graph of --phrases phrases.  Device events on the launch
stream.  B = 32, T = 1000, V = 3000 peaky logits with the order-3 model recipe of tests/ctc_beam_lm_reference.py (full_inputs);
the phrases are 2-5-token spans of the greedy transcripts (a quarter) and random phrases of 2-5 tokens; (beam_width, top_k) in
(8, 8), (16, 16), (64, 32), alpha = 0.5, beta = 1.0; --repeats rounds of --iters launches each.  One JSON line per measurement,
and the probe-chain statistics of the graph's table counted on the host: per look-up, and the longest of the 128 look-ups (two
keys for each of 64 lanes) that one wave waits for in a step.

usage: python tools/time_ctx_bias.py [--iters 10] [--warmup 2] [--repeats 3] [--phrases 1000] [--configs 8x8,16x16,64x32]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from time_ctc_beam import timed  # noqa: E402


def make_phrases(rs, transcripts, V, count):
    table = {}
    while len(table) < count // 4:
        tr = transcripts[rs.randint(len(transcripts))]
        n = int(rs.randint(2, 6))
        i = int(rs.randint(0, len(tr) - n + 1))
        table.setdefault(tuple(int(c) for c in tr[i:i + n]), float(rs.choice([0.5, 1.0, 2.0])))
    while len(table) < count:
        p = tuple(int(c) for c in rs.randint(1, V, size=rs.randint(2, 6)))
        table.setdefault(p, float(rs.choice([0.5, 1.0, 2.0])))
    return list(table), list(table.values())


def chain_stats(img, V, rs, waves=500):
    """probes per look-up of (state, token) and (0, token) for random states and tokens (mostly misses, as in the search), and
    the longest chain among the 128 look-ups of one wave-step"""
    import ctx_bias_reference as cref
    S = np.asarray(rs.randint(0, img["n_states"], size=(waves, 64)))
    C = np.asarray(rs.randint(1, V, size=(waves, 64)))
    per, longest = [], []
    for w in range(waves):
        p = [cref.probes_needed(img, int(s), int(c)) for s, c in zip(S[w], C[w])]
        p += [cref.probes_needed(img, 0, int(c)) for c in C[w]]
        per += p
        longest.append(max(p))
    return dict(mean_probes=round(float(np.mean(per)), 3), wave_longest_mean=round(float(np.mean(longest)), 2),
                wave_longest_median=float(np.median(longest)), wave_longest_p95=float(np.percentile(longest, 95)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--configs", default="8x8,16x16,64x32")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import torch
    import ctc_beam_lm_reference as lmref
    from asr import _lib, _ops, bias, lm
    dev = torch.device("cuda:0")
    B, T, V = 32, 1000, 3000
    lib = _lib.lib()
    xh, _, ng = lmref.full_inputs(B, T, V, 3)
    x = torch.from_numpy(xh).to(dev)
    model = lm.NGramLM.from_ngrams(ng, V, V, V + 1).to(dev)
    img = model.image
    rs = np.random.RandomState(22)
    tr = [lmref.greedy(xh[:, b]) for b in range(B)]
    phrases, weights = make_phrases(rs, tr, V, a.phrases)
    graphs = {"empty": bias.ContextGraph([], V).to(dev), "phrases": bias.ContextGraph(phrases, V, weights).to(dev)}
    h = graphs["phrases"].host_image()
    print(json.dumps(dict(op="graph", phrases=len(phrases), states=h["n_states"], stored=int((h["keys"][:, 0] >= 0).sum()),
                          slots=h["slots"], max_probe=h["max_probe"], **chain_stats(h, V, rs))))
    no_lm = (None, 0, None, None, 0, 0, 0)
    for cfg in a.configs.split(","):
        W, K = (int(v) for v in cfg.split("x"))
        n = lib.asr_ctc_beam_workspace_bytes(T, B, V, W, K)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
        ln = torch.empty((B, W), dtype=torch.int32, device=dev)
        sc, cc, lc, bc = (torch.empty((B, W), dtype=torch.float32, device=dev) for _ in range(4))

        def plain():
            rc = lib.asr_ctc_beam_search(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), _lib.ptr(ws), n,
                                         _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc))
            assert rc == 0, rc

        def fused():
            rc = lib.asr_ctc_beam_search_lm(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), *_ops._lm_args(img),
                                            model.bos_id, model.eos_id, 0.5, 1.0, _lib.ptr(ws), n, _lib.ptr(ids), _lib.ptr(ln),
                                            _lib.ptr(sc), _lib.ptr(cc), _lib.ptr(lc))
            assert rc == 0, rc

        def biased(graph, with_lm):
            def run():
                lm_args, bos, eos = (_ops._lm_args(img), model.bos_id, model.eos_id) if with_lm else (no_lm, -1, -1)
                rc = lib.asr_ctc_beam_search_bias(_lib.stream(), _lib.ptr(x), None, T, B, V, 0, W, K, float("-inf"), *lm_args, bos,
                                                  eos, 0.5, 1.0, _lib.ptr(ws), n, _lib.ptr(ids), _lib.ptr(ln), _lib.ptr(sc),
                                                  _lib.ptr(cc), _lib.ptr(lc), *_ops._graph_args(graph.image), _lib.ptr(bc))
                assert rc == 0, rc
            return run
        for parent, fn, with_lm in (("ctc_beam_search", plain, False), ("ctc_beam_search_lm", fused, True)):
            runs = {"parent": fn, "empty": biased(graphs["empty"], with_lm), "phrases": biased(graphs["phrases"], with_lm)}
            ms = {k: [] for k in runs}
            for _ in range(a.repeats):
                for k, f in runs.items():
                    ms[k].append(round(timed(f, a.warmup, a.iters), 4))
            p = min(ms["parent"])
            print(json.dumps(dict(op="ctc_beam_search_bias", parent=parent, beam_width=W, top_k=K, B=B, T=T, V=V,
                                  parent_ms=ms["parent"], empty_graph_ms=ms["empty"], phrases_ms=ms["phrases"],
                                  empty_extra_us_per_frame=round((min(ms["empty"]) - p) * 1e3 / T, 3),
                                  phrases_extra_us_per_frame=round((min(ms["phrases"]) - p) * 1e3 / T, 3),
                                  top1_bias_mean=float(bc[:, 0].mean().item()))))
    N, L = 512, 150
    seq = torch.from_numpy(np.random.RandomState(1).randint(1, V, size=(N, L)).astype(np.int32)).to(dev)
    g = graphs["phrases"]
    ms = [round(timed(lambda: _ops.ctx_score(g.image, V, seq, None, True), a.warmup, a.iters), 4) for _ in range(a.repeats)]
    print(json.dumps(dict(op="ctx_score", N=N, L=L, ms=ms, Mtok_per_s=round(N * L / min(ms) / 1e3, 1))))


if __name__ == "__main__":
    main()
