"""Time the CTC keyword search (asr_kws_detect + asr_kws_hits) against two things the parent commit already has, on the same logits,
in the same process, alternating: the forced alignment (asr_ctc_align: its gather pass is the yardstick for the logits pass -- the
same rows read once) and the beam search at beam 16 (asr.error.beam_decode: what a user runs today to look for a phrase).
B = 32, T = 1000, V = 3000 f32 randn logits, K = 64 phrases of 2 to 16 tokens, x_len ~ U{600..1000}; device events on the launch
stream after warm-up; --rounds rounds of (align, detect, hits, detect + hits, beam), so every figure comes with its spread.
One JSON line per measurement and a summary line (min / median / max over the rounds).

usage: python tools/time_keyword_search.py [--iters 20] [--warmup 3] [--rounds 5] [--K 64] [--full-length]
For the kernel split run it under rocprofv3 --kernel-trace --stats (ctc_kws::rows_kernel, sweep_kernel, hits_kernel;
ctc_align::gather_kernel, align_kernel)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--full-length", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import keyword_reference as ref
    from asr import _lib, _ops, error, spot
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    B, T, V, K, Lalign, H = 32, 1000, 3000, a.K, 120, 4
    rs = np.random.RandomState(0)
    x = torch.from_numpy(ref.random_logits(T, B, V, 1, scale=1.0)).to(dev)
    xl = None if a.full_length else torch.from_numpy(rs.randint(600, T + 1, size=B).astype(np.int32)).to(dev)
    kws = spot.KeywordSet(ref.random_phrases(K, V, 2, 16, 2), V).to(dev)
    img = kws.image
    U, Lmax = kws.U, kws.Lmax
    p = _lib.ptr
    # the aligner's inputs: one transcript of 40 .. 120 labels per utterance
    lab = torch.from_numpy(rs.randint(1, V, size=(B, Lalign)).astype(np.int32)).to(dev)
    ll = torch.from_numpy(rs.randint(40, Lalign + 1, size=B).astype(np.int32)).to(dev)
    n_align = lib.asr_ctc_align_workspace_bytes(T, B, V, Lalign, 0)
    ws_align = torch.empty(n_align, dtype=torch.uint8, device=dev)
    frames = torch.empty((B, T), dtype=torch.int32, device=dev)
    tok = [torch.empty((B, Lalign), dtype=torch.int32, device=dev) for _ in range(4)]
    tok_logp = torch.empty((B, Lalign), dtype=torch.float32, device=dev)
    n_tok = torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    n_kws = lib.asr_kws_workspace_bytes(T, B, U)
    ws_kws = torch.empty(n_kws, dtype=torch.uint8, device=dev)
    det = torch.empty((B, K, T), dtype=torch.float32, device=dev)
    det_start = torch.empty((B, K, T), dtype=torch.int32, device=dev)
    fill = torch.empty((B, T), dtype=torch.float32, device=dev)
    hs, he = (torch.empty((B, K, H), dtype=torch.int32, device=dev) for _ in range(2))
    sc, lp = (torch.empty((B, K, H), dtype=torch.float32, device=dev) for _ in range(2))
    nh = torch.empty((B, K), dtype=torch.int32, device=dev)

    def align():
        rc = lib.asr_ctc_align(_lib.stream(), p(x), p(lab), None, p(xl), p(ll), T, B, V, Lalign, 0, p(frames), p(tok[0]), p(tok[1]),
                               p(tok[2]), p(tok[3]), p(tok_logp), p(n_tok), p(score), p(ws_align), n_align)
        assert rc == 0, rc

    def detect():
        rc = lib.asr_kws_detect(_lib.stream(), p(x), p(xl), T, B, V, 0, p(img["uniq"]), U, p(img["node_tok"]), p(img["kw_len"]), K,
                                Lmax, None, p(det), p(det_start), p(fill), p(ws_kws), n_kws)
        assert rc == 0, rc

    def hits():
        rc = lib.asr_kws_hits(_lib.stream(), p(det), p(det_start), p(fill), p(xl), B, K, T, H, float("-inf"), p(hs), p(he), p(sc),
                              p(lp), p(nh))
        assert rc == 0, rc

    def search():
        detect()
        hits()

    def public():
        spot.keyword_search(x, kws, xl, H)

    def beam():
        error.beam_decode(x, 16, 16, 0, xl)

    common = dict(B=B, T=T, V=V, K=K, U=U, Lmax=Lmax, max_hits=H, full_length=bool(a.full_length))
    ops = (("ctc_align", align), ("kws_detect", detect), ("kws_hits", hits), ("kws_detect+hits", search),
           ("keyword_search (python)", public), ("beam_decode beam 16", beam))
    table = {name: [] for name, _ in ops}
    for r in range(a.rounds):
        for name, fn in ops:
            ms = timed(fn, a.warmup, a.iters)
            table[name].append(ms)
            print(json.dumps(dict(op=name, round=r, ms=round(ms, 4), **common)), flush=True)
    for name, v in table.items():
        v = sorted(v)
        print(json.dumps(dict(op=name, summary=True, min_ms=round(v[0], 4), median_ms=round(v[len(v) // 2], 4), max_ms=round(v[-1], 4))))
    print(json.dumps(dict(op="workspace_bytes", align=n_align, kws=n_kws, state=lib.asr_kws_state_bytes(B, K, Lmax), **common)))
    print(json.dumps(dict(op="check", n_hits_mean=float(nh.float().mean().item()), best_score_mean=float(sc[:, :, 0].mean().item()),
                          **common)))


if __name__ == "__main__":
    main()
