"""Time the Gram-CTC keyword search (asr_gram_kws_detect + asr_kws_hits) against two things the parent commit already has, on the same
logits, in the same process, alternating: the CTC keyword search (asr_kws_detect + asr_kws_hits) on ONE fixed tokenisation of the
same phrases (all unigram tokens: what a user with a Gram-CTC model could run before), and the Gram-CTC beam search at beam 16,
top_k 16 (asr.error.gram_beam_decode: what such a user runs today to look for a phrase in every decomposition).
B = 32, T = 1000, V = 3000 f32 randn logits over an inventory of 118 unigrams and 2881 bigrams, K = 64 phrases of 2 to 16
characters, x_len ~ U{600..1000}, max_hits = 4; device events on the launch stream after warm-up; --rounds rounds of every
operation, so every figure comes with its spread.  One JSON line per measurement and a summary line (min / median / max).

usage: python tools/time_gram_keyword_search.py [--iters 20] [--warmup 3] [--rounds 5] [--K 64] [--full-length] [--no-beam]
                                                [--other-lib PATH]
--other-lib: a second build of libasr_hip.so (the parent commit's, say); its asr_kws_detect and asr_kws_hits join the rounds, so
that the kernels this feature does not touch are compared with their earlier selves in one process.
For the kernel split run it under rocprofv3 --kernel-trace --stats (ctc_kws::rows_kernel, gram_sweep_kernel, sweep_kernel,
hits_kernel)."""
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
    ap.add_argument("--no-beam", action="store_true")
    ap.add_argument("--other-lib", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import gram_keyword_reference as gref
    from asr import _lib, error, spot
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    B, T, V, K, H, NU = 32, 1000, 3000, a.K, 4, 118
    rs = np.random.RandomState(0)
    gram = gref.big_table(NU, V, seed=0)                             # 118 unigrams (token c spells character c), 2881 bigrams
    x = torch.from_numpy(gref.random_logits(T, B, V, 1, scale=1.0)).to(dev)
    xl = None if a.full_length else torch.from_numpy(rs.randint(600, T + 1, size=B).astype(np.int32)).to(dev)
    phrases = gref.random_strings(K, NU, 2, 16, 2)
    gkw = spot.GramKeywordSet(phrases, gram).to(dev)
    ckw = spot.KeywordSet(phrases, V).to(dev)                        # the all-unigram tokenisation of the same phrases
    gi, ci = gkw.image, ckw.image
    Lmax = gkw.Lmax
    assert ckw.Lmax == Lmax
    p = _lib.ptr
    n_g = lib.asr_kws_workspace_bytes(T, B, gkw.U)
    n_c = lib.asr_kws_workspace_bytes(T, B, ckw.U)
    ws = torch.empty(max(n_g, n_c), dtype=torch.uint8, device=dev)
    det = torch.empty((B, K, T), dtype=torch.float32, device=dev)
    det_start = torch.empty((B, K, T), dtype=torch.int32, device=dev)
    fill = torch.empty((B, T), dtype=torch.float32, device=dev)
    hs, he = (torch.empty((B, K, H), dtype=torch.int32, device=dev) for _ in range(2))
    sc, lp = (torch.empty((B, K, H), dtype=torch.float32, device=dev) for _ in range(2))
    nh = torch.empty((B, K), dtype=torch.int32, device=dev)

    def gram_detect():
        rc = lib.asr_gram_kws_detect(_lib.stream(), p(x), p(xl), T, B, V, 0, p(gi["uniq"]), gkw.U, p(gi["node_uni"]),
                                     p(gi["node_big"]), p(gi["kw_len"]), K, Lmax, None, p(det), p(det_start), p(fill), p(ws), n_g)
        assert rc == 0, rc

    def ctc_detect():
        rc = lib.asr_kws_detect(_lib.stream(), p(x), p(xl), T, B, V, 0, p(ci["uniq"]), ckw.U, p(ci["node_tok"]), p(ci["kw_len"]), K,
                                Lmax, None, p(det), p(det_start), p(fill), p(ws), n_c)
        assert rc == 0, rc

    def hits():
        rc = lib.asr_kws_hits(_lib.stream(), p(det), p(det_start), p(fill), p(xl), B, K, T, H, float("-inf"), p(hs), p(he), p(sc),
                              p(lp), p(nh))
        assert rc == 0, rc

    def other(handle):
        for name in ("asr_kws_detect", "asr_kws_hits"):
            getattr(handle, name).restype, getattr(handle, name).argtypes = _lib.SIGNATURES[name]

        def detect():
            rc = handle.asr_kws_detect(_lib.stream(), p(x), p(xl), T, B, V, 0, p(ci["uniq"]), ckw.U, p(ci["node_tok"]), p(ci["kw_len"]),
                                       K, Lmax, None, p(det), p(det_start), p(fill), p(ws), n_c)
            assert rc == 0, rc

        def hits_():
            rc = handle.asr_kws_hits(_lib.stream(), p(det), p(det_start), p(fill), p(xl), B, K, T, H, float("-inf"), p(hs), p(he),
                                     p(sc), p(lp), p(nh))
            assert rc == 0, rc
        return detect, hits_

    def gram_search():
        gram_detect()
        hits()

    def ctc_search():
        ctc_detect()
        hits()

    def public():
        spot.keyword_search(x, gkw, xl, H)

    def beam():
        error.gram_beam_decode(x, gram, 16, 16, 0, xl)

    common = dict(B=B, T=T, V=V, K=K, U_gram=gkw.U, U_ctc=ckw.U, Lmax=Lmax, max_hits=H, full_length=bool(a.full_length))
    ops = [("ctc kws_detect", ctc_detect), ("gram_kws_detect", gram_detect), ("kws_hits", hits), ("ctc kws_detect+hits", ctc_search),
           ("gram_kws_detect+hits", gram_search), ("keyword_search (python, gram)", public)]
    if a.other_lib:
        import ctypes
        od, oh = other(ctypes.CDLL(os.path.abspath(a.other_lib)))
        ops[1:1] = [("ctc kws_detect (other lib)", od)]
        ops.append(("kws_hits (other lib)", oh))
    if not a.no_beam:
        ops.append(("gram_beam_decode beam 16 top_k 16", beam))
    table = {name: [] for name, _ in ops}
    for r in range(a.rounds):
        order = list(ops)
        if a.other_lib and r % 2:                                    # the two builds of asr_kws_detect trade places every round
            order[0], order[1] = order[1], order[0]
        for name, fn in order:
            ms = timed(fn, a.warmup, a.iters)
            table[name].append(ms)
            print(json.dumps(dict(op=name, round=r, ms=round(ms, 4), **common)), flush=True)
    for name, v in table.items():
        v = sorted(v)
        print(json.dumps(dict(op=name, summary=True, min_ms=round(v[0], 4), median_ms=round(v[len(v) // 2], 4), max_ms=round(v[-1], 4))))
    gram_search()
    torch.cuda.synchronize()
    print(json.dumps(dict(op="workspace_bytes", gram=n_g, ctc=n_c, gram_state=lib.asr_gram_kws_state_bytes(B, K, Lmax),
                          ctc_state=lib.asr_kws_state_bytes(B, K, Lmax), **common)))
    print(json.dumps(dict(op="check", n_hits_mean=float(nh.float().mean().item()), best_score_mean=float(sc[:, :, 0].mean().item()),
                          **common)))


if __name__ == "__main__":
    main()
