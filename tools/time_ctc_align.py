"""Time the CTC / Gram-CTC forced alignment (asr_ctc_align) against the loss forward (asr_ctc_forward) on the same inputs, with
device events on the launch stream: B = 32, T = 1000, V = 3000, L ~ U{40..120}, x_len ~ U{600..1000} (the randn full-size case of
tests/ctc_align_reference.py), CTC and Gram-CTC; warm-up, then --iters timed launches of each, alternating in one process:
loss forward, alignment, loss forward again -- the two loss figures give that measurement's own run-to-run spread.
One JSON line per measurement; GBps = T*B*V*4 bytes of logits over the whole call (both calls read them once from HBM).

usage: python tools/time_ctc_align.py [--iters 20] [--warmup 3] [--modes ctc,gram] [--full-length] [--dead-labels]
  --full-length  every utterance has all T frames (x_len = NULL)
  --dead-labels  every label is an id outside [0, V): no utterance has a live path, so the alignment is prep + gather + sweep only
                 (no back-trace, no spans) -- the difference to the normal run is what those two cost
For the split gather / sweep + back-trace + spans run it under rocprofv3 --kernel-trace --stats (gather_kernel, align_kernel;
rows_kernel, lattice_kernel for the loss)."""
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
    ap.add_argument("--modes", default="ctc,gram")
    ap.add_argument("--full-length", action="store_true")
    ap.add_argument("--dead-labels", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    import torch
    import ctc_align_reference as ref
    from asr import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    B, T, V, Lmax = 32, 1000, 3000, 120
    for mode in a.modes.split(","):
        gram = mode == "gram"
        xs, uni, big, xl, tl = ref.full_case("randn", gram, seed=20 + gram, B=B, T=T, V=V, Lmax=Lmax)
        if a.dead_labels:
            uni[:] = V
        x, u, l2 = torch.from_numpy(xs).to(dev), torch.from_numpy(uni).to(dev), torch.from_numpy(tl).to(dev)
        g = torch.from_numpy(big).to(dev) if gram else None
        l1 = None if a.full_length else torch.from_numpy(xl).to(dev)
        p = _lib.ptr
        n_loss = lib.asr_ctc_workspace_bytes(T, B, V, Lmax, int(gram))
        n_align = lib.asr_ctc_align_workspace_bytes(T, B, V, Lmax, int(gram))
        ws_loss = torch.empty(n_loss, dtype=torch.uint8, device=dev)
        ws_align = torch.empty(n_align, dtype=torch.uint8, device=dev)
        loss_b = torch.empty(B, dtype=torch.float32, device=dev)
        frames = torch.empty((B, T), dtype=torch.int32, device=dev)
        tok = [torch.empty((B, Lmax), dtype=torch.int32, device=dev) for _ in range(4)]
        tok_logp = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
        n_tok = torch.empty(B, dtype=torch.int32, device=dev)
        score = torch.empty(B, dtype=torch.float32, device=dev)

        def loss():
            rc = lib.asr_ctc_forward(_lib.stream(), p(x), p(u), p(g), p(l1), p(l2), T, B, V, Lmax, 0, p(loss_b), None, p(ws_loss), n_loss)
            assert rc == 0, rc

        def align():
            rc = lib.asr_ctc_align(_lib.stream(), p(x), p(u), p(g), p(l1), p(l2), T, B, V, Lmax, 0, p(frames), p(tok[0]), p(tok[1]),
                                   p(tok[2]), p(tok[3]), p(tok_logp), p(n_tok), p(score), p(ws_align), n_align)
            assert rc == 0, rc

        common = dict(mode=mode, B=B, T=T, V=V, Lmax=Lmax, full_length=bool(a.full_length), dead_labels=bool(a.dead_labels))
        gbps = lambda ms: round(T * B * V * 4 / ms / 1e6, 1)      # noqa: E731
        for op, fn in (("ctc_forward", loss), ("ctc_align", align), ("ctc_forward_again", loss)):
            ms = timed(fn, a.warmup, a.iters)
            print(json.dumps(dict(op=op, ms=round(ms, 4), GBps=gbps(ms), **common)))
        print(json.dumps(dict(op="workspace_bytes", loss=n_loss, align=n_align, **common)))
        print(json.dumps(dict(op="check", score_mean=float(score.mean().item()), minus_loss_mean=float(-loss_b.mean().item()),
                              n_tok_mean=float(n_tok.float().mean().item()), **common)))


if __name__ == "__main__":
    main()
