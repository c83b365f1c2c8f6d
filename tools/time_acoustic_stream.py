"""Time the streaming forward (asr.model.stream.AcousticStream) and the lookahead convolution kernels on the GPU.

Model: BASELINE configs[1] made forward-only (2 conv blocks, 4 x GRU-512, dense 320, V = 3000), lookahead tau in {0, 20}.
  stream    ms per ``advance`` of full chunks at B in {1, 8, 32}, Tc in {8, 16, 32, 64}: host clock around --iters advances that
            end in a device synchronise (an advance is some hundred launches; the synchronised wall time is what a serving loop
            sees), best of --repeats rounds and their spread; us per frame = ms / Tc.  Beside it the one-shot forward of the same
            model over T = 1000 frames, per frame.
  gru       the same chunk through the four ``nn.GRU`` calls alone (input projection + asr_gru_fwd_state), and through the four
            asr_gru_fwd_state calls alone (the one-launch-per-time-step recurrences): their share of the advance.
  lookahead asr_lookahead_fwd / asr_lookahead_bwd at (T, B, D) = (1000, 32, 512), tau = 20, device events over --kernel-iters
            launches, as GB/s over the tensors the operation must move (forward: x in, y out; backward: gy and x in, dx out),
            beside a device copy of one such tensor (one in, one out).
One JSON line per measurement, also written to --out.

usage: python tools/time_acoustic_stream.py [--iters 20] [--repeats 3] [--kernel-iters 200] [--out profiles/acoustic_stream.txt]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wall_ms(fn, warmup, iters):
    """host clock around `iters` calls ending in a synchronise, per call"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_ms(fn, warmup, iters):
    """device events around `iters` calls, per call"""
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


def rounds(fn, repeats, *args):
    ms = [fn(*args) for _ in range(repeats)]
    return round(min(ms), 4), round(max(ms) - min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--chunks", default="8,16,32,64")
    ap.add_argument("--taus", default="0,20")
    ap.add_argument("--vocab", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "acoustic_stream.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured on the host")
    from asr import _lib, _ops
    from asr.model import ds2
    from asr.model.stream import AcousticStream
    dev = torch.device("cuda:0")
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    batches = [int(v) for v in a.batches.split(",")]
    chunks = [int(v) for v in a.chunks.split(",")]
    for tau in (int(v) for v in a.taus.split(",")):
        torch.manual_seed(0)
        cfg = ds2.configure()
        cfg.vocab_size, cfg.bidirectional, cfg.lookahead = a.vocab, False, tau
        model = ds2.Model(cfg).to_gpu()
        H = cfg.ndim_rnn
        for B in batches:
            with torch.no_grad():
                x1000 = torch.randn((B, 3, cfg.num_mel_filters, 1000), device=dev)
                oneshot, spread = rounds(wall_ms, a.repeats, lambda: model(x1000, split_into_variables=False), 1, 3)
            emit(op="oneshot", tau=tau, B=B, T=1000, ms=oneshot, spread_ms=spread, us_per_frame=round(oneshot, 3))
            grus = [layer for layer in model.rnn_blocks.layers if hasattr(layer, "w_hh")]
            for Tc in chunks:
                s = AcousticStream(model, B, max_chunk=max(chunks))
                x = torch.randn((B, 3, cfg.num_mel_filters, Tc), device=dev)
                try:
                    ms, spread = rounds(wall_ms, a.repeats, lambda: s.advance(x), 3, a.iters)
                except _lib.AsrHipError as e:           # a shape one of the model's kernels does not serve: recorded, not timed
                    emit(op="advance", tau=tau, B=B, Tc=Tc, error=str(e))
                    continue
                # the recurrent layers alone, on inputs of the shapes they see inside the advance
                with torch.no_grad():
                    widths = [s.model._merged[0] * s.model._merged[1]] + [H] * (len(grus) - 1)
                    inputs = [torch.randn((Tc, B, w), device=dev).to(_ops.BF16).permute(1, 2, 0) for w in widths]
                    hx = torch.zeros((1, B, H), device=dev)
                    gi = torch.randn((Tc * B, 3 * H), device=dev)

                    def links():
                        for layer, inp in zip(grus, inputs):
                            layer(inp, None, hx=hx)

                    def steps():
                        for layer in grus:
                            _ops.gru_fwd_state(gi, layer._compute_cache["whh16"][1], layer.b_hh.detach().reshape(-1), hx, Tc, B, H, 1, None)

                    ms_links, _ = rounds(wall_ms, a.repeats, links, 3, a.iters)
                    ms_steps, _ = rounds(wall_ms, a.repeats, steps, 3, a.iters)
                emit(op="advance", tau=tau, B=B, Tc=Tc, ms=ms, spread_ms=spread, us_per_frame=round(ms * 1e3 / Tc, 3),
                     oneshot_us_per_frame=round(oneshot, 3), gru_links_ms=ms_links, gru_steps_ms=ms_steps,
                     gru_links_share=round(ms_links / ms, 3), gru_steps_share=round(ms_steps / ms, 3))
        del model
    # the lookahead kernels against the copy rate
    T, B, D, tau = 1000, 32, 512, 20
    x = torch.randn((T, B, D), device=dev).to(_ops.BF16)
    gy = torch.randn((T, B, D), device=dev).to(_ops.BF16)
    W = torch.randn((D, tau + 1), device=dev)
    dW = torch.zeros_like(W)
    y = torch.empty_like(x)
    tensor_bytes = x.numel() * 2
    for name, fn, tensors in (("copy", lambda: y.copy_(x), 2),
                              ("lookahead_fwd", lambda: _ops.lookahead_fwd(x, W, None, out=y), 2),
                              ("lookahead_bwd_dx", lambda: _ops.lookahead_bwd(gy, None, W, None, None), 2),
                              ("lookahead_bwd_dw", lambda: _ops.lookahead_bwd(gy, x, W, None, dW, need_dx=False), 2),
                              ("lookahead_bwd", lambda: _ops.lookahead_bwd(gy, x, W, None, dW), 3)):
        ms, spread = rounds(event_ms, a.repeats, fn, 10, a.kernel_iters)
        emit(op=name, T=T, B=B, D=D, tau=tau, us=round(ms * 1e3, 2), spread_us=round(spread * 1e3, 2), tensors_moved=tensors,
             GBps=round(tensors * tensor_bytes / (ms * 1e-3) / 1e9, 1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
