"""Time the latency-controlled bidirectional GRU (asr.nn.LCBiGRU, csrc/lc_window.hip) on the GPU.

  copy      asr_lc_gather, asr_lc_scatter (both modes, the forward pass's with its addend) and asr_lc_push at
            (T, B, R) = (1000, 32, 512), (Nc, Nr) = --control: device events over --kernel-iters launches, as GB/s over the tensors
            a kernel reads and writes, beside a device copy of one (T, B, R) tensor.
  train     BASELINE configs[1] (2 conv blocks, 4 recurrent layers of 512, dense 320, V = 3000, B = 32, T = 1000, bf16): forward + CTC +
            backward of the plain bidirectional model and of the same model with latency_control = --control, device events around
            --iters steps behind a warm-up, best of --repeats rounds and their spread.
  stream    the latency-controlled configs[1]: ms per ``AcousticStream.advance`` of full chunks of Tc frames at B in {1, 8, 32},
            Tc in {8, 16, 32, 64}: host clock around --iters advances that end in a device synchronise (what a serving loop sees), best
            of --repeats rounds and their spread; beside it the forward-only model of profiles/acoustic_stream.txt in the same run.
One JSON line per measurement, also written to --out.

usage: python tools/time_lc_bigru.py [--only copy,train,stream] [--control 32,16] [--out profiles/lc_bigru.txt]"""
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
    ap.add_argument("--only", default="copy,train,stream")
    ap.add_argument("--control", default="32,16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--chunks", default="8,16,32,64")
    ap.add_argument("--vocab", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "lc_bigru.txt"))
    a = ap.parse_args()
    for p in (HERE, os.path.join(HERE, "chainer-speech-recognition_amd")):
        sys.path.insert(0, p)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured on the host")
    from asr import _ops
    from asr.functions import join_side_stream
    from asr.loss import connectionist_temporal_classification
    from asr.model import ds2
    from asr.model.stream import AcousticStream
    from oracle import model as omodel
    dev = torch.device("cuda:0")
    only = a.only.split(",")
    Nc, Nr = (int(v) for v in a.control.split(","))
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    if "copy" in only:
        T, B, R = 1000, 32, 512
        x = torch.randn((T, B, R), device=dev).to(_ops.BF16)
        y = torch.empty_like(x)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        tensor_bytes = x.numel() * 2
        ms_copy, spread = rounds(event_ms, a.repeats, lambda: y.copy_(x), 10, a.kernel_iters)
        emit(op="copy", T=T, B=B, R=R, us=round(ms_copy * 1e3, 2), spread_us=round(spread * 1e3, 2),
             GBps=round(2 * tensor_bytes / (ms_copy * 1e-3) / 1e9, 1))
        xw, _ = _ops.lc_gather(x, Nc, Nr, _ops.LC_WINDOW, lens)
        window_bytes = xw.numel() * 2
        cases = (("lc_gather_window", lambda: _ops.lc_gather(x, Nc, Nr, _ops.LC_WINDOW, lens), tensor_bytes + window_bytes),
                 ("lc_gather_block", lambda: _ops.lc_gather(x, Nc, Nr, _ops.LC_BLOCK, lens, want_len=False), tensor_bytes + window_bytes),
                 ("lc_scatter_block_addend", lambda: _ops.lc_scatter(xw, T, B, Nc, Nr, _ops.LC_BLOCK, x, lens, out=y), 3 * tensor_bytes),
                 ("lc_scatter_window", lambda: _ops.lc_scatter(xw, T, B, Nc, Nr, _ops.LC_WINDOW, None, lens, out=y),
                  window_bytes + tensor_bytes))
        for name, fn, moved in cases:
            ms, spread = rounds(event_ms, a.repeats, fn, 10, a.kernel_iters)
            emit(op=name, Nc=Nc, Nr=Nr, T=T, B=B, R=R, windows=xw.shape[1], window_rows=xw.shape[0], us=round(ms * 1e3, 2),
                 spread_us=round(spread * 1e3, 2), GBps=round(moved / (ms * 1e-3) / 1e9, 1),
                 of_copy_rate=round(moved / (ms * 1e-3) / (2 * tensor_bytes / (ms_copy * 1e-3)), 3))
        K, Tc = Nc + Nr - 1, 64
        state = torch.zeros((K, B, R), dtype=_ops.BF16, device=dev)
        m = torch.zeros((B,), dtype=torch.int32, device=dev)
        chunk, window = x[:Tc].contiguous(), torch.empty((K + Tc, B, R), dtype=_ops.BF16, device=dev)
        ms, spread = rounds(event_ms, a.repeats, lambda: _ops.lc_push(state, m, chunk, None, window, Nc, Nr), 10, a.kernel_iters)
        moved = (2 * (K + Tc) + 2 * K) * B * R * 2                # window written and read, state read and written
        emit(op="lc_push", Nc=Nc, Nr=Nr, Tc=Tc, B=B, R=R, launches=2, us=round(ms * 1e3, 2), spread_us=round(spread * 1e3, 2),
             GBps=round(moved / (ms * 1e-3) / 1e9, 1))

    def configs1(**fields):
        torch.manual_seed(0)
        cfg = ds2.configure()
        cfg.vocab_size = a.vocab
        for name, value in fields.items():
            setattr(cfg, name, value)
        return cfg, ds2.Model(cfg).to_gpu()

    if "train" in only:
        B, T = 32, 1000
        x, labels, x_len, l_len = omodel.synthetic_batch(B, T, a.vocab, seed=0)
        x, x_len, labels, l_len = x.to(dev), x_len.to(dev), labels.to(dev), l_len.to(dev)
        for control in (None, (Nc, Nr)):
            cfg, model = configs1(latency_control=control)

            def forward():
                with torch.no_grad():
                    model(x, x_length=x_len)

            def step():
                for p in model.parameters():
                    p.grad = None
                loss = connectionist_temporal_classification(model(x, x_length=x_len), labels, 0, x_len, l_len)
                loss.backward()
                join_side_stream()

            ms_f, sp_f = rounds(event_ms, a.repeats, forward, 3, a.iters)
            ms, spread = rounds(event_ms, a.repeats, step, 3, a.iters)
            emit(op="train_step", latency_control=control, B=B, T=T, V=a.vocab, forward_ms=ms_f, forward_spread_ms=sp_f, ms=ms, spread_ms=spread,
                 windows=None if control is None else -(-T // Nc) * B, window_rows=None if control is None else Nc + Nr)
            del model

    if "stream" in only:
        batches = [int(v) for v in a.batches.split(",")]
        chunks = [int(v) for v in a.chunks.split(",")]
        for name, fields in (("forward_only", dict(bidirectional=False)), ("latency_control", dict(latency_control=(Nc, Nr)))):
            cfg, model = configs1(**fields)
            for B in batches:
                for Tc in chunks:
                    s = AcousticStream(model, B, max_chunk=max(chunks))
                    x = torch.randn((B, 3, cfg.num_mel_filters, Tc), device=dev)
                    ms, spread = rounds(wall_ms, a.repeats, lambda: s.advance(x), 3, a.iters * 2)
                    emit(op="advance", model=name, control=fields.get("latency_control"), delay=s.delay, B=B, Tc=Tc, ms=ms, spread_ms=spread,
                         us_per_frame=round(ms * 1e3 / Tc, 3))
            del model
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
