"""Time the streaming forward of a convolutional recipe (asr.model.stream.AcousticStream over a cnn.AcousticModel) on the GPU.

Model: BASELINE configs[4] as bench.py builds it (``bench.cnn_config``: `zhang+residual`, ndim_h 128, ndim_dense 320, V = 119,
--num-conv-layers 4), sized by one call.
  oneshot   the one-shot forward of the model over T = 1000 frames, host clock around calls that end in a synchronise; per frame.
  advance   ms per ``advance`` of full chunks at B in {1, 8, 32}, Tc in {8, 16, 32, 64}: host clock around --iters advances that end
            in a device synchronise, best of --repeats rounds and their spread; us per frame = ms / Tc.  Beside it
              launches        kernels per advance and how many of them are the carry (asr_stream_push: two each), counted by the profiler over
                              one advance, with the device time of all kernels and of the carry kernels in that advance
              enqueue_ms      the host clock around the same advances WITHOUT the closing synchronise divided by their number: what
                              the host spends queueing one advance
              ds2_ms          the ds2 stream's row for the same (B, Tc), tau = 0, read from profiles/acoustic_stream.txt
  launch    an empty kernel's cost from the same clock (1000 one-element fills, then a synchronise).
One JSON line per measurement, also written to --out.

usage: python tools/time_cnn_stream.py [--iters 20] [--repeats 3] [--num-conv-layers 4] [--out profiles/cnn_stream.txt]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wall_ms(fn, warmup, iters, sync=True):
    """host clock around `iters` calls, per call; with `sync` the clock stops after a synchronise"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return ((time.perf_counter() if sync else t1) - t0) * 1e3 / iters


def rounds(fn, repeats, *args):
    ms = [fn(*args) for _ in range(repeats)]
    return round(min(ms), 4), round(max(ms) - min(ms), 4)


def kernels_of(fn):
    """[(kernel name, device us)] of one call of fn, from the profiler's device records; None where it gives none"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = [(e.name, float(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total))
           for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and not e.name.startswith(("Memcpy", "Memset"))]
    return out or None


def ds2_rows(path):
    rows = {}
    if os.path.isfile(path):
        with open(path) as fp:
            for line in fp:
                row = json.loads(line)
                if row.get("op") == "advance" and row.get("tau") == 0 and "ms" in row:
                    rows[(row["B"], row["Tc"])] = row["ms"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--chunks", default="8,16,32,64")
    ap.add_argument("--num-conv-layers", type=int, default=4)
    ap.add_argument("--vocab", type=int, default=119)
    ap.add_argument("--ds2", default=os.path.join(HERE, "profiles", "acoustic_stream.txt"))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "cnn_stream.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured on the host")
    import bench
    from asr import _lib, _ops
    from asr.model.architectures import build_model
    from asr.model.stream import AcousticStream
    dev = torch.device("cuda:0")
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    one = torch.zeros((1,), device=dev)
    launch_us = min(wall_ms(lambda: _ops.fill_(one, 0.0), 100, 1000) for _ in range(a.repeats)) * 1e3
    emit(op="launch", us=round(launch_us, 3))
    torch.manual_seed(0)
    cfg = bench.cnn_config(a, a.vocab)
    model = build_model(cfg).to_gpu()
    with torch.no_grad():
        model(torch.randn((2, 3, cfg.num_mel_filters, 64), device=dev))         # sizes the lazy parameters
    what = "%s, %d conv layers, ndim_h %d, ndim_dense %d, V %d" % (cfg.architecture, cfg.num_conv_layers, cfg.ndim_h, cfg.ndim_dense, a.vocab)
    ds2 = ds2_rows(a.ds2)
    chunks = [int(v) for v in a.chunks.split(",")]
    for B in (int(v) for v in a.batches.split(",")):
        with torch.no_grad():
            x1000 = torch.randn((B, 3, cfg.num_mel_filters, 1000), device=dev)
            oneshot, spread = rounds(wall_ms, a.repeats, lambda: model(x1000, split_into_variables=False), 1, 3)
        emit(op="oneshot", model=what, B=B, T=1000, ms=oneshot, spread_ms=spread, us_per_frame=round(oneshot, 3))
        for Tc in chunks:
            s = AcousticStream(model, B, max_chunk=max(chunks))
            x = torch.randn((B, 3, cfg.num_mel_filters, Tc), device=dev)
            try:
                ms, spread = rounds(wall_ms, a.repeats, lambda: s.advance(x), 3, a.iters)
            except _lib.AsrHipError as e:               # a shape one of the model's kernels does not serve: recorded, not timed
                emit(op="advance", B=B, Tc=Tc, error=str(e))
                continue
            enqueue, _ = rounds(wall_ms, a.repeats, lambda: s.advance(x), 3, a.iters, False)
            row = dict(op="advance", B=B, Tc=Tc, ms=ms, spread_ms=spread, us_per_frame=round(ms * 1e3 / Tc, 3),
                       oneshot_us_per_frame=round(oneshot, 3), enqueue_ms=enqueue, ds2_ms=ds2.get((B, Tc)))
            try:
                ks = kernels_of(lambda: s.advance(x))
            except Exception as e:                      # (a profiler that cannot see the device: the times above stand without it)
                ks, row["profiler"] = None, "%s: %s" % (type(e).__name__, e)
            if ks:
                push = [us for name, us in ks if "stream_window_kernel" in name or "stream_state_kernel" in name]      # csrc/stream.hip
                row.update(launches=len(ks), push_launches=len(push), kernels_us=round(sum(us for _, us in ks), 1),
                           push_us=round(sum(push), 1), empty_launches_us=round(len(ks) * launch_us, 1))
            emit(**row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
