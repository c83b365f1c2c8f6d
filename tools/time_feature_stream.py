"""Time the streaming log-mel front end (asr.fft.FeatureStream) on the GPU.

  advance   ms per ``advance`` at B in {1, 8, 32} and chunks of 1280, 2560 and 10240 int16 samples (80, 160 and 640 ms of audio at the
            Processor defaults): host clock around --iters advances that end in one device synchronise (what a serving loop sees),
            best of --repeats rounds and their spread; us per feature frame = ms / Tc.
  oneshot   ``Processor.logfbank_batch`` on the same total audio (B signals of iters * chunk samples, already padded on the device),
            the same clock: the yardstick, per frame.
  acoustic  one ``AcousticStream.advance`` of the matching frame count on the model of tools/time_acoustic_stream.py (2 conv blocks,
            4 x GRU-512, dense 320, V = 3000, lookahead 20), so the front end's share of a live chunk is on record.
  launch    an empty kernel's cost from the same clock (1000 launches of a one-element fill, then a synchronise): the floor three
            launches set.
One JSON line per measurement, also written to --out.

usage: python tools/time_feature_stream.py [--iters 20] [--repeats 3] [--out profiles/feature_stream.txt] [--no-acoustic]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wall_ms(fn, warmup, iters, before=None):
    """host clock around `iters` calls ending in a synchronise, per call"""
    import torch
    for _ in range(warmup):
        fn()
    if before is not None:
        before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def rounds(repeats, *args, **kw):
    ms = [wall_ms(*args, **kw) for _ in range(repeats)]
    return round(min(ms), 4), round(max(ms) - min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--chunks", default="1280,2560,10240")
    ap.add_argument("--no-acoustic", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "feature_stream.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured on the host")
    from asr import fft
    dev = torch.device("cuda:0")
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    one = torch.zeros((1,), device=dev)
    ms, spread = rounds(a.repeats, lambda: one.fill_(1.0), 10, 1000)
    emit(op="launch", us=round(ms * 1e3, 2), spread_us=round(spread * 1e3, 2))
    launch_us = ms * 1e3

    proc = fft.Processor(device=dev)
    S = proc.frame_step
    model = None
    if not a.no_acoustic:
        from asr.model import ds2
        from asr.model.stream import AcousticStream
        torch.manual_seed(0)
        cfg = ds2.configure()
        cfg.vocab_size, cfg.bidirectional, cfg.lookahead = 3000, False, 20
        model = ds2.Model(cfg).to_gpu()
    gen = torch.Generator(device="cpu").manual_seed(0)
    for B in (int(v) for v in a.batches.split(",")):
        for Nc in (int(v) for v in a.chunks.split(",")):
            audio = (torch.randn((B, a.iters * Nc), generator=gen) * 3000).round().to(torch.int16).to(dev)
            chunks = [audio[:, i * Nc:(i + 1) * Nc].contiguous() for i in range(a.iters)]
            fs = fft.FeatureStream(proc, B, Nc)
            Tc = fs.max_frames
            it = iter(())

            def restart():
                nonlocal it
                fs.reset()
                it = iter(chunks)

            def step():
                nonlocal it
                try:
                    c = next(it)
                except StopIteration:       # (the warm-up rounds wrap around)
                    it = iter(chunks)
                    c = next(it)
                fs.advance(c)

            ms, spread = rounds(a.repeats, step, 3, a.iters, before=restart)
            lens = (a.iters * Nc,) * B
            ms1, spread1 = rounds(a.repeats, lambda: proc.logfbank_batch((audio, lens)), 2, 3)
            frames1 = fft.num_frames(a.iters * Nc, proc.frame_len, S) - 2
            row = dict(op="advance", B=B, samples=Nc, audio_ms=round(Nc / 16.0, 1), Tc=Tc, ms=ms, spread_ms=spread,
                       us_per_frame=round(ms * 1e3 / Tc, 3), launches=3, empty_launches_us=round(3 * launch_us, 2),
                       oneshot_ms=ms1, oneshot_spread_ms=spread1, oneshot_frames=frames1, oneshot_us_per_frame=round(ms1 * 1e3 / frames1, 3))
            if model is not None:
                ac = AcousticStream(model, B, max_chunk=max(Tc, 8))
                x = torch.randn((B, 3, proc.num_mel_filters, Tc), device=dev)
                ms2, spread2 = rounds(a.repeats, lambda: ac.advance(x), 3, a.iters)
                row.update(acoustic_advance_ms=ms2, acoustic_spread_ms=spread2, front_end_share=round(ms / (ms + ms2), 4))
            emit(**row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
