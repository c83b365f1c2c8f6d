"""Time the SRU sequence layer (asr.nn.SeqSRU / BiSeqSRU, csrc/sru_seq.hip) and ds2.Model(rnn="sru") on the GPU, all in one run.

  scan      asr_sru_seq_fwd / asr_sru_seq_bwd alone at T = 1000, B = 32, D = 512, k in {3, 4}, ndir in {1, 2}, beside the parent's
            asr_sru_fwd / asr_sru_bwd (k = 3, ndir = 1) and a device copy of as many bytes: device events over --kernel-iters launches.
            Bytes are what include/asr_hip.h's semantics imply a scan must move (every operand read once, every result written once;
            the summary pass's second read of f, z and C1's read-back are not counted): `of_copy_rate` is that rate over the copy's.
            Every scan rotates over four sets of operands, so that no launch finds its inputs in the last-level cache.
  layer     the layer through autograd (projection + scan; + backward scan and the two gradient products) at I = D = 512 and I = 384,
            ndir 1 and 2, beside the parent's nn.SRU (I = D, ndir = 1) and the GRU / BiGRU layer of the same width.
  train     BASELINE configs[1] (2 conv blocks, 4 recurrent layers of 512, dense 320, V = 3000, B = 32, T = 1000, bf16): forward and forward +
            CTC + backward with rnn="gru" and rnn="sru", bidirectional and forward-only, alternating, best of --repeats rounds and spread.
  stream    forward-only configs[1]: ms per ``AcousticStream.advance`` of full chunks of 8 and 64 frames for 32 slots, rnn="gru" against
            rnn="sru": host clock around --iters advances that end in a device synchronise.
One JSON line per measurement, also written to --out.

usage: python tools/time_sru_stack.py [--only scan,layer,train,stream] [--out profiles/sru_stack.txt]"""
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


def scan_bytes(T, B, D, k, ndir):
    """(forward, backward) bytes the semantics imply: forward reads U (4 k ndir) and x (2, k = 3), writes C (4 ndir) and y (2); backward
    reads U, C (4 ndir), gy (2) and x (2, k = 3), writes gU (2 k ndir) and gxh (2, k = 3) -- per (t, b, d)"""
    n, hx = T * B * D, 2 if k == 3 else 0
    return n * (4 * k * ndir + hx + 4 * ndir + 2), n * (4 * k * ndir + 4 * ndir + 2 + hx + 2 * k * ndir + hx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="scan,layer,train,stream")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=1000)
    ap.add_argument("--vocab", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sru_stack.txt"))
    a = ap.parse_args()
    for p in (HERE, os.path.join(HERE, "chainer-speech-recognition_amd")):
        sys.path.insert(0, p)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured on the host")
    from asr import _ops, nn
    from asr.functions import join_side_stream
    from asr.loss import connectionist_temporal_classification
    from asr.model import ds2
    from asr.model.stream import AcousticStream
    from oracle import model as omodel
    dev = torch.device("cuda:0")
    only = a.only.split(",")
    lines = []
    T, B, D = 1000, 32, 512

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    if "scan" in only:
        big = torch.empty((T * B * D * 16,), dtype=torch.uint8, device=dev)           # 262 MB each way: beyond the caches
        dst = torch.empty_like(big)
        ms_copy, spread = rounds(event_ms, a.repeats, lambda: dst.copy_(big), 5, 20)
        copy_rate = 2 * big.numel() / (ms_copy * 1e-3)
        emit(op="copy", bytes_each_way=big.numel(), ms=ms_copy, spread_ms=spread, GBps=round(copy_rate / 1e9, 1))
        del big, dst
        # every scan rotates over ROT sets of its operands, so that a launch finds none of its inputs in the 256 MB last-level cache
        # (a set is 300 .. 900 MB with its results; re-running one set would flatter the scan against the copy)
        ROT = 4
        turn = [0]

        def rotate(fn):
            def call():
                turn[0] = (turn[0] + 1) % ROT
                fn(turn[0])
            return call
        xs = [torch.randn((T, B, D), device=dev).to(_ops.BF16) for _ in range(ROT)]
        gys = [torch.randn((T, B, D), device=dev).to(_ops.BF16) for _ in range(ROT)]
        U3 = [torch.randn((T * B, 3 * D), device=dev) for _ in range(ROT)]
        bias1, c0, gb1 = torch.zeros((2 * D,), device=dev), torch.zeros((B, D), device=dev), torch.zeros((2 * D,), device=dev)
        Cs = [_ops.sru_fwd(xs[i], U3[i], bias1, c0, None, True)[1] for i in range(ROT)]
        fb, bb = scan_bytes(T, B, D, 3, 1)
        ms_f, sp_f = rounds(event_ms, a.repeats, rotate(lambda i: _ops.sru_fwd(xs[i], U3[i], bias1, c0, None, True)), 5, a.kernel_iters)
        ms_b, sp_b = rounds(event_ms, a.repeats, rotate(lambda i: _ops.sru_bwd(xs[i], U3[i], bias1, Cs[i], c0, None, gys[i], None, gb1, True)),
                            5, a.kernel_iters)
        emit(op="parent_scan", entry="asr_sru_fwd/asr_sru_bwd", k=3, ndir=1, T=T, B=B, D=D, fwd_ms=ms_f, fwd_spread_ms=sp_f, bwd_ms=ms_b,
             bwd_spread_ms=sp_b, fwd_of_copy_rate=round(fb / (ms_f * 1e-3) / copy_rate, 3), bwd_of_copy_rate=round(bb / (ms_b * 1e-3) / copy_rate, 3))
        del U3, Cs
        for ragged in (False, True):
            for ndir in (1, 2):
                for k in (3, 4):
                    Us = [torch.randn((T * B, ndir * k * D), device=dev) for _ in range(ROT)]
                    bias, gb = torch.zeros((ndir, 2 * D), device=dev), torch.zeros((ndir, 2 * D), device=dev)
                    n = torch.linspace(T // 2, T, B, device=dev).to(torch.int32) if ragged else None
                    xk = xs if k == 3 else [None] * ROT
                    Ck = [_ops.sru_seq_fwd(xk[i], Us[i], bias, None, n, T, B, D, k, ndir, True)[1] for i in range(ROT)]
                    fb, bb = scan_bytes(T, B, D, k, ndir)
                    ms_f, sp_f = rounds(event_ms, a.repeats,
                                        rotate(lambda i: _ops.sru_seq_fwd(xk[i], Us[i], bias, None, n, T, B, D, k, ndir, True)), 5, a.kernel_iters)
                    ms_b, sp_b = rounds(event_ms, a.repeats,
                                        rotate(lambda i: _ops.sru_seq_bwd(xk[i], Us[i], bias, Ck[i], None, n, gys[i], None, gb, T, B, D, k, ndir, True)),
                                        5, a.kernel_iters)
                    row = dict(op="seq_scan", entry="asr_sru_seq_fwd/asr_sru_seq_bwd", k=k, ndir=ndir, ragged=ragged, T=T, B=B, D=D, fwd_ms=ms_f,
                               fwd_spread_ms=sp_f, bwd_ms=ms_b, bwd_spread_ms=sp_b)
                    if not ragged:      # (a ragged batch moves fewer bytes than the padded block: no rate is claimed for it)
                        row.update(fwd_bytes=fb, bwd_bytes=bb, fwd_of_copy_rate=round(fb / (ms_f * 1e-3) / copy_rate, 3),
                                   bwd_of_copy_rate=round(bb / (ms_b * 1e-3) / copy_rate, 3))
                    emit(**row)

    def time_layer(name, layer, I, call):
        xin = torch.randn((B, I, T), device=dev).to(_ops.BF16).requires_grad_(True)
        g = torch.randn((B, D, T), device=dev).to(_ops.BF16)

        def forward():
            with torch.no_grad():
                call(layer, xin)

        def both():
            for p in layer.parameters():
                p.grad = None
            xin.grad = None
            call(layer, xin).backward(g)
            join_side_stream()
        ms_f, sp_f = rounds(event_ms, a.repeats, forward, 3, a.iters * 2)
        ms, sp = rounds(event_ms, a.repeats, both, 3, a.iters * 2)
        emit(op="layer", layer=name, I=I, D=D, T=T, B=B, fwd_ms=ms_f, fwd_spread_ms=sp_f, fwd_bwd_ms=ms, fwd_bwd_spread_ms=sp)

    if "layer" in only:
        torch.manual_seed(0)
        zero = torch.zeros((B, D), device=dev)
        time_layer("nn.SRU (parent)", nn.SRU(D).to(dev), D, lambda layer, v: layer(v, zero)[0])
        for I in (D, 384):
            time_layer("nn.SeqSRU", nn.SeqSRU(I, D).to(dev), I, lambda layer, v: layer(v))
            time_layer("nn.BiSeqSRU", nn.BiSeqSRU(I, D).to(dev), I, lambda layer, v: layer(v))
            time_layer("nn.GRU", nn.GRU(I, D).to(dev), I, lambda layer, v: layer(v))
            time_layer("nn.BiGRU", nn.BiGRU(I, D).to(dev), I, lambda layer, v: layer(v))

    def configs1(**fields):
        torch.manual_seed(0)
        cfg = ds2.configure()
        cfg.vocab_size = a.vocab
        for name, value in fields.items():
            setattr(cfg, name, value)
        return cfg, ds2.Model(cfg).to_gpu()

    if "train" in only:
        x, labels, x_len, l_len = omodel.synthetic_batch(B, T, a.vocab, seed=0)
        x, x_len, labels, l_len = x.to(dev), x_len.to(dev), labels.to(dev), l_len.to(dev)
        for bidirectional in (True, False):
            models = {rnn: configs1(rnn=rnn, bidirectional=bidirectional)[1] for rnn in ("gru", "sru")}
            best = {rnn: [[], []] for rnn in models}
            for _ in range(a.repeats):              # the two versions alternate inside one run
                for rnn, model in models.items():
                    def forward():
                        with torch.no_grad():
                            model(x, x_length=x_len)

                    def step():
                        for p in model.parameters():
                            p.grad = None
                        connectionist_temporal_classification(model(x, x_length=x_len), labels, 0, x_len, l_len).backward()
                        join_side_stream()
                    best[rnn][0].append(event_ms(forward, 2, a.iters))
                    best[rnn][1].append(event_ms(step, 2, a.iters))
            for rnn, (f, s) in best.items():
                emit(op="train_step", rnn=rnn, bidirectional=bidirectional, B=B, T=T, V=a.vocab, forward_ms=round(min(f), 3),
                     forward_spread_ms=round(max(f) - min(f), 3), ms=round(min(s), 3), spread_ms=round(max(s) - min(s), 3),
                     parameters=sum(p.numel() for p in models[rnn].parameters()))
            del models

    if "stream" in only:
        for rnn in ("gru", "sru"):
            cfg, model = configs1(rnn=rnn, bidirectional=False)
            for Tc in (8, 64):
                s = AcousticStream(model, 32, max_chunk=64)
                xc = torch.randn((32, 3, cfg.num_mel_filters, Tc), device=dev)
                ms, spread = rounds(wall_ms, a.repeats, lambda: s.advance(xc), 3, a.iters * 2)
                emit(op="advance", rnn=rnn, B=32, Tc=Tc, ms=ms, spread_ms=spread, us_per_frame=round(ms * 1e3 / Tc, 3))
            del model
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
