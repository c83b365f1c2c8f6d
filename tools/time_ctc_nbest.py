"""Time the N-best CTC scoring (asr.loss.ctc_nbest_logp: forward + backward of sum gy * logp) against the route the project had
before it: connectionist_temporal_classification(reduce="no") on logits replicated N times (repeat_interleave(N, dim=1)), the same
gy, and the reduction of the replicated gradient back to (T, B, V).  Device events on the launch stream, warm-up, then --iters
timed forward + backward passes of each, in one process, in the order baseline, N-best, baseline again -- the two baseline figures
give that measurement's own run-to-run spread.  The replication of the logits itself is NOT timed (it favours the baseline).

Inputs: B = 32, T = 1000, V = 3000, x_len ~ U{600..1000}; logits = tests/ctc_beam_reference.py: peaky per utterance (randn, a
best path of 1-3 frame runs 7-14 above the rest, 15 % confusable frames with a second token at most 2 behind), seed 3 -- peaked
enough that the beam fills all N slots; hypotheses = asr.error.beam_decode(x, N, 16, lengths=x_len), ids cut to the longest
hypothesis; gy ~ N(0, 1), seed 4.

One JSON line per measurement.  For the kernel split run it under rocprofv3 --kernel-trace --stats (ctc_nbest::rows_kernel,
ctc::lattice_kernel<3>, ctc_nbest::grad_kernel; ctc::rows_kernel, ctc::grad_kernel and the reduction for the baseline).

usage: python tools/time_ctc_nbest.py [--iters 20] [--warmup 3] [--n 1,4,16]"""
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
    ap.add_argument("--n", default="1,4,16")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import ctc_beam_reference as beam_ref
    from asr import _lib
    from asr.error import beam_decode
    from asr.loss import connectionist_temporal_classification, ctc_nbest_logp
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    dev = torch.device("cuda:0")
    B, T, V = 32, 1000, 3000
    rs = np.random.RandomState(3)
    xs = np.stack([beam_ref.peaky(rs, T, V) for _ in range(B)], axis=1).astype(np.float32)
    rs = np.random.RandomState(4)
    x_len = rs.randint(600, T + 1, size=B).astype(np.int32)
    x0 = torch.from_numpy(xs).to(dev)
    xl = torch.from_numpy(x_len).to(dev)
    valid_rows = int(x_len.sum())
    for N in [int(v) for v in a.n.split(",")]:
        ids, lens, scores = beam_decode(x0, N, 16, 0, xl)
        lens = torch.where(scores > float("-inf"), lens, torch.full_like(lens, -1))
        width = max(1, int(lens.max().item()))
        hyps = ids[:, :, :width].contiguous()
        gy = torch.from_numpy(rs.randn(B, N).astype(np.float32)).to(dev)
        x = x0.clone().requires_grad_(True)
        x_rep = x0.repeat_interleave(N, dim=1).contiguous().requires_grad_(True)
        lab_rep, len_rep = hyps.reshape(B * N, width).contiguous(), lens.clamp_min(0).reshape(B * N).contiguous()
        xl_rep, gy_rep = xl.repeat_interleave(N).contiguous(), (-gy).reshape(B * N).contiguous()
        out = {}

        def baseline():
            x_rep.grad = None
            loss = connectionist_temporal_classification(x_rep, lab_rep, 0, xl_rep, len_rep, "no")
            loss.backward(gy_rep)
            out["base"] = x_rep.grad.view(T, B, N, V).sum(dim=2) if N > 1 else x_rep.grad
            out["base_logp"] = -loss.detach().reshape(B, N)

        def nbest():
            x.grad = None
            logp = ctc_nbest_logp(x, hyps, lens, 0, xl)
            logp.backward(gy)
            out["new"], out["new_logp"] = x.grad, logp.detach()

        def nbest_forward():
            ctc_nbest_logp(x.detach(), hyps, lens, 0, xl)

        # node_frames: sum over the used slots of (2 len + 1) * x_len[b] -- the alpha / beta entries (8 B each) the gradient pass reads
        node_frames = int((torch.where(lens >= 0, 2 * lens + 1, torch.zeros_like(lens)).sum(dim=1).long() * xl.long()).sum().item())
        common = dict(B=B, T=T, V=V, N=N, Lmax=width, valid_rows=valid_rows, used_slots=int((lens >= 0).sum().item()),
                      node_frames=node_frames)
        ms = {}
        for op, fn in (("baseline", baseline), ("nbest", nbest), ("baseline_again", baseline), ("nbest_forward_only", nbest_forward)):
            ms[op] = timed(fn, a.warmup, a.iters)
            print(json.dumps(dict(op=op, ms=round(ms[op], 4), **common)), flush=True)
        spread = abs(ms["baseline"] - ms["baseline_again"])
        base = min(ms["baseline"], ms["baseline_again"])
        print(json.dumps(dict(op="ratio", nbest_over_baseline=round(ms["nbest"] / base, 4), baseline_spread_ms=round(spread, 4),
                              not_longer_than_baseline_plus_spread=bool(ms["nbest"] <= max(ms["baseline"], ms["baseline_again"]) + spread),
                              shorter_than_baseline=bool(ms["nbest"] < base), **common)))
        lib = _lib.lib()
        print(json.dumps(dict(op="workspace_bytes", nbest=lib.asr_ctc_nbest_workspace_bytes(T, B, V, N, width),
                              baseline_loss=lib.asr_ctc_workspace_bytes(T, B * N, V, width, 0),
                              baseline_logits_and_gradient=2 * 4 * T * B * N * V, **common)))
        dg = float((out["new"] - out["base"]).abs().max()) / float(out["base"].abs().max())
        dl = float(((out["new_logp"] - out["base_logp"]).abs() / out["base_logp"].abs()).max())
        print(json.dumps(dict(op="check", max_dgrad_over_max_grad=dg, max_rel_dlogp=dl, **common)), flush=True)
        del x_rep, out


if __name__ == "__main__":
    main()
