"""Time the N-best Gram-CTC scoring (asr.loss.gram_ctc_nbest_logp: forward + backward of sum gy * logp) against the only route the
project had before it: gram_ctc(reduce="no") on logits replicated N times (repeat_interleave(N, dim=1)) with the labels of every
string looked up on the host beforehand (not timed), the same gy, and the reduction of the replicated gradient back to (T, B, V).
Device events on the launch stream, warm-up, then --iters timed forward + backward passes of each, in one process, in the order
baseline, N-best, baseline again -- the two baseline figures give that measurement's own run-to-run spread.  The replication of the
logits itself is NOT timed (it favours the baseline).

Inputs: B = 32, T = 1000, V = 3000 = blank + 118 characters + 2881 bigrams dealt onto shuffled token ids
(tests/gram_nbest_reference.py: shuffled_table(118, 2881, seed 3000)), x_len ~ U{600..1000}; logits =
tests/gram_beam_reference.py: peaky_gram per utterance, seed 3; strings = asr.error.gram_beam_decode(x, gram, N, 16, lengths=x_len),
ids cut to the longest string; gy ~ N(0, 1), seed 4.

"nbest" is the public function with the NumPy table: it validates the table on the host and uploads it on every call.
"nbest_checked_table" is the same forward + backward on a table that is validated and on the device already.

One JSON line per measurement.  "new_kernels" times the three launches the Gram-CTC entry puts in front of the shared ones (index
fill, index insert, gram_labels) by themselves: the forward at T = 1 on the same strings, minus nothing -- an upper bound, since
that call still runs the five shared kernels on one frame.  For the exact split run it under rocprofv3 --kernel-trace --stats.

usage: python tools/time_gram_ctc_nbest.py [--iters 20] [--warmup 3] [--n 1,4,16]"""
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
    import gram_beam_reference as gref
    import gram_nbest_reference as nref
    from asr import _lib
    from asr.error import gram_beam_decode
    from asr.loss import gram_ctc, gram_ctc_nbest_logp
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    dev = torch.device("cuda:0")
    B, T = 32, 1000
    gram = nref.shuffled_table(118, 2881, seed=3000)
    V = len(gram)
    uni = gref.unigram_ids(gram)
    rs = np.random.RandomState(3)
    xs = np.stack([gref.peaky_gram(rs, T, gram) for _ in range(B)], axis=1).astype(np.float32)
    rs = np.random.RandomState(4)
    x_len = rs.randint(600, T + 1, size=B).astype(np.int32)
    x0 = torch.from_numpy(xs).to(dev)
    xl = torch.from_numpy(x_len).to(dev)
    table = torch.from_numpy(gram).to(dev)
    valid_rows = int(x_len.sum())
    lib = _lib.lib()
    for N in [int(v) for v in a.n.split(",")]:
        ids, lens, scores = gram_beam_decode(x0, gram, N, 16, 0, xl)
        lens = torch.where(scores > float("-inf"), lens, torch.full_like(lens, -1))
        width = max(1, int(lens.max().item()))
        hyps = ids[:, :, :width].contiguous()
        gy = torch.from_numpy(rs.randn(B, N).astype(np.float32)).to(dev)
        # the baseline's labels, on the host: unigram token of every character, bigram token of every adjacent pair or -1
        hh, lh = hyps.cpu().numpy().reshape(B * N, width), lens.clamp_min(0).cpu().numpy().reshape(B * N)
        lu = np.zeros((B * N, width), np.int32)
        lb = np.full((B * N, width), -1, np.int32)
        for u in range(B * N):
            s = [int(c) for c in hh[u, :lh[u]]]
            lu[u, :lh[u]] = [uni[c] for c in s]
            lb[u, :lh[u]] = gref.label_bigrams(s, gram) if s else []
        lu_rep, lb_rep, len_rep = torch.from_numpy(lu).to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(lh.astype(np.int32)).to(dev)
        x = x0.clone().requires_grad_(True)
        x_rep = x0.repeat_interleave(N, dim=1).contiguous().requires_grad_(True)
        xl_rep, gy_rep = xl.repeat_interleave(N).contiguous(), (-gy).reshape(B * N).contiguous()
        out = {}

        def baseline():
            x_rep.grad = None
            loss = gram_ctc(x_rep, lu_rep, lb_rep, 0, xl_rep, len_rep, "no")
            loss.backward(gy_rep)
            out["base"] = x_rep.grad.view(T, B, N, V).sum(dim=2) if N > 1 else x_rep.grad
            out["base_logp"] = -loss.detach().reshape(B, N)

        def nbest():
            x.grad = None
            logp = gram_ctc_nbest_logp(x, hyps, lens, gram, 0, xl)      # the NumPy table: validated on the host, no synchronisation
            logp.backward(gy)
            out["new"], out["new_logp"] = x.grad, logp.detach()

        def nbest_checked_table():           # the autograd function on a table that is on the device already (how gram_mwer_loss scores)
            from asr.loss.nbest import _NbestFunction
            x.grad = None
            _NbestFunction.apply(x, hyps, lens, xl, 0, table).backward(gy)

        # the raw forward entry (no table validation on the host): whole, and at T = 1, where the three new kernels are nearly all of it
        nbytes = lib.asr_gram_ctc_nbest_workspace_bytes(T, B, V, N, width)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lp_out = torch.empty((B, N), dtype=torch.float32, device=dev)
        p, st = _lib.ptr, _lib.stream()

        def raw_forward(frames):
            def call():
                rc = lib.asr_gram_ctc_nbest_forward(st, p(x0), p(hyps), p(lens), p(xl), p(table), frames, B, V, N, width, 0, p(lp_out),
                                                    p(ws), nbytes)
                assert rc == 0, rc
            return call

        # node_frames: sum over the used slots of (3 len + 1) * x_len[b] -- the alpha / beta entries (8 B each) the gradient pass reads
        node_frames = int((torch.where(lens >= 0, 3 * lens + 1, torch.zeros_like(lens)).sum(dim=1).long() * xl.long()).sum().item())
        common = dict(B=B, T=T, V=V, N=N, Lmax=width, valid_rows=valid_rows, used_slots=int((lens >= 0).sum().item()),
                      node_frames=node_frames)
        ms = {}
        for op, fn in (("baseline", baseline), ("nbest", nbest), ("baseline_again", baseline), ("nbest_checked_table", nbest_checked_table),
                       ("nbest_forward_only", raw_forward(T)),
                       ("new_kernels", raw_forward(1))):
            ms[op] = timed(fn, a.warmup, a.iters)
            print(json.dumps(dict(op=op, ms=round(ms[op], 4), **common)), flush=True)
        spread = abs(ms["baseline"] - ms["baseline_again"])
        base = min(ms["baseline"], ms["baseline_again"])
        print(json.dumps(dict(op="ratio", nbest_over_baseline=round(ms["nbest"] / base, 4), baseline_spread_ms=round(spread, 4),
                              checked_table_over_baseline=round(ms["nbest_checked_table"] / base, 4),
                              new_kernels_upper_bound_ms=round(ms["new_kernels"], 4),
                              not_longer_than_baseline_plus_spread=bool(ms["nbest"] <= max(ms["baseline"], ms["baseline_again"]) + spread),
                              shorter_than_baseline=bool(ms["nbest"] < base), **common)))
        print(json.dumps(dict(op="workspace_bytes", nbest=nbytes, baseline_loss=lib.asr_ctc_workspace_bytes(T, B * N, V, width, 1),
                              baseline_logits_and_gradient=2 * 4 * T * B * N * V, **common)))
        dg = float((out["new"] - out["base"]).abs().max()) / float(out["base"].abs().max())
        dl = float(((out["new_logp"] - out["base_logp"]).abs() / out["base_logp"].abs()).max())
        print(json.dumps(dict(op="check", max_dgrad_over_max_grad=dg, max_rel_dlogp=dl, **common)), flush=True)
        del x_rep, out, ws


if __name__ == "__main__":
    main()
