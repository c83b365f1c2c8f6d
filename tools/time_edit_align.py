"""Time the edit-alignment kernels (csrc/edit_align.hip) on real N-best lists, in one process on one GPU.  Device events on the launch
stream, warm-up, then --iters timed calls of each; where two routes are compared the order is baseline, new, baseline again -- the
two baseline figures give that measurement's own run-to-run spread.

Inputs: B = 32, T = 1000, V = 3000, x_len ~ U{600..1000} (seed 4); logits = tests/ctc_beam_reference.py: peaky per utterance, seed 3;
lists = asr.error.beam_decode(x, 16, 16, lengths=x_len): ids (32, 16, 1000), for (a) and (b) cut to the longest hypothesis.

(a) asr_nbest_pairwise_distance on the (B, N, L) list against the route the project had before it for the same (B, N, N) matrix:
    repeat_interleave / repeat of the ids to B N N ordered pairs and one asr_edit_distance pair per copy.  The replication is NOT
    timed (it favours the baseline).  The two matrices are compared.
(b) asr_edit_align on those same B N N pairs with both maps and with both maps null, against asr_edit_distance.
(c) asr.error.mbr_decode end to end (posterior, distances, risk, pick, confidence) on the uncut list as beam_decode returns it, and
    on the cut one, beside the beam_decode that produced it.

One JSON line per measurement.  usage: python tools/time_edit_align.py [--iters 20] [--warmup 3]"""
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
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "chainer-speech-recognition_amd"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import ctc_beam_reference as beam_ref
    from asr import _lib, _ops
    from asr.error import beam_decode, mbr_decode
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    dev = torch.device("cuda:0")
    B, T, V, N = 32, 1000, 3000, 16
    rs = np.random.RandomState(3)
    xs = np.stack([beam_ref.peaky(rs, T, V) for _ in range(B)], axis=1).astype(np.float32)
    x_len = np.random.RandomState(4).randint(600, T + 1, size=B).astype(np.int32)
    x0, xl = torch.from_numpy(xs).to(dev), torch.from_numpy(x_len).to(dev)
    ids, lens, scores = beam_decode(x0, N, 16, 0, xl)
    used = int(torch.isfinite(scores).sum().item())
    width = max(1, int(lens.max().item()))
    cut = ids[:, :, :width].contiguous()
    klens = torch.where(torch.isfinite(scores), lens, torch.full_like(lens, -1)).contiguous()
    common = dict(B=B, N=N, L=width, used_slots=used, mean_length=round(float(lens.float().mean()), 1))

    def show(op, ms, **more):
        print(json.dumps(dict(op=op, ms=round(ms, 4), **more, **common)), flush=True)

    # ---- (a): the (B, N, N) matrix.  The replicated operands are made here, outside the timed region
    left = cut.repeat_interleave(N, dim=1).reshape(B * N * N, width).contiguous()
    right = cut.repeat(1, N, 1).reshape(B * N * N, width).contiguous()
    ll = klens.repeat_interleave(N, dim=1).reshape(-1).clamp_min(0).contiguous()
    rl = klens.repeat(1, N).reshape(-1).clamp_min(0).contiguous()
    out = {}

    def baseline():
        out["base"] = _ops.edit_distance(left, ll, right, rl)

    def pairwise():
        out["new"] = _ops.nbest_pairwise_distance(cut, klens)

    ms = {}
    for op, fn in (("a_baseline", baseline), ("a_pairwise", pairwise), ("a_baseline_again", baseline)):
        ms[op] = timed(fn, a.warmup, a.iters)
        show(op, ms[op], pairs=B * N * N if fn is baseline else B * N * (N - 1) // 2)
    spread = abs(ms["a_baseline"] - ms["a_baseline_again"])
    base = min(ms["a_baseline"], ms["a_baseline_again"])
    live = (klens >= 0)
    mask = (live[:, :, None] & live[:, None, :]).reshape(-1)
    same = bool(torch.equal(torch.where(mask, out["base"], torch.zeros_like(out["base"])).reshape(B, N, N), out["new"]))
    print(json.dumps(dict(op="a_ratio", pairwise_over_baseline=round(ms["a_pairwise"] / base, 4), baseline_spread_ms=round(spread, 4),
                          not_slower_than_baseline_plus_spread=bool(ms["a_pairwise"] <= max(ms["a_baseline"], ms["a_baseline_again"]) + spread),
                          matrices_equal=same, **common)), flush=True)

    # ---- (b): the path's price, on the same B N N pairs
    def align_paths():
        out["paths"] = _ops.edit_align(left, ll, right, rl, True)

    def align_counts():
        out["counts"] = _ops.edit_align(left, ll, right, rl, False)

    for op, fn in (("b_edit_distance", baseline), ("b_edit_align_paths", align_paths), ("b_edit_align_no_maps", align_counts),
                   ("b_edit_distance_again", baseline)):
        show(op, timed(fn, a.warmup, a.iters), pairs=B * N * N)
    ok = bool(torch.equal(out["paths"][0][:, 0], out["base"]) and torch.equal(out["counts"][0], out["paths"][0]))
    cells = int((ll.long() * rl.long()).sum().item())
    print(json.dumps(dict(op="b_check", distances_equal=ok, table_cells=cells, steps_walked_back=int((ll.long() + rl.long()).sum().item()),
                          workspace_bytes=_lib.lib().asr_edit_align_workspace_bytes(B * N * N, width, width), **common)), flush=True)

    # ---- (c): the whole decode
    def search():
        out["list"] = beam_decode(x0, N, 16, 0, xl)

    def mbr_uncut():
        out["mbr"] = mbr_decode(ids, lens, scores)

    def mbr_cut():
        out["mbr_cut"] = mbr_decode(cut, lens, scores)

    def mbr_no_conf():
        mbr_decode(cut, lens, scores, confidence=False)

    for op, fn in (("c_beam_decode", search), ("c_mbr_decode_uncut_L%d" % T, mbr_uncut), ("c_mbr_decode_cut", mbr_cut),
                   ("c_mbr_decode_cut_no_confidence", mbr_no_conf), ("c_beam_decode_again", search)):
        show(op, timed(fn, a.warmup, a.iters))
    m, c = out["mbr"], out["mbr_cut"]
    print(json.dumps(dict(op="c_check", cut_equals_uncut=bool(torch.equal(m.index, c.index) and torch.equal(m.confidence[:, :width], c.confidence)),
                          picks_other_than_slot_0=int((m.index > 0).sum().item()), mean_confidence=round(float(
                              (m.confidence.sum(dim=1) / m.lengths.clamp_min(1)).mean()), 4), **common)), flush=True)


if __name__ == "__main__":
    main()
