"""``ds2.Model(rnn="sru")`` end to end: one-shot forward and gradients, a train step, checkpoints, data parallelism and the stream.

The oracle is oracle.model.DS2Oracle's float32 forward with the recurrent stack swapped for the float64 restatement of the SRU sequence
layer (tests/sru_seq_reference.py, forward and analytic backward behind a torch.autograd.Function), the restated frame stacking and
lookahead layer where the model has them (as tests/test_time_reduction_gpu.py composes them).  The bar is the repository's rule for a
new layer in a measured model: E <= 2 E_gru, where E_gru is the relative L2 distance (valid frames; for gradients the worst parameter)
of the SAME model with rnn="gru" to its own oracle at the same sizes and seed, measured in the same run on the unchanged GRU path.
What an MI355X run measured is in DESIGN.md section 42."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lookahead_reference as lref
import sru_seq_reference as R
import time_stack_reference as ts

pytestmark = pytest.mark.gpu

V, B, T = 32, 3, 70
X_LEN = [70, 41, 9]
VARIANTS = {"forward": (False, 0, 1), "bidirectional": (True, 0, 1), "lookahead": (False, 3, 1), "reduced": (False, 0, 2)}


def _rel(got, want):
    """relative L2 over the valid frames of all slots"""
    a = torch.cat([g.double().flatten() for g in got])
    b = torch.cat([w.double().flatten() for w in want])
    assert bool(torch.isfinite(a).all())
    return float((a - b).norm() / b.norm())


def _valid(tbv, lens):
    return [tbv[:n, b] for b, n in enumerate(lens)]


def _stack(h, k, x_len):
    """tests/time_stack_reference.py::fwd in differentiable torch: h (T, B, R) -> ((G, B, k * R), lengths)"""
    Tn, Bn, R_ = h.shape
    G = -(-Tn // k)
    n = torch.full((Bn,), Tn, dtype=torch.long) if x_len is None else x_len.long().clamp(0, Tn)
    live = (torch.arange(Tn).reshape(Tn, 1) < n.reshape(1, Bn)).unsqueeze(2)
    z = torch.where(live, h, torch.zeros_like(h))
    z = torch.cat([z, torch.zeros(G * k - Tn, Bn, R_)]).reshape(G, k, Bn, R_)
    y = z.permute(0, 2, 1, 3).reshape(G, Bn, k * R_)
    want, want_len = ts.fwd(h.detach().numpy(), k, None if x_len is None else x_len.numpy())
    assert np.array_equal(y.detach().numpy(), want) and np.array_equal(((n + k - 1) // k).numpy(), want_len)
    return y, ((n + k - 1) // k).to(torch.int32)


def _schedule(kind, lens, seed=0):
    """the input frames per slot of every call.  "whole": one chunk; "single": 1-frame chunks; "ragged": every slot a different
    number per call, some of them 0"""
    rng = np.random.default_rng(seed)
    left = np.array(lens)
    calls, turn = [], 0
    while left.sum() > 0:
        turn += 1
        if kind == "whole":
            n = left.copy()
        elif kind == "single":
            n = np.minimum(left, 1)
        else:
            n = np.minimum(left, rng.integers(0, 8, size=len(lens)))
            n[turn % len(lens)] = 0
            if n.sum() == 0:
                continue
        calls.append(n)
        left = left - n
    return calls


def _feed(stream, x, calls, start=None, each=None, Tc_of=None):
    """run `calls` (per call: input frames per slot, taken from x (B, C, H, T) at every slot's own position) -> per call
    (logits, lengths, n).  Rows of a chunk beyond a slot's share hold 9.0, which nothing may read."""
    k = stream.k
    pos = np.zeros(x.shape[0], dtype=np.int64) if start is None else np.array(start)
    out = []
    for i, n in enumerate(calls):
        Tc = int(n.max()) if Tc_of is None else Tc_of[i]
        chunk = torch.full(tuple(x.shape[:3]) + (Tc,), 9.0)
        for b, nb in enumerate(n):
            chunk[b, :, :, :nb] = x[b, :, :, pos[b]:pos[b] + nb]
        pos += n
        logits, lengths = stream.advance(chunk.to(stream.device), n.astype(np.int32))
        assert tuple(logits.shape) == ((k - 1 + Tc + k - 1) // k, x.shape[0], V) and logits.dtype == torch.float32
        assert lengths.dtype == torch.int32
        if each is not None:
            each(logits, lengths)
        out.append((logits, lengths, n))
    return out


def _per_slot(outs):
    """the valid rows of every call, concatenated per slot"""
    nslots = outs[0][0].shape[1]
    lens = [o[1].cpu().tolist() for o in outs]
    return [torch.cat([o[0][:l[b], b] for o, l in zip(outs, lens)]).cpu() for b in range(nslots)]


def _build(device, rnn, bidirectional, lookahead=0, k=1, seed=0):
    from asr.model import ds2
    torch.manual_seed(seed)
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers, cfg.bidirectional = V, 16, 64, 32, 2, bidirectional
    cfg.lookahead, cfg.time_reduction, cfg.rnn = lookahead, k, rnn
    model = ds2.Model(cfg)
    model.to_gpu()
    if lookahead:
        with torch.no_grad():
            model.lookahead.W.copy_(torch.randn(model.lookahead.W.shape) * 0.4)
    return cfg, model


class _SRULayer(torch.autograd.Function):
    """tests/sru_seq_reference.py as a differentiable layer: h (T, B, I) -> (T, B, D)"""

    @staticmethod
    def forward(ctx, h, W, Bias, x_len):
        ctx.save_for_backward(h, W, Bias)
        ctx.x_len = x_len
        y, _, _ = R.layer_fwd(h.numpy(), W.numpy(), Bias.numpy(), None, x_len)
        return torch.from_numpy(y).float()

    @staticmethod
    def backward(ctx, gy):
        h, W, Bias = ctx.saved_tensors
        gx, gW, gb, _ = R.layer_bwd(h.numpy(), W.numpy(), Bias.numpy(), None, ctx.x_len, gy.numpy())
        return torch.from_numpy(gx).float(), torch.from_numpy(gW).float(), torch.from_numpy(gb).float(), None


class _LookaheadLayer(torch.autograd.Function):
    """tests/lookahead_reference.py as a differentiable layer: h (T, B, D), W (D, tau + 1) -> (T, B, D)"""

    @staticmethod
    def forward(ctx, h, W, x_len):
        ctx.save_for_backward(h, W)
        ctx.x_len = x_len
        return torch.from_numpy(lref.forward(h.numpy(), W.numpy(), x_len)).float()

    @staticmethod
    def backward(ctx, gy):
        h, W = ctx.saved_tensors
        dx, dW = lref.backward(gy.numpy(), h.numpy(), W.numpy(), ctx.x_len)
        return torch.from_numpy(dx).float(), torch.from_numpy(dW).float(), None


def _oracle(state, cfg):
    from oracle import model as omodel
    from oracle import nn as onn
    from oracle import bf16 as Q
    k = cfg.time_reduction

    class Oracle(omodel.DS2Oracle):
        def forward(self, x, x_len=None):
            h = x
            for i, pool in enumerate([3] + [2] * (self.nconv - 1)):
                W, b = self.g("conv_blocks._sequential_%d.W" % (4 * i)), self.g("conv_blocks._sequential_%d.b" % (4 * i))
                h = onn.maxpool_h(onn.maxout2(onn.conv2d_causal(h, W, b, 0)), pool)
            Bn, C, H, Tn = h.shape
            h = h.permute(3, 0, 2, 1).reshape(Tn, Bn, H * C)
            if k > 1:
                h, x_len = _stack(h, k, x_len)
                Tn = h.shape[0]
            for i in range(self.nrnn):
                pre = "rnn_blocks._sequential_%d." % (2 * i)
                if cfg.rnn == "sru":
                    h = _SRULayer.apply(h, self.g(pre + "W"), self.g(pre + "B"), None if x_len is None else x_len.numpy())
                else:
                    h = Q.gru(h, *(self.g(pre + n) for n in ("w_ih", "w_hh", "b_ih", "b_hh")), x_len, False, False, None, False)
            if "lookahead__W" in self.p:
                h = _LookaheadLayer.apply(h, self.g("lookahead.W"), None if x_len is None else x_len.numpy())
            for idx in (0, 3):
                W, b = self.g("dense_blocks._sequential_%d.W" % idx), self.g("dense_blocks._sequential_%d.b" % idx)
                h = Q.linear(h, W[:, :, 0], b, False)
                h = h.reshape(Tn, Bn, -1, 2).max(dim=3)[0]
            W, b = self.g("dense_blocks._sequential_6.W"), self.g("dense_blocks._sequential_6.b")
            h = Q.linear(h, W[:, :, 0], b, False, f32_out=True)
            return Q.layer_norm_rows(h, self.g("dense_blocks._sequential_7.norm.gamma"), self.g("dense_blocks._sequential_7.norm.beta"))

    return Oracle(state, cfg.num_conv_layers, cfg.num_rnn_layers, bidirectional=cfg.bidirectional, matched=False)


def _batch():
    from oracle import model as omodel
    x, labels, _, l_len = omodel.synthetic_batch(B, T, V, Lmin=3, Lmax=9, seed=0, ragged=True)
    return x, labels, l_len


def _labels(k):
    """the synthetic transcripts cut against the frames the loss will see"""
    from asr.data.processing import truncate_labels_for_ctc
    _, labels, l_len = _batch()
    labels, l_len = labels.clone(), l_len.clone()
    for b, n in enumerate(X_LEN):
        ids = labels[b, :l_len[b]].tolist()
        keep = len(truncate_labels_for_ctc(ids, ids, -(-n // k))[0])
        labels[b, keep:] = 0
        l_len[b] = keep
    return labels, l_len


_CACHE = {}


def _setup(device, rnn, variant):
    """model, its one-shot logits, the oracle's, their distance E and the parameter-gradient distances -- once per (cell, variant)"""
    key = (rnn, variant)
    if key not in _CACHE:
        from asr.functions import join_side_stream
        from asr.loss import connectionist_temporal_classification
        from oracle import model as omodel
        bidirectional, tau, k = VARIANTS[variant]
        cfg, model = _build(device, rnn, bidirectional, tau, k)
        x = _batch()[0]
        x_len = torch.tensor(X_LEN, dtype=torch.int32)
        out_len = [-(-n // k) for n in X_LEN]
        with torch.no_grad():
            one = model(x.to(device), split_into_variables=False, x_length=x_len.to(device)).float().cpu()
        assert tuple(one.shape) == (B, -(-T // k), V) and model.output_length(X_LEN) == out_len
        state = {name: v.detach().cpu() for name, v in model.state_dict().items()}
        ref = _oracle(state, cfg)
        with torch.no_grad():
            want = _valid(ref(x, x_len).detach(), out_len)
        one = [one[b, :n] for b, n in enumerate(out_len)]
        s = dict(cfg=cfg, model=model, state=state, x=x, x_len=x_len, out_len=out_len, one=one, want=want, E=_rel(one, want))
        labels, l_len = _labels(k)
        olen = torch.tensor(out_len, dtype=torch.int32)
        ys = model(x.to(device), x_length=x_len.to(device))
        loss = connectionist_temporal_classification(ys, labels.to(device), 0, olen.to(device), l_len.to(device))
        loss.backward()
        join_side_stream()
        torch.cuda.synchronize()
        loss_ref = omodel.ctc_mean_loss(ref(x, x_len), labels, olen, l_len)
        loss_ref.backward()
        errs = {}
        for name, p in model.named_parameters():
            g, gr = p.grad.detach().cpu().double(), ref.g(name).grad.double()
            assert bool(torch.isfinite(g).all()), name
            errs[name] = float((g - gr).norm() / gr.norm())
        s.update(errs=errs, loss=loss.item(), loss_ref=loss_ref.item())
        for p in model.parameters():
            p.grad = None
        _CACHE[key] = s
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ one-shot forward and gradients
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_logits_and_gradients_against_the_restatement(device, variant):
    g, s = _setup(device, "gru", variant), _setup(device, "sru", variant)
    worst, worst_g = max(s["errs"], key=s["errs"].get), max(g["errs"], key=g["errs"].get)
    first = "rnn_blocks._sequential_0.W"
    line = "ds2 rnn=sru %s: logits E %.4e (gru: %.4e)  loss %.5f (oracle %.5f)  worst gradient %.4e (%s; gru: %.4e, %s)  first W %.4e" % (
        variant, s["E"], g["E"], s["loss"], s["loss_ref"], s["errs"][worst], worst, g["errs"][worst_g], worst_g, s["errs"][first])
    if "lookahead.W" in s["errs"]:
        line += "  lookahead.W %.4e (gru: %.4e)" % (s["errs"]["lookahead.W"], g["errs"]["lookahead.W"])
    print(line)
    assert s["E"] <= 2 * g["E"], (s["E"], g["E"])
    assert abs(s["loss"] - s["loss_ref"]) <= 3e-2 * abs(s["loss_ref"])              # (the float32-oracle bar of smoke())
    assert s["errs"][worst] <= 2 * g["errs"][worst_g], (worst, s["errs"][worst], g["errs"][worst_g])


def test_without_lengths_the_padded_block_runs(device):
    s = _setup(device, "sru", "bidirectional")
    with torch.no_grad():
        whole = s["model"](s["x"].to(device), split_into_variables=False).float().cpu()
        want = _oracle(s["state"], s["cfg"])(s["x"], None).detach()
    e = _rel([whole[b] for b in range(B)], [want[:, b] for b in range(B)])
    assert e <= 2 * _setup(device, "gru", "bidirectional")["E"], e


def test_one_train_step(device):
    from asr.loss import connectionist_temporal_classification
    from asr.optimizers import Adam, GradientClipping, WeightDecay
    _, model = _build(device, "sru", True, seed=3)
    model.rnn_blocks.layers[1].ratio = 0.0
    x, labels, l_len = _batch()
    x_len = torch.tensor(X_LEN, dtype=torch.int32, device=device)
    opt = Adam(1e-3, 0.9)
    opt.setup(model)
    opt.add_hook(GradientClipping(1.0))
    opt.add_hook(WeightDecay(1e-5))
    labels, l_len = _labels(1)
    ys = model(x.to(device), x_length=x_len)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss = connectionist_temporal_classification(ys, labels.to(device), 0, x_len, l_len.to(device))
    opt.update(lossfun=lambda: loss)
    loss2 = connectionist_temporal_classification(model(x.to(device), x_length=x_len), labels.to(device), 0, x_len, l_len.to(device))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and torch.isfinite(loss2).item() and opt.applied_steps() == 1
    for n, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[n]), n


# ------------------------------------------------------------------------------------------------ checkpoints
def test_round_trip_and_cross_refusals(device, tmp_path):
    s = _setup(device, "sru", "reduced")
    model, x, x_len = s["model"], s["x"].to(device), s["x_len"].to(device)
    for name in ("model.hdf5", "model.npz"):
        path = str(tmp_path / name)
        model.save(path)
        _, fresh = _build(device, "sru", False, 0, 2, seed=7)
        assert fresh.load(path)
        assert list(fresh.state_dict().keys()) == list(model.state_dict().keys())
        for key, value in model.state_dict().items():
            assert torch.equal(fresh.state_dict()[key], value), key
        with torch.no_grad():
            again = fresh(x, split_into_variables=False, x_length=x_len).float().cpu()
        assert all(torch.equal(again[b, :n], s["one"][b]) for b, n in enumerate(s["out_len"]))
        _, other = _build(device, "gru", False, 0, 2, seed=7)
        with pytest.raises(KeyError):
            other.load(path)                                    # an "sru" checkpoint into a "gru" model
    g = _setup(device, "gru", "reduced")
    path = str(tmp_path / "gru.npz")
    g["model"].save(path)
    _, fresh = _build(device, "sru", False, 0, 2, seed=7)
    with pytest.raises(KeyError):
        fresh.load(path)                                        # and the reverse


# ------------------------------------------------------------------------------------------------ two ranks == one rank
def test_two_ranks_reproduce_one_rank_on_the_whole_batch(tmp_path):
    """tests/test_parallel_gpu.py's identity (two gloo ranks on one device, half a batch each, against one rank on the whole batch),
    restated for rnn="sru" with momentum SGD, which is linear in the clipped mean gradient: a wrong bucket order or a slice summed
    before its gradient was written is an O(1) error in the parameters' movement"""
    import test_parallel_gpu as tp
    script = tp.DP_SCRIPT.replace("cfg.num_rnn_layers = V, 16, 128, 32, 2", "cfg.num_rnn_layers = V, 16, 128, 32, 2; cfg.rnn = \"sru\"")
    assert script != tp.DP_SCRIPT
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def spawn(world, port):
        procs, outs = [], []
        for r in range(world):
            out = str(tmp_path / ("sru_w%d_r%d.pt" % (world, r)))
            env = dict(os.environ, ASR_ROOT=root, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE=str(world),
                       LOCAL_RANK="0", ASR_TEST_BACKEND="gloo")
            procs.append(subprocess.Popen([sys.executable, "-c", script, "ds2", "msgd", out], env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.PIPE, text=True))
            outs.append(out)
        for p in procs:
            _, se = p.communicate(timeout=600)
            assert p.returncode == 0, se[-3000:]
        return [torch.load(o) for o in outs]
    one = spawn(1, 29671)[0]
    two = spawn(2, 29672)
    assert torch.equal(two[0]["start"], two[1]["start"]) and torch.equal(two[0]["start"], one["start"])
    assert torch.equal(two[0]["end"], two[1]["end"]), "ranks diverged"
    assert one["applied"] == 3 and two[0]["applied"] == 3
    for s in range(3):
        mean2 = 0.5 * (two[0]["losses"][s] + two[1]["losses"][s])
        assert abs(mean2 - one["losses"][s]) <= 2e-3 * abs(one["losses"][s]), (s, mean2, one["losses"][s])
        assert abs(two[0]["norms"][s] - one["norms"][s]) <= 2e-2 * one["norms"][s], (s, two[0]["norms"][s], one["norms"][s])
    moved1, moved2 = one["end"] - one["start"], two[0]["end"] - two[0]["start"]
    rel = float((moved2 - moved1).norm() / moved1.norm())
    print("two ranks against one, rnn=sru, msgd: the parameters' movement differs by %.3e" % rel)
    assert rel < 0.03, rel
    ks = [k for k, _ in two[0]["launches"]]
    assert sorted(ks) == list(range(len(ks)))


# ------------------------------------------------------------------------------------------------ the stream
@pytest.mark.parametrize("variant", ["forward", "lookahead", "reduced"])
def test_stream_against_the_restatement(device, variant):
    """any cuts, then flush: exactly output_length(x_len) frames per slot, as close to the restatement as the one-shot forward (bar:
    twice the one-shot distance); a stream that forgets c between chunks misses that bar by the printed factor"""
    from asr.model.stream import AcousticStream
    _, tau, k = VARIANTS[variant]
    s = _setup(device, "sru", variant)
    out_len, E = s["out_len"], s["E"]
    got, Es = {}, {}
    for kind in ("whole", "single", "ragged"):
        st = AcousticStream(s["model"], B, max_chunk=T)
        assert st.delay == tau and st.k == k and [h.shape for h in st._h] == [(1, B, 64)] * 2 and st._h[0].dtype == torch.float32
        outs = _feed(st, s["x"], _schedule(kind, X_LEN))
        tail = st.flush()
        assert st.frames.cpu().tolist() == out_len
        got[kind] = _per_slot(outs + [tail + (None,)])
        assert [g.shape[0] for g in got[kind]] == out_len
        Es[kind] = _rel(got[kind], s["want"])
        assert all(bool((h == 0).all()) for h in st._h)                 # flush reset the carried states
    st = AcousticStream(s["model"], B, max_chunk=T)
    calls = _schedule("ragged", X_LEN)
    outs = []
    for i, n in enumerate(calls):                                         # the same frames, c forgotten between the chunks
        outs += _feed(st, s["x"], [n], start=np.sum(calls[:i], axis=0).astype(np.int64) if i else None)
        for h in st._h:
            h.zero_()
    lost = _per_slot(outs + [st.flush() + (None,)])
    assert [g.shape[0] for g in lost] == out_len
    bad = _rel(lost, s["want"])
    diff = max(float((a - b).abs().max()) for kind in ("single", "ragged") for a, b in zip(got["whole"], got[kind]))
    print("sru stream %s: one-shot %.4e  whole %.4e single %.4e ragged %.4e  c forgotten %.4e (%.1f bars)  | schedules differ by at most %.3e"
          % (variant, E, Es["whole"], Es["single"], Es["ragged"], bad, bad / (2 * E), diff))
    for kind in Es:
        assert Es[kind] <= 2 * E, (kind, Es[kind], E)
    assert bad > 2 * E, "the bar cannot tell a stream that forgets its state from one that carries it"


def test_a_chunk_costs_the_same_launches_whatever_its_length(device):
    """the SRU layers of a chunk are one projection and one scan each: chunks of 8 and of 31 frames launch the same kernels, one scan
    launch per layer; from 32 frames on a scan is a summary and an apply launch, two per layer, at 32 frames as at the 64 that
    tools/time_sru_stack.py times -- a fixed number either way, never one per frame"""
    from asr.model.stream import AcousticStream
    from torch.profiler import ProfilerActivity, profile
    s = _setup(device, "sru", "forward")
    st = AcousticStream(s["model"], B, max_chunk=T)
    counts = []
    for Tc in (8, 31, 8, 31, 32, 64):
        chunk = s["x"][:, :, :, :Tc].to(device)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            st.advance(chunk)
            torch.cuda.synchronize()
        counts.append(sum(1 for e in prof.events() if "sruseq" in e.name))
    print("sru_seq kernels per chunk of 8 / 31 / 8 / 31 / 32 / 64 frames:", counts)
    assert counts[:4] == [2, 2, 2, 2]           # two layers, one scan launch each (T < 32: no summary pass)
    assert counts[4:] == [4, 4]                 # two layers, summary + apply each


def test_slots_restart_on_bits_and_the_decoders_take_the_output(device):
    """slot 1 ends (flush) and starts its utterance again while the others go on: the second pass equals the first on bits; every
    (logits, lengths) goes unchanged into a BeamStream and a KeywordStream, which equal the one-shot searches on bits"""
    from asr import error, spot
    from asr.model.stream import AcousticStream
    s = _setup(device, "sru", "lookahead")
    x, out_len = s["x"], s["out_len"]
    st = AcousticStream(s["model"], B, max_chunk=64)
    only1 = [np.array([0, n, 0]) for n in (7, 20, 14)]
    first = _feed(st, x, only1, Tc_of=[7, 20, 14])
    tail1 = st.flush([0, 1, 0])
    a = _per_slot(first + [tail1 + (None,)])[1]
    assert a.shape[0] == 41 == st.frames.cpu().tolist()[1]
    kws = spot.KeywordSet([(3, 4), (5,), (7, 8, 9), (2, 2)], V)
    beam = error.BeamStream(B, V, max_frames=256, beam_width=8, top_k=8)
    spotter = spot.KeywordStream(B, V, kws, device)
    dets = []

    def each(logits, lengths):
        beam.advance(logits, lengths)
        dets.append((spotter.advance(logits, lengths), lengths.cpu().tolist()))
    outs = _feed(st, x, _schedule("ragged", X_LEN, seed=2), each=each)
    tail = st.flush()
    each(*tail)
    got = _per_slot(outs + [tail + (None,)])
    assert [g.shape[0] for g in got] == out_len and torch.equal(got[1], a)
    cat = torch.zeros((T, B, V))
    for slot, g in enumerate(got):
        cat[:g.shape[0], slot] = g
    cat, lens = cat.to(device), torch.tensor(out_len, dtype=torch.int32, device=device)
    ids, n, scores = error.beam_decode(cat, beam_width=8, top_k=8, lengths=lens)
    sids, sn, sscores = beam.result()
    assert torch.equal(sn, n) and torch.equal(sscores, scores)
    w = min(T, sids.shape[2])
    assert torch.equal(sids[:, :, :w], ids[:, :, :w]) and bool((sids[:, :, w:] == 0).all()) and bool((ids[:, :, w:] == 0).all())
    K = len(kws.phrases)
    score = torch.full((B, K, T), float("-inf"), device=device)
    start = torch.full((B, K, T), -1, dtype=torch.int32, device=device)
    fill = torch.zeros((B, T), device=device)
    pos = [0] * B
    for det, lengths in dets:
        for slot, nb in enumerate(lengths):
            score[slot, :, pos[slot]:pos[slot] + nb] = det.score[slot, :, :nb]
            start[slot, :, pos[slot]:pos[slot] + nb] = det.start[slot, :, :nb]
            fill[slot, pos[slot]:pos[slot] + nb] = det.fill[slot, :nb]
            pos[slot] += nb
    assert pos == out_len
    want = spot.keyword_search(cat, kws, lens)
    have = spot.keyword_hits(spot.Detection(score, start, fill), lens)
    for w_, h_ in zip(want, have):
        assert torch.equal(w_, h_)


def test_a_bidirectional_sru_model_is_refused_by_the_stream(device):
    from asr.model.stream import AcousticStream
    with pytest.raises(ValueError, match="bidirectional"):
        AcousticStream(_setup(device, "sru", "bidirectional")["model"], B)
