"""``time_reduction`` = k of ds2.Model and of asr.model.stream.AcousticStream, end to end against the float32 oracle.

The oracle is oracle.model.DS2Oracle with the restated frame stacking (tests/time_stack_reference.py) between the conv stack and
the first GRU, and the restated lookahead layer (tests/lookahead_reference.py) where tau > 0.  The bar is E <= 2 E1, as in
tests/test_acoustic_stream_gpu.py: E1 is the relative L2 distance over the valid output frames between the k = 1 model's one-shot
forward and the oracle at the same sizes and seed, measured at run time -- code that time reduction does not touch.  Stacking
adds no arithmetic, so the k > 1 error is a second draw from the same distribution; frames stacked in the wrong order, groups
that start one frame off or a pending frame that is dropped are errors of order 1, and the tests show that the bar tells them.
The gradients are held to the same rule: 2 x the k = 1 model's worst parameter-gradient distance, measured in the same run.
A run on an MI355X (bf16), forward-only tau = 0: E1 = 4.057e-3; k = 2: one-shot 5.386e-3, stream 5.297e-3 under each of the three
schedules (the same bits), 3.9e-1 with the groups reversed or one frame late, 6.7e-1 with resets; k = 3: 4.775e-3, 4.663e-3,
2.9e-1 .. 3.2e-1, 6.2e-1.  tau = 3: E1 = 4.321e-3; k = 2: 6.355e-3 / 6.144e-3; k = 3: 5.011e-3 / 4.831e-3.  Bidirectional:
E1 = 5.095e-3; k = 2: 4.831e-3; k = 3: 5.481e-3.
"""
import numpy as np
import pytest
import torch

import lookahead_reference as lref
import time_stack_reference as ts

pytestmark = pytest.mark.gpu

V, B, T = 32, 4, 41
X_LEN = [41, 29, 5, 36]                    # slot 2 is shorter than most chunks


def _reduced(lens, k):
    return [-(-int(n) // k) for n in lens]


def _build(device, k, bidirectional=False, lookahead=0, seed=0):
    from asr.model import ds2
    torch.manual_seed(seed)
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers, cfg.bidirectional = V, 16, 64, 32, 2, bidirectional
    cfg.lookahead, cfg.time_reduction = lookahead, k
    model = ds2.Model(cfg)
    model.to_gpu()
    if lookahead:
        with torch.no_grad():               # (a fresh lookahead layer is the identity: give every tap something to do)
            model.lookahead.W.copy_(torch.randn(model.lookahead.W.shape) * 0.4)
    return cfg, model


def _stack(h, k, x_len, variant=None):
    """tests/time_stack_reference.py::fwd in differentiable torch: h (T, B, R) -> ((G, B, k * R), lengths).  variant "reversed":
    the frames of every group in reverse order; "shifted": every group starts one frame late -- the two ways to get it wrong"""
    Tn, Bn, R = h.shape
    G = -(-Tn // k)
    n = torch.full((Bn,), Tn, dtype=torch.long) if x_len is None else x_len.long().clamp(0, Tn)
    live = (torch.arange(Tn).reshape(Tn, 1) < n.reshape(1, Bn)).unsqueeze(2)
    z = torch.where(live, h, torch.zeros_like(h))
    if variant == "shifted":
        z = torch.cat([z[1:], torch.zeros(1, Bn, R)])
    z = torch.cat([z, torch.zeros(G * k - Tn, Bn, R)]).reshape(G, k, Bn, R)
    if variant == "reversed":
        z = z.flip(1)
    y = z.permute(0, 2, 1, 3).reshape(G, Bn, k * R)
    if variant is None:
        want, want_len = ts.fwd(h.detach().numpy(), k, None if x_len is None else x_len.numpy())
        assert np.array_equal(y.detach().numpy(), want) and np.array_equal(((n + k - 1) // k).numpy(), want_len)
    return y, ((n + k - 1) // k).to(torch.int32)


def _oracle(state, cfg, variant=None):
    """DS2Oracle (float32) with the restated stacking in front of the GRUs and the restated lookahead layer behind them"""
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
                h, x_len = _stack(h, k, x_len, variant)
                Tn = h.shape[0]
            for i in range(self.nrnn):
                pre = "rnn_blocks._sequential_%d." % (2 * i)
                h = Q.gru(h, *(self.g(pre + n) for n in ("w_ih", "w_hh", "b_ih", "b_hh")), x_len, False, False, None, False)
            if "lookahead__W" in self.p:
                h = torch.from_numpy(lref.forward(h.detach().numpy(), self.g("lookahead.W").detach().numpy(),
                                                  None if x_len is None else x_len.numpy())).float()
            for idx in (0, 3):
                W, b = self.g("dense_blocks._sequential_%d.W" % idx), self.g("dense_blocks._sequential_%d.b" % idx)
                h = Q.linear(h, W[:, :, 0], b, False)
                h = h.reshape(Tn, Bn, -1, 2).max(dim=3)[0]
            W, b = self.g("dense_blocks._sequential_6.W"), self.g("dense_blocks._sequential_6.b")
            h = Q.linear(h, W[:, :, 0], b, False, f32_out=True)
            return Q.layer_norm_rows(h, self.g("dense_blocks._sequential_7.norm.gamma"), self.g("dense_blocks._sequential_7.norm.beta"))

    return Oracle(state, cfg.num_conv_layers, cfg.num_rnn_layers, bidirectional=cfg.bidirectional, matched=False)


def _rel(got, want):
    """relative L2 over the valid frames of all slots"""
    a = torch.cat([g.double().flatten() for g in got])
    b = torch.cat([w.double().flatten() for w in want])
    assert bool(torch.isfinite(a).all())
    return float((a - b).norm() / b.norm())


def _valid(tbv, lens):
    return [tbv[:n, b] for b, n in enumerate(lens)]


_CACHE = {}


def _setup(device, k, bidirectional=False, lookahead=0):
    """model, input, its one-shot logits, the oracle's logits (valid frames per slot) and their distance E -- once per case"""
    key = (k, bidirectional, lookahead)
    if key not in _CACHE:
        from oracle import model as omodel
        cfg, model = _build(device, k, bidirectional, lookahead)
        x = omodel.synthetic_batch(B, T, V, Lmin=3, Lmax=9, seed=0, ragged=True)[0]
        x_len = torch.tensor(X_LEN, dtype=torch.int32)
        out_len = _reduced(X_LEN, k)
        with torch.no_grad():
            one = model(x.to(device), split_into_variables=False, x_length=x_len.to(device)).float().cpu()      # (B, T', V)
        assert tuple(one.shape) == (B, -(-T // k), V) and model.output_length(X_LEN) == out_len and model.time_reduction == k
        state = {name: v.detach().cpu() for name, v in model.state_dict().items()}
        ref = _oracle(state, cfg)
        with torch.no_grad():
            want = ref(x, x_len).detach()                                                                       # (T', B, V)
        if k == 1 and lookahead == 0:                                           # the restated forward is DS2Oracle's
            plain = omodel.DS2Oracle(state, cfg.num_conv_layers, cfg.num_rnn_layers, bidirectional=bidirectional, matched=False)
            assert _rel(_valid(want, out_len), _valid(plain(x, x_len).detach(), out_len)) == 0.0
        want = _valid(want, out_len)
        one = [one[b, :n] for b, n in enumerate(out_len)]
        _CACHE[key] = dict(cfg=cfg, model=model, state=state, x=x, x_len=x_len, out_len=out_len, one=one, want=want, E=_rel(one, want))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ one-shot forward
@pytest.mark.parametrize("bidirectional,lookahead", [(False, 0), (False, 3), (True, 0)])
@pytest.mark.parametrize("k", [2, 3])
def test_one_shot_forward_against_the_float32_oracle(device, k, bidirectional, lookahead):
    """(1), (2): the reverse direction of a bidirectional model starts in the zero-completed last group"""
    E1 = _setup(device, 1, bidirectional, lookahead)["E"]
    s = _setup(device, k, bidirectional, lookahead)
    wrong = {}
    for variant in ("reversed", "shifted"):
        with torch.no_grad():
            wrong[variant] = _rel(s["one"], _valid(_oracle(s["state"], s["cfg"], variant)(s["x"], s["x_len"]).detach(), s["out_len"]))
    print("time reduction k=%d bidirectional=%s tau=%d: E1 %.4e  E %.4e  | frames of a group reversed %.4e  groups one frame late %.4e"
          % (k, bidirectional, lookahead, E1, s["E"], wrong["reversed"], wrong["shifted"]))
    assert s["E"] <= 2 * E1, (s["E"], E1)
    for variant, e in wrong.items():
        assert e > 10 * 2 * E1, "the bar cannot tell %s stacking from the right one: %.3e against %.3e" % (variant, e, 2 * E1)


def test_without_lengths_the_padded_block_is_stacked(device):
    """x_length None: the block as it is; the model hands back ceil(T / k) steps per time step or as (B, T', V)"""
    s = _setup(device, 3)
    with torch.no_grad():
        ys = s["model"](s["x"].to(device))
        whole = s["model"](s["x"].to(device), split_into_variables=False)
    assert len(ys) == 14 and tuple(ys[0].shape) == (B, V) and tuple(whole.shape) == (B, 14, V)
    with torch.no_grad():
        want = _oracle(s["state"], s["cfg"])(s["x"], None).detach()
    e = _rel([whole[b].float().cpu() for b in range(B)], [want[:, b] for b in range(B)])
    assert e <= 2 * _setup(device, 1)["E"], e


# ------------------------------------------------------------------------------------------------------------ gradients
def _labels(k):
    """the synthetic transcripts, cut as the data side cuts them: against the frames the loss will see"""
    from asr.data.processing import truncate_labels_for_ctc
    from oracle import model as omodel
    labels, l_len = omodel.synthetic_batch(B, T, V, Lmin=3, Lmax=9, seed=0, ragged=True)[1::2]
    labels, l_len = labels.clone(), l_len.clone()
    for b, n in enumerate(_reduced(X_LEN, k)):
        ids = labels[b, :l_len[b]].tolist()
        keep = len(truncate_labels_for_ctc(ids, ids, n)[0])
        labels[b, keep:] = 0
        l_len[b] = keep
    return labels, l_len


_GRADS = {}


def _gradient_errors(device, k, bidirectional):
    """{parameter: relative L2 of its CTC gradient against the oracle's autograd}"""
    if (k, bidirectional) not in _GRADS:
        from asr.functions import join_side_stream
        from asr.loss import connectionist_temporal_classification
        from oracle import model as omodel
        s = _setup(device, k, bidirectional)
        model, x_len = s["model"], s["x_len"]
        labels, l_len = _labels(k)
        out_len = model.output_length(x_len)
        assert out_len.dtype == torch.int32 and out_len.tolist() == s["out_len"]
        for p in model.parameters():
            p.grad = None
        ys = model(s["x"].to(device), x_length=x_len.to(device))
        loss = connectionist_temporal_classification(ys, labels.to(device), 0, out_len.to(device), l_len.to(device))
        loss.backward()
        join_side_stream()
        torch.cuda.synchronize()
        ref = _oracle(s["state"], s["cfg"])
        loss_ref = omodel.ctc_mean_loss(ref(s["x"], x_len), labels, out_len, l_len)
        loss_ref.backward()
        errs, model_grad = {}, {}
        for name, p in model.named_parameters():
            g, gr = p.grad.detach().cpu().double(), ref.g(name).grad.double()
            assert bool(torch.isfinite(g).all()), name
            errs[name], model_grad[name] = float((g - gr).norm() / gr.norm()), g
        wrong = {}
        first = "rnn_blocks._sequential_0.w_ih"
        for variant in (("reversed", "shifted") if k > 1 else ()):               # the same gradient against a wrongly stacked oracle
            bad = _oracle(s["state"], s["cfg"], variant)
            omodel.ctc_mean_loss(bad(s["x"], x_len), labels, out_len, l_len).backward()
            g, gr = model_grad[first], bad.g(first).grad.double()
            wrong[variant] = float((g - gr).norm() / gr.norm())
        _GRADS[(k, bidirectional)] = (errs, loss.item(), loss_ref.item(), l_len.tolist(), wrong)
        for p in model.parameters():
            p.grad = None
    return _GRADS[(k, bidirectional)]


@pytest.mark.parametrize("bidirectional", [False, True])
@pytest.mark.parametrize("k", [2, 3])
def test_gradients_against_the_oracles_autograd(device, k, bidirectional):
    """(3) CTC on output_length(x_len) frames, labels cut against them.  The bar is 2 x the worst parameter-gradient distance of the
    k = 1 model in the same run.  The first recurrent layer's w_ih sees the stacked columns and is held to that bar on its own,
    and the bar can tell: against an oracle that stacks the frames of a group in reverse, or one frame late, the same gradient
    misses it.  (w_ih's own k = 1 distance is no yardstick for it: its gradient is the sum over the recurrent steps of
    dgi^T x_stacked, formed by the GRU backward from k times fewer steps, so its bf16 noise averages over fewer terms -- measured on
    an MI355X, unidirectional: 1.8e-2 at k = 1 (135 steps), 3.6e-2 at k = 2 (57), 9.0e-2 at k = 3 (38); bidirectional 2.0e-2,
    1.1e-2, 2.8e-2; the worst parameter, conv_blocks._sequential_0.W, 1.2e-1 at k = 1 and 1.0e-1 .. 1.7e-1 at k = 2, 3.)"""
    first = "rnn_blocks._sequential_0.w_ih"
    errs1, loss1, ref1, _, _ = _gradient_errors(device, 1, bidirectional)
    errs, loss, ref, l_len, wrong = _gradient_errors(device, k, bidirectional)
    worst1, worst = max(errs1, key=errs1.get), max(errs, key=errs.get)
    bar = 2 * errs1[worst1]
    print("time reduction k=%d bidirectional=%s: labels %s  loss %.5f (oracle %.5f)  worst gradient %.4e (%s); k=1: %.4e (%s)  | first w_ih "
          "%.4e; k=1: %.4e; against reversed groups %.4e, groups one frame late %.4e"
          % (k, bidirectional, l_len, loss, ref, errs[worst], worst, errs1[worst1], worst1, errs[first], errs1[first],
             wrong["reversed"], wrong["shifted"]))
    assert abs(loss - ref) <= 3e-2 * abs(ref), (loss, ref)                      # (the float32-oracle bar of smoke())
    assert errs[worst] <= bar, (worst, errs[worst], errs1[worst1])
    assert errs[first] <= bar, (errs[first], errs1[worst1])
    for variant, e in wrong.items():
        assert e > bar, "the bar cannot tell w_ih's gradient under %s stacking from the right one: %.3e against %.3e" % (variant, e, bar)


# ------------------------------------------------------------------------------------------------------------ the stream
def _schedule(kind, lens, seed=0):
    """tests/test_acoustic_stream_gpu.py::_schedule: "whole": one chunk; "single": 1-frame chunks; "ragged": every slot a different
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


def _feed(stream, x, calls, start=None, each=None, reset_between=False, Tc_of=None):
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
        if reset_between:
            stream.reset()
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


@pytest.mark.parametrize("tau", [0, 3])
@pytest.mark.parametrize("k", [2, 3])
def test_stream_against_the_float32_oracle(device, k, tau):
    """(4) any cuts, then flush: exactly ceil(x_len / k) frames per slot, as close to the oracle as the k = 1 one-shot forward"""
    from asr.model.stream import AcousticStream
    E1 = _setup(device, 1, False, tau)["E"]
    s = _setup(device, k, False, tau)
    out_len = s["out_len"]
    got, Es = {}, {}
    for kind in ("whole", "single", "ragged"):
        st = AcousticStream(s["model"], B, max_chunk=64)
        assert st.delay == tau and st.k == k and st.plan["time_reduction"] == k
        pend, held = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        outs = _feed(st, s["x"], _schedule(kind, X_LEN))
        for logits, lengths, n in outs:                                          # the groups completed, minus what the lookahead holds
            groups = (pend + n) // k
            assert lengths.cpu().tolist() == np.maximum(0, held + groups - tau).tolist()
            pend, held = (pend + n) % k, np.minimum(tau, held + groups)
        assert st.frames.cpu().tolist() == [max(0, n // k - tau) for n in X_LEN]
        tail, tail_len = st.flush()
        assert tuple(tail.shape) == (tau + 1, B, V)
        assert tail_len.cpu().tolist() == [g - max(0, n // k - tau) for g, n in zip(out_len, X_LEN)]
        assert st.frames.cpu().tolist() == out_len
        got[kind] = _per_slot(outs + [(tail, tail_len, None)])
        assert [g.shape[0] for g in got[kind]] == out_len
        Es[kind] = _rel(got[kind], s["want"])
        again, again_len = st.flush()                                            # nothing is pending any more
        assert again_len.cpu().tolist() == [0] * B
    st = AcousticStream(s["model"], B, max_chunk=64)                             # the same frames, the carried rows dropped
    outs = _feed(st, s["x"], _schedule("ragged", X_LEN), reset_between=True)
    lost = _per_slot(outs + [st.flush() + (None,)])
    padded = []
    for g, n in zip(lost, out_len):                                              # (dropped pending frames are missing frames: count them as zeros)
        padded.append(torch.cat([g[:n], torch.zeros(max(0, n - g.shape[0]), V)]))
    bad = _rel(padded, s["want"])
    same = all(torch.equal(a, b) for kind in ("single", "ragged") for a, b in zip(got["whole"], got[kind]))
    diff = max(float((a - b).abs().max()) for kind in ("single", "ragged") for a, b in zip(got["whole"], got[kind]))
    print("acoustic stream k=%d tau=%d: E1 %.4e  one-shot %.4e  Es whole %.4e single %.4e ragged %.4e  with resets %.4e (%s of %s frames)"
          "  | the cut schedules give %s bits (differ by at most %.3e)"
          % (k, tau, E1, s["E"], Es["whole"], Es["single"], Es["ragged"], bad, [g.shape[0] for g in lost], out_len,
             "the same" if same else "different", diff))
    for kind in Es:
        assert Es[kind] <= 2 * E1, (kind, Es[kind], E1)
    assert bad > 2 * E1, "the bar cannot tell a stream that forgets its state from one that carries it"


@pytest.mark.parametrize("k", [2, 3])
def test_slots_are_independent(device, k):
    """(5) slot 2 ends its utterance in the middle (flush) and starts another one while the others go on: they do not notice, and the
    new utterance comes out as it does from a fresh stream"""
    from asr.model.stream import AcousticStream
    from oracle import model as omodel
    s = _setup(device, k, False, 3)
    x = s["x"]
    second = omodel.synthetic_batch(B, 17, V, Lmin=3, Lmax=9, seed=5)[0]        # slot 2's second utterance: 17 frames
    calls = _schedule("ragged", X_LEN, seed=1)
    cut = next(i for i in range(len(calls)) if sum(c[2] for c in calls[:i + 1]) == X_LEN[2]) + 1     # slot 2 is through after `cut` calls
    assert cut < len(calls) - 3
    mask = [0, 0, 1, 0]
    # run A: with the restart
    a = AcousticStream(s["model"], B, max_chunk=64)
    outs_a = _feed(a, x, calls[:cut])
    tail_a = a.flush(mask)
    first_a = _per_slot(outs_a + [tail_a + (None,)])[2]
    flushed = tail_a[1].cpu().tolist()
    assert tuple(tail_a[0].shape) == (4, B, V) and [flushed[b] for b in (0, 1, 3)] == [0, 0, 0]
    assert first_a.shape[0] == a.frames.cpu().tolist()[2] == -(-X_LEN[2] // k)
    rest, left2 = [], 17
    for c in calls[cut:]:
        c = c.copy()
        c[2] = min(left2, 4)
        left2 -= c[2]
        rest.append(c)
    assert left2 == 0
    xa = x.clone()
    xa[2, :, :, :17] = second[2]
    pos = np.sum(calls[:cut], axis=0)
    pos[2] = 0
    outs_a2 = _feed(a, xa, rest, start=pos)
    end_a = a.flush()
    assert a.frames.cpu().tolist() == _reduced([X_LEN[0], X_LEN[1], 17, X_LEN[3]], k)
    # run B: slot 2 just stays idle after its first utterance
    b = AcousticStream(s["model"], B, max_chunk=64)
    idle = [np.array([c[0], c[1], 0, c[3]]) for c in rest]
    outs_b = _feed(b, x, calls[:cut]) + _feed(b, x, idle, start=np.sum(calls[:cut], axis=0), Tc_of=[int(c.max()) for c in rest])
    end_b = b.flush()
    for (la, na, _), (lb, nb, _) in zip(outs_a + outs_a2 + [end_a + (None,)], outs_b + [end_b + (None,)]):
        na, nb = na.cpu().tolist(), nb.cpu().tolist()
        for slot in (0, 1, 3):
            assert na[slot] == nb[slot] and torch.equal(la[:na[slot], slot], lb[:nb[slot], slot])
    # run C: the second utterance alone in a fresh stream, cut the same way
    c = AcousticStream(s["model"], B, max_chunk=64)
    alone = [np.array([0, 0, r[2], 0]) for r in rest]
    outs_c = _feed(c, xa, alone, Tc_of=[int(r.max()) for r in rest])
    end_c = c.flush()
    got_a = _per_slot(outs_a2 + [end_a + (None,)])[2]
    got_c = _per_slot(outs_c + [end_c + (None,)])[2]
    assert got_a.shape[0] == -(-17 // k) and torch.equal(got_a, got_c)


@pytest.mark.parametrize("k", [2, 3])
def test_the_stream_feeds_the_decoders(device, k):
    """(6) (logits, lengths) of every advance and of the flush go as they are into a BeamStream and a KeywordStream: bit for bit the
    one-shot beam search / keyword search of the concatenated stream logits"""
    from asr import error, spot
    from asr.model.stream import AcousticStream
    s = _setup(device, k, False, 3)
    out_len, To = s["out_len"], -(-T // k)
    kws = spot.KeywordSet([(3, 4), (5,), (7, 8, 9), (2, 2)], V)
    beam = error.BeamStream(B, V, max_frames=256, beam_width=8, top_k=8)
    spotter = spot.KeywordStream(B, V, kws, device)
    dets = []

    def each(logits, lengths):
        beam.advance(logits, lengths)
        dets.append((spotter.advance(logits, lengths), lengths.cpu().tolist()))

    st = AcousticStream(s["model"], B, max_chunk=64)
    outs = _feed(st, s["x"], _schedule("ragged", X_LEN, seed=2), each=each)
    tail = st.flush()
    each(*tail)
    got = _per_slot(outs + [tail + (None,)])
    cat = torch.zeros((To, B, V))
    for slot, g in enumerate(got):
        cat[:g.shape[0], slot] = g
    cat, lens = cat.to(device), torch.tensor(out_len, dtype=torch.int32, device=device)
    ids, n, scores = error.beam_decode(cat, beam_width=8, top_k=8, lengths=lens)
    sids, sn, sscores = beam.result()
    assert torch.equal(sn, n) and torch.equal(sscores, scores)
    w = min(To, sids.shape[2])                  # (the stream's ids are as wide as the rows it was fed, the one-shot's as T')
    assert torch.equal(sids[:, :, :w], ids[:, :, :w]) and bool((sids[:, :, w:] == 0).all()) and bool((ids[:, :, w:] == 0).all())
    K = len(kws.phrases)
    score = torch.full((B, K, To), float("-inf"), device=device)
    start = torch.full((B, K, To), -1, dtype=torch.int32, device=device)
    fill = torch.zeros((B, To), device=device)
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
    for w, h in zip(want, have):
        assert torch.equal(w, h)


# ------------------------------------------------------------------------------------------------------------ checkpoints, refusals
def test_round_trip_and_refusals(device, tmp_path):
    """(7) save -> fresh build -> load: identical logits at k = 2; AcousticStream refuses what it refused"""
    from asr.model import ds2
    from asr.model.stream import AcousticStream
    s = _setup(device, 2)
    model, x, x_len = s["model"], s["x"].to(device), s["x_len"].to(device)
    for name in ("model.hdf5", "model.npz"):
        path = str(tmp_path / name)
        model.save(path)
        cfg, fresh = _build(device, 2, seed=7)
        assert fresh.load(path)
        assert list(fresh.state_dict().keys()) == list(model.state_dict().keys())
        for key, value in model.state_dict().items():
            assert torch.equal(fresh.state_dict()[key], value), key
        with torch.no_grad():
            again = fresh(x, split_into_variables=False, x_length=x_len).float().cpu()
        assert all(torch.equal(again[b, :n], s["one"][b]) for b, n in enumerate(s["out_len"]))
    st = AcousticStream(model, B, max_chunk=8)
    with pytest.raises(ValueError):
        st.advance(x[:, :, :, :9])                                              # longer than max_chunk
    with pytest.raises(ValueError):
        st.advance(x[:3, :, :, :4])                                             # wrong B
    with pytest.raises(ValueError):
        st.advance(x[:, :, :, :4], [4, 5, 0, 1])                                # a length above Tc
    with pytest.raises(ValueError):
        st.advance(x[:, :, :, :4], [4, 4, 4])                                   # one length per slot
    with pytest.raises(ValueError):
        st.reset([1, 0])
    with pytest.raises(ValueError):
        st.flush([1, 0])
    with pytest.raises(ValueError):
        st.advance(x[:, :, :39, :4])                                            # not the model's features
    assert st.frames.cpu().tolist() == [0] * B                                  # (nothing was consumed)
    logits, lengths = st.advance(x[:, :, :, :0])                                # an empty chunk changes nothing
    assert tuple(logits.shape) == (0, B, V) and lengths.tolist() == [0] * B
    with pytest.raises(ValueError):
        AcousticStream(_build(device, 2, bidirectional=True)[1], B)             # bidirectional
    with pytest.raises(ValueError):
        AcousticStream(torch.nn.Linear(2, 2), B)
