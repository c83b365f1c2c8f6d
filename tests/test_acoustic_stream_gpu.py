"""asr.model.stream.AcousticStream: a causal ds2.Model fed chunk by chunk against the float32 oracle of the whole utterance.

The bar of (1) and (2) is Es <= 2 E1: E1 is the relative L2 distance, over the valid frames, between today's one-shot forward
and the float32 oracle -- measured at run time -- and Es the same distance for the concatenated stream output.  The stream rounds
where the one-shot forward rounds (its GRU input projection even stays float32), so its error is a second draw from the same
distribution; a context that is off by one frame or a state that is not carried is an error of order 1.  The test shows that the
bar can tell: the same frames with ``reset()`` between the chunks fail it.
A run on an MI355X (bf16): tau = 0: E1 = 4.057e-3, Es = 3.915e-3 for each of one chunk / 1-frame chunks / ragged chunks (the three
schedules gave the same bits), with resets 4.23e-1; tau = 3: E1 = 4.321e-3, Es = 4.338e-3.
"""
import numpy as np
import pytest
import torch

import lookahead_reference as lref

pytestmark = pytest.mark.gpu

V, B, T = 32, 4, 41
X_LEN = [41, 29, 5, 36]                    # slot 2 is shorter than most chunks


def _build(device, lookahead=0, seed=0):
    """tests/test_model_gpu.py::_build with V = 32, forward-only"""
    from asr.model import ds2
    torch.manual_seed(seed)
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers, cfg.bidirectional = V, 16, 64, 32, 2, False
    cfg.lookahead = lookahead
    model = ds2.Model(cfg)
    model.to_gpu()
    if lookahead:
        with torch.no_grad():               # (a fresh lookahead layer is the identity: give every tap something to do)
            model.lookahead.W.copy_(torch.randn(model.lookahead.W.shape) * 0.4)
    return cfg, model


def _lookahead_oracle(state, cfg):
    """DS2Oracle (float32) with the float64 restatement of the lookahead layer between the GRU stack and the dense layers"""
    from oracle import model as omodel
    from oracle import nn as onn
    from oracle import bf16 as Q

    class Oracle(omodel.DS2Oracle):
        def forward(self, x, x_len=None):
            h = x
            for i, pool in enumerate([3] + [2] * (self.nconv - 1)):
                W, b = self.g("conv_blocks._sequential_%d.W" % (4 * i)), self.g("conv_blocks._sequential_%d.b" % (4 * i))
                h = onn.maxpool_h(onn.maxout2(onn.conv2d_causal(h, W, b, 0)), pool)
            Bn, C, H, Tn = h.shape
            h = h.permute(3, 0, 2, 1).reshape(Tn, Bn, H * C)
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

    return Oracle(state, cfg.num_conv_layers, cfg.num_rnn_layers, bidirectional=False, matched=False)


_CACHE = {}


def _setup(device, lookahead):
    """model, input, the one-shot logits, the oracle's logits (valid frames, per slot) and E1 -- once per lookahead"""
    if lookahead not in _CACHE:
        from oracle import model as omodel
        cfg, model = _build(device, lookahead)
        x = omodel.synthetic_batch(B, T, V, Lmin=3, Lmax=9, seed=0, ragged=True)[0]
        x_len = torch.tensor(X_LEN, dtype=torch.int32)
        with torch.no_grad():
            one = model(x.to(device), split_into_variables=False, x_length=x_len.to(device)).float().cpu()      # (B, T, V)
        state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        if lookahead == 0:
            ref = omodel.DS2Oracle(state, cfg.num_conv_layers, cfg.num_rnn_layers, bidirectional=False, matched=False)
            assert _rel([_lookahead_oracle(state, cfg)(x, x_len).detach()[:n, b] for b, n in enumerate(X_LEN)],
                        [ref(x, x_len).detach()[:n, b] for b, n in enumerate(X_LEN)]) == 0.0       # the restated forward is DS2Oracle's
        else:
            ref = _lookahead_oracle(state, cfg)
        with torch.no_grad():
            want = ref(x, x_len).detach()                                                                       # (T, B, V)
        want = [want[:n, b] for b, n in enumerate(X_LEN)]
        E1 = _rel([one[b, :n] for b, n in enumerate(X_LEN)], want)
        _CACHE[lookahead] = dict(cfg=cfg, model=model, x=x, x_len=x_len, want=want, E1=E1)
    return _CACHE[lookahead]


def _rel(got, want):
    """relative L2 over the valid frames of all slots"""
    a = torch.cat([g.double().flatten() for g in got])
    b = torch.cat([w.double().flatten() for w in want])
    assert bool(torch.isfinite(a).all())
    return float((a - b).norm() / b.norm())


def _schedule(kind, lens, seed=0):
    """per call: the frames every slot gets.  "whole": everything in one chunk; "single": chunks of 1 frame; "ragged": every
    slot a different number per call, some of them 0"""
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
    """run `calls` (per call: frames per slot, taken from x (B, C, H, T) at every slot's own position) -> per call
    (logits, lengths, n).  Rows of a chunk beyond a slot's share hold 9.0, which nothing may read."""
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
        assert tuple(logits.shape) == (Tc, x.shape[0], V) and logits.dtype == torch.float32 and lengths.dtype == torch.int32
        if each is not None:
            each(logits, lengths)
        out.append((logits, lengths, n))
    return out


def _per_slot(outs):
    """the valid rows of every call, concatenated per slot"""
    nslots = outs[0][0].shape[1]
    lens = [o[1].cpu().tolist() for o in outs]
    return [torch.cat([o[0][:l[b], b] for o, l in zip(outs, lens)]).cpu() for b in range(nslots)]


def test_tau_0_against_the_float32_oracle(device):
    from asr.model.stream import AcousticStream
    s0 = _setup(device, 0)
    got, Es = {}, {}
    for kind in ("whole", "single", "ragged"):
        s = AcousticStream(s0["model"], B, max_chunk=64)
        assert s.delay == 0
        outs = _feed(s, s0["x"], _schedule(kind, X_LEN))
        for logits, lengths, n in outs:
            assert lengths.cpu().tolist() == n.tolist()                          # tau = 0: what goes in comes out
        assert s.frames.cpu().tolist() == X_LEN
        tail, tail_len = s.flush()
        assert tail.shape[0] == 0 and tail_len.cpu().tolist() == [0] * B and s.frames.cpu().tolist() == X_LEN
        got[kind] = _per_slot(outs)
        assert [g.shape[0] for g in got[kind]] == X_LEN
        Es[kind] = _rel(got[kind], s0["want"])
    s = AcousticStream(s0["model"], B, max_chunk=64)
    bad = _rel(_per_slot(_feed(s, s0["x"], _schedule("ragged", X_LEN), reset_between=True)), s0["want"])
    diff = max(float((a - b).abs().max()) for k in ("single", "ragged") for a, b in zip(got["whole"], got[k]))
    print("acoustic stream tau=0: E1 %.4e  Es whole %.4e single %.4e ragged %.4e  with resets %.4e  | cut schedules differ by at most %.3e"
          % (s0["E1"], Es["whole"], Es["single"], Es["ragged"], bad, diff))
    for kind in Es:
        assert Es[kind] <= 2 * s0["E1"], (kind, Es[kind], s0["E1"])
    assert bad > 2 * s0["E1"], "the bar cannot tell a stream that forgets its state from one that carries it"


def test_tau_3_against_the_restated_oracle(device):
    from asr.model.stream import AcousticStream
    tau = 3
    s3 = _setup(device, tau)
    Es = {}
    for kind in ("whole", "single", "ragged"):
        s = AcousticStream(s3["model"], B, max_chunk=64)
        assert s.delay == tau
        m = np.zeros(B, dtype=np.int64)
        outs = _feed(s, s3["x"], _schedule(kind, X_LEN))
        for logits, lengths, n in outs:
            assert lengths.cpu().tolist() == np.maximum(0, m + n - tau).tolist()
            m = np.minimum(tau, m + n)
        assert s.frames.cpu().tolist() == [max(0, n - tau) for n in X_LEN]
        tail, tail_len = s.flush()
        assert tuple(tail.shape) == (tau, B, V) and tail_len.cpu().tolist() == [min(tau, n) for n in X_LEN]
        assert s.frames.cpu().tolist() == X_LEN
        got = _per_slot(outs + [(tail, tail_len, None)])
        assert [g.shape[0] for g in got] == X_LEN
        Es[kind] = _rel(got, s3["want"])
        again, again_len = s.flush()                                             # nothing is pending any more
        assert again_len.cpu().tolist() == [0] * B
    print("acoustic stream tau=3: E1 %.4e  Es whole %.4e single %.4e ragged %.4e" % (s3["E1"], Es["whole"], Es["single"], Es["ragged"]))
    for kind in Es:
        assert Es[kind] <= 2 * s3["E1"], (kind, Es[kind], s3["E1"])


def test_slots_are_independent(device):
    """slot 2 ends its utterance in the middle and starts another one while the others go on: they do not notice, and the new
    utterance comes out as it does from a fresh stream"""
    from asr.model.stream import AcousticStream
    from oracle import model as omodel
    s3 = _setup(device, 3)
    x = s3["x"]
    second = omodel.synthetic_batch(B, 17, V, Lmin=3, Lmax=9, seed=5)[0]        # slot 2's second utterance: 17 frames
    calls = _schedule("ragged", X_LEN, seed=1)
    cut = next(i for i in range(len(calls)) if sum(c[2] for c in calls[:i + 1]) == X_LEN[2]) + 1     # slot 2 is through after `cut` calls
    assert cut < len(calls) - 3
    mask = [0, 0, 1, 0]
    # run A: with the restart
    a = AcousticStream(s3["model"], B, max_chunk=64)
    outs_a = _feed(a, x, calls[:cut])
    tail_a = a.flush(mask)
    assert tail_a[1].cpu().tolist() == [0, 0, min(3, X_LEN[2]), 0] and a.frames.cpu().tolist()[2] == X_LEN[2]
    rest, left2, pos2 = [], 17, []
    for c in calls[cut:]:
        c = c.copy()
        c[2] = min(left2, 4)
        pos2.append(17 - left2)
        left2 -= c[2]
        rest.append(c)
    assert left2 == 0
    xa = x.clone()
    xa[2, :, :, :17] = second[2]
    pos = np.sum(calls[:cut], axis=0)
    pos[2] = 0
    outs_a2 = _feed(a, xa, rest, start=pos)
    end_a = a.flush()
    assert a.frames.cpu().tolist() == [X_LEN[0], X_LEN[1], 17, X_LEN[3]]
    # run B: slot 2 just stays idle after its first utterance
    b = AcousticStream(s3["model"], B, max_chunk=64)
    idle = [np.array([c[0], c[1], 0, c[3]]) for c in rest]
    outs_b = _feed(b, x, calls[:cut]) + _feed(b, x, idle, start=np.sum(calls[:cut], axis=0), Tc_of=[int(c.max()) for c in rest])
    end_b = b.flush()
    for (la, na, _), (lb, nb, _) in zip(outs_a + outs_a2 + [end_a + (None,)], outs_b + [end_b + (None,)]):
        na, nb = na.cpu().tolist(), nb.cpu().tolist()
        for slot in (0, 1, 3):
            assert na[slot] == nb[slot] and torch.equal(la[:na[slot], slot], lb[:nb[slot], slot])
    # run C: the second utterance alone in a fresh stream, cut the same way
    c = AcousticStream(s3["model"], B, max_chunk=64)
    alone = [np.array([0, 0, r[2], 0]) for r in rest]
    outs_c = _feed(c, xa, alone, Tc_of=[int(r.max()) for r in rest])
    end_c = c.flush()
    got_a = _per_slot(outs_a2 + [end_a + (None,)])[2]
    got_c = _per_slot(outs_c + [end_c + (None,)])[2]
    assert got_a.shape[0] == 17 and torch.equal(got_a, got_c)


def test_the_stream_feeds_the_decoders(device):
    """(logits, lengths) of every advance and of the flush go as they are into a BeamStream and a KeywordStream: bit for bit the
    one-shot beam search / keyword search of the concatenated stream logits"""
    from asr import error, spot
    from asr.model.stream import AcousticStream
    s3 = _setup(device, 3)
    kws = spot.KeywordSet([(3, 4), (5,), (7, 8, 9), (2, 2)], V)
    beam = error.BeamStream(B, V, max_frames=256, beam_width=8, top_k=8)
    spotter = spot.KeywordStream(B, V, kws, device)
    dets = []

    def each(logits, lengths):
        beam.advance(logits, lengths)
        dets.append((spotter.advance(logits, lengths), lengths.cpu().tolist()))

    s = AcousticStream(s3["model"], B, max_chunk=64)
    outs = _feed(s, s3["x"], _schedule("ragged", X_LEN, seed=2), each=each)
    tail = s.flush()
    each(*tail)
    got = _per_slot(outs + [tail + (None,)])
    cat = torch.zeros((T, B, V))
    for slot, g in enumerate(got):
        cat[:g.shape[0], slot] = g
    cat, lens = cat.to(device), torch.tensor(X_LEN, dtype=torch.int32, device=device)
    ids, n, scores = error.beam_decode(cat, beam_width=8, top_k=8, lengths=lens)
    sids, sn, sscores = beam.result()
    assert torch.equal(sn, n) and torch.equal(sscores, scores)
    w = min(T, sids.shape[2])                   # (the stream's ids are as wide as the rows it was fed, the one-shot's as T)
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
    assert pos == X_LEN
    want = spot.keyword_search(cat, kws, lens)
    have = spot.keyword_hits(spot.Detection(score, start, fill), lens)
    for w, h in zip(want, have):
        assert torch.equal(w, h)
    assert int(want.count.sum()) > 0


def test_refusals(device):
    from asr.model.stream import AcousticStream
    s0 = _setup(device, 0)
    s = AcousticStream(s0["model"], B, max_chunk=8)
    x = s0["x"].to(device)
    with pytest.raises(ValueError):
        s.advance(x[:, :, :, :9])                                               # longer than max_chunk
    with pytest.raises(ValueError):
        s.advance(x[:3, :, :, :4])                                              # wrong B
    with pytest.raises(ValueError):
        s.advance(x[:, :, :, :4], [4, 5, 0, 1])                                 # a length above Tc
    with pytest.raises(ValueError):
        s.advance(x[:, :, :, :4], [4, 4, 4])                                    # one length per slot
    with pytest.raises(ValueError):
        s.reset([1, 0])
    with pytest.raises(ValueError):
        s.advance(x[:, :, :39, :4])                                             # not the model's features
    assert s.frames.cpu().tolist() == [0] * B                                   # (nothing was consumed)
    from asr.model import ds2
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers = V, 16, 64, 32, 2
    with pytest.raises(ValueError):
        AcousticStream(ds2.Model(cfg).to_gpu(), B)                              # bidirectional
    with pytest.raises(ValueError):
        AcousticStream(torch.nn.Linear(2, 2), B)
