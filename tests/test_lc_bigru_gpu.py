"""``latency_control`` = (Nc, Nr) of ds2.Model (asr.nn.LCBiGRU) and of asr.model.stream.AcousticStream, end to end against the
float32 oracle: oracle.model.DS2Oracle with the restated layer of tests/lc_bigru_reference.py in place of every recurrent layer.

The bars are measured at run time from code this feature does not touch: the plain bidirectional model (nn.BiGRU) of the same sizes,
seed and ``time_reduction`` against DS2Oracle on the same inputs.  FORWARD: E <= 2 E1, E1 the relative L2 distance of its one-shot
logits to the oracle over the valid frames; GRADIENT: twice its worst parameter-gradient distance under the CTC loss, for every
parameter, and twice its worst distance over the recurrent layers' parameters for those (a tighter bar, and the one that reaches a
mistake in the layer's backward pass).  The
latency-controlled model rounds where the plain one rounds (and once more: the forward direction's output before the two directions
are summed), so its error is another draw from the same distribution, while a window that is off by one frame, a right context that
is not there or a reverse state carried across blocks is an error of order 1e-1: the tests show that the bars tell.

A run on an MI355X (bf16) is recorded in DESIGN.md section 41.6."""
import numpy as np
import pytest
import torch

import lc_bigru_reference as lc

pytestmark = pytest.mark.gpu

V, B, T = 32, 4, 41
X_LEN = [41, 29, 5, 36]                    # slot 2 is shorter than most chunks
CONTROLS = [(8, 4), (5, 7), (64, 0)]
SEED = 1


def _reduced(lens, k):
    return [-(-int(n) // k) for n in lens]


def _build(device, control, k):
    from asr.model import ds2
    torch.manual_seed(SEED)
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers, cfg.bidirectional = V, 16, 64, 32, 2, True
    cfg.time_reduction, cfg.latency_control = k, control
    model = ds2.Model(cfg)
    model.to_gpu()
    return cfg, model


def _rel(got, want):
    """relative L2 over the valid frames of all slots"""
    a = torch.cat([g.double().flatten() for g in got])
    b = torch.cat([w.double().flatten() for w in want])
    assert bool(torch.isfinite(a).all())
    return float((a - b).norm() / b.norm())


def _valid(tbv, lens):
    return [tbv[:n, b] for b, n in enumerate(lens)]


_CACHE = {}


def _setup(device, control, k):
    """model, input, its one-shot logits, the oracle's logits (valid frames per slot) and their distance E -- once per case.
    control None: the plain bidirectional model against DS2Oracle, whose distances are the bars."""
    key = (control, k)
    if key not in _CACHE:
        from oracle import model as omodel
        cfg, model = _build(device, control, k)
        x = omodel.synthetic_batch(B, T, V, Lmin=3, Lmax=9, seed=0, ragged=True)[0]
        x_len = torch.tensor(X_LEN, dtype=torch.int32)
        out_len = _reduced(X_LEN, k)
        with torch.no_grad():
            one = model(x.to(device), split_into_variables=False, x_length=x_len.to(device)).float().cpu()      # (B, T', V)
        assert tuple(one.shape) == (B, -(-T // k), V)
        state = {name: v.detach().cpu() for name, v in model.state_dict().items()}
        ref = lc.oracle(state, cfg)
        with torch.no_grad():
            want = ref(x, x_len).detach()                                                                       # (T', B, V)
        if control is None and k == 1:                                          # the restated forward is DS2Oracle's
            plain = omodel.DS2Oracle(state, cfg.num_conv_layers, cfg.num_rnn_layers, bidirectional=True, matched=False)
            assert _rel(_valid(want, out_len), _valid(plain(x, x_len).detach(), out_len)) == 0.0
        want = _valid(want, out_len)
        one = [one[b, :n] for b, n in enumerate(out_len)]
        _CACHE[key] = dict(cfg=cfg, model=model, state=state, x=x, x_len=x_len, out_len=out_len, one=one, want=want, E=_rel(one, want))
    return _CACHE[key]


def _forward_bar(device, k):
    return 2 * _setup(device, None, k)["E"]


# ------------------------------------------------------------------------------------------------------------ one-shot forward
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("control", CONTROLS)
def test_one_shot_forward_against_the_restated_oracle(device, control, k):
    bar = _forward_bar(device, k)
    s = _setup(device, control, k)
    wrong = {}
    if control != (64, 0):                                  # (with one block per utterance there is nothing to get wrong)
        for variant in lc.MUTANTS[:3]:
            with torch.no_grad():
                wrong[variant] = _rel(s["one"], _valid(lc.oracle(s["state"], s["cfg"], variant)(s["x"], s["x_len"]).detach(), s["out_len"]))
    print("latency control %s k=%d: plain E1 %.4e  E %.4e  | against mutants %s"
          % (control, k, bar / 2, s["E"], {name: "%.3e" % e for name, e in wrong.items()}))
    assert s["E"] <= bar, (s["E"], bar)
    for variant, e in wrong.items():
        assert e > 5 * bar, "the bar cannot tell the mutant %s from the layer: %.3e against %.3e" % (variant, e, bar)


@pytest.mark.parametrize("k", [1, 2])
def test_one_block_per_utterance_is_the_bidirectional_model(device, k):
    """(64, 0): the blocks are longer than the utterances, so the layer is nn.BiGRU -- the plain model with the same parameters, up to
    the rounding of the forward direction's output before the sum"""
    s, plain = _setup(device, (64, 0), k), _setup(device, None, k)
    plain["model"].load_state_dict(s["model"].state_dict())                     # (same seed: the same values already; names and shapes agree)
    with torch.no_grad():
        one = plain["model"](s["x"].to(device), split_into_variables=False, x_length=s["x_len"].to(device)).float().cpu()
    e = _rel(s["one"], [one[b, :n] for b, n in enumerate(s["out_len"])])
    print("latency control (64, 0) k=%d against nn.BiGRU with the same parameters: %.4e (bar %.4e)" % (k, e, _forward_bar(device, k)))
    assert e <= _forward_bar(device, k)


def test_without_lengths_the_padded_block_is_one_utterance(device):
    s = _setup(device, (5, 7), 1)
    with torch.no_grad():
        whole = s["model"](s["x"].to(device), split_into_variables=False)
        want = lc.oracle(s["state"], s["cfg"])(s["x"], None).detach()
    assert tuple(whole.shape) == (B, T, V)
    e = _rel([whole[b].float().cpu() for b in range(B)], [want[:, b] for b in range(B)])
    assert e <= _forward_bar(device, 1), e


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


def _gradient_errors(device, control, k, mutant=None):
    """({parameter: relative L2 of its CTC gradient against the oracle's autograd}, losses, the same against the mutant oracle)"""
    if (control, k) not in _GRADS:
        from asr.functions import join_side_stream
        from asr.loss import connectionist_temporal_classification
        from oracle import model as omodel
        s = _setup(device, control, k)
        model, x_len = s["model"], s["x_len"]
        labels, l_len = _labels(k)
        out_len = model.output_length(x_len)
        for p in model.parameters():
            p.grad = None
        ys = model(s["x"].to(device), x_length=x_len.to(device))
        loss = connectionist_temporal_classification(ys, labels.to(device), 0, out_len.to(device), l_len.to(device))
        loss.backward()
        join_side_stream()
        torch.cuda.synchronize()

        def against(variant):
            ref = lc.oracle(s["state"], s["cfg"], variant)
            loss_ref = omodel.ctc_mean_loss(ref(s["x"], x_len), labels, out_len, l_len)
            loss_ref.backward()
            errs = {}
            for name, p in model.named_parameters():
                g, gr = p.grad.detach().cpu().double(), ref.g(name).grad.double()
                assert bool(torch.isfinite(g).all()), name
                norms.setdefault(name, gr.norm())           # (of the right oracle's gradient, for the mutant's distance as well)
                errs[name] = float((g - gr).norm() / norms[name])
            return errs, loss_ref.item()

        norms = {}
        errs, loss_ref = against(None)
        wrong = against(mutant)[0] if mutant else None
        _GRADS[(control, k)] = (errs, loss.item(), loss_ref, wrong)
        for p in model.parameters():
            p.grad = None
    return _GRADS[(control, k)]


def _recurrent(errs):
    return {name: e for name, e in errs.items() if name.startswith("rnn_blocks.")}


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("control", CONTROLS)
def test_gradients_against_the_oracles_autograd(device, control, k):
    """CTC on output_length(x_len) frames.  Two bars from the plain bidirectional model in the same run: every parameter's gradient is
    held to twice its worst parameter-gradient distance (the first convolution's weight, whose bf16 noise no recurrent layer has a part
    in), and the recurrent layers' parameters -- the gradients this layer computes -- to twice its worst distance over those
    parameters alone, a bar three to four times tighter.  The bars tell: the same device gradients against an oracle whose
    right-context outputs receive gradient (the forward pass is the right one) are more than five recurrent bars away."""
    errs1 = _gradient_errors(device, None, k)[0]
    errs, loss, ref, wrong = _gradient_errors(device, control, k, None if control == (64, 0) else "right_context_gradient")
    worst1, worst = max(errs1, key=errs1.get), max(errs, key=errs.get)
    bar = 2 * errs1[worst1]
    rec1, rec = _recurrent(errs1), _recurrent(errs)
    assert len(rec) == 8 and len(rec1) == 8
    rbar = 2 * max(rec1.values())
    print("latency control %s k=%d: loss %.5f (oracle %.5f)  worst gradient %.4e (%s); plain: %.4e (%s)  | recurrent parameters: worst "
          "%.4e; plain: %.4e%s"
          % (control, k, loss, ref, errs[worst], worst, errs1[worst1], worst1, max(rec.values()), max(rec1.values()),
             "" if wrong is None else "; against right-context gradient: %.4e" % max(_recurrent(wrong).values())))
    assert abs(loss - ref) <= 3e-2 * abs(ref), (loss, ref)                      # (the float32-oracle bar of smoke())
    assert errs[worst] <= bar, (worst, errs[worst], bar)
    assert max(rec.values()) <= rbar, (max(rec, key=rec.get), max(rec.values()), rbar)
    if wrong is not None:
        far = max(_recurrent(wrong).values())
        assert far > 5 * rbar, "the bar cannot tell right-context gradient from none: %.3e against %.3e" % (far, rbar)


def test_a_layer_whose_input_asks_for_no_gradient(device):
    """the layer alone on an input without requires_grad: its parameters still get their gradients, bit for bit those of the same
    call on an input that asks for one"""
    from asr import nn
    from asr.functions import join_side_stream
    torch.manual_seed(3)
    layer = nn.LCBiGRU(16, 32, block=4, right=3).to_gpu()
    x = torch.randn(3, 16, 13, device=device)
    x_len = torch.tensor([13, 6, 9], dtype=torch.int32, device=device)
    g = torch.randn(3, 32, 13, device=device)
    grads = []
    for needs in (False, True):
        layer.cleargrads()
        xin = x.clone().requires_grad_(needs)
        y = layer(xin, x_len)
        assert y.requires_grad
        y.backward(g.to(y.dtype))
        join_side_stream()
        torch.cuda.synchronize()
        grads.append({name: p.grad.clone() for name, p in layer.named_parameters()})
        assert (xin.grad is not None) == needs
    for name, value in grads[0].items():
        assert all(bool(value[d].abs().sum() > 0) for d in range(2)), name
        assert torch.equal(value, grads[1][name]), name


def test_the_weight_copies_follow_an_optimiser_step(device):
    """the 16-bit copies of the two directions' weights live in holders of their own: after an optimiser step the layer computes with
    the new weights -- bit for bit what a fresh model loaded with them computes -- and the step has moved every recurrent parameter
    of both directions"""
    from asr.loss import connectionist_temporal_classification
    from asr.optimizers import Adam
    s = _setup(device, (5, 7), 1)
    _, model = _build(device, (5, 7), 1)
    x, x_len = s["x"].to(device), s["x_len"].to(device)
    labels, l_len = _labels(1)
    with torch.no_grad():
        model(x, x_length=x_len)                                                # (sizes the lazily sized parameters)
    before = {name: p.detach().clone() for name, p in model.named_parameters()}
    opt = Adam(1e-3, 0.9)
    opt.setup(model)
    loss = connectionist_temporal_classification(model(x, x_length=x_len), labels.to(device), 0, x_len, l_len.to(device))
    opt.update(lossfun=lambda: loss)
    for name, p in model.named_parameters():
        if "rnn_blocks" in name:
            assert all(bool((p.detach()[d] != before[name][d]).any()) for d in range(2)), name
    with torch.no_grad():
        after = model(x, split_into_variables=False, x_length=x_len).float()
    _, fresh = _build(device, (5, 7), 1)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        want = fresh(x, split_into_variables=False, x_length=x_len).float()
    valid = (lambda bt: [bt[b, :n] for b, n in enumerate(X_LEN)])
    assert all(torch.equal(a, w) for a, w in zip(valid(after), valid(want)))
    assert _rel(valid(after.cpu()), s["one"]) > 1e-3                            # (and they are not the old weights' logits)


# ------------------------------------------------------------------------------------------------------------ the stream
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


def _feed(stream, x, calls, start=None, each=None, Tc_of=None):
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
        logits, lengths = stream.advance(chunk.to(stream.device), n.astype(np.int32))
        rows = stream.delay + (stream.k - 1 + Tc + stream.k - 1) // stream.k
        assert tuple(logits.shape) == (rows, x.shape[0], V) and logits.dtype == torch.float32 and lengths.dtype == torch.int32
        if each is not None:
            each(logits, lengths)
        out.append((logits, lengths, n))
    return out


def _per_slot(outs):
    """the valid rows of every call, concatenated per slot"""
    nslots = outs[0][0].shape[1]
    lens = [o[1].cpu().tolist() for o in outs]
    return [torch.cat([o[0][:l[b], b] for o, l in zip(outs, lens)]).cpu() for b in range(nslots)]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("control", CONTROLS)
def test_stream_against_the_restated_oracle(device, control, k):
    """one chunk, 1-frame chunks and ragged chunks: the same utterances, each against the oracle at the forward bar; every slot has
    emitted ceil(x_len / k) frames after the flush, never more than whole blocks with their right context before it"""
    from asr.model.stream import AcousticStream
    s = _setup(device, control, k)
    Nc, Nr = control
    bar = _forward_bar(device, k)
    got, Es = {}, {}
    for kind in ("whole", "single", "ragged"):
        stream = AcousticStream(s["model"], B, max_chunk=64)
        assert stream.delay == 2 * (Nc + Nr - 1) and stream.k == k
        outs = _feed(stream, s["x"], _schedule(kind, X_LEN))
        fed = np.zeros(B, dtype=np.int64)
        for (logits, lengths, n), frames in zip(outs, np.cumsum([o[1].cpu().numpy() for o in outs], axis=0)):
            fed += n
            assert all(f % Nc == 0 and f <= max(0, r // k - 2 * Nr) for f, r in zip(frames, fed)), (kind, frames, fed)
        tail, tail_len = stream.flush()
        assert tail.shape[0] <= stream.delay + (1 if k > 1 else 0) and tail.shape[1:] == (B, V)
        assert stream.frames.cpu().tolist() == s["out_len"]
        got[kind] = _per_slot(outs + [(tail, tail_len, None)])
        assert [g.shape[0] for g in got[kind]] == s["out_len"]                   # exactly ceil(x_len / k) frames per slot
        Es[kind] = _rel(got[kind], s["want"])
        again, again_len = stream.flush()                                        # nothing is pending any more
        assert again_len.cpu().tolist() == [0] * B
    same = {kind: all(torch.equal(a, b) for a, b in zip(got["whole"], got[kind])) for kind in ("single", "ragged")}
    diff = max(float((a - b).abs().max()) for kind in ("single", "ragged") for a, b in zip(got["whole"], got[kind]))
    print("latency control %s k=%d stream: bar %.4e  one-shot %.4e  whole %.4e single %.4e ragged %.4e  | same bits as one chunk: %s "
          "(largest difference %.3e)" % (control, k, bar, s["E"], Es["whole"], Es["single"], Es["ragged"], same, diff))
    for kind in Es:
        assert Es[kind] <= bar, (kind, Es[kind], bar)


def test_blocks_of_one_frame_hold_nothing_back(device):
    """(Nc, Nr) = (1, 0): every frame is a block of its own, K = 0: what goes in comes out, the delay is 0 and ``flush`` has no rows"""
    from asr.model.stream import AcousticStream
    s = _setup(device, (1, 0), 1)
    assert s["E"] <= _forward_bar(device, 1)
    stream = AcousticStream(s["model"], B, max_chunk=64)
    assert stream.delay == 0
    outs = _feed(stream, s["x"], _schedule("ragged", X_LEN))
    for logits, lengths, n in outs:
        assert lengths.cpu().tolist() == n.tolist()
    assert stream.frames.cpu().tolist() == X_LEN
    tail, tail_len = stream.flush([1, 0, 1, 0])
    assert tuple(tail.shape) == (0, B, V) and tail_len.cpu().tolist() == [0] * B and stream.frames.cpu().tolist() == X_LEN
    assert _rel(_per_slot(outs), s["want"]) <= _forward_bar(device, 1)


def test_slots_are_independent(device):
    """slot 2 ends its utterance in the middle and starts another one while the others go on: they do not notice, and the new
    utterance comes out as it does from a fresh stream cut the same way"""
    from asr.model.stream import AcousticStream
    from oracle import model as omodel
    s = _setup(device, (5, 7), 1)
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
    assert tail_a[1].cpu().tolist() == [0, 0, X_LEN[2], 0] and a.frames.cpu().tolist()[2] == X_LEN[2]    # (5 frames: no whole block before)
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
    assert a.frames.cpu().tolist() == [X_LEN[0], X_LEN[1], 17, X_LEN[3]]
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
    assert got_a.shape[0] == 17 and torch.equal(got_a, got_c)
    # reset(mask) drops what a slot holds: slot 0 starts over, the frames it had pending never come out
    d = AcousticStream(s["model"], B, max_chunk=64)
    _feed(d, x, [np.array([9, 9, 0, 9])])
    assert d.frames.cpu().tolist() == [0, 0, 0, 0]
    d.reset([1, 0, 0, 0])
    _feed(d, x, [np.array([5, 8, 0, 8])], start=[0, 9, 0, 9])
    assert d.frames.cpu().tolist() == [0, 0, 0, 0]                             # (17 frames: two blocks through the first layer, none through the second)
    tail, tail_len = d.flush()
    assert tail_len.cpu().tolist() == [5, 17, 0, 17] and d.frames.cpu().tolist() == [5, 17, 0, 17]


def test_a_model_that_never_ran_streams(device):
    """the recurrent layers size their input weights at the first chunk, as the one-shot forward does at its first call"""
    from asr.model.stream import AcousticStream
    s = _setup(device, (8, 4), 2)
    _, model = _build(device, (8, 4), 2)
    assert model.rnn_blocks.layers[0].w_ih.numel() == 0
    stream = AcousticStream(model, B, max_chunk=64)
    outs = _feed(stream, s["x"], _schedule("whole", X_LEN))
    tail = stream.flush()
    assert tuple(model.rnn_blocks.layers[0].w_ih.shape) == (2, 192, 192) and stream.frames.cpu().tolist() == s["out_len"]
    got = _per_slot(outs + [tail + (None,)])
    assert [g.shape[0] for g in got] == s["out_len"] and all(bool(torch.isfinite(g).all()) for g in got)


def test_the_stream_feeds_the_decoders(device):
    """(logits, lengths) of every advance and of the flush go as they are into a BeamStream and a KeywordStream: bit for bit the
    one-shot beam search / keyword search of the concatenated stream logits"""
    from asr import error, spot
    from asr.model.stream import AcousticStream
    s = _setup(device, (8, 4), 1)
    kws = spot.KeywordSet([(3, 4), (5,), (7, 8, 9), (2, 2)], V)
    beam = error.BeamStream(B, V, max_frames=1024, beam_width=8, top_k=8)      # (every advance hands over delay + Tc rows)
    spotter = spot.KeywordStream(B, V, kws, device)
    dets = []

    def each(logits, lengths):
        beam.advance(logits, lengths)
        dets.append((spotter.advance(logits, lengths), lengths.cpu().tolist()))

    stream = AcousticStream(s["model"], B, max_chunk=64)
    outs = _feed(stream, s["x"], _schedule("ragged", X_LEN, seed=2), each=each)
    tail = stream.flush()
    each(*tail)
    got = _per_slot(outs + [tail + (None,)])
    cat = torch.zeros((T, B, V))
    for slot, g in enumerate(got):
        cat[:g.shape[0], slot] = g
    cat, lens = cat.to(device), torch.tensor(X_LEN, dtype=torch.int32, device=device)
    ids, n, scores = error.beam_decode(cat, beam_width=8, top_k=8, lengths=lens)
    sids, sn, sscores = beam.result()
    assert torch.equal(sn, n) and torch.equal(sscores, scores)
    w = min(ids.shape[2], sids.shape[2])        # (the stream's ids are as wide as the rows it was fed, the one-shot's as T)
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
    from asr import nn
    from asr.model.stream import AcousticStream
    s = _setup(device, (8, 4), 1)
    stream = AcousticStream(s["model"], B, max_chunk=8)
    x = s["x"].to(device)
    with pytest.raises(ValueError):
        stream.advance(x[:, :, :, :9])                                          # longer than max_chunk
    with pytest.raises(ValueError):
        stream.advance(x[:3, :, :, :4])                                         # wrong B
    with pytest.raises(ValueError):
        stream.advance(x[:, :, :, :4], [4, 5, 0, 1])                            # a length above Tc
    with pytest.raises(ValueError):
        stream.advance(x[:, :, :39, :4])                                        # not the model's features
    with pytest.raises(ValueError):
        stream.reset([1, 0])
    assert stream.frames.cpu().tolist() == [0] * B                              # (nothing was consumed)
    with pytest.raises(ValueError, match="a bidirectional model cannot be streamed: its reverse recurrences start at the end of the utterance"):
        AcousticStream(_setup(device, None, 1)["model"], B)                     # plain BiGRU layers: refused as ever
    layer = nn.LCBiGRU(16, 8, block=4, right=2).to_gpu()
    with pytest.raises(ValueError):
        layer(torch.zeros(2, 16, 5, device=device), hx=torch.zeros(2, 2, 8, device=device))
    with pytest.raises(ValueError):
        layer(torch.zeros(2, 16, device=device))                                # not (B, D, T)
    from asr import functions
    with pytest.raises(ValueError):
        functions.lc_bigru(torch.zeros(2, 16, 5, device=device), layer.w_ih, layer.w_hh, layer.b_ih, layer.b_hh, layer, 0, 2)
