"""asr.model.stream.AcousticStream over the convolutional recipes (cnn.AcousticModel, architectures.build_model) fed chunk by chunk,
against ``oracle.cnn.forward`` (float32, unmatched) of the whole utterances.

The bar of (1) is Es <= 2 E1, as in tests/test_acoustic_stream_gpu.py: E1 is the relative L2 distance, over the valid frames, between
today's one-shot ``model(x)`` and the oracle -- measured at run time -- and Es the same distance for the concatenated stream output.
The stream rounds where the one-shot forward rounds, so its error is a second draw from the same distribution.  2 E1 must lie below
0.05: tests/test_cnn_stream_cpu.py shows that every convolution whose carry is dropped or a frame late moves these recipes' logits
by more than that, and here the same frames with ``reset()`` between the chunks must miss the bar.

The parameters are redrawn after the sizing call (cnn_stream_reference.redraw): at the default initialisation the `glu` recipe's
logits barely depend on the input, and no bar could see a broken carry there.

A run on an MI355X (bf16): E1 between 4.64e-3 (`zhang+layernorm`) and 7.44e-3 (`glu`, weight-normalised); Es equal to E1 to the
printed digits for every recipe, and the three schedules gave the same bits (printed, not gated); with resets 0.51 to 1.11 (the table
is in DESIGN.md section 39.3).
"""
import numpy as np
import pytest
import torch

import cnn_stream_reference as ref

pytestmark = pytest.mark.gpu

V, B, T = ref.V, 4, 41
X_LEN = [41, 29, 5, 36]                    # slot 2 is shorter than most chunks
SEED = 11
MUTANT_BAR = 0.05                          # tests/test_cnn_stream_cpu.py: every broken carry is farther off than this


def _build(device, recipe):
    """the recipe's model on the device, sized by one call, its convolution weights and biases redrawn; the features"""
    from asr.model.architectures import build_model
    from oracle import model as omodel
    arch, nconv, wn = recipe
    torch.manual_seed(SEED)
    cfg = ref.config(arch, nconv, wn)
    model = build_model(cfg).to_gpu()
    x = omodel.synthetic_batch(B, T, V, Lmin=3, Lmax=9, seed=0, ragged=True)[0]
    with torch.no_grad():
        model(x.to(device))                 # lazily sized parameters; data-dependent weight-norm initialisation of g and b
        drawn = ref.redraw({k: v.detach().cpu() for k, v in model.named_parameters()}, SEED)
        for name, p in model.named_parameters():
            p.copy_(drawn[name].to(device))
    return cfg, model, x


def _yardstick(device, recipe, cfg, model, x):
    """the oracle's logits (valid frames per slot) with the model's parameters as they are now, and E1 of the one-shot forward"""
    from oracle import cnn as ocnn
    with torch.no_grad():
        one = model(x.to(device), split_into_variables=False).float().cpu()                     # (B, T, V)
        params = {k: v.detach().float().cpu() for k, v in model.named_parameters()}
        # the VALUE of a weight-normalised W as the device formed it (tests/test_model_gpu.py does the same)
        weights = {name: mod.W.detach().float().cpu() for name, mod in model.named_modules() if hasattr(mod, "V") and hasattr(mod, "g")}
        assert bool(weights) == recipe[2]
        want = ocnn.logits_tbv(ocnn.forward(recipe[0], cfg, params, x, matched=False, weights=weights)).detach()
    want = [want[:n, b] for b, n in enumerate(X_LEN)]
    return want, ref.rel([one[b, :n] for b, n in enumerate(X_LEN)], want)


_CACHE = {}


def _setup(device, recipe):
    if recipe not in _CACHE:
        cfg, model, x = _build(device, recipe)
        want, E1 = _yardstick(device, recipe, cfg, model, x)
        _CACHE[recipe] = dict(cfg=cfg, model=model, x=x, want=want, E1=E1)
    return _CACHE[recipe]


def _feed(stream, x, calls, start=None, each=None, reset_between=False, Tc_of=None, watch=None):
    """run `calls` (per call: frames per slot, taken from x (B, C, H, T) at every slot's own position) -> per call
    (logits, lengths, n).  Rows of a chunk beyond a slot's share hold 9.0, which nothing may read.  watch: a slot whose carried
    tensors must come out of every call in which it gets no frame exactly as they went in."""
    pos = np.zeros(x.shape[0], dtype=np.int64) if start is None else np.array(start)
    out = []
    for i, n in enumerate(calls):
        Tc = int(n.max()) if Tc_of is None else Tc_of[i]
        chunk = ref.chunk_of(x, pos, n, Tc)
        pos += n
        if reset_between:
            stream.reset()
        before = [state[:, watch].clone() for _, state, _ in stream._ctx] if watch is not None and n[watch] == 0 else None
        logits, lengths = stream.advance(chunk.to(stream.device), n.astype(np.int32))
        assert tuple(logits.shape) == (Tc, x.shape[0], V) and logits.dtype == torch.float32 and lengths.dtype == torch.int32
        assert lengths.cpu().tolist() == n.tolist()                                             # delay 0: what goes in comes out
        if before is not None:
            assert len(before) > 0 and all(torch.equal(state[:, watch], was) for (_, state, _), was in zip(stream._ctx, before))
        if each is not None:
            each(logits, lengths)
        out.append((logits, lengths, n))
    return out


def _per_slot(outs):
    """the valid rows of every call, concatenated per slot"""
    nslots = outs[0][0].shape[1]
    lens = [o[1].cpu().tolist() for o in outs]
    return [torch.cat([o[0][:l[b], b] for o, l in zip(outs, lens)]).cpu() for b in range(nslots)]


def _under_the_schedules(model, x, want, E1, tag):
    """items (1) and (2) for one model: every schedule within 2 E1 of the oracle, 2 E1 below the mutants, the bookkeeping"""
    from asr.model.stream import AcousticStream
    got, Es = {}, {}
    for kind in ("whole", "single", "ragged"):
        s = AcousticStream(model, B, max_chunk=64)
        assert s.delay == 0
        outs = _feed(s, x, ref.schedule(kind, X_LEN))
        assert s.frames.cpu().tolist() == X_LEN
        tail, tail_len = s.flush()
        assert tuple(tail.shape) == (0, B, V) and tail_len.cpu().tolist() == [0] * B and s.frames.cpu().tolist() == X_LEN
        got[kind] = _per_slot(outs)
        assert [g.shape[0] for g in got[kind]] == X_LEN
        Es[kind] = ref.rel(got[kind], want)
    s = AcousticStream(model, B, max_chunk=64)
    bad = ref.rel(_per_slot(_feed(s, x, ref.schedule("ragged", X_LEN), reset_between=True)), want)
    diff = max(float((a - b).abs().max()) for k in ("single", "ragged") for a, b in zip(got["whole"], got[k]))
    same = all(torch.equal(a, b) for k in ("single", "ragged") for a, b in zip(got["whole"], got[k]))
    print("cnn stream %s: E1 %.4e  Es whole %.4e single %.4e ragged %.4e  with resets %.4e  | cut schedules differ by at most %.3e (%s)"
          % (tag, E1, Es["whole"], Es["single"], Es["ragged"], bad, diff, "the same bits" if same else "not the same bits"))
    for kind in Es:
        assert Es[kind] <= 2 * E1, (kind, Es[kind], E1)
    assert 2 * E1 < MUTANT_BAR, E1
    assert bad > 2 * E1, "the bar cannot tell a stream that forgets its carry from one that keeps it"
    return got


@pytest.mark.parametrize("recipe", ref.RECIPES, ids=ref.recipe_id)
def test_against_the_oracle(device, recipe):
    s0 = _setup(device, recipe)
    _under_the_schedules(s0["model"], s0["x"], s0["want"], s0["E1"], ref.recipe_id(recipe))


@pytest.mark.parametrize("recipe", [("zhang+residual", 4, False), ("glu", 2, False)], ids=ref.recipe_id)
def test_slots_are_independent(device, recipe):
    """slot 2 ends its utterance in the middle and starts another one while the others go on: they do not notice, the new utterance
    comes out as it does from a fresh stream, and a slot that gets no frame keeps every carried byte"""
    from asr.model.stream import AcousticStream
    from oracle import model as omodel
    s0 = _setup(device, recipe)
    x, model = s0["x"], s0["model"]
    second = omodel.synthetic_batch(B, 17, V, Lmin=3, Lmax=9, seed=5)[0]        # slot 2's second utterance: 17 frames
    calls = ref.schedule("ragged", X_LEN, seed=1)
    cut = next(i for i in range(len(calls)) if sum(c[2] for c in calls[:i + 1]) == X_LEN[2]) + 1     # slot 2 is through after `cut` calls
    assert cut < len(calls) - 3
    mask = [0, 0, 1, 0]
    # run A: with the restart
    a = AcousticStream(model, B, max_chunk=64)
    outs_a = _feed(a, x, calls[:cut], watch=2)
    tail = a.flush(mask)
    assert tail[0].shape[0] == 0 and tail[1].cpu().tolist() == [0] * B and a.frames.cpu().tolist()[2] == X_LEN[2]
    assert all(bool((state[:, 2] == 0).all()) and bool((state[:, 0] != 0).any()) for _, state, _ in a._ctx)
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
    outs_a2 = _feed(a, xa, rest, start=pos, watch=2)
    assert a.frames.cpu().tolist() == [X_LEN[0], X_LEN[1], 17, X_LEN[3]]
    # run B: slot 2 just stays idle after its first utterance
    b = AcousticStream(model, B, max_chunk=64)
    idle = [np.array([c[0], c[1], 0, c[3]]) for c in rest]
    outs_b = _feed(b, x, calls[:cut]) + _feed(b, x, idle, start=np.sum(calls[:cut], axis=0), Tc_of=[int(c.max()) for c in rest], watch=2)
    for (la, na, _), (lb, nb, _) in zip(outs_a + outs_a2, outs_b):
        na, nb = na.cpu().tolist(), nb.cpu().tolist()
        for slot in (0, 1, 3):
            assert na[slot] == nb[slot] and torch.equal(la[:na[slot], slot], lb[:nb[slot], slot])
    # run C: the second utterance alone in a fresh stream, cut the same way
    c = AcousticStream(model, B, max_chunk=64)
    alone = [np.array([0, 0, r[2], 0]) for r in rest]
    outs_c = _feed(c, xa, alone, Tc_of=[int(r.max()) for r in rest], watch=0)
    got_a, got_c = _per_slot(outs_a2)[2], _per_slot(outs_c)[2]
    assert got_a.shape[0] == 17 and torch.equal(got_a, got_c)


def test_weight_normalisation_waits_for_refresh(device):
    """the W of a weight-normalised layer is formed at construction: a new g shows only after refresh(), and then the stream is as
    close to the oracle of the NEW parameters as the one-shot forward is"""
    from asr import nn
    from asr.model.stream import AcousticStream
    recipe = ("zhang+residual", 3, True)
    cfg, model, x = _build(device, recipe)
    calls = ref.schedule("ragged", X_LEN)
    s = AcousticStream(model, B, max_chunk=64)
    before = _per_slot(_feed(s, x, calls))
    layers = [m for m in model.modules() if isinstance(m, nn.WeightnormConvolution2D)]
    assert len(layers) == 7                     # 4 carrying convolutions, the 2 dense ones and the projection
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for layer in layers:
            layer.g.mul_((0.6 + 0.8 * torch.rand(layer.g.shape, generator=gen)).to(device))
    s.reset()
    stale = _per_slot(_feed(s, x, calls))
    assert all(torch.equal(a, b) for a, b in zip(before, stale))
    s.refresh()
    s.reset()
    fresh = _per_slot(_feed(s, x, calls))
    want, E1 = _yardstick(device, recipe, cfg, model, x)
    moved, Es = ref.rel(before, want), ref.rel(fresh, want)
    print("cnn stream weightnorm: new g, E1 %.4e, stream before refresh %.4e, after %.4e" % (E1, moved, Es))
    assert Es <= 2 * E1 and 2 * E1 < MUTANT_BAR and moved > 2 * E1
    _under_the_schedules(model, x, want, E1, "zhang+residual-3-wn with the new g")       # (fresh streams see the new g as well)


def test_the_stream_feeds_the_decoders(device):
    """(logits, lengths) of every advance go as they are into a BeamStream and a KeywordStream: bit for bit the one-shot beam
    search / keyword search of the concatenated stream logits"""
    from asr import error, spot
    from asr.model.stream import AcousticStream
    s0 = _setup(device, ("zhang+residual", 4, False))
    kws = spot.KeywordSet([(3, 4), (5,), (7, 8, 9), (2, 2)], V)
    beam = error.BeamStream(B, V, max_frames=256, beam_width=8, top_k=8)
    spotter = spot.KeywordStream(B, V, kws, device)
    dets = []

    def each(logits, lengths):
        beam.advance(logits, lengths)
        dets.append((spotter.advance(logits, lengths), lengths.cpu().tolist()))

    s = AcousticStream(s0["model"], B, max_chunk=64)
    outs = _feed(s, s0["x"], ref.schedule("ragged", X_LEN, seed=2), each=each)
    assert s.flush()[0].shape[0] == 0             # delay 0: nothing is held back, the decoders have seen every frame
    got = _per_slot(outs)
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


def test_from_samples_to_hypotheses(device):
    """int16 samples -> FeatureStream -> AcousticStream (cnn) -> BeamStream in chunks of 800 samples, against an equal stream fed the
    ``Processor.logfbank_batch`` features under the same cuts: logits and hypotheses bit for bit"""
    import test_feature_stream_gpu as tfs
    from asr import error
    from asr.model.stream import AcousticStream
    assert tfs.B == B
    model = _setup(device, ("glu", 2, False))["model"]
    want, xl, _ = tfs._oneshot(device, "long", False)
    fs = tfs._stream(device, 800, False)
    feats = tfs._feed(fs, tfs._signals("long"), tfs._schedule(800, tfs.BATCHES["long"]))
    feats.append(fs.flush())

    def run(chunks):
        ac = AcousticStream(model, B, max_chunk=64)
        beam = error.BeamStream(B, V, max_frames=256, beam_width=8, top_k=8)
        outs = []
        for x, lengths in chunks:
            logits, ll = ac.advance(x, lengths)
            assert torch.equal(ll, lengths)
            beam.advance(logits, ll)
            outs.append((logits, ll))
        assert ac.flush()[0].shape[0] == 0 and ac.frames.cpu().tolist() == xl
        return outs, beam.result()

    outs_s, hyp_s = run(feats)
    cut, pos = [], [0] * B
    for x, lengths in feats:                                                     # the one-shot features in the same chunks
        same = torch.zeros_like(x)
        for b, l in enumerate(lengths.cpu().tolist()):
            same[b, :, :, :l] = want[b][:, :, pos[b]:pos[b] + l].to(device)
            pos[b] += l
        cut.append((same, lengths.clone()))
    assert pos == xl and max(xl) > 20
    outs_r, hyp_r = run(cut)
    for (ls, ns), (lr, nr) in zip(outs_s, outs_r):
        ns, nr = ns.cpu().tolist(), nr.cpu().tolist()
        assert ns == nr
        for b in range(B):
            assert torch.equal(ls[:ns[b], b], lr[:nr[b], b])
    for s, r in zip(hyp_s, hyp_r):
        assert torch.equal(s, r)


def test_refusals(device):
    from asr.model.architectures import build_model
    from asr.model.stream import AcousticStream
    s0 = _setup(device, ("zhang", 3, False))
    s = AcousticStream(s0["model"], B, max_chunk=8)
    x = s0["x"].to(device)
    with pytest.raises(ValueError):
        s.advance(x[:, :, :, :9])                                               # longer than max_chunk
    with pytest.raises(ValueError):
        s.advance(x[:3, :, :, :4])                                              # wrong B
    with pytest.raises(ValueError):
        s.advance(x[:, :, :39, :4])                                             # not the model's features
    with pytest.raises(ValueError):
        s.advance(x[:, :2, :, :4])
    with pytest.raises(ValueError):
        s.advance(x[:, :, :, :4], [4, 5, 0, 1])                                 # a length above Tc
    assert s.frames.cpu().tolist() == [0] * B                                   # (nothing was consumed)
    assert all(bool((state == 0).all()) for _, state, _ in s._ctx)
    logits, lengths = s.advance(x[:, :, :, :0])                                 # an empty chunk touches nothing
    assert tuple(logits.shape) == (0, B, V) and lengths.cpu().tolist() == [0] * B
    for recipe in (("zhang", 3, False), ("glu", 2, True)):
        with pytest.raises(ValueError, match="run it once or load it"):
            AcousticStream(build_model(ref.config(*recipe)).to_gpu(), B)        # never called: its lazy parameters have no size
