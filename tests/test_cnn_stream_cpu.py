"""Host side of the streaming forward of the convolutional recipes (asr/model/stream.py over a cnn.AcousticModel): what
``stream_plan`` says such a stream carries and which containers it refuses; that the float64 restatement of the chunked forward
(tests/cnn_stream_reference.py) is ``oracle.cnn.forward``; and that a bar of 0.05 relative L2 tells a broken carry from a whole
one.  No GPU.

(3) measured here: at most 7e-16 under every cut schedule.  (4) measured here with B = 3, T = 37 and the redrawn parameters, the
smallest mutant distance per recipe: carry dropped 0.070 (`zhang+residual`, wide branch) to 0.44, carry a frame late 0.056 (the
same recipe) to 0.49; the test prints every one.
"""
import pytest
import torch

import cnn_stream_reference as ref

ARCHITECTURES = ("zhang", "zhang+fc_relu", "zhang+residual", "zhang+layernorm", "glu", "relu+layernorm", "relu+layernorm+residual")
PLAIN = [r for r in ref.RECIPES if not r[2]]
B, T = 3, 37
X_LEN = [37, 22, 30]
SEED = 11
MUTANT_BAR = 0.05


def _model(arch, nconv, wn=False):
    from asr.model.architectures import build_model
    cfg = ref.config(arch, nconv, wn)
    return cfg, build_model(cfg)


def _resolve(model, path):
    from asr import nn
    layer = model.layers[path[0]]
    if len(path) == 2:
        assert isinstance(layer, nn.Residual)
        layer = layer.layers[path[1]]
    return layer.W if isinstance(layer, nn.GLU) else layer


# ------------------------------------------------------------------------------------------------------------------------ 1. the plan
def _expected_entries(arch, nconv):
    """[(height, channels, inside a Residual, a GLU)] of the carrying convolutions, from the recipes as run/ctc/cnn/model.py has them:
    the first reads 40 mel rows x 3 channels, every later one the 13 rows MaxPooling2D((3, 1)) leaves of the first's 38"""
    h = 16
    out = [(40, 3, False, False)]
    if arch in ("zhang", "zhang+fc_relu", "zhang+residual"):
        narrow, wide = min(nconv, 4), max(0, nconv - 4)
        res = arch == "zhang+residual"
        out += [(13, h, res and idx != narrow - 1, False) for idx in range(narrow)]
        out += [(13, 2 * h, res, False) for _ in range(narrow if wide else 0)]
    elif arch == "glu":
        out += [(13, h, False, True)] * nconv
    else:
        out += [(13, h, arch == "relu+layernorm+residual", False)] * nconv
    return out


@pytest.mark.parametrize("wn", [False, True])
@pytest.mark.parametrize("nconv", [2, 5])
@pytest.mark.parametrize("arch", ARCHITECTURES)
def test_plan(arch, nconv, wn):
    from asr import nn
    from asr.model.stream import stream_plan
    cfg, model = _model(arch, nconv, wn)
    plan = stream_plan(model)
    assert sorted(plan) == ["delay", "layers"] and plan["delay"] == 0
    want = _expected_entries(arch, nconv)
    assert len(plan["layers"]) == len(want)
    assert plan["layers"][0]["R"] == 120
    last = -1
    for e, (height, channels, inner, gated) in zip(plan["layers"], want):
        assert e["kind"] == "context" and e["K"] == 4
        assert (e["height"], e["channels"], e["R"]) == (height, channels, height * channels)
        assert e["pad_h"] == (0 if height == 40 else 1)
        assert e["path"][0] == e["index"] and len(e["path"]) == (2 if inner else 1) and e["index"] > last
        last = e["index"]
        layer = model.layers[e["index"]]
        assert isinstance(layer, nn.Residual) == inner and isinstance(layer, nn.GLU) == gated
        conv = _resolve(model, e["path"])
        assert isinstance(conv, nn.WeightnormConvolution2D if wn else nn.PlainConvolution2D) and conv.ksize == (3, 5)
        # the very object the model registered under the checkpoint's name
        assert conv is getattr(model, "layer_" + "_".join(str(i) for i in e["path"]))
    if arch == "glu":
        assert all(isinstance(model.layers[e["index"]], nn.GLU) for e in plan["layers"][1:])
    if arch in ("zhang+residual", "relu+layernorm+residual"):
        assert sum(len(e["path"]) == 2 for e in plan["layers"]) >= 1


def test_plan_follows_the_configuration():
    """another kernel width, another number of mel rows: K = kw - 1, heights from the configuration"""
    from asr.model.architectures import build_model
    from asr.model.stream import stream_plan
    cfg = ref.config("zhang", 2)
    cfg.kernel_size, cfg.num_mel_filters = (3, 3), 47
    plan = stream_plan(build_model(cfg))
    assert [(e["K"], e["height"], e["channels"], e["R"]) for e in plan["layers"]] == [(2, 47, 3, 141), (2, 15, 16, 240), (2, 15, 16, 240)]


# ------------------------------------------------------------------------------------------------------------------------ 2. refusals
def _container(*layers):
    from asr.model.cnn import AcousticModel
    model = AcousticModel()
    model.layer(*layers)
    return model


def test_refusals():
    from asr import nn
    from asr.model.cnn import AcousticModel
    from asr.model.stream import stream_plan
    head = lambda: nn.Convolution2D(3, 8, (3, 5), pad=(0, 4), causal=True)
    assert len(stream_plan(_container(head()))["layers"]) == 1
    with pytest.raises(ValueError, match="not causal"):
        stream_plan(_container(nn.Convolution2D(3, 8, (3, 5), pad=(0, 2))))                     # symmetric time padding
    with pytest.raises(ValueError, match="not causal"):
        stream_plan(_container(nn.Convolution2D(3, 8, (3, 5), pad=(0, 4))))                     # padded as a causal one, never cropped
    with pytest.raises(ValueError, match="not causal"):
        stream_plan(_container(head(), nn.GLU(8, 8, (3, 5), pad=(1, 2))))
    with pytest.raises(ValueError, match="no streaming form of BatchNormalization"):
        stream_plan(_container(head(), nn.BatchNormalization(8)))
    with pytest.raises(ValueError, match="no streaming form of GRU"):
        stream_plan(_container(head(), nn.GRU(8, 8)))
    with pytest.raises(ValueError, match="no streaming form"):
        stream_plan(_container(head(), nn.Residual(nn.Convolution2D(8, 16, (3, 5), pad=(1, 4), causal=True))))     # changes the shape
    with pytest.raises(ValueError, match="no streaming form"):
        stream_plan(_container(head(), nn.MaxPooling2D((2, 2))))                                # pools over time
    with pytest.raises(ValueError):
        stream_plan(AcousticModel())                                                             # empty
    with pytest.raises(ValueError):
        stream_plan(nn.Module())


# ------------------------------------------------------------------------------------- 3. the restatement is oracle.cnn.forward
_CACHE = {}


def _setup(recipe):
    """parameters, input and the float64 logits of the whole utterances (valid frames per slot) -- once per recipe"""
    if recipe not in _CACHE:
        from oracle import cnn as ocnn
        arch, nconv, _ = recipe
        cfg = ref.config(arch, nconv)
        params = ref.host_params(arch, cfg, SEED)
        x = torch.randn((B, 3, 40, T), generator=torch.Generator().manual_seed(SEED + 1), dtype=torch.float64)
        full = ocnn.logits_tbv(ocnn.forward(arch, cfg, params, x))                              # (T, B, V)
        _CACHE[recipe] = dict(cfg=cfg, params=params, x=x, want=[full[:n, b] for b, n in enumerate(X_LEN)])
    return _CACHE[recipe]


@pytest.mark.parametrize("recipe", PLAIN, ids=ref.recipe_id)
def test_the_restatement_is_the_oracle(recipe):
    s = _setup(recipe)
    for kind in ("whole", "single", "ragged"):
        calls = ref.schedule(kind, X_LEN)
        if kind == "ragged":
            assert any(0 in c.tolist() for c in calls) and max(int(c.max()) for c in calls) <= 7
        got = ref.run_schedule(ref.Stream(recipe[0], s["cfg"], s["params"], B), s["x"], calls)
        assert [g.shape[0] for g in got] == X_LEN
        err = ref.rel(got, s["want"])
        print("cnn stream restatement %s %s: %.2e" % (ref.recipe_id(recipe), kind, err))
        assert err < 1e-12, (kind, err)


# ------------------------------------------------------------------------------------------------------------ 4. the bar can tell
@pytest.mark.parametrize("recipe", PLAIN, ids=ref.recipe_id)
def test_a_broken_carry_is_seen(recipe):
    s = _setup(recipe)
    calls = ref.schedule("ragged", X_LEN)
    ncarry = len(ref.Stream(recipe[0], s["cfg"], s["params"], B).carrying)
    assert ncarry == len(_expected_entries(recipe[0], recipe[1]))
    dist = {}
    for kind in ("drop", "shift"):
        for j in range(ncarry):
            mutant = ref.Stream(recipe[0], s["cfg"], s["params"], B, mutant=(kind, j))
            dist[kind, j] = ref.rel(ref.run_schedule(mutant, s["x"], calls), s["want"])
    print("cnn stream mutants %s: dropped %s | a frame late %s" % (
        ref.recipe_id(recipe), " ".join("%.3f" % dist["drop", j] for j in range(ncarry)),
        " ".join("%.3f" % dist["shift", j] for j in range(ncarry))))
    for key, d in dist.items():
        assert d > MUTANT_BAR, (key, d)
