"""Host side of the streaming forward (asr/model/stream.py): what ``stream_plan`` says a stream carries, which models it refuses,
and that the lookahead layer moves no existing parameter name.  No GPU."""
import pytest


def _ds2_small(**fields):
    from asr.model import ds2
    cfg = ds2.configure()
    cfg.vocab_size, cfg.ndim_conv, cfg.ndim_rnn, cfg.ndim_dense, cfg.num_rnn_layers = 17, 8, 32, 16, 2
    for name, value in fields.items():
        assert hasattr(cfg, name), name
        setattr(cfg, name, value)
    return cfg, ds2.Model(cfg)


def test_plan_of_the_default_stack():
    from asr.model.stream import stream_plan
    cfg, model = _ds2_small(bidirectional=False, lookahead=5)
    plan = stream_plan(model)
    assert plan["delay"] == 5
    kinds = [e["kind"] for e in plan["layers"]]
    assert kinds == ["context", "context", "state", "state", "lookahead"]
    c1, c2, g1, g2, la = plan["layers"]
    # block 1 reads the features: 40 mel rows x 3 channels, kernel (3, 5); block 2 what Maxout and MaxPooling((3, 1)) leave of the
    # 38 rows x 16 channels of block 1: ceil(38 / 3) = 13 rows x 8 channels
    assert (c1["K"], c1["height"], c1["channels"], c1["R"]) == (4, 40, 3, 120)
    assert (c2["K"], c2["height"], c2["channels"], c2["R"]) == (4, 13, 8, 104)
    assert model.conv_blocks.layers[c1["index"]] is model.conv_blocks._sequential_0
    assert model.conv_blocks.layers[c2["index"]] is model.conv_blocks._sequential_4
    assert g1["H"] == g2["H"] == 32 and [model.rnn_blocks.layers[g["index"]] for g in (g1, g2)] == \
        [model.rnn_blocks._sequential_0, model.rnn_blocks._sequential_2]
    assert (la["K"], la["R"]) == (5, 32)


def test_plan_follows_the_configuration():
    from asr.model.stream import stream_plan
    cfg, model = _ds2_small(bidirectional=False, kernel_size=(5, 3), num_conv_layers=3, num_rnn_layers=1, num_mel_filters=48)
    plan = stream_plan(model)
    assert plan["delay"] == 0 and [e["kind"] for e in plan["layers"]] == ["context"] * 3 + ["state"]
    # heights: 48 -> conv 44 -> pool 3: 15 -> conv 11 -> pool 2: 6 -> conv 2 -> pool 2: 1
    assert [(e["K"], e["height"], e["channels"]) for e in plan["layers"][:3]] == [(2, 48, 3), (2, 15, 8), (2, 6, 8)]
    assert [e["R"] for e in plan["layers"][:3]] == [144, 120, 48]
    assert model._merged == (8, 1)


def test_the_conv_stack_is_planned_by_the_shared_walker():
    """the conv stack of a ds2.Model goes through the walker that plans the layers of a cnn.AcousticModel: the plan's context
    entries are its result on conv_blocks.layers, and they carry its keys ("path", "pad_h")"""
    from asr.model.stream import _walk_layers, stream_plan
    for fields in (dict(lookahead=5), dict(kernel_size=(5, 3), num_conv_layers=3, num_mel_filters=48, time_reduction=2)):
        cfg, model = _ds2_small(bidirectional=False, **fields)
        plan = stream_plan(model)
        contexts = [e for e in plan["layers"] if e["kind"] not in ("stack", "state", "lookahead")]
        assert len(contexts) == cfg.num_conv_layers
        assert all(e["kind"] == "context" and e["path"] == (e["index"],) and e["pad_h"] == 0 for e in contexts)
        entries, height, channels = _walk_layers(model.conv_blocks.layers, cfg.num_mel_filters, cfg.ndim_audio_features)
        assert contexts == entries and (channels, height) == model._merged


def _swap_conv_layer(model, index, layer):
    """put `layer` where conv_blocks.layers[index] is, in the list and under the registered name"""
    layers = list(model.conv_blocks.layers)
    layers[index] = layer
    model.conv_blocks.layers = layers
    setattr(model.conv_blocks, "_sequential_%d" % index, layer)


def test_a_conv_stack_that_pools_over_time_is_refused():
    from asr import nn
    from asr.model.stream import stream_plan
    cfg, model = _ds2_small(bidirectional=False)
    assert type(model.conv_blocks.layers[3]).__name__ == "MaxPooling2D"
    stream_plan(model)
    _swap_conv_layer(model, 3, nn.MaxPooling2D((2, 2)))
    with pytest.raises(ValueError, match="no streaming form of MaxPooling2D"):
        stream_plan(model)


def test_a_conv_stack_that_looks_ahead_is_refused():
    from asr.model.stream import stream_plan
    cfg, model = _ds2_small(bidirectional=False)
    model.conv_blocks.layers[0].causal = False
    with pytest.raises(ValueError, match="not causal"):
        stream_plan(model)


def test_a_bidirectional_model_is_refused():
    from asr.model.stream import AcousticStream, stream_plan
    cfg, model = _ds2_small()
    with pytest.raises(ValueError):
        stream_plan(model)
    with pytest.raises(ValueError):
        AcousticStream(model, 2, device="cpu")


def test_only_ds2_models_are_planned():
    from asr import nn
    from asr.model.stream import stream_plan
    with pytest.raises(ValueError):
        stream_plan(nn.Module())


def test_lookahead_moves_no_parameter_name():
    cfg, plain = _ds2_small(bidirectional=False)
    cfg0, zero = _ds2_small(bidirectional=False, lookahead=0)
    cfg3, look = _ds2_small(bidirectional=False, lookahead=3)
    today = ["conv_blocks._sequential_0.W", "conv_blocks._sequential_0.b", "conv_blocks._sequential_4.W", "conv_blocks._sequential_4.b",
             "rnn_blocks._sequential_0.w_ih", "rnn_blocks._sequential_0.w_hh", "rnn_blocks._sequential_0.b_ih",
             "rnn_blocks._sequential_0.b_hh", "rnn_blocks._sequential_2.w_ih", "rnn_blocks._sequential_2.w_hh",
             "rnn_blocks._sequential_2.b_ih", "rnn_blocks._sequential_2.b_hh", "dense_blocks._sequential_0.W",
             "dense_blocks._sequential_0.b", "dense_blocks._sequential_3.W", "dense_blocks._sequential_3.b",
             "dense_blocks._sequential_6.W", "dense_blocks._sequential_6.b", "dense_blocks._sequential_7.norm.gamma",
             "dense_blocks._sequential_7.norm.beta"]
    assert list(plain.state_dict().keys()) == list(zero.state_dict().keys()) and sorted(plain.state_dict().keys()) == sorted(today)
    assert not hasattr(zero, "lookahead")
    keys = list(look.state_dict().keys())
    assert [k for k in keys if k != "lookahead.W"] == list(plain.state_dict().keys()) and "lookahead.W" in keys
    w = look.state_dict()["lookahead.W"]
    assert tuple(w.shape) == (32, 4) and bool((w[:, 0] == 1).all()) and bool((w[:, 1:] == 0).all())
    for key, value in plain.state_dict().items():                                   # (the old parameters keep their shapes too)
        assert look.state_dict()[key].shape == value.shape
