"""Streaming forward of a causal acoustic model: features in chunk by chunk, logits out chunk by chunk, all state on the device.

Two families of models are causal end to end and can be streamed (``stream_plan`` says what each of them carries):

A ``ds2.Model`` with ``bidirectional=False``: causal convolutions, pooling over height only, forward GRUs, per-frame dense layers
and LayerNormalization, and the only subsampling in time is frame stacking (``time_reduction`` = k: k frames in, one out), which is
causal too.  What has to be carried from one chunk to the next is small and local: the last kw - 1 input rows of every convolution,
the up to k - 1 frames of a group not yet complete, the hidden state of every GRU layer, and the pending frames of the lookahead
convolution, whose ``lookahead`` frames are the stream's delay.  A bidirectional model streams when it was built with
``latency_control`` = (Nc, Nr): its reverse directions restart per block of Nc frames and see Nr frames beyond it, so a layer holds
back at most Nc + Nr - 1 frames (``_blocks``; csrc/lc_window.hip).

The seven convolutional recipes of architectures.py (``cnn.AcousticModel``, what ``build_model`` returns): every
time-padded convolution is pad_t = kw - 1 followed by the crop (``nn.GLU`` pads and crops itself), pooling runs over height only, the
4-d LayerNormalization takes its statistics over (C, H) of one frame and the residual adds are per frame.  There is no recurrence and
no lookahead: the carry is the last kw - 1 input rows of every convolution wider than one frame, and the delay is 0.

Both families go through the same code: ``_walk_layers`` plans the convolutional front of either, a
``_StreamedConvolution`` stands in for each of its carrying convolutions in the layer list that ``nn.nn._apply_layers`` runs on every
chunk, and what a ds2.Model has behind that front (frame stacking, recurrences, lookahead, dense layers) a recipe simply has not.

The carry kernels are csrc/stream.hip and csrc/time_stack.hip; every other launch is the model's own.  ``(logits, lengths)`` go as they
are into ``asr.error.BeamStream.advance``, ``asr.error.GramBeamStream.advance`` and ``asr.spot.KeywordStream.advance``.

The features come chunk by chunk from ``asr.fft.FeatureStream``: its ``(x, lengths)`` go as they are into
``advance``, with ``max_chunk >= FeatureStream.max_frames``.

A ``ds2.Model`` with ``rnn="sru"`` and ``bidirectional=False`` streams the same way: an ``nn.SeqSRU`` layer
carries its cell state, (1, B, D) float32 per layer, and a chunk is one projection and one scan per layer whatever its frame count.

Not covered: ``nn.SRU`` itself (the reference's link has no per-slot lengths and its reference model drops the recurrent output), a
bidirectional SRU stack, and a backward pass through a stream.
"""
import torch

from .. import _ops, functions, nn
from ..link import Link
from . import ds2
from ._acoustic import AcousticCall, mark_logit_layers


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _name(layer):
    return getattr(layer, "__name__", None) or type(layer).__name__


def _convolution_of(layer):
    """(the convolution link of a layer, whether a GLU wraps it), or (None, False)"""
    if isinstance(layer, nn.GLU):
        return layer.W, True
    if isinstance(layer, (nn.PlainConvolution2D, nn.WeightnormConvolution2D)):
        return layer, False
    return None, False


def _walk_layers(layers, height, channels, outer=()):
    """The one structural walk, for the layers of a cnn.AcousticModel and for the conv stack of a ds2.Model: from the (height,
    channels) that enter `layers` -> (the "context" entries, height, channels behind the last layer).  ValueError for whatever
    has no per-frame form.  `outer`: the path of the Residual whose layers these are."""
    entries = []
    for index, layer in enumerate(layers):
        path = outer + (index,)
        at = "_".join(str(i) for i in path)
        where = "layer %s (%s)" % (at, _name(layer))
        conv, gated = _convolution_of(layer)
        if conv is not None:
            (kh, kw), (pad_h, pad_t) = conv.ksize, conv.pad
            if kw > 1:
                if pad_t != kw - 1 or not (gated or conv.causal):
                    raise ValueError("%s is not causal: a stream needs pad_t = kw - 1 and the crop behind it" % where)
                entries.append({"kind": "context", "K": kw - 1, "R": height * channels, "height": height, "channels": channels,
                                "index": path[0], "path": path, "pad_h": pad_h})
            elif pad_t != 0:
                raise ValueError("%s pads the time axis of a one-frame kernel" % where)
            height, channels = height + 2 * pad_h - kh + 1, conv.out_channels // 2 if gated else conv.out_channels
            if height < 1:
                raise ValueError("%s is higher than its input" % where)
        elif _name(layer) == "Maxout":
            if not isinstance(layer.pool_size, int) or channels % layer.pool_size:
                raise ValueError("no streaming form of Maxout(%r) over %d channels" % (layer.pool_size, channels))
            channels //= layer.pool_size
        elif _name(layer) == "MaxPooling2D":
            ks = _pair(layer.ksize)
            if len(ks) != 2 or ks[1] != 1 or layer.stride is not None or layer.pad not in (0, (0, 0)):
                raise ValueError("no streaming form of MaxPooling2D(%r): a stream pools over height only" % (layer.ksize,))
            height = _ops.pooled_height(height, ks[0])
        elif isinstance(layer, nn.Residual):
            if outer:
                raise ValueError("no streaming form of a Residual inside a Residual")
            inner, h, c = _walk_layers(layer.layers, height, channels, path)
            if (h, c) != (height, channels):
                raise ValueError("no streaming form of the Residual at layer %d: it turns (height, channels) = %s into %s"
                                 % (index, (height, channels), (h, c)))
            entries += inner
        elif not (getattr(layer, "_asr_identity", False) or layer is functions.relu or _name(layer) == "Dropout"
                  or isinstance(layer, nn.LayerNormalization)):
            raise ValueError("no streaming form of %s (layer %s)" % (_name(layer), at))
    return entries, height, channels


def _front(model):
    """the layers in front of whatever else a stream runs: all of a cnn.AcousticModel, the conv stack of a ds2.Model"""
    if isinstance(model, ds2.Model):
        return model.conv_blocks
    if isinstance(model, AcousticCall) and isinstance(model, nn.Stream):
        return model
    raise ValueError("a stream runs a ds2.Model or a cnn.AcousticModel, got %s" % type(model).__name__)


def _walk(model):
    """_walk_layers over the front of `model`, from the features' (height, channels)"""
    layers = _front(model).layers
    convs = (_convolution_of(sub)[0] for layer in layers for sub in (layer.layers if isinstance(layer, nn.Residual) else (layer,)))
    first = next((conv for conv in convs if conv is not None), None)
    master = None if first is None else (first.V if isinstance(first, nn.WeightnormConvolution2D) else first.W)
    if master is None or master.dim() != 4:
        raise ValueError("no streaming form of %s: it has no sized convolution that says how many channels the features have"
                         % type(model).__name__)
    # (both model builders record the configuration's num_mel_filters; a container filled by hand gets the front end's default of 40 rows)
    return _walk_layers(layers, getattr(model, "_input_height", 40), master.shape[1])


def stream_plan(model):
    """What a stream over `model` carries, layer by layer, from the model's structure alone (no device, no parameters read):
    {"delay": output frames the output lags the input, "layers": [...]} with one entry per carrying layer, in order:
      {"kind": "context", "K": kw - 1, "R": height * channels of the block's input, "height", "channels", "index": position in
       conv_blocks.layers, "path": (index,), "pad_h"}            a causal convolution's left context, K rows of R features
      {"kind": "stack", "K": k - 1, "R": height * channels of the conv stack's output, "k": k}      the frames of a group of
       k not yet complete (only with time_reduction = k > 1, and then the plan also has "time_reduction": k)
      {"kind": "state", "H": units, "index": position in rnn_blocks.layers}      a GRU layer's hidden state
      {"kind": "state", "H": units, "index": position in rnn_blocks.layers, "cell": "sru"}      an nn.SeqSRU layer's cell state
      {"kind": "lookahead", "K": lookahead, "R": features}                       the lookahead layer's pending frames
      {"kind": "lc", "H": units, "index": position in rnn_blocks.layers, "Nc": block, "Nr": right context, "K": Nc + Nr - 1,
       "R": the layer's input width}      a latency-controlled BiGRU layer: the forward direction's state and up to K pending
       input rows that wait for the right context of their block; "delay" is then the bound num_layers * K
    A ``cnn.AcousticModel`` (architectures.build_model) carries only convolution contexts, and its delay is 0: one "context" entry
    per convolution wider than one frame, as above with "index": position in model.layers and "path": (index,), or (index, inner)
    for a layer inside a Residual.  The convolution of a GLU is model.layers[index].W.
    ValueError: neither of the two, a ds2.Model with plain BiGRU or BiSeqSRU layers (their reverse recurrences need the whole utterance), or, in the layers
    of a cnn.AcousticModel as in the conv stack of a ds2.Model (_walk_layers walks both), a convolution that looks ahead in time or a
    layer without a per-frame form (pooling over time, BatchNormalization, a recurrent layer, a Residual that changes shape)."""
    layers, height, channels = _walk(model)
    if not isinstance(model, ds2.Model):
        return {"delay": 0, "layers": layers}
    k = getattr(model, "time_reduction", 1)
    if k > 1:
        layers.append({"kind": "stack", "K": k - 1, "R": height * channels, "k": k})
    delay, width = 0, k * height * channels
    for index, layer in enumerate(model.rnn_blocks.layers):
        if isinstance(layer, (nn.BiGRU, nn.BiSeqSRU)):
            raise ValueError("a bidirectional model cannot be streamed: its reverse recurrences start at the end of the utterance")
        if isinstance(layer, nn.LCBiGRU):
            K = layer.block + layer.right - 1
            layers.append({"kind": "lc", "H": layer.out_size, "index": index, "Nc": layer.block, "Nr": layer.right, "K": K, "R": width})
            delay += K
        if isinstance(layer, nn.GRU):
            layers.append({"kind": "state", "H": layer.out_size, "index": index})
        if isinstance(layer, nn.SeqSRU):
            layers.append({"kind": "state", "H": layer.out_size, "index": index, "cell": "sru"})
        width = getattr(layer, "out_size", width)
    look = getattr(model, "lookahead", None)
    kinds = {e["kind"] for e in layers}
    if "lc" in kinds and ("state" in kinds or look is not None):
        raise ValueError("no streaming form of latency-controlled recurrences beside forward-only ones or a lookahead layer")
    if look is not None:
        delay = look.lookahead
        layers.append({"kind": "lookahead", "K": delay, "R": look.W.shape[0]})
    plan = {"delay": delay, "layers": layers}
    if k > 1:
        plan["time_reduction"] = k
    return plan


class _ChunkLengths:
    """The valid frames per slot of the chunk that is running, (B) int32 on the device or None for all of them: ``advance`` fills
    it before the layer list runs, and the stand-ins of that list read it when they push."""
    n = None


class _StreamedConvolution:
    """Stands in an ``AcousticStream``'s layer list for one convolution (or GLU) of the model.  With `carry`, its own (plan entry,
    carried rows, window), it pushes its input rows and runs the layer's own convolution un-padded in time over [the K carried rows |
    the chunk], which is the causal convolution of the whole sequence; without one (a one-frame kernel) it is the layer itself.
    Either way the W of a weight-normalised layer, and through `link` the 16-bit matrices made from it, are the ones ``refresh``
    formed."""

    def __init__(self, conv, gated, carry, lengths):
        self.conv, self.gated, self.carry, self.lengths = conv, gated, carry, lengths
        self.derived = isinstance(conv, nn.WeightnormConvolution2D)
        self.refresh()

    def refresh(self):
        if self.derived:        # (a new link: its cache is keyed by the weight's address, which a freed W may hand to the next one)
            self.W, self.link = self.conv.W, Link()

    def _weight(self):
        return (self.W, self.link) if self.derived else (self.conv.W, self.conv)

    def _window(self, x):
        """the view of [carried rows | chunk] this layer reads, before it is filled"""
        entry, _, window = self.carry
        return functions.logical4(window[:entry["K"] + x.shape[3]].view(-1, window.shape[1], entry["height"], entry["channels"]))

    def _push(self, x):
        entry, state, window = self.carry
        Tc = x.shape[3]
        _ops.stream_push(state, None, functions.phys4(x).reshape(Tc, window.shape[1], entry["R"]), self.lengths.n,
                         window[:entry["K"] + Tc], _ops.STREAM_CONTEXT)

    def __call__(self, x):
        conv = self.conv
        W, link = self._weight()
        pad, causal = conv.pad, conv.causal
        if self.carry is not None:
            xw = self._window(x)
            self._push(x)
            x, pad, causal = xw, (conv.pad[0], 0), False
        y = functions.convolution_2d(x, W, conv.b, link, pad, causal, conv.output_float32)
        return functions.glu(y) if self.gated else y

    def fused_maxout_pool(self, x, k):
        """the model's first block as one pass, where the one-shot forward runs it as one (nn.nn._apply_layers); None: three layers"""
        conv = self.conv
        if self.carry is None or self.gated or conv.output_float32:
            return None
        W, link = self._weight()
        xw, pad = self._window(x), (conv.pad[0], 0)
        if not functions.convolution_maxout_pool_ok(xw, tuple(W.shape), pad, False, k):
            return None
        self._push(x)
        return functions.convolution_maxout_pool(xw, W, conv.b, link, pad, False, k)


class AcousticStream:
    """``model(x)`` of a causal ``ds2.Model``, or of a ``cnn.AcousticModel`` (the recipes of architectures.py), fed chunk by chunk,
    for `B` batch slots that start and end on their own:

        s = AcousticStream(model, B, max_chunk=64)
        for x, n in chunks:                             # x (B, C, n_mel, Tc) features, n (B): valid frames per slot (0: untouched)
            logits, lengths = s.advance(x, n)           # (To, B, V) f32 left-aligned per slot, (B) int32 on the device
            beam.advance(logits, lengths)
        logits, lengths = s.flush(mask)                 # end of utterance of the masked slots: the `delay` frames held back

    ``delay`` is the model's lookahead: a slot's first `delay` frames come out with later chunks or with ``flush``, which feeds
    the pending frames a zero future (as the one-shot forward does at an utterance's end) and then resets the slots.

    With ``time_reduction`` = k > 1 every k input frames give one output frame: To = ceil((k - 1 + Tc) / k) rows, of which
    ``lengths[b]`` = (pending + n[b]) // k are the slot's; the up to k - 1 frames of an incomplete group wait for the next chunk,
    and ``flush`` completes them with zeros (the one-shot forward's last group) before it drains the lookahead, so it returns up
    to ``delay + 1`` frames.  A slot fed x_len frames in any cuts and flushed has emitted ceil(x_len / k) frames.  ``delay``,
    ``lengths`` and ``frames`` count output frames; in input frames the output lags by up to k * delay + k - 1.

    A model with ``latency_control`` = (Nc, Nr) (bidirectional, every recurrent layer an ``nn.LCBiGRU``) streams
    too: every layer carries its forward direction's state and the up to K = Nc + Nr - 1 input rows that wait for the right context
    of their block, and emits whole blocks.  ``delay`` = num_layers * K is then a bound: ``advance`` returns ``delay`` + To rows, of
    which ``lengths[b]`` (a multiple of Nc) are the slot's, and ``flush`` ends the masked slots layer by layer -- a layer's [pending
    rows | what the layer in front of it emitted] are its utterance's end, every block in them is closed as the one-shot forward
    closes a truncated one -- and returns up to ``delay`` (+ 1 with ``time_reduction``) rows.  The blocks are anchored at a slot's
    frame 0, so what comes out does not depend on the cuts.

    ``frames``
    (B) int32 on the device counts the logit frames a slot has emitted since it was last reset (``flush`` leaves the finished
    utterance's count standing until the slot is fed again).  Rows of `logits` at or beyond ``lengths[b]`` are unspecified (the
    epsilon-free LayerNormalization turns a constant row into NaN).  Runs under ``torch.no_grad()``; dropout layers are skipped.
    Nothing here synchronises with the host.

    A ``cnn.AcousticModel`` must have been called or loaded once, so that every lazily sized parameter has its size.  Its delay is 0:
    ``advance`` returns ``lengths == n`` and ``flush`` no rows.  The W = g V / (||V|| + 1e-9) of its weight-normalised layers, and the
    16-bit matrices made from it, are formed once, here: the stream sees a later change of such a layer's V or g only after
    ``refresh()`` (every other parameter is read as it is when the chunk runs)."""

    def __init__(self, model, B, max_chunk=64, device=None):
        self.plan = stream_plan(model)
        self.model, self.B, self.max_chunk, self.delay = model, int(B), int(max_chunk), self.plan["delay"]
        if self.B < 1 or self.max_chunk < 1:
            raise ValueError("B and max_chunk must be positive")
        front = _front(model)
        if any(p.numel() == 0 for p in front.parameters()):
            raise ValueError("the model has parameters without a size yet: run it once or load it before it is streamed")
        if device is None:
            device = next(model.parameters()).device
        self.device = dev = torch.device(device)
        for entry in self.plan["layers"]:
            if entry["kind"] != "state" and entry["R"] % 8 != 0:
                raise ValueError("carried rows must be a multiple of 8 features wide, got %d" % entry["R"])

        def rows(count, width):
            return torch.zeros((count, self.B, width), dtype=_ops.BF16, device=dev)

        def per_slot(dtype=torch.int32):
            return torch.zeros((self.B,), dtype=dtype, device=dev)

        # per carrying layer (carried rows[, their count per slot], the window a chunk is laid into)
        kinds = {e["kind"]: e for e in self.plan["layers"]}
        self._ctx = [(e, rows(e["K"], e["R"]), rows(e["K"] + self.max_chunk, e["R"]))
                     for e in self.plan["layers"] if e["kind"] == "context"]
        self._h = [torch.zeros((1, self.B, e["H"]), dtype=torch.float32, device=dev) for e in self.plan["layers"] if e["kind"] == "state"]
        e = kinds.get("lookahead")
        self._look = e and (rows(e["K"], e["R"]), per_slot(), rows(e["K"] + self.max_chunk, e["R"]))
        self.k, e = self.plan.get("time_reduction", 1), kinds.get("stack")
        self._stack = e and (rows(e["K"], e["R"]), per_slot(), rows(-(-(e["K"] + self.max_chunk) // self.k), self.k * e["R"]))
        # per latency-controlled layer (plan entry, the layer, the forward direction's state, pending rows, their count per slot, the
        # window [pending | incoming]): layer l takes up to l * K + To rows from the one in front of it and holds up to K of its own
        self._lc, incoming = [], -(-(self.k - 1 + self.max_chunk) // self.k)
        for e in self.plan["layers"]:
            if e["kind"] == "lc":
                self._lc.append((e, model.rnn_blocks.layers[e["index"]], torch.zeros((1, self.B, e["H"]), dtype=torch.float32, device=dev),
                                 rows(e["K"], e["R"]), per_slot(), rows(e["K"] + incoming, e["R"])))
                incoming += e["K"]
        self.frames = per_slot()
        self._ended = per_slot(torch.bool)          # flushed and not fed since: `frames` is the old count
        self._ones = torch.ones((self.B,), dtype=torch.int32, device=dev)
        # the layer list every chunk runs in front: the model's own layers without the dropouts, a _StreamedConvolution for every
        # convolution that carries rows or whose weight is derived
        self._lengths, self._streamed = _ChunkLengths(), []
        carries = {c[0]["path"]: c for c in self._ctx}

        def stand_ins(layers, outer=()):
            out = []
            for index, layer in enumerate(layers):
                path = outer + (index,)
                conv, gated = _convolution_of(layer)
                if _name(layer) == "Dropout":
                    continue
                if isinstance(layer, nn.Residual):
                    layer = nn.Residual(*stand_ins(layer.layers, path))
                elif conv is not None and (path in carries or isinstance(conv, nn.WeightnormConvolution2D)):
                    layer = _StreamedConvolution(conv, gated, carries.get(path), self._lengths)
                    self._streamed.append(layer)
                out.append(layer)
            return out

        self._layers = stand_ins(front.layers)
        # and what runs behind it: nothing for a recipe, whose last layer gives the logits
        self._grus, self._dense = [], []
        if front is model:
            _, height, self._vocab = _walk(model)
            if height != 1:
                raise ValueError("the model leaves %d rows per frame: logits need one" % height)
            mark_logit_layers(model.layers)     # the last projection and normalisation write float32, as in the one-shot call
        else:
            self._grus = [layer for layer in model.rnn_blocks.layers if isinstance(layer, (nn.GRU, nn.SeqSRU))]
            self._dense = [layer for layer in model.dense_blocks.layers if _name(layer) != "Dropout"]
            self._vocab = model.dense_blocks.layers[-2].out_channels

    def refresh(self):
        """read the weight-normalised layers' parameters again: W = g V / (||V|| + 1e-9) and its 16-bit matrices, one pass per layer
        (a ds2.Model has none: nothing to do)"""
        with torch.no_grad():
            for layer in self._streamed:
                layer.refresh()

    # ---------------------------------------------------------------------------------------------------------------- arguments
    def _slots(self, values, what):
        """(B) integers, host or device -> int32 on the device"""
        values = torch.as_tensor(values).to(self.device, torch.int32).contiguous()
        if tuple(values.shape) != (self.B,):
            raise ValueError("%s must have one entry per utterance (%d)" % (what, self.B))
        return values

    def reset(self, mask=None):
        """start every slot over, or those with mask[b] != 0 (`mask`: (B) integers, host or device)"""
        mask = None if mask is None else self._slots(mask, "mask")
        for _, state, _ in self._ctx:
            if state.shape[0] > 0:
                _ops.stream_push_reset(state, None, mask)
        if self._stack is not None:
            _ops.time_stack_push_reset(self._stack[0], self._stack[1], mask)
        if self._look is not None:
            _ops.stream_push_reset(self._look[0], self._look[1], mask)
        for _, _, _, state, m, _ in self._lc:
            _ops.stream_push_reset(state, m, mask)
        states = self._h + [carry[2] for carry in self._lc]
        if mask is None:
            for h in states:
                h.zero_()
            self.frames.zero_()
            self._ended.zero_()
        else:
            on = mask != 0
            for h in states:
                h.masked_fill_(on.view(1, self.B, 1), 0)
            self.frames.masked_fill_(on, 0)
            self._ended.masked_fill_(on, False)

    def _emitted(self, lengths, fed):
        """count `lengths` into ``frames``; the slots in `fed` (None: all) that were flushed before start their count over first"""
        again = self._ended.clone() if fed is None else self._ended & fed
        self.frames.masked_fill_(again, 0)
        self._ended.logical_xor_(again)
        self.frames += lengths

    # ---------------------------------------------------------------------------------------------------------------- the chunk
    def advance(self, x, x_length=None):
        """x (B, C, n_mel, Tc) features, Tc <= max_chunk; x_length (B), host or device: the valid frames of this chunk per slot,
        left-aligned (0: the slot is left exactly as it is), None: all Tc -> (logits (To, B, V) f32, lengths (B) int32), To = Tc, or
        ceil((k - 1 + Tc) / k) with time_reduction = k (an empty chunk, Tc = 0, touches nothing and returns no rows)"""
        first = self._ctx[0][0] if self._ctx else None
        if x.dim() != 4 or x.shape[0] != self.B or (first is not None and tuple(x.shape[1:3]) != (first["channels"], first["height"])):
            want = ("C", "n_mel") if first is None else (first["channels"], first["height"])
            raise ValueError("the chunk must be (%d, %s, %s, Tc), got %s" % ((self.B,) + want + (tuple(x.shape),)))
        Tc = x.shape[3]
        if Tc > self.max_chunk:
            raise ValueError("a chunk of %d frames exceeds max_chunk = %d" % (Tc, self.max_chunk))
        n = None
        if x_length is not None:
            on_host = not (isinstance(x_length, torch.Tensor) and x_length.is_cuda)
            if on_host and torch.as_tensor(x_length).numel() == self.B and int(torch.as_tensor(x_length).max()) > Tc:
                raise ValueError("x_length exceeds the chunk's %d frames" % Tc)
            n = self._slots(x_length, "x_length")
            if not on_host:
                n = n.clamp(0, Tc)
        if Tc == 0:
            return (torch.empty((0, self.B, self._vocab), dtype=torch.float32, device=self.device),
                    torch.zeros((self.B,), dtype=torch.int32, device=self.device))
        with torch.no_grad():
            # the front on this chunk -> logical (B, C', H', Tc): the one-shot forward's own sequencer, so the same fused passes, with
            # every carrying convolution un-padded in time over [its K carried rows | the chunk]
            self._lengths.n = n
            out = functions.reshape(nn.nn._apply_layers(self._layers, x.to(self.device)), (self.B, -1, Tc))
            To, steps = Tc, n
            if self._stack is not None:     # the whole groups of [pending | chunk]; the rest waits
                state, m, groups = self._stack
                To = (self.k - 1 + Tc + self.k - 1) // self.k
                groups = groups[:To]
                steps = _ops.time_stack_push(state, m, functions.phys3(out), n, groups, self.k)
                out = functions.logical3(groups)
            if self._lc:
                logits, lengths = self._tail(*self._blocks(out, steps), None)
            else:
                logits, lengths = self._tail(self._recurrences(out, steps), steps, self.delay + To, To)
            if lengths is None:
                lengths = torch.full((self.B,), Tc, dtype=torch.int32, device=self.device)
            elif lengths is n:
                lengths = n.clone()         # (the caller's own tensor stays the caller's)
            self._emitted(lengths, None if n is None else n > 0)
        return logits, lengths

    def _recurrences(self, out, steps):
        """the GRU or SeqSRU layers on (B, D, To) from their carried states, over steps[b] frames per slot (None: all)"""
        for layer, h in zip(self._grus, self._h):
            out, hy = layer(out, steps, hx=h)
            # (a slot beyond its length keeps its state bit for bit: csrc/gru.hip pins its update gate, csrc/sru_seq.hip hands cx on)
            h.copy_(hy)
        return out

    def _blocks(self, out, steps, flush=None):
        """The latency-controlled layers on `out` (B, D, To) with steps[b] new frames per slot (None: all; `out` None: nothing new).
        Every layer lays [its pending rows | the incoming ones] into its window, runs the forward direction from the carried state
        over the emit[b] frames of the whole blocks whose right context is there, the reverse direction over those w[b] blocks as
        windows (the one-shot layer's own kernels and order of sums), and hands the emit[b] frames on as the next layer's chunk.
        The slots in `flush` end: their rows are the utterance's end, every block of them is whole (the one-shot rule for a
        truncated window) and all of them are emitted.  -> (the last layer's output (B, H, rows of its window), emitted frames (B));
        a layer that holds nothing back (Nc = 1, Nr = 0: K = 0) and is handed nothing has no rows: (None, zeros) if it is the last."""
        chunk = None if out is None else functions.phys3(out)
        for entry, layer, h, state, m, window in self._lc:
            Nc, Nr = entry["Nc"], entry["Nr"]
            rows = entry["K"] + (0 if chunk is None else chunk.shape[0])
            if rows == 0:
                chunk, steps = None, torch.zeros((self.B,), dtype=torch.int32, device=self.device)
                continue
            window = window[:rows]
            a, w, steps = _ops.lc_push(state, m, chunk, steps, window, Nc, Nr, flush)
            if layer.w_ih.numel() == 0:     # (a model that never ran: the layer sizes its input weights at its first call)
                layer._initialize_params(entry["R"])
            params = (layer.w_ih, layer.w_hh, layer.b_ih, layer.b_hh)
            fwd, hy = functions.gru(functions.logical3(window), *functions.lc_direction(params, 0), layer.directions[0], 1, steps, hx=h)
            h.copy_(hy)                     # (a slot beyond its length keeps its state bit for bit, as in _recurrences)
            xw, w_len = _ops.lc_gather(window, Nc, Nr, _ops.LC_WINDOW, a, w)
            yw = functions.gru(functions.logical3(xw), *functions.lc_direction(params, 1), layer.directions[1], 1, w_len)
            chunk = _ops.lc_scatter(functions.phys3(yw), rows, self.B, Nc, Nr, _ops.LC_BLOCK, functions.phys3(fwd), a, w)
        return (None if chunk is None else functions.logical3(chunk)), steps

    def _tail(self, out, steps, rows, keep=None, flush=None, ended=None):
        """What follows the recurrences: the lookahead, if the model has one, and the dense layers.  `out` (B, D, To) with steps[b]
        frames per slot (None: nothing new, the slots in `flush` end) goes behind the lookahead's pending frames into the first
        `rows` rows of its window, the layer runs over them with nothing to come, and the first `keep` rows of that (None: all)
        go through the dense layers and the per-frame LayerNormalization -> (logits (rows kept, B, V) float32, lengths (B): the
        frames the push says a slot emits, or with `ended` every valid window row of the slots in it and none of the others);
        without a lookahead `out` goes straight on and lengths are `steps`."""
        lengths = steps
        if self._look is not None:
            state, m, window = self._look
            window = window[:rows]
            wlen, lengths = _ops.stream_push(state, m, None if out is None else functions.phys3(out), steps, window,
                                             _ops.STREAM_LOOKAHEAD, flush=flush)
            out = functions.logical3(_ops.lookahead_fwd(window, self.model.lookahead.W.detach(), wlen)[:keep])
            if ended is not None:
                lengths = torch.where(ended != 0, wlen, torch.zeros_like(wlen))
        out = nn.nn._apply_layers(self._dense, out)
        return out.permute(2, 0, 1).to(torch.float32).contiguous(), lengths

    def _flush_stacked(self, mask):
        """the masked slots' incomplete group, completed with zeros, goes through the recurrences as one more frame; behind it the
        lookahead runs over [its pending frames | that frame] with nothing to come, which is the one-shot forward's utterance end"""
        state, m, groups = self._stack
        groups = groups[:1]
        steps = _ops.time_stack_push(state, m, None, None, groups, self.k, flush=mask)      # (B) of 0 or 1
        return self._tail(self._recurrences(functions.logical3(groups), steps), steps, self.delay + 1, ended=mask)

    def flush(self, mask=None):
        """end of utterance for every slot, or those with mask[b] != 0: -> (logits (delay, B, V), lengths (B)) with the frames the
        lookahead held back, computed with a zero future; then these slots are reset (``frames`` keeps the finished count until
        the slot is fed again).  With time_reduction > 1: (delay + 1, B, V), the zero-completed last group first."""
        mask = self._ones if mask is None else self._slots(mask, "mask")
        with torch.no_grad():
            logits = None
            if self._lc:
                # layer by layer: the incomplete group, if there is one, is the first layer's last frame; every layer then emits all
                # of [its pending rows | what the layer in front of it emitted], up to `delay` (+ 1) frames behind the last one
                out = steps = None
                if self._stack is not None:
                    state, m, groups = self._stack
                    steps = _ops.time_stack_push(state, m, None, None, groups[:1], self.k, flush=mask)
                    out = functions.logical3(groups[:1])
                out, lengths = self._blocks(out, steps, flush=mask)
                if out is not None:
                    logits, lengths = self._tail(out, lengths, None)
            elif self._stack is not None:
                logits, lengths = self._flush_stacked(mask)
            elif self._look is not None:
                logits, lengths = self._tail(None, None, self.delay, flush=mask)
            else:
                lengths = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
            if logits is None:              # (nothing is held back anywhere)
                logits = torch.empty((0, self.B, self._vocab), dtype=torch.float32, device=self.device)
        count = self.frames + lengths
        self.reset(mask)
        on = mask != 0
        self.frames.copy_(torch.where(on, count, self.frames))
        self._ended.logical_or_(on)
        return logits, lengths
