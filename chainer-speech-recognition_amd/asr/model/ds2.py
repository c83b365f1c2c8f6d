"""Deep-Speech-2-style conv + (Bi)GRU CTC acoustic model -- the model BASELINE.json's configs[0..2] name.

The reference ships no GRU model; this one is written against the `asr.nn` API in the shape of the reference's
conv + recurrent template run/ctc/sru/model.py:10-139 (conv blocks -> reshape (B, C*H, T) -> recurrent blocks ->
1x1 dense blocks with Maxout -> LayerNormalization -> per-time-step split), with the recurrent output actually fed
forward (the template drops it, run/ctc/sru/model.py:120-124).  SURVEY.md section 8(d) fixes the sizes:
  conv1 3->2*ndim_conv k(3,5) -> Maxout -> MaxPool(3,1);  conv2 ndim_conv->2*ndim_conv -> Maxout -> MaxPool(2,1);
  num_rnn_layers x BiGRU(ndim_rnn) (directions summed);  Conv1D(->2*dense)+Maxout, Conv1D(dense->2*dense)+Maxout,
  Conv1D(dense->V), LayerNormalization.  ``lookahead`` > 0 (with bidirectional=False: the deployable streaming recipe,
  asr/model/stream.py) puts nn.LookaheadConvolution(ndim_rnn, lookahead) between the recurrent stack and the dense layers.
  ``time_reduction`` = k > 1 puts nn.TimeStack(k) between the reshape and the first recurrent layer, as Deep Speech 2 reduces its
  frame rate in front of the recurrences: k frames of C*H features become one of k*C*H, the recurrent, lookahead and dense layers
  run over ceil(T / k) frames and the model emits that many (``output_length``).
  ``latency_control`` = (Nc, Nr) (with bidirectional=True) makes every recurrent layer an nn.LCBiGRU: the reverse directions restart
  per block of Nc frames with Nr frames of right context, and the model streams with a delay of num_rnn_layers * (Nc + Nr - 1) frames.
  ``rnn`` = "sru" makes every recurrent layer an nn.BiSeqSRU (or nn.SeqSRU with bidirectional=False) in place of the GRU links: the
  cell recurrence is linear in its state, so a layer is two scans that run time in parallel chunks and not T dependent steps
  (csrc/sru_seq.hip); it takes x_length, lookahead, time_reduction and dropout as the GRU stack does and, forward-only, streams.
"""
from .. import _ops, functions, nn
from .base import NeedsVocabulary
from ._acoustic import load_if_exists, save_atomic, split_output


_RECURRENT = (nn.GRU, nn.BiGRU, nn.LCBiGRU, nn.SeqSRU, nn.BiSeqSRU)


class Configuration(NeedsVocabulary):
    FIELDS = dict(ndim_audio_features=3, ndim_conv=64, ndim_rnn=512, ndim_dense=320, num_conv_layers=2, num_rnn_layers=4,
                  bidirectional=True, kernel_size=(3, 5), dropout=0, lookahead=0, time_reduction=1, latency_control=None,
                  rnn="gru")


def configure():
    return Configuration()


class Model(nn.Module):
    def __init__(self, config):
        super(Model, self).__init__()
        kernel_size = tuple(config.kernel_size)
        pad = kernel_size[1] - 1
        dropout = config.dropout
        self.num_rnn_layers = config.num_rnn_layers
        k = getattr(config, "time_reduction", 1)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _ops.TIME_STACK_MAX:
            raise ValueError("time_reduction must be an integer in 1..%d, got %r" % (_ops.TIME_STACK_MAX, k))
        self.time_reduction = k

        conv_blocks = nn.Module()
        pools = [3] + [2] * (config.num_conv_layers - 1)
        in_ch = config.ndim_audio_features
        for pool in pools:
            conv_blocks.add(
                # causal=True == pad=(0, kw-1) followed by the reference's `lambda x: x[..., :-pad]`
                nn.Convolution2D(in_ch, config.ndim_conv * 2, kernel_size, stride=1, pad=(0, pad), causal=True),
                nn.Maxout(2),
                nn.Dropout(dropout),
                nn.MaxPooling2D(ksize=(pool, 1)),
            )
            in_ch = config.ndim_conv
        self.conv_blocks = conv_blocks
        height = config.num_mel_filters
        self._input_height = height         # (asr/model/stream.py sizes the carried rows of the first block from it)
        for pool in pools:          # pad_h = 0 convolution, then cover_all pooling
            height -= kernel_size[0] - 1
            height = 1 if height <= pool else -(-(height - pool) // pool) + 1
        self._merged = (config.ndim_conv, height)

        # time reduction by frame stacking in front of the recurrences.  It has no parameters and is an attribute of its own, so no
        # checkpoint name moves; at k = 1 the model holds no such layer at all.
        if k > 1:
            self.time_stack = nn.TimeStack(k)

        # latency control (Nc, Nr): every recurrent layer of a bidirectional model becomes an nn.LCBiGRU, whose reverse direction is
        # restarted per block of Nc frames with Nr frames of right context -- a BiGRU's parameters under a BiGRU's names, so no
        # checkpoint name moves.  Blocks count the frames the recurrences see: reduced ones with time_reduction > 1.
        control = getattr(config, "latency_control", None)
        if control is not None:
            if not isinstance(control, (tuple, list)) or len(control) != 2:
                raise ValueError("latency_control must be None or (block, right context), got %r" % (control,))
            control = functions.lc_check(*control)
            if not config.bidirectional:
                raise ValueError("latency_control restarts the reverse direction of a bidirectional model: bidirectional=False has none")
            if config.lookahead > 0:
                raise ValueError("latency_control and lookahead > 0 do not combine: the right context is the model's lookahead")
        self.latency_control = control

        # the recurrent cell.  A configuration from before the field reads as "gru"; with "gru" the model is what it was, attribute
        # for attribute and parameter name for parameter name.
        cell = getattr(config, "rnn", "gru")
        if cell not in ("gru", "sru"):
            raise ValueError("rnn must be \"gru\" or \"sru\", got %r" % (cell,))
        if cell == "sru" and control is not None:
            raise ValueError("latency_control with rnn=\"sru\" is not built: the windowed reverse direction exists for the GRU only")

        rnn_blocks = nn.Module()
        for _ in range(config.num_rnn_layers):
            if cell == "sru":
                rnn = (nn.BiSeqSRU if config.bidirectional else nn.SeqSRU)(None, config.ndim_rnn)
            elif control is not None:
                rnn = nn.LCBiGRU(None, config.ndim_rnn, block=control[0], right=control[1])
            else:
                rnn = (nn.BiGRU if config.bidirectional else nn.GRU)(None, config.ndim_rnn)
            rnn_blocks.add(rnn, nn.Dropout(dropout))
        self.rnn_blocks = rnn_blocks

        # Deep Speech 2's lookahead convolution between the recurrent stack and the dense layers: `lookahead` future frames for a
        # forward-only stack.  An attribute of its own -- the _sequential_%d names of the blocks are checkpoint names and stay put.
        if config.lookahead > 0:
            self.lookahead = nn.LookaheadConvolution(config.ndim_rnn, config.lookahead)

        dense_blocks = nn.Module()
        dense_blocks.add(nn.Convolution1D(None, config.ndim_dense * 2), nn.Maxout(2), nn.Dropout(dropout))
        dense_blocks.add(nn.Convolution1D(config.ndim_dense, config.ndim_dense * 2), nn.Maxout(2), nn.Dropout(dropout))
        logits = nn.Convolution1D(config.ndim_dense, config.vocab_size)
        norm = nn.LayerNormalization()
        logits.output_float32 = True
        norm.output_float32 = True
        dense_blocks.add(logits, _PerFrame(norm))
        self.dense_blocks = dense_blocks

    def __call__(self, x, split_into_variables=True, x_length=None):
        """x_length (B) int32 on the device (the Loader's x_length_batch, asr/data/loaders/base.py:30): the recurrent layers then
        run every utterance over its own frames (the reverse direction starts at the utterance's last frame, not in the padding);
        None = the padded block as it is.  With ``time_reduction`` = k the output has ceil(T / k) frames, of which
        ``output_length(x_length)`` are an utterance's own."""
        batchsize = x.shape[0]
        seq_length = x.shape[3]
        out_data = self.conv_blocks(x)
        out_data = functions.reshape(out_data, (batchsize, -1, seq_length))
        if self.time_reduction > 1:
            out_data, x_length = self.time_stack(out_data, x_length)
            seq_length = out_data.shape[2]
        if x_length is None:
            out_data = self.rnn_blocks(out_data)
        else:
            for layer in self.rnn_blocks.layers:
                out_data = layer(out_data, x_length) if isinstance(layer, _RECURRENT) else layer(out_data)
        if getattr(self, "lookahead", None) is not None:
            out_data = self.lookahead(out_data, x_length)
        out_data = self.dense_blocks(out_data)
        assert out_data.shape[2] == seq_length
        return split_output(out_data, batchsize, seq_length, split_into_variables)

    def output_length(self, x_length):
        """the logit frames of an utterance of `x_length` input frames: ceil(x_length / time_reduction), for an int, a list or a
        tensor (of the same kind).  It is what the CTC and Gram-CTC losses, the decoders and the aligners take as the length."""
        return functions.reduced_length(x_length, self.time_reduction)

    def column_permutations(self):
        """parameters whose last axis indexes the merged (channel, height) features of the conv stack: {name: (C, H)}.
        The reference's ``reshape(out, (B, -1, T))`` (run/ctc/sru/model.py:114) orders them (c, h), the physical layout here
        (h, c) -- asr/serializers.py stores the reference's order.  With time_reduction = k the stacked columns are (j, h, c),
        j the frame of the group; they are declared as (C, k * H), so the file holds them as (c, j, h): channel-major like the
        reference's, a fixed permutation that load inverts exactly (no reference checkpoint has stacked features to agree with)."""
        first = "W" if isinstance(self.rnn_blocks.layers[0], (nn.SeqSRU, nn.BiSeqSRU)) else "w_ih"
        return {"rnn_blocks._sequential_0.%s" % first: (self._merged[0], self._merged[1] * self.time_reduction)}

    def save(self, filename):
        save_atomic(self, filename)

    def load(self, filename):
        return load_if_exists(self, filename)


class _PerFrame(nn.Link):
    """LayerNormalization over the vocabulary of every frame: views (B, V, T) as the reference's 4-d (B, V, 1, T)
    so that axes (1, 2) are (V, 1) -- the statistics the CNN models use (asr/model/cnn.py + asr/nn/nn.py:260-265) --
    rather than (V, T), which would make an utterance's logits depend on its padding."""

    def __init__(self, norm):
        super().__init__()
        self.norm = norm

    def __call__(self, x):
        return self.norm(x.unsqueeze(2)).squeeze(2)


def build_model(config):
    return Model(config)
