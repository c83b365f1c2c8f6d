"""SeqSRU / BiSeqSRU: the SRU as a recurrent layer with the GRU links' call signature (asr/nn/gru.py), so that a ``ds2.Model`` takes
either cell and ``asr.model.stream.AcousticStream`` carries either state.  ``nn.SRU`` (asr/nn/sru.py, the reference's link) is untouched:
this layer adds per-utterance lengths, a reverse direction, an input width that differs from its own and a carried state
(include/asr_hip.h states the semantics; csrc/sru_seq.hip).  Dropout is the model's business (``nn.Dropout`` between the layers)."""
import math

from .. import functions
from ..link import Link, Parameter, Uniform, get_initializer


class _SeqSRUBase(Link):
    def __init__(self, in_size, out_size, ndir, use_tanh=True):
        super().__init__()
        self.in_size, self.out_size, self.ndir, self.use_tanh = in_size, out_size, ndir, use_tanh
        self.W = Parameter()
        self.B = Parameter(get_initializer(0)((ndir, 2 * out_size)))
        if in_size is not None:
            self._initialize_params(in_size)

    def _initialize_params(self, in_size):
        """k is decided here: 3 blocks [z; f; r] when the input has the layer's own width (the highway carries x, the reference's form),
        4 blocks [z; f; r; p] otherwise (it carries the projection p)"""
        self.in_size = in_size
        self.k = 3 if in_size == self.out_size else 4
        init = Uniform(math.sqrt(3.0 / in_size))        # (the SRU paper's: unit variance through the projection)
        self.W.data = init((self.ndir, self.k * self.out_size, in_size)).to(self.W.device)

    def __call__(self, x, x_length=None, hx=None):
        """x (B, I, T) -> (B, D, T); the outputs of a bidirectional layer are summed, as BiGRU's are.  x_length (B) int32 on the device:
        every utterance over its own length.  hx (ndir, B, D) float32: the initial cell state -- the call then returns (y, hy), hy
        (ndir, B, D) the state after every utterance's last own frame, so that a sequence can be fed in pieces."""
        if self.W.numel() == 0:
            self._initialize_params(x.shape[1])
        return functions.sru_seq(x, self.W, self.B, self, self.ndir, x_length, hx, self.use_tanh)


class SeqSRU(_SeqSRUBase):
    def __init__(self, in_size, out_size=None, use_tanh=True):
        if out_size is None:
            in_size, out_size = None, in_size
        super().__init__(in_size, out_size, 1, use_tanh)


class BiSeqSRU(_SeqSRUBase):
    def __init__(self, in_size, out_size=None, use_tanh=True):
        if out_size is None:
            in_size, out_size = None, in_size
        super().__init__(in_size, out_size, 2, use_tanh)
