"""Lookahead (row) convolution of Deep Speech 2 (Amodei et al. 2016, section 3.7): every feature of a forward-only recurrent stack
looks ``lookahead`` frames ahead through its own (lookahead + 1)-tap filter.  The reference has no such layer (its recurrent
recipe is the SRU); it is what makes ``ds2.Model(bidirectional=False)`` worth deploying, and its ``lookahead`` frames are the
delay of ``asr.model.stream.AcousticStream``.  Kernels: csrc/lookahead.hip."""
import torch

from .. import functions
from ..link import Link, Parameter


class LookaheadConvolution(Link):
    """``layer(x, x_length=None)``: x (B, D, T) -> (B, D, T), y[b, d, t] = sum_{j=0..lookahead} W[d, j] x[b, d, t + j]; frames at and
    beyond ``x_length[b]`` read as zero and come out zero.  W (D, lookahead + 1) float32, no bias; a fresh layer is the identity
    (W[:, 0] = 1).  ``size`` None: sized by the first call."""

    def __init__(self, size=None, lookahead=0):
        super().__init__()
        if lookahead < 0:
            raise ValueError("lookahead must be >= 0, got %r" % (lookahead,))
        self.lookahead = int(lookahead)
        self.W = Parameter()
        if size is not None:
            self._initialize_params(size)

    def _initialize_params(self, size):
        w = torch.zeros((size, self.lookahead + 1), dtype=torch.float32)
        w[:, 0] = 1.0
        self.W.data = w.to(self.W.device)

    def __call__(self, x, x_length=None):
        if self.W.numel() == 0:
            self._initialize_params(x.shape[1])
        return functions.lookahead_convolution(x, self.W, x_length)
