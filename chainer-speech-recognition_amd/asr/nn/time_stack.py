"""Time reduction by frame stacking: k consecutive frames become one frame of k times the features, so every layer behind it
(the recurrences above all) runs over ceil(T / k) steps.  It loses no information and has no parameters.  Kernels:
csrc/time_stack.hip; the streaming form is ``asr.model.stream.AcousticStream``'s."""
from .. import _ops, functions


class TimeStack:
    """``layer(x, x_length=None)``: x (B, D, T) -> (y (B, k * D, ceil(T / k)), y_length), y[b, j * D + d, g] = x[b, d, g * k + j];
    frames at and beyond ``x_length[b]`` read as zero, so a partly filled last group is completed with zeros;
    y_length = ceil(x_length / k), None when x_length is None."""

    def __init__(self, k):
        if int(k) != k or not 1 <= k <= _ops.TIME_STACK_MAX:
            raise ValueError("k must be an integer in 1..%d, got %r" % (_ops.TIME_STACK_MAX, k))
        self.k = int(k)

    def __call__(self, x, x_length=None):
        return functions.time_stack(x, self.k, x_length)
