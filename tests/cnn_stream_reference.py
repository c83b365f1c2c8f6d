"""Float64 restatement of the streaming forward of the convolutional recipes (asr.model.stream.AcousticStream over a
cnn.AcousticModel), on top of oracle.cnn.program and the oracle's own operators.  TEST INFRASTRUCTURE, no GPU.

Every op runs on the chunk alone.  A convolution with pad_t = kw - 1 > 0 runs un-padded in time on [its K = kw - 1 carried input
frames | the chunk]; what it carries to the next chunk is, per slot, the last K frames of [carried | the slot's n valid frames], so a
slot fed n = 0 keeps what it has.  Frames of a chunk beyond a slot's n are never read by a valid output frame: every op here is per
frame or looks back only.

Also here, shared by tests/test_cnn_stream_cpu.py and tests/test_cnn_stream_gpu.py: the recipes, the small configuration, the seeded
redraw of the parameters, and the cut schedules.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn as ocnn

V = 32
# (architecture, conv layers, weight normalisation)
RECIPES = [("zhang", 3, False), ("zhang+fc_relu", 2, False), ("zhang+residual", 4, False), ("zhang+residual", 6, False),
           ("zhang+residual", 3, True), ("zhang+layernorm", 2, False), ("glu", 2, False), ("glu", 2, True),
           ("relu+layernorm", 2, False), ("relu+layernorm+residual", 3, False)]


def recipe_id(recipe):
    return "%s-%d%s" % (recipe[0], recipe[1], "-wn" if recipe[2] else "")


def config(arch, nconv, wn=False):
    from asr.model import cnn
    cfg = cnn.configure()
    cfg.vocab_size, cfg.ndim_audio_features, cfg.num_mel_filters, cfg.ndim_h, cfg.ndim_dense = V, 3, 40, 16, 24
    cfg.num_conv_layers, cfg.architecture, cfg.weightnorm = nconv, arch, wn
    return cfg


def redraw(params, seed):
    """{name: tensor} -> the same names with every convolution weight (``.W``, or ``.V`` of a weight-normalised layer) drawn as
    N(0, 1 / fan_in) and every bias as 0.1 N(0, 1), in the order of the sorted names; everything else (g, gamma, beta) as it is.
    At the default initialisation the `glu` recipe's logits barely depend on the input, and no bar could see a broken carry."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(params):
        p = params[name]
        leaf = name.rsplit(".", 1)[1]
        if leaf in ("W", "V") and p.dim() == 4:
            fan_in = p.shape[1] * p.shape[2] * p.shape[3]
            out[name] = (torch.randn(p.shape, generator=gen, dtype=torch.float64) / fan_in ** 0.5).to(p.dtype)
        elif leaf == "b":
            out[name] = (0.1 * torch.randn(p.shape, generator=gen, dtype=torch.float64)).to(p.dtype)
        else:
            out[name] = p.detach().clone()
    return out


def host_params(arch, cfg, seed):
    """float64 parameters of a recipe without weight normalisation, no device needed: the convolutions take their shapes from the
    model as built, a LayerNormalization (sized on the first call there) the channels in front of it, gamma = 1 and beta = 0"""
    from asr.model.architectures import build_model
    assert not cfg.weightnorm
    shapes = {k: tuple(v.shape) for k, v in build_model(cfg).state_dict().items()}
    params, channels = {}, cfg.ndim_audio_features
    for op, name, _ in ocnn.program(arch, cfg):
        if op in ("conv", "glu"):
            params[name + ".W"] = torch.zeros(shapes[name + ".W"], dtype=torch.float64)
            params[name + ".b"] = torch.zeros(shapes[name + ".b"], dtype=torch.float64)
            assert shapes[name + ".W"][1] == channels, name
            channels = shapes[name + ".W"][0] // (2 if op == "glu" else 1)
        elif op == "maxout":
            channels //= 2
        elif op == "ln":
            params[name + ".gamma"] = torch.ones(channels, dtype=torch.float64)
            params[name + ".beta"] = torch.zeros(channels, dtype=torch.float64)
    return redraw(params, seed)


class Stream:
    """the chunked forward: ``advance(x (B, C, H, Tc), n (B))`` -> logits (B, V, 1, Tc), of which the first n[b] frames are slot b's.
    mutant: None, ("drop", j): the j-th carrying convolution forgets its carry before every chunk, or ("shift", j): its carry is
    one frame late (frames t - K - 1 .. t - 2 where t - K .. t - 1 belong)."""

    def __init__(self, arch, cfg, params, B, mutant=None):
        self.prog, self.params, self.B, self.mutant = ocnn.program(arch, cfg), params, B, mutant
        self.K = cfg.kernel_size[1] - 1
        self.carrying = [i for i, (op, _, args) in enumerate(self.prog) if op in ("conv", "glu") and args[1] > 0]
        self.hist = {}              # op index -> (B, C, H, K + 1): the last K + 1 valid input frames (the mutant reads the oldest)

    def advance(self, x, n):
        h, skip = x, None
        for i, (op, name, args) in enumerate(self.prog):
            if op == "res_begin":
                skip = h
            elif op == "res_end":
                h = h + skip
            elif i in self.carrying:
                h = self._carrying(i, name, op, args, h, n)
            else:
                h = ocnn.run(self.prog, i, i + 1, self.params, h)
        return h

    def _carrying(self, i, name, op, args, h, n):
        K, j = self.K, self.carrying.index(i)
        assert args[1] == K
        if i not in self.hist:
            self.hist[i] = torch.zeros(h.shape[:3] + (K + 1,), dtype=h.dtype)
        hist = self.hist[i]
        carried = hist[..., 1:]
        if self.mutant == ("drop", j):
            carried = torch.zeros_like(carried)
        elif self.mutant == ("shift", j):
            carried = hist[..., :K]
        W, b = self.params[name + ".W"], self.params[name + ".b"]
        y = F.conv2d(torch.cat([carried, h], dim=3), W, None, stride=1, padding=(args[0], 0)) + b.reshape(1, -1, 1, 1)
        assert y.shape[3] == h.shape[3]
        if op == "glu":
            a, g = torch.chunk(y, 2, dim=1)
            y = a * torch.sigmoid(g)
        self.hist[i] = torch.stack([torch.cat([hist[s], h[s, :, :, :int(n[s])]], dim=2)[..., -(K + 1):] for s in range(self.B)])
        return y


def schedule(kind, lens, seed=0):
    """per call: the frames every slot gets.  "whole": everything in one chunk; "single": chunks of 1 frame; "ragged": every slot
    a different number in 0..7 per call, one slot idle in turn"""
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


def chunk_of(x, pos, n, Tc=None):
    """the chunk of a call: slot b's frames pos[b] .. pos[b] + n[b] of x (B, C, H, T), left-aligned; the rest holds 9.0, which
    nothing may read"""
    Tc = int(max(n)) if Tc is None else Tc
    chunk = torch.full(tuple(x.shape[:3]) + (Tc,), 9.0, dtype=x.dtype)
    for b, nb in enumerate(n):
        chunk[b, :, :, :nb] = x[b, :, :, pos[b]:pos[b] + nb]
    return chunk


def run_schedule(stream, x, calls):
    """-> per slot, the (frames, V) logits of its valid frames, concatenated over the calls"""
    pos = np.zeros(x.shape[0], dtype=np.int64)
    got = [[] for _ in range(x.shape[0])]
    for n in calls:
        out = stream.advance(chunk_of(x, pos, n), n)
        for b, nb in enumerate(n):
            got[b].append(out[b, :, 0, :nb].T)
        pos += n
    return [torch.cat(g) for g in got]


def rel(got, want):
    """relative L2 over the valid frames of all slots"""
    a = torch.cat([g.double().flatten() for g in got])
    b = torch.cat([w.double().flatten() for w in want])
    assert bool(torch.isfinite(a).all())
    return float((a - b).norm() / b.norm())
