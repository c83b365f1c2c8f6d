"""CPU oracle for the operator layer (asr/nn).  TEST INFRASTRUCTURE -- see oracle/__init__.py.

numpy restatements of arithmetic the reference owns (layer-norm, SRU, weight-norm), torch-CPU fp32 for what
the reference delegates to Chainer (conv, max-pool, maxout, GRU; PARITY UNPINNED at that boundary).
All functions use the reference's logical layouts: images (B, C, H, T), sequences (B, D, T).
"""
import numpy as np
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------- conv / pooling
def conv2d_causal(x, W, b=None, pad_h=0):
    """nn.Convolution2D(pad=(pad_h, kw-1)) followed by x[..., :-(kw-1)]  (asr/nn/nn.py:235-238,
    run/ctc/cnn/model.py:43-44).  x (B,C,H,T), W (Co,Ci,kh,kw) torch tensors."""
    kw = W.shape[3]
    y = F.conv2d(x, W, b, stride=1, padding=(pad_h, kw - 1))
    return y[..., :-(kw - 1)] if kw > 1 else y


def maxout2(x):
    """chainer.functions.maxout(x, 2, axis=1): max over adjacent channel pairs (asr/nn/nn.py:45-50)."""
    s = x.shape
    return x.reshape(s[0], s[1] // 2, 2, *s[2:]).max(dim=2)[0]


def maxpool_h(x, k):
    """chainer.functions.max_pooling_2d(x, (k,1)) with its defaults stride=ksize, cover_all=True (asr/nn/nn.py:95-103)."""
    return F.max_pool2d(x, kernel_size=(k, 1), stride=(k, 1), ceil_mode=True)


# ---------------------------------------------------------------------------------------------- layer norm
def normalize_layer_fwd(x):
    """asr/nn/layernorm.py:33-48 (no epsilon).  x (B, C, H, T) or (B, V, T) numpy."""
    size = x.shape[1] * x.shape[2]
    mean = x.mean(axis=(1, 2), keepdims=True)
    diff = x - mean
    std = np.sqrt((diff ** 2).sum(axis=(1, 2), keepdims=True) / size)
    return diff / std, diff, std


def normalize_layer_bwd(gy, diff, std):
    """asr/nn/layernorm.py:50-61 restated (sum-to-shape then broadcast)."""
    size = diff.shape[1] * diff.shape[2]
    std_grad = (-gy / (std ** 2) * diff).sum(axis=(1, 2), keepdims=True)
    var_grad = np.broadcast_to(std_grad * 0.5 / std, diff.shape) / size
    var_grad = var_grad * 2 * diff
    var_grad = var_grad + gy / std
    grad_broad = (-var_grad).sum(axis=(1, 2), keepdims=True)
    mean_grad = np.broadcast_to(grad_broad, diff.shape) / size
    return var_grad + mean_grad


def layer_normalization(x, gamma, beta):
    """nn.LayerNormalization.__call__ (asr/nn/nn.py:260-265): normalise, scale and bias along axis 1."""
    xh, diff, std = normalize_layer_fwd(x)
    shape = [1, -1] + [1] * (x.ndim - 2)
    return xh * gamma.reshape(shape) + beta.reshape(shape), (xh, diff, std)


def layer_normalization_bwd(gy, gamma, cache):
    xh, diff, std = cache
    shape = [1, -1] + [1] * (gy.ndim - 2)
    axes = tuple(i for i in range(gy.ndim) if i != 1)
    dgamma = (gy * xh).sum(axis=axes)
    dbeta = gy.sum(axis=axes)
    dx = normalize_layer_bwd(gy * gamma.reshape(shape), diff, std)
    return dx, dgamma, dbeta


# ---------------------------------------------------------------------------------------------- SRU
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def sru_fwd(X, W, Bias, c0, use_tanh=True, mask=None):
    """asr/nn/sru.py:289-324 (forward_cpu) == kernel K1 (:17-73).  X (B,D,T), W (3D,D) rows [z;f;r], Bias (2D,)
    = [b_f; b_r].  The highway term uses x * mask; U = W X uses the caller's X (forward_cpu does not mask it)."""
    Bn, D, T = X.shape
    U = np.matmul(W, X)
    Z, Fg, R = U[:, :D], U[:, D:2 * D], U[:, 2 * D:]
    xm = X if mask is None else X * mask[..., None]
    C = np.empty_like(X)
    H = np.empty_like(X)
    c = c0
    for t in range(T):
        f = _sigmoid(Fg[..., t] + Bias[:D])
        r = _sigmoid(R[..., t] + Bias[D:])
        c = f * c + (1 - f) * Z[..., t]
        g = np.tanh(c) if use_tanh else c
        H[..., t] = r * g + (1 - r) * xm[..., t]
        C[..., t] = c
    return H, C, C[..., -1]


def sru_bwd(X, W, Bias, c0, gH, gcT, use_tanh=True):
    """Kernel K2 (asr/nn/sru.py:75-191) + host part (:421-433) restated in numpy (no dropout mask)."""
    Bn, D, T = X.shape
    U = np.matmul(W, X)
    Z, Fg, R = U[:, :D], U[:, D:2 * D], U[:, 2 * D:]
    _, C, _ = sru_fwd(X, W, Bias, c0, use_tanh)
    gU = np.zeros_like(U)
    gxh = np.zeros_like(X)
    gb = np.zeros(2 * D, dtype=X.dtype)
    gc = np.zeros_like(c0) if gcT is None else gcT.copy()
    for t in range(T - 1, -1, -1):
        f = _sigmoid(Fg[..., t] + Bias[:D])
        r = _sigmoid(R[..., t] + Bias[D:])
        c = C[..., t]
        cp = c0 if t == 0 else C[..., t - 1]
        g = np.tanh(c) if use_tanh else c
        gh = gH[..., t]
        gbr = gh * (g - X[..., t]) * (1 - r) * r
        gtanh = (1 - g * g) if use_tanh else 1.0
        gct = gh * r * gtanh
        gbf = (gct + gc) * (cp - Z[..., t]) * (1 - f) * f
        gxh[..., t] = gh * (1 - r)
        gU[:, :D, t] = (gct + gc) * (1 - f)
        gU[:, D:2 * D, t] = gbf
        gU[:, 2 * D:, t] = gbr
        gb[:D] += gbf.sum(axis=0)
        gb[D:] += gbr.sum(axis=0)
        gc = (gct + gc) * f
    gX = np.einsum("od,bot->bdt", W, gU) + gxh
    gW = np.einsum("bot,bdt->od", gU, X)
    return gX, gW, gb, gc


# ---------------------------------------------------------------------------------------------- weight norm
def weightnorm_W(V, g):
    """asr/nn/convolution_2d.py:21-25,62-64: W = g * V / (||V|| + 1e-9), norm per output channel."""
    norm = np.sqrt((V ** 2).sum(axis=(1, 2, 3), keepdims=True)) + 1e-9
    return g * V / norm, V / norm, norm


def weightnorm_bwd(gW, V, g):
    """asr/nn/convolution_2d.py:92-93."""
    _, Vn, norm = weightnorm_W(V, g)
    gg = (gW * Vn).sum(axis=(1, 2, 3), keepdims=True)
    gV = g * (gW - gg * Vn) / norm
    return gV, gg


# ---------------------------------------------------------------------------------------------- GRU (torch CPU)
def bigru_sum(x_tbi, params, H, ndir=2):
    """torch.nn.GRU on CPU; directions summed (the DS2-style stack of BASELINE.json).  params: dict with
    w_ih (ndir,3H,I), w_hh (ndir,3H,H), b_ih (ndir,3H), b_hh (ndir,3H) torch tensors.  x (T,B,I)."""
    I = x_tbi.shape[2]
    gru = torch.nn.GRU(I, H, num_layers=1, bidirectional=(ndir == 2))
    with torch.no_grad():
        for d, suf in enumerate(["", "_reverse"][:ndir]):
            getattr(gru, "weight_ih_l0" + suf).copy_(params["w_ih"][d])
            getattr(gru, "weight_hh_l0" + suf).copy_(params["w_hh"][d])
            getattr(gru, "bias_ih_l0" + suf).copy_(params["b_ih"][d])
            getattr(gru, "bias_hh_l0" + suf).copy_(params["b_hh"][d])
    out, _ = gru(x_tbi)
    if ndir == 2:
        out = out[..., :H] + out[..., H:]
    return out, gru


# ---------------------------------------------------------------------------------------------- optimiser
def gradient_factor(sqnorm, clip, grad_scale=1.0):
    """What every gradient element is multiplied by before the decay is added: grad_scale (1 / world size after a sum
    all-reduce, 1 / loss scale) times GradientClipping's min(1, clip / ||grad_scale g||).  clip = 0: no clipping; a zero
    norm never clips (clip / 0 is not < 1)."""
    norm = float(np.sqrt(sqnorm)) * abs(grad_scale)
    if clip > 0 and norm > 0 and clip / norm < 1:
        return grad_scale * (clip / norm)
    return grad_scale


def clip_decay_adam(p, g, m, v, step, alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, decay=1e-5, clip=1.0, grad_scale=1.0):
    """GradientClipping(clip) -> WeightDecay(decay) -> Chainer-v2 Adam (run/ctc/cnn/train.py:142-147; Chainer is an
    absent third-party: formulas recalled from chainer/optimizers/adam.py v2, PARITY UNPINNED)."""
    g = g.astype(np.float64)
    g = g * gradient_factor((g ** 2).sum(), clip, grad_scale)
    g = g + decay * p
    m = m + (1 - beta1) * (g - m)
    v = v + (1 - beta2) * (g * g - v)
    lr = alpha * np.sqrt(1 - beta2 ** step) / (1 - beta1 ** step)
    p = p - lr * m / (np.sqrt(v) + eps)
    return p, m, v


def clip_decay_sgd(p, g, v, kind, lr, momentum, decay, clip, grad_scale=1.0):
    """GradientClipping(clip) -> WeightDecay(decay) -> one of the three rules asr/optimizers.py:43-52 offers beside Adam
    (Chainer is an absent third party: formulas recalled from chainer/optimizers/{sgd,momentum_sgd,nesterov_ag}.py v2,
    PARITY UNPINNED; tests/test_oracle_misc.py pins kinds 0 and 1 to torch.optim.SGD and kind 2 to a hand-worked example):
      kind 0  SGD          p -= lr g
      kind 1  MomentumSGD  v = mu v - lr g;  p += v
      kind 2  NesterovAG   v = mu v - lr g;  p += mu^2 v - (1 + mu) lr g      (the NEW v)
    v may be None for kind 0 and comes back as it went in.  All float64."""
    g = g.astype(np.float64)
    g = g * gradient_factor((g ** 2).sum(), clip, grad_scale)
    g = g + decay * p
    if kind == 0:
        return p - lr * g, v
    v = momentum * v - lr * g
    if kind == 1:
        return p + v, v
    if kind == 2:
        return p + momentum * momentum * v - (1 + momentum) * lr * g, v
    raise ValueError(kind)


LOSS_SCALE_MIN, LOSS_SCALE_MAX = 2.0 ** -24, 2.0 ** 24


def step_control(g, state, clip, grad_scale, alpha, beta1, beta2, abort=False, reserved_index=-1, loss_scale=None):
    """What asr_step_control(_scaled) decides for one step: include/asr_hip.h, "optimiser step", in float64 and Python ints.

    g: the flat gradient; state = (applied steps so far, give-up drops so far = ctl[6]); abort: an abort word is raised;
    loss_scale: None or [S, applied steps since S changed, growth interval (0 = static), overflows so far].
    Returns (ctl[0..6], applied steps afterwards, the loss-scale quadruple afterwards or None):
      ctl[0] drop (1 / 0)   ctl[1] gradient factor   ctl[2] Adam's alpha_t   ctl[3] t   ctl[4] squared norm
      ctl[5] dropped because a recurrence gave up   ctl[6] such drops, ever.
    The step is dropped when the squared norm is not finite as a float32 (the device's format), an abort word is raised or the
    reserved element is not finite; the last two are a recurrence giving up and leave the loss scale alone.  Any other drop is
    an overflow: counted, and a dynamic scale is halved (not below 2^-24); `interval` applied steps in a row double it (not
    above 2^24).  The gradient factor carries 1 / S of the scale the backward pass was seeded with, and is left unclipped on a
    dropped step.  t counts applied steps only; alpha_t = alpha sqrt(1 - beta2^t) / (1 - beta1^t) with t clamped to >= 1.
    The hyperparameters are used as given: a caller that compares with the device passes the float32 values widened."""
    applied, gave_up_count = int(state[0]), float(state[1])
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = float((g ** 2).sum())
        finite = bool(np.isfinite(np.float32(sq)))
    drop = not finite
    gave_up = bool(abort)
    if reserved_index >= 0 and not np.isfinite(g[reserved_index]):
        gave_up = True
    if gave_up:
        drop = True
    ls = None
    if loss_scale is not None:
        ls = [float(x) for x in loss_scale]
        grad_scale = grad_scale / ls[0]
        if drop and not gave_up:
            if ls[2] > 0:
                ls[0] = max(ls[0] * 0.5, LOSS_SCALE_MIN)
            ls[1] = 0.0
            ls[3] += 1.0
        elif not drop:
            ls[1] += 1.0
            if ls[2] > 0 and ls[1] >= ls[2]:
                ls[0] = min(ls[0] * 2.0, LOSS_SCALE_MAX)
                ls[1] = 0.0
    rate = grad_scale if drop else gradient_factor(sq, clip, grad_scale)
    if not drop:
        applied += 1
    t = max(applied, 1)
    alpha_t = alpha * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    if gave_up:
        gave_up_count += 1.0
    ctl = [1.0 if drop else 0.0, float(rate), float(alpha_t), float(applied), sq, 1.0 if gave_up else 0.0, gave_up_count]
    return ctl, applied, ls


def batch_normalization(x, gamma, beta, avg_mean, avg_var, eps=2e-5, decay=0.9, train=True):
    """chainer.links.BatchNormalization as documented by Chainer (third party, absent: parity unpinned; torch's
    batch_norm is the cross-check in tests): x (B, C, ...) float64 numpy; returns y and the updated running averages."""
    import numpy as np
    axes = (0,) + tuple(range(2, x.ndim))
    shape = (1, -1) + (1,) * (x.ndim - 2)
    if train:
        mean, var = x.mean(axis=axes), x.var(axis=axes)
        n = x.size // x.shape[1]
        avg_mean = decay * avg_mean + (1 - decay) * mean
        avg_var = decay * avg_var + (1 - decay) * var * n / max(n - 1, 1)
    else:
        mean, var = avg_mean, avg_var
    y = gamma.reshape(shape) * (x - mean.reshape(shape)) / np.sqrt(var.reshape(shape) + eps) + beta.reshape(shape)
    return y, avg_mean, avg_var
