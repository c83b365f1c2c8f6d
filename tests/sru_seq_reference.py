"""float64 NumPy restatement of the SRU sequence layer (include/asr_hip.h, "SRU as a sequence layer"): forward and analytic backward.

Physical layout throughout: x (T, B, I), U (T, B, ndir, k, D), W (ndir, k D, I) rows [z; f; r (; p)], bias (ndir, 2 D) = [b_f; b_r],
cx / cy / dcy / dcx (ndir, B, D), C (ndir, T, B, D), y / gy (T, B, D), x_len (B) integers or None (= T everywhere; entries are clamped
to 0 .. T as the kernels clamp them).  ``scan_*`` start from a given U (what the kernels see), ``layer_*`` include the two products.

`mutant` names one deliberate error, for the tests that show the bars tell a wrong kernel from a right one:
  "thaw"      the state is not frozen in the padding (the scan runs on over the padded frames)
  "reverse_T" direction 1 starts at T - 1 in place of x_len - 1
  "highway_x" k = 4 takes the highway from x (cut or zero-filled to D columns) in place of the projection
"""
import numpy as np

U32 = 2.0 ** -24        # the unit roundoff of float32


def _sigmoid(a):
    """accurate to a few units of float64 RELATIVE to the value in both tails (1 + tanh cancels to an exact 0 below a = -37, where a
    float32 kernel still holds e^a)"""
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1.0, e) / (1.0 + e)


# ---------------------------------------------------------------------------------------------------------------- error shapes
# What float32 arithmetic of the kernels' form may differ from the float64 value by, element by element: the caps of the GPU tests are
# `slack` times these shapes plus half a unit of the format a value is stored in (bounds=True below returns them).
#   sigmoid  rcp(1 + __expf(-a)), a = U + b: the argument rounds (u |a|) and goes through the slope s (1 - s); __expf scales its argument
#            (relative error 2^-23 (1 + |a|) of e, again through s (1 - s)); the sum and the reciprocal cost 2^-22 s.
#   tanh     1 - 2 e rcp(1 + e), e = __expf(-2 |c|): 2^-23 (1 + 2 |c|) of e through 1 - g^2, 2^-21 |g| for quotient and product, and an
#            absolute 2^-23 for the subtraction where it cancels; an error E of c goes through 1 - g^2.
#   c        f (c' - z) + z with one fused rounding: E <- f E' + |c' - z| e_f + u (|c' - z| + |c|).
#   flush    below a = -87.3 the quotient is a float32 subnormal, which v_rcp_f32 gives as 0 (for a < -88.7 the exp overflows and the
#            quotient IS 0): where s is below 2^-125 the device's value may be 0, an error of s itself (the products formed from it,
#            gf = tx (c' - z) (1 - f) f first of all, can still be normal numbers).
def _e_sigmoid(s, a):
    return s * (1.0 - s) * (2.0 ** -23 * (1.0 + np.abs(a)) + U32 * np.abs(a)) + 2.0 ** -22 * s + np.where(s < 2.0 ** -125, s, 0.0)


def _e_tanh(g, c, E):
    return (1.0 - g * g) * (E + 2.0 ** -23 * (1.0 + 2.0 * np.abs(c))) + 2.0 ** -21 * np.abs(g) + 2.0 ** -23


def half_unit(v, bits=7):
    """half a unit in the last place of a format with `bits` stored fraction bits (7: the bfloat16 activations, 23: float32) at |v|;
    nothing below the smallest normal number is trusted (a device may flush it): at least 2^-126"""
    v = np.maximum(np.abs(v), 2.0 ** -126)
    return np.maximum(2.0 ** (np.floor(np.log2(v)) - bits - 1), 2.0 ** -126)


def lengths(x_len, T, B):
    return np.full((B,), T, dtype=np.int64) if x_len is None else np.clip(np.asarray(x_len, dtype=np.int64), 0, T)


def _order(direction, n, T, mutant):
    """the frames utterance-with-n-frames visits, in scan order"""
    if mutant == "thaw":
        n = T
    if direction == 0:
        return list(range(n))
    if mutant == "reverse_T":
        return list(range(T - 1, -1, -1))
    return list(range(n - 1, -1, -1))


def _highway(U, x, k, mutant):
    """xh (ndir, T, B, D): what the highway carries"""
    T, B, ndir, _, D = U.shape
    if k == 3:
        return np.broadcast_to(x[None], (ndir, T, B, D))
    if mutant == "highway_x":
        xx = np.zeros((T, B, D))
        w = min(D, x.shape[2])
        xx[..., :w] = x[..., :w]
        return np.broadcast_to(xx[None], (ndir, T, B, D))
    return np.moveaxis(U[:, :, :, 3, :], 2, 0)


def scan_fwd(U, x, bias, cx=None, x_len=None, use_tanh=True, mutant=None, bounds=False):
    """U (T, B, ndir, k, D) -> y (T, B, D), C (ndir, T, B, D) (NaN where the kernels write nothing: the padding), cy (ndir, B, D);
    bounds=True: and the error shapes (Ey, EC, Ecy) of float32 arithmetic (above), without the storage half units"""
    U = np.asarray(U, dtype=np.float64)
    T, B, ndir, k, D = U.shape
    bias = np.asarray(bias, dtype=np.float64).reshape(ndir, 2, D)
    n = lengths(x_len, T, B)
    xh = _highway(U, None if x is None else np.asarray(x, dtype=np.float64), k, mutant)
    y = np.zeros((T, B, D))
    C = np.full((ndir, T, B, D), np.nan)
    cy = np.zeros((ndir, B, D)) if cx is None else np.array(cx, dtype=np.float64)
    Ey, EC, Ecy = np.zeros((T, B, D)), np.zeros((ndir, T, B, D)), np.zeros((ndir, B, D))
    for d in range(ndir):
        for b in range(B):
            c = cy[d, b].copy()
            E = np.zeros(D)
            for t in _order(d, int(n[b]), T, mutant):
                z = U[t, b, d, 0]
                af, ar = U[t, b, d, 1] + bias[d, 0], U[t, b, d, 2] + bias[d, 1]
                f, r = _sigmoid(af), _sigmoid(ar)
                E = f * E + np.abs(c - z) * _e_sigmoid(f, af)
                c = f * c + (1.0 - f) * z
                E = E + U32 * (np.abs(c - z) + np.abs(c))
                C[d, t, b] = c
                EC[d, t, b] = E
                g = np.tanh(c) if use_tanh else c
                if t < n[b] or mutant == "thaw":
                    h = r * g + (1.0 - r) * xh[d, t, b]
                    y[t, b] += h
                    eg = _e_tanh(g, c, E) if use_tanh else E
                    Ey[t, b] += np.abs(g - xh[d, t, b]) * _e_sigmoid(r, ar) + r * eg + U32 * (2.0 * np.abs(r * (g - xh[d, t, b])) + 2.0 * np.abs(h))
            cy[d, b] = c
            Ecy[d, b] = E
    if bounds:
        return y, C, cy, (Ey + U32 * np.abs(y), EC, Ecy)
    return y, C, cy


def scan_bwd(U, x, bias, C, cx, x_len, gy, dcy=None, use_tanh=True, bounds=False):
    """-> gU (T, B, ndir, k, D), gxh (T, B, D) (the highway's gradient of x; zeros for k = 4), gbias (ndir, 2 D), dcx (ndir, B, D);
    bounds=True: and the error shapes (EgU, Egxh, Egbias, Edcx) of float32 arithmetic on exactly these inputs (C is an input: the
    kernels read the saved states), without the storage half units"""
    U = np.asarray(U, dtype=np.float64)
    T, B, ndir, k, D = U.shape
    bias = np.asarray(bias, dtype=np.float64).reshape(ndir, 2, D)
    n = lengths(x_len, T, B)
    xh = _highway(U, None if x is None else np.asarray(x, dtype=np.float64), k, None)
    gy = np.asarray(gy, dtype=np.float64)
    gU = np.zeros_like(U)
    gxh = np.zeros((T, B, D))
    gbias = np.zeros((ndir, 2, D))
    dcx = np.zeros((ndir, B, D)) if dcy is None else np.array(dcy, dtype=np.float64)
    c0 = np.zeros((ndir, B, D)) if cx is None else np.asarray(cx, dtype=np.float64)
    EgU, Egxh, Egb, Edcx = np.zeros_like(U), np.zeros((T, B, D)), np.zeros((ndir, 2, D)), np.zeros((ndir, B, D))
    Sgb = np.zeros((ndir, 2, D))        # sum of magnitudes and number of terms, for the float32 sums of the bias gradients
    terms = int(n.sum())
    for d in range(ndir):
        for b in range(B):
            order = _order(d, int(n[b]), T, None)
            gc = dcx[d, b].copy()
            E = np.zeros(D)
            for i in range(len(order) - 1, -1, -1):
                t = order[i]
                cp = c0[d, b] if i == 0 else C[d, order[i - 1], b]
                z = U[t, b, d, 0]
                f = _sigmoid(U[t, b, d, 1] + bias[d, 0])
                r = _sigmoid(U[t, b, d, 2] + bias[d, 1])
                c = C[d, t, b]
                g = np.tanh(c) if use_tanh else c
                gh = gy[t, b]
                gr = gh * (g - xh[d, t, b]) * r * (1.0 - r)
                tx = gh * r * ((1.0 - g * g) if use_tanh else 1.0) + gc
                gf = tx * (cp - z) * f * (1.0 - f)
                gU[t, b, d, 0] = tx * (1.0 - f)
                gU[t, b, d, 1] = gf
                gU[t, b, d, 2] = gr
                if k == 4:
                    gU[t, b, d, 3] = gh * (1.0 - r)
                else:
                    gxh[t, b] += gh * (1.0 - r)
                gbias[d, 0] += gf
                gbias[d, 1] += gr
                # error shapes: every product rounds once per factor; the factors' own errors go through the other factors
                af, ar = U[t, b, d, 1] + bias[d, 0], U[t, b, d, 2] + bias[d, 1]
                ef, er = _e_sigmoid(f, af), _e_sigmoid(r, ar)
                eg = _e_tanh(g, c, 0.0) if use_tanh else np.zeros(D)
                dg = (1.0 - g * g) if use_tanh else 1.0
                egct = np.abs(gh) * (er * dg + r * 2.0 * np.abs(g) * eg) + 4.0 * U32 * np.abs(gh * r * dg)
                Etx = egct + E + U32 * np.abs(tx)
                EgU[t, b, d, 0] = Etx * (1.0 - f) + np.abs(tx) * ef + 3.0 * U32 * np.abs(tx * (1.0 - f))
                egf = Etx * np.abs((cp - z) * f * (1.0 - f)) + np.abs(tx * (cp - z)) * ef + 6.0 * U32 * np.abs(gf)
                EgU[t, b, d, 1] = egf
                egr = np.abs(gh) * (eg * r * (1.0 - r) + np.abs(g - xh[d, t, b]) * er) + 6.0 * U32 * np.abs(gr)
                EgU[t, b, d, 2] = egr
                ep = np.abs(gh) * er + 2.0 * U32 * np.abs(gh * (1.0 - r))
                if k == 4:
                    EgU[t, b, d, 3] = ep
                else:
                    Egxh[t, b] += ep + U32 * np.abs(gxh[t, b])
                Egb[d, 0] += egf
                Egb[d, 1] += egr
                Sgb[d, 0] += np.abs(gf)
                Sgb[d, 1] += np.abs(gr)
                E = Etx * f + np.abs(tx) * ef + U32 * np.abs(tx * f)
                gc = tx * f
            dcx[d, b] = gc
            Edcx[d, b] = E
    gbias = gbias.reshape(ndir, 2 * D)
    if bounds:      # the bias sums: registers over t, LDS over batch rows, float atomics over workgroups -- any order
        return gU, gxh, gbias, dcx, (EgU, Egxh, (Egb + (terms + 4) * U32 * Sgb).reshape(ndir, 2 * D), Edcx)
    return gU, gxh, gbias, dcx


def project(x, W):
    """U (T, B, ndir, k, D) = W x"""
    x = np.asarray(x, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    T, B, I = x.shape
    ndir = W.shape[0]
    D = W.shape[1] // (3 if I * 3 == W.shape[1] else 4)
    k = W.shape[1] // D
    return (x.reshape(T * B, I) @ W.reshape(ndir * k * D, I).T).reshape(T, B, ndir, k, D)


def layer_fwd(x, W, bias, cx=None, x_len=None, use_tanh=True, mutant=None):
    """x (T, B, I), W (ndir, k D, I): k = 3 exactly when I == D -> y, C, cy"""
    U = project(x, W)
    assert (U.shape[3] == 3) == (x.shape[2] == U.shape[4])
    return scan_fwd(U, x, bias, cx, x_len, use_tanh, mutant)


def layer_bwd(x, W, bias, cx, x_len, gy, dcy=None, use_tanh=True):
    """-> gx (T, B, I), gW (ndir, k D, I), gbias (ndir, 2 D), dcx (ndir, B, D)"""
    x = np.asarray(x, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    T, B, I = x.shape
    U = project(x, W)
    _, C, _ = scan_fwd(U, x, bias, cx, x_len, use_tanh)
    gU, gxh, gbias, dcx = scan_bwd(U, x, bias, C, cx, x_len, gy, dcy, use_tanh)
    g2 = gU.reshape(T * B, -1)
    gW = (g2.T @ x.reshape(T * B, I)).reshape(W.shape)
    gx = (g2 @ W.reshape(-1, I)).reshape(T, B, I)
    if U.shape[3] == 3:
        gx = gx + gxh
    return gx, gW, gbias, dcx
