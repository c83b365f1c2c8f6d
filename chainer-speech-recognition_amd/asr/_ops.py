"""Thin, autograd-free Python faces of the C ABI (include/asr_hip.h): shape checks + pointer plumbing only.

Everything numeric happens inside libasr_hip.so.  torch is used for allocation and stream handles.
"""
import os

import torch

from . import _lib
from ._lib import check, ptr, stream

BF16 = _lib.act_dtype()      # the 16-bit activation format of the loaded library: bfloat16 (default build) or float16 (ASR_ACT=f16)
F32 = torch.float32


def _is_bf16(t):
    if t.dtype == BF16:
        return 1
    if t.dtype == F32:
        return 0
    raise TypeError("expected float32 or bfloat16, got %s" % t.dtype)


def gemm_nt(a, b, bias=None, out_dtype=BF16, out=None):
    """C[M,N] = a[M,K] @ b[N,K]^T (+ bias).  a, b bf16 with unit inner stride."""
    assert a.dtype == BF16 and b.dtype == BF16 and a.dim() == 2 and b.dim() == 2
    assert a.stride(1) == 1 and b.stride(1) == 1 and a.shape[1] == b.shape[1]
    M, K = a.shape
    N = b.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    assert out.stride(1) == 1
    rc = _lib.lib().asr_gemm_nt(stream(), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(),
                                out.stride(0), ptr(bias), M, N, K, _is_bf16(out))
    check(rc, "asr_gemm_nt")
    return out


def gemm_nt_8ph(a, b, bias=None, out_dtype=BF16, out=None):
    """gemm_nt on the 256 x 256 tile / eight-wave kernel only (asr_gemm_nt_8ph: tests and timings; asr_gemm_nt routes to it by itself);
    raises when the product does not qualify (K % 64, N % 4, alignment)"""
    assert a.dtype == BF16 and b.dtype == BF16 and a.dim() == 2 and b.dim() == 2
    assert a.stride(1) == 1 and b.stride(1) == 1 and a.shape[1] == b.shape[1]
    M, K = a.shape
    N = b.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    assert out.stride(1) == 1
    rc = _lib.lib().asr_gemm_nt_8ph(stream(), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(),
                                    out.stride(0), ptr(bias), M, N, K, _is_bf16(out))
    check(rc, "asr_gemm_nt_8ph")
    return out


def gemm_tn_acc(a, b, c):
    """c[M,N] += a[K,M]^T @ b[K,N]; a, b bf16 row-major (unit inner stride), c f32."""
    assert a.dtype == BF16 and b.dtype == BF16 and c.dtype == F32
    assert a.stride(1) == 1 and b.stride(1) == 1 and c.stride(1) == 1 and a.shape[0] == b.shape[0]
    K, M = a.shape
    N = b.shape[1]
    assert c.shape == (M, N)
    rc = _lib.lib().asr_gemm_tn_acc(stream(), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
                                    c.stride(0), M, N, K)
    check(rc, "asr_gemm_tn_acc")
    return c


TN_GROUP = [_lib.debug_flag("tn_group", 1) != 0]     # ASR_DEBUG tn_group=0: one launch per product (comparison)


def gemm_tn_acc_group(products):
    """c += a^T @ b for up to four (a, b, c) triples in one launch (gemm_tn_acc's operand rules for each)."""
    n = len(products)
    assert 1 <= n <= 4
    if not TN_GROUP[0]:
        for a, b, c in products:
            gemm_tn_acc(a, b, c)
        return
    for a, b, c in products:
        assert a.dtype == BF16 and b.dtype == BF16 and c.dtype == F32
        assert a.stride(1) == 1 and b.stride(1) == 1 and c.stride(1) == 1 and a.shape[0] == b.shape[0]
        assert c.shape == (a.shape[1], b.shape[1])
    import ctypes
    ptrs = lambda k: (ctypes.c_void_p * n)(*[p[k].data_ptr() for p in products])
    ints = lambda f: (ctypes.c_int * n)(*[f(p) for p in products])
    rc = _lib.lib().asr_gemm_tn_acc_group(stream(), n, ptrs(0), ints(lambda p: p[0].stride(0)), ptrs(1),
                                          ints(lambda p: p[1].stride(0)), ptrs(2), ints(lambda p: p[2].stride(0)),
                                          ints(lambda p: p[0].shape[1]), ints(lambda p: p[1].shape[1]),
                                          ints(lambda p: p[0].shape[0]))
    check(rc, "asr_gemm_tn_acc_group")


def gemm_tn_acc_group_8ph(products):
    """gemm_tn_acc_group on the 256 x 256 tile / eight-wave kernel only (asr_gemm_tn_acc_group_8ph: tests and timings)"""
    n = len(products)
    assert 1 <= n <= 4
    import ctypes
    ptrs = lambda k: (ctypes.c_void_p * n)(*[p[k].data_ptr() for p in products])
    ints = lambda f: (ctypes.c_int * n)(*[f(p) for p in products])
    rc = _lib.lib().asr_gemm_tn_acc_group_8ph(stream(), n, ptrs(0), ints(lambda p: p[0].stride(0)), ptrs(1),
                                              ints(lambda p: p[1].stride(0)), ptrs(2), ints(lambda p: p[2].stride(0)),
                                              ints(lambda p: p[0].shape[1]), ints(lambda p: p[1].shape[1]),
                                              ints(lambda p: p[0].shape[0]))
    check(rc, "asr_gemm_tn_acc_group_8ph")


def cast_bf16(src, transpose=False, out=None):
    """f32 (rows, cols) -> bf16 copy, optionally transposed; `out`: a contiguous bf16 tensor of the result's size."""
    assert src.dtype == F32 and src.is_contiguous()
    s2 = src.reshape(src.shape[0], -1) if src.dim() != 2 else src
    rows, cols = s2.shape
    dst = out if out is not None else torch.empty((cols, rows) if transpose else (rows, cols), dtype=BF16, device=src.device)
    assert dst.dtype == BF16 and dst.is_contiguous() and dst.numel() == rows * cols
    check(_lib.lib().asr_cast_bf16(stream(), ptr(s2), ptr(dst), rows, cols, int(transpose)), "asr_cast_bf16")
    return dst


def bf16_to_f32(src):
    dst = torch.empty(src.shape, dtype=F32, device=src.device)
    check(_lib.lib().asr_bf16_to_f32(stream(), ptr(src.contiguous()), ptr(dst), src.numel()), "asr_bf16_to_f32")
    return dst


def permute4(src, shape, strides, out_dtype):
    """dense (d0,d1,d2,d3) tensor of `out_dtype` gathered from `src` storage with the given element strides."""
    dst = torch.empty(shape, dtype=out_dtype, device=src.device)
    rc = _lib.lib().asr_permute4(stream(), src.data_ptr(), _is_bf16(src), ptr(dst), _is_bf16(dst), *shape, *strides)
    check(rc, "asr_permute4")
    return dst


def im2col(x, strides_tbhc, T, B, Hin, Cin, KH, KW, pad_h, pad_t=None, Tout=None):
    """pad_t defaults to KW-1 and Tout to T: the causal convolution."""
    pad_t = KW - 1 if pad_t is None else pad_t
    Tout = T if Tout is None else Tout
    Kp = (KH * KW * Cin + 7) // 8 * 8
    Hout = Hin + 2 * pad_h - KH + 1
    col = torch.empty((Tout * B * Hout, Kp), dtype=BF16, device=x.device)
    rc = _lib.lib().asr_im2col(stream(), x.data_ptr(), _is_bf16(x), *strides_tbhc, T, B, Hin, Cin, KH, KW, pad_h, pad_t,
                               Tout, Kp, ptr(col))
    check(rc, "asr_im2col")
    return col


def col2im(dcol, T, B, Hin, Cin, KH, KW, pad_h, pad_t=None, Tout=None):
    pad_t = KW - 1 if pad_t is None else pad_t
    Tout = T if Tout is None else Tout
    Kp = dcol.shape[1]
    dx = torch.empty((T, B, Hin, Cin), dtype=BF16, device=dcol.device)
    check(_lib.lib().asr_col2im(stream(), ptr(dcol), T, B, Hin, Cin, KH, KW, pad_h, pad_t, Tout, Kp, ptr(dx)), "asr_col2im")
    return dx


def conv_weight_pack(W, transpose=False, Kp=None):
    """(Co, Ci, kh, kw) f32 -> bf16 (Co, Kp) [or (Kp, Co)], k = (kh, kw, ci), Kp = K rounded up to 8 (or as given), zero padded."""
    assert W.dtype == F32 and W.is_contiguous() and W.dim() == 4
    Co, Ci, KH, KW = W.shape
    Kp = (KH * KW * Ci + 7) // 8 * 8 if Kp is None else int(Kp)
    dst = torch.empty((Kp, Co) if transpose else (Co, Kp), dtype=BF16, device=W.device)
    check(_lib.lib().asr_conv_weight_pack(stream(), ptr(W), ptr(dst), Co, Ci, KH, KW, Kp, int(transpose)), "asr_conv_weight_pack")
    return dst


def conv_weight_grad_unpack(scratch, gW, channel_pitch=0):
    """gW (Co, Ci, KH, KW) += scratch (Co, Kp) with k = (kh, kw, c), c < channel_pitch (0: Ci); a scratch of shape (copies, Co, Kp)
    (per-XCD copies, conv_tn_copies) is summed over its first axis on the way"""
    Co, Ci, KH, KW = gW.shape
    assert scratch.dtype == F32 and scratch.is_contiguous() and gW.is_contiguous()
    copies = scratch.shape[0] if scratch.dim() == 3 else 1
    check(_lib.lib().asr_conv_weight_grad_unpack_copies(stream(), ptr(scratch), copies, ptr(gW), Co, Ci, KH, KW, scratch.shape[-1],
                                                        int(channel_pitch)), "asr_conv_weight_grad_unpack_copies")


def conv_tn_copies(Co, Cs, KH, KW):
    """8 if the weight-gradient kernel wants one scratch copy per XCD for this layer (few output tiles), else 1"""
    return int(_lib.lib().asr_conv_tn_copies(int(Co), int(Cs), int(KH), int(KW)))


def conv_tn_acc(g2, x, scratch, KH, KW, pad_h, pad_t, Tr, Hr):
    """scratch (Co, KH*KW*Cs) f32 += weight gradient of the convolution that maps x (Ts, B, Hs, Cs) bf16 to (Tr, B, Hr, Co),
    g2 (Tr*B*Hr, Co) bf16 its output gradient: the implicit form of gemm_tn_acc(g2, im2col(x), scratch).  scratch may be
    (8, Co, KH*KW*Cs) where conv_tn_copies says so: every XCD adds into its own copy."""
    Ts, B, Hs, Cs = x.shape
    Co = g2.shape[1]
    assert x.dtype == BF16 and g2.dtype == BF16 and scratch.dtype == F32 and g2.shape[0] == Tr * B * Hr
    copies = scratch.shape[0] if scratch.dim() == 3 else 1
    assert tuple(scratch.shape[-2:]) == (Co, KH * KW * Cs) and scratch.is_contiguous() and copies in (1, 8)
    rc = _lib.lib().asr_conv_tn_acc_copies(stream(), ptr(g2), g2.stride(0), ptr(x), ptr(scratch), scratch.shape[-1], copies, Co, Ts, B,
                                           Hs, Cs, KH, KW, pad_h, pad_t, Tr, Hr)
    check(rc, "asr_conv_tn_acc_copies")


def conv_tn_acc_8ph(g2, x, scratch, KH, KW, pad_h, pad_t, Tr, Hr):
    """conv_tn_acc on the eight-wave kernel only (asr_conv_tn_acc_8ph: tests and timings; asr_conv_tn_acc dispatches by itself)"""
    Ts, B, Hs, Cs = x.shape
    Co = g2.shape[1]
    assert tuple(scratch.shape) == (Co, KH * KW * Cs) and scratch.is_contiguous()
    rc = _lib.lib().asr_conv_tn_acc_8ph(stream(), ptr(g2), g2.stride(0), ptr(x), ptr(scratch), scratch.shape[-1], Co, Ts, B, Hs, Cs, KH, KW,
                                        pad_h, pad_t, Tr, Hr)
    check(rc, "asr_conv_tn_acc_8ph")


ACT_KINDS = {"relu": 0, "clipped_relu": 1, "leaky_relu": 2, "elu": 3, "sigmoid": 4, "tanh": 5, "hard_sigmoid": 6,
             "softplus": 7}


def activation_fwd(x, kind, alpha=0.0):
    assert x.dtype == BF16 and x.is_contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().asr_activation_fwd(stream(), ptr(x), ptr(y), x.numel(), ACT_KINDS[kind], float(alpha)), "asr_activation_fwd")
    return y


def activation_bwd(x, dy, kind, alpha=0.0):
    dx = torch.empty_like(x)
    check(_lib.lib().asr_activation_bwd(stream(), ptr(x), ptr(dy.contiguous()), ptr(dx), x.numel(), ACT_KINDS[kind],
                                        float(alpha)), "asr_activation_bwd")
    return dx


def glu_fwd(x):
    """x (..., 2C) bf16 -> (..., C): A * sigmoid(B)."""
    assert x.dtype == BF16 and x.is_contiguous() and x.shape[-1] % 2 == 0
    C = x.shape[-1] // 2
    y = torch.empty(x.shape[:-1] + (C,), dtype=BF16, device=x.device)
    check(_lib.lib().asr_glu_fwd(stream(), ptr(x), ptr(y), x.numel() // (2 * C), C), "asr_glu_fwd")
    return y


def glu_bwd(x, dy):
    C = x.shape[-1] // 2
    dx = torch.empty_like(x)
    check(_lib.lib().asr_glu_bwd(stream(), ptr(x), ptr(dy.contiguous()), ptr(dx), x.numel() // (2 * C), C), "asr_glu_bwd")
    return dx


def dropout(x, ratio, seed):
    assert x.dtype == BF16
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().asr_dropout(stream(), ptr(x), ptr(y), x.numel(), float(ratio), int(seed) & 0xffffffff), "asr_dropout")
    return y


def maxout2_fwd(x):
    assert x.dtype == BF16 and x.is_contiguous() and x.shape[-1] % 2 == 0
    y = torch.empty(x.shape[:-1] + (x.shape[-1] // 2,), dtype=BF16, device=x.device)
    check(_lib.lib().asr_maxout2_fwd(stream(), ptr(x), ptr(y), y.numel()), "asr_maxout2_fwd")
    return y


def maxout2_bwd(x, dy):
    dx = torch.empty_like(x)
    check(_lib.lib().asr_maxout2_bwd(stream(), ptr(x), ptr(dy.contiguous()), ptr(dx), dy.numel()), "asr_maxout2_bwd")
    return dx


def pooled_height(Hin, k):
    return 1 if Hin <= k else -(-(Hin - k) // k) + 1


def maxout2_pool_ok(x):
    return x.dtype == BF16 and x.dim() == 4 and x.is_contiguous() and x.shape[3] % 16 == 0


def maxout2_pool_fwd(x, k):
    """x (T, B, H, 2C) bf16 -> (T, B, ceil(H / k), C): Maxout(2) then MaxPooling2D((k, 1)) in one pass."""
    T, B, H, C2 = x.shape
    y = torch.empty((T, B, pooled_height(H, k), C2 // 2), dtype=BF16, device=x.device)
    check(_lib.lib().asr_maxout2_pool_fwd(stream(), ptr(x), ptr(y), T * B, H, C2 // 2, k), "asr_maxout2_pool_fwd")
    return y


def maxout2_pool_bwd(x, dy, k, db=None):
    """dx of maxout(2) + max pooling over (k, 1); db (2 C floats, optional) += column sums of dx (bias gradient of the producer)"""
    T, B, H, C2 = x.shape
    dx = torch.empty_like(x)
    if db is not None:
        assert db.dtype == F32 and db.numel() == C2 and db.is_contiguous()
    check(_lib.lib().asr_maxout2_pool_bwd_db(stream(), ptr(x), ptr(dy.contiguous()), ptr(dx), ptr(db), T * B, H, C2 // 2, k),
          "asr_maxout2_pool_bwd_db")
    return dx


def maxout2_pool_bwd_db_ok(C):
    return bool(_lib.lib().asr_maxout2_pool_bwd_db_ok(int(C)))


def maxpool_h_fwd(x, k):
    """x (T, B, H, C) bf16 -> (T, B, Hout, C)."""
    assert x.dtype == BF16 and x.is_contiguous() and x.dim() == 4
    T, B, H, C = x.shape
    y = torch.empty((T, B, pooled_height(H, k), C), dtype=BF16, device=x.device)
    check(_lib.lib().asr_maxpool_h_fwd(stream(), ptr(x), ptr(y), T * B, H, C, k), "asr_maxpool_h_fwd")
    return y


def maxpool_h_bwd(x, dy, k):
    T, B, H, C = x.shape
    dx = torch.empty_like(x)
    check(_lib.lib().asr_maxpool_h_bwd(stream(), ptr(x), ptr(dy.contiguous()), ptr(dx), T * B, H, C, k), "asr_maxpool_h_bwd")
    return dx


def add_bf16(a, b):
    assert a.dtype == BF16 and b.dtype == BF16 and a.shape == b.shape
    y = torch.empty_like(a, memory_format=torch.contiguous_format)
    check(_lib.lib().asr_add_bf16(stream(), ptr(a.contiguous()), ptr(b.contiguous()), ptr(y), y.numel()), "asr_add_bf16")
    return y


def colsum_acc(x, out):
    """out[c] += sum_r x[r][c]; x 2-d (unit inner stride), out f32."""
    assert x.dim() == 2 and x.stride(1) == 1 and out.dtype == F32
    rc = _lib.lib().asr_colsum_acc(stream(), x.data_ptr(), _is_bf16(x), x.shape[0], x.shape[1], x.stride(0), ptr(out))
    check(rc, "asr_colsum_acc")
    return out


def layernorm_fwd(x, gamma, beta, C, out_dtype, want_lse=False):
    """x (rows, D) f32/bf16; statistics per row; channel = index % C.  want_lse (float32 rows normalised over their whole width only):
    also the log-sum-exp of every output row, formed while the row is in registers -> (y, mean, rstd, lse)"""
    assert x.dim() == 2 and x.is_contiguous()
    rows, D = x.shape
    y = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=F32, device=x.device)
    rstd = torch.empty(rows, dtype=F32, device=x.device)
    if want_lse:
        assert x.dtype == F32 and out_dtype == F32 and _lib.lib().asr_layernorm_fwd_lse_ok(D, C)
        lse = torch.empty(rows, dtype=F32, device=x.device)
        rc = _lib.lib().asr_layernorm_fwd_lse(stream(), ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(lse), rows, D)
        check(rc, "asr_layernorm_fwd_lse")
        return y, mean, rstd, lse
    rc = _lib.lib().asr_layernorm_fwd(stream(), ptr(x), _is_bf16(x), ptr(y), _is_bf16(y), ptr(gamma), ptr(beta),
                                      ptr(mean), ptr(rstd), rows, D, C)
    check(rc, "asr_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, C, dx_dtype, dgamma=None, dbeta=None, need_dx=True):
    """dx (of dx_dtype) and dgamma += / dbeta +=.  float32 x and dy (the logits path) take the one-sweep kernel
    (asr_layernorm_bwd_rows: dx and the column sums in one pass), everything else asr_layernorm_bwd."""
    rows, D = x.shape
    dy = dy.contiguous()
    dx = torch.empty((rows, D), dtype=dx_dtype, device=x.device) if need_dx else None
    lib = _lib.lib()
    if x.dtype == F32 and dy.dtype == F32 and C % 4 == 0:
        nbytes = lib.asr_layernorm_bwd_rows_ws_bytes(rows, D)
        if nbytes > 0:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if dgamma is not None else None
            rc = lib.asr_layernorm_bwd_rows(stream(), ptr(x), ptr(dy), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx),
                                            _is_bf16(dx) if need_dx else 0, ptr(dgamma), ptr(dbeta), rows, D, C, ptr(ws), nbytes)
            check(rc, "asr_layernorm_bwd_rows")
            return dx
    rc = lib.asr_layernorm_bwd(stream(), ptr(x), _is_bf16(x), ptr(dy), _is_bf16(dy), ptr(gamma), ptr(mean),
                               ptr(rstd), ptr(dx), _is_bf16(dx) if need_dx else 0, ptr(dgamma), ptr(dbeta),
                               rows, D, C)
    check(rc, "asr_layernorm_bwd")
    return dx


CALLS = {}          # call counters of a few entry points (tests check which path ran)


def layernorm_ctc_bwd(x, gamma, beta, mean, rstd, T, B, dx_dtype, dgamma, dbeta, need_dx, recipes, dxsum=None):
    """asr_layernorm_ctc_bwd: `recipes` = one or two dicts left by CTC-family losses on the normalised rows (asr/loss/ctc.py):
    ws, Lmax, gram, x_len, gy, gy_per_utt, scale"""
    rows, V = x.shape
    assert x.dtype == F32 and x.is_contiguous() and rows == T * B and 1 <= len(recipes) <= 2
    CALLS["layernorm_ctc_bwd"] = CALLS.get("layernorm_ctc_bwd", 0) + 1
    lib = _lib.lib()
    dx = torch.empty((rows, V), dtype=dx_dtype, device=x.device) if need_dx else None
    nbytes = lib.asr_layernorm_ctc_bwd_ws_bytes(T, B, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if dgamma is not None else None
    args = []
    for r in (recipes + recipes)[:2]:
        args += [ptr(r["ws"]), int(r["Lmax"]), int(r["gram"]), ptr(r["x_len"]), ptr(r["gy"]), int(r["gy_per_utt"]), float(r["scale"])]
    rc = lib.asr_layernorm_ctc_bwd(stream(), ptr(x), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(dx), _is_bf16(dx) if need_dx else 0,
                                   ptr(dgamma), ptr(dbeta), T, B, V, ptr(ws), nbytes, len(recipes), *args, ptr(dxsum))
    check(rc, "asr_layernorm_ctc_bwd")
    return dx


GRU_MODE = [int(os.environ.get("ASR_GRU_MODE", "0"))]      # (ASR_GRU_MODE: rehearsals with several processes on one GPU use 1)  asr_hip.h: 0 automatic, 1 per-step launches, 2 persistent placement-free, 4 local with flags, 7 forged placement, 8 local with polled payload (= 0), 9 / 10 partial-sum backward (asked for / forged placement)


_SYNC = {}          # (device index, stream) -> one reusable control buffer; its abort word (int 1023) is sticky
_STATUS = {}        # (device index, stream) -> [pinned host word, event of the copy in flight]


def _sync_buffer(dev, nbytes):
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _SYNC.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.zeros(max(nbytes // 4 + 1, 2048), dtype=torch.int32, device=dev)
        _SYNC[key] = buf
    return buf


def gru_poll_status():
    """Called once per step (optimizer.update): looks, without synchronising, at the abort words copied out during the
    previous step and raises if a persistent GRU launch gave up; then queues this step's copy."""
    for key, buf in list(_SYNC.items()):         # one control buffer per (device, stream) that launched a recurrence
        st = _STATUS.get(key)
        if st is None:
            st = _STATUS[key] = [torch.zeros(1, dtype=torch.int32).pin_memory(), None]
        if st[1] is not None and st[1].query() and int(st[0][0]) != 0:
            code = int(st[0][0])
            buf[1023:1024].zero_()
            st[0][0] = 0
            st[1] = None
            raise _lib.AsrHipError("a persistent GRU kernel gave up an in-launch wait (code %d): the results of that step are "
                                   "invalid" % code)
        if st[1] is None or st[1].query():
            st[0].copy_(buf[1023:1024], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            st[1] = ev


def reset_poll_status():
    """forget the abort-word copies in flight (the optimiser has just reported and cleared the words)"""
    for st in _STATUS.values():
        st[0][0] = 0
        st[1] = None


# asr.parallel hangs two callables here during a data-parallel backward pass: "before" runs before a recurrence is
# queued (the launch stream then waits for every collective in flight), "after" right behind it (complete gradient slices
# are all-reduced in the gap that follows).  A persistent recurrence wants every CU; see asr/parallel.py.
RECURRENCE_HOOKS = {"before": None, "after": None}


def _hook(name):
    fn = RECURRENCE_HOOKS[name]
    if fn is not None:
        fn()


GRU_GI_BF16 = [True]        # write the input projections in bf16 where the recurrence kernel takes them (tests may switch it off)
# saved gates in IEEE half, blocked by workgroup, where the default kernel pair serves (asr_hip.h): a row's r | z | n | q of 16 units
# are ONE 128-B line instead of four 64-B pieces of four lines.  Measured at T=1000, B=32, H=512: forward 1.256 -> 1.210 us per step,
# backward 1.347 -> 1.329 (half gates in the plain [4][H] layout had bought nothing: the CU's memory queue beside the hand-off is
# bound by the NUMBER of requests).  ASR_DEBUG gru_gates_f16=0 keeps float32 gates.
GRU_GATES_F16 = [_lib.debug_flag("gru_gates_f16", 1) != 0]


def gru_gates_standard(gates, H):
    """the saved gates as float32 (T*B, ndir, 4, H) whatever form gru_fwd kept them in (tests, inspection): the half form is blocked
    by workgroup, (T*B, ndir, H/16, 4, 16) -- asr_hip.h"""
    if gates.dtype != torch.float16:
        return gates
    rows, ndir = gates.shape[0], gates.shape[1]
    return gates.reshape(rows, ndir, H // 16, 4, 16).permute(0, 1, 3, 2, 4).reshape(rows, ndir, 4, H).float()


def gru_gates_f16(T, B, H, ndir):
    """whether a recurrence of this shape keeps its saved gates in half precision (the rounding-matched oracle asks)"""
    return bool(GRU_GATES_F16[0] and _lib.lib().asr_gru_gates_f16_ok(T, B, H, ndir, GRU_MODE[0]))


def gru_gi_dtype(T, B, H, ndir):
    """dtype the input-projection GEMM should write for the recurrence that follows: bf16 when the kernel serving this
    shape streams it (half the projection's output bytes and of the recurrence's loader traffic), else float32"""
    if GRU_GI_BF16[0] and _lib.lib().asr_gru_fwd_accepts_bf16_gi(T, B, H, ndir, GRU_MODE[0]):
        return BF16
    return F32


def _len_i32(x_len, B, dev):
    if x_len is None:
        return None
    if x_len.dtype != torch.int32 or x_len.numel() != B or x_len.device != dev:
        raise ValueError("x_length must be %d int32 frame counts on %s" % (B, dev))
    return x_len.contiguous()


def gru_fwd(gi, whh16, bhh, T, B, H, ndir, x_len=None):
    """x_len (B) int32 or None: per-utterance lengths (asr_hip.h: the dead rows' update-gate columns of gi are overwritten)"""
    dev = gi.device
    x_len = _len_i32(x_len, B, dev)
    sync = _sync_buffer(dev, _lib.lib().asr_gru_sync_bytes(B, H, ndir))
    hseq = torch.empty((T * B, ndir * H), dtype=F32, device=dev)
    hseq16 = torch.empty((T * B, ndir * H), dtype=BF16, device=dev)
    f16 = bool(GRU_GATES_F16[0] and _lib.lib().asr_gru_gates_f16_ok(T, B, H, ndir, GRU_MODE[0]))
    gates = torch.empty((T * B, ndir, 4, H), dtype=torch.float16 if f16 else F32, device=dev)
    y = torch.empty((T * B, H), dtype=BF16, device=dev)
    rc = _lib.lib().asr_gru_fwd(stream(), ptr(gi), _is_bf16(gi), ptr(whh16), ptr(bhh), ptr(hseq), ptr(hseq16), ptr(gates), ptr(y),
                                T, B, H, ndir, ptr(sync), GRU_MODE[0], ptr(x_len), int(f16))
    check(rc, "asr_gru_fwd")
    LAST_SYNC[0] = sync
    return y, hseq, hseq16, gates


def gru_fwd_state(gi, whh16, bhh, hx, T, B, H, ndir, x_len=None):
    """the layer with an initial state hx (ndir, B, H) float32 (asr_gru_fwd_state: per-step kernels, float32 gi and gates)"""
    dev = gi.device
    assert gi.dtype == F32 and hx.dtype == F32 and hx.shape == (ndir, B, H) and hx.is_contiguous()
    x_len = _len_i32(x_len, B, dev)
    hseq = torch.empty((T * B, ndir * H), dtype=F32, device=dev)
    hseq16 = torch.empty((T * B, ndir * H), dtype=BF16, device=dev)
    gates = torch.empty((T * B, ndir, 4, H), dtype=F32, device=dev)
    y = torch.empty((T * B, H), dtype=BF16, device=dev)
    rc = _lib.lib().asr_gru_fwd_state(stream(), ptr(gi), ptr(whh16), ptr(bhh), ptr(hx), ptr(hseq), ptr(hseq16), ptr(gates), ptr(y),
                                      T, B, H, ndir, ptr(x_len))
    check(rc, "asr_gru_fwd_state")
    return y, hseq, hseq16, gates


def gru_bwd_state(dy, gates, hseq, hx, dhy, whhT16, T, B, H, ndir, db_ih=None, db_hh=None, x_len=None):
    """-> dgi, dgh (bf16 rows) and dhx (ndir, B, H) float32; dhy: gradient of the final state or None"""
    dev = dy.device
    x_len = _len_i32(x_len, B, dev)
    dy_ws = torch.empty((T * B, H), dtype=BF16, device=dev) if x_len is not None else None
    dgi = torch.empty((T * B, ndir * 3 * H), dtype=BF16, device=dev)
    dgh = torch.empty((T * B, ndir * 3 * H), dtype=BF16, device=dev)
    carry = torch.empty((ndir, B, H), dtype=F32, device=dev)
    dhx = torch.empty((ndir, B, H), dtype=F32, device=dev)
    rc = _lib.lib().asr_gru_bwd_state(stream(), ptr(dy.contiguous()), ptr(gates), ptr(hseq), ptr(hx), None if dhy is None else ptr(dhy.contiguous()),
                                      ptr(whhT16), ptr(dgi), ptr(dgh), ptr(carry), ptr(db_ih), ptr(db_hh), ptr(dhx), T, B, H, ndir,
                                      ptr(x_len), ptr(dy_ws))
    check(rc, "asr_gru_bwd_state")
    return dgi, dgh, dhx


LAST_SYNC = [None]


def gru_check_sync():
    """(debug / tests) synchronise and raise if the last persistent GRU launch abandoned an in-launch wait"""
    s = LAST_SYNC[0]
    if s is not None and int(s[1023:1024].cpu()[0]) != 0:
        s[1023:1024].zero_()
        raise _lib.AsrHipError("persistent GRU kernel timed out waiting for another workgroup")


def gru_check_all():
    """synchronising check of EVERY control buffer of this process: the evaluation path calls it where it reads results back
    anyway (asr.error.compute_minibatch_error), because forward-only loops never reach optimizer.update's polling"""
    bad = []
    for key, buf in list(_SYNC.items()):
        if int(buf[1023:1024].cpu()[0]) != 0:
            buf[1023:1024].zero_()
            bad.append(key)
    if bad:
        raise _lib.AsrHipError("a persistent GRU kernel gave up an in-launch wait: the outputs of that forward pass are invalid")


def gru_bwd(dy, gates, hseq, whhT16, T, B, H, ndir, db_ih=None, db_hh=None, x_len=None):
    """db_ih / db_hh: (ndir * 3H) f32 buffers the bias gradients are accumulated into (optional)."""
    dev = dy.device
    x_len = _len_i32(x_len, B, dev)
    dy_ws = torch.empty((T * B, H), dtype=BF16, device=dev) if x_len is not None else None
    if gates.dtype == torch.float16 and (db_ih is None or db_hh is None):
        # half gates belong to the partial-sum backward kernel, which sums the bias gradients in registers: give it somewhere to put them
        scratch = torch.empty((2, ndir * 3 * H), dtype=F32, device=dev)
        fill_(scratch, 0.0)
        db_ih = scratch[0] if db_ih is None else db_ih
        db_hh = scratch[1] if db_hh is None else db_hh
    dgi = torch.empty((T * B, ndir * 3 * H), dtype=BF16, device=dev)
    dgh = torch.empty((T * B, ndir * 3 * H), dtype=BF16, device=dev)
    sync = _sync_buffer(dev, _lib.lib().asr_gru_sync_bytes(B, H, ndir))
    carry = torch.empty((ndir, B, H), dtype=F32, device=dev)
    _hook("before")
    rc = _lib.lib().asr_gru_bwd(stream(), ptr(dy.contiguous()), ptr(gates), ptr(hseq), ptr(whhT16), ptr(dgi), ptr(dgh),
                                ptr(carry), ptr(db_ih), ptr(db_hh), T, B, H, ndir, ptr(sync), GRU_MODE[0], ptr(x_len), ptr(dy_ws),
                                int(gates.dtype == torch.float16))
    check(rc, "asr_gru_bwd")
    _hook("after")
    LAST_SYNC[0] = sync
    return dgi, dgh


def fill_(t, value):
    assert t.dtype == F32 and t.is_contiguous()
    check(_lib.lib().asr_fill_f32(stream(), ptr(t), t.numel(), float(value)), "asr_fill_f32")
    return t


def sqnorm_acc(g, out):
    check(_lib.lib().asr_sqnorm_acc(stream(), ptr(g), g.numel(), ptr(out)), "asr_sqnorm_acc")
    return out


def clip_decay_adam(p, g, m, v, alpha, beta1, beta2, eps, weight_decay, clip, grad_scale, sqnorm, step):
    rc = _lib.lib().asr_clip_decay_adam(stream(), ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), alpha, beta1, beta2, eps,
                                        weight_decay, clip, grad_scale, ptr(sqnorm), int(step))
    check(rc, "asr_clip_decay_adam")


def abort_words():
    """the abort words of every control buffer a recurrence of this process has used (asr_hip.h: sync_ws int 1023)"""
    return [buf[1023:1024] for buf in _SYNC.values()]


_ABORT = {}         # device index -> [addresses of the abort words covered, device table of them, the ORed word]


def gather_abort(dev, poison=None):
    """ONE device word = the OR of every abort word on `dev` (any number of control buffers: a process that ran recurrences on three
    streams -- eval on the default stream, then two half-batch streams -- has three), queued on the current stream.  poison: an
    element of the local gradient buffer that gets a NaN when a word is raised (data parallelism: every rank then drops the step)."""
    words = [w for w in abort_words() if w.device == dev]
    ptrs = tuple(w.data_ptr() for w in words)           # (a control buffer that grew was replaced: same count, another address)
    st = _ABORT.get(dev.index)
    if st is None or st[0] != ptrs:
        table = torch.tensor(list(ptrs) or [0], dtype=torch.int64).to(dev)
        st = _ABORT[dev.index] = [ptrs, table, torch.zeros(1, dtype=torch.int32, device=dev) if st is None else st[2]]
    check(_lib.lib().asr_gather_abort(stream(), ptr(st[1]), len(words), ptr(st[2]), ptr(poison)), "asr_gather_abort")
    return st[2]


def clear_abort_words(dev):
    for w in abort_words():
        if w.device == dev:
            w.zero_()


def step_control(g, partials, clip, grad_scale, alpha, beta1, beta2, applied, ctl, any_abort=None, reserved_index=-1, loss_scale=None):
    """any_abort: the word gather_abort returned for this step (None: gathered here); reserved_index, loss_scale (device float[4] or
    None): see asr_hip.h"""
    if any_abort is None:
        any_abort = gather_abort(g.device)
    rc = _lib.lib().asr_step_control_scaled(stream(), ptr(g), g.numel(), ptr(partials), ptr(any_abort), None, float(clip),
                                            float(grad_scale), float(alpha), float(beta1), float(beta2), ptr(applied), ptr(ctl),
                                            int(reserved_index), None if loss_scale is None else ptr(loss_scale))
    check(rc, "asr_step_control_scaled")


def sqnorm_partials_count(n):
    return int(_lib.lib().asr_sqnorm_partials_count(int(n)))


def adam_ctl(p, g, m, v, beta1, beta2, eps, weight_decay, ctl):
    rc = _lib.lib().asr_adam_ctl(stream(), ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), beta1, beta2, eps, weight_decay, ptr(ctl))
    check(rc, "asr_adam_ctl")


def sgd_ctl(p, g, v, kind, lr, momentum, weight_decay, ctl):
    rc = _lib.lib().asr_sgd_ctl(stream(), ptr(p), ptr(g), ptr(v), p.numel(), int(kind), lr, momentum, weight_decay, ptr(ctl))
    check(rc, "asr_sgd_ctl")


SRU_CHUNKED = [True]        # (tests switch the chunked scans off to run the one-thread-per-column kernels)


def _sru_ws(T, B, D, dev):
    n = int(_lib.lib().asr_sru_ws_bytes(T, B, D)) if SRU_CHUNKED[0] else 0
    return (torch.empty(n, dtype=torch.uint8, device=dev), n) if n else (None, 0)


def sru_fwd(x, U, bias, c0, mask, use_tanh):
    """x (T, B, D) bf16, U (T*B, 3D) f32 -> H bf16, C f32, cT (B, D) f32."""
    T, B, D = x.shape
    H = torch.empty_like(x)
    C = torch.empty((T, B, D), dtype=F32, device=x.device)
    cT = torch.empty((B, D), dtype=F32, device=x.device)
    ws, n = _sru_ws(T, B, D, x.device)
    rc = _lib.lib().asr_sru_fwd(stream(), ptr(x), ptr(U), ptr(bias), ptr(c0), ptr(mask), ptr(H), ptr(C), ptr(cT), T, B, D,
                                int(bool(use_tanh)), ptr(ws), n)
    check(rc, "asr_sru_fwd")
    return H, C, cT


def sru_bwd(x, U, bias, C, c0, mask, gH, gcT, gbias, use_tanh):
    T, B, D = x.shape
    gU = torch.empty((T * B, 3 * D), dtype=BF16, device=x.device)
    gxh = torch.empty_like(x)
    gc0 = torch.empty((B, D), dtype=F32, device=x.device)
    ws, n = _sru_ws(T, B, D, x.device)
    rc = _lib.lib().asr_sru_bwd(stream(), ptr(x), ptr(U), ptr(bias), ptr(C), ptr(c0), ptr(mask), ptr(gH), ptr(gcT), ptr(gU),
                                ptr(gxh), ptr(gbias), ptr(gc0), T, B, D, int(bool(use_tanh)), ptr(ws), n)
    check(rc, "asr_sru_bwd")
    return gU, gxh, gc0


def sru_combine(a, b, mask):
    out = torch.empty_like(a)
    BD = a.shape[-2] * a.shape[-1]
    check(_lib.lib().asr_sru_combine(stream(), ptr(a), ptr(b), ptr(mask), ptr(out), a.numel(), BD), "asr_sru_combine")
    return out


def _sru_seq_ws(T, B, D, ndir, dev):
    n = int(_lib.lib().asr_sru_seq_ws_bytes(T, B, D, ndir))
    return (torch.empty(n, dtype=torch.uint8, device=dev), n) if n else (None, 0)


def sru_seq_fwd(x, U, bias, cx, x_len, T, B, D, k, ndir, use_tanh):
    """x (T, B, D) bf16 (k = 3; None for k = 4), U (T*B, ndir k D) f32, bias (ndir, 2D), cx (ndir, B, D) f32 or None, x_len (B) int32
    or None -> y (T, B, D) bf16 (directions summed), C (ndir, T, B, D) f32, cy (ndir, B, D) f32   (include/asr_hip.h)"""
    dev = U.device
    x_len = _len_i32(x_len, B, dev)
    y = torch.empty((T, B, D), dtype=BF16, device=dev)
    C = torch.empty((ndir, T, B, D), dtype=F32, device=dev)
    cy = torch.empty((ndir, B, D), dtype=F32, device=dev)
    ws, n = _sru_seq_ws(T, B, D, ndir, dev)
    rc = _lib.lib().asr_sru_seq_fwd(stream(), ptr(x), ptr(U), ptr(bias), ptr(cx), ptr(x_len), ptr(y), ptr(C), ptr(cy), T, B, D, int(k),
                                    int(ndir), int(bool(use_tanh)), ptr(ws), n)
    check(rc, "asr_sru_seq_fwd")
    return y, C, cy


def sru_seq_bwd(x, U, bias, C, cx, x_len, gy, dcy, gbias, T, B, D, k, ndir, use_tanh, need_dcx=True):
    """-> gU (T*B, ndir k D) bf16, gxh (T, B, D) bf16 (k = 3) or None, dcx (ndir, B, D) f32 or None; gbias (ndir, 2D) f32 is added to"""
    dev = U.device
    x_len = _len_i32(x_len, B, dev)
    gU = torch.empty((T * B, ndir * k * D), dtype=BF16, device=dev)
    gxh = torch.empty((T, B, D), dtype=BF16, device=dev) if k == 3 else None
    dcx = torch.empty((ndir, B, D), dtype=F32, device=dev) if need_dcx else None
    ws, n = _sru_seq_ws(T, B, D, ndir, dev)
    rc = _lib.lib().asr_sru_seq_bwd(stream(), ptr(x), ptr(U), ptr(bias), ptr(C), ptr(cx), ptr(x_len), ptr(gy), ptr(dcy), ptr(gU), ptr(gxh),
                                    ptr(gbias), ptr(dcx), T, B, D, int(k), int(ndir), int(bool(use_tanh)), ptr(ws), n)
    check(rc, "asr_sru_seq_bwd")
    return gU, gxh, dcx


def clip_decay_sgd(p, g, v, kind, lr, momentum, weight_decay, clip, grad_scale, sqnorm):
    rc = _lib.lib().asr_clip_decay_sgd(stream(), ptr(p), ptr(g), ptr(v), p.numel(), int(kind), lr, momentum, weight_decay,
                                       clip, grad_scale, ptr(sqnorm))
    check(rc, "asr_clip_decay_sgd")


def weightnorm_fwd(V, g):
    """V (Co, ...) f32, g (Co, 1, 1, 1) -> W (same shape as V) f32, norm (Co)."""
    Co = V.shape[0]
    K = V.numel() // Co
    W = torch.empty_like(V, memory_format=torch.contiguous_format)
    norm = torch.empty(Co, dtype=F32, device=V.device)
    check(_lib.lib().asr_weightnorm_fwd(stream(), ptr(V.contiguous()), ptr(g.contiguous()), ptr(W), ptr(norm), Co, K), "asr_weightnorm_fwd")
    return W, norm


def weightnorm_bwd(gW, V, g, norm, gV, gg):
    Co = V.shape[0]
    K = V.numel() // Co
    rc = _lib.lib().asr_weightnorm_bwd(stream(), ptr(gW), ptr(V.contiguous()), ptr(g.contiguous()), ptr(norm), ptr(gV), ptr(gg), Co, K)
    check(rc, "asr_weightnorm_bwd")


def channel_mean_std(x2):
    rows, C = x2.shape
    mean = torch.empty(C, dtype=F32, device=x2.device)
    std = torch.empty(C, dtype=F32, device=x2.device)
    check(_lib.lib().asr_channel_stats(stream(), ptr(x2), rows, C, ptr(mean), ptr(std)), "asr_channel_stats")
    return mean, std


def weightnorm_init(mean, std):
    g = torch.empty_like(mean)
    b = torch.empty_like(mean)
    check(_lib.lib().asr_weightnorm_init(stream(), ptr(mean), ptr(std), ptr(g), ptr(b), mean.numel()), "asr_weightnorm_init")
    return g, b


def channel_affine(x2, scale, shift):
    y = torch.empty(x2.shape, dtype=BF16, device=x2.device)
    check(_lib.lib().asr_channel_affine(stream(), ptr(x2), ptr(scale), ptr(shift), ptr(y), x2.numel(), x2.shape[1]), "asr_channel_affine")
    return y


# ------------------------------------------------------------------------------------------------ decode / CER / loader extras
I32 = torch.int32


def argmax_rows(logits):
    """(T, B, V) f32 logits -> (B, T) int32 greedy ids."""
    T, B, V = logits.shape
    ids = torch.empty((B, T), dtype=I32, device=logits.device)
    check(_lib.lib().asr_argmax_rows(stream(), ptr(logits), T, B, V, ptr(ids)), "asr_argmax_rows")
    return ids


def ctc_collapse(ids, lengths, blank, merge_repeats=True):
    """(B, T) int32 -> (compacted ids (B, T) padded with blank, lengths (B))."""
    B, T = ids.shape
    out = torch.empty_like(ids)
    out_len = torch.empty((B,), dtype=I32, device=ids.device)
    rc = _lib.lib().asr_ctc_collapse(stream(), ptr(ids), None if lengths is None else ptr(lengths), B, T, int(blank), int(merge_repeats),
                                     ptr(out), ptr(out_len))
    check(rc, "asr_ctc_collapse")
    return out, out_len


def edit_distance(ref, ref_len, hyp, hyp_len):
    """row-wise Levenshtein distance of two padded int32 id matrices -> (pairs,) int32."""
    pairs = ref.shape[0]
    dist = torch.empty((pairs,), dtype=I32, device=ref.device)
    rc = _lib.lib().asr_edit_distance(stream(), ptr(ref), ptr(ref_len), ref.shape[1], ptr(hyp), ptr(hyp_len), hyp.shape[1], pairs, ptr(dist))
    check(rc, "asr_edit_distance")
    return dist


def edit_align(ref, ref_len, hyp, hyp_len, paths=True, budget=None):
    """row-wise edit alignment of two padded int32 id matrices (asr_edit_align) -> (counts (pairs, 4) int32: distance,
    substitutions, deletions, insertions; ref_to_hyp (pairs, ref_pitch) int32; hyp_to_ref (pairs, hyp_pitch) int32), the maps None
    without `paths`.  With `paths` the back-pointer workspace of one launch stays within `budget` bytes (None: one launch): the
    pairs are split over several launches that reuse it; a single pair beyond the budget still gets its launch."""
    pairs, rp, hp = ref.shape[0], ref.shape[1], hyp.shape[1]
    dev = ref.device
    counts = torch.empty((pairs, 4), dtype=I32, device=dev)
    rmap = torch.empty((pairs, rp), dtype=I32, device=dev) if paths else None
    hmap = torch.empty((pairs, hp), dtype=I32, device=dev) if paths else None
    if pairs == 0:
        return counts, rmap, hmap
    lib = _lib.lib()
    step = pairs
    if paths and budget is not None:
        step = max(1, min(pairs, int(budget) // max(1, lib.asr_edit_align_workspace_bytes(1, rp, hp))))
    nbytes = lib.asr_edit_align_workspace_bytes(step, rp, hp) if paths else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev) if paths else None
    for s in range(0, pairs, step):
        e = min(pairs, s + step)
        rc = lib.asr_edit_align(stream(), ptr(ref[s:e]), ptr(ref_len[s:e]), rp, ptr(hyp[s:e]), ptr(hyp_len[s:e]), hp, e - s,
                                ptr(counts[s:e]), ptr(rmap[s:e]) if paths else None, ptr(hmap[s:e]) if paths else None, ptr(ws), nbytes)
        check(rc, "asr_edit_align")
    return counts, rmap, hmap


def nbest_pairwise_distance(ids, lens):
    """ids (B, N, L) int32, lens (B, N) int32 (negative: unused slot) -> (B, N, N) int32 Levenshtein distances between the slots of
    every utterance (asr_nbest_pairwise_distance): symmetric, diagonal 0, rows and columns of unused slots 0."""
    B, N, L = ids.shape
    dist = torch.empty((B, N, N), dtype=I32, device=ids.device)
    if dist.numel():
        check(_lib.lib().asr_nbest_pairwise_distance(stream(), ptr(ids), ptr(lens), B, N, L, ptr(dist)), "asr_nbest_pairwise_distance")
    return dist


def nbest_consensus(ids, lens, pivot, post, budget=None):
    """ids (B, N, L) int32, lens (B, N) int32 (negative: unused), pivot (B) int32 (-1: none), post (B, N) f32 -> conf (B, L) f32: the
    posterior mass of the slots whose token aligned to position l of the pivot equals the pivot's (asr_nbest_consensus).  The
    workspace of one launch stays within `budget` bytes (None: one launch): the utterances are split over several launches."""
    B, N, L = ids.shape
    conf = torch.empty((B, L), dtype=torch.float32, device=ids.device)
    if conf.numel() == 0 or N == 0:
        return conf.zero_()
    lib = _lib.lib()
    step = B if budget is None else max(1, min(B, int(budget) // max(1, lib.asr_nbest_consensus_workspace_bytes(1, N, L))))
    nbytes = lib.asr_nbest_consensus_workspace_bytes(step, N, L)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=ids.device)
    for s in range(0, B, step):
        e = min(B, s + step)
        rc = lib.asr_nbest_consensus(stream(), ptr(ids[s:e]), ptr(lens[s:e]), ptr(pivot[s:e]), ptr(post[s:e]), e - s, N, L,
                                     ptr(conf[s:e]), ptr(ws), nbytes)
        check(rc, "asr_nbest_consensus")
    return conf


def _min_logp(min_logp):
    """the candidate threshold as the C entries take it: None is no threshold"""
    return float("-inf") if min_logp is None else float(min_logp)


def _nbest_out(B, beam_width, L, dev, n_scores=1):
    """uninitialised outputs of a beam search: ids (B, beam_width, L) int32, lengths (B, beam_width) int32 and a tuple of
    `n_scores` (B, beam_width) f32 tensors"""
    ids = torch.empty((B, beam_width, L), dtype=I32, device=dev)
    out_len = torch.empty((B, beam_width), dtype=I32, device=dev)
    return ids, out_len, tuple(torch.empty((B, beam_width), dtype=torch.float32, device=dev) for _ in range(n_scores))


def _check_gram(gram, V, dev):
    if gram.dtype != I32 or tuple(gram.shape) != (V, 2) or gram.device != dev or not gram.is_contiguous():
        raise ValueError("gram must be a contiguous (V, 2) int32 tensor on the logits' device")


_NO_LM = (None, 0, None, None, 0, 0, 0)
_NO_GRAPH = (None, None, 0, 0, None, 0)


def _lm_args(image):
    """(uni, vlm, keys, vals, slots, max_probe, order) of a device image of asr.lm.NGramLM.to(device)"""
    return (ptr(image["uni"]), int(image["uni"].shape[0]), ptr(image["keys"]), ptr(image["vals"]), int(image["slots"]),
            int(image["max_probe"]), int(image["order"]))


def _graph_args(image):
    """(keys, vals, slots, max_probe, ret, n_states) of a device image of asr.bias.ContextGraph.to(device)"""
    return (ptr(image["keys"]), ptr(image["vals"]), int(image["slots"]), int(image["max_probe"]), ptr(image["ret"]),
            int(image["n_states"]))


def _lm_or_none(image):
    return _NO_LM if image is None else _lm_args(image)


def _graph_or_none(graph):
    return _NO_GRAPH if graph is None else _graph_args(graph)


# ---- the beam searches.  One implementation per kind of entry; the public names below it are forwards that say which C entry
# they reach.  The C arguments come in the runs that _lib names: the search's, [gram], the model's, the graph's, the buffers.
def _beam_search(kind, logits, lengths, blank, beam_width, top_k, min_logp, gram=None, image=None, graph=None, alpha=0.0, beta=0.0,
                 bos=-1, eos=-1):
    """the one-shot search asr_[gram_]ctc_beam_search`kind` (Gram-CTC with `gram`): kind "" returns (ids, lengths, scores), "_lm"
    (the model `image`) adds ctc_scores and lm_scores, "_bias" (`graph`, and `image` or None) adds bias_scores as well"""
    T, B, V = logits.shape
    dev = logits.device
    if gram is not None:
        _check_gram(gram, V, dev)
    name = "asr_gram_ctc_beam" if gram is not None else "asr_ctc_beam"
    nbytes = getattr(_lib.lib(), name + kind + "_workspace_bytes")(T, B, V, int(beam_width), int(top_k))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    ids, out_len, scores = _nbest_out(B, beam_width, (2 if gram is not None else 1) * T, dev, {"": 1, "_lm": 3, "_bias": 4}[kind])
    args = [stream(), ptr(logits), ptr(lengths), T, B, V, int(blank), int(beam_width), int(top_k), _min_logp(min_logp)]
    if gram is not None:
        args.append(ptr(gram))
    if kind:
        args += _lm_args(image) if kind == "_lm" else _lm_or_none(image)
        args += [int(bos), int(eos), float(alpha), float(beta)]
    args += [ptr(ws), nbytes, ptr(ids), ptr(out_len)] + [ptr(s) for s in scores[:3]]
    if kind == "_bias":
        args += _graph_args(graph) + (ptr(scores[3]),)
    check(getattr(_lib.lib(), name + "_search" + kind)(*args), name + "_search" + kind)
    return (ids, out_len) + scores


# The three families of streaming entries: CTC's, Gram-CTC's without a graph argument, and Gram-CTC's with one.  Only CTC's
# reset takes bos (Gram-CTC's advance and result do), only CTC's result takes eos after the weights, and "gram" has no with_bias,
# no graph and no out_bias.
_STREAM = {"ctc": "asr_ctc_beam_stream_", "gram": "asr_gram_ctc_beam_stream_", "gram_bias": "asr_gram_ctc_beam_bias_stream_"}


def _stream_flags(fam, with_lm, with_bias):
    return [int(bool(with_lm))] + ([] if fam == "gram" else [int(bool(with_bias))])


def _stream_state_bytes(fam, B, beam_width, max_frames, with_lm, with_bias=False):
    return getattr(_lib.lib(), _STREAM[fam] + "state_bytes")(int(B), int(beam_width), int(max_frames),
                                                             *_stream_flags(fam, with_lm, with_bias))


def _stream_workspace_bytes(fam, Tc, B, V, beam_width, top_k):
    name = _STREAM["ctc" if fam == "ctc" else "gram"] + "workspace_bytes"           # one size with or without a graph
    return getattr(_lib.lib(), name)(int(Tc), int(B), int(V), int(beam_width), int(top_k))


def _stream_reset(fam, state, B, beam_width, max_frames, with_lm, with_bias, bos, mask):
    name = _STREAM[fam] + "reset"
    rc = getattr(_lib.lib(), name)(stream(), ptr(state), state.numel(), int(B), int(beam_width), int(max_frames),
                                   *_stream_flags(fam, with_lm, with_bias), *([int(bos)] if fam == "ctc" else []), ptr(mask))
    check(rc, name)


def _stream_advance(fam, state, logits, lengths, blank, beam_width, top_k, gram, frames_before, max_frames, image, graph, alpha, beta,
                    bos, min_logp):
    Tc, B, V = logits.shape
    if fam != "ctc":
        _check_gram(gram, V, logits.device)
    nbytes = _stream_workspace_bytes(fam, Tc, B, V, beam_width, top_k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=logits.device)
    args = [stream(), ptr(logits), ptr(lengths), Tc, B, V, int(blank), int(beam_width), int(top_k), _min_logp(min_logp)]
    if fam != "ctc":
        args.append(ptr(gram))
    args += _lm_or_none(image)
    if fam != "ctc":
        args.append(int(bos))
    if fam != "gram":
        args += _graph_or_none(graph)
    args += [float(alpha), float(beta), int(frames_before), int(max_frames), ptr(state), state.numel(), ptr(ws), nbytes]
    check(getattr(_lib.lib(), _STREAM[fam] + "advance")(*args), _STREAM[fam] + "advance")


def _stream_result(fam, state, B, beam_width, max_frames, blank, Lcap, image, graph, alpha, beta, bos, eos):
    dev = state.device
    n = 1 if image is None and graph is None else (3 if graph is None else 4)
    ids, out_len, scores = _nbest_out(B, beam_width, Lcap, dev, n)
    frames = torch.empty((B,), dtype=I32, device=dev)
    extra = [ptr(s) for s in scores[1:]] + [None] * ((3 if fam == "gram" else 4) - n)
    args = [stream(), *_lm_or_none(image)]
    if fam != "ctc":
        args += [int(bos), int(eos)]
    if fam != "gram":
        args += _graph_or_none(graph)
    args += [float(alpha), float(beta)]
    if fam == "ctc":
        args.append(int(eos))
    args += [int(B), int(beam_width), int(max_frames), int(blank), int(Lcap), ptr(state), state.numel(), ptr(ids), ptr(out_len),
             ptr(scores[0]), *extra, ptr(frames)]
    check(getattr(_lib.lib(), _STREAM[fam] + "result")(*args), _STREAM[fam] + "result")
    return (ids, out_len) + scores, frames


def ctc_beam_search(logits, lengths, blank, beam_width, top_k, min_logp=None):
    """(T, B, V) f32 logits -> (ids (B, beam_width, T) int32 padded with blank, lengths (B, beam_width) int32,
    scores (B, beam_width) f32): the N-best of the CTC prefix beam search, best first; unused slots have length 0 and
    score -inf.  `lengths` (B) int32 or None (all T frames); min_logp None: no candidate threshold."""
    return _beam_search("", logits, lengths, blank, beam_width, top_k, min_logp)


def gram_ctc_beam_search(logits, lengths, blank, beam_width, top_k, gram, min_logp=None):
    """(T, B, V) f32 logits, gram (V, 2) int32 on the same device -> (ids (B, beam_width, 2T) int32 unigram ids padded with blank,
    lengths (B, beam_width) int32, scores (B, beam_width) f32): the N-best strings of the Gram-CTC beam search
    (asr_gram_ctc_beam_search), best first; unused slots have length 0 and score -inf.  The table is not checked here
    (asr.error.gram_beam_decode does)."""
    return _beam_search("", logits, lengths, blank, beam_width, top_k, min_logp, gram)


def ngram_score(image, ids, lengths=None, bos=-1, eos=-1):
    """ids (N, Lmax) int32, lengths (N) int32 or None -> (tok (N, Lmax) f32: log P(token | context) of every token, 0 past the
    length; total (N) f32: their sum plus the eos term) of asr_ngram_score over the device image of an asr.lm.NGramLM"""
    N, Lmax = ids.shape
    dev = ids.device
    tok = torch.empty((N, Lmax), dtype=torch.float32, device=dev)
    total = torch.empty((N,), dtype=torch.float32, device=dev)
    if N == 0 or Lmax == 0:
        raise ValueError("ngram_score needs at least one sequence and one column")
    rc = _lib.lib().asr_ngram_score(stream(), *_lm_args(image), ptr(ids), ptr(lengths), N, Lmax, int(bos), int(eos), ptr(tok),
                                    ptr(total))
    check(rc, "asr_ngram_score")
    return tok, total


def ctc_beam_search_lm(logits, lengths, blank, beam_width, top_k, image, alpha, beta, bos=-1, eos=-1, min_logp=None):
    """ctc_beam_search ranked by ctc + alpha * lm + beta * len (asr_ctc_beam_search_lm) -> (ids, lengths, scores, ctc_scores,
    lm_scores); `image`: the device image of an asr.lm.NGramLM"""
    return _beam_search("_lm", logits, lengths, blank, beam_width, top_k, min_logp, None, image, None, alpha, beta, bos, eos)


def ctx_score(image, V, ids, lengths=None, finalize=True):
    """ids (N, Lmax) int32, lengths (N) int32 or None -> (tok (N, Lmax) f32: the bonus step of every token, 0 past the length;
    total (N) f32: their sum, plus ret[state] with `finalize`) of asr_ctx_score over the device image of an
    asr.bias.ContextGraph"""
    N, Lmax = ids.shape
    dev = ids.device
    if N == 0 or Lmax == 0:
        raise ValueError("ctx_score needs at least one sequence and one column")
    tok = torch.empty((N, Lmax), dtype=torch.float32, device=dev)
    total = torch.empty((N,), dtype=torch.float32, device=dev)
    rc = _lib.lib().asr_ctx_score(stream(), *_graph_args(image), int(V), ptr(ids), ptr(lengths), N, Lmax, int(bool(finalize)),
                                  ptr(tok), ptr(total))
    check(rc, "asr_ctx_score")
    return tok, total


def ctc_beam_search_bias(logits, lengths, blank, beam_width, top_k, graph, image=None, alpha=0.0, beta=0.0, bos=-1, eos=-1,
                         min_logp=None):
    """ctc_beam_search (image None) or ctc_beam_search_lm ranked with the phrase bonus of `graph` on top
    (asr_ctc_beam_search_bias) -> (ids, lengths, scores, ctc_scores, lm_scores, bias_scores); `graph`: the device image of an
    asr.bias.ContextGraph, `image`: that of an asr.lm.NGramLM"""
    return _beam_search("_bias", logits, lengths, blank, beam_width, top_k, min_logp, None, image, graph, alpha, beta, bos, eos)


def ctc_beam_stream_state_bytes(B, beam_width, max_frames, with_lm, with_bias):
    """bytes of the device-resident state of a streaming beam search (asr_ctc_beam_stream_state_bytes; host only)"""
    return _stream_state_bytes("ctc", B, beam_width, max_frames, with_lm, with_bias)


def ctc_beam_stream_workspace_bytes(Tc, B, V, beam_width, top_k):
    """bytes of the per-call scratch of ctc_beam_stream_advance for a chunk of Tc frames (host only)"""
    return _stream_workspace_bytes("ctc", Tc, B, V, beam_width, top_k)


def ctc_beam_stream_reset(state, B, beam_width, max_frames, with_lm, with_bias, bos=-1, mask=None):
    """the root beam into `state` (uint8, ctc_beam_stream_state_bytes) for every utterance, or for those with mask[b] != 0
    (mask (B) int32 on the device): asr_ctc_beam_stream_reset"""
    _stream_reset("ctc", state, B, beam_width, max_frames, with_lm, with_bias, bos, mask)


def ctc_beam_stream_advance(state, logits, lengths, blank, beam_width, top_k, frames_before, max_frames, image=None, graph=None,
                            alpha=0.0, beta=0.0, min_logp=None):
    """one chunk (Tc, B, V) f32 of logits into the beam kept in `state` (asr_ctc_beam_stream_advance); `lengths` (B) int32: the valid
    frames of this chunk per utterance, or None; `image` / `graph`: the device images of an asr.lm.NGramLM / asr.bias.ContextGraph"""
    _stream_advance("ctc", state, logits, lengths, blank, beam_width, top_k, None, frames_before, max_frames, image, graph, alpha,
                    beta, -1, min_logp)


def ctc_beam_stream_result(state, B, beam_width, max_frames, blank, Lcap, image=None, graph=None, alpha=0.0, beta=0.0, eos=-1):
    """the N-best of the beam kept in `state`, which stays as it is (asr_ctc_beam_stream_result) -> ((ids (B, beam_width, Lcap),
    lengths, scores[, ctc_scores, lm_scores[, bias_scores]]) as the one-shot search of the same variant returns them,
    frames (B) int32: the frames every utterance has consumed)"""
    return _stream_result("ctc", state, B, beam_width, max_frames, blank, Lcap, image, graph, alpha, beta, -1, eos)


def gram_ctc_beam_search_lm(logits, lengths, blank, beam_width, top_k, gram, image, alpha, beta, bos=-1, eos=-1, min_logp=None):
    """gram_ctc_beam_search ranked by ctc + alpha * lm + beta * len over the spelled characters (asr_gram_ctc_beam_search_lm) ->
    (ids (B, beam_width, 2T), lengths, scores, ctc_scores, lm_scores); `image`: the device image of an asr.lm.NGramLM over the
    unigram ids of `gram`.  The table is not checked here (asr.error.gram_beam_decode_lm does)."""
    return _beam_search("_lm", logits, lengths, blank, beam_width, top_k, min_logp, gram, image, None, alpha, beta, bos, eos)


def gram_ctc_beam_stream_state_bytes(B, beam_width, max_frames, with_lm):
    """bytes of the device-resident state of a streaming Gram-CTC beam search (asr_gram_ctc_beam_stream_state_bytes; host only)"""
    return _stream_state_bytes("gram", B, beam_width, max_frames, with_lm)


def gram_ctc_beam_stream_workspace_bytes(Tc, B, V, beam_width, top_k):
    """bytes of the per-call scratch of gram_ctc_beam_stream_advance for a chunk of Tc frames (host only)"""
    return _stream_workspace_bytes("gram", Tc, B, V, beam_width, top_k)


def gram_ctc_beam_stream_reset(state, B, beam_width, max_frames, with_lm, mask=None):
    """the root beam into `state` (uint8, gram_ctc_beam_stream_state_bytes) for every utterance, or for those with mask[b] != 0
    (mask (B) int32 on the device): asr_gram_ctc_beam_stream_reset"""
    _stream_reset("gram", state, B, beam_width, max_frames, with_lm, False, -1, mask)


def gram_ctc_beam_stream_advance(state, logits, lengths, blank, beam_width, top_k, gram, frames_before, max_frames, image=None,
                                 alpha=0.0, beta=0.0, bos=-1, min_logp=None):
    """one chunk (Tc, B, V) f32 of logits into the beam of strings kept in `state` (asr_gram_ctc_beam_stream_advance); gram (V, 2)
    int32 on the same device (not checked here); `lengths` (B) int32: the valid frames of this chunk per utterance, or None;
    `image`: the device image of an asr.lm.NGramLM over the unigram ids of `gram`"""
    _stream_advance("gram", state, logits, lengths, blank, beam_width, top_k, gram, frames_before, max_frames, image, None, alpha,
                    beta, bos, min_logp)


def gram_ctc_beam_stream_result(state, B, beam_width, max_frames, blank, Lcap, image=None, alpha=0.0, beta=0.0, bos=-1, eos=-1):
    """the N-best strings of the beam kept in `state`, which stays as it is (asr_gram_ctc_beam_stream_result) -> ((ids (B, beam_width,
    Lcap), lengths, scores[, ctc_scores, lm_scores]) as the one-shot search of the same variant returns them, frames (B) int32:
    the frames every utterance has consumed)"""
    return _stream_result("gram", state, B, beam_width, max_frames, blank, Lcap, image, None, alpha, beta, bos, eos)


def gram_ctc_beam_search_bias(logits, lengths, blank, beam_width, top_k, gram, graph, image=None, alpha=0.0, beta=0.0, bos=-1, eos=-1,
                              min_logp=None):
    """gram_ctc_beam_search (image None) or gram_ctc_beam_search_lm ranked with the phrase bonus of `graph` on top
    (asr_gram_ctc_beam_search_bias) -> (ids (B, beam_width, 2T), lengths, scores, ctc_scores, lm_scores, bias_scores); `graph`: the
    device image of an asr.bias.ContextGraph over the unigram ids of `gram`, `image`: that of an asr.lm.NGramLM over them.  The
    table is not checked here (asr.error.gram_beam_decode_biased does)."""
    _check_gram(gram, logits.shape[2], logits.device)
    ptr(logits)                                   # a CPU tensor is refused here, before anything asks for the device's stream
    return _beam_search("_bias", logits, lengths, blank, beam_width, top_k, min_logp, gram, image, graph, alpha, beta, bos, eos)


def gram_ctc_beam_bias_stream_state_bytes(B, beam_width, max_frames, with_lm, with_bias):
    """bytes of the device-resident state of a streaming Gram-CTC beam search with or without a graph
    (asr_gram_ctc_beam_bias_stream_state_bytes; host only); without one, gram_ctc_beam_stream_state_bytes"""
    return _stream_state_bytes("gram_bias", B, beam_width, max_frames, with_lm, with_bias)


def gram_ctc_beam_bias_stream_reset(state, B, beam_width, max_frames, with_lm, with_bias, mask=None):
    """gram_ctc_beam_stream_reset for a state of gram_ctc_beam_bias_stream_state_bytes: asr_gram_ctc_beam_bias_stream_reset"""
    _stream_reset("gram_bias", state, B, beam_width, max_frames, with_lm, with_bias, -1, mask)


def gram_ctc_beam_bias_stream_advance(state, logits, lengths, blank, beam_width, top_k, gram, frames_before, max_frames, image=None,
                                      graph=None, alpha=0.0, beta=0.0, bos=-1, min_logp=None):
    """gram_ctc_beam_stream_advance with `graph`, the device image of an asr.bias.ContextGraph over the unigram ids of `gram`, or
    None (asr_gram_ctc_beam_bias_stream_advance)"""
    _stream_advance("gram_bias", state, logits, lengths, blank, beam_width, top_k, gram, frames_before, max_frames, image, graph,
                    alpha, beta, bos, min_logp)


def gram_ctc_beam_bias_stream_result(state, B, beam_width, max_frames, blank, Lcap, image=None, graph=None, alpha=0.0, beta=0.0,
                                     bos=-1, eos=-1):
    """gram_ctc_beam_stream_result with `graph` (asr_gram_ctc_beam_bias_stream_result) -> ((ids (B, beam_width, Lcap), lengths,
    scores[, ctc_scores, lm_scores[, bias_scores]]) as the one-shot search of the same variant returns them, frames (B) int32)"""
    return _stream_result("gram_bias", state, B, beam_width, max_frames, blank, Lcap, image, graph, alpha, beta, bos, eos)


def beam_stream_commit_workspace_bytes(B, beam_width, max_frames, per_frame):
    """bytes of the per-call scratch of beam_stream_commit (asr_beam_stream_commit_workspace_bytes; host only)"""
    return _lib.lib().asr_beam_stream_commit_workspace_bytes(int(B), int(beam_width), int(max_frames), int(per_frame))


def beam_stream_commit(state, gram, B, beam_width, max_frames, with_lm, with_bias, prefix=None, prefix_len=None, compact=True,
                       max_rows=None, out_pitch=1):
    """commit a prefix of the beam kept in `state` and compact its prefix table (asr_ctc_beam_stream_commit, or with `gram`
    asr_gram_ctc_beam_stream_commit on a state of gram_ctc_beam_bias_stream_state_bytes); `prefix` (B, n) int32 with `prefix_len`
    (B) int32, or None for the longest common prefix; `max_rows`: None for max_frames -> (tokens (B, out_pitch) int32 zero-padded,
    counts, committed, rows, status (B) int32)"""
    dev = state.device
    per_frame = 2 if gram else 1
    nbytes = _lib.lib().asr_beam_stream_commit_workspace_bytes(int(B), int(beam_width), int(max_frames), per_frame)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    out_pitch = max(int(out_pitch), 1)
    tokens = torch.zeros((B, out_pitch), dtype=I32, device=dev)
    counts, committed, rows, status = (torch.empty((B,), dtype=I32, device=dev) for _ in range(4))
    name = "asr_gram_ctc_beam_stream_commit" if gram else "asr_ctc_beam_stream_commit"
    rc = getattr(_lib.lib(), name)(stream(), ptr(state), state.numel(), int(B), int(beam_width), int(max_frames), int(bool(with_lm)),
                                   int(bool(with_bias)), ptr(prefix), 0 if prefix is None else prefix.shape[1], ptr(prefix_len),
                                   int(bool(compact)), int(max_frames if max_rows is None else max_rows), ptr(ws), nbytes,
                                   ptr(tokens), out_pitch, ptr(counts), ptr(committed), ptr(rows), ptr(status))
    check(rc, name)
    return tokens, counts, committed, rows, status


def ctc_align(xs, label_unigram, label_bigram, x_len, l_len, blank):
    """(T, B, V) f32 logits + labels (B, Lmax) int32 (label_bigram None: CTC, else Gram-CTC) -> the forced alignment
    (frame_ids (B, T), tok_ids, tok_pos, tok_start, tok_end (B, Lmax) int32, tok_logp (B, Lmax) f32, n_tok (B) int32,
    score (B) f32) of asr_ctc_align; x_len / l_len (B) int32 or None."""
    T, B, V = xs.shape
    Lmax = label_unigram.shape[1]
    dev = xs.device
    gram = label_bigram is not None
    nbytes = _lib.lib().asr_ctc_align_workspace_bytes(T, B, V, Lmax, int(gram))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    frames = torch.empty((B, T), dtype=I32, device=dev)
    tok = [torch.empty((B, Lmax), dtype=I32, device=dev) for _ in range(4)]
    tok_logp = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    n_tok = torch.empty((B,), dtype=I32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    rc = _lib.lib().asr_ctc_align(stream(), ptr(xs), ptr(label_unigram), ptr(label_bigram), ptr(x_len), ptr(l_len), T, B, V, Lmax,
                                  int(blank), ptr(frames), ptr(tok[0]), ptr(tok[1]), ptr(tok[2]), ptr(tok[3]), ptr(tok_logp),
                                  ptr(n_tok), ptr(score), ptr(ws), nbytes)
    check(rc, "asr_ctc_align")
    return frames, tok[0], tok[1], tok[2], tok[3], tok_logp, n_tok, score


def kws_state(B, K, Lmax, device):
    """the carried state of a keyword stream, reset for every utterance: asr_kws_state_bytes rounded UP to whole 8-byte words
    (the size is 24 B K Lmax + 4 B bytes: not a multiple of 8 for odd B), int64 so that its float64 part is aligned"""
    nbytes = _lib.lib().asr_kws_state_bytes(int(B), int(K), int(Lmax))
    state = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.int64, device=device)
    return kws_state_reset(state, B, K, Lmax, None)


def kws_state_reset(state, B, K, Lmax, mask):
    """asr_kws_state_reset: mask (B) int32 or None (all utterances)"""
    check(_lib.lib().asr_kws_state_reset(stream(), ptr(state), int(B), int(K), int(Lmax), ptr(mask)), "asr_kws_state_reset")
    return state


def kws_detect(logits, lengths, blank, image, state=None):
    """(T, B, V) f32 logits + the keyword image of asr/spot.py (uniq (U), node_tok (K, Lmax), kw_len (K) int32 on the device) ->
    det (B, K, T) f32, det_start (B, K, T) int32, fill (B, T) f32 of asr_kws_detect; lengths (B) int32 or None; state: None (one
    shot) or the tensor of kws_state"""
    T, B, V = logits.shape
    uniq, node_tok, kw_len = image["uniq"], image["node_tok"], image["kw_len"]
    K, Lmax = node_tok.shape
    U = uniq.numel()
    dev = logits.device
    nbytes = _lib.lib().asr_kws_workspace_bytes(T, B, U)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    det = torch.empty((B, K, T), dtype=F32, device=dev)
    det_start = torch.empty((B, K, T), dtype=I32, device=dev)
    fill = torch.empty((B, T), dtype=F32, device=dev)
    rc = _lib.lib().asr_kws_detect(stream(), ptr(logits), ptr(lengths), T, B, V, int(blank), ptr(uniq), U, ptr(node_tok), ptr(kw_len),
                                   K, Lmax, ptr(state), ptr(det), ptr(det_start), ptr(fill), ptr(ws), nbytes)
    check(rc, "asr_kws_detect")
    return det, det_start, fill


def gram_kws_state(B, K, Lmax, device):
    """kws_state for the Gram-CTC search: asr_gram_kws_state_bytes (36 B K Lmax + 4 B bytes: three nodes per position) rounded UP
    to whole 8-byte words"""
    nbytes = _lib.lib().asr_gram_kws_state_bytes(int(B), int(K), int(Lmax))
    state = torch.empty((max(nbytes, 8) + 7) // 8, dtype=torch.int64, device=device)
    return gram_kws_state_reset(state, B, K, Lmax, None)


def gram_kws_state_reset(state, B, K, Lmax, mask):
    """asr_gram_kws_state_reset: mask (B) int32 or None (all utterances)"""
    check(_lib.lib().asr_gram_kws_state_reset(stream(), ptr(state), int(B), int(K), int(Lmax), ptr(mask)),
          "asr_gram_kws_state_reset")
    return state


def gram_kws_detect(logits, lengths, blank, image, state=None):
    """kws_detect for a GramKeywordSet image (uniq (U), node_uni, node_big (K, Lmax), kw_len (K) int32 on the device) -> det,
    det_start, fill of asr_gram_kws_detect; state: None (one shot) or the tensor of gram_kws_state"""
    T, B, V = logits.shape
    uniq, node_uni, node_big, kw_len = image["uniq"], image["node_uni"], image["node_big"], image["kw_len"]
    K, Lmax = node_uni.shape
    U = uniq.numel()
    dev = logits.device
    nbytes = _lib.lib().asr_kws_workspace_bytes(T, B, U)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    det = torch.empty((B, K, T), dtype=F32, device=dev)
    det_start = torch.empty((B, K, T), dtype=I32, device=dev)
    fill = torch.empty((B, T), dtype=F32, device=dev)
    rc = _lib.lib().asr_gram_kws_detect(stream(), ptr(logits), ptr(lengths), T, B, V, int(blank), ptr(uniq), U, ptr(node_uni),
                                        ptr(node_big), ptr(kw_len), K, Lmax, ptr(state), ptr(det), ptr(det_start), ptr(fill),
                                        ptr(ws), nbytes)
    check(rc, "asr_gram_kws_detect")
    return det, det_start, fill


def kws_hits(det, det_start, fill, lengths, max_hits, min_score):
    """asr_kws_hits on the outputs of kws_detect -> hit_start, hit_end (B, K, max_hits) int32, hit_score, hit_logp (B, K, max_hits)
    f32, n_hits (B, K) int32"""
    B, K, T = det.shape
    dev = det.device
    H = int(max_hits)
    hs, he = (torch.empty((B, K, H), dtype=I32, device=dev) for _ in range(2))
    sc, lp = (torch.empty((B, K, H), dtype=F32, device=dev) for _ in range(2))
    n = torch.empty((B, K), dtype=I32, device=dev)
    rc = _lib.lib().asr_kws_hits(stream(), ptr(det), ptr(det_start), ptr(fill), ptr(lengths), B, K, T, H, float(min_score), ptr(hs),
                                 ptr(he), ptr(sc), ptr(lp), ptr(n))
    check(rc, "asr_kws_hits")
    return hs, he, sc, lp, n


def cmn_pspec(pspec, nframes):
    B, Fmax, nbins = pspec.shape
    check(_lib.lib().asr_cmn_pspec(stream(), ptr(pspec), ptr(nframes), B, Fmax, nbins), "asr_cmn_pspec")
    return pspec


def add_white_noise(signals, lengths, gain, seed):
    B, pitch = signals.shape
    check(_lib.lib().asr_add_white_noise(stream(), ptr(signals), ptr(lengths), pitch, B, ptr(gain), int(seed) & (2 ** 64 - 1)),
          "asr_add_white_noise")
    return signals


def running_stats_update(x, lengths, total_before, mean, nvar, mean32, std32):
    B, T = x.shape[0], x.shape[-1]
    CM = x.numel() // (B * T)
    rc = _lib.lib().asr_running_stats_update(stream(), ptr(x), ptr(lengths), B, CM, T, int(total_before), ptr(mean), ptr(nvar),
                                             ptr(mean32), ptr(std32))
    check(rc, "asr_running_stats_update")


def normalize_bcmt(x, mean32, std32):
    B, T = x.shape[0], x.shape[-1]
    CM = x.numel() // (B * T)
    check(_lib.lib().asr_normalize_bcmt(stream(), ptr(x), ptr(mean32), ptr(std32), B, CM, T), "asr_normalize_bcmt")
    return x


def augment_specgram(pspec, nframes_out, speed, ratio, Fmax_out):
    """(B, Fin, nbins) f32 power spectra -> (B, Fmax_out, nbins): asr/fft.py:21-50 with given float64 factors per utterance."""
    B, Fin, nbins = pspec.shape
    out = torch.empty((B, Fmax_out, nbins), dtype=F32, device=pspec.device)
    rc = _lib.lib().asr_augment_specgram(stream(), ptr(pspec), ptr(nframes_out), ptr(speed), ptr(ratio), B, Fin, Fmax_out, nbins, ptr(out))
    check(rc, "asr_augment_specgram")
    return out


def batchnorm_stats(x2, eps, decay, avg_mean=None, avg_var=None):
    """x2 (R, C) bf16 -> (mean, rstd) f32 (C); running averages updated in place when given."""
    R, C = x2.shape
    ws = torch.empty(2 * C, dtype=torch.float64, device=x2.device)
    mean = torch.empty(C, dtype=F32, device=x2.device)
    rstd = torch.empty(C, dtype=F32, device=x2.device)
    rc = _lib.lib().asr_batchnorm_stats(stream(), ptr(x2), R, C, float(eps), float(decay), ptr(ws), ptr(mean), ptr(rstd),
                                        ptr(avg_mean), ptr(avg_var))
    check(rc, "asr_batchnorm_stats")
    return mean, rstd


def rsqrt_eps(var, eps):
    out = torch.empty_like(var)
    check(_lib.lib().asr_rsqrt_eps(stream(), ptr(var), float(eps), ptr(out), var.numel()), "asr_rsqrt_eps")
    return out


def batchnorm_fwd(x2, mean, rstd, gamma, beta):
    R, C = x2.shape
    y = torch.empty_like(x2)
    check(_lib.lib().asr_batchnorm_fwd(stream(), ptr(x2), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), R, C, ptr(y)), "asr_batchnorm_fwd")
    return y


def batchnorm_bwd(x2, gy, mean, rstd, gamma, dgamma, dbeta, need_dx=True):
    R, C = x2.shape
    ws = torch.empty(2 * C, dtype=torch.float64, device=x2.device)
    dx = torch.empty_like(x2) if need_dx else None
    rc = _lib.lib().asr_batchnorm_bwd(stream(), ptr(x2), ptr(gy), ptr(mean), ptr(rstd), ptr(gamma), R, C, ptr(ws), ptr(dx), ptr(dgamma),
                                      ptr(dbeta))
    check(rc, "asr_batchnorm_bwd")
    return dx


def conv_implicit_ok(Cs, KH, KW):
    """the implicit-GEMM convolution wants whole 16-B chunks per tap and whole 32-wide K tiles"""
    return Cs % 8 == 0 and (KH * KW * Cs) % 32 == 0


def conv_nt(x, W2, bias, out_dtype, KH, KW, pad_h, pad_t, sgn, Tr, Hr):
    """x (Ts, B, Hs, Cs) bf16 contiguous; W2 (N, KH*KW*Cs) bf16 -> (Tr*B*Hr, N): asr_hip.h asr_conv_nt."""
    Ts, B, Hs, Cs = x.shape
    N = W2.shape[0]
    assert x.dtype == BF16 and x.is_contiguous() and W2.dtype == BF16 and W2.is_contiguous() and W2.shape[1] >= KH * KW * Cs
    out = torch.empty((Tr * B * Hr, N), dtype=out_dtype, device=x.device)
    rc = _lib.lib().asr_conv_nt(stream(), ptr(x), ptr(W2), W2.shape[1], ptr(out), _is_bf16(out), ptr(bias), Ts, B, Hs, Cs, KH, KW,
                                pad_h, pad_t, int(sgn), Tr, Hr, N)
    check(rc, "asr_conv_nt")
    return out


def conv_nt_8ph(x, W2, bias, out_dtype, KH, KW, pad_h, pad_t, sgn, Tr, Hr):
    """conv_nt on the eight-wave implicit-GEMM kernel only (csrc/gemm8.hip; Cs % 64 == 0): tests / tools, asr_conv_nt dispatches by itself"""
    Ts, B, Hs, Cs = x.shape
    N = W2.shape[0]
    out = torch.empty((Tr * B * Hr, N), dtype=out_dtype, device=x.device)
    rc = _lib.lib().asr_conv_nt_8ph(stream(), ptr(x), ptr(W2), W2.shape[1], ptr(out), _is_bf16(out), ptr(bias), Ts, B, Hs, Cs, KH, KW,
                                    pad_h, pad_t, int(sgn), Tr, Hr, N)
    check(rc, "asr_conv_nt_8ph")
    return out


def conv_nt_8pn(x, W2, bias, out_dtype, KH, KW, pad_h, pad_t, sgn, Tr, Hr):
    """conv_nt on the narrow eight-wave kernel only (N <= 128; csrc/gemm8.hip): tests / tools"""
    Ts, B, Hs, Cs = x.shape
    N = W2.shape[0]
    out = torch.empty((Tr * B * Hr, N), dtype=out_dtype, device=x.device)
    rc = _lib.lib().asr_conv_nt_8pn(stream(), ptr(x), ptr(W2), W2.shape[1], ptr(out), _is_bf16(out), ptr(bias), Ts, B, Hs, Cs, KH, KW,
                                    pad_h, pad_t, int(sgn), Tr, Hr, N)
    check(rc, "asr_conv_nt_8pn")
    return out


def conv_direct_nt(x, W2, bias, KH, KW, pad_h, pad_t, sgn, Tr, Hr):
    """conv_nt through the LDS-resident kernel (csrc/conv_direct.hip), bf16 out; raises where asr_conv_direct_ok says no (tests / tools:
    asr_conv_nt dispatches by itself)"""
    Ts, B, Hs, Cs = x.shape
    N = W2.shape[0]
    out = torch.empty((Tr * B * Hr, N), dtype=BF16, device=x.device)
    rc = _lib.lib().asr_conv_direct_nt(stream(), ptr(x), ptr(W2), W2.shape[1], ptr(out), ptr(bias), Ts, B, Hs, Cs, KH, KW, pad_h, pad_t,
                                       int(sgn), Tr, Hr, N)
    check(rc, "asr_conv_direct_nt")
    return out


def conv_mp_ok(Ci, KH, KW, Co, k):
    return bool(_lib.lib().asr_conv_mp_ok(int(Ci), int(KH), int(KW), int(Co), int(k)))


def conv_mp_fwd(x8, W2, bias, KH, KW, pad_h, pad_t, Tout, Hout, k):
    """first block in one pass (csrc/conv_first.hip): x8 (Ts, B, Hs, 8) bf16, W2 (Co, 128) bf16 -> pooled maxout of the convolution
    (Tout, B, Hp, Co / 2) bf16 and the winners' indices (same shape, uint8)"""
    Ts, B, Hs, Cs = x8.shape
    Co = W2.shape[0]
    assert Cs == 8 and x8.dtype == BF16 and x8.is_contiguous() and W2.dtype == BF16 and W2.is_contiguous() and W2.shape[1] == 128
    Hp = pooled_height(Hout, k)
    y = torch.empty((Tout, B, Hp, Co // 2), dtype=BF16, device=x8.device)
    idx = torch.empty((Tout, B, Hp, Co // 2), dtype=torch.uint8, device=x8.device)
    CALLS["conv_mp_fwd"] = CALLS.get("conv_mp_fwd", 0) + 1
    rc = _lib.lib().asr_conv_mp_fwd(stream(), ptr(x8), ptr(W2), 128, ptr(bias), ptr(y), ptr(idx), Ts, B, Hs, KH, KW, pad_h, pad_t, Tout,
                                    Hout, Co, k)
    check(rc, "asr_conv_mp_fwd")
    return y, idx


def conv_mp_bwd(gy, idx, x8, gW, gb, KH, KW, pad_h, pad_t, Hout, k):
    """gW (Co, Ci, KH, KW) f32 += weight gradient, gb (Co) f32 += bias gradient (None: none) of conv_mp_fwd"""
    Ts, B, Hs, _ = x8.shape
    Tout, _, Hp, Cp = gy.shape
    Co, Ci = gW.shape[0], gW.shape[1]
    assert gy.dtype == BF16 and gy.is_contiguous() and idx.shape == gy.shape and idx.dtype == torch.uint8 and idx.is_contiguous()
    assert gW.dtype == F32 and gW.is_contiguous() and Co == 2 * Cp and Hp == pooled_height(Hout, k)
    assert gb is None or (gb.dtype == F32 and gb.is_contiguous() and gb.numel() == Co)
    nbytes = _lib.lib().asr_conv_mp_bwd_workspace(Tout, B, Hout, Co, k)
    ws = torch.empty((nbytes // 4,), dtype=F32, device=gy.device)
    rc = _lib.lib().asr_conv_mp_bwd(stream(), ptr(gy), ptr(idx), ptr(x8), ptr(ws), ptr(gW), ptr(gb), Ts, B, Hs, Ci, KH, KW, pad_h, pad_t,
                                    Tout, Hout, Co, k)
    check(rc, "asr_conv_mp_bwd")


def conv_weight_pack_bwd(W):
    """(Co, Ci, kh, kw) f32 -> bf16 (Ci, kh*kw*Co), k = (kh, kw, co)."""
    Co, Ci, KH, KW = W.shape
    dst = torch.empty((Ci, KH * KW * Co), dtype=BF16, device=W.device)
    check(_lib.lib().asr_conv_weight_pack_bwd(stream(), ptr(W), ptr(dst), Co, Ci, KH, KW), "asr_conv_weight_pack_bwd")
    return dst


def pack_input_pad(x, strides_tbhc, T, B, H, C, Cpad):
    """any strided (T, B, H, C) view of x -> dense (T, B, H, Cpad) bf16 with zero channels behind C."""
    out = torch.empty((T, B, H, Cpad), dtype=BF16, device=x.device)
    rc = _lib.lib().asr_pack_input_pad(stream(), x.data_ptr(), _is_bf16(x), *strides_tbhc, T, B, H, C, Cpad, ptr(out))
    check(rc, "asr_pack_input_pad")
    return out


# ------------------------------------------------------------------------------------------------ the rest of asr.nn's function layers
def crelu_fwd(x):
    """x (..., C) bf16 contiguous -> (..., 2C): [relu(x) | relu(-x)] along the channels"""
    assert x.dtype == BF16 and x.is_contiguous()
    C = x.shape[-1]
    y = torch.empty(x.shape[:-1] + (2 * C,), dtype=BF16, device=x.device)
    check(_lib.lib().asr_crelu_fwd(stream(), ptr(x), ptr(y), x.numel() // C, C), "asr_crelu_fwd")
    return y


def crelu_bwd(x, dy):
    C = x.shape[-1]
    dx = torch.empty_like(x)
    check(_lib.lib().asr_crelu_bwd(stream(), ptr(x), ptr(dy.contiguous()), ptr(dx), x.numel() // C, C), "asr_crelu_bwd")
    return dx


def softmax_fwd(x, log_form):
    assert x.dtype == BF16 and x.is_contiguous()
    C = x.shape[-1]
    y = torch.empty_like(x)
    check(_lib.lib().asr_softmax_fwd(stream(), ptr(x), ptr(y), x.numel() // C, C, int(bool(log_form))), "asr_softmax_fwd")
    return y


def softmax_bwd(y, dy, log_form):
    C = y.shape[-1]
    dx = torch.empty_like(y)
    check(_lib.lib().asr_softmax_bwd(stream(), ptr(y), ptr(dy.contiguous()), ptr(dx), y.numel() // C, C, int(bool(log_form))), "asr_softmax_bwd")
    return dx


def avgpool_h_fwd(x, k):
    """x (T, B, H, C) bf16 -> (T, B, (H - k) // k + 1, C): mean over whole windows of k rows"""
    assert x.dtype == BF16 and x.is_contiguous() and x.dim() == 4
    T, B, H, C = x.shape
    y = torch.empty((T, B, (H - k) // k + 1, C), dtype=BF16, device=x.device)
    check(_lib.lib().asr_avgpool_h_fwd(stream(), ptr(x), ptr(y), T * B, H, C, k), "asr_avgpool_h_fwd")
    return y


def avgpool_h_bwd(dy, H, k):
    T, B, _, C = dy.shape
    dx = torch.empty((T, B, H, C), dtype=BF16, device=dy.device)
    check(_lib.lib().asr_avgpool_h_bwd(stream(), ptr(dy.contiguous()), ptr(dx), T * B, H, C, k), "asr_avgpool_h_bwd")
    return dx


def unpool_h_fwd(x, k, Hout):
    assert x.dtype == BF16 and x.is_contiguous() and x.dim() == 4
    T, B, H, C = x.shape
    y = torch.empty((T, B, Hout, C), dtype=BF16, device=x.device)
    check(_lib.lib().asr_unpool_h_fwd(stream(), ptr(x), ptr(y), T * B, H, Hout, C, k), "asr_unpool_h_fwd")
    return y


def unpool_h_bwd(dy, H, k):
    T, B, Hout, C = dy.shape
    dx = torch.empty((T, B, H, C), dtype=BF16, device=dy.device)
    check(_lib.lib().asr_unpool_h_bwd(stream(), ptr(dy.contiguous()), ptr(dx), T * B, H, Hout, C, k), "asr_unpool_h_bwd")
    return dx


def maxpool_h_indexes(x, k):
    """x (T, B, H, C) bf16 -> uint8 (T, B, Hout, C): row inside its window of the first maximum (what max_pooling_2d routes its gradient to)"""
    assert x.dtype == BF16 and x.is_contiguous() and x.dim() == 4
    T, B, H, C = x.shape
    idx = torch.empty((T, B, pooled_height(H, k), C), dtype=torch.uint8, device=x.device)
    check(_lib.lib().asr_maxpool_h_indexes(stream(), ptr(x), ptr(idx), T * B, H, C, k), "asr_maxpool_h_indexes")
    return idx


def upsample_h_fwd(x, idx, k, Hout):
    assert x.dtype == BF16 and x.is_contiguous() and idx.dtype == torch.uint8 and idx.is_contiguous() and idx.shape == x.shape
    T, B, H, C = x.shape
    y = torch.empty((T, B, Hout, C), dtype=BF16, device=x.device)
    check(_lib.lib().asr_upsample_h_fwd(stream(), ptr(x), ptr(idx), ptr(y), T * B, H, Hout, C, k), "asr_upsample_h_fwd")
    return y


def upsample_h_bwd(dy, idx, k):
    T, B, Hout, C = dy.shape
    H = idx.shape[2]
    dx = torch.empty((T, B, H, C), dtype=BF16, device=dy.device)
    check(_lib.lib().asr_upsample_h_bwd(stream(), ptr(dy.contiguous()), ptr(idx), ptr(dx), T * B, H, Hout, C, k), "asr_upsample_h_bwd")
    return dx


def spp_fwd(x, pyramid_height, want_pos):
    """x (T, B, H, C) bf16 -> y (B, bins, C) bf16 [, pos (B, bins, C) int32]"""
    assert x.dtype == BF16 and x.is_contiguous() and x.dim() == 4
    T, B, H, C = x.shape
    bins = _lib.lib().asr_spp_bins(int(pyramid_height))
    if bins <= 0:
        raise ValueError("pyramid_height must be in 1..8")
    y = torch.empty((B, bins, C), dtype=BF16, device=x.device)
    pos = torch.empty((B, bins, C), dtype=torch.int32, device=x.device) if want_pos else None
    check(_lib.lib().asr_spp_fwd(stream(), ptr(x), ptr(y), ptr(pos), T, B, H, C, int(pyramid_height)), "asr_spp_fwd")
    return y, pos


def spp_bwd(dy, pos, shape, pyramid_height):
    T, B, H, C = shape
    dx32 = torch.empty((T, B, H, C), dtype=F32, device=dy.device)
    fill_(dx32, 0.0)
    check(_lib.lib().asr_spp_bwd(stream(), ptr(dy.contiguous()), ptr(pos), ptr(dx32), T, B, H, C, int(pyramid_height)), "asr_spp_bwd")
    return cast_bf16(dx32.reshape(T * B * H, C)).reshape(T, B, H, C)


def gaussian_noise(x, std, seed):
    assert x.dtype == BF16
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().asr_gaussian_noise(stream(), ptr(x), ptr(y), x.numel(), float(std), int(seed) & 0xffffffff), "asr_gaussian_noise")
    return y


# ---------------------------------------------------------------------------------------------- lookahead convolution / carried rows
LOOKAHEAD_MAX_TAU = 96          # ASR_LOOKAHEAD_MAX_TAU and ASR_LOOKAHEAD_TIME_TILE of include/asr_hip.h
LOOKAHEAD_TIME_TILE = 64
STREAM_CONTEXT, STREAM_LOOKAHEAD = 0, 1


def _lookahead_args(x, w):
    if x.dtype != BF16 or x.dim() != 3 or not x.is_contiguous():
        raise ValueError("expected contiguous (T, B, D) activations, got %s %s" % (x.dtype, tuple(x.shape)))
    T, B, D = x.shape
    if w.dtype != F32 or w.dim() != 2 or w.shape[0] != D or not w.is_contiguous():
        raise ValueError("the lookahead weight must be (%d, tau + 1) float32, got %s" % (D, tuple(w.shape)))
    return T, B, D, w.shape[1] - 1


def lookahead_fwd(x, w, x_len=None, out=None):
    """x (T, B, D) activations, w (D, tau + 1) f32, x_len (B) int32 or None -> y (T, B, D): y[t] = sum_j w[:, j] x[t + j] (asr_hip.h)"""
    T, B, D, tau = _lookahead_args(x, w)
    x_len = _len_i32(x_len, B, x.device)
    y = torch.empty_like(x) if out is None else out
    assert y.dtype == BF16 and y.shape == x.shape and y.is_contiguous()
    check(_lib.lib().asr_lookahead_fwd(stream(), ptr(x), ptr(w), ptr(x_len), ptr(y), T, B, D, tau), "asr_lookahead_fwd")
    return y


def lookahead_bwd(gy, x, w, x_len=None, dW=None, need_dx=True):
    """-> dx (T, B, D) or None; dW (D, tau + 1) f32 (optional) += the weight gradient, in two ordered stages (bit-reproducible)"""
    T, B, D, tau = _lookahead_args(gy, w)
    x_len = _len_i32(x_len, B, gy.device)
    dx = torch.empty_like(gy) if need_dx else None
    ws, nbytes = None, 0
    if dW is not None:
        assert dW.dtype == F32 and dW.shape == w.shape and dW.is_contiguous() and x.shape == gy.shape and x.dtype == BF16 and x.is_contiguous()
        nbytes = _lib.lib().asr_lookahead_ws_bytes(T, B, D, tau)
        ws = torch.empty(max(nbytes, 4) // 4, dtype=F32, device=gy.device)
    check(_lib.lib().asr_lookahead_bwd(stream(), ptr(gy), ptr(x) if dW is not None else None, ptr(w), ptr(x_len), ptr(dx), ptr(dW), ptr(ws),
                                       nbytes, T, B, D, tau), "asr_lookahead_bwd")
    return dx


def stream_push(state, m, chunk, n, window, mode, flush=None):
    """asr_stream_push: state (K, B, R) activations (updated), m (B) int32 (lookahead mode; updated) or None, chunk (Tc, B, R) or None
    (a flush), n (B) int32 or None, window (K + Tc, B, R) (written) -> (wlen, emit), (B) int32 each"""
    K, B, R = state.shape
    Tc = 0 if chunk is None else chunk.shape[0]
    assert state.dtype == BF16 and window.dtype == BF16 and tuple(window.shape) == (K + Tc, B, R)
    assert chunk is None or (chunk.dtype == BF16 and tuple(chunk.shape[1:]) == (B, R))
    wlen = torch.empty((B,), dtype=torch.int32, device=state.device)
    emit = torch.empty((B,), dtype=torch.int32, device=state.device)
    check(_lib.lib().asr_stream_push(stream(), ptr(state) if K else None, ptr(m), ptr(chunk), ptr(_len_i32(n, B, state.device)),
                                     ptr(_len_i32(flush, B, state.device)), ptr(window), ptr(wlen), ptr(emit), K, Tc, B, R, int(mode)),
          "asr_stream_push")
    return wlen, emit


def stream_push_reset(state, m=None, mask=None):
    """zero the carried rows (and m) of every slot, or of those with mask[b] != 0"""
    K, B, R = state.shape
    check(_lib.lib().asr_stream_push_reset(stream(), ptr(state) if K else None, ptr(m), ptr(_len_i32(mask, B, state.device)), K, B, R),
          "asr_stream_push_reset")


# ---------------------------------------------------------------------------------------------- time reduction by frame stacking
TIME_STACK_MAX = 8              # ASR_TIME_STACK_MAX of include/asr_hip.h


def _stack_args(x, what):
    if x.element_size() != 2 or x.dim() != 3 or not x.is_contiguous():
        raise ValueError("expected contiguous 16-bit %s, got %s %s" % (what, x.dtype, tuple(x.shape)))
    return x.shape


def time_stack_fwd(x, k, x_len=None, want_len=True):
    """asr_time_stack_fwd: x (T, B, R) 16-bit, x_len (B) int32 or None -> (y (ceil(T / k), B, k * R), y_len (B) int32 or None):
    y[g, b, j * R + r] = x[g * k + j, b, r] below x_len[b], zero elsewhere; y_len = ceil(x_len / k) (None if not `want_len`)"""
    T, B, R = _stack_args(x, "(T, B, R) activations")
    k = int(k)
    y = torch.empty((-(-T // k) if k > 0 else 0, B, k * R), dtype=x.dtype, device=x.device)
    y_len = torch.empty((B,), dtype=torch.int32, device=x.device) if want_len else None
    check(_lib.lib().asr_time_stack_fwd(stream(), ptr(x), ptr(_len_i32(x_len, B, x.device)), ptr(y), ptr(y_len), T, B, R, k),
          "asr_time_stack_fwd")
    return y, y_len


def time_stack_bwd(gy, k, T, x_len=None, out=None):
    """asr_time_stack_bwd: gy (ceil(T / k), B, k * R) -> dx (T, B, R), every element written (zero at and beyond x_len[b])"""
    G, B, KR = _stack_args(gy, "(G, B, k * R) gradients")
    k, T = int(k), int(T)
    if k < 1 or KR % k != 0 or G != -(-T // k):
        raise ValueError("gy %s is not the stacked form of %d frames at k = %d" % (tuple(gy.shape), T, k))
    dx = torch.empty((T, B, KR // k), dtype=gy.dtype, device=gy.device) if out is None else out
    assert dx.dtype == gy.dtype and tuple(dx.shape) == (T, B, KR // k) and dx.is_contiguous()
    check(_lib.lib().asr_time_stack_bwd(stream(), ptr(gy), ptr(_len_i32(x_len, B, gy.device)), ptr(dx), T, B, KR // k, k),
          "asr_time_stack_bwd")
    return dx


def time_stack_push(state, m, chunk, n, y, k, flush=None):
    """asr_time_stack_push: state (k - 1, B, R) 16-bit pending rows and m (B) int32 their counts (both updated), chunk (Tc, B, R) or
    None (a flush), n (B) int32 or None, y (ceil((k - 1 + Tc) / k), B, k * R) (written: the groups of [pending | new], the trailing
    partial one zero-completed) -> emit (B) int32, the whole groups in y"""
    K, B, R = state.shape
    k = int(k)
    Tc = 0 if chunk is None else chunk.shape[0]
    assert K == k - 1 and state.element_size() == 2 and y.dtype == state.dtype and tuple(y.shape) == (-(-(K + Tc) // k), B, k * R)
    assert chunk is None or (chunk.dtype == state.dtype and tuple(chunk.shape[1:]) == (B, R))
    assert m is None or (m.dtype == torch.int32 and m.numel() == B)
    emit = torch.empty((B,), dtype=torch.int32, device=state.device)
    check(_lib.lib().asr_time_stack_push(stream(), ptr(state) if K else None, ptr(m), ptr(chunk) if Tc else None,
                                         ptr(_len_i32(n, B, state.device)), ptr(_len_i32(flush, B, state.device)),
                                         ptr(y) if y.numel() else None, ptr(emit), Tc, B, R, k), "asr_time_stack_push")
    return emit


def time_stack_push_reset(state, m=None, mask=None):
    """zero the pending rows (and m) of every slot, or of those with mask[b] != 0; state (k - 1, B, R)"""
    K, B, R = state.shape
    check(_lib.lib().asr_time_stack_push_reset(stream(), ptr(state) if K else None, ptr(m), ptr(_len_i32(mask, B, state.device)), B, R, K + 1),
          "asr_time_stack_push_reset")


# ---------------------------------------------------------------------------------------------- latency-controlled BiGRU: window copies
LC_MAX_WINDOW = 4096            # ASR_LC_MAX_WINDOW, ASR_LC_WINDOW and ASR_LC_BLOCK of include/asr_hip.h
LC_WINDOW, LC_BLOCK = 0, 1


def lc_window_shape(T, B, Nc, Nr):
    """(W, C * B): the rows of a window and the windows of a (T, B, .) sequence"""
    return min(Nc + Nr, T), -(-T // Nc) * B


def lc_gather(x, Nc, Nr, mode, x_len=None, n_win=None, want_len=True):
    """asr_lc_gather: x (T, B, R) 16-bit -> (xw (W, C * B, R): window c * B + b holds block c of slot b with its right context,
    time-reversed; w_len (C * B) int32, its live rows, or None).  mode LC_WINDOW: every live row; LC_BLOCK: only the block's own."""
    T, B, R = _stack_args(x, "(T, B, R) activations")
    Nc, Nr = int(Nc), int(Nr)
    W, CB = lc_window_shape(T, B, max(Nc, 1), max(Nr, 0))
    xw = torch.empty((W, CB, R), dtype=x.dtype, device=x.device)
    w_len = torch.empty((CB,), dtype=torch.int32, device=x.device) if want_len else None
    check(_lib.lib().asr_lc_gather(stream(), ptr(x), ptr(_len_i32(x_len, B, x.device)), ptr(_len_i32(n_win, B, x.device)), ptr(xw),
                                   ptr(w_len), T, B, R, Nc, Nr, int(mode)), "asr_lc_gather")
    return xw, w_len


def lc_scatter(yw, T, B, Nc, Nr, mode, addend=None, x_len=None, n_win=None, out=None):
    """asr_lc_scatter: yw (W, C * B, R) -> y (T, B, R) = addend + the windows' rows of every frame below x_len[b] (LC_BLOCK: the
    frame's own block; LC_WINDOW: every window that holds it), float32 sums in a fixed order; zero at and beyond x_len[b]"""
    W, CB, R = _stack_args(yw, "(W, C * B, R) windows")
    T, B, Nc, Nr = int(T), int(B), int(Nc), int(Nr)
    if (W, CB) != lc_window_shape(T, B, max(Nc, 1), max(Nr, 0)):
        raise ValueError("yw %s is not the window batch of (%d, %d, .) at Nc = %d, Nr = %d" % (tuple(yw.shape), T, B, Nc, Nr))
    y = torch.empty((T, B, R), dtype=yw.dtype, device=yw.device) if out is None else out
    assert y.dtype == yw.dtype and tuple(y.shape) == (T, B, R) and y.is_contiguous()
    assert addend is None or (addend.dtype == yw.dtype and tuple(addend.shape) == (T, B, R) and addend.is_contiguous())
    check(_lib.lib().asr_lc_scatter(stream(), ptr(yw), ptr(addend), ptr(_len_i32(x_len, B, yw.device)), ptr(_len_i32(n_win, B, yw.device)),
                                    ptr(y), T, B, R, Nc, Nr, int(mode)), "asr_lc_scatter")
    return y


def lc_push(state, m, chunk, n, window, Nc, Nr, flush=None):
    """asr_lc_push: state (Nc + Nr - 1, B, R) 16-bit pending rows and m (B) int32 their counts (both updated), chunk (Tc, B, R) or None,
    n (B) int32 or None, flush (B) int32 or None (these slots end), window (K + Tc, B, R) (written: [pending | new | zeros]) ->
    (a, w, emit), (B) int32 each: the rows in the window, its whole blocks, the frames the layer emits"""
    K, B, R = state.shape
    Nc, Nr = int(Nc), int(Nr)
    Tc = 0 if chunk is None else chunk.shape[0]
    assert K == Nc + Nr - 1 and state.element_size() == 2 and window.dtype == state.dtype and tuple(window.shape) == (K + Tc, B, R)
    assert chunk is None or (chunk.dtype == state.dtype and tuple(chunk.shape[1:]) == (B, R) and chunk.is_contiguous())
    assert m.dtype == torch.int32 and m.numel() == B and window.is_contiguous()
    dev = state.device
    a, w, emit = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    check(_lib.lib().asr_lc_push(stream(), ptr(state) if K else None, ptr(m), ptr(chunk) if Tc else None, ptr(_len_i32(n, B, dev)),
                                 ptr(_len_i32(flush, B, dev)), ptr(window) if window.numel() else None, ptr(a), ptr(w), ptr(emit),
                                 Tc, B, R, Nc, Nr), "asr_lc_push")
    return a, w, emit


# ---------------------------------------------------------------------------------------------- streaming log-mel front end
FBANK_STREAM_MAX_FRAMES = 128   # ASR_FBANK_STREAM_MAX_FRAMES, ASR_FBANK_STREAM_MAX_FILT and ASR_FBANK_STREAM_META of include/asr_hip.h
FBANK_STREAM_MAX_FILT = 64
FBANK_STREAM_META = 8


def fbank_stream_push(chunk, n, flush, pend, last, meta, window, wlen, k, frame_len, frame_step, preemph):
    """asr_fbank_stream_push: chunk (B, Nc) int16 / float32 or None (a flush), n / flush (B) int32 or None; pend (B, >= L) f32, last (B)
    f32 and meta (B, 8) int32 are the slots' state (updated); window (B, pitch) f32, wlen and k (B) int32 are written"""
    B = meta.shape[0]
    Nc = 0 if chunk is None else chunk.shape[1]
    if chunk is not None and chunk.dtype not in (F32, torch.int16):
        raise ValueError("samples must be int16 or float32, got %s" % chunk.dtype)
    assert chunk is None or (chunk.dim() == 2 and chunk.shape[0] == B and chunk.stride(1) == 1)
    assert pend.dtype == F32 and last.dtype == F32 and window.dtype == F32 and window.stride(1) == 1 and pend.stride(1) == 1
    assert meta.dtype == torch.int32 and tuple(meta.shape) == (B, FBANK_STREAM_META) and wlen.dtype == torch.int32 and k.dtype == torch.int32
    dev = meta.device
    check(_lib.lib().asr_fbank_stream_push(stream(), chunk.data_ptr() if Nc else None, 1 if chunk is not None and chunk.dtype == F32 else 0,
                                           chunk.stride(0) if Nc else 0, Nc, ptr(_len_i32(n, B, dev)), ptr(_len_i32(flush, B, dev)),
                                           pend.data_ptr(), pend.stride(0), ptr(last), ptr(meta), window.data_ptr(), window.stride(0),
                                           ptr(wlen), ptr(k), B, int(frame_len), int(frame_step), float(preemph)), "asr_fbank_stream_push")


def fbank_stream_deltas(logmel, k, flush, meta, out, lengths, mean=None, std=None):
    """asr_fbank_stream_deltas: logmel (B, Fmax, nfilt) f32 (rows 0..3 of a slot: carried, updated; rows 4..: this call's), k / flush (B)
    int32, meta (B, 8) int32 (updated); out (B, 3, nfilt, Tc) f32 and lengths (B) int32 are written"""
    B, Fmax, nfilt = logmel.shape
    Tc = out.shape[3]
    assert logmel.dtype == F32 and out.dtype == F32 and tuple(out.shape) == (B, 3, nfilt, Tc) and lengths.dtype == torch.int32
    dev = meta.device
    check(_lib.lib().asr_fbank_stream_deltas(stream(), ptr(logmel), ptr(_len_i32(k, B, dev)), ptr(_len_i32(flush, B, dev)), ptr(meta), B, Fmax,
                                             nfilt, Tc, ptr(mean), ptr(std), ptr(out), ptr(lengths)), "asr_fbank_stream_deltas")


def fbank_stream_reset(meta, mask=None):
    """empty every slot of a feature stream, or those with mask[b] != 0"""
    B = meta.shape[0]
    check(_lib.lib().asr_fbank_stream_reset(stream(), ptr(meta), ptr(_len_i32(mask, B, meta.device)), B), "asr_fbank_stream_reset")
