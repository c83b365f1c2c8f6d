// Window copies of the latency-controlled bidirectional GRU (asr.nn.LCBiGRU, asr/functions.py: lc_bigru; the semantics are stated in
// include/asr_hip.h).  The reverse direction of the layer is restarted for every block of Nc frames and sees Nr frames of right
// context: asr_lc_gather lays block c of slot b, with its right context and time-reversed, into window c * B + b of a (W, C * B, R)
// batch that the ndir = 1 recurrence runs with per-window lengths; asr_lc_scatter brings the windows' rows back to (T, B, R) and adds
// them up.  Each is the other's adjoint, so the backward pass is the same two kernels.  asr_lc_push is the streaming carry: per slot,
// [m pending rows | n new rows], the whole blocks in them and the rows that wait for their right context.
// One thread per 16-byte lane of the tensor a kernel WRITES, so every store of a wave is dense; no atomics, every output element is
// written by exactly one thread.  The sums of the scatter are float32 in a fixed order (addend, then ascending block) with one rounding.
#include "common.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace {

__device__ __forceinline__ int clamped(const int* len, int T, int b) { return len ? min(max(len[b], 0), T) : T; }

// the live rows of window (c, b): the frames from c * Nc that the slot has, at most W, none for a window the caller switched off
__device__ __forceinline__ int live_rows(int len, const int* n_win, int b, int c, int Nc, int W) {
    if (n_win && c >= n_win[b]) return 0;
    return min(max(len - c * Nc, 0), W);                    // (c * Nc < T: no overflow)
}

// one thread per 16-byte lane of xw (W, C * B, L): (row j, window c * B + b, lane l)
__global__ __launch_bounds__(256) void lc_gather_kernel(const uint4* __restrict__ x, const int* __restrict__ x_len,
                                                        const int* __restrict__ n_win, uint4* __restrict__ xw, int* __restrict__ w_len,
                                                        int T, int B, int L, int Nc, int W, int CB, int keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)W * CB * L) return;
    const int l = (int)(i % L), wi = (int)((i / L) % CB), j = (int)(i / ((long long)L * CB));
    const int c = wi / B, b = wi - c * B;
    const int rows = live_rows(clamped(x_len, T, b), n_win, b, c, Nc, W);
    if (w_len && j == 0 && l == 0) w_len[wi] = rows;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    const int off = rows - 1 - j;                           // the frame of the block this row holds: the window is time-reversed
    if (off >= 0 && off < keep) v = x[((size_t)(c * Nc + off) * B + b) * L + l];       // (c * Nc + off < len <= T)
    xw[i] = v;
}

__device__ __forceinline__ void add_lane(float* acc, const uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[2 * q] += bf16_to_f32((uint16_t)(w[q] & 0xffffu));
        acc[2 * q + 1] += bf16_to_f32((uint16_t)(w[q] >> 16));
    }
}

// one thread per 16-byte lane of y (T, B, L): (frame t, slot b, lane l).  all_windows: every window whose live rows hold t, else the
// frame's own block only.
__global__ __launch_bounds__(256) void lc_scatter_kernel(const uint4* __restrict__ yw, const uint4* __restrict__ addend,
                                                         const int* __restrict__ x_len, const int* __restrict__ n_win,
                                                         uint4* __restrict__ y, int T, int B, int L, int Nc, int W, int CB,
                                                         int all_windows) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)T * B * L) return;
    const int l = (int)(i % L), b = (int)((i / L) % B), t = (int)(i / ((long long)L * B));
    const int len = clamped(x_len, T, b);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (t < len) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (addend) add_lane(acc, addend[i]);
        const int c_hi = t / Nc;
        const int c_lo = !all_windows ? c_hi : (t >= W ? (t - W) / Nc + 1 : 0);        // c * Nc + W > t, or the window cannot hold t
        for (int c = c_lo; c <= c_hi; ++c) {
            const int rows = live_rows(len, n_win, b, c, Nc, W), off = t - c * Nc;
            if (off < rows) add_lane(acc, yw[((size_t)(rows - 1 - off) * CB + c * B + b) * L + l]);     // (row < W, window < CB)
        }
        v = make_uint4(pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]), pack_bf16x2(acc[6], acc[7]));
    }
    y[i] = v;
}

__device__ __forceinline__ int pending_rows(const int* m, int K, int b) { return K > 0 ? min(max(m[b], 0), K) : 0; }
__device__ __forceinline__ int chunk_rows(const int* n, int Tc, int b) { return n ? min(max(n[b], 0), Tc) : Tc; }

// first launch of a push: one thread per 16-byte lane of the window (K + Tc, B, L).  Reads the state, never writes it.
__global__ __launch_bounds__(256) void lc_window_kernel(const uint4* __restrict__ state, const int* __restrict__ m,
                                                        const uint4* __restrict__ chunk, const int* __restrict__ n,
                                                        const int* __restrict__ flush, uint4* __restrict__ window, int* __restrict__ a,
                                                        int* __restrict__ w, int* __restrict__ emit, int K, int Tc, int B, int L, int Nc,
                                                        int Nr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)max(K + Tc, 1) * B * L) return;
    const int l = (int)(i % L), b = (int)((i / L) % B), r = (int)(i / ((long long)L * B));
    const int mb = pending_rows(m, K, b), nb = chunk_rows(n, Tc, b);
    if (r == 0 && l == 0) {
        const int ab = mb + nb, ended = flush && flush[b];
        const int wb = ended ? (ab + Nc - 1) / Nc : max(0, ab - Nr) / Nc;
        a[b] = ab;
        w[b] = wb;
        emit[b] = ended ? ab : wb * Nc;
    }
    if (r >= K + Tc) return;                                // (no rows at all: only the counts are written)
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r < mb) v = state[((size_t)r * B + b) * L + l];
    else if (r < mb + nb) v = chunk[((size_t)(r - mb) * B + b) * L + l];
    window[i] = v;
}

// second launch of a push: one thread per 16-byte lane of the state (K, B, L).  Reads the window and the counts of the first launch:
// the rows behind the emitted ones wait for their right context.  A slot that was fed nothing and does not end keeps its bytes.
__global__ __launch_bounds__(256) void lc_state_kernel(uint4* __restrict__ state, int* __restrict__ m, const uint4* __restrict__ window,
                                                       const int* __restrict__ a, const int* __restrict__ emit,
                                                       const int* __restrict__ n, const int* __restrict__ flush, int K, int Tc, int B,
                                                       int L) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)K * B * L) return;
    const int l = (int)(i % L), b = (int)((i / L) % B), k = (int)(i / ((long long)L * B));
    if (chunk_rows(n, Tc, b) == 0 && !(flush && flush[b])) return;
    const int first = emit[b], rest = a[b] - first;         // rest <= K: a - Nr < (w + 1) * Nc
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (k < rest) v = window[((size_t)(first + k) * B + b) * L + l];       // (first + k < a <= K + Tc)
    state[i] = v;
    if (k == 0 && l == 0) m[b] = rest;
}

// the shape of a gather or a scatter, checked and reduced: Nc and Nr beyond T change nothing, so they are clamped to it and every
// product of the index arithmetic below stays within int
struct Windows {
    int Nc, W, CB, L;
    bool ok;
};

Windows windows_of(int T, int B, int R, int Nc, int Nr, int mode) {
    Windows s = {0, 0, 0, 0, false};
    if (T < 0 || T > (1 << 30) || B < 1 || R < 8 || R % 8 != 0 || Nc < 1 || Nr < 0 || (mode != ASR_LC_WINDOW && mode != ASR_LC_BLOCK)) return s;
    s.L = R / 8;
    if (T == 0) {
        s.ok = true;
        return s;
    }
    s.Nc = min(Nc, T);
    s.W = (int)min((long long)s.Nc + min(Nr, T), (long long)T);
    const long long CB = (long long)((T + s.Nc - 1) / s.Nc) * B;
    if (s.W > ASR_LC_MAX_WINDOW || CB > INT_MAX || (long long)s.W * CB * s.L > INT_MAX || (long long)T * B * s.L > INT_MAX) return s;
    s.CB = (int)CB;
    s.ok = true;
    return s;
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" int asr_lc_gather(void* stream, const void* x, const int* x_len, const int* n_win, void* xw, int* w_len, int T, int B, int R,
                             int Nc, int Nr, int mode) {
    const Windows s = windows_of(T, B, R, Nc, Nr, mode);
    if (!s.ok || (T > 0 && (!x || !xw))) return ASR_ERR_BAD_ARG;
    if (T == 0) return ASR_OK;
    hipLaunchKernelGGL(lc_gather_kernel, dim3(cdiv((long long)s.W * s.CB * s.L, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x,
                       x_len, n_win, (uint4*)xw, w_len, T, B, s.L, s.Nc, s.W, s.CB, mode == ASR_LC_WINDOW ? s.W : s.Nc);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_lc_scatter(void* stream, const void* yw, const void* addend, const int* x_len, const int* n_win, void* y, int T, int B,
                              int R, int Nc, int Nr, int mode) {
    const Windows s = windows_of(T, B, R, Nc, Nr, mode);
    if (!s.ok || (T > 0 && (!yw || !y))) return ASR_ERR_BAD_ARG;
    if (T == 0) return ASR_OK;
    hipLaunchKernelGGL(lc_scatter_kernel, dim3(cdiv((long long)T * B * s.L, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)yw,
                       (const uint4*)addend, x_len, n_win, (uint4*)y, T, B, s.L, s.Nc, s.W, s.CB, mode == ASR_LC_WINDOW ? 1 : 0);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_lc_push(void* stream, void* state, int* m, const void* chunk, const int* n, const int* flush, void* window, int* a,
                           int* w, int* emit, int Tc, int B, int R, int Nc, int Nr) {
    if (Tc < 0 || B < 1 || R < 8 || R % 8 != 0 || Nc < 1 || Nr < 0 || (long long)Nc + Nr > ASR_LC_MAX_WINDOW || !a || !w || !emit)
        return ASR_ERR_BAD_ARG;
    const int K = Nc + Nr - 1, L = R / 8;
    const long long lanes = ((long long)K + Tc) * B * L;
    if (lanes > INT_MAX || (K > 0 && (!state || !m)) || (Tc > 0 && !chunk) || (K + Tc > 0 && !window)) return ASR_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lc_window_kernel, dim3(cdiv((long long)max(K + Tc, 1) * B * L, 256)), dim3(256), 0, st, (const uint4*)state, m,
                       (const uint4*)chunk, n, flush, (uint4*)window, a, w, emit, K, Tc, B, L, Nc, Nr);
    ASR_LAUNCH_CHECK();
    if (K > 0) {
        hipLaunchKernelGGL(lc_state_kernel, dim3(cdiv((long long)K * B * L, 256)), dim3(256), 0, st, (uint4*)state, m, (const uint4*)window,
                           a, emit, n, flush, K, Tc, B, L);
        ASR_LAUNCH_CHECK();
    }
    return ASR_OK;
}
