// Carry kernels of the streaming forward (asr/model/stream.py): a per-slot delay line of K rows of R 16-bit features.
// asr_stream_push assembles, per slot b, the left-aligned window [m[b] carried rows | n[b] new rows | zeros] in a
// (K + Tc, B, R) buffer, the window's valid length, the number of rows the layer behind it may emit, and the new state (the last
// min(K, m + n) valid rows).  Two launches: the first only reads the state, the second only reads the window, so a chunk shorter
// than K (old state rows shift) never reads what it has overwritten.  Copies only: 16-byte vector loads and stores.
#include "common.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace {

__device__ __forceinline__ int slot_rows(int mode, const int* m, int K, int b) {
    return mode == ASR_STREAM_CONTEXT ? K : min(max(m[b], 0), K);
}
__device__ __forceinline__ int chunk_rows(const int* n, const int* flush, int Tc, int b) {
    if (flush) return 0;                                    // an end-of-utterance call feeds nothing
    return n ? min(max(n[b], 0), Tc) : Tc;
}

// one thread per 16-byte lane of the window: (row w, slot b, lane l)
__global__ __launch_bounds__(256) void stream_window_kernel(const uint4* __restrict__ state, const int* __restrict__ m,
                                                            const uint4* __restrict__ chunk, const int* __restrict__ n,
                                                            const int* __restrict__ flush, uint4* __restrict__ window,
                                                            int* __restrict__ wlen, int* __restrict__ emit, int K, int Tc, int B,
                                                            int L, int mode) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)(K + Tc) * B * L) return;
    const int l = (int)(i % L), b = (int)((i / L) % B), w = (int)(i / ((long long)L * B));
    const int mb = slot_rows(mode, m, K, b), nb = chunk_rows(n, flush, Tc, b);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (w < mb) v = state[((size_t)w * B + b) * L + l];
    else if (w < mb + nb) v = chunk[((size_t)(w - mb) * B + b) * L + l];
    window[i] = v;
    if (w == 0 && l == 0) {
        wlen[b] = mb + nb;
        if (mode == ASR_STREAM_CONTEXT) emit[b] = nb;
        else emit[b] = (flush && flush[b]) ? mb : max(0, mb + nb - K);
    }
}

// one thread per 16-byte lane of the state: (row k, slot b, lane l).  A slot that was fed nothing keeps its bytes.
__global__ __launch_bounds__(256) void stream_state_kernel(uint4* __restrict__ state, int* __restrict__ m,
                                                           const uint4* __restrict__ window, const int* __restrict__ wlen,
                                                           const int* __restrict__ n, const int* __restrict__ flush, int K, int Tc,
                                                           int B, int L, int mode) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)K * B * L) return;
    const int l = (int)(i % L), b = (int)((i / L) % B), k = (int)(i / ((long long)L * B));
    if (flush) {                                            // end of utterance: the flushed slots start over, the others stay
        if (!flush[b]) return;
        state[i] = make_uint4(0u, 0u, 0u, 0u);
        if (m && k == 0 && l == 0) m[b] = 0;
        return;
    }
    if (chunk_rows(n, flush, Tc, b) == 0) return;
    const int valid = wlen[b], keep = min(K, valid);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (k < keep) v = window[((size_t)(valid - keep + k) * B + b) * L + l];
    state[i] = v;
    if (mode != ASR_STREAM_CONTEXT && k == 0 && l == 0) m[b] = keep;
}

__global__ __launch_bounds__(256) void stream_reset_kernel(uint4* __restrict__ state, int* __restrict__ m, const int* __restrict__ mask,
                                                           int K, int B, int L) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)max(K, 1) * B * L) return;
    const int l = (int)(i % L), b = (int)((i / L) % B), k = (int)(i / ((long long)L * B));
    if (mask && !mask[b]) return;
    if (k < K) state[i] = make_uint4(0u, 0u, 0u, 0u);
    if (m && k == 0 && l == 0) m[b] = 0;
}

bool push_shape_ok(int K, int B, int R, int mode) {
    return K >= 0 && B >= 1 && R >= 8 && (mode == ASR_STREAM_CONTEXT || mode == ASR_STREAM_LOOKAHEAD);
}

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" int asr_stream_push(void* stream, void* state, int* m, const void* chunk, const int* n, const int* flush, void* window,
                               int* wlen, int* emit, int K, int Tc, int B, int R, int mode) {
    if (!push_shape_ok(K, B, R, mode) || Tc < 0 || K + Tc < 1 || !window || !wlen || !emit || (K > 0 && !state) || (Tc > 0 && !chunk) ||
        (mode == ASR_STREAM_LOOKAHEAD && !m) || (flush && mode != ASR_STREAM_LOOKAHEAD))
        return ASR_ERR_BAD_ARG;
    if (R % 8 != 0) return ASR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int L = R / 8;
    hipLaunchKernelGGL(stream_window_kernel, dim3(cdiv((long long)(K + Tc) * B * L, 256)), dim3(256), 0, st, (const uint4*)state, m,
                       (const uint4*)chunk, n, flush, (uint4*)window, wlen, emit, K, Tc, B, L, mode);
    ASR_LAUNCH_CHECK();
    if (K > 0) {
        hipLaunchKernelGGL(stream_state_kernel, dim3(cdiv((long long)K * B * L, 256)), dim3(256), 0, st, (uint4*)state, m,
                           (const uint4*)window, wlen, n, flush, K, Tc, B, L, mode);
        ASR_LAUNCH_CHECK();
    }
    return ASR_OK;
}

extern "C" int asr_stream_push_reset(void* stream, void* state, int* m, const int* mask, int K, int B, int R) {
    if (K < 0 || B < 1 || R < 8 || (K > 0 && !state)) return ASR_ERR_BAD_ARG;
    if (R % 8 != 0) return ASR_ERR_UNSUPPORTED;
    const int L = R / 8;
    hipLaunchKernelGGL(stream_reset_kernel, dim3(cdiv((long long)max(K, 1) * B * L, 256)), dim3(256), 0, (hipStream_t)stream,
                       (uint4*)state, m, mask, K, B, L);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
