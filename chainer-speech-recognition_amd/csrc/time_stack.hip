// Time reduction by frame stacking (asr.nn.TimeStack, asr/model/stream.py): k consecutive frames of R 16-bit features become one
// frame of k * R features.  asr_time_stack_fwd / _bwd are the one-shot copy and its inverse; asr_time_stack_push is the streaming
// form: per slot, the groups of [m pending rows | n new rows], and the last (m + n) % k rows carried to the next chunk.
// Copies only: one thread per 16-byte lane of the tensor a kernel WRITES, so every store of a wave is dense; the loads are k
// dense runs of R features.  No atomics, every output element is written by exactly one thread.
#include "common.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace {

__device__ __forceinline__ int clamped(const int* len, int T, int b) { return len ? min(max(len[b], 0), T) : T; }

// one thread per 16-byte lane of y (G, B, k * L): (group g, slot b, frame j of the group, lane l)
__global__ __launch_bounds__(256) void time_stack_fwd_kernel(const uint4* __restrict__ x, const int* __restrict__ x_len,
                                                             uint4* __restrict__ y, int* __restrict__ y_len, int T, int G, int B, int L,
                                                             int k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int KL = k * L;
    if (i >= (long long)max(G, 1) * B * KL) return;
    const int c = (int)(i % KL), b = (int)((i / KL) % B), g = (int)(i / ((long long)KL * B));
    const int len = clamped(x_len, T, b);
    if (y_len && g == 0 && c == 0) y_len[b] = (len + k - 1) / k;
    if (g >= G) return;                                     // (T == 0: only the lengths are written)
    const int j = c / L, l = c - j * L, t = g * k + j;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (t < len) v = x[((size_t)t * B + b) * L + l];
    y[i] = v;
}

// one thread per 16-byte lane of dx (T, B, L): the inverse copy, zero at and beyond x_len[b]
__global__ __launch_bounds__(256) void time_stack_bwd_kernel(const uint4* __restrict__ gy, const int* __restrict__ x_len,
                                                             uint4* __restrict__ dx, int T, int B, int L, int k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)T * B * L) return;
    const int l = (int)(i % L), b = (int)((i / L) % B), t = (int)(i / ((long long)L * B));
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (t < clamped(x_len, T, b)) {
        const int g = t / k, j = t - g * k;
        v = gy[((size_t)g * B + b) * k * L + (size_t)j * L + l];
    }
    dx[i] = v;
}

// first launch of a push: one thread per 16-byte lane of y (G, B, k * L), G = ceil((k - 1 + Tc) / k).  Reads the state, never
// writes it.  Row s of the slot's sequence is state row s for s < m[b], chunk row s - m[b] for s < m[b] + n[b], zero behind: the
// trailing partial group lands in y zero-completed, where the second launch picks the new state up.
__global__ __launch_bounds__(256) void time_stack_groups_kernel(const uint4* __restrict__ state, const int* __restrict__ m,
                                                                const uint4* __restrict__ chunk, const int* __restrict__ n,
                                                                const int* __restrict__ flush, uint4* __restrict__ y,
                                                                int* __restrict__ emit, int Tc, int G, int B, int L, int k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int KL = k * L;
    if (i >= (long long)max(G, 1) * B * KL) return;
    const int c = (int)(i % KL), b = (int)((i / KL) % B), g = (int)(i / ((long long)KL * B));
    int mb = k > 1 ? min(max(m[b], 0), k - 1) : 0;
    int nb = n ? min(max(n[b], 0), Tc) : Tc;
    if (flush) {                                            // end of utterance: nothing is fed, the flushed slots give their rest
        nb = 0;
        if (!flush[b]) mb = 0;
    }
    if (g == 0 && c == 0) emit[b] = flush ? (mb > 0 ? 1 : 0) : (mb + nb) / k;
    if (g >= G) return;                                     // (k == 1 and Tc == 0: only emit is written)
    const int j = c / L, l = c - j * L, s = g * k + j;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (s < mb) v = state[((size_t)s * B + b) * L + l];
    else if (s < mb + nb) v = chunk[((size_t)(s - mb) * B + b) * L + l];
    y[i] = v;
}

// second launch of a push: one workgroup per slot, so that m[b] is read by all of its threads before one of them writes it.
// Reads y only: the new state is the zero-completed partial group behind the emitted ones.
__global__ __launch_bounds__(256) void time_stack_state_kernel(uint4* __restrict__ state, int* __restrict__ m,
                                                               const uint4* __restrict__ y, const int* __restrict__ n,
                                                               const int* __restrict__ flush, int Tc, int B, int L, int k) {
    const int b = blockIdx.x;
    const int mb = min(max(m[b], 0), k - 1);
    __syncthreads();
    if (flush) {                                            // the flushed slots start over, the others stay
        if (!flush[b]) return;
        for (int i = threadIdx.x; i < (k - 1) * L; i += 256) state[((size_t)(i / L) * B + b) * L + i % L] = make_uint4(0u, 0u, 0u, 0u);
        if (threadIdx.x == 0) m[b] = 0;
        return;
    }
    const int nb = n ? min(max(n[b], 0), Tc) : Tc;
    if (nb == 0) return;                                    // a slot that was fed nothing keeps its bytes
    const int g = (mb + nb) / k, rest = (mb + nb) - g * k;
    for (int i = threadIdx.x; i < (k - 1) * L; i += 256) {
        const int j = i / L, l = i - j * L;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (j < rest) v = y[((size_t)g * B + b) * k * L + (size_t)j * L + l];       // (rest > 0 implies g < G)
        state[((size_t)j * B + b) * L + l] = v;
    }
    if (threadIdx.x == 0) m[b] = rest;
}

// one workgroup per slot
__global__ __launch_bounds__(256) void time_stack_reset_kernel(uint4* __restrict__ state, int* __restrict__ m,
                                                               const int* __restrict__ mask, int B, int L, int k) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    for (int i = threadIdx.x; i < (k - 1) * L; i += 256) state[((size_t)(i / L) * B + b) * L + i % L] = make_uint4(0u, 0u, 0u, 0u);
    if (m && threadIdx.x == 0) m[b] = 0;
}

bool stack_supported(int R, int k) { return R % 8 == 0 && k >= 1 && k <= ASR_TIME_STACK_MAX; }

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" int asr_time_stack_fwd(void* stream, const void* x, const int* x_len, void* y, int* y_len, int T, int B, int R, int k) {
    if (T < 0 || B < 1 || R < 1 || (T > 0 && (!x || !y))) return ASR_ERR_BAD_ARG;
    if (!stack_supported(R, k)) return ASR_ERR_UNSUPPORTED;
    const int L = R / 8, G = (T + k - 1) / k;
    if (G == 0 && !y_len) return ASR_OK;
    hipLaunchKernelGGL(time_stack_fwd_kernel, dim3(cdiv((long long)max(G, 1) * B * k * L, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint4*)x, x_len, (uint4*)y, y_len, T, G, B, L, k);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_time_stack_bwd(void* stream, const void* gy, const int* x_len, void* dx, int T, int B, int R, int k) {
    if (T < 0 || B < 1 || R < 1 || (T > 0 && (!gy || !dx))) return ASR_ERR_BAD_ARG;
    if (!stack_supported(R, k)) return ASR_ERR_UNSUPPORTED;
    if (T == 0) return ASR_OK;
    const int L = R / 8;
    hipLaunchKernelGGL(time_stack_bwd_kernel, dim3(cdiv((long long)T * B * L, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)gy,
                       x_len, (uint4*)dx, T, B, L, k);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_time_stack_push(void* stream, void* state, int* m, const void* chunk, const int* n, const int* flush, void* y,
                                   int* emit, int Tc, int B, int R, int k) {
    if (Tc < 0 || B < 1 || R < 1 || !emit || (Tc > 0 && !flush && !chunk)) return ASR_ERR_BAD_ARG;
    if (!stack_supported(R, k)) return ASR_ERR_UNSUPPORTED;
    const int L = R / 8, G = (k - 1 + Tc + k - 1) / k;
    if ((G > 0 && !y) || (k > 1 && (!state || !m))) return ASR_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(time_stack_groups_kernel, dim3(cdiv((long long)max(G, 1) * B * k * L, 256)), dim3(256), 0, st, (const uint4*)state,
                       m, (const uint4*)chunk, n, flush, (uint4*)y, emit, Tc, G, B, L, k);
    ASR_LAUNCH_CHECK();
    if (k > 1) {
        hipLaunchKernelGGL(time_stack_state_kernel, dim3(B), dim3(256), 0, st, (uint4*)state, m, (const uint4*)y, n, flush, Tc, B, L, k);
        ASR_LAUNCH_CHECK();
    }
    return ASR_OK;
}

extern "C" int asr_time_stack_push_reset(void* stream, void* state, int* m, const int* mask, int B, int R, int k) {
    if (B < 1 || R < 1) return ASR_ERR_BAD_ARG;
    if (!stack_supported(R, k)) return ASR_ERR_UNSUPPORTED;
    if (k > 1 && !state) return ASR_ERR_BAD_ARG;
    hipLaunchKernelGGL(time_stack_reset_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (uint4*)state, m, mask, B, R / 8, k);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
