// Lookahead (row) convolution of Deep Speech 2: a per-feature FIR over the next tau frames, (T, B, D) activations.
//   y[t, b, d]  = sum_{j=0..tau} W[d, j] * x[t + j, b, d]      x = 0 at and beyond len[b]; y = 0 there as well
//   dx[t, b, d] = sum_{j=0..tau} W[d, j] * gy[t - j, b, d]     gy ignored at and beyond len[b]; dx = 0 there
//   dW[d, j]   += sum_{t, b} gy[t, b, d] * x[t + j, b, d]      two stages: per-workgroup partial sums, then one ordered sum
// Forward and backward-data are ONE kernel: a workgroup stages kTT + tau rows of one utterance and 128 features in LDS (the halo
// behind the tile forward, in front of it backward; the weights reversed backward), and every lane slides over the staged rows
// once, holding the last kRows taps in registers -- one LDS row read and one weight read per 4 x 8 multiply-adds.  Every output
// is a chain of exactly tau + 1 float32 fused multiply-adds in a fixed tap order (j = 0..tau forward, tau..0 backward) started
// from 0 and rounded once at the store: it does not depend on T, on the tile it fell into, or on where a stream was cut.
#include "common.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace {

constexpr int kTT = ASR_LOOKAHEAD_TIME_TILE;       // output rows per workgroup
constexpr int kDC = 128;                           // features per workgroup: 16 lanes of 8 (16 bytes)
constexpr int kRows = 4;                           // consecutive output rows per lane
constexpr int kBG = 4;                             // utterances a weight-gradient workgroup sums over
static_assert(kTT == 16 * kRows, "256 threads = 16 feature lanes x 16 row groups of kRows");

__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = bf16_to_f32((uint16_t)(w[i] & 0xffffu));
        f[2 * i + 1] = bf16_to_f32((uint16_t)(w[i] >> 16));
    }
}

// LDS image: xs[kTT + tau][16] uint4 (256-byte rows: a ds_read_b128 lane group covers 16 different 16-byte slots of a row
// whatever rows its lanes are on, so the plain pitch is conflict free), then ws[tau + 1][kDC] float (tap-major: a lane's 8
// weights of one tap are 32 contiguous bytes, the same for all row groups -- a broadcast).
template <bool BWD>
__global__ __launch_bounds__(256) void lookahead_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                        const int* __restrict__ len, uint16_t* __restrict__ y, int T, int B, int D,
                                                        int tau) {
    extern __shared__ uint4 smem[];
    uint4* xs = smem;
    float* ws = reinterpret_cast<float*>(smem + (size_t)(kTT + tau) * 16);
    const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
    const int t0 = blockIdx.x * kTT, b = blockIdx.y, d0 = blockIdx.z * kDC;
    const int n = len ? min(max(len[b], 0), T) : T;
    const int d = d0 + c * 8;
    const bool lane_on = d < D;
    const int tbase = BWD ? t0 - tau : t0;                  // time of staged row 0
    if (t0 < n) {                                           // (a tile wholly beyond the length only writes zeros)
        for (int i = r; i < kTT + tau; i += 16) {
            const int t = tbase + i;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (lane_on && t >= 0 && t < n) v = *reinterpret_cast<const uint4*>(x + ((size_t)t * B + b) * D + d);
            xs[i * 16 + c] = v;
        }
        for (int i = threadIdx.x; i < (tau + 1) * kDC; i += 256) {
            const int s = i / kDC, dd = i - s * kDC;        // step s of the slide applies tap s forward, tap tau - s backward
            ws[i] = (d0 + dd < D) ? w[(size_t)(d0 + dd) * (tau + 1) + (BWD ? tau - s : s)] : 0.f;
        }
    }
    __syncthreads();
    if (!lane_on) return;
    float acc[kRows][8];
#pragma unroll
    for (int o = 0; o < kRows; ++o)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[o][e] = 0.f;
    if (t0 < n) {
        // output o of this lane (tile row r * kRows + o) takes staged rows r * kRows + o + s, s = 0..tau, with weight step s.
        // Slide: staged row r * kRows + q serves output o at step s = q - o; wreg[o] holds the weights of step q - o.
        float wreg[kRows][8] = {};
        const int row0 = r * kRows;
        for (int q = 0; q < tau + kRows; ++q) {
#pragma unroll
            for (int o = kRows - 1; o > 0; --o)
#pragma unroll
                for (int e = 0; e < 8; ++e) wreg[o][e] = wreg[o - 1][e];
            if (q <= tau) {
                const float4 wa = *reinterpret_cast<const float4*>(ws + q * kDC + c * 8);
                const float4 wb = *reinterpret_cast<const float4*>(ws + q * kDC + c * 8 + 4);
                wreg[0][0] = wa.x; wreg[0][1] = wa.y; wreg[0][2] = wa.z; wreg[0][3] = wa.w;
                wreg[0][4] = wb.x; wreg[0][5] = wb.y; wreg[0][6] = wb.z; wreg[0][7] = wb.w;
            }
            float xv[8];
            unpack8(xs[(row0 + q) * 16 + c], xv);
#pragma unroll
            for (int o = 0; o < kRows; ++o) {
                if (q - o >= 0 && q - o <= tau) {           // (uniform: q is a loop counter)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[o][e] = fmaf(wreg[o][e], xv[e], acc[o][e]);
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        const int t = t0 + r * kRows + o;
        if (t >= T) break;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (t < n) {
            v.x = pack_bf16x2(acc[o][0], acc[o][1]);
            v.y = pack_bf16x2(acc[o][2], acc[o][3]);
            v.z = pack_bf16x2(acc[o][4], acc[o][5]);
            v.w = pack_bf16x2(acc[o][6], acc[o][7]);
        }
        *reinterpret_cast<uint4*>(y + ((size_t)t * B + b) * D + d) = v;
    }
}

// Weight gradient, stage 1.  Workgroup (time tile, group of kBG utterances, 128 features): lane (c, r) owns the taps j = r, r + 16, ...
// of its 8 features and adds gy[t] * x[t + j] over the tile's rows t ascending, utterance after utterance: one chain per (d, j) and
// workgroup.  Partial sums go to ws[(tile * groups + group)][j][D].
constexpr int kMaxTapSlots = (ASR_LOOKAHEAD_MAX_TAU + 1 + 15) / 16;

__global__ __launch_bounds__(256) void lookahead_dw_partial_kernel(const uint16_t* __restrict__ gy, const uint16_t* __restrict__ x,
                                                                   const int* __restrict__ len, float* __restrict__ part, int T,
                                                                   int B, int D, int tau) {
    extern __shared__ uint4 smem[];
    uint4* xs = smem;                                       // [kTT + tau][16]
    uint4* gs = smem + (size_t)(kTT + tau) * 16;            // [kTT][16]
    const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
    const int t0 = blockIdx.x * kTT, g = blockIdx.y, d0 = blockIdx.z * kDC;
    const int d = d0 + c * 8;
    const bool lane_on = d < D;
    float acc[kMaxTapSlots][8];
#pragma unroll
    for (int k = 0; k < kMaxTapSlots; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
    for (int b = g * kBG; b < min(B, (g + 1) * kBG); ++b) {
        const int n = len ? min(max(len[b], 0), T) : T;
        if (t0 >= n) continue;                              // (uniform)
        __syncthreads();                                    // the previous utterance's rows have been read
        for (int i = r; i < kTT + tau; i += 16) {
            const int t = t0 + i;
            uint4 v = make_uint4(0u, 0u, 0u, 0u), u = v;
            if (lane_on && t < n) {
                v = *reinterpret_cast<const uint4*>(x + ((size_t)t * B + b) * D + d);
                if (i < kTT) u = *reinterpret_cast<const uint4*>(gy + ((size_t)t * B + b) * D + d);
            }
            xs[i * 16 + c] = v;
            if (i < kTT) gs[i * 16 + c] = u;
        }
        __syncthreads();
        const int rows = min(kTT, n - t0);
        for (int i = 0; i < rows; ++i) {
            float gv[8];
            unpack8(gs[i * 16 + c], gv);
#pragma unroll
            for (int k = 0; k < kMaxTapSlots; ++k) {
                const int j = r + 16 * k;
                if (j <= tau) {
                    float xv[8];
                    unpack8(xs[(i + j) * 16 + c], xv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[k][e] = fmaf(gv[e], xv[e], acc[k][e]);
                }
            }
        }
    }
    if (!lane_on) return;
    float* out = part + ((size_t)blockIdx.x * gridDim.y + g) * (size_t)(tau + 1) * D;
#pragma unroll
    for (int k = 0; k < kMaxTapSlots; ++k) {
        const int j = r + 16 * k;
        if (j <= tau) {
            *reinterpret_cast<float4*>(out + (size_t)j * D + d) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
            *reinterpret_cast<float4*>(out + (size_t)j * D + d + 4) = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
        }
    }
}

// stage 2: dW[d][j] += the partial sums in workgroup order -- one thread per (j, d), one accumulation into the gradient buffer
__global__ __launch_bounds__(256) void lookahead_dw_sum_kernel(const float* __restrict__ part, float* __restrict__ dW, int P, int D,
                                                               int tau) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (tau + 1) * D) return;
    const int j = i / D, d = i - j * D;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += part[(size_t)p * (tau + 1) * D + i];
    dW[(size_t)d * (tau + 1) + j] += s;
}

bool shape_ok(int T, int B, int D, int tau) {
    return T >= 1 && B >= 1 && D >= 8 && tau >= 0;
}
// the largest image (tau = ASR_LOOKAHEAD_MAX_TAU) is past the 64 KB a kernel gets without asking
constexpr size_t kMaxLds = (size_t)(kTT + ASR_LOOKAHEAD_MAX_TAU) * 256 + (size_t)(ASR_LOOKAHEAD_MAX_TAU + 1) * kDC * sizeof(float);
template <bool BWD>
void launch_lookahead(hipStream_t st, const void* x, const float* w, const int* len, void* y, int T, int B, int D, int tau) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)lookahead_kernel<BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
        attr = true;
    }
    const size_t lds = (size_t)(kTT + tau) * 256 + (size_t)(tau + 1) * kDC * sizeof(float);
    hipLaunchKernelGGL(lookahead_kernel<BWD>, dim3(cdiv(T, kTT), B, cdiv(D, kDC)), dim3(256), lds, st, (const uint16_t*)x, w, len,
                       (uint16_t*)y, T, B, D, tau);
}
bool served(int B, int D, int tau) { return D % 8 == 0 && tau <= ASR_LOOKAHEAD_MAX_TAU && B <= 65535 && cdiv(D, kDC) <= 65535; }

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" size_t asr_lookahead_ws_bytes(int T, int B, int D, int tau) {
    if (!shape_ok(T, B, D, tau) || !served(B, D, tau)) return 0;
    return (size_t)cdiv(T, kTT) * cdiv(B, kBG) * (size_t)(tau + 1) * D * sizeof(float);
}

extern "C" int asr_lookahead_fwd(void* stream, const void* x_bf16, const float* w, const int* x_len, void* y_bf16, int T, int B, int D,
                                 int tau) {
    if (!x_bf16 || !w || !y_bf16 || !shape_ok(T, B, D, tau)) return ASR_ERR_BAD_ARG;
    if (!served(B, D, tau)) return ASR_ERR_UNSUPPORTED;
    launch_lookahead<false>((hipStream_t)stream, x_bf16, w, x_len, y_bf16, T, B, D, tau);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_lookahead_bwd(void* stream, const void* gy_bf16, const void* x_bf16, const float* w, const int* x_len, void* dx_bf16,
                                 float* dW, void* ws, size_t ws_bytes, int T, int B, int D, int tau) {
    if (!gy_bf16 || !w || !shape_ok(T, B, D, tau) || (dW && !x_bf16)) return ASR_ERR_BAD_ARG;
    if (!served(B, D, tau)) return ASR_ERR_UNSUPPORTED;
    if (dW && (!ws || ws_bytes < asr_lookahead_ws_bytes(T, B, D, tau))) return ASR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (dx_bf16) {
        launch_lookahead<true>(st, gy_bf16, w, x_len, dx_bf16, T, B, D, tau);
        ASR_LAUNCH_CHECK();
    }
    if (dW) {
        const int tiles = cdiv(T, kTT), groups = cdiv(B, kBG);
        const size_t lds = (size_t)(2 * kTT + tau) * 256;
        hipLaunchKernelGGL(lookahead_dw_partial_kernel, dim3(tiles, groups, cdiv(D, kDC)), dim3(256), lds, st, (const uint16_t*)gy_bf16,
                           (const uint16_t*)x_bf16, x_len, (float*)ws, T, B, D, tau);
        ASR_LAUNCH_CHECK();
        hipLaunchKernelGGL(lookahead_dw_sum_kernel, dim3(cdiv((long long)(tau + 1) * D, 256)), dim3(256), 0, st, (const float*)ws, dW,
                           tiles * groups, D, tau);
        ASR_LAUNCH_CHECK();
    }
    return ASR_OK;
}
