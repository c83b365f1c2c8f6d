// CTC and Gram-CTC loss + gradient for gfx950.
//
// Replaces (reference file:line):
//   Chainer F.connectionist_temporal_classification   call sites run/ctc/cnn/train.py:162,191
//   asr/loss/gram_ctc.py:219-297 (GramCTC.forward/backward), :142-178 (alpha/beta), :180-217 (label prob)
//
// The reference multiplies dense (B, N, N) log connection matrices every time step; the lattice only has
// the diagonals k in {0,1,2} (CTC) / {0,1,2,3,5,6,7} (Gram-CTC), so each node reads <= 7 neighbours from LDS.
//
// Four kernels, all on the caller's stream:
//   prep     (B workgroups)      path labels + per-node edge bitmask (csrc/ctc_lattice.hpp, shared with the alignment)
//   rows     (T*B workgroups)    log-sum-exp of every logit row, gather log p on the path        [HBM: read T*B*V]
//   lattice  (2*B workgroups)    alpha (blockIdx.y=0) and beta (blockIdx.y=1) recursions, state in LDS;
//                                f64 accumulation, f32 exp/log only on differences <= 0
//                                (csrc/ctc_sweep.hpp, shared with the N-best scoring of csrc/ctc_nbest.hip)
//   grad     (T*B workgroups)    occupancy scatter into an LDS row, grad = (softmax - occ) * scale [HBM: read+write T*B*V]
#include "common.hpp"
#include "ctc_ws.hpp"
#include "ctc_lattice.hpp"
#include "ctc_sweep.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace ctc {

// ------------------------------------------------------------------------------------------------ rows
// One workgroup per (t, b) row of logits: lse = log sum exp, then lp[b][t][s] = x[label_s] - lse.
__global__ __launch_bounds__(256) void rows_kernel(const float* __restrict__ xs, const int* __restrict__ x_len,
                                                   const int* __restrict__ path_label, int T, int B, int V, int Sp,
                                                   float* __restrict__ lse_out, float* __restrict__ lp, const float* __restrict__ lse_in) {
    __shared__ float scratch[32];
    if (lse_in) {       // the producer of the logits formed the row's log-sum-exp while it had the row in registers: gather only,
                        // one wave per row, four rows per workgroup
        const int row = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (row >= T * B) return;
        const int t = row / B, b = row - t * B;
        const int xl = x_len ? min(x_len[b], T) : T;
        if (t >= xl) return;
        const float* x = xs + (size_t)row * V;
        const float lse = lse_in[row];
        if (lane == 0) lse_out[row] = lse;
        const int* pl = path_label + (size_t)b * Sp;
        float* out = lp + ((size_t)b * T + t) * Sp;
        for (int s = lane; s < Sp; s += 64) {
            const int l = pl[s];
            out[s] = l >= 0 ? x[l] - lse : -INFINITY;
        }
        return;
    }
    const int row = blockIdx.x;            // row = t * B + b
    const int t = row / B, b = row - t * B;
    const int xl = x_len ? min(x_len[b], T) : T;
    if (t >= xl) return;
    const float* x = xs + (size_t)row * V;
    float m = -INFINITY;
    const bool vec = ((V & 3) == 0) && ((((uintptr_t)x) & 15) == 0);
    if (vec) {
        const float4* x4 = reinterpret_cast<const float4*>(x);
        for (int i = threadIdx.x; i < (V >> 2); i += blockDim.x) {
            const float4 v = x4[i];
            m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
    } else {
        for (int i = threadIdx.x; i < V; i += blockDim.x) m = fmaxf(m, x[i]);
    }
    m = block_max(m, scratch);
    float sum = 0.f;
    if (vec) {
        const float4* x4 = reinterpret_cast<const float4*>(x);
        for (int i = threadIdx.x; i < (V >> 2); i += blockDim.x) {
            const float4 v = x4[i];
            sum += __expf(v.x - m) + __expf(v.y - m) + __expf(v.z - m) + __expf(v.w - m);
        }
    } else {
        for (int i = threadIdx.x; i < V; i += blockDim.x) sum += __expf(x[i] - m);
    }
    sum = block_sum(sum, scratch);
    const float lse = m + __logf(sum);
    if (threadIdx.x == 0) lse_out[row] = lse;
    const int* pl = path_label + (size_t)b * Sp;
    float* out = lp + ((size_t)b * T + t) * Sp;
    for (int s = threadIdx.x; s < Sp; s += blockDim.x) {
        const int l = pl[s];
        out[s] = l >= 0 ? x[l] - lse : -INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ grad
constexpr int kOccChunk = 8192;

__global__ __launch_bounds__(256) void grad_kernel(const float* __restrict__ xs, const int* __restrict__ x_len,
                                                   const int* __restrict__ path_label,
                                                   const int* __restrict__ path_len, const float* __restrict__ lse_in,
                                                   const double* __restrict__ alpha, const double* __restrict__ beta,
                                                   const double* __restrict__ total, const float* __restrict__ gy,
                                                   int gy_per_utt, float scale, int T, int B, int V, int Sp,
                                                   float* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* occ = reinterpret_cast<float*>(smem);
    const int row = blockIdx.x;
    const int t = row / B, b = row - t * B;
    const int xl = x_len ? min(x_len[b], T) : T;
    float* g = grad + (size_t)row * V;
    const bool vec = ((V & 3) == 0) && ((((uintptr_t)g) & 15) == 0) && ((((uintptr_t)(xs + (size_t)row * V)) & 15) == 0);
    if (t >= xl) {      // asr/loss/gram_ctc.py:296
        if (vec) {
            float4* g4 = reinterpret_cast<float4*>(g);
            for (int i = threadIdx.x; i < (V >> 2); i += blockDim.x) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int i = threadIdx.x; i < V; i += blockDim.x) g[i] = 0.f;
        }
        return;
    }
    const float* x = xs + (size_t)row * V;
    const float lse = lse_in[row];
    const double tot = total[b];
    float sc = scale;
    if (gy) sc *= gy_per_utt ? gy[b] : gy[0];
    const int S = path_len[b];
    const int* pl = path_label + (size_t)b * Sp;
    const double* al = alpha + ((size_t)b * T + t) * Sp;
    const double* be = beta + ((size_t)b * T + t) * Sp;
    for (int v0 = 0; v0 < V; v0 += kOccChunk) {
        const int vn = min(kOccChunk, V - v0);
        for (int i = threadIdx.x; i < vn; i += blockDim.x) occ[i] = 0.f;
        __syncthreads();
        if (tot != -INFINITY) {
            for (int s = threadIdx.x; s < S; s += blockDim.x) {
                const int l = pl[s];
                if (l >= v0 && l < v0 + vn) {
                    const double e = al[s] + be[s] - tot;
                    if (e > -80.0) atomicAdd(&occ[l - v0], expf((float)e));
                }
            }
        }
        __syncthreads();
        if (vec) {
            const float4* x4 = reinterpret_cast<const float4*>(x + v0);
            const float4* o4 = reinterpret_cast<const float4*>(occ);
            float4* g4 = reinterpret_cast<float4*>(g + v0);
            for (int i = threadIdx.x; i < (vn >> 2); i += blockDim.x) {
                const float4 xv = x4[i];
                const float4 ov = o4[i];
                float4 r;
                r.x = (__expf(xv.x - lse) - ov.x) * sc;
                r.y = (__expf(xv.y - lse) - ov.y) * sc;
                r.z = (__expf(xv.z - lse) - ov.z) * sc;
                r.w = (__expf(xv.w - lse) - ov.w) * sc;
                g4[i] = r;
            }
        } else {
            for (int i = threadIdx.x; i < vn; i += blockDim.x) g[v0 + i] = (__expf(x[v0 + i] - lse) - occ[i]) * sc;
        }
        __syncthreads();
    }
}

__global__ void mean_kernel(const float* __restrict__ loss, int B, float* __restrict__ out) {
    __shared__ float scratch[32];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) s += loss[i];
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) out[0] = s / (float)B;
}

}  // namespace ctc
}  // namespace asr

using namespace asr;
using namespace asr::ctc;

extern "C" size_t asr_ctc_workspace_bytes(int T, int B, int V, int Lmax, int gram) {
    (void)V;
    if (T <= 0 || B <= 0 || Lmax <= 0) return 0;
    return carve(nullptr, T, B, Lmax, gram).bytes;
}

extern "C" int asr_ctc_forward_lse(void* stream_, const float* xs, const int32_t* label_unigram,
                                   const int32_t* label_bigram, const int32_t* x_len, const int32_t* l_len, int T, int B,
                                   int V, int Lmax, int blank, float* loss_per_utt, float* loss_mean, void* workspace,
                                   size_t workspace_bytes, const float* row_lse) {
    if (!xs || !label_unigram || !loss_per_utt || !workspace) return ASR_ERR_BAD_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || Lmax <= 0 || blank < 0 || blank >= V) return ASR_ERR_BAD_ARG;
    const int gram = label_bigram != nullptr;
    Workspace w = carve(workspace, T, B, Lmax, gram);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    const int Sp = path_pad(Lmax, gram);
    const size_t lds = sizeof(double) * 2 * (Sp + 16) + sizeof(int) * (Sp + 8);
    if (lds > 150 * 1024) return ASR_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    if (gram)
        hipLaunchKernelGGL(prep_kernel<true>, dim3(B), dim3(256), 0, stream, label_unigram, label_bigram, l_len, Lmax, Sp,
                           V, blank, w.path_label, w.path_mask, w.path_len);
    else
        hipLaunchKernelGGL(prep_kernel<false>, dim3(B), dim3(256), 0, stream, label_unigram, label_bigram, l_len, Lmax,
                           Sp, V, blank, w.path_label, w.path_mask, w.path_len);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rows_kernel, dim3(row_lse ? (T * B + 3) / 4 : T * B), dim3(256), 0, stream, xs, x_len, w.path_label, T, B, V, Sp, w.lse, w.lp, row_lse);
    ASR_LAUNCH_CHECK();
    const int threads = Sp < 1024 ? Sp : 1024;
    if (gram) {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)lattice_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(lattice_kernel<7>, dim3(B, 2), dim3(threads), lds, stream, w.lp, x_len, w.path_label,
                           w.path_mask, w.path_len, T, B, Sp, w.alpha, w.beta, w.total, loss_per_utt);
    } else {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)lattice_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(lattice_kernel<3>, dim3(B, 2), dim3(threads), lds, stream, w.lp, x_len, w.path_label,
                           w.path_mask, w.path_len, T, B, Sp, w.alpha, w.beta, w.total, loss_per_utt);
    }
    ASR_LAUNCH_CHECK();
    if (loss_mean) {
        hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, stream, loss_per_utt, B, loss_mean);
        ASR_LAUNCH_CHECK();
    }
    return ASR_OK;
}

extern "C" int asr_ctc_forward(void* stream_, const float* xs, const int32_t* label_unigram,
                               const int32_t* label_bigram, const int32_t* x_len, const int32_t* l_len, int T, int B,
                               int V, int Lmax, int blank, float* loss_per_utt, float* loss_mean, void* workspace,
                               size_t workspace_bytes) {
    return asr_ctc_forward_lse(stream_, xs, label_unigram, label_bigram, x_len, l_len, T, B, V, Lmax, blank, loss_per_utt, loss_mean,
                               workspace, workspace_bytes, nullptr);
}

extern "C" int asr_ctc_backward(void* stream_, const float* xs, const int32_t* x_len, int T, int B, int V, int Lmax,
                                int gram, const float* gy, int gy_per_utt, float scale, float* grad,
                                const void* workspace, size_t workspace_bytes) {
    if (!xs || !grad || !workspace) return ASR_ERR_BAD_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || Lmax <= 0) return ASR_ERR_BAD_ARG;
    Workspace w = carve(const_cast<void*>(workspace), T, B, Lmax, gram);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    const int Sp = path_pad(Lmax, gram);
    const size_t lds = sizeof(float) * (size_t)(V < kOccChunk ? (int)align_up(V, 4) : kOccChunk);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(grad_kernel, dim3(T * B), dim3(256), lds, stream, xs, x_len, w.path_label, w.path_len, w.lse,
                       w.alpha, w.beta, w.total, gy, gy_per_utt, scale, T, B, V, Sp, grad);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_ctc_loss_grad(void* stream, const float* xs, const int32_t* label_unigram,
                                 const int32_t* label_bigram, const int32_t* x_len, const int32_t* l_len, int T, int B,
                                 int V, int Lmax, int blank, float scale, float* loss_per_utt, float* loss_mean,
                                 float* grad, void* workspace, size_t workspace_bytes) {
    int rc = asr_ctc_forward(stream, xs, label_unigram, label_bigram, x_len, l_len, T, B, V, Lmax, blank, loss_per_utt,
                             loss_mean, workspace, workspace_bytes);
    if (rc != ASR_OK) return rc;
    return asr_ctc_backward(stream, xs, x_len, T, B, V, Lmax, label_bigram != nullptr, nullptr, 0, scale, grad,
                            workspace, workspace_bytes);
}
