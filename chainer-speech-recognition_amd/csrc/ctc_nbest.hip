// N-best CTC scoring for gfx950: the exact log p(h_n | x_b) of N hypotheses per utterance and the gradient of
// sum_{b,n} gy[b,n] log p(h_n | x_b) with respect to the logits -- the primitive under expected-error (MWER) training and exact
// rescoring of a beam's N-best list.  The reference has no counterpart (its only sequence criterion is the CTC / Gram-CTC loss).
//
// The N hypotheses of an utterance share its logit rows, so the two passes over the logits run once per (t, b) row, not once
// per (t, b, n); only the lattices are per hypothesis.  "Utterance" u = b * N + n for the kernels shared with the loss:
//   prep     (B*N workgroups)    csrc/ctc_lattice.hpp, the loss's; a hypothesis of length 0 is the single blank node
//   rows     (T*B workgroups)    log-sum-exp of the row as ctc::rows_kernel forms it, then log p on the path nodes of all N
//                                lattices of b; frame 0 also writes every lattice's x_len (0 for an unused slot)
//                                                                                                [HBM: read T*B*V once]
//   lattice  (2*B*N workgroups)  csrc/ctc_sweep.hpp, the loss's alpha / beta recursion, float64
//   logp     (1 workgroup)       total -> f32 log p, -inf for an unused or infeasible slot
//   grad     (T*B workgroups)    sum_n gy[b,n] * occupancy_n scattered into one LDS row, grad = that - (sum_n gy[b,n]) * softmax;
//                                each row written once                                           [HBM: read+write T*B*V once]
//
// Gram-CTC (asr_gram_ctc_nbest_*): the hypotheses are strings of characters, and the lattice of a string offers the unigram token
// of every character and the bigram token of every adjacent pair that the table `gram` spells.  Three kernels in front of the
// same five turn characters into the lattice's two label rows:
//   index fill / insert          an open-addressing table spelling -> token id, built in the workspace from `gram` on every call
//   gram_labels (B*N workgroups) uni[i] = token of (s[i]), big[i] = token of (s[i-1], s[i]), the effective length of the slot
// then prep<true>, rows, lattice<7>, logp and, in the backward call, grad exactly as above with the padded path length of 3 L + 1.
#include "common.hpp"
#include "ctc_ws.hpp"
#include "ctc_lattice.hpp"
#include "ctc_sweep.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace ctc_nbest {

constexpr int kMaxN = 128;          // the beam's limit (csrc/ctc_beam.hip)
constexpr int kOccChunk = 8192;     // as ctc::grad_kernel

// One workgroup per (t, b) row: lse exactly as ctc::rows_kernel (same loops, same reductions), then
// lp[u][t][s] = x[label_s] - lse for the N lattices u = b * N + n.  The gathers hit the row this workgroup has just read.
// The workgroups of frame 0 also write the x_len of the N lattices of their utterance for the sweep: the utterance's for a used
// slot, 0 for an unused one (the sweep then reports -inf and touches nothing).
__global__ __launch_bounds__(256) void rows_kernel(const float* __restrict__ xs, const int* __restrict__ x_len,
                                                   const int* __restrict__ hyp_len, const int* __restrict__ path_label, int T,
                                                   int B, int V, int N, int Sp, int* __restrict__ x_len_u,
                                                   float* __restrict__ lse_out, float* __restrict__ lp) {
    __shared__ float scratch[32];
    const int row = blockIdx.x;            // row = t * B + b
    const int t = row / B, b = row - t * B;
    const int xl = x_len ? min(x_len[b], T) : T;
    if (t == 0 && (int)threadIdx.x < N) x_len_u[b * N + threadIdx.x] = hyp_len[b * N + threadIdx.x] < 0 ? 0 : max(xl, 0);
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
    // node (n, s) = flat index threadIdx.x + k * blockDim.x; Sp is a multiple of 64: a wave stays inside one lattice
    int n = (int)threadIdx.x / Sp, s = (int)threadIdx.x - n * Sp;
    while (n < N) {                         // (an unused slot is the one-node lattice of the empty labelling; its sweep reads nothing)
        const size_t u = (size_t)b * N + n;
        const int l = path_label[u * Sp + s];
        lp[(u * T + t) * Sp + s] = l >= 0 ? x[l] - lse : -INFINITY;
        s += blockDim.x;
        while (s >= Sp) { s -= Sp; ++n; }
    }
}

__global__ void logp_kernel(const double* __restrict__ total, int U, float* __restrict__ logp) {
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < U; u += gridDim.x * blockDim.x) {
        const double tot = total[u];
        logp[u] = tot == -INFINITY ? -INFINITY : (float)tot;
    }
}

// One workgroup per (t, b) row.  grad = sum_n c_n (occ_n - softmax), c_n = gy[b, n] for a slot with a finite log p and 0 for
// every other slot, whose gy (which may hold anything) is selected away.  V not a multiple of 4, unaligned rows and V above the
// occupancy chunk as in ctc::grad_kernel.
__global__ __launch_bounds__(256) void grad_kernel(const float* __restrict__ xs, const int* __restrict__ x_len,
                                                   const int* __restrict__ path_label, const int* __restrict__ path_len,
                                                   const float* __restrict__ lse_in, const double* __restrict__ alpha,
                                                   const double* __restrict__ beta, const double* __restrict__ total,
                                                   const float* __restrict__ gy, int T, int B, int V, int N, int Sp,
                                                   float* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float coef[kMaxN];
    __shared__ int len_s[kMaxN];
    __shared__ double tot_s[kMaxN];
    float* occ = reinterpret_cast<float*>(smem);
    const int row = blockIdx.x;
    const int t = row / B, b = row - t * B;
    const int xl = x_len ? min(x_len[b], T) : T;
    float* g = grad + (size_t)row * V;
    const bool vec = ((V & 3) == 0) && ((((uintptr_t)g) & 15) == 0) && ((((uintptr_t)(xs + (size_t)row * V)) & 15) == 0);
    if (t >= xl) {
        if (vec) {
            float4* g4 = reinterpret_cast<float4*>(g);
            for (int i = threadIdx.x; i < (V >> 2); i += blockDim.x) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int i = threadIdx.x; i < V; i += blockDim.x) g[i] = 0.f;
        }
        return;
    }
    if ((int)threadIdx.x < N) {
        const size_t u = (size_t)b * N + threadIdx.x;
        const double tot = total[u];        // three independent loads; a dead slot's gy is selected away, never used in arithmetic
        const float gv = gy[u];
        const int len = path_len[u];
        const bool live = tot != -INFINITY;
        coef[threadIdx.x] = live ? gv : 0.f;
        tot_s[threadIdx.x] = tot;
        len_s[threadIdx.x] = live ? len : 0;
    }
    for (int i = threadIdx.x; i < min(kOccChunk, V); i += blockDim.x) occ[i] = 0.f;
    __syncthreads();                        // coef / tot_s / len_s and the zeroed occ are visible
    float csum = 0.f;                       // every thread adds the same N values in the same order (LDS broadcasts)
    for (int n = 0; n < N; ++n) csum += coef[n];
    const float* x = xs + (size_t)row * V;
    const float lse = lse_in[row];
    for (int v0 = 0; v0 < V; v0 += kOccChunk) {
        const int vn = min(kOccChunk, V - v0);
        if (v0 > 0) {
            for (int i = threadIdx.x; i < vn; i += blockDim.x) occ[i] = 0.f;
            __syncthreads();
        }
        // node (n, s) = flat index threadIdx.x + k * blockDim.x
        int n = (int)threadIdx.x / Sp, s = (int)threadIdx.x - n * Sp;
        while (n < N) {
            if (s < len_s[n]) {
                const size_t u = (size_t)b * N + n;
                const int l = path_label[u * Sp + s];
                if (l >= v0 && l < v0 + vn) {
                    const size_t at = (u * T + t) * Sp + s;
                    const double e = alpha[at] + beta[at] - tot_s[n];
                    if (e > -80.0) atomicAdd(&occ[l - v0], coef[n] * expf((float)e));
                }
            }
            s += blockDim.x;
            while (s >= Sp) { s -= Sp; ++n; }
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
                r.x = ov.x - __expf(xv.x - lse) * csum;
                r.y = ov.y - __expf(xv.y - lse) * csum;
                r.z = ov.z - __expf(xv.z - lse) * csum;
                r.w = ov.w - __expf(xv.w - lse) * csum;
                g4[i] = r;
            }
        } else {
            for (int i = threadIdx.x; i < vn; i += blockDim.x) g[v0 + i] = occ[i] - __expf(x[v0 + i] - lse) * csum;
        }
        if (v0 + kOccChunk < V) __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ spelling index (Gram-CTC)
// Open addressing, linear probing, capacity a power of two >= 2 V.  Key: first character in the high word, second (or -1) in the
// low word; the empty key is the blank's (-1, -1), which is never inserted.  Table values are only hashed and compared, never used
// as an index (the rule of the Gram-CTC beam, csrc/ctc_beam.hip).
constexpr unsigned long long kEmptyKey = ~0ull;

__device__ __forceinline__ unsigned long long spell_key(int first, int second) {
    return ((unsigned long long)(unsigned)first << 32) | (unsigned long long)(unsigned)second;
}

__device__ __forceinline__ size_t spell_hash(unsigned long long k) {      // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (size_t)k;
}

__global__ void index_fill_kernel(unsigned long long* __restrict__ key, int* __restrict__ val, size_t cap) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (size_t)gridDim.x * blockDim.x) {
        key[i] = kEmptyKey;
        val[i] = 0x7fffffff;
    }
}

// One row of `gram` per thread.  Two rows with the same spelling (a table the Python wrapper rejects) share a slot and keep the
// smaller token id, whatever order the threads arrive in.
__global__ void index_insert_kernel(const int* __restrict__ gram, int V, unsigned long long* __restrict__ key,
                                    int* __restrict__ val, size_t cap) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int a = gram[2 * (size_t)v], b = gram[2 * (size_t)v + 1];
    if (a < 0 || a >= V || b < -1 || b >= V) return;        // the blank, an id that is never emitted, or not a spelling
    const unsigned long long k = spell_key(a, b);
    size_t slot = spell_hash(k) & (cap - 1);
    for (size_t probe = 0; probe < cap; ++probe) {          // (at most V of the >= 2 V slots are ever claimed: the loop ends early)
        const unsigned long long seen = atomicCAS(&key[slot], kEmptyKey, k);
        if (seen == kEmptyKey || seen == k) {
            atomicMin(&val[slot], v);
            return;
        }
        slot = (slot + 1) & (cap - 1);
    }
}

// token id that spells (first, second), -1: none.  Reads what index_insert_kernel wrote in an earlier launch.
__device__ __forceinline__ int spell_find(const unsigned long long* __restrict__ key, const int* __restrict__ val, size_t cap,
                                          int first, int second) {
    if (first < 0 || second < -1) return -1;                // (would be, or alias, the empty key)
    const unsigned long long k = spell_key(first, second);
    size_t slot = spell_hash(k) & (cap - 1);
    for (size_t probe = 0; probe < cap; ++probe) {
        const unsigned long long seen = key[slot];
        if (seen == k) return val[slot];
        if (seen == kEmptyKey) return -1;
        slot = (slot + 1) & (cap - 1);
    }
    return -1;
}

// One workgroup per slot u = b * N + n: the two label rows of the string's Gram-CTC lattice (every bigram of the table offered)
// and the slot's effective length -- hyp_len clamped to Lmax; -1 (unused, log p = -inf) for hyp_len < 0 and for a string with a
// character that has no unigram token (a negative or out-of-range character included).
__global__ __launch_bounds__(256) void gram_labels_kernel(const int* __restrict__ hyp, const int* __restrict__ hyp_len, int Lmax,
                                                          const unsigned long long* __restrict__ key,
                                                          const int* __restrict__ val, size_t cap, int* __restrict__ uni,
                                                          int* __restrict__ big, int* __restrict__ eff_len) {
    const size_t u = blockIdx.x;
    const int len = min(hyp_len[u], Lmax);
    const int* s = hyp + u * Lmax;
    int missing = 0;
    for (int i = threadIdx.x; i < Lmax; i += blockDim.x) {
        int lu = -1, lb = -1;
        if (i < len) {
            const int c = s[i];
            lu = spell_find(key, val, cap, c, -1);
            if (i >= 1 && c >= 0) lb = spell_find(key, val, cap, s[i - 1], c);
            missing |= lu < 0;
        }
        uni[u * Lmax + i] = lu;
        big[u * Lmax + i] = lb;
    }
    missing = __syncthreads_or(missing);
    if (threadIdx.x == 0) eff_len[u] = (len < 0 || missing) ? -1 : len;
}

static size_t lattice_lds(int Sp) { return sizeof(double) * 2 * (Sp + 16) + sizeof(int) * (Sp + 8); }

// BAD_ARG / UNSUPPORTED for the dimensions both calls take; ASR_OK otherwise
static int check_dims(int T, int B, int V, int N, int Lmax, int gram) {
    if (T <= 0 || B <= 0 || V <= 0 || Lmax <= 0) return ASR_ERR_BAD_ARG;
    if (N <= 0) return gram ? ASR_ERR_UNSUPPORTED : ASR_ERR_BAD_ARG;      // the Gram-CTC entries report every N outside [1, 128] alike
    if (N > kMaxN) return ASR_ERR_UNSUPPORTED;
    if (Lmax > 0x7fffffff / 4) return ASR_ERR_UNSUPPORTED;                                            // 3 Lmax + 1 + padding is an int
    if ((long long)B * N > 0x7fffffffLL / ctc::path_pad(Lmax, gram)) return ASR_ERR_UNSUPPORTED;   // int lattice indices
    if (lattice_lds(ctc::path_pad(Lmax, gram)) > 150 * 1024) return ASR_ERR_UNSUPPORTED;           // as asr_ctc_forward_lse
    return ASR_OK;
}

}  // namespace ctc_nbest
}  // namespace asr

using namespace asr;

extern "C" size_t asr_ctc_nbest_workspace_bytes(int T, int B, int V, int N, int Lmax) {
    if (ctc_nbest::check_dims(T, B, V, N, Lmax, 0) != ASR_OK) return 0;
    return ctc::carve_nbest(nullptr, T, B, N, Lmax, 0, V).bytes;
}

extern "C" int asr_ctc_nbest_forward(void* stream_, const float* xs, const int32_t* hyp, const int32_t* hyp_len,
                                     const int32_t* x_len, int T, int B, int V, int N, int Lmax, int blank, float* logp,
                                     void* workspace, size_t workspace_bytes) {
    if (!xs || !hyp || !hyp_len || !logp || !workspace) return ASR_ERR_BAD_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || Lmax <= 0 || blank < 0 || blank >= V) return ASR_ERR_BAD_ARG;
    const int rc = ctc_nbest::check_dims(T, B, V, N, Lmax, 0);
    if (rc != ASR_OK) return rc;
    ctc::NbestWorkspace w = ctc::carve_nbest(workspace, T, B, N, Lmax, 0, V);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    const int Sp = ctc::path_pad(Lmax, 0), U = B * N;
    const size_t lds = ctc_nbest::lattice_lds(Sp);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(ctc::prep_kernel<false>, dim3(U), dim3(256), 0, stream, hyp, (const int*)nullptr, hyp_len, Lmax, Sp, V, blank,
                       w.path_label, w.path_mask, w.path_len);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_nbest::rows_kernel, dim3(T * B), dim3(256), 0, stream, xs, x_len, hyp_len, w.path_label, T, B, V, N, Sp,
                       w.x_len, w.lse, w.lp);
    ASR_LAUNCH_CHECK();
    const int threads = Sp < 1024 ? Sp : 1024;
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)ctc::lattice_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(ctc::lattice_kernel<3>, dim3(U, 2), dim3(threads), lds, stream, w.lp, w.x_len, w.path_label, w.path_mask,
                       w.path_len, T, U, Sp, w.alpha, w.beta, w.total, w.loss);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_nbest::logp_kernel, dim3(cdiv(U, 256)), dim3(256), 0, stream, w.total, U, logp);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_ctc_nbest_backward(void* stream_, const float* xs, const int32_t* x_len, int T, int B, int V, int N, int Lmax,
                                      const float* gy, float* grad, const void* workspace, size_t workspace_bytes) {
    if (!xs || !gy || !grad || !workspace) return ASR_ERR_BAD_ARG;
    const int rc = ctc_nbest::check_dims(T, B, V, N, Lmax, 0);
    if (rc != ASR_OK) return rc;
    ctc::NbestWorkspace w = ctc::carve_nbest(const_cast<void*>(workspace), T, B, N, Lmax, 0, V);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    const int Sp = ctc::path_pad(Lmax, 0);
    const size_t lds = sizeof(float) * (size_t)(V < ctc_nbest::kOccChunk ? (int)align_up(V, 4) : ctc_nbest::kOccChunk);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(ctc_nbest::grad_kernel, dim3(T * B), dim3(256), lds, stream, xs, x_len, w.path_label, w.path_len, w.lse,
                       w.alpha, w.beta, w.total, gy, T, B, V, N, Sp, grad);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

// ------------------------------------------------------------------------------------------------ Gram-CTC
extern "C" size_t asr_gram_ctc_nbest_workspace_bytes(int T, int B, int V, int N, int Lmax) {
    if (ctc_nbest::check_dims(T, B, V, N, Lmax, 1) != ASR_OK) return 0;
    return ctc::carve_nbest(nullptr, T, B, N, Lmax, 1, V).bytes;
}

extern "C" int asr_gram_ctc_nbest_forward(void* stream_, const float* xs, const int32_t* hyp, const int32_t* hyp_len,
                                          const int32_t* x_len, const int32_t* gram, int T, int B, int V, int N, int Lmax,
                                          int blank, float* logp, void* workspace, size_t workspace_bytes) {
    if (!xs || !hyp || !hyp_len || !logp || !workspace) return ASR_ERR_BAD_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || Lmax <= 0 || blank < 0 || blank >= V) return ASR_ERR_BAD_ARG;
    const int rc = ctc_nbest::check_dims(T, B, V, N, Lmax, 1);
    if (rc != ASR_OK) return rc;
    if (!gram) return ASR_ERR_UNSUPPORTED;                  // as asr_gram_ctc_beam_search
    ctc::NbestWorkspace w = ctc::carve_nbest(workspace, T, B, N, Lmax, 1, V);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    const int Sp = ctc::path_pad(Lmax, 1), U = B * N;
    const size_t lds = ctc_nbest::lattice_lds(Sp);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(ctc_nbest::index_fill_kernel, dim3(w.idx_cap < 256 * 1024 ? cdiv((long long)w.idx_cap, 256) : 1024), dim3(256), 0,
                       stream, w.idx_key, w.idx_val, w.idx_cap);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_nbest::index_insert_kernel, dim3(cdiv(V, 256)), dim3(256), 0, stream, gram, V, w.idx_key, w.idx_val,
                       w.idx_cap);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_nbest::gram_labels_kernel, dim3(U), dim3(256), 0, stream, hyp, hyp_len, Lmax, w.idx_key, w.idx_val,
                       w.idx_cap, w.lab_uni, w.lab_big, w.eff_len);
    ASR_LAUNCH_CHECK();
    // from here on the loss's Gram-CTC lattice and the CTC N-best's row / sweep / logp kernels, on the effective lengths
    hipLaunchKernelGGL(ctc::prep_kernel<true>, dim3(U), dim3(256), 0, stream, w.lab_uni, w.lab_big, w.eff_len, Lmax, Sp, V, blank,
                       w.path_label, w.path_mask, w.path_len);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_nbest::rows_kernel, dim3(T * B), dim3(256), 0, stream, xs, x_len, w.eff_len, w.path_label, T, B, V, N, Sp,
                       w.x_len, w.lse, w.lp);
    ASR_LAUNCH_CHECK();
    const int threads = Sp < 1024 ? Sp : 1024;
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)ctc::lattice_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(ctc::lattice_kernel<7>, dim3(U, 2), dim3(threads), lds, stream, w.lp, w.x_len, w.path_label, w.path_mask,
                       w.path_len, T, U, Sp, w.alpha, w.beta, w.total, w.loss);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_nbest::logp_kernel, dim3(cdiv(U, 256)), dim3(256), 0, stream, w.total, U, logp);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_gram_ctc_nbest_backward(void* stream_, const float* xs, const int32_t* x_len, int T, int B, int V, int N,
                                           int Lmax, const float* gy, float* grad, const void* workspace,
                                           size_t workspace_bytes) {
    if (!xs || !gy || !grad || !workspace) return ASR_ERR_BAD_ARG;
    const int rc = ctc_nbest::check_dims(T, B, V, N, Lmax, 1);
    if (rc != ASR_OK) return rc;
    ctc::NbestWorkspace w = ctc::carve_nbest(const_cast<void*>(workspace), T, B, N, Lmax, 1, V);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    const int Sp = ctc::path_pad(Lmax, 1);
    const size_t lds = sizeof(float) * (size_t)(V < ctc_nbest::kOccChunk ? (int)align_up(V, 4) : ctc_nbest::kOccChunk);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(ctc_nbest::grad_kernel, dim3(T * B), dim3(256), lds, stream, xs, x_len, w.path_label, w.path_len, w.lse,
                       w.alpha, w.beta, w.total, gy, T, B, V, N, Sp, grad);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
