// The alpha / beta sweep of the CTC / Gram-CTC lattice: the sum over all paths.  ONE definition for the loss (csrc/ctc.hip: one
// lattice per utterance) and the N-best scoring (csrc/ctc_nbest.hip: one lattice per (utterance, hypothesis)), so that the two
// can never disagree about the recursion or its numerics (float64 accumulation).
#pragma once
#include "common.hpp"
#include "ctc_lattice.hpp"

namespace asr {
namespace ctc {

// ------------------------------------------------------------------------------------------------ lattice
// log(sum_j exp(v_j)) over the inputs the mask names.  The offset m only has to be NEAR the maximum (the identity holds for any m),
// so it is found in float32 -- one v_max3_f32 per three inputs instead of a chain of canonicalising v_max_f64 / v_cndmask pairs --
// and floored at -1e30: dead inputs (-inf) then give exp(-inf) = 0 and an all-dead node log(0) = -inf without a branch.  The
// differences v_j - m are formed in float64 (exact), the transcendentals in float32 on arguments <= ~1e-3: absolute error ~1e-7
// as before.  The step of the lattice is one dependent chain (LDS read -> ... -> LDS write, ~0.3 us); this form has 16 instructions
// on it instead of 35 (v_log_f32 x ln 2 instead of the denormal-safe logf sequence: the sum lies in [1, NK]).
template <int NK>
__device__ __forceinline__ double lse_masked(const double* v, int mask) {
    float f[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) f[j] = (mask & (1 << j)) ? (float)v[j] : -INFINITY;
    float m32 = -1e30f;
#pragma unroll
    for (int j = 0; j < NK; ++j) m32 = __builtin_fmaxf(m32, f[j]);
    const double m = (double)m32;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const float e = __expf((float)(v[j] - m));
        acc += (mask & (1 << j)) ? e : 0.f;
    }
    return m + (double)(__builtin_amdgcn_logf(acc) * 0.69314718f);       // acc == 0 (no live input): log2 -> -inf
}

template <int NK>
__global__ __launch_bounds__(1024) void lattice_kernel(const float* __restrict__ lp, const int* __restrict__ x_len,
                                                       const int* __restrict__ path_label,
                                                       const int* __restrict__ path_mask,
                                                       const int* __restrict__ path_len, int T, int B, int Sp,
                                                       double* __restrict__ alpha, double* __restrict__ beta,
                                                       double* __restrict__ total, float* __restrict__ loss) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* buf0 = reinterpret_cast<double*>(smem);          // Sp + 8 doubles each, 8 guard slots in front
    double* buf1 = buf0 + (Sp + 16);
    int* mask_s = reinterpret_cast<int*>(buf1 + (Sp + 16));  // Sp + 8 ints (8 guard slots behind)
    const int b = blockIdx.x;
    const bool backward = blockIdx.y == 1;
    const int xl = x_len ? min(x_len[b], T) : T;
    const int S = path_len[b];
    const float* lpb = lp + (size_t)b * T * Sp;
    double* outb = (backward ? beta : alpha) + (size_t)b * T * Sp;
    const int* pm = path_mask + (size_t)b * Sp;
    const int* pl = path_label + (size_t)b * Sp;

    // guards: reading s - k (forward) or s + k (backward) outside [0, Sp) sees -inf / mask 0
    for (int i = threadIdx.x; i < Sp + 16; i += blockDim.x) {
        buf0[i] = -INFINITY;
        buf1[i] = -INFINITY;
    }
    for (int i = threadIdx.x; i < Sp + 8; i += blockDim.x) mask_s[i] = i < Sp ? pm[i] : 0;
    __syncthreads();
    double* prev = buf0 + 8;   // index s in [-8, Sp + 8)
    double* cur = buf1 + 8;

    if (xl <= 0) {
        if (!backward && threadIdx.x == 0) { total[b] = -INFINITY; loss[b] = 1e10f; }
        return;
    }

    const bool one_node = (int)blockDim.x >= Sp;          // one node per thread: lp is prefetched PF steps ahead in registers
    constexpr int PF = 4;
    if (!backward && one_node) {
        if (threadIdx.x == 0) prev[0] = 0.0;
        __syncthreads();
        const int sidx = threadIdx.x;
        const int mk = mask_s[sidx];
        // Whole blocks of PF steps run without a branch and every step issues exactly one store and one load (the prefetch index is
        // clamped, not guarded): gfx9 counts loads and stores in ONE in-order counter, and only in straight-line code can the
        // compiler wait for "all but the 2 (PF - 1) youngest" -- behind a branch it waits for vmcnt(0), i.e. every step paid the
        // round trip of the alpha store and the prefetch it had just issued.
        float lq[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) lq[j] = lpb[(size_t)min(j, xl - 1) * Sp + sidx];
        int t0 = 0;
        for (; t0 + PF <= xl; t0 += PF) {
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int t = t0 + j;
                double v[NK];
#pragma unroll
                for (int q = 0; q < NK; ++q) v[q] = prev[sidx - koff<NK>(q)];
                const double a = lse_masked<NK>(v, mk) + (double)lq[j];
                cur[sidx] = a;
                outb[(size_t)t * Sp + sidx] = a;
                lq[j] = lpb[(size_t)min(t + PF, xl - 1) * Sp + sidx];
                ASR_LDS_BARRIER();
                double* tmp = prev; prev = cur; cur = tmp;
            }
        }
#pragma unroll
        for (int j = 0; j < PF - 1; ++j) {         // the last xl % PF steps: their log-probabilities are in lq[0 .. ] already
            const int t = t0 + j;
            if (t < xl) {                          // uniform over the workgroup
                double v[NK];
#pragma unroll
                for (int q = 0; q < NK; ++q) v[q] = prev[sidx - koff<NK>(q)];
                const double a = lse_masked<NK>(v, mk) + (double)lq[j];
                cur[sidx] = a;
                outb[(size_t)t * Sp + sidx] = a;
                ASR_LDS_BARRIER();
                double* tmp = prev; prev = cur; cur = tmp;
            }
        }
        if (threadIdx.x == 0) {
            double v[3] = {-INFINITY, -INFINITY, -INFINITY};
            v[0] = prev[S - 1];
            if (S >= 2) v[1] = prev[S - 2];
            if (NK != 3 && S >= 3) v[2] = prev[S - 3];
            const double tot = lse_masked<3>(v, 7);
            total[b] = tot;
            loss[b] = tot == -INFINITY ? 1e10f : (float)(-tot);
        }
    } else if (backward && one_node) {
        const int sidx = threadIdx.x;
        bool fin;
        if (NK == 3) fin = (sidx == S - 1) || (sidx == S - 2 && S >= 2);
        else fin = (sidx == S - 1) || (S >= 3 && (sidx == S - 2 || sidx == S - 3));
        fin = fin && pl[sidx] >= 0;
        const double bt0 = fin ? 0.0 : -INFINITY;
        outb[(size_t)(xl - 1) * Sp + sidx] = bt0;
        prev[sidx] = bt0 + (double)lpb[(size_t)(xl - 1) * Sp + sidx];
        int mkd = 0;                                 // edge s -> s + k belongs to the destination's mask
#pragma unroll
        for (int q = 0; q < NK; ++q) mkd |= ((mask_s[sidx + koff<NK>(q)] >> q) & 1) << q;
        __syncthreads();
        float lq[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) lq[j] = lpb[(size_t)max(xl - 2 - j, 0) * Sp + sidx];
        int t0 = xl - 2;
        for (; t0 - (PF - 1) >= 0; t0 -= PF) {      // whole blocks of PF steps, branch-free (see the forward loop)
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const int t = t0 - j;
                double v[NK];
#pragma unroll
                for (int q = 0; q < NK; ++q) v[q] = prev[sidx + koff<NK>(q)];
                const double bt = lse_masked<NK>(v, mkd);
                outb[(size_t)t * Sp + sidx] = bt;
                cur[sidx] = bt + (double)lq[j];
                lq[j] = lpb[(size_t)max(t - PF, 0) * Sp + sidx];
                ASR_LDS_BARRIER();
                double* tmp = prev; prev = cur; cur = tmp;
            }
        }
#pragma unroll
        for (int j = 0; j < PF - 1; ++j) {
            const int t = t0 - j;
            if (t >= 0) {
                double v[NK];
#pragma unroll
                for (int q = 0; q < NK; ++q) v[q] = prev[sidx + koff<NK>(q)];
                const double bt = lse_masked<NK>(v, mkd);
                outb[(size_t)t * Sp + sidx] = bt;
                cur[sidx] = bt + (double)lq[j];
                ASR_LDS_BARRIER();
                double* tmp = prev; prev = cur; cur = tmp;
            }
        }
    } else if (!backward) {
        if (threadIdx.x == 0) prev[0] = 0.0;    // virtual alpha_{-1} = e_0  (asr/loss/gram_ctc.py:144)
        __syncthreads();
        for (int t = 0; t < xl; ++t) {
            const float* lpt = lpb + (size_t)t * Sp;
            double* ot = outb + (size_t)t * Sp;
            for (int s = threadIdx.x; s < Sp; s += blockDim.x) {
                const int mk = mask_s[s];
                double v[NK];
#pragma unroll
                for (int j = 0; j < NK; ++j) v[j] = prev[s - koff<NK>(j)];
                double a = lse_masked<NK>(v, mk);
                a += (double)lpt[s];
                cur[s] = a;
                ot[s] = a;
            }
            __syncthreads();
            double* tmp = prev; prev = cur; cur = tmp;
        }
        // prev = alpha_{xl-1}; final nodes: last blank, last unigram, last bigram (if alive)
        if (threadIdx.x == 0) {
            double v[3] = {-INFINITY, -INFINITY, -INFINITY};
            v[0] = prev[S - 1];
            if (S >= 2) v[1] = prev[S - 2];
            if (NK != 3 && S >= 3) v[2] = prev[S - 3];
            // dead nodes hold -inf already (their lp is -inf)
            const double tot = lse_masked<3>(v, 7);
            total[b] = tot;
            loss[b] = tot == -INFINITY ? 1e10f : (float)(-tot);
        }
    } else {
        // beta_{xl-1}[s] = 0 on final nodes
        for (int s = threadIdx.x; s < Sp; s += blockDim.x) {
            bool fin;
            if (NK == 3) fin = (s == S - 1) || (s == S - 2 && S >= 2);
            else fin = (s == S - 1) || (S >= 3 && (s == S - 2 || s == S - 3));
            fin = fin && pl[s] >= 0;
            const double bt = fin ? 0.0 : -INFINITY;
            outb[(size_t)(xl - 1) * Sp + s] = bt;
            prev[s] = bt + (double)lpb[(size_t)(xl - 1) * Sp + s];     // w_{xl-1}
        }
        __syncthreads();
        for (int t = xl - 2; t >= 0; --t) {
            const float* lpt = lpb + (size_t)t * Sp;
            double* ot = outb + (size_t)t * Sp;
            for (int s = threadIdx.x; s < Sp; s += blockDim.x) {
                double v[NK];
                int mk = 0;
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    const int k = koff<NK>(j);
                    v[j] = prev[s + k];
                    mk |= ((mask_s[s + k] >> j) & 1) << j;     // edge s -> s + k belongs to the destination's mask
                }
                const double bt = lse_masked<NK>(v, mk);
                ot[s] = bt;
                cur[s] = bt + (double)lpt[s];
            }
            __syncthreads();
            double* tmp = prev; prev = cur; cur = tmp;
        }
    }
}

}  // namespace ctc
}  // namespace asr
