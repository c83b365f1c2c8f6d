// The CTC / Gram-CTC lattice: node labels, edge masks and path length of every utterance.  ONE definition for the loss
// (csrc/ctc.hip: the sum over all paths) and the forced alignment (csrc/ctc_align.hip: the best path), so that the two
// can never disagree about which paths exist.
#pragma once
#include "common.hpp"

namespace asr {
namespace ctc {

// diagonal offset of edge class j: CTC {0,1,2}; Gram-CTC {0,1,2,3,5,6,7}
template <int NK>
__device__ __forceinline__ constexpr int koff(int j) { return NK == 3 ? j : (j < 4 ? j : j + 1); }

// ------------------------------------------------------------------------------------------------ prep
template <bool GRAM>
__global__ void prep_kernel(const int* __restrict__ uni, const int* __restrict__ big, const int* __restrict__ l_len,
                            int Lmax, int Sp, int V, int blank, int* __restrict__ path_label,
                            int* __restrict__ path_mask, int* __restrict__ path_len) {
    const int b = blockIdx.x;
    int len = l_len ? l_len[b] : Lmax;
    len = min(max(len, 0), Lmax);
    const int S = (GRAM ? 3 : 2) * len + 1;
    if (threadIdx.x == 0) path_len[b] = S;
    const int* u = uni + (size_t)b * Lmax;
    const int* g = GRAM ? big + (size_t)b * Lmax : nullptr;
    for (int s = threadIdx.x; s < Sp; s += blockDim.x) {
        int label = -1, mask = 0;
        if (s < S) {
            if (!GRAM) {
                const int i = (s - 1) >> 1;
                const bool odd = s & 1;
                label = odd ? u[i] : blank;
                if (label < 0 || label >= V) label = -1;
                if (label >= 0) {
                    mask = 1;
                    if (s >= 1) mask |= 2;
                    if (odd && i >= 1 && u[i] != u[i - 1]) mask |= 4;
                }
            } else {
                const int kind = s % 3, i = s / 3;
                auto alive_at = [&](int q) -> bool {   // node q of this path is usable
                    if (q < 0 || q >= S) return false;
                    const int kq = q % 3, iq = q / 3;
                    const int l = kq == 0 ? blank : (kq == 1 ? u[iq] : g[iq]);
                    return l >= 0 && l < V;
                };
                label = kind == 0 ? blank : (kind == 1 ? u[i] : g[i]);
                if (label < 0 || label >= V) label = -1;
                if (label >= 0) {
                    mask = 1;                                                        // k = 0
                    if (kind != 2 && alive_at(s - 1)) mask |= 1 << 1;                 // k = 1
                    if (kind != 2 && alive_at(s - 2)) mask |= 1 << 2;                 // k = 2
                    if (kind == 1 && i >= 1 && u[i] != u[i - 1] && alive_at(s - 3)) mask |= 1 << 3;   // k = 3
                    if (kind == 2 && alive_at(s - 5)) mask |= 1 << 4;                 // k = 5
                    if (kind == 2 && i >= 2 && g[i] != g[i - 2] && alive_at(s - 6)) mask |= 1 << 5;   // k = 6
                    if (kind == 2 && alive_at(s - 7)) mask |= 1 << 6;                 // k = 7
                }
            }
        }
        path_label[(size_t)b * Sp + s] = label;
        path_mask[(size_t)b * Sp + s] = mask;
    }
}

// __syncthreads() is s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier: in the one-node-per-thread loops it made every time step wait for
// the alpha / beta store it had just issued AND for the lp prefetch of four steps ahead -- a memory round trip per step on a chain of
// 1000 steps.  The exchange between the steps is LDS only: wait for the LDS operations, then the barrier; the prefetched values are
// waited for where they are used (the compiler counts vmcnt), the stores never.
#define ASR_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

}  // namespace ctc
}  // namespace asr
