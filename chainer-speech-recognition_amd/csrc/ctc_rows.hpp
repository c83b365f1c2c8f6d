// The row reduction that the forced alignment (csrc/ctc_align.hip: gather_kernel) and the keyword search (csrc/ctc_kws.hip:
// rows_kernel) share: the f32 maximum of one row of logits and the sum of exp(x - max) over it, by one workgroup.  ONE copy, so that
// "lse is the same f32 value in both" is a property of the code: the same loops (float4 where the row allows it), the same block
// reductions, the same order of additions.
#pragma once
#include "common.hpp"

namespace asr {
namespace ctc {

// x: the row (V floats); scratch: 32 floats of LDS; every thread of the workgroup calls it and gets the same m and sum back.
// lse = m + __logf(sum).
__device__ __forceinline__ void row_max_sumexp(const float* __restrict__ x, int V, float* scratch, float& m_out, float& sum_out) {
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
    m_out = m;
    sum_out = block_sum(sum, scratch);
}

}  // namespace ctc
}  // namespace asr
