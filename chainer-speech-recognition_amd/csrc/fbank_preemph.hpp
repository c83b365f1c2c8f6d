// The pre-emphasis of the log-mel front end, shared by the one-shot kernels (fbank.hip) and the streaming ones (fbank_stream.hip): both
// must form a sample with the same instructions, or a stream would not reproduce the one-shot features bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace asr {
namespace fbank {

// y[n] = x[n] - c x[n - 1] with the coefficient to float64 precision, as its float32 head and tail in two fused multiply-adds: on a slowly
// varying signal the difference is a small fraction of its terms (1/32 of them on a constant), and the rounding of 0.97 to float32 (3e-8)
// alone then put 1e-6 on every sample -- 2e-6 on the power spectrum of a constant, fifty times what float32 arithmetic costs there
// (tests/test_fbank_edges_gpu.py: dc)
__device__ __forceinline__ float preemphasised(float x, float prev, double c) {
    const float hi = (float)c, lo = (float)(c - (double)hi);
    return fmaf(-lo, prev, fmaf(-hi, prev, x));
}

}  // namespace fbank
}  // namespace asr
