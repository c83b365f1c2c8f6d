// The log-mel front end fed chunk by chunk (asr.fft.FeatureStream; semantics: include/asr_hip.h).  Three launches per chunk:
//   fbank_stream_push_kernel    per slot: [pending pre-emphasised samples | the chunk's samples, pre-emphasised] -> one float32 window row,
//                               its length, the number k of complete frames in it, and the new pending part
//   asr_specgram_bands          (fbank.hip, unchanged) on the window rows with a zero coefficient: k log-mel rows per slot, written behind
//                               the slot's four carried rows
//   fbank_stream_deltas_kernel  per slot: [carried rows | new rows] -> the feature frames that are now complete, the padding, the new
//                               carried rows and the counters
// One workgroup per slot in both kernels: each stages what it reads of the slot's state in LDS, then writes after a barrier, so no
// launch reads a global location another workgroup of the same launch writes.  The data is tiny (a 640 ms chunk of 32 slots is 0.65 MB):
// the cost is the three launches.
#include "common.hpp"
#include "fbank_preemph.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace fbank {
namespace {

constexpr int kMeta = ASR_FBANK_STREAM_META;              // ints per slot: pending samples, a predecessor exists, log-mel frames, feature frames, ended
constexpr int kStreamFrames = ASR_FBANK_STREAM_MAX_FRAMES;
constexpr int kStreamFilt = ASR_FBANK_STREAM_MAX_FILT;
constexpr int kCarry = 4;                                 // log-mel rows kept: frame t needs rows t - 2 .. t + 2
constexpr int kMaxLen = 1024;                             // frame_len <= nfft <= 1024 (asr_specgram)

__host__ __device__ inline int frames_of(int samples, int frame_step) { return samples > 0 ? 1 + (samples - 1) / frame_step : 0; }

template <typename SigT>
__global__ __launch_bounds__(256) void fbank_stream_push_kernel(const SigT* __restrict__ chunk, long long chunk_pitch, int Nc,
                                                                const int* __restrict__ n, const int* __restrict__ flush, float* pend,
                                                                int pend_pitch, float* last, int* meta, float* __restrict__ window,
                                                                long long win_pitch, int* __restrict__ wlen, int* __restrict__ kout,
                                                                int L, int S, double preemph) {
    __shared__ float sp[kMaxLen];
    __shared__ int smeta[kMeta];
    __shared__ float slast;
    const int b = blockIdx.x, tid = threadIdx.x;
    int* mt = meta + (size_t)b * kMeta;
    float* pd = pend + (size_t)b * pend_pitch;
    const int m = min(max(mt[0], 0), L - 1);                     // (consumed by every lane before the barrier: the loop bound below)
    for (int i = tid; i < m; i += 256) sp[i] = pd[i];
    if (tid < kMeta) smeta[tid] = mt[tid];
    if (tid == 0) slast = last[b];
    __syncthreads();                    // the slot's state is in LDS: nothing below reads it from global memory again
    const int has = smeta[1], c = smeta[2], ended = smeta[4];
    const float prev0 = slast;
    const bool fl = flush != nullptr;
    const bool touched = fl ? flush[b] != 0 : true;
    const int nb = fl ? 0 : (n ? min(max(n[b], 0), Nc) : Nc);
    const int wl = m + nb;
    int k;
    if (fl) k = (touched && (c == 0 || m > L - S)) ? 1 : 0;      // the pending samples make one last zero-padded frame
    else k = wl < L ? 0 : 1 + (wl - L) / S;
    if (tid == 0) { wlen[b] = wl; kout[b] = k; }
    if (!touched || (!fl && nb == 0)) return;                    // an untouched slot keeps every byte of its state
    const int p0 = fl ? wl : k * S;                              // the window from here on stays pending (a flush leaves nothing)
    const int wp = (int)win_pitch;
    const int fill = min(wp, ((wl + 3) & ~3) + 4);               // zeros behind the samples: the transform loads four samples past wl
    float* wr = window + (size_t)b * win_pitch;
    const SigT* ch = chunk + (size_t)b * chunk_pitch;
    for (int i4 = 4 * tid; i4 < fill; i4 += 1024) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i4 + u;
            float y = 0.f;
            if (i < m) y = sp[i];
            else if (i < wl) {
                const int j = i - m;
                const float x = (float)ch[j];
                const float prev = j > 0 ? (float)ch[j - 1] : prev0;
                y = (j == 0 && !has) ? x : preemphasised(x, prev, preemph);      // (the very first sample after a reset stays raw)
            }
            v[u] = y;
            if (i >= p0 && i < wl) pd[i - p0] = y;
        }
        *reinterpret_cast<float4*>(wr + i4) = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (tid == 0) {
        mt[0] = wl - p0;
        mt[1] = fl ? 0 : 1;
        if (!fl) {
            last[b] = (float)ch[nb - 1];
            if (ended) { mt[3] = 0; mt[4] = 0; }                 // fed again after a flush: the finished utterance's count goes
        }
    }
}

// x[b][c][m][col] for the feature frames e0 + col, e0 = max(0, c - 2), col < max(0, c + k - 2) - e0; the padding beyond; the carried rows
__global__ __launch_bounds__(256) void fbank_stream_deltas_kernel(float* logmel, const int* __restrict__ k, const int* __restrict__ flush,
                                                                  int* meta, int Fmax, int nfilt, int Tc, const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv, float* __restrict__ out,
                                                                  int* __restrict__ lengths) {
    __shared__ float tile[(kCarry + kStreamFrames) * (kStreamFilt + 1)];
    __shared__ float smean[3 * kStreamFilt], sstd[3 * kStreamFilt];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (mean && tid < 3 * nfilt) { smean[tid] = mean[tid]; sstd[tid] = stdv[tid]; }
    __shared__ int scount[2];
    int* mt = meta + (size_t)b * kMeta;
    if (tid == 0) { scount[0] = mt[2]; scount[1] = mt[3]; }
    __syncthreads();                    // the counters are read once, by the lane that writes them at the end
    const int c = max(scount[0], 0);
    const bool fl = flush && flush[b];
    const int kb = min(max(k[b], 0), min(Fmax - kCarry, kStreamFrames));
    const int r = min(kCarry, c), pitch = nfilt | 1;
    float* lm = logmel + (size_t)b * Fmax * nfilt;
    const int lo = kCarry - r;
    if (kb > 0)
        for (int i = tid; i < (r + kb) * nfilt; i += 256) {
            const int rr = lo + i / nfilt, cc = i % nfilt;
            tile[rr * pitch + cc] = lm[(size_t)rr * nfilt + cc];
        }
    __syncthreads();                    // rows c - r .. c + kb - 1 are in LDS at tile rows q - c + 4
    const int e0 = max(0, c - 2), cnt = min(max(0, c + kb - 2) - e0, Tc);
    const int tl = tid & 31;
    auto cl = [](int q) -> int { return q < 0 ? 0 : q; };       // the left edge repeats frame 0; the right edge is never reached
    auto row = [&](int q) -> int { return (cl(q) - c + kCarry) * pitch; };
    for (int t0 = 0; t0 < Tc; t0 += 32) {
        const int col = t0 + tl;
        if (col >= Tc) continue;
        const bool live = col < cnt;
        const int t = e0 + col;
        const int c0 = cl(t - 1), c1 = cl(t), c2 = cl(t + 1);
        const int r_t = row(c1);
        const int r_d0a = row(c0 + 1), r_d0b = row(c0 - 1);      // dl(t - 1)
        const int r_d1a = row(c1 + 1), r_d1b = row(c1 - 1);      // dl(t)
        const int r_d2a = row(c2 + 1), r_d2b = row(c2 - 1);      // dl(t + 1)
        for (int m = tid >> 5; m < nfilt; m += 8) {
            float v0 = 0.f, v1 = 0.f, v2 = 0.f;
            if (live) {                 // the expressions of deltas_tile_kernel (fbank.hip)
                v0 = tile[r_t + m];
                v1 = (tile[r_d1a + m] - tile[r_d1b + m]) * 0.5f;
                v2 = ((tile[r_d2a + m] - tile[r_d2b + m]) * 0.5f - (tile[r_d0a + m] - tile[r_d0b + m]) * 0.5f) * 0.5f;
            }
            if (mean) {
                v0 = (v0 - smean[m]) / sstd[m];
                v1 = (v1 - smean[nfilt + m]) / sstd[nfilt + m];
                v2 = (v2 - smean[2 * nfilt + m]) / sstd[2 * nfilt + m];
            }
            float* o = out + ((size_t)b * 3 * nfilt + m) * Tc + col;
            o[0] = v0;
            o[(size_t)nfilt * Tc] = v1;
            o[(size_t)2 * nfilt * Tc] = v2;
        }
    }
    if (kb > 0 && !fl) {                // the last min(4, c + kb) rows, right-aligned in the slot's first four
        const int c2 = c + kb, r2 = min(kCarry, c2);
        for (int i = tid; i < r2 * nfilt; i += 256) {
            const int rr = i / nfilt, cc = i % nfilt;
            lm[(size_t)(kCarry - r2 + rr) * nfilt + cc] = tile[(c2 - r2 + rr - c + kCarry) * pitch + cc];
        }
    }
    if (tid == 0) {
        lengths[b] = cnt;
        if (kb > 0 || fl) {
            mt[2] = fl ? 0 : c + kb;
            mt[3] = scount[1] + cnt;
            if (fl) mt[4] = 1;
        }
    }
}

__global__ void fbank_stream_reset_kernel(int* __restrict__ meta, const int* __restrict__ mask, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * kMeta) return;
    if (mask && !mask[i / kMeta]) return;
    meta[i] = 0;
}

}  // namespace
}  // namespace fbank
}  // namespace asr

using namespace asr;
using namespace asr::fbank;

extern "C" int asr_fbank_stream_push(void* stream, const void* chunk, int chunk_is_f32, long long chunk_pitch, int Nc, const int32_t* n,
                                     const int32_t* flush, float* pend, int pend_pitch, float* last, int32_t* meta, float* window,
                                     long long win_pitch, int32_t* wlen, int32_t* k, int B, int frame_len, int frame_step, double preemph) {
    if (!pend || !last || !meta || !window || !wlen || !k || B <= 0 || Nc < 0 || frame_len <= 0 || frame_step <= 0) return ASR_ERR_BAD_ARG;
    if (flush ? Nc != 0 : (Nc > 0 && (!chunk || chunk_pitch < Nc))) return ASR_ERR_BAD_ARG;
    if (frame_len > kMaxLen || frame_step > frame_len || frames_of(Nc, frame_step) > kStreamFrames) return ASR_ERR_UNSUPPORTED;
    if (pend_pitch < frame_len || win_pitch < ((frame_len - 1 + Nc + 3) & ~3) + 4 || (win_pitch & 3) != 0 || (((uintptr_t)window) & 15) != 0)
        return ASR_ERR_WORKSPACE;
    if (!flush && Nc == 0) return ASR_OK;
    hipStream_t s = (hipStream_t)stream;
    if (chunk_is_f32)
        hipLaunchKernelGGL(fbank_stream_push_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)chunk, chunk_pitch, Nc, n, flush, pend,
                           pend_pitch, last, meta, window, win_pitch, wlen, k, frame_len, frame_step, preemph);
    else
        hipLaunchKernelGGL(fbank_stream_push_kernel<short>, dim3(B), dim3(256), 0, s, (const short*)chunk, chunk_pitch, Nc, n, flush, pend,
                           pend_pitch, last, meta, window, win_pitch, wlen, k, frame_len, frame_step, preemph);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_fbank_stream_deltas(void* stream, float* logmel, const int32_t* k, const int32_t* flush, int32_t* meta, int B, int Fmax,
                                       int nfilt, int Tc, const float* mean, const float* stdv, float* out, int32_t* lengths) {
    if (!logmel || !k || !meta || !out || !lengths || B <= 0 || nfilt <= 0 || Tc <= 0 || Fmax <= kCarry) return ASR_ERR_BAD_ARG;
    if ((mean == nullptr) != (stdv == nullptr)) return ASR_ERR_BAD_ARG;
    if (nfilt > kStreamFilt || Tc > kStreamFrames) return ASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(fbank_stream_deltas_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logmel, k, flush, meta, Fmax, nfilt, Tc, mean,
                       stdv, out, lengths);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_fbank_stream_reset(void* stream, int32_t* meta, const int32_t* mask, int B) {
    if (!meta || B <= 0) return ASR_ERR_BAD_ARG;
    hipLaunchKernelGGL(fbank_stream_reset_kernel, dim3(cdiv((long long)B * kMeta, 256)), dim3(256), 0, (hipStream_t)stream, meta, mask, B);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
