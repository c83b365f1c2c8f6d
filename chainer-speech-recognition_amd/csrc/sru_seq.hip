// SRU as a sequence layer for gfx950: per-utterance lengths, one or two directions, a projected highway (k = 4) and a carried cell
// state per direction -- asr_sru_seq_fwd / asr_sru_seq_bwd; include/asr_hip.h states the semantics.  csrc/sru.hip (the reference's
// kernel pair, asr/nn/sru.py:17-191) is untouched and stays what nn.SRU runs.
//
// The design is that file's chunked scan: the cell recurrence  c <- f c + (1 - f) z  and its backward  gc <- f (gc + gct)  are linear
// in the state, so time is cut into NC chunks; a summary pass reduces every (direction, chunk, column) to (P, S) with
// state_out = P state_in + S, and an apply pass folds the summaries in front of a chunk into its entry state and runs the chunk.
// What is new:
//   lengths     a chunk covers [t0, min(t1, x_len[b])): one that lies wholly in the padding has no step, and its summary is never
//               folded (1 * c + 0 would turn a -0.0f state into +0.0f: cy == cx must hold on bits for x_len = 0); the chunk that
//               straddles x_len stops there.  The apply passes write the zeros of the padding (y; gU, gxh).
//   directions  one thread runs its chunk for both: first direction 1 (t descending; it writes C1 -- saved for the backward pass
//               anyway), then direction 0 (t ascending), which reads x once, reads C1[t] back (its own store, same address) and
//               writes y = h0 + h1: the sum in float32 registers, ONE rounding to 16 bits.  No per-direction h, no second pass over x.
//   backward    mirrored: direction 1 first (its gradient scan runs t ascending), then direction 0 (descending), which completes the
//               highway gradient gxh = gy ((1 - r0) + (1 - r1)) with one rounding.
//   k = 4       the highway input is U's fourth block (float32): x is not read at all, gU gets a fourth block gy (1 - r).
//   lanes       W = 2 adjacent features per lane (8-B float / 4-B packed 16-bit accesses) where D is even and the operands are aligned,
//               W = 1 otherwise; T < 32 (or too few steps per chunk) runs as NC = 1.  The same kernels serve all of it: a shape the
//               wide chunked form refuses changes template parameters, not code.
// No branch on data inside the time loops (the first step's previous state is an always-valid load followed by a select), bias
// gradients: registers -> LDS over the batch rows of a workgroup -> one atomic per (workgroup, column).
#include "common.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace sruseq {

__device__ __forceinline__ float fsig(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float ftanh(float x) {
    const float e = __expf(-2.0f * fabsf(x));
    return copysignf(1.0f - 2.0f * e * __builtin_amdgcn_rcpf(1.0f + e), x);
}

template <int W> struct Vec { float v[W]; };

template <int W> __device__ __forceinline__ Vec<W> ldf(const float* p) {
    Vec<W> r;
    if (W == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        r.v[0] = t.x; r.v[W - 1] = t.y;
    } else {
        r.v[0] = p[0];
    }
    return r;
}
template <int W> __device__ __forceinline__ void stf(float* p, const Vec<W>& a) {
    if (W == 2) *reinterpret_cast<float2*>(p) = make_float2(a.v[0], a.v[W - 1]);
    else p[0] = a.v[0];
}
template <int W> __device__ __forceinline__ Vec<W> ldh(const uint16_t* p) {
    Vec<W> r;
    if (W == 2) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
        r.v[0] = bf16_to_f32((uint16_t)(w & 0xffffu)); r.v[W - 1] = bf16_to_f32((uint16_t)(w >> 16));
    } else {
        r.v[0] = bf16_to_f32(p[0]);
    }
    return r;
}
template <int W> __device__ __forceinline__ void sth(uint16_t* p, const Vec<W>& a) {
    if (W == 2) *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(a.v[0], a.v[W - 1]);
    else p[0] = f32_to_bf16(a.v[0]);
}
template <int W> __device__ __forceinline__ Vec<W> splat(float x) {
    Vec<W> r;
#pragma unroll
    for (int j = 0; j < W; ++j) r.v[j] = x;
    return r;
}

constexpr int SX = 64, SY = 4;        // workgroup: 64 lanes of W features x 4 batch rows

struct Shape {
    int T, B, D, Tc, NC;
    const int* x_len;
};

// this thread's (chunk, batch row, first feature) and the valid steps [t0, v1) of its chunk; [pad0, t1) is the chunk's padding
struct Work {
    int b, d, k, len, t0, t1, v1, pad0;
    bool ok;
};
template <int W> __device__ __forceinline__ Work my_work(const Shape& s, int k) {
    Work w;
    w.d = W * (blockIdx.x * SX + threadIdx.x);
    w.b = blockIdx.y * SY + threadIdx.y;
    w.ok = w.d < s.D && w.b < s.B;
    w.k = k;
    const int bb = w.b < s.B ? w.b : 0;
    w.len = s.x_len ? min(max(s.x_len[bb], 0), s.T) : s.T;      // an entry outside 0 .. T is clamped
    w.t0 = k * s.Tc;
    w.t1 = min(s.T, w.t0 + s.Tc);
    w.v1 = min(w.t1, w.len);
    w.pad0 = max(w.t0, w.v1);
    return w;
}

// ------------------------------------------------------------------------------------------------------------------ forward
// (P, S) of (direction, chunk) = blockIdx.z: direction 0 needs chunks 0 .. NC - 2, direction 1 chunks 1 .. NC - 1
template <int W>
__global__ __launch_bounds__(SX * SY) void fwd_summary_kernel(const float* __restrict__ U, const float* __restrict__ bias, float* __restrict__ ws,
                                                              Shape s, int K, int ndir) {
    const int dir = blockIdx.z / s.NC;
    const Work w = my_work<W>(s, blockIdx.z % s.NC);
    if (!w.ok || (dir == 0 ? w.k == s.NC - 1 : w.k == 0)) return;
    const size_t us = (size_t)ndir * K * s.D;
    const Vec<W> bf = ldf<W>(bias + dir * 2 * s.D + w.d);
    const float* ub = U + (size_t)w.b * us + (size_t)dir * K * s.D + w.d;
    const int n = max(0, w.v1 - w.t0), step = dir == 0 ? 1 : -1;
    int t = dir == 0 ? w.t0 : w.v1 - 1;
    Vec<W> P = splat<W>(1.f), S = splat<W>(0.f);
#pragma unroll 4
    for (int i = 0; i < n; ++i, t += step) {
        const float* u = ub + (size_t)t * s.B * us;
        const Vec<W> z = ldf<W>(u), fp = ldf<W>(u + s.D);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float f = fsig(fp.v[j] + bf.v[j]);
            P.v[j] *= f;
            S.v[j] = f * (S.v[j] - z.v[j]) + z.v[j];
        }
    }
    const size_t plane = (size_t)ndir * s.NC * s.B * s.D, at = (((size_t)dir * s.NC + w.k) * s.B + w.b) * s.D + w.d;
    stf<W>(ws + at, P);
    stf<W>(ws + plane + at, S);
}

// state <- P state + S over the chunks `from`, `from + step`, ... (count of them) that hold a frame of the utterance
template <int W>
__device__ __forceinline__ void fold(Vec<W>& c, const float* __restrict__ ws, const Shape& s, int ndir, int dir, const Work& w, int from,
                                     int step, int count) {
    const size_t plane = (size_t)ndir * s.NC * s.B * s.D;
    for (int i = 0, kk = from; i < count; ++i, kk += step) {
        if (kk * s.Tc >= w.len) continue;           // wholly in the padding: the identity, on bits
        const size_t at = (((size_t)dir * s.NC + kk) * s.B + w.b) * s.D + w.d;
        const Vec<W> P = ldf<W>(ws + at), S = ldf<W>(ws + plane + at);
#pragma unroll
        for (int j = 0; j < W; ++j) c.v[j] = P.v[j] * c.v[j] + S.v[j];
    }
}

template <int W, int NDIR, int K, bool TANH>
__global__ __launch_bounds__(SX * SY) void fwd_apply_kernel(const uint16_t* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
                                                            const float* __restrict__ cx, const float* __restrict__ ws, uint16_t* __restrict__ y,
                                                            float* C, float* __restrict__ cy, Shape s) {
    const Work w = my_work<W>(s, blockIdx.z);
    if (!w.ok) return;
    const int D = s.D, B = s.B;
    const size_t us = (size_t)NDIR * K * D, col = (size_t)w.b * D + w.d, xs = (size_t)B * D;
    const float* ub = U + (size_t)w.b * us + w.d;
    if (NDIR == 2) {        // direction 1 over the chunk, t descending: C1
        const Vec<W> bf = ldf<W>(bias + 2 * D + w.d);
        Vec<W> c = cx ? ldf<W>(cx + xs + col) : splat<W>(0.f);
        fold<W>(c, ws, s, NDIR, 1, w, s.NC - 1, -1, s.NC - 1 - w.k);
        float* C1 = C + (size_t)s.T * xs + col;
#pragma unroll 4
        for (int t = w.v1 - 1; t >= w.t0; --t) {
            const float* u = ub + (size_t)t * B * us + K * D;
            const Vec<W> z = ldf<W>(u), fp = ldf<W>(u + D);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float f = fsig(fp.v[j] + bf.v[j]);
                c.v[j] = f * (c.v[j] - z.v[j]) + z.v[j];
            }
            stf<W>(C1 + (size_t)t * xs, c);
        }
        if (w.k == 0) stf<W>(cy + xs + col, c);
    }
    const Vec<W> bf = ldf<W>(bias + w.d), br = ldf<W>(bias + D + w.d);
    const Vec<W> br1 = NDIR == 2 ? ldf<W>(bias + 3 * D + w.d) : splat<W>(0.f);
    Vec<W> c = cx ? ldf<W>(cx + col) : splat<W>(0.f);
    fold<W>(c, ws, s, NDIR, 0, w, 0, 1, w.k);
#pragma unroll 4
    for (int t = w.t0; t < w.v1; ++t) {
        const float* u = ub + (size_t)t * B * us;
        const size_t row = (size_t)t * xs + col;
        const Vec<W> z = ldf<W>(u), fp = ldf<W>(u + D), rp = ldf<W>(u + 2 * D);
        const Vec<W> xt = K == 3 ? ldh<W>(x + row) : ldf<W>(u + 3 * D);
        Vec<W> rp1 = splat<W>(0.f), c1 = splat<W>(0.f), xt1 = xt;
        if (NDIR == 2) {
            rp1 = ldf<W>(u + K * D + 2 * D);
            c1 = ldf<W>(C + (size_t)s.T * xs + row);
            if (K == 4) xt1 = ldf<W>(u + K * D + 3 * D);
        }
        Vec<W> h;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float f = fsig(fp.v[j] + bf.v[j]), r = fsig(rp.v[j] + br.v[j]);
            c.v[j] = f * (c.v[j] - z.v[j]) + z.v[j];
            const float g = TANH ? ftanh(c.v[j]) : c.v[j];
            h.v[j] = r * (g - xt.v[j]) + xt.v[j];
            if (NDIR == 2) {
                const float r1 = fsig(rp1.v[j] + br1.v[j]);
                const float g1 = TANH ? ftanh(c1.v[j]) : c1.v[j];
                h.v[j] += r1 * (g1 - xt1.v[j]) + xt1.v[j];
            }
        }
        stf<W>(C + row, c);
        sth<W>(y + row, h);
    }
    // the state after the utterance's last own frame: the chunk that holds frame len - 1 (len = 0: chunk 0 hands cx on)
    if (w.len == 0 ? w.k == 0 : (w.t0 < w.len && w.len <= w.t1)) stf<W>(cy + col, c);
    const Vec<W> zero = splat<W>(0.f);
    for (int t = w.pad0; t < w.t1; ++t) sth<W>(y + (size_t)t * xs + col, zero);
}

// ------------------------------------------------------------------------------------------------------------------ backward
// gc leaving a chunk = P gc_in + S.  Direction 0 (gradient scan t descending) needs chunks 1 .. NC - 1, direction 1 chunks 0 .. NC - 2.
template <int W, bool TANH>
__global__ __launch_bounds__(SX * SY) void bwd_summary_kernel(const float* __restrict__ U, const float* __restrict__ bias, const float* __restrict__ C,
                                                              const uint16_t* __restrict__ gy, float* __restrict__ ws, Shape s, int K, int ndir) {
    const int dir = blockIdx.z / s.NC;
    const Work w = my_work<W>(s, blockIdx.z % s.NC);
    if (!w.ok || (dir == 0 ? w.k == 0 : w.k == s.NC - 1)) return;
    const int D = s.D;
    const size_t us = (size_t)ndir * K * D, xs = (size_t)s.B * D, col = (size_t)w.b * D + w.d;
    const Vec<W> bf = ldf<W>(bias + dir * 2 * D + w.d), br = ldf<W>(bias + dir * 2 * D + D + w.d);
    const float* ub = U + (size_t)w.b * us + (size_t)dir * K * D + w.d;
    const float* Cd = C + (size_t)dir * s.T * xs + col;
    const int n = max(0, w.v1 - w.t0), step = dir == 0 ? -1 : 1;
    int t = dir == 0 ? w.v1 - 1 : w.t0;
    Vec<W> P = splat<W>(1.f), S = splat<W>(0.f);
#pragma unroll 4
    for (int i = 0; i < n; ++i, t += step) {
        const float* u = ub + (size_t)t * s.B * us;
        const Vec<W> fp = ldf<W>(u + D), rp = ldf<W>(u + 2 * D), c = ldf<W>(Cd + (size_t)t * xs), gh = ldh<W>(gy + (size_t)t * xs + col);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float f = fsig(fp.v[j] + bf.v[j]), r = fsig(rp.v[j] + br.v[j]);
            const float g = TANH ? ftanh(c.v[j]) : c.v[j];
            const float gct = gh.v[j] * r * (TANH ? (1.f - g * g) : 1.f);
            S.v[j] = (gct + S.v[j]) * f;
            P.v[j] *= f;
        }
    }
    const size_t plane = (size_t)ndir * s.NC * s.B * D, at = (((size_t)dir * s.NC + w.k) * s.B + w.b) * D + w.d;
    stf<W>(ws + at, P);
    stf<W>(ws + plane + at, S);
}

// one direction of one chunk: gU's blocks of that direction, its bias sums and -- direction 0 -- the highway gradient of both
template <int W, int NDIR, int K, bool TANH, int DIR>
__device__ __forceinline__ void bwd_direction(const uint16_t* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
                                              const float* __restrict__ C, const float* __restrict__ cx, const uint16_t* __restrict__ gy,
                                              const float* __restrict__ dcy, const float* __restrict__ ws, uint16_t* __restrict__ gU,
                                              uint16_t* __restrict__ gxh, float* __restrict__ dcx, const Shape& s, const Work& w, Vec<W>& sbf,
                                              Vec<W>& sbr) {
    const int D = s.D, B = s.B;
    const size_t us = (size_t)NDIR * K * D, xs = (size_t)B * D, col = (size_t)w.b * D + w.d;
    const Vec<W> bf = ldf<W>(bias + DIR * 2 * D + w.d), br = ldf<W>(bias + DIR * 2 * D + D + w.d);
    const Vec<W> br1 = (NDIR == 2 && DIR == 0 && K == 3) ? ldf<W>(bias + 3 * D + w.d) : splat<W>(0.f);
    const Vec<W> cfirst = cx ? ldf<W>(cx + DIR * xs + col) : splat<W>(0.f);
    Vec<W> gc = dcy ? ldf<W>(dcy + DIR * xs + col) : splat<W>(0.f);
    if (DIR == 0) fold<W>(gc, ws, s, NDIR, 0, w, s.NC - 1, -1, s.NC - 1 - w.k);
    else fold<W>(gc, ws, s, NDIR, 1, w, 0, 1, w.k);
    const float* ub = U + (size_t)w.b * us + (size_t)DIR * K * D + w.d;
    uint16_t* gub = gU + (size_t)w.b * us + (size_t)DIR * K * D + w.d;
    const float* Cd = C + (size_t)DIR * s.T * xs + col;
    const int n = max(0, w.v1 - w.t0), step = DIR == 0 ? -1 : 1;
    int t = DIR == 0 ? w.v1 - 1 : w.t0;
    Vec<W> c = n > 0 ? ldf<W>(Cd + (size_t)t * xs) : splat<W>(0.f);
#pragma unroll 2
    for (int i = 0; i < n; ++i, t += step) {
        // the state this step started from: the scan's previous frame, or cx at the direction's first frame (an always-valid load,
        // then a select: no branch in the loop)
        const bool first = DIR == 0 ? t == 0 : t == w.len - 1;
        Vec<W> cp = ldf<W>(Cd + (size_t)(first ? t : t + step) * xs);
        const float* u = ub + (size_t)t * B * us;
        uint16_t* gu = gub + (size_t)t * B * us;
        const size_t row = (size_t)t * xs + col;
        const Vec<W> z = ldf<W>(u), fp = ldf<W>(u + D), rp = ldf<W>(u + 2 * D), gh = ldh<W>(gy + row);
        const Vec<W> xt = K == 3 ? ldh<W>(x + row) : ldf<W>(u + 3 * D);
        Vec<W> rp1 = splat<W>(0.f);
        if (NDIR == 2 && DIR == 0 && K == 3) rp1 = ldf<W>(u + K * D + 2 * D);
        Vec<W> gz, gf, gr, gp;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (first) cp.v[j] = cfirst.v[j];
            const float f = fsig(fp.v[j] + bf.v[j]), r = fsig(rp.v[j] + br.v[j]);
            const float g = TANH ? ftanh(c.v[j]) : c.v[j];
            gr.v[j] = gh.v[j] * (g - xt.v[j]) * (1.f - r) * r;
            const float gct = gh.v[j] * r * (TANH ? (1.f - g * g) : 1.f);
            const float tx = gct + gc.v[j];
            gf.v[j] = tx * (cp.v[j] - z.v[j]) * (1.f - f) * f;
            gz.v[j] = tx * (1.f - f);
            gp.v[j] = gh.v[j] * (1.f - r);
            if (NDIR == 2 && DIR == 0 && K == 3) gp.v[j] += gh.v[j] * (1.f - fsig(rp1.v[j] + br1.v[j]));
            gc.v[j] = tx * f;
            sbf.v[j] += gf.v[j];
            sbr.v[j] += gr.v[j];
        }
        sth<W>(gu, gz);
        sth<W>(gu + D, gf);
        sth<W>(gu + 2 * D, gr);
        if (K == 4) sth<W>(gu + 3 * D, gp);
        if (K == 3 && DIR == 0) sth<W>(gxh + row, gp);
        c = cp;
    }
    // the gradient of cx leaves through the chunk that holds the direction's first frame (len = 0: chunk 0 hands dcy on)
    const bool owner = DIR == 0 ? w.k == 0 : (w.len == 0 ? w.k == 0 : (w.t0 < w.len && w.len <= w.t1));
    if (dcx && owner) stf<W>(dcx + DIR * xs + col, gc);
}

template <int W, int NDIR, int K, bool TANH>
__global__ __launch_bounds__(SX * SY) void bwd_apply_kernel(const uint16_t* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
                                                            const float* __restrict__ C, const float* __restrict__ cx, const uint16_t* __restrict__ gy,
                                                            const float* __restrict__ dcy, const float* __restrict__ ws, uint16_t* __restrict__ gU,
                                                            uint16_t* __restrict__ gxh, float* __restrict__ gbias, float* __restrict__ dcx, Shape s) {
    __shared__ float red[SY][NDIR * 2][W * SX];
    const Work w = my_work<W>(s, blockIdx.z);
    Vec<W> sb[NDIR * 2];
#pragma unroll
    for (int i = 0; i < NDIR * 2; ++i) sb[i] = splat<W>(0.f);
    if (w.ok) {
        if (NDIR == 2) bwd_direction<W, NDIR, K, TANH, NDIR - 1>(x, U, bias, C, cx, gy, dcy, ws, gU, gxh, dcx, s, w, sb[NDIR * 2 - 2], sb[NDIR * 2 - 1]);
        bwd_direction<W, NDIR, K, TANH, 0>(x, U, bias, C, cx, gy, dcy, ws, gU, gxh, dcx, s, w, sb[0], sb[1]);
        const size_t us = (size_t)NDIR * K * s.D, xs = (size_t)s.B * s.D, col = (size_t)w.b * s.D + w.d;
        const Vec<W> zero = splat<W>(0.f);
        for (int t = w.pad0; t < w.t1; ++t) {       // the padding receives and passes no gradient
            uint16_t* gu = gU + ((size_t)t * s.B + w.b) * us + w.d;
#pragma unroll
            for (int blk = 0; blk < NDIR * K; ++blk) sth<W>(gu + blk * s.D, zero);
            if (K == 3) sth<W>(gxh + (size_t)t * xs + col, zero);
        }
    }
#pragma unroll
    for (int i = 0; i < NDIR * 2; ++i)
#pragma unroll
        for (int j = 0; j < W; ++j) red[threadIdx.y][i][W * threadIdx.x + j] = sb[i].v[j];
    __syncthreads();
    if (threadIdx.y < NDIR * 2) {       // row i of the workgroup folds sum i (direction i / 2, b_f or b_r) of the SY batch rows
        const int which = threadIdx.y;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int d = W * (blockIdx.x * SX + threadIdx.x) + j;
            if (d < s.D) {
                float a = 0.f;
#pragma unroll
                for (int yy = 0; yy < SY; ++yy) a += red[yy][which][W * threadIdx.x + j];
                atomicAdd(gbias + (size_t)which * s.D + d, a);      // (ndir, 2, D): which = 2 dir + gate
            }
        }
    }
}

}  // namespace sruseq
}  // namespace asr

using namespace asr;
using namespace asr::sruseq;

// number of time chunks: enough waves for >= 8 per CU, chunks of at least 16 steps; 1 = the whole sequence in one chunk, no summaries
static int seq_chunks(int T, int B, int D) {
    if (T < 32) return 1;
    const long long waves = ((long long)B * ((D + 1) / 2) + 63) / 64;
    long long nc = (2048 + waves - 1) / waves;
    if (nc > 32) nc = 32;
    if (nc > T / 16) nc = T / 16;
    if (nc < 2) return 1;
    const int Tc = (int)((T + nc - 1) / nc);
    return (T + Tc - 1) / Tc;           // no empty chunk at the end
}

extern "C" size_t asr_sru_seq_ws_bytes(int T, int B, int D, int ndir) {
    if (T <= 0 || B <= 0 || D <= 0 || ndir < 1 || ndir > 2) return 0;
    const int nc = seq_chunks(T, B, D);
    return nc > 1 ? (size_t)2 * ndir * nc * B * D * sizeof(float) : 0;
}

static bool al(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

#define SEQ_PICK4(KERNEL, W, ...)                                                                          \
    do {                                                                                                   \
        if (ndir == 1 && k == 3 && use_tanh) hipLaunchKernelGGL((KERNEL<W, 1, 3, true>), __VA_ARGS__);     \
        else if (ndir == 1 && k == 3) hipLaunchKernelGGL((KERNEL<W, 1, 3, false>), __VA_ARGS__);           \
        else if (ndir == 1 && use_tanh) hipLaunchKernelGGL((KERNEL<W, 1, 4, true>), __VA_ARGS__);          \
        else if (ndir == 1) hipLaunchKernelGGL((KERNEL<W, 1, 4, false>), __VA_ARGS__);                     \
        else if (k == 3 && use_tanh) hipLaunchKernelGGL((KERNEL<W, 2, 3, true>), __VA_ARGS__);             \
        else if (k == 3) hipLaunchKernelGGL((KERNEL<W, 2, 3, false>), __VA_ARGS__);                        \
        else if (use_tanh) hipLaunchKernelGGL((KERNEL<W, 2, 4, true>), __VA_ARGS__);                       \
        else hipLaunchKernelGGL((KERNEL<W, 2, 4, false>), __VA_ARGS__);                                    \
    } while (0)

extern "C" int asr_sru_seq_fwd(void* stream, const void* x_bf16, const float* U, const float* bias, const float* cx, const int* x_len,
                               void* y_bf16, float* C, float* cy, int T, int B, int D, int k, int ndir, int use_tanh, void* ws,
                               size_t ws_bytes) {
    if (ASR_ACT_IS_F16) return ASR_ERR_UNSUPPORTED;      // (bfloat16 semantics of the recurrent entries: common.hpp)
    if (T <= 0 || B <= 0 || D <= 0 || (k != 3 && k != 4) || (ndir != 1 && ndir != 2)) return ASR_ERR_BAD_ARG;
    if (!U || !bias || !y_bf16 || !C || !cy || (k == 3 && !x_bf16)) return ASR_ERR_BAD_ARG;
    const int nc = seq_chunks(T, B, D);
    if (nc > 1 && (!ws || ws_bytes < asr_sru_seq_ws_bytes(T, B, D, ndir) || !al(ws, 4))) return ASR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Shape s = {T, B, D, (T + nc - 1) / nc, nc, x_len};
    const uint16_t* x = (const uint16_t*)x_bf16;
    uint16_t* y = (uint16_t*)y_bf16;
    float* wsf = (float*)ws;
    const bool wide = !(D & 1) && al(U, 8) && al(bias, 8) && al(C, 8) && al(cy, 8) && al(cx, 8) && al(ws, 8) && al(x, 4) && al(y, 4);
    const int lanes = wide ? D / 2 : D;
    const dim3 block(SX, SY), grid((lanes + SX - 1) / SX, (B + SY - 1) / SY, nc), sgrid(grid.x, grid.y, nc * ndir);
    if (wide) {
        if (nc > 1) hipLaunchKernelGGL(fwd_summary_kernel<2>, sgrid, block, 0, st, U, bias, wsf, s, k, ndir);
        SEQ_PICK4(fwd_apply_kernel, 2, grid, block, 0, st, x, U, bias, cx, (const float*)wsf, y, C, cy, s);
    } else {
        if (nc > 1) hipLaunchKernelGGL(fwd_summary_kernel<1>, sgrid, block, 0, st, U, bias, wsf, s, k, ndir);
        SEQ_PICK4(fwd_apply_kernel, 1, grid, block, 0, st, x, U, bias, cx, (const float*)wsf, y, C, cy, s);
    }
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_sru_seq_bwd(void* stream, const void* x_bf16, const float* U, const float* bias, const float* C, const float* cx,
                               const int* x_len, const void* gy_bf16, const float* dcy, void* gU_bf16, void* gxh_bf16, float* gbias,
                               float* dcx, int T, int B, int D, int k, int ndir, int use_tanh, void* ws, size_t ws_bytes) {
    if (ASR_ACT_IS_F16) return ASR_ERR_UNSUPPORTED;      // (bfloat16 semantics of the recurrent entries: common.hpp)
    if (T <= 0 || B <= 0 || D <= 0 || (k != 3 && k != 4) || (ndir != 1 && ndir != 2)) return ASR_ERR_BAD_ARG;
    if (!U || !bias || !C || !gy_bf16 || !gU_bf16 || !gbias || (k == 3 && (!x_bf16 || !gxh_bf16))) return ASR_ERR_BAD_ARG;
    const int nc = seq_chunks(T, B, D);
    if (nc > 1 && (!ws || ws_bytes < asr_sru_seq_ws_bytes(T, B, D, ndir) || !al(ws, 4))) return ASR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Shape s = {T, B, D, (T + nc - 1) / nc, nc, x_len};
    const uint16_t *x = (const uint16_t*)x_bf16, *gy = (const uint16_t*)gy_bf16;
    uint16_t *gU = (uint16_t*)gU_bf16, *gxh = (uint16_t*)gxh_bf16;
    float* wsf = (float*)ws;
    const bool wide = !(D & 1) && al(U, 8) && al(bias, 8) && al(C, 8) && al(cx, 8) && al(dcy, 8) && al(dcx, 8) && al(ws, 8) && al(x, 4) &&
                      al(gy, 4) && al(gU, 4) && al(gxh, 4);
    const int lanes = wide ? D / 2 : D;
    const dim3 block(SX, SY), grid((lanes + SX - 1) / SX, (B + SY - 1) / SY, nc), sgrid(grid.x, grid.y, nc * ndir);
    if (wide) {
        if (nc > 1) {
            if (use_tanh) hipLaunchKernelGGL((bwd_summary_kernel<2, true>), sgrid, block, 0, st, U, bias, C, gy, wsf, s, k, ndir);
            else hipLaunchKernelGGL((bwd_summary_kernel<2, false>), sgrid, block, 0, st, U, bias, C, gy, wsf, s, k, ndir);
        }
        SEQ_PICK4(bwd_apply_kernel, 2, grid, block, 0, st, x, U, bias, C, cx, gy, dcy, (const float*)wsf, gU, gxh, gbias, dcx, s);
    } else {
        if (nc > 1) {
            if (use_tanh) hipLaunchKernelGGL((bwd_summary_kernel<1, true>), sgrid, block, 0, st, U, bias, C, gy, wsf, s, k, ndir);
            else hipLaunchKernelGGL((bwd_summary_kernel<1, false>), sgrid, block, 0, st, U, bias, C, gy, wsf, s, k, ndir);
        }
        SEQ_PICK4(bwd_apply_kernel, 1, grid, block, 0, st, x, U, bias, C, cx, gy, dcy, (const float*)wsf, gU, gxh, gbias, dcx, s);
    }
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
