// CTC and Gram-CTC forced (Viterbi) alignment for gfx950: given logits and a transcript, which frames belong to which token.
//
// The max-product twin of the loss (csrc/ctc.hip) on the SAME lattice (csrc/ctc_lattice.hpp: prep_kernel).  The reference has no
// aligner; its run/gram_ctc/cnn/refine.py:94-107 ("usage of grams") asks which grams the model uses with a per-frame argmax that
// ignores the transcript -- the best path through the Gram-CTC lattice is the transcript-conditioned answer.
//
// Three kernels, all on the caller's stream:
//   prep    (B workgroups)     path labels + per-node edge bitmask (shared with the loss)
//   gather  (T*B workgroups)   log-sum-exp of every logit row (f32, formed as the loss's rows pass forms it) and the RAW f32 logit
//                              of every path node                                                         [HBM: read T*B*V]
//   align   (B workgroups)     per utterance, state in LDS:
//       sweep       cur[s] = max_j prev[s - k_j] + (double)logit[t][s]: float64 on the raw logits, ONE addition per step and nothing
//                   else on the chain (the row's log-sum-exp is the same for every node of a frame, so it cannot change the path; it
//                   only enters the scores).  A NumPy float64 restatement therefore reproduces every decision bit for bit.
//                   Ties: the smallest diagonal offset wins; among equal final nodes the largest node index.
//                   The winning edge class of every (t, s) is kept as bit planes, 2 (CTC) or 3 (Gram-CTC) bits per node: one
//                   wave-wide ballot per plane gives the 64 nodes of a wave as one 64-bit word, written to LDS by one lane.
//       back-trace  one wave walks the planes IN LDS (a dependent chain of LDS reads, not of T global round trips), and a whole run
//                   of frames on one node per link of the chain: 64 lanes read the classes of 64 frames at once.  Frames are
//                   kept in blocks of TC: a block that is full is spilled to the workspace by the whole workgroup and staged back,
//                   last block first, for the walk; with T <= TC (CTC Lmax 120 / Gram-CTC Lmax 120 at T = 1000) nothing is spilled.
//       spans       workgroup scans over the frames (token starts; float64 prefix of the frames' log-probabilities): tokens, label
//                   positions, [start, end), per-token and path log-probability.
#include "common.hpp"
#include "ctc_ws.hpp"
#include "ctc_lattice.hpp"
#include "ctc_rows.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace ctc_align {

using asr::ctc::koff;
using asr::ctc::path_pad;
using asr::ctc::prep_kernel;

typedef unsigned long long u64;

constexpr size_t kLdsMax = 160 * 1024;      // one workgroup may own the whole LDS of a CU

struct Workspace {
    int* path_label;   // (B, Sp)
    int* path_mask;    // (B, Sp)
    int* path_len;     // (B)
    float* lse;        // (T, B)
    float* xg;         // (B, T, Sp)  raw logits on the path, -inf on dead nodes
    u64* bp;           // (B, T, Sp / 64, planes)  spilled back-pointer planes
    int* state;        // (B, T)  node of the best path at every frame
    size_t bytes;
};

static Workspace carve(void* base, int T, int B, int Lmax, int gram) {
    Workspace w;
    const size_t Sp = (size_t)path_pad(Lmax, gram);
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p ? p + off : nullptr; off += align_up(n, 256); return r; };
    w.path_label = (int*)take(sizeof(int) * B * Sp);
    w.path_mask = (int*)take(sizeof(int) * B * Sp);
    w.path_len = (int*)take(sizeof(int) * B);
    w.lse = (float*)take(sizeof(float) * (size_t)T * B);
    w.xg = (float*)take(sizeof(float) * (size_t)B * T * Sp);
    w.bp = (u64*)take(sizeof(u64) * (size_t)B * T * (Sp / 64) * (gram ? 3 : 2));
    w.state = (int*)take(sizeof(int) * (size_t)B * T);
    w.bytes = off;
    return w;
}

// LDS of the align kernel: two float64 state rows (8 guard slots in front), TC frames of planes, scan scratch, byte masks
static size_t lds_fixed(int Sp) { return sizeof(double) * 2 * (Sp + 16) + sizeof(int) * 32 + (size_t)Sp; }

// ------------------------------------------------------------------------------------------------ gather
// One workgroup per (t, b) row of logits: lse = log sum exp (as ctc::rows_kernel forms it), xg[b][t][s] = x[label_s].
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ xs, const int* __restrict__ x_len,
                                                     const int* __restrict__ path_label, int T, int B, int V, int Sp,
                                                     float* __restrict__ lse_out, float* __restrict__ xg) {
    __shared__ float scratch[32];
    const int row = blockIdx.x;            // row = t * B + b
    const int t = row / B, b = row - t * B;
    const int xl = x_len ? min(x_len[b], T) : T;
    if (t >= xl) return;
    const float* x = xs + (size_t)row * V;
    float m, sum;
    asr::ctc::row_max_sumexp(x, V, scratch, m, sum);                 // shared with the keyword search (csrc/ctc_rows.hpp)
    if (threadIdx.x == 0) lse_out[row] = m + __logf(sum);
    const int* pl = path_label + (size_t)b * Sp;
    float* out = xg + ((size_t)b * T + t) * Sp;
    for (int s = threadIdx.x; s < Sp; s += blockDim.x) {
        const int l = pl[s];
        out[s] = l >= 0 ? x[l] : -INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ align
// best predecessor of node s.  off[q] = s - k_q where the mask has edge class q, else -8: a guard slot that always holds -inf, so
// the mask costs nothing on the chain LDS read -> max -> add -> LDS write.  The maximum is a tree of v_max_f64; the winning class is
// found beside the chain: the smallest q whose candidate equals the maximum, which is the tie rule (a later candidate wins only
// if it is strictly larger than every earlier one).
template <int NK>
__device__ __forceinline__ void edge_offsets(int s, int mk, int* off) {
#pragma unroll
    for (int q = 0; q < NK; ++q) off[q] = ((mk >> q) & 1) ? s - koff<NK>(q) : -8;
}

template <int NK>
__device__ __forceinline__ double best_prev(const double* prev, const int* off, int& bj) {
    double v[NK];
#pragma unroll
    for (int q = 0; q < NK; ++q) v[q] = prev[off[q]];
    double best;
    if (NK == 3) {
        best = __builtin_fmax(__builtin_fmax(v[0], v[1]), v[2]);
    } else {
        best = __builtin_fmax(__builtin_fmax(__builtin_fmax(v[0], v[1]), __builtin_fmax(v[2], v[3])),
                              __builtin_fmax(__builtin_fmax(v[4], v[5]), v[NK - 1]));
    }
    bj = NK - 1;
#pragma unroll
    for (int q = NK - 2; q >= 0; --q) bj = v[q] == best ? q : bj;
    return best;
}

// the edge classes of the 64 nodes of this wave as NB 64-bit planes, written by one lane in one go; `row` = the frame's planes
template <int NB>
__device__ __forceinline__ void put_planes(u64* row, int block64, int bj, int lane) {
    u64 m[NB];
#pragma unroll
    for (int p = 0; p < NB; ++p) m[p] = __ballot((bj >> p) & 1);
    if (lane == 0) {
        u64* dst = row + block64 * NB;
        if (NB == 2) {
            *reinterpret_cast<ulonglong2*>(dst) = make_ulonglong2(m[0], m[1]);      // 16-byte aligned: see the LDS layout
        } else {
#pragma unroll
            for (int p = 0; p < NB; ++p) dst[p] = m[p];
        }
    }
}

template <int NK>
__global__ __launch_bounds__(1024) void align_kernel(const float* __restrict__ xg, const float* __restrict__ lse,
                                                     const int* __restrict__ x_len, const int* __restrict__ path_label,
                                                     const int* __restrict__ path_mask, const int* __restrict__ path_len,
                                                     int T, int B, int Sp, int Lmax, int TC, int blank, u64* __restrict__ bp_g,
                                                     int* __restrict__ state_g, int* __restrict__ frame_ids,
                                                     int* __restrict__ tok_ids, int* __restrict__ tok_pos,
                                                     int* __restrict__ tok_start, int* __restrict__ tok_end,
                                                     float* __restrict__ tok_logp, int* __restrict__ n_tok,
                                                     float* __restrict__ score) {
    constexpr int NB = NK == 3 ? 2 : 3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int fw = (Sp >> 6) * NB;                                  // 64-bit words of planes per frame
    double* buf0 = reinterpret_cast<double*>(smem);                  // Sp + 16 doubles each, 8 guard slots in front
    double* buf1 = buf0 + (Sp + 16);
    u64* bpc = reinterpret_cast<u64*>(buf1 + (Sp + 16));             // TC frames of planes
    int* scr = reinterpret_cast<int*>(bpc + (size_t)TC * fw);        // 32 ints
    unsigned char* mask_s = reinterpret_cast<unsigned char*>(scr + 32);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int xl = x_len ? min(x_len[b], T) : T;
    const int S = path_len[b];
    const float* xb = xg + (size_t)b * T * Sp;
    const int* pm = path_mask + (size_t)b * Sp;
    const int* pl = path_label + (size_t)b * Sp;
    u64* bpb = bp_g + (size_t)b * T * fw;
    int* st = state_g + (size_t)b * T;

    for (int i = tid; i < Sp + 16; i += blockDim.x) {                // guards: reading s - k below 0 sees -inf
        buf0[i] = -INFINITY;
        buf1[i] = -INFINITY;
    }
    for (int i = tid; i < Sp; i += blockDim.x) mask_s[i] = (unsigned char)pm[i];
    if (tid == 0) scr[31] = -1;
    __syncthreads();
    double* prev = buf0 + 8;
    double* cur = buf1 + 8;

    // ---- sweep
    if (xl > 0) {
        if (tid == 0) prev[0] = 0.0;                                 // virtual step -1 = e_0, as in the loss
        __syncthreads();
        constexpr int PF = 4;                                        // TC is a multiple of PF (host)
        if ((int)blockDim.x >= Sp) {                                 // one node per thread, logits prefetched PF steps ahead in registers
            const int sidx = tid, blk = tid >> 6;
            int off[NK];
            edge_offsets<NK>(sidx, mask_s[sidx], off);
            float lq[PF];
#pragma unroll
            for (int j = 0; j < PF; ++j) lq[j] = xb[(size_t)min(j, xl - 1) * Sp + sidx];
            for (int c0 = 0; c0 < xl; c0 += TC) {
                const int c1 = min(c0 + TC, xl);
                int t0 = c0;
                for (; t0 + PF <= c1; t0 += PF) {                    // whole blocks of PF steps, branch-free (see ctc::lattice_kernel)
#pragma unroll
                    for (int j = 0; j < PF; ++j) {
                        const int t = t0 + j;
                        int bj;
                        const double a = best_prev<NK>(prev, off, bj) + (double)lq[j];
                        cur[sidx] = a;
                        put_planes<NB>(bpc + (size_t)(t - c0) * fw, blk, bj, lane);
                        lq[j] = xb[(size_t)min(t + PF, xl - 1) * Sp + sidx];
                        ASR_LDS_BARRIER();
                        double* tmp = prev; prev = cur; cur = tmp;
                    }
                }
#pragma unroll
                for (int j = 0; j < PF - 1; ++j) {                   // the last xl % PF steps (only in the last block of frames)
                    const int t = t0 + j;
                    if (t < c1) {
                        int bj;
                        const double a = best_prev<NK>(prev, off, bj) + (double)lq[j];
                        cur[sidx] = a;
                        put_planes<NB>(bpc + (size_t)(t - c0) * fw, blk, bj, lane);
                        ASR_LDS_BARRIER();
                        double* tmp = prev; prev = cur; cur = tmp;
                    }
                }
                if (c1 < xl) {                                       // block full: spill it, the planes of the next one take its place
                    for (int i = tid; i < TC * fw; i += blockDim.x) bpb[(size_t)c0 * fw + i] = bpc[i];
                    __syncthreads();
                }
            }
        } else {
            for (int c0 = 0; c0 < xl; c0 += TC) {
                const int c1 = min(c0 + TC, xl);
                for (int t = c0; t < c1; ++t) {
                    const float* xt = xb + (size_t)t * Sp;
                    for (int s = tid; s < Sp; s += blockDim.x) {     // Sp and blockDim are multiples of 64: whole waves
                        int bj, off[NK];
                        edge_offsets<NK>(s, mask_s[s], off);
                        const double a = best_prev<NK>(prev, off, bj) + (double)xt[s];
                        cur[s] = a;
                        put_planes<NB>(bpc + (size_t)(t - c0) * fw, s >> 6, bj, lane);
                    }
                    __syncthreads();
                    double* tmp = prev; prev = cur; cur = tmp;
                }
                if (c1 < xl) {
                    for (int i = tid; i < TC * fw; i += blockDim.x) bpb[(size_t)c0 * fw + i] = bpc[i];
                    __syncthreads();
                }
            }
        }
        // prev = the last frame; final nodes: last blank, last label (CTC) / last bigram, last unigram (Gram-CTC).  Dead nodes hold
        // -inf.  Equal values: the largest node index.
        if (tid == 0) {
            double bv = prev[S - 1];
            int bs = S - 1;
            if (S >= 2 && prev[S - 2] > bv) { bv = prev[S - 2]; bs = S - 2; }
            if (NK != 3 && S >= 3 && prev[S - 3] > bv) { bv = prev[S - 3]; bs = S - 3; }
            scr[31] = bv == -INFINITY ? -1 : bs;
        }
        __syncthreads();
    }
    const int sfin = scr[31];
    const bool feasible = sfin >= 0;

    // ---- back-trace: the last block of frames is still in LDS, the earlier ones come back from the workspace
    if (feasible) {
        const int nchunk = (xl + TC - 1) / TC;
        int s = __builtin_amdgcn_readfirstlane(sfin);
        for (int c = nchunk - 1; c >= 0; --c) {
            const int c0 = c * TC, c1 = min(c0 + TC, xl);
            if (c != nchunk - 1) {
                __syncthreads();
                for (int i = tid; i < TC * fw; i += blockDim.x) bpc[i] = bpb[(size_t)c0 * fw + i];
                __syncthreads();
            }
            if (tid < 64) {
                // Wave 0 walks.  A path mostly stays on its node, so one LDS round trip serves a whole run of frames: lane l reads the
                // edge class that node s has at frame t - l; the first lane whose class is not "stay" is where the path entered s.
                // The lanes up to it store s for their frames in one go, the class of that lane gives the node before.  The chain has
                // one link per node of the path (plus one per 64 frames of a long run), not one per frame.
                int t = c1 - 1;
                while (t >= c0) {
                    const int tt = t - lane;
                    const bool valid = tt >= c0;
                    const u64* row = bpc + (size_t)(valid ? tt - c0 : 0) * fw + (s >> 6) * NB;
                    int code = 0;
#pragma unroll
                    for (int p = 0; p < NB; ++p) code |= (int)((row[p] >> (s & 63)) & 1) << p;
                    const u64 m = __ballot(valid && code != 0);
                    const int n = m ? __ffsll((long long)m) - 1 : min(63, t - c0);      // lanes 0 .. n stand on node s
                    if (lane <= n) st[tt] = s;
                    const int cn = m ? __builtin_amdgcn_readlane(code, n) : 0;
                    s = __builtin_amdgcn_readfirstlane(max(s - (NK == 3 ? cn : (cn < 4 ? cn : cn + 1)), 0));
                    t -= n + 1;
                }
            }
        }
        __threadfence();
    }
    __syncthreads();

    // ---- spans: one frame per thread; over the workgroup an exclusive scan of the token starts (which token a frame belongs to) and
    // an inclusive float64 scan of the frames' log-probabilities (a token's log-probability = prefix at its last frame - prefix before
    // its first: no thread walks a run; the path's log-probability is the last prefix).  Fixed order: bitwise reproducible.
    const int wid = tid >> 6, nwv = blockDim.x >> 6;
    double* wsum = buf0;            // the waves' sums of this block of frames
    double* pst = buf1;             // prefix before each token's first frame (Lmax < Sp doubles)
    double carry = 0.0;
    int base = 0;
    for (int tb = 0; tb < T; tb += blockDim.x) {
        const int t = tb + tid;
        const bool valid = feasible && t < xl;
        int s = 0, lab = blank;
        bool start = false, last = false;
        double v = 0.0;
        if (valid) {
            s = st[t];
            const int sp = t > 0 ? st[t - 1] : -1;
            const int sn = t + 1 < xl ? st[t + 1] : -1;
            lab = pl[s];
            const bool token = NK == 3 ? (s & 1) : (s % 3 != 0);
            start = token && s != sp;
            last = token && s != sn;
            v = (double)xb[(size_t)t * Sp + s] - (double)lse[(size_t)t * B + b];
        }
        if (t < T) frame_ids[(size_t)b * T + t] = lab;
        double inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(inc, o, 64);
            inc += lane >= o ? u : 0.0;
        }
        const u64 bal = __ballot(start);
        if (lane == 63) wsum[wid] = inc;
        if (lane == 0) scr[wid] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
        double pbefore = 0.0, ptot = 0.0;
        for (int w = 0; w < nwv; ++w) {
            const int c = scr[w];
            const double d = wsum[w];
            tot += c;
            ptot += d;
            before += w < wid ? c : 0;
            pbefore += w < wid ? d : 0.0;
        }
        const double incl = carry + (pbefore + inc);
        const int k = base + before + __popcll(bal & ((2ull << lane) - 1ull)) - 1;      // the token of this frame, if it has one
        if (start && k < Lmax) {
            const size_t o = (size_t)b * Lmax + k;
            tok_ids[o] = lab;
            tok_pos[o] = NK == 3 ? (s - 1) >> 1 : (s % 3 == 1 ? s / 3 : s / 3 - 1);
            tok_start[o] = t;
            pst[k] = incl - v;
        }
        __syncthreads();
        if (last && k < Lmax) {
            const size_t o = (size_t)b * Lmax + k;
            tok_end[o] = t + 1;
            tok_logp[o] = (float)(incl - pst[k]);
        }
        carry += ptot;
        base += tot;
    }
    for (int k = base + tid; k < Lmax; k += blockDim.x) {
        const size_t o = (size_t)b * Lmax + k;
        tok_ids[o] = blank;
        tok_pos[o] = 0;
        tok_start[o] = 0;
        tok_end[o] = 0;
        tok_logp[o] = 0.f;
    }
    if (tid == 0) {
        n_tok[b] = base;
        score[b] = feasible ? (float)carry : -INFINITY;
    }
}

}  // namespace ctc_align
}  // namespace asr

using namespace asr;
using namespace asr::ctc_align;

extern "C" size_t asr_ctc_align_workspace_bytes(int T, int B, int V, int Lmax, int gram) {
    (void)V;
    if (T <= 0 || B <= 0 || Lmax <= 0) return 0;
    return carve(nullptr, T, B, Lmax, gram).bytes;
}

extern "C" int asr_ctc_align(void* stream_, const float* xs, const int32_t* label_unigram, const int32_t* label_bigram,
                             const int32_t* x_len, const int32_t* l_len, int T, int B, int V, int Lmax, int blank,
                             int32_t* frame_ids, int32_t* tok_ids, int32_t* tok_pos, int32_t* tok_start, int32_t* tok_end,
                             float* tok_logp, int32_t* n_tok, float* score, void* workspace, size_t workspace_bytes) {
    if (!xs || !label_unigram || !frame_ids || !tok_ids || !tok_pos || !tok_start || !tok_end || !tok_logp || !n_tok || !score ||
        !workspace)
        return ASR_ERR_BAD_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || Lmax <= 0 || blank < 0 || blank >= V) return ASR_ERR_BAD_ARG;
    const int gram = label_bigram != nullptr;
    Workspace w = carve(workspace, T, B, Lmax, gram);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    const int Sp = path_pad(Lmax, gram);
    if (sizeof(double) * 2 * (Sp + 16) + sizeof(int) * (Sp + 8) > 150 * 1024) return ASR_ERR_UNSUPPORTED;   // the loss's bound
    const size_t frame_bytes = sizeof(u64) * (size_t)(Sp / 64) * (gram ? 3 : 2);
    const size_t room = (kLdsMax - lds_fixed(Sp)) / frame_bytes;
    const int TC = (int)(room < (size_t)align_up(T, 4) ? room & ~(size_t)3 : align_up(T, 4));
    if (TC < 4) return ASR_ERR_UNSUPPORTED;
    const size_t lds = lds_fixed(Sp) + frame_bytes * TC;
    hipStream_t stream = (hipStream_t)stream_;
    if (gram)
        hipLaunchKernelGGL(prep_kernel<true>, dim3(B), dim3(256), 0, stream, label_unigram, label_bigram, l_len, Lmax, Sp,
                           V, blank, w.path_label, w.path_mask, w.path_len);
    else
        hipLaunchKernelGGL(prep_kernel<false>, dim3(B), dim3(256), 0, stream, label_unigram, label_bigram, l_len, Lmax,
                           Sp, V, blank, w.path_label, w.path_mask, w.path_len);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gather_kernel, dim3(T * B), dim3(256), 0, stream, xs, x_len, w.path_label, T, B, V, Sp, w.lse, w.xg);
    ASR_LAUNCH_CHECK();
    const int threads = Sp < 1024 ? Sp : 1024;
    if (gram) {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)align_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(align_kernel<7>, dim3(B), dim3(threads), lds, stream, w.xg, w.lse, x_len, w.path_label, w.path_mask,
                           w.path_len, T, B, Sp, Lmax, TC, blank, w.bp, w.state, frame_ids, tok_ids, tok_pos, tok_start,
                           tok_end, tok_logp, n_tok, score);
    } else {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)align_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(align_kernel<3>, dim3(B), dim3(threads), lds, stream, w.xg, w.lse, x_len, w.path_label, w.path_mask,
                           w.path_len, T, B, Sp, Lmax, TC, blank, w.bp, w.state, frame_ids, tok_ids, tok_pos, tok_start,
                           tok_end, tok_logp, n_tok, score);
    }
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
