// CTC keyword spotting for gfx950: where, if anywhere, does a phrase occur in the logits, and how sure is the model (DESIGN.md
// section 30).  A sibling of csrc/ctc_align.hip on the same footing -- float64 max-plus, ONE addition per step, reproducible bit for
// bit by a NumPy restatement (tests/keyword_reference.py) -- but with free boundaries: an occurrence may start and end on any frame.
// The reference has no keyword search.
//
// Per utterance and keyword w_1..w_L the lattice is tok_1, blk_2, tok_2, .., blk_L, tok_L (no leading or trailing blank); the cost of
// label v at frame t is c(t, v) = (double)x[t][v] - (double)xmax[t] <= 0 (log p(v) - log p(argmax): the row's log-sum-exp cancels):
//   tok_1[t] = c(t, w_1)   + best(tok_1[t-1], fresh (0.0, start = t))
//   blk_i[t] = c(t, blank) + best(blk_i[t-1], tok_{i-1}[t-1])
//   tok_i[t] = c(t, w_i)   + best(tok_i[t-1], blk_i[t-1], tok_{i-1}[t-1] only if w_i != w_{i-1})
// `best` takes the FIRST maximum in the order written, the start frame travels with the winner.  det[t] = (float)tok_L[t].
//
// Four kernels, all on the caller's stream:
//   rows   (T*B workgroups)          one read of every valid logit row, reduced as ctc_align::gather_kernel reduces it: xmax, the
//                                    blank's logit, the U logits of the distinct keyword tokens, fill = xmax - lse  [HBM: read T*B*V]
//   sweep  (B*ceil(K/kGroup) wg)     one wave per (b, k) lattice, lane i owns tok_{i+1} and blk_{i+1}; the neighbour's value crosses
//                                    lanes in registers (__shfl_up), there is no barrier of any kind: the kGroup waves of a workgroup
//                                    are keywords of one utterance, so they hit the same xmax / blank lines, and run independently.
//                                    A lane's logits come kTile frames at a time into registers, the next tile while this one runs.
//                                    det of the kTile frames is collected one lane per frame and written as one coalesced store.
//   hits   (B*K workgroups)          non-maximum suppression: block arg-max by (det desc, start asc, end desc), max_hits rounds
//   reset  (B*K workgroups)          the carried state of a stream: values -inf, starts -1, frames consumed 0
//
// The Gram-CTC form (asr_gram_kws_detect) searches a phrase of characters c_1..c_L over every way of cutting it
// into unigram and bigram tokens at once: position i has the nodes U_i (the token spelled c_i), G_i (the token spelled c_{i-1} c_i,
// i >= 2) and B_i (the blank between positions i-1 and i, i >= 2) -- the edges of ctc_lattice.hpp's prep_kernel<true> with its two
// guards, minus the outer blanks, plus a fresh start into U_1 and G_2:
//   B_i[t] = c(t, blank) + best(B_i[t-1], U_{i-1}[t-1], G_{i-1}[t-1])
//   U_i[t] = c(t, u_i)   + best(U_i[t-1], B_i[t-1], U_{i-1}[t-1] only if c_i != c_{i-1}, G_{i-1}[t-1])
//   G_i[t] = c(t, g_i)   + best(G_i[t-1], B_{i-1}[t-1], U_{i-2}[t-1], G_{i-2}[t-1] only if g_i != g_{i-2})
//   det[t] = (float)best(U_L[t], G_L[t])
// rows, hits and the workspace are the ones above (uniq simply holds bigram token ids too); the sweep is gram_sweep_kernel: lane i-1
// owns U_i, G_i and B_i, five values and five starts cross lanes per step, still without a barrier.
#include "common.hpp"
#include "ctc_rows.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace ctc_kws {

constexpr int kGroup = 4;        // keywords (waves) per sweep workgroup         (asr/spot.py: SWEEP_GROUP)
constexpr int kTile = 32;        // frames per register tile of the sweep        (asr/spot.py: SWEEP_TILE)
constexpr int kMaxLen = 64;      // one token and its blank per lane
constexpr int kMaxHits = 4096;   // spans kept in LDS by the hits kernel
constexpr int kGramTile = 32;    // frames per register tile of the Gram sweep   (asr/spot.py: GRAM_SWEEP_TILE)

struct Workspace {
    float* xmax;     // (B, T)
    float* xblank;   // (B, T)
    float* xg;       // (B, T, U)  raw logits of the distinct keyword tokens
    int* base;       // (B)        frames consumed before this call (0 in the one-shot form)
    size_t bytes;
};

// no rounding between the parts: every part is a whole number of 4-byte words, and the query grows with each argument
static Workspace carve(void* ws, int T, int B, int U) {
    Workspace w;
    char* p = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p ? p + off : nullptr; off += n; return r; };
    w.xmax = (float*)take(sizeof(float) * (size_t)B * T);
    w.xblank = (float*)take(sizeof(float) * (size_t)B * T);
    w.xg = (float*)take(sizeof(float) * (size_t)B * T * U);
    w.base = (int*)take(sizeof(int) * (size_t)B);
    w.bytes = off;
    return w;
}

// the carried state: per (b, k) the float64 values of the `nodes` nodes of every position (CTC: tok, blk; Gram-CTC: U, B, G), their
// int starts; per b the frames consumed
struct State {
    double* val;     // (B, K, nodes, Lmax)
    int* start;      // (B, K, nodes, Lmax)
    int* consumed;   // (B)
    size_t bytes;
};

static State carve_state(void* st, int B, int K, int Lmax, int nodes = 2) {
    State s;
    char* p = (char*)st;
    const size_t n = (size_t)B * K * nodes * Lmax;
    s.val = (double*)p;
    s.start = (int*)(p ? p + sizeof(double) * n : nullptr);
    s.consumed = (int*)(p ? p + (sizeof(double) + sizeof(int)) * n : nullptr);
    s.bytes = (sizeof(double) + sizeof(int)) * n + sizeof(int) * (size_t)B;
    return s;
}

// ------------------------------------------------------------------------------------------------ rows
// One workgroup per (t, b) row.  The maximum and the sum come from the function ctc_align::gather_kernel calls (csrc/ctc_rows.hpp),
// so lse is the same f32 value.
__global__ __launch_bounds__(256) void rows_kernel(const float* __restrict__ xs, const int* __restrict__ x_len,
                                                   const int* __restrict__ uniq, int T, int B, int V, int U, int blank,
                                                   int* __restrict__ consumed, float* __restrict__ xmax_out,
                                                   float* __restrict__ xblank_out, float* __restrict__ xg, int* __restrict__ base,
                                                   float* __restrict__ fill) {
    __shared__ float scratch[32];
    const int row = blockIdx.x;            // row = t * B + b
    const int t = row / B, b = row - t * B;
    const int xl = x_len ? min(max(x_len[b], 0), T) : T;
    if (t == 0 && threadIdx.x == 0) {      // the one workgroup of utterance b that moves its frame counter
        const int c = consumed ? consumed[b] : 0;
        base[b] = c;
        if (consumed) consumed[b] = c + xl;
    }
    const size_t o = (size_t)b * T + t;
    if (t >= xl) {
        if (threadIdx.x == 0) fill[o] = 0.f;
        return;
    }
    const float* x = xs + (size_t)row * V;
    float m, sum;
    asr::ctc::row_max_sumexp(x, V, scratch, m, sum);
    if (threadIdx.x == 0) {
        const float lse = m + __logf(sum);
        xmax_out[o] = m;
        xblank_out[o] = x[blank];
        fill[o] = m - lse;
    }
    float* out = xg + o * U;
    for (int u = threadIdx.x; u < U; u += blockDim.x) {
        const int id = uniq[u];
        out[u] = (id >= 0 && id < V) ? x[id] : -INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ sweep
__device__ __forceinline__ float bcast_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double bcast_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kGroup * 64) void sweep_kernel(const float* __restrict__ xmax, const float* __restrict__ xblank,
                                                            const float* __restrict__ xg, const int* __restrict__ x_len,
                                                            const int* __restrict__ node_tok, const int* __restrict__ kw_len,
                                                            const int* __restrict__ base, int T, int B, int U, int K, int Lmax,
                                                            double* __restrict__ st_val, int* __restrict__ st_start,
                                                            float* __restrict__ det, int* __restrict__ det_start) {
    const int lane = threadIdx.x & 63;
    const int groups = (K + kGroup - 1) / kGroup;
    const int b = blockIdx.x / groups;
    const int k = __builtin_amdgcn_readfirstlane((blockIdx.x - b * groups) * kGroup + (int)(threadIdx.x >> 6));
    if (k >= K) return;                    // whole waves leave; nothing below waits for another wave
    const int xl = x_len ? min(max(x_len[b], 0), T) : T;
    const int L = __builtin_amdgcn_readfirstlane(kw_len[k]);
    const bool okL = L >= 1 && L <= Lmax;
    const int idx = lane < Lmax ? node_tok[(size_t)k * Lmax + lane] : -1;
    const bool mine = okL && lane < L;
    const bool live = okL && __ballot(mine && (idx < 0 || idx >= U)) == 0ull;
    float* dk = det + ((size_t)b * K + k) * T;
    int* sk = det_start + ((size_t)b * K + k) * T;
    int done = 0;                          // frames of this call whose det is written

    if (live && xl > 0) {
        const int idx_up = __shfl_up(idx, 1, 64);
        const bool first = lane == 0;
        const bool diff = first || idx != idx_up;                    // w_i != w_{i-1}: uniq is one to one with the ids
        const bool has_blk = mine && !first;
        const int t_base = base[b];
        const size_t so = ((size_t)b * K + k) * 2 * Lmax + lane;
        double tok = -INFINITY, blk = -INFINITY;
        int ts = -1, bs = -1;
        if (st_val && lane < Lmax) {
            tok = st_val[so];
            blk = st_val[so + Lmax];
            ts = st_start[so];
            bs = st_start[so + Lmax];
        }
        const float* gx = xg + (size_t)b * T * U + (mine ? idx : 0);
        const float* mb = xmax + (size_t)b * T;
        const float* bb = xblank + (size_t)b * T;
        const int last = xl - 1;
        float xc[kTile], xn[kTile];
#pragma unroll
        for (int j = 0; j < kTile; ++j) xc[j] = gx[(size_t)min(j, last) * U];
        float mc = mb[min(lane, last)], bc = bb[min(lane, last)];     // lane j holds frame t0 + j of the tile
        const int Lm1 = L - 1;
        for (int t0 = 0; t0 < xl; t0 += kTile) {
            const int n = min(kTile, xl - t0);
#pragma unroll
            for (int j = 0; j < kTile; ++j) xn[j] = gx[(size_t)min(t0 + kTile + j, last) * U];      // the next tile, clamped
            const float mn = mb[min(t0 + kTile + lane, last)], bn = bb[min(t0 + kTile + lane, last)];
            const double cb_l = (double)bc - (double)mc;             // c(t, blank) of the lane's frame
            float keep_v = -INFINITY;
            int keep_s = -1;
#pragma unroll
            for (int j = 0; j < kTile; ++j) {
                if (j < n) {                                         // uniform
                    // the costs: formed beside the chain (they do not depend on the carried values)
                    const double cm = (double)bcast_f(mc, j);
                    const double ct = mine ? (double)xc[j] - cm : -INFINITY;
                    const double cb = has_blk ? bcast_d(cb_l, j) : -INFINITY;
                    // the chain: neighbour across lanes, max, one add; the selects carry the start
                    double up_v = __shfl_up(tok, 1, 64);
                    int up_s = __shfl_up(ts, 1, 64);
                    up_v = first ? 0.0 : up_v;                       // the fresh start of the first token
                    up_s = first ? t_base + t0 + j : up_s;
                    const double ub = first ? -INFINITY : up_v;      // there is no blank in front of the first token
                    const double uv = diff ? up_v : -INFINITY;
                    const double m1 = __builtin_fmax(tok, blk);
                    const int s1 = blk > tok ? bs : ts;
                    const double nblk = cb + __builtin_fmax(blk, ub);
                    const int nbs = ub > blk ? up_s : bs;
                    const double ntok = ct + __builtin_fmax(m1, uv);
                    const int nts = uv > m1 ? up_s : s1;
                    tok = ntok;
                    ts = mine ? nts : -1;                            // lanes past L stay (-inf, -1), also in the carried state
                    blk = nblk;
                    bs = has_blk ? nbs : -1;
                    const float dv = (float)bcast_d(tok, Lm1);
                    const int dsv = __builtin_amdgcn_readlane(ts, Lm1);
                    keep_v = lane == j ? dv : keep_v;
                    keep_s = lane == j ? dsv : keep_s;
                }
            }
            if (lane < n) {
                dk[t0 + lane] = keep_v;
                sk[t0 + lane] = keep_s;
            }
#pragma unroll
            for (int j = 0; j < kTile; ++j) xc[j] = xn[j];
            mc = mn;
            bc = bn;
        }
        if (st_val && lane < Lmax) {
            st_val[so] = tok;
            st_val[so + Lmax] = blk;
            st_start[so] = ts;
            st_start[so + Lmax] = bs;
        }
        done = xl;
    }
    for (int t = done + lane; t < T; t += 64) {                      // frames past the length; every frame of a keyword without a path
        dk[t] = -INFINITY;
        sk[t] = -1;
    }
}

// ------------------------------------------------------------------------------------------------ gram sweep
// the first maximum of (a, b): b wins only if it is strictly larger, the start travels with the winner
__device__ __forceinline__ void first_max(double a, int as, double b, int bs, double& m, int& s) {
    m = __builtin_fmax(a, b);
    s = b > a ? bs : as;
}
// `best` of four candidates in the order written, as a tree: the first maximum of (a, b), the first maximum of (c, d), and the
// second pair wins only if it is strictly larger -- the same winner as the left-to-right scan, two max deep instead of three
__device__ __forceinline__ void best4(double a, int as, double b, int bs, double c, int cs, double d, int ds, double& m, int& s) {
    double l, r;
    int ls, rs;
    first_max(a, as, b, bs, l, ls);
    first_max(c, cs, d, ds, r, rs);
    first_max(l, ls, r, rs, m, s);
}

// One wave per (b, k) lattice; lane p owns position i = p + 1: U_i, G_i (p >= 1) and B_i (p >= 1).  From lane p - 1 come U, G and B,
// from lane p - 2 come U and G.  What __shfl_up hands the lanes below its distance is the lane's OWN value, so:
//   lane 0, distance 1   the U slot is the fresh start of U_1; its G and B slots are lane 0's own G and B, which do not exist and
//                        are -inf from the reset on (their cost is -inf on every frame)
//   lane 1, distance 2   the U slot is the fresh start of G_2, the G slot is masked to -inf (its own G_2 is live)
//   lane 0, distance 2   feeds only G_1, which does not exist: whatever arrives is added to a cost of -inf
// An absent node (no such token in the inventory) has cost -inf, so its value stays -inf; a node whose new value is -inf gets start
// -1, which also keeps the starts of absent nodes and of the lanes >= L at -1 although a live neighbour hands them one.
__global__ __launch_bounds__(kGroup * 64) void gram_sweep_kernel(const float* __restrict__ xmax, const float* __restrict__ xblank,
                                                                 const float* __restrict__ xg, const int* __restrict__ x_len,
                                                                 const int* __restrict__ node_uni, const int* __restrict__ node_big,
                                                                 const int* __restrict__ kw_len, const int* __restrict__ base, int T,
                                                                 int B, int U, int K, int Lmax, double* __restrict__ st_val,
                                                                 int* __restrict__ st_start, float* __restrict__ det,
                                                                 int* __restrict__ det_start) {
    const int lane = threadIdx.x & 63;
    const int groups = (K + kGroup - 1) / kGroup;
    const int b = blockIdx.x / groups;
    const int k = __builtin_amdgcn_readfirstlane((blockIdx.x - b * groups) * kGroup + (int)(threadIdx.x >> 6));
    if (k >= K) return;                    // whole waves leave; nothing below waits for another wave
    const int xl = x_len ? min(max(x_len[b], 0), T) : T;
    const int L = __builtin_amdgcn_readfirstlane(kw_len[k]);
    const bool okL = L >= 1 && L <= Lmax;
    float* dk = det + ((size_t)b * K + k) * T;
    int* sk = det_start + ((size_t)b * K + k) * T;
    int done = 0;                          // frames of this call whose det is written

    if (okL && xl > 0) {
        const bool mine = lane < L;
        const bool first = lane == 0, second = lane == 1;
        int iu = mine ? node_uni[(size_t)k * Lmax + lane] : -1;
        int ig = mine && !first ? node_big[(size_t)k * Lmax + lane] : -1;
        iu = iu >= 0 && iu < U ? iu : -1;                            // absent nodes: one spelling
        ig = ig >= 0 && ig < U ? ig : -1;
        const bool has_u = iu >= 0, has_g = ig >= 0, has_b = mine && !first;
        // the guards: uniq is one to one with the token ids, so equal indices are equal characters / equal bigrams; where a node
        // is absent the guard is moot (one side of the edge is -inf).  The shuffles stand alone: behind a short-circuit they would
        // run with the source lanes switched off.
        const int iu1 = __shfl_up(iu, 1, 64), ig2 = __shfl_up(ig, 2, 64);
        const bool same_u = !first && has_u && iu == iu1;                           // c_i == c_{i-1}
        const bool same_g = lane >= 2 && has_g && ig == ig2;                        // g_i == g_{i-2}
        const int t_base = base[b];
        const size_t so = ((size_t)b * K + k) * 3 * Lmax + lane;
        double uv = -INFINITY, bv = -INFINITY, gv = -INFINITY;
        int us = -1, bs = -1, gs = -1;
        if (st_val && lane < Lmax) {
            uv = st_val[so];
            bv = st_val[so + Lmax];
            gv = st_val[so + 2 * Lmax];
            us = st_start[so];
            bs = st_start[so + Lmax];
            gs = st_start[so + 2 * Lmax];
        }
        const float* gxu = xg + (size_t)b * T * U + (has_u ? iu : 0);
        const float* gxg = xg + (size_t)b * T * U + (has_g ? ig : 0);
        const float* mb = xmax + (size_t)b * T;
        const float* bb = xblank + (size_t)b * T;
        const int last = xl - 1;
        float xcu[kGramTile], xcg[kGramTile], xnu[kGramTile], xng[kGramTile];
#pragma unroll
        for (int j = 0; j < kGramTile; ++j) {
            xcu[j] = gxu[(size_t)min(j, last) * U];
            xcg[j] = gxg[(size_t)min(j, last) * U];
        }
        float mc = mb[min(lane, last)], bc = bb[min(lane, last)];     // lane j holds frame t0 + j of the tile
        const int Lm1 = L - 1;
        for (int t0 = 0; t0 < xl; t0 += kGramTile) {
            const int n = min(kGramTile, xl - t0);
#pragma unroll
            for (int j = 0; j < kGramTile; ++j) {                     // the next tile, clamped
                xnu[j] = gxu[(size_t)min(t0 + kGramTile + j, last) * U];
                xng[j] = gxg[(size_t)min(t0 + kGramTile + j, last) * U];
            }
            const float mn = mb[min(t0 + kGramTile + lane, last)], bn = bb[min(t0 + kGramTile + lane, last)];
            const double cb_l = (double)bc - (double)mc;             // c(t, blank) of the lane's frame
            float keep_v = -INFINITY;
            int keep_s = -1;
#pragma unroll
            for (int j = 0; j < kGramTile; ++j) {
                if (j < n) {                                         // uniform
                    // the costs: formed beside the chain (they do not depend on the carried values)
                    const double cm = (double)bcast_f(mc, j);
                    const double cu = has_u ? (double)xcu[j] - cm : -INFINITY;
                    const double cg = has_g ? (double)xcg[j] - cm : -INFINITY;
                    const double cb = has_b ? bcast_d(cb_l, j) : -INFINITY;
                    const int now = t_base + t0 + j;
                    // the chain: neighbours across lanes, max, one add; the selects carry the starts
                    double u1 = __shfl_up(uv, 1, 64), g1 = __shfl_up(gv, 1, 64), b1 = __shfl_up(bv, 1, 64);
                    int u1s = __shfl_up(us, 1, 64), g1s = __shfl_up(gs, 1, 64), b1s = __shfl_up(bs, 1, 64);
                    double u2 = __shfl_up(uv, 2, 64), g2 = __shfl_up(gv, 2, 64);
                    int u2s = __shfl_up(us, 2, 64), g2s = __shfl_up(gs, 2, 64);
                    u1 = first ? 0.0 : u1;                           // the fresh start of U_1
                    u1s = first ? now : u1s;
                    u2 = second ? 0.0 : u2;                          // the fresh start of G_2
                    u2s = second ? now : u2s;
                    g2 = lane < 2 ? -INFINITY : g2;                  // there is no G_0 (and no G_{-1})
                    const double u1g = same_u ? -INFINITY : u1;
                    const double g2g = same_g ? -INFINITY : g2;
                    double r, nb, nu, ng;
                    int rs, nbs, nus, ngs;
                    first_max(u1, u1s, g1, g1s, r, rs);              // B_i: stay, U_{i-1}, G_{i-1}
                    first_max(bv, bs, r, rs, nb, nbs);
                    best4(uv, us, bv, bs, u1g, u1s, g1, g1s, nu, nus);
                    best4(gv, gs, b1, b1s, u2, u2s, g2g, g2s, ng, ngs);
                    uv = cu + nu;
                    bv = cb + nb;
                    gv = cg + ng;
                    us = uv == -INFINITY ? -1 : nus;
                    bs = bv == -INFINITY ? -1 : nbs;
                    gs = gv == -INFINITY ? -1 : ngs;
                    double dl;                                       // det: best(U_L, G_L), both in lane L - 1
                    int dls;
                    first_max(uv, us, gv, gs, dl, dls);
                    const float dv = (float)bcast_d(dl, Lm1);
                    const int dsv = __builtin_amdgcn_readlane(dls, Lm1);
                    keep_v = lane == j ? dv : keep_v;
                    keep_s = lane == j ? dsv : keep_s;
                }
            }
            if (lane < n) {
                dk[t0 + lane] = keep_v;
                sk[t0 + lane] = keep_s;
            }
#pragma unroll
            for (int j = 0; j < kGramTile; ++j) {
                xcu[j] = xnu[j];
                xcg[j] = xng[j];
            }
            mc = mn;
            bc = bn;
        }
        if (st_val && lane < Lmax) {
            st_val[so] = uv;
            st_val[so + Lmax] = bv;
            st_val[so + 2 * Lmax] = gv;
            st_start[so] = us;
            st_start[so + Lmax] = bs;
            st_start[so + 2 * Lmax] = gs;
        }
        done = xl;
    }
    for (int t = done + lane; t < T; t += 64) {                      // frames past the length; every frame of a phrase without a path
        dk[t] = -INFINITY;
        sk[t] = -1;
    }
}

// ------------------------------------------------------------------------------------------------ reset
__global__ __launch_bounds__(128) void reset_kernel(double* __restrict__ val, int* __restrict__ start, int* __restrict__ consumed,
                                                    const int* __restrict__ mask, int K, int per) {      // per = nodes * Lmax
    const int bk = blockIdx.x, b = bk / K;
    if (mask && mask[b] == 0) return;
    const size_t o = (size_t)bk * per;
    for (int i = threadIdx.x; i < per; i += blockDim.x) {
        val[o + i] = -INFINITY;
        start[o + i] = -1;
    }
    if (bk - b * K == 0 && threadIdx.x == 0) consumed[b] = 0;
}

// ------------------------------------------------------------------------------------------------ hits
struct Cand {
    float v;
    int s, e;
};
// the three keys: larger det, then the smaller start, then the larger end
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
    return a.v > b.v || (a.v == b.v && (a.s < b.s || (a.s == b.s && a.e > b.e)));
}

__global__ __launch_bounds__(256) void hits_kernel(const float* __restrict__ det, const int* __restrict__ det_start,
                                                   const float* __restrict__ fill, const int* __restrict__ lengths, int K, int T,
                                                   int max_hits, float min_score, int* __restrict__ hit_start,
                                                   int* __restrict__ hit_end, float* __restrict__ hit_score,
                                                   float* __restrict__ hit_logp, int* __restrict__ n_hits) {
    extern __shared__ int span[];          // (max_hits, 2): start, end (inclusive) of the recorded hits
    __shared__ float wv[4];
    __shared__ int wse[8];
    const int bk = blockIdx.x, b = bk / K, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int xl = lengths ? min(max(lengths[b], 0), T) : T;
    const float* d = det + (size_t)bk * T;
    const int* ds = det_start + (size_t)bk * T;
    const float* fb = fill + (size_t)b * T;
    const size_t ho = (size_t)bk * max_hits;
    int n = 0;
    for (; n < max_hits; ++n) {
        Cand best = {-INFINITY, 0x7fffffff, -1};
        for (int e = tid; e < xl; e += blockDim.x) {
            const Cand c = {d[e], ds[e], e};
            if (!(c.v >= min_score) || !(fabsf(c.v) < INFINITY)) continue;
            bool free_ = true;
            for (int h = 0; h < n; ++h) free_ = free_ && !(c.s <= span[2 * h + 1] && e >= span[2 * h]);
            if (free_ && better(c, best)) best = c;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const Cand c = {__shfl_xor(best.v, o, 64), __shfl_xor(best.s, o, 64), __shfl_xor(best.e, o, 64)};
            if (better(c, best)) best = c;
        }
        if (lane == 0) {
            wv[wid] = best.v;
            wse[2 * wid] = best.s;
            wse[2 * wid + 1] = best.e;
        }
        __syncthreads();
        best = {wv[0], wse[0], wse[1]};
        for (int w = 1; w < 4; ++w) {
            const Cand c = {wv[w], wse[2 * w], wse[2 * w + 1]};
            if (better(c, best)) best = c;
        }
        if (best.e < 0) break;             // uniform: every thread folds the same four entries in the same order
        if (tid == 0) {
            span[2 * n] = best.s;
            span[2 * n + 1] = best.e;
            // left to right over the span, float64, by one thread: the pinned order.  A prefix sum of fill per utterance would
            // serve every hit with two reads but rounds differently, so hit_logp would no longer be this sum bit for bit.
            double acc = 0.0;
            for (int t = max(best.s, 0); t <= best.e; ++t) acc += (double)fb[t];
            hit_start[ho + n] = best.s;
            hit_end[ho + n] = best.e + 1;
            hit_score[ho + n] = best.v;
            hit_logp[ho + n] = (float)((double)best.v + acc);
        }
        __syncthreads();
    }
    for (int h = n + tid; h < max_hits; h += blockDim.x) {
        hit_start[ho + h] = -1;
        hit_end[ho + h] = -1;
        hit_score[ho + h] = -INFINITY;
        hit_logp[ho + h] = -INFINITY;
    }
    if (tid == 0) n_hits[bk] = n;
}

}  // namespace ctc_kws
}  // namespace asr

using namespace asr;
using namespace asr::ctc_kws;

static bool too_many(long long blocks) { return blocks > 0x7fffffffLL; }

extern "C" size_t asr_kws_workspace_bytes(int T, int B, int U) {
    if (T <= 0 || B <= 0 || U <= 0) return 0;
    return carve(nullptr, T, B, U).bytes;
}

extern "C" size_t asr_kws_state_bytes(int B, int K, int Lmax) {
    if (B <= 0 || K <= 0 || Lmax <= 0) return 0;
    return carve_state(nullptr, B, K, Lmax).bytes;
}

extern "C" int asr_kws_state_reset(void* stream_, void* state, int B, int K, int Lmax, const int32_t* mask) {
    if (!state || B <= 0 || K <= 0 || Lmax <= 0) return ASR_ERR_BAD_ARG;
    if (Lmax > kMaxLen || too_many((long long)B * K)) return ASR_ERR_UNSUPPORTED;
    State s = carve_state(state, B, K, Lmax);
    hipLaunchKernelGGL(reset_kernel, dim3(B * K), dim3(128), 0, (hipStream_t)stream_, s.val, s.start, s.consumed, mask, K,
                       2 * Lmax);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_kws_detect(void* stream_, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                              const int32_t* uniq, int U, const int32_t* node_tok, const int32_t* kw_len, int K, int Lmax,
                              void* state, float* det, int32_t* det_start, float* fill, void* workspace, size_t workspace_bytes) {
    if (!logits || !uniq || !node_tok || !kw_len || !det || !det_start || !fill || !workspace) return ASR_ERR_BAD_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || U <= 0 || K <= 0 || Lmax <= 0 || blank < 0 || blank >= V) return ASR_ERR_BAD_ARG;
    const long long groups = (K + kGroup - 1) / kGroup;
    if (Lmax > kMaxLen || too_many((long long)T * B) || too_many((long long)B * groups)) return ASR_ERR_UNSUPPORTED;
    Workspace w = carve(workspace, T, B, U);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    State s = carve_state(state, B, K, Lmax);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(rows_kernel, dim3(T * B), dim3(256), 0, stream, logits, lengths, uniq, T, B, V, U, blank,
                       state ? s.consumed : nullptr, w.xmax, w.xblank, w.xg, w.base, fill);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)(B * groups)), dim3(kGroup * 64), 0, stream, w.xmax, w.xblank, w.xg, lengths,
                       node_tok, kw_len, w.base, T, B, U, K, Lmax, state ? s.val : nullptr, state ? s.start : nullptr, det,
                       det_start);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" size_t asr_gram_kws_state_bytes(int B, int K, int Lmax) {
    if (B <= 0 || K <= 0 || Lmax <= 0) return 0;
    return carve_state(nullptr, B, K, Lmax, 3).bytes;
}

extern "C" int asr_gram_kws_state_reset(void* stream_, void* state, int B, int K, int Lmax, const int32_t* mask) {
    if (!state || B <= 0 || K <= 0 || Lmax <= 0) return ASR_ERR_BAD_ARG;
    if (Lmax > kMaxLen || too_many((long long)B * K)) return ASR_ERR_UNSUPPORTED;
    State s = carve_state(state, B, K, Lmax, 3);
    hipLaunchKernelGGL(reset_kernel, dim3(B * K), dim3(128), 0, (hipStream_t)stream_, s.val, s.start, s.consumed, mask, K,
                       3 * Lmax);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_gram_kws_detect(void* stream_, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                   const int32_t* uniq, int U, const int32_t* node_uni, const int32_t* node_big,
                                   const int32_t* kw_len, int K, int Lmax, void* state, float* det, int32_t* det_start, float* fill,
                                   void* workspace, size_t workspace_bytes) {
    if (!logits || !uniq || !node_uni || !node_big || !kw_len || !det || !det_start || !fill || !workspace) return ASR_ERR_BAD_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || U <= 0 || K <= 0 || Lmax <= 0 || blank < 0 || blank >= V) return ASR_ERR_BAD_ARG;
    const long long groups = (K + kGroup - 1) / kGroup;
    if (Lmax > kMaxLen || too_many((long long)T * B) || too_many((long long)B * groups)) return ASR_ERR_UNSUPPORTED;
    Workspace w = carve(workspace, T, B, U);
    if (workspace_bytes < w.bytes) return ASR_ERR_WORKSPACE;
    State s = carve_state(state, B, K, Lmax, 3);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(rows_kernel, dim3(T * B), dim3(256), 0, stream, logits, lengths, uniq, T, B, V, U, blank,
                       state ? s.consumed : nullptr, w.xmax, w.xblank, w.xg, w.base, fill);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gram_sweep_kernel, dim3((unsigned)(B * groups)), dim3(kGroup * 64), 0, stream, w.xmax, w.xblank, w.xg, lengths,
                       node_uni, node_big, kw_len, w.base, T, B, U, K, Lmax, state ? s.val : nullptr, state ? s.start : nullptr,
                       det, det_start);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_kws_hits(void* stream_,const float* det, const int32_t* det_start, const float* fill, const int32_t* lengths,
                            int B, int K, int T, int max_hits, float min_score, int32_t* hit_start, int32_t* hit_end,
                            float* hit_score, float* hit_logp, int32_t* n_hits) {
    if (!det || !det_start || !fill || !hit_start || !hit_end || !hit_score || !hit_logp || !n_hits) return ASR_ERR_BAD_ARG;
    if (B <= 0 || K <= 0 || T <= 0 || max_hits <= 0) return ASR_ERR_BAD_ARG;
    if (max_hits > kMaxHits || too_many((long long)B * K)) return ASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(hits_kernel, dim3(B * K), dim3(256), sizeof(int) * 2 * (size_t)max_hits, (hipStream_t)stream_, det,
                       det_start, fill, lengths, K, T, max_hits, min_score, hit_start, hit_end, hit_score, hit_logp, n_hits);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
