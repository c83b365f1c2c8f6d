// CTC prefix beam search on the GPU (gfx950): the N most probable labellings of every utterance, with their log-probabilities.
//
// The reference decodes greedily only (xp.argmax + the collapse loop: run/ctc/cnn/dev.py:102-106, run/ctc/cnn/test.py:102;
// csrc/decode.hip here).  This is the standard prefix beam search in log space, in two passes:
//
// cand_kernel : one wave per (t, b) row of the (T, B, V) f32 logits, like argmax_rows_kernel; the row is read once.  Writes the
//               row's log-sum-exp, lp[blank] and the top_k non-blank (id, lp) pairs in rank order (value descending, lower id on
//               equal values), cut where lp < min_logp.  Each lane keeps the 4 best of its stripe in registers; the wave pops the
//               best lane head top_k times, and a lane whose 4 were all taken rescans its stripe (L2-hot) for the next 4.
// beam_kernel : one workgroup per utterance, sequential over frames t < lengths[b].  The beam (label prefixes with pb / pnb, a
//               64-bit prefix hash, length, last token and the hash / last token of the parent prefix) and the frame's
//               m + m * n scored entries (stays first, then extensions in (parent rank, candidate rank) order) live in LDS.
//               An extension h + c that is already a beam prefix is merged into that stay: the stay finds its parent in the
//               beam by (hash, length, last token).  The best beam_width entries (ties: earlier canonical position) are found
//               by a radix select on the scores (8 bits per pass); each extension that survives becomes a node (parent node,
//               token) of the utterance's prefix table in the workspace, and a final backtrack writes the N-best ids.  The next
//               frame's candidate row and repeat-stay logits are loaded one frame ahead.
//               beam_kernel<LM, BIAS>: with a language model (section 17) and / or contextual phrase biasing (section 22) in the
//               ranking; beam_kernel<false, false> is the search described here.
// gram_beam_kernel : the same frame loop for the Gram-CTC inventory, over spelled strings (the end of this file).
//               gram_beam_kernel<LM, BIAS, MODE>: with a character language model (section 20) and / or phrase biasing over the
//               spelled characters (section 32); resumable like beam_kernel (section 26).
// Integer atomics only, on LDS histograms: the same inputs give bitwise the same outputs on every launch.
#include "common.hpp"
#include "ngram.hpp"
#include "ctxgraph.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace beam {

constexpr int MAX_BEAM = 128, MAX_TOPK = 64, MAX_EXT = 4096;      // beam_width, top_k, beam_width * top_k
constexpr int MAX_ENTRIES = MAX_BEAM + MAX_EXT;
constexpr int THREADS = 256;
constexpr int NONE = 0x7fffffff;

struct Ws {
    float* lse;         // (T * B)           row log-sum-exp
    float* lpb;         // (T * B)           lp[blank]
    int* n;             // (T * B)           number of candidates kept
    int* cid;           // (T * B, K)        candidate ids in rank order
    float* clp;         // (T * B, K)        their log-probabilities
    int2* node;         // (B, T * W)        prefix table: (parent node or -1, token)
};

__host__ __device__ inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// the layout functions' step: `field` gets the next piece of `bytes` (rounded up to 256) at base + off
template <class P>
__host__ __device__ inline void take(P*& field, char* base, size_t& off, size_t bytes) {
    field = (P*)(base + off);
    off += align256(bytes);
}

// K = min(top_k, V - 1): the candidates a row can have.  -> the bytes; fills *ws if there is one
__host__ __device__ inline size_t ws_layout(int T, int B, int W, int K, char* base, Ws* ws) {
    Ws sizing;
    Ws& w = ws ? *ws : sizing;
    const size_t rows = (size_t)T * B;
    size_t off = 0;
    take(w.lse, base, off, rows * 4);
    take(w.lpb, base, off, rows * 4);
    take(w.n, base, off, rows * 4);
    take(w.cid, base, off, rows * K * 4);
    take(w.clp, base, off, rows * K * 4);
    take(w.node, base, off, rows * W * 8);
    return off;
}

// (v, i) ranks before (w, j): larger value first, lower id on equal values (a total order on non-NaN f32)
__device__ inline bool before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

struct Top4 {
    float v[4];
    int i[4];
};

__device__ inline void top4_clear(Top4& s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { s.v[k] = -INFINITY; s.i[k] = NONE; }
}

// ids arrive in increasing order within a lane
__device__ inline void top4_insert(Top4& s, float x, int id) {
    if (!before(x, id, s.v[3], s.i[3])) return;
    s.v[3] = x;
    s.i[3] = id;
#pragma unroll
    for (int k = 3; k > 0; --k) {
        if (before(s.v[k], s.i[k], s.v[k - 1], s.i[k - 1])) {
            const float tv = s.v[k]; s.v[k] = s.v[k - 1]; s.v[k - 1] = tv;
            const int ti = s.i[k]; s.i[k] = s.i[k - 1]; s.i[k - 1] = ti;
        }
    }
}

template <int CTRL>
__device__ inline void best_dpp(float& v, int& i) {
    const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
    const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, false);
    if (before(ov, oi, v, i)) { v = ov; i = oi; }
}

// the best (v, i) of the wave in every lane: within rows of 16 lanes by DPP (quad swaps, half-row and row mirrors), then two
// cross-row shuffles -- the selection's serial step, so two LDS round trips instead of six
__device__ inline void wave_best(float& v, int& i) {
    best_dpp<0xB1>(v, i);       // quad_perm [1, 0, 3, 2]
    best_dpp<0x4E>(v, i);       // quad_perm [2, 3, 0, 1]
    best_dpp<0x141>(v, i);      // row_half_mirror
    best_dpp<0x140>(v, i);      // row_mirror
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (before(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// the 4 best non-blank elements of this lane's stripe that rank after (av, ai); with LSE also the lane's (max, sum exp)
template <bool LSE>
__device__ inline void scan_stripe(const float* __restrict__ p, int V, int blank, int lane, float av, int ai, Top4& s, float& m,
                                   float& sum) {
    top4_clear(s);
    auto take = [&](float f, int v) {
        if (LSE) {
            const float hi = fmaxf(m, f), lo = fminf(m, f);
            const float e = lo == -INFINITY ? 0.f : __expf(lo - hi);
            sum = f > m ? sum * e + 1.f : sum + e;
            m = hi;
        }
        if (v != blank && before(av, ai, f, v)) top4_insert(s, f, v);
    };
    int v = lane;
    for (; v + 64 * 7 < V; v += 64 * 8) {
        float f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = p[v + 64 * k];
#pragma unroll
        for (int k = 0; k < 8; ++k) take(f[k], v + 64 * k);
    }
    for (; v < V; v += 64) take(p[v], v);
}

__global__ __launch_bounds__(256) void cand_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths, int T, int B,
                                                   int V, int blank, int K, float min_logp, Ws ws) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + wave;       // row = t * B + b
    if (row >= (long long)T * B) return;
    const int t = (int)(row / B), b = (int)(row - (long long)t * B);
    if (lengths && t >= lengths[b]) return;                        // frames past the utterance are never read
    const float* p = x + row * V;
    Top4 s;
    float m = -INFINITY, sum = 0.f;
    scan_stripe<true>(p, V, blank, lane, INFINITY, -1, s, m, sum);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(m, off), os = __shfl_xor(sum, off);
        const float hi = fmaxf(m, om);
        if (hi != -INFINITY) sum = (m == -INFINITY ? 0.f : sum * __expf(m - hi)) + (om == -INFINITY ? 0.f : os * __expf(om - hi));
        m = hi;
    }
    const float lse = m + logf(sum);
    int my_id = 0, n = 0, taken = 0;
    float my_lp = 0.f;
    for (int r = 0; r < K; ++r) {
        float bv = s.v[0];
        int bi = s.i[0];
        wave_best(bv, bi);
        if (bi == NONE) break;                       // fewer than K orderable elements (NaN rows)
        const float lp = bv - lse;
        if (lp < min_logp) break;                    // ranks are by value: the rest are below the threshold too
        if (lane == r) { my_id = bi; my_lp = lp; }
        n = r + 1;
        if (s.i[0] == bi) {                          // this lane held it: pop
#pragma unroll
            for (int k = 0; k < 3; ++k) { s.v[k] = s.v[k + 1]; s.i[k] = s.i[k + 1]; }
            s.v[3] = -INFINITY;
            s.i[3] = NONE;
            if (++taken == 4 && r + 1 < K) {        // all 4 taken: the next 4 of the stripe, after the one just taken
                taken = 0;
                float dm = 0.f, ds = 0.f;
                scan_stripe<false>(p, V, blank, lane, bv, bi, s, dm, ds);
            }
        }
    }
    if (lane < n) {
        ws.cid[row * K + lane] = my_id;
        ws.clp[row * K + lane] = my_lp;
    }
    if (lane == 0) {
        ws.lse[row] = lse;
        ws.lpb[row] = p[blank] - lse;
        ws.n[row] = n;
    }
}

__device__ inline float lae(float a, float b) {       // log(exp(a) + exp(b))
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    if (lo == -INFINITY) return hi;
    return hi + log1pf(expf(lo - hi));
}

__device__ inline unsigned long long fin64(unsigned long long z) {   // splitmix64 finaliser (a bijection)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr unsigned long long ROOT_HASH = 0x9E3779B97F4A7C15ull;

// hash of the prefix h + c from the hash of h
__device__ inline unsigned long long hash_append(unsigned long long h, int c) {
    return fin64(fin64(h) ^ (unsigned long long)(unsigned)(c + 1));
}

// larger score -> larger key; NaN and -inf entries are not valid and never get here
__device__ inline unsigned order_key(float f) {
    const unsigned u = __float_as_uint(f + 0.f);          // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline bool valid(float f) { return f > -INFINITY; }     // false for -inf and NaN

struct Beam {
    float pb[MAX_BEAM], pnb[MAX_BEAM];
    unsigned long long hash[MAX_BEAM], phash[MAX_BEAM];       // prefix hash, hash of the prefix without its last token
    int len[MAX_BEAM], last[MAX_BEAM], plast[MAX_BEAM], node[MAX_BEAM];   // last = -1 for the empty prefix
    float xl[MAX_BEAM];                                         // the logit of `last` in the frame the beam goes into
};

// exclusive scan over the workgroup's 256 threads (wsum: 4 ints of LDS); *total = the sum over all threads
__device__ inline int block_excl_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before_me = 0;
    for (int w = 0; w < wave; ++w) before_me += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return before_me + incl - v;
}

// the rank of entry tid among v[0, n): score descending, ties to the lower index
__device__ inline int rank_of(const float* v, int n, float f, int tid) {
    int rank = 0;
    for (int u = 0; u < n; ++u) {
        const float g2 = v[u];
        rank += g2 > f || (g2 == f && u < tid);
    }
    return rank;
}

// The language-model side of the fused search (asr_ctc_beam_search_lm): beam_kernel<true, .> ranks by
// total + (alpha * lm + beta * len); beam_kernel<false, .> carries none of this and is the unfused search as it was.
template <bool LM>
struct Fuse {};                                                  // kernel arguments

template <>
struct Fuse<true> {
    ngram::Lm lm;
    int bos, eos;
    float alpha, beta;
    float* out_ctc;
    float* out_lm;
};

template <bool LM>
struct FuseLds {};

template <>
struct FuseLds<true> {
    float lm[2][MAX_BEAM];                                       // lm(h) of the beam's prefixes
    int c0[2][MAX_BEAM], c1[2][MAX_BEAM], c2[2][MAX_BEAM];       // their last tokens, newest first (-1: none), from (bos)
    float step[MAX_EXT];                                         // log P(c | context of the parent) of the frame's extensions
};

// The phrase-biasing side of asr_ctc_beam_search_bias: beam_kernel<LM, true> adds bias_open(h) to the ranking
// of either search; beam_kernel<LM, false> carries none of this.  Per prefix: bias_open and the automaton state, both fixed when
// the prefix enters the beam.  Nothing is kept per extension: a frame's m * n look-ups give the ranking its deltas, and the
// <= beam_width extensions that survive repeat theirs (the same loads, so the same bits) for the delta and the next state.
template <bool BIAS>
struct Bias {};                                                  // kernel arguments

template <>
struct Bias<true> {
    ctx::Graph g;
    float* out_ctc;
    float* out_lm;
    float* out_bias;
};

template <bool BIAS>
struct BiasLds {};

template <>
struct BiasLds<true> {
    float open[2][MAX_BEAM];                                     // bias_open(h) of the beam's prefixes
    int state[2][MAX_BEAM];                                      // their automaton states
};

// The resumable search (asr_ctc_beam_stream_*): the beam between two chunks of frames lives in a State in
// device memory.  beam_kernel<., ., ADVANCE> loads it instead of the root, runs the frame loop over the chunk and stores it back;
// beam_kernel<., ., RESULT> loads it and runs the tail only (end terms, final order, backtrack) without storing anything;
// beam_kernel<., ., ONESHOT> carries none of this and is the one-shot search as it was.
constexpr int ONESHOT = 0, ADVANCE = 1, RESULT = 2;
constexpr int STATE_MAGIC = 0x43424d53;
constexpr int HDR_WORDS = 8;      // per utterance: magic, B, beam_width, max_frames, variant, m, table rows in use, tokens committed
constexpr int H_MAGIC = 0, H_B = 1, H_W = 2, H_F = 3, H_VARIANT = 4, H_M = 5, H_FRAMES = 6, H_COMMITTED = 7;
// H_FRAMES is the frames consumed until the first commit (commit_kernel below); H_COMMITTED is 0 until then

struct State {
    int* hdr;                                        // (B, HDR_WORDS)
    float* pb;                                       // (B, W) each: the beam's fields as Beam keeps them, slot-major per utterance
    float* pnb;
    unsigned long long* hash;
    unsigned long long* phash;
    int* len;
    int* last;
    int* plast;
    int* node;
    float* lm;                                       // with a model: FuseLds' fields
    int* c0;
    int* c1;
    int* c2;
    float* open;                                     // with a graph: BiasLds' fields
    int* state;
    int2* table;                                     // (B, max_frames * W) prefix table
};

// F = max_frames; variant = with_lm | with_bias << 1
__host__ __device__ inline size_t state_layout(int B, int W, int F, int variant, char* base, State* s) {
    State sizing;
    State& w = s ? *s : sizing;
    w = State{};                                     // the fields of a side the variant does not have stay null
    const size_t slots = (size_t)B * W;
    size_t off = 0;
    take(w.hdr, base, off, (size_t)B * HDR_WORDS * 4);
    take(w.pb, base, off, slots * 4);
    take(w.pnb, base, off, slots * 4);
    take(w.hash, base, off, slots * 8);
    take(w.phash, base, off, slots * 8);
    take(w.len, base, off, slots * 4);
    take(w.last, base, off, slots * 4);
    take(w.plast, base, off, slots * 4);
    take(w.node, base, off, slots * 4);
    if (variant & 1) {
        take(w.lm, base, off, slots * 4);
        take(w.c0, base, off, slots * 4);
        take(w.c1, base, off, slots * 4);
        take(w.c2, base, off, slots * 4);
    }
    if (variant & 2) {
        take(w.open, base, off, slots * 4);
        take(w.state, base, off, slots * 4);
    }
    take(w.table, base, off, slots * F * 8);
    return off;
}

struct StrmArgs {
    State s;
    int max_frames, variant;
    int32_t* out_frames;                             // RESULT only
};

template <int MODE>
struct Strm : StrmArgs {};                           // kernel arguments

template <>
struct Strm<ONESHOT> {};

// the header of utterance b was written for these dimensions and this variant
__device__ inline bool state_matches(const int* h, int B, int W, int F, int variant) {
    return h[H_MAGIC] == STATE_MAGIC && h[H_B] == B && h[H_W] == W && h[H_F] == F && h[H_VARIANT] == variant;
}

// What a streaming kernel reads from the header of utterance b (hdr: that utterance's words) before it loads the beam: the beam's
// size m, the frames consumed so far f0 and the frames this call may consume len_b, all clamped so that a header other code
// wrote into cannot lead outside the state; a header that does not match gives m = 0.  ADVANCE: len_b <= 0 means there is
// nothing to consume, and the caller returns without touching the state.  RESULT: len_b = 0, and out_frames[b] = f0 or -1.
// Returns the utterance's prefix table: `per_frame` nodes per frame and beam slot (1, Gram-CTC 2).
struct StrmHead {
    int2* nodes;
    int m, f0, len_b;
};

template <int MODE>
__device__ inline StrmHead stream_begin(const int* hdr, int2* table, int per_frame, int B, int W, int F, int variant,
                                        int32_t* out_frames, int b, int len_b) {
    const bool ok = state_matches(hdr, B, W, F, variant);
    StrmHead r;
    r.nodes = table + (size_t)b * per_frame * F * W;
    r.m = ok ? min(max(hdr[H_M], 0), W) : 0;
    r.f0 = ok ? min(max(hdr[H_FRAMES], 0), F) : 0;
    if constexpr (MODE == ADVANCE) {
        r.len_b = ok ? min(len_b, F - r.f0) : 0;            // no node beyond the table, whatever the host says
    } else {
        r.len_b = 0;
        if (threadIdx.x == 0) out_frames[b] = ok ? r.f0 : -1;
    }
    return r;
}

// ADVANCE's last step: the beam's size and the frames consumed go back into the header
__device__ inline void stream_end(int* hdr, int m, int frames) {
    if (threadIdx.x == 0) {
        hdr[H_M] = m;
        hdr[H_FRAMES] = frames;
    }
}

// The two halves of every N-best tail; the caller's own writes for the slot sit between them.
// fill_blank: in the utterance's ids, rows of `pitch`, the positions from a hypothesis' length on get blank; row i < m is beam slot
// order[i] (slot i with no order), the rows from m on are all blank.  `c`: the utterance's committed tokens, which the rows leave out.
__device__ inline void fill_blank(int32_t* ids, int pitch, int W, int m, const int* len, const int* order, int blank, int c) {
    for (size_t k = threadIdx.x; k < (size_t)W * pitch; k += THREADS) {
        const int i = (int)(k / pitch), p = (int)(k - (size_t)i * pitch);
        if (p >= (i < m ? len[order ? order[i] : i] - c : 0)) ids[k] = blank;
    }
}

// RESULT after a commit: the tokens a hypothesis of length `len` has beyond the utterance's `c` committed ones, which is what its
// chain in the prefix table holds and what result returns; c is 0 in the other modes and in a stream that never committed.
template <int MODE>
__device__ inline int tail_len(int len, int c) {
    return MODE == RESULT ? max(len - c, 0) : len;
}

// walk_chain: one hypothesis of length L walks its prefix table chain from node nd back to the root and writes its row of ids.
// RESULT: a hypothesis longer than the row is cut (its length is reported in full), and a chain that leaves the table's table_n
// nodes (a state that other code wrote into) ends there.
template <int MODE>
__device__ inline void walk_chain(int32_t* row, int pitch, int L, int nd, const int2* nodes, int table_n) {
    for (int p = L - 1; p >= 0; --p) {
        if (MODE == RESULT && (unsigned)nd >= (unsigned)table_n) break;
        const int2 e = nodes[nd];
        if (MODE != RESULT || p < pitch) row[p] = e.y;
        nd = e.x;
    }
}

// ADVANCE: x, lengths and T are the chunk's (Tc frames, lengths[b] of them valid), ws holds the chunk's candidate rows and the
// outputs are unused.  RESULT: x, lengths and ws are unused, T is the ids' row pitch (Lcap).
template <bool LM, bool BIAS, int MODE>
__global__ __launch_bounds__(THREADS) void beam_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths, int T, int B,
                                                       int V, int W, int K, int blank, Ws ws, int32_t* __restrict__ out_ids,
                                                       int32_t* __restrict__ out_len, float* __restrict__ out_score, Fuse<LM> fz,
                                                       Bias<BIAS> bz, Strm<MODE> sz) {
    __shared__ Beam bm[2];
    __shared__ FuseLds<LM> fl;
    __shared__ BiasLds<BIAS> bl;
    __shared__ float tot[MAX_ENTRIES];                 // scores of the frame's entries in canonical order
    __shared__ float btot[MAX_BEAM], spb[MAX_BEAM], spnb[MAX_BEAM];
    __shared__ int par[MAX_BEAM], cnd[MAX_BEAM];      // a stay's parent prefix (beam slot) and the candidate rank of its last token
    __shared__ int cid[MAX_TOPK];
    __shared__ float clp[MAX_TOPK];
    __shared__ unsigned hist[2][256];
    __shared__ float sv_tot[MAX_BEAM];
    __shared__ int sv_pos[MAX_BEAM];
    __shared__ float xnext[MAX_BEAM + MAX_TOPK];       // next frame's logits of the beam's last tokens, then of the candidates
    __shared__ int wsum[4];
    __shared__ int s_digit, s_need, s_all, s_done;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int len_b = lengths ? min(max(lengths[b], 0), T) : T;
    int2* nodes;
    int cur = 0, m = 1, f0 = 0;                        // f0: the frames this utterance consumed before this call
    if constexpr (MODE != ONESHOT) {
        const StrmHead hd = stream_begin<MODE>(sz.s.hdr + (size_t)b * HDR_WORDS, sz.s.table, 1, B, W, sz.max_frames, sz.variant,
                                               sz.out_frames, b, len_b);
        nodes = hd.nodes; m = hd.m; f0 = hd.f0; len_b = hd.len_b;
        if (MODE == ADVANCE && len_b <= 0) return;     // nothing to consume: the state is not touched
        if (tid < m) {
            const size_t i = (size_t)b * W + tid;
            const int last = sz.s.last[i], len = sz.s.len[i];
            bm[0].pb[tid] = sz.s.pb[i];
            bm[0].pnb[tid] = sz.s.pnb[i];
            bm[0].hash[tid] = sz.s.hash[i];
            bm[0].phash[tid] = sz.s.phash[i];
            bm[0].len[tid] = len;
            bm[0].last[tid] = last;
            bm[0].plast[tid] = sz.s.plast[i];
            bm[0].node[tid] = sz.s.node[i];
            if constexpr (LM) {
                fl.lm[0][tid] = sz.s.lm[i];
                fl.c0[0][tid] = sz.s.c0[i];
                fl.c1[0][tid] = sz.s.c1[i];
                fl.c2[0][tid] = sz.s.c2[i];
            }
            if constexpr (BIAS) {
                bl.open[0][tid] = sz.s.open[i];
                bl.state[0][tid] = sz.s.state[i];
            }
            // the logit of the prefix's last token in the chunk's first frame: the value the one-shot loop loads one frame ahead
            if constexpr (MODE == ADVANCE)
                bm[0].xl[tid] = len > 0 && (unsigned)last < (unsigned)V ? x[(size_t)b * V + last] : 0.f;
        }
    } else {
        nodes = ws.node + (size_t)b * T * W;
    }
    if (MODE == ONESHOT && tid == 0) {
        bm[0].pb[0] = 0.f;
        bm[0].pnb[0] = -INFINITY;
        bm[0].hash[0] = ROOT_HASH;
        bm[0].phash[0] = 0;
        bm[0].len[0] = 0;
        bm[0].last[0] = -1;
        bm[0].plast[0] = -2;
        bm[0].node[0] = -1;
        if constexpr (LM) {
            fl.lm[0][0] = 0.f;
            fl.c0[0][0] = fz.bos;
            fl.c1[0][0] = -1;
            fl.c2[0][0] = -1;
        }
        if constexpr (BIAS) {
            bl.open[0][0] = 0.f;
            bl.state[0][0] = 0;
        }
    }
    // a frame's candidate row, loaded one frame ahead so that its latency stays off the serial path
    int q_n = 0, q_id = 0;
    float q_lse = 0.f, q_lpb = 0.f, q_lp = 0.f;
    auto load_row = [&](int t) {
        const size_t row = (size_t)t * B + b;
        q_n = ws.n[row];
        q_lse = ws.lse[row];
        q_lpb = ws.lpb[row];
        if (tid < K) {                                 // entries past n are never used
            q_id = ws.cid[row * K + tid];
            q_lp = ws.clp[row * K + tid];
        }
    };
    if (len_b > 0) load_row(0);
    __syncthreads();
    for (int t = 0; MODE != RESULT && t < len_b; ++t) {
        const Beam& o = bm[cur];
        Beam& nx = bm[cur ^ 1];
        const int n = min(q_n, K);
        const float lse = q_lse, lpb = q_lpb;
        // A: the frame's candidates
        if (tid < n) {
            cid[tid] = q_id;
            clp[tid] = q_lp;
        }
        if (tid < m) {
            btot[tid] = lae(o.pb[tid], o.pnb[tid]);
            par[tid] = -1;
            cnd[tid] = -1;
        }
        hist[0][tid] = 0;
        __syncthreads();
        // issue the next frame's loads now; they land during this frame's work: its candidate row, and the logit of every
        // token that can end a prefix after this frame (the beam's last tokens and this frame's candidates), for the repeat stays
        float gx = 0.f;
        if (t + 1 < len_b) {
            load_row(t + 1);
            const float* xr = x + ((size_t)(t + 1) * B + b) * V;
            if (tid < m) {
                if (o.len[tid] > 0) gx = xr[o.last[tid]];
            } else if (tid < m + n) {
                gx = xr[cid[tid - m]];
            }
        }
        // B: extension scores; for every non-empty stay, its parent prefix in the beam (by hash, length and last token) and the
        // candidate rank of its last token -- the extension of that parent which equals the stay's prefix
        const int E = m + m * n;
        ngram::Step st;
        ctx::Step cs;
        if constexpr (LM || BIAS) {
            // the m * n step look-ups, one or more per thread: the first one's loads are started here and are in flight during
            // the parent / candidate matching below
            if (m + tid < E) {
                const int j = tid / n, r = tid - j * n;
                if constexpr (LM) st = ngram::step_issue(fz.lm, fl.c0[cur][j], fl.c1[cur][j], fl.c2[cur][j], cid[r]);
                if constexpr (BIAS) cs = ctx::step_issue(bz.g, bl.state[cur][j], cid[r]);
            }
        } else {
            for (int e = m + tid; e < E; e += THREADS) {
                const int q = e - m, j = q / n, r = q - j * n;
                const float base = o.last[j] == cid[r] ? o.pb[j] : btot[j];
                tot[e] = base + clp[r];
            }
        }
        for (int p = tid; p < m * m; p += THREADS) {
            const int i = p / m, j = p - i * m;
            if (o.len[i] > 0 && o.hash[j] == o.phash[i] && o.len[j] == o.len[i] - 1 && o.last[j] == o.plast[i]) par[i] = j;
        }
        for (int p = tid; p < m * n; p += THREADS) {
            const int i = p / n, r = p - i * n;
            if (o.len[i] > 0 && cid[r] == o.last[i]) cnd[i] = r;
        }
        if constexpr (LM && !BIAS) {
            for (int e = m + tid; e < E; e += THREADS) {
                const int q = e - m, j = q / n, r = q - j * n;
                if (q >= THREADS) st = ngram::step_issue(fz.lm, fl.c0[cur][j], fl.c1[cur][j], fl.c2[cur][j], cid[r]);
                const float s = ngram::step_finish(fz.lm, st);
                fl.step[q] = s;
                const float base = o.last[j] == cid[r] ? o.pb[j] : btot[j];
                tot[e] = (base + clp[r]) + (fz.alpha * (fl.lm[cur][j] + s) + fz.beta * (float)(o.len[j] + 1));
            }
        }
        if constexpr (BIAS) {
            for (int e = m + tid; e < E; e += THREADS) {
                const int q = e - m, j = q / n, r = q - j * n;
                if (q >= THREADS) {
                    if constexpr (LM) st = ngram::step_issue(fz.lm, fl.c0[cur][j], fl.c1[cur][j], fl.c2[cur][j], cid[r]);
                    cs = ctx::step_issue(bz.g, bl.state[cur][j], cid[r]);
                }
                const float base = o.last[j] == cid[r] ? o.pb[j] : btot[j];
                float v = base + clp[r];
                if constexpr (LM) {
                    const float s = ngram::step_finish(fz.lm, st);
                    fl.step[q] = s;
                    v += fz.alpha * (fl.lm[cur][j] + s) + fz.beta * (float)(o.len[j] + 1);
                }
                int unused;
                tot[e] = v + (bl.open[cur][j] + ctx::step_finish(bz.g, cs, &unused));     // + bias_open(h + c)
            }
        }
        __syncthreads();
        // C: stays, merged with that extension (one entry, at the stay's position)
        if (tid < m) {
            const int i = tid, j = par[i], r = cnd[i];
            const float npb = btot[i] + lpb;
            float npnb = o.len[i] > 0 ? o.pnb[i] + (o.xl[i] - lse) : -INFINITY;
            if (j >= 0 && r >= 0) {
                const float base = o.last[j] == o.last[i] ? o.pb[j] : btot[j];
                npnb = lae(npnb, base + clp[r]);
                tot[m + j * n + r] = -INFINITY;
            }
            spb[i] = npb;
            spnb[i] = npnb;
            if constexpr (LM) tot[i] = lae(npb, npnb) + (fz.alpha * fl.lm[cur][i] + fz.beta * (float)o.len[i]);
            else tot[i] = lae(npb, npnb);
            if constexpr (BIAS) tot[i] += bl.open[cur][i];
        }
        __syncthreads();
        // (D and E stand in both kernels, line for line the same: as one __device__ function the pass loop was laid out differently
        // and every frame loop ran 0.5 - 1.7 % slower; a change to one copy belongs in the other too)
        // D: radix select of the W best valid entries, 8 bits of the key per pass from the top: key >> sh > tau >> sh, and the
        // first `need` (canonical order) with key >> sh == tau >> sh.  It stops early once the boundary digit's entries are all kept.
        const int chunk = (E + THREADS - 1) / THREADS, e0 = min(E, tid * chunk), e1 = min(E, e0 + chunk);
        unsigned prefix = 0;
        int need = W, all = 0, sh = 0;
        for (int shift = 24, pass = 0; shift >= 0; shift -= 8, ++pass) {
            unsigned* h = hist[pass & 1];
            hist[(pass + 1) & 1][tid] = 0;           // the next pass's histogram; the last reader of it was the pass before
            for (int e = e0; e < e1; ++e) {
                const float f = tot[e];
                if (!valid(f)) continue;
                const unsigned key = order_key(f);
                if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&h[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) {
                int c[4], sum = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { c[k] = (int)h[255 - 4 * lane - k]; sum += c[k]; }
                int incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int u = __shfl_up(incl, off);
                    if (lane >= off) incl += u;
                }
                const int count = __shfl(incl, 63);
                if (shift == 24 && count <= W) {
                    if (lane == 0) s_all = 1;
                } else {
                    if (lane == 0) s_all = 0;
                    const unsigned long long hit = __ballot(incl >= need);
                    const int L = __ffsll((long long)hit) - 1;
                    if (lane == L) {
                        int acc = incl - sum;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (acc + c[k] >= need) {
                                s_digit = 255 - 4 * lane - k;
                                s_need = need - acc;
                                s_done = acc + c[k] == need;
                                break;
                            }
                            acc += c[k];
                        }
                    }
                }
            }
            __syncthreads();
            if (s_all) { all = 1; break; }
            prefix |= (unsigned)s_digit << shift;
            need = s_need;
            sh = shift;
            if (s_done) break;          // (s_digit / s_need / s_done are rewritten after the next pass's first barrier)
        }
        const unsigned tau = all ? 0u : prefix;
        const int need_eq = all ? 0 : need;
        // E: compact the kept entries in canonical order
        int gt = 0, eq = 0;
        for (int e = e0; e < e1; ++e) {
            const float f = tot[e];
            if (!valid(f)) continue;
            const unsigned key = order_key(f) >> sh;
            gt += key > tau >> sh;
            eq += key == tau >> sh;
        }
        int packed_total;
        const int packed = block_excl_scan((gt << 16) | eq, wsum, &packed_total);
        int g = packed >> 16, q = packed & 0xffff;
        for (int e = e0; e < e1; ++e) {
            const float f = tot[e];
            if (!valid(f)) continue;
            const unsigned key = order_key(f) >> sh;
            int slot = -1;
            if (key > tau >> sh) slot = g + min(q, need_eq), ++g;
            else if (key == tau >> sh) { if (q < need_eq) slot = g + q; ++q; }
            if (slot >= 0) { sv_pos[slot] = e; sv_tot[slot] = f; }
        }
        const int M = (packed_total >> 16) + min(packed_total & 0xffff, need_eq);
        if (tid < m + n) xnext[tid] = gx;
        __syncthreads();
        // F: rank the survivors (score descending, canonical position on ties) into the next beam
        if (tid < M) {
            const float f = sv_tot[tid];
            const int e = sv_pos[tid];
            if constexpr (BIAS) {
                // a surviving extension looks its step up again, for the delta and the next state; the loads fly during the count
                if (e >= m) cs = ctx::step_issue(bz.g, bl.state[cur][(e - m) / n], cid[(e - m) % n]);
            }
            const int rank = rank_of(sv_tot, M, f, tid);
            if (e < m) {
                nx.pb[rank] = spb[e];
                nx.pnb[rank] = spnb[e];
                nx.hash[rank] = o.hash[e];
                nx.phash[rank] = o.phash[e];
                nx.len[rank] = o.len[e];
                nx.last[rank] = o.last[e];
                nx.plast[rank] = o.plast[e];
                nx.node[rank] = o.node[e];
                nx.xl[rank] = xnext[e];
                if constexpr (LM) {
                    fl.lm[cur ^ 1][rank] = fl.lm[cur][e];
                    fl.c0[cur ^ 1][rank] = fl.c0[cur][e];
                    fl.c1[cur ^ 1][rank] = fl.c1[cur][e];
                    fl.c2[cur ^ 1][rank] = fl.c2[cur][e];
                }
                if constexpr (BIAS) {
                    bl.open[cur ^ 1][rank] = bl.open[cur][e];
                    bl.state[cur ^ 1][rank] = bl.state[cur][e];
                }
            } else {
                const int q2 = e - m, j = q2 / n, r = q2 - j * n, c = cid[r];
                const int id = (MODE == ADVANCE ? f0 + t : t) * W + rank;
                nx.pb[rank] = -INFINITY;
                if constexpr (LM) {
                    // f is the ranking score here; the CTC score is phase B's sum again, bit for bit
                    nx.pnb[rank] = (o.last[j] == c ? o.pb[j] : btot[j]) + clp[r];
                    fl.lm[cur ^ 1][rank] = fl.lm[cur][j] + fl.step[q2];
                    fl.c0[cur ^ 1][rank] = c;
                    fl.c1[cur ^ 1][rank] = fl.c0[cur][j];
                    fl.c2[cur ^ 1][rank] = fl.c1[cur][j];
                } else if constexpr (BIAS) {
                    nx.pnb[rank] = (o.last[j] == c ? o.pb[j] : btot[j]) + clp[r];
                } else {
                    nx.pnb[rank] = f;
                }
                if constexpr (BIAS) {
                    int next;
                    bl.open[cur ^ 1][rank] = bl.open[cur][j] + ctx::step_finish(bz.g, cs, &next);
                    bl.state[cur ^ 1][rank] = next;
                }
                nx.hash[rank] = hash_append(o.hash[j], c);
                nx.phash[rank] = o.hash[j];
                nx.len[rank] = o.len[j] + 1;
                nx.last[rank] = c;
                nx.plast[rank] = o.last[j];
                nx.node[rank] = id;
                nx.xl[rank] = xnext[m + r];
                nodes[id] = make_int2(o.node[j], c);
            }
        }
        __syncthreads();
        cur ^= 1;
        m = M;
    }
    __threadfence();
    __syncthreads();
    const Beam& o = bm[cur];
    if constexpr (MODE == ADVANCE) {
        // the beam goes back where it came from; slots past m keep what they held
        if (tid < m) {
            const size_t i = (size_t)b * W + tid;
            sz.s.pb[i] = o.pb[tid];
            sz.s.pnb[i] = o.pnb[tid];
            sz.s.hash[i] = o.hash[tid];
            sz.s.phash[i] = o.phash[tid];
            sz.s.len[i] = o.len[tid];
            sz.s.last[i] = o.last[tid];
            sz.s.plast[i] = o.plast[tid];
            sz.s.node[i] = o.node[tid];
            if constexpr (LM) {
                sz.s.lm[i] = fl.lm[cur][tid];
                sz.s.c0[i] = fl.c0[cur][tid];
                sz.s.c1[i] = fl.c1[cur][tid];
                sz.s.c2[i] = fl.c2[cur][tid];
            }
            if constexpr (BIAS) {
                sz.s.open[i] = bl.open[cur][tid];
                sz.s.state[i] = bl.state[cur][tid];
            }
        }
        stream_end(sz.s.hdr + (size_t)b * HDR_WORDS, m, f0 + len_b);
        return;
    }
    // the N-best, sorted by score: the ids by fill_blank and walk_chain (RESULT: a hypothesis longer than the row pitch is cut there, and its
    // length is reported in full)
    int table_n = 0, cm = 0;                           // cm: the committed tokens (RESULT only)
    if constexpr (MODE == RESULT) {
        table_n = sz.max_frames * W;
        if (m > 0) cm = max(sz.s.hdr[(size_t)b * HDR_WORDS + H_COMMITTED], 0);
    }
    int32_t* ids = out_ids + (size_t)b * W * T;
    if constexpr (LM || BIAS) {
        // the end terms, then the final order: score descending, ties to the earlier slot
        float* o_ctc;
        float* o_lm;
        if constexpr (BIAS) { o_ctc = bz.out_ctc; o_lm = bz.out_lm; }
        else { o_ctc = fz.out_ctc; o_lm = fz.out_lm; }
        float ctc = 0.f, lmv = 0.f, bv = 0.f, sc = 0.f;
        if (tid < m) {
            ctc = lae(o.pb[tid], o.pnb[tid]);
            sc = ctc;
            if constexpr (LM) {
                lmv = fl.lm[cur][tid];
                if (fz.eos >= 0) lmv += ngram::step(fz.lm, fl.c0[cur][tid], fl.c1[cur][tid], fl.c2[cur][tid], fz.eos);
                sc = ctc + (fz.alpha * lmv + fz.beta * (float)o.len[tid]);
            }
            if constexpr (BIAS) {
                bv = bl.open[cur][tid] + bz.g.ret[bl.state[cur][tid]];        // the advance of an unfinished match goes back
                sc += bv;
            }
            sv_tot[tid] = sc;
        }
        __syncthreads();
        if (tid < m) {
            const int rank = rank_of(sv_tot, m, sc, tid);
            sv_pos[rank] = tid;
            out_score[b * W + rank] = sc;
            o_ctc[b * W + rank] = ctc;
            o_lm[b * W + rank] = lmv;
            if constexpr (BIAS) bz.out_bias[b * W + rank] = bv;
        }
        __syncthreads();
        fill_blank(ids, T, W, m, o.len, sv_pos, blank, cm);
        if (tid < W) {
            if (tid < m) {
                const int h = sv_pos[tid], L = tail_len<MODE>(o.len[h], cm);
                out_len[b * W + tid] = L;
                walk_chain<MODE>(ids + (size_t)tid * T, T, L, o.node[h], nodes, table_n);
            } else {
                out_len[b * W + tid] = 0;
                out_score[b * W + tid] = -INFINITY;
                o_ctc[b * W + tid] = -INFINITY;
                o_lm[b * W + tid] = 0.f;
                if constexpr (BIAS) bz.out_bias[b * W + tid] = 0.f;
            }
        }
        return;
    }
    fill_blank(ids, T, W, m, o.len, nullptr, blank, cm);
    if (tid < W) {
        if (tid < m) {
            const int L = tail_len<MODE>(o.len[tid], cm);
            out_len[b * W + tid] = L;
            out_score[b * W + tid] = lae(o.pb[tid], o.pnb[tid]);
            walk_chain<MODE>(ids + (size_t)tid * T, T, L, o.node[tid], nodes, table_n);
        } else {
            out_len[b * W + tid] = 0;
            out_score[b * W + tid] = -INFINITY;
        }
    }
}

// ---------------------------------------------------------------------------------------------- the small kernels
// asr_ngram_score: one workgroup per sequence; a thread scores the positions tid, tid + 256, ...; the sum is the threads' partial sums (each in
// position order) reduced by a fixed tree, so it repeats bitwise
__global__ __launch_bounds__(THREADS) void ngram_score_kernel(ngram::Lm lm, const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ lengths, int Lmax, int bos, int eos,
                                                              float* __restrict__ out_tok, float* __restrict__ out_sum) {
    __shared__ float part[THREADS];
    const int nseq = blockIdx.x, tid = threadIdx.x;
    const int32_t* row = ids + (size_t)nseq * Lmax;
    const int len = lengths ? min(max(lengths[nseq], 0), Lmax) : Lmax;
    auto tok = [&](int i) { return i >= 0 ? row[i] : (i == -1 ? bos : -1); };
    float acc = 0.f;
    for (int p = tid; p < Lmax; p += THREADS) {
        float v = 0.f;
        if (p < len) v = ngram::step(lm, tok(p - 1), tok(p - 2), tok(p - 3), row[p]);
        out_tok[(size_t)nseq * Lmax + p] = v;
        acc += v;
    }
    if (tid == THREADS - 1 && eos >= 0) acc += ngram::step(lm, tok(len - 1), tok(len - 2), tok(len - 3), eos);
    part[tid] = acc;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) out_sum[nseq] = part[0];
}

// asr_ctx_score: one sequence per thread: a step's state comes from the step before it, so a sequence is walked in order; the sum is the
// left-to-right f32 sum of the deltas
__global__ __launch_bounds__(64) void ctx_score_kernel(ctx::Graph g, int V, const int32_t* __restrict__ ids,
                                                       const int32_t* __restrict__ lengths, int N, int Lmax, int finalize,
                                                       float* __restrict__ out_tok, float* __restrict__ out_sum) {
    const int nseq = blockIdx.x * 64 + threadIdx.x;
    if (nseq >= N) return;
    const int32_t* row = ids + (size_t)nseq * Lmax;
    float* tok = out_tok + (size_t)nseq * Lmax;
    const int len = lengths ? min(max(lengths[nseq], 0), Lmax) : Lmax;
    int s = 0;
    float acc = 0.f;
    for (int p = 0; p < len; ++p) {
        const int c = row[p];
        float d;
        if (c < 0 || c >= V) {                          // not a token: NaN, and the match starts over
            d = __int_as_float(0x7fc00000);
            s = 0;
        } else {
            d = ctx::step(g, s, c, &s);
        }
        tok[p] = d;
        acc += d;
    }
    for (int p = len; p < Lmax; ++p) tok[p] = 0.f;
    if (finalize) acc += g.ret[s];
    out_sum[nseq] = acc;
}

// asr_ctc_beam_stream_reset: the header and the root beam (what beam_kernel<., ., ONESHOT> starts from) of every utterance, or of those with mask[b] != 0
__global__ __launch_bounds__(256) void stream_reset_kernel(State s, int B, int W, int F, int variant, int bos,
                                                           const int32_t* __restrict__ mask) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B || (mask && mask[b] == 0)) return;
    int* h = s.hdr + (size_t)b * HDR_WORDS;
    h[H_MAGIC] = STATE_MAGIC;
    h[H_B] = B;
    h[H_W] = W;
    h[H_F] = F;
    h[H_VARIANT] = variant;
    h[H_M] = 1;
    h[H_FRAMES] = 0;
    h[HDR_WORDS - 1] = 0;
    const size_t i = (size_t)b * W;
    s.pb[i] = 0.f;
    s.pnb[i] = -INFINITY;
    s.hash[i] = ROOT_HASH;
    s.phash[i] = 0;
    s.len[i] = 0;
    s.last[i] = -1;
    s.plast[i] = -2;
    s.node[i] = -1;
    if (variant & 1) {
        s.lm[i] = 0.f;
        s.c0[i] = bos;
        s.c1[i] = -1;
        s.c2[i] = -1;
    }
    if (variant & 2) {
        s.open[i] = 0.f;
        s.state[i] = 0;
    }
}

// ------------------------------------------------------------------------------ Gram-CTC: beam search over spelled strings
// asr_gram_ctc_beam_search.  The hypotheses are strings of unigrams; a string carries the mass of the paths
// that end in blank (pb), in the unigram token of its last character (pu) and in the bigram token of its last two (pg), so every
// way of cutting it into unigram and bigram tokens is summed.  cand_kernel is the one above; gram_rows_kernel spells its
// candidates; gram_beam_kernel is beam_kernel's frame loop with three masses, a three-deep identity (the hashes and last
// characters of s, s[:-1] and s[:-2]) and one more merge: two extensions of one frame that spell the same string.

constexpr unsigned short NO_MATE = 0xffff;

// the (V, 2) spelling of every candidate, so that the serial pass gets it with the candidate row instead of chasing the id
__global__ __launch_bounds__(256) void gram_rows_kernel(const int32_t* __restrict__ lengths, int T, int B, int K, Ws ws,
                                                        const int2* __restrict__ gram, int2* __restrict__ cgr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)T * B * K) return;
    const long long row = i / K;
    const int k = (int)(i - row * K), t = (int)(row / B), b = (int)(row - (long long)t * B);
    if (lengths && t >= lengths[b]) return;
    if (k < ws.n[row]) cgr[i] = gram[ws.cid[i]];
}

struct GBeam {
    float pb[MAX_BEAM], pu[MAX_BEAM], pg[MAX_BEAM];
    unsigned long long h0[MAX_BEAM], h1[MAX_BEAM], h2[MAX_BEAM];   // hash of s, of s[:-1], of s[:-2] (0 where s is too short)
    int len[MAX_BEAM], c1[MAX_BEAM], c2[MAX_BEAM], c3[MAX_BEAM];  // s[-1], s[-2], s[-3]; -1 where s is too short
    int utok[MAX_BEAM], gtok[MAX_BEAM];                            // the token ids behind pu and pg; -1 until a candidate named them
    int node[MAX_BEAM];
    float xu[MAX_BEAM], xg[MAX_BEAM];                              // the logits of utok / gtok in the frame the beam goes into
};

__device__ inline float lae3(float a, float b, float c) { return lae(lae(a, b), c); }

// The language-model side of asr_gram_ctc_beam_search_lm: gram_beam_kernel<true> ranks by
// total + (alpha * lm + beta * len) with lm over the string's characters, the arguments being section 17's Fuse<true>;
// gram_beam_kernel<false> carries none of this and is the unfused string search as it was.
template <bool LM>
struct GFuseLds {};

template <>
struct GFuseLds<true> {
    float lm[2][MAX_BEAM];                                       // lm(s) of the beam's strings
    float elm[MAX_EXT];                                          // lm(s + a) or lm(s + a + b) of the frame's extensions
};

// The phrase-biasing side of asr_gram_ctc_beam_search_bias: gram_beam_kernel<., true> adds bias_open(s), the
// arguments being section 22's Bias<true>; gram_beam_kernel<., false> carries none of this.  Per string: bias_open and the
// automaton state, both fixed when the string enters the beam.  Per extension the same two, kept from phase B for phases C1 and F:
// a bigram extension takes two dependent steps, and a survivor that repeated them in phase F would wait for both again.
template <bool BIAS>
struct GBiasLds {};

template <>
struct GBiasLds<true> {
    float open[2][MAX_BEAM];                                     // bias_open(s) of the beam's strings
    int state[2][MAX_BEAM];                                      // their automaton states
    float eopen[MAX_EXT];                                        // bias_open(s + a) or bias_open(s + a + b) of the frame's extensions
    int estate[MAX_EXT];                                         // and the state after them
};

// The model's bonus alpha * lm + beta * len in the two roundings that gram_beam_kernel<true, false, .> is compiled to (with
// -ffp-contract=fast the choice is the compiler's, site by site): both products rounded before the sum in phases B and C2 and in
// the final order, alpha * lm fused into the sum in phase C1.  With a graph without phrases gram_beam_kernel<true, true, .> must
// rank and score exactly as that kernel does, for weights whose products round as well, so it states the choice at every site
// instead of leaving it open (tests/test_gram_ctx_bias_gpu.py compares the two on bytes with alpha = 0.7, beta = 0.4).
__device__ inline float bonus_rounded(float alpha, float lm, float beta, float len) {
    float p = alpha * lm, q = beta * len;
    asm volatile("" : "+v"(p), "+v"(q));                         // the products exist as f32 values: nothing can fuse them
    return p + q;
}

__device__ inline float bonus_fused(float alpha, float lm, float beta, float len) { return __builtin_fmaf(alpha, lm, beta * len); }

// the k-th newest character of the string in beam slot j as a model context: (bos) stands right before the string, nothing
// before that; the identity fields c1 .. c3 keep their -1
__device__ inline int lm_ctx(const GBeam& g, int j, int k, int bos) {
    const int L = g.len[j];
    if (k >= L) return k == L ? bos : -1;
    return k == 0 ? g.c1[j] : (k == 1 ? g.c2[j] : g.c3[j]);
}

// The resumable string search (asr_gram_ctc_beam_stream_*): section 23's scheme for GBeam.  The header has
// the CTC stream's place and words, and its variant word carries GRAM_VARIANT, so that neither family reads the other's state:
// state_matches compares the whole word, and the CTC variants are 0 .. 3.
constexpr int GRAM_VARIANT = 4;

struct GState {
    int* hdr;                                        // (B, HDR_WORDS), as State's
    float* pb;                                       // (B, W) each: the beam's fields as GBeam keeps them, slot-major per utterance
    float* pu;
    float* pg;
    unsigned long long* h0;
    unsigned long long* h1;
    unsigned long long* h2;
    int* len;
    int* c1;
    int* c2;
    int* c3;
    int* utok;
    int* gtok;
    int* node;
    float* lm;                                       // with a model: GFuseLds' lm
    int2* table;                                     // (B, 2 * max_frames * W) prefix table
};

// With a graph the state also holds GBiasLds' open and state, (B, W) each, between lm and the table.  They travel in a struct
// of their own, after the other kernel arguments, so that the kernels without a graph keep their argument block.
struct GBiasState {
    float* open;
    int* state;
};

// F = max_frames; variant = GRAM_VARIANT | with_lm | with_bias << 1
__host__ __device__ inline size_t gram_state_layout(int B, int W, int F, int variant, char* base, GState* s,
                                                    GBiasState* bs = nullptr) {
    GState sizing;
    GState& w = s ? *s : sizing;
    w = GState{};                                    // the fields of a side the variant does not have stay null
    const size_t slots = (size_t)B * W;
    size_t off = 0;
    take(w.hdr, base, off, (size_t)B * HDR_WORDS * 4);
    take(w.pb, base, off, slots * 4);
    take(w.pu, base, off, slots * 4);
    take(w.pg, base, off, slots * 4);
    take(w.h0, base, off, slots * 8);
    take(w.h1, base, off, slots * 8);
    take(w.h2, base, off, slots * 8);
    take(w.len, base, off, slots * 4);
    take(w.c1, base, off, slots * 4);
    take(w.c2, base, off, slots * 4);
    take(w.c3, base, off, slots * 4);
    take(w.utok, base, off, slots * 4);
    take(w.gtok, base, off, slots * 4);
    take(w.node, base, off, slots * 4);
    if (variant & 1) take(w.lm, base, off, slots * 4);
    GBiasState g{};
    if (variant & 2) {
        take(g.open, base, off, slots * 4);
        take(g.state, base, off, slots * 4);
    }
    if (bs) *bs = g;
    take(w.table, base, off, slots * F * 16);
    return off;
}

struct GStrmArgs {
    GState s;
    int max_frames, variant;
    int32_t* out_frames;                             // RESULT only
};

template <int MODE>
struct GStrm : GStrmArgs {};                         // kernel arguments

template <>
struct GStrm<ONESHOT> {};

template <bool ON>
struct GBiasStrm {};                                 // kernel arguments: ON = BIAS && MODE != ONESHOT

template <>
struct GBiasStrm<true> : GBiasState {};

// ADVANCE: x, lengths and T are the chunk's (Tc frames, lengths[b] of them valid), ws and cgr hold the chunk's candidate rows and
// their spellings and the outputs are unused.  RESULT: x, lengths, ws and cgr are unused, T is the ids' row pitch (Lcap).
template <bool LM, bool BIAS, int MODE>
__global__ __launch_bounds__(THREADS) void gram_beam_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths, int T,
                                                            int B, int V, int W, int K, int blank, Ws ws,
                                                            const int2* __restrict__ cgr, int32_t* __restrict__ out_ids,
                                                            int32_t* __restrict__ out_len, float* __restrict__ out_score,
                                                            Fuse<LM> fz, GStrm<MODE> sz, Bias<BIAS> bz,
                                                            GBiasStrm<BIAS && MODE != ONESHOT> bs) {
    __shared__ GBeam bm[2];
    __shared__ GFuseLds<LM> fl;
    __shared__ GBiasLds<BIAS> bl;
    __shared__ float tot[MAX_ENTRIES];                 // scores of the frame's entries in canonical order
    __shared__ unsigned short mt[MAX_EXT];             // an extension that took in a second one of the same string: that one's index
    __shared__ float btot[MAX_BEAM], bpu[MAX_BEAM], bpg[MAX_BEAM];     // pb + pu + pg, pb + pu, pb + pg of the beam
    __shared__ float spb[MAX_BEAM], spu[MAX_BEAM], spg[MAX_BEAM];      // the stays' new masses
    __shared__ int par1[MAX_BEAM], par2[MAX_BEAM];     // the beam slots of s[:-1] and s[:-2]
    __shared__ int cu[MAX_BEAM], cg[MAX_BEAM];         // the candidate ranks of the unigram token of s[-1] and the bigram of s[-2:]
    __shared__ int cid[MAX_TOPK], ca[MAX_TOPK], cb[MAX_TOPK], cmate[MAX_TOPK];   // id, spelling (a, b or -1); for a bigram
    __shared__ float clp[MAX_TOPK];                                              // candidate, the rank of the unigram (b)
    __shared__ unsigned hist[2][256];
    __shared__ float sv_tot[MAX_BEAM];
    __shared__ int sv_pos[MAX_BEAM];
    __shared__ float xnext[2 * MAX_BEAM + MAX_TOPK];   // next frame's logits of the beam's utok, of its gtok, of the candidates
    __shared__ int wsum[4];
    __shared__ int s_digit, s_need, s_all, s_done;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int len_b = lengths ? min(max(lengths[b], 0), T) : T;
    const int T2 = MODE == RESULT ? T : 2 * T;        // the ids' row pitch
    int2* nodes;
    int cur = 0, m = 1, f0 = 0;                        // f0: the frames this utterance consumed before this call
    if constexpr (MODE != ONESHOT) {
        const StrmHead hd = stream_begin<MODE>(sz.s.hdr + (size_t)b * HDR_WORDS, sz.s.table, 2, B, W, sz.max_frames,
                                               sz.variant, sz.out_frames, b, len_b);
        nodes = hd.nodes; m = hd.m; f0 = hd.f0; len_b = hd.len_b;
        if (MODE == ADVANCE && len_b <= 0) return;     // nothing to consume: the state is not touched
        if (tid < m) {
            const size_t i = (size_t)b * W + tid;
            const int utok = sz.s.utok[i], gtok = sz.s.gtok[i];
            GBeam& r = bm[0];
            r.pb[tid] = sz.s.pb[i];
            r.pu[tid] = sz.s.pu[i];
            r.pg[tid] = sz.s.pg[i];
            r.h0[tid] = sz.s.h0[i];
            r.h1[tid] = sz.s.h1[i];
            r.h2[tid] = sz.s.h2[i];
            r.len[tid] = sz.s.len[i];
            r.c1[tid] = sz.s.c1[i];
            r.c2[tid] = sz.s.c2[i];
            r.c3[tid] = sz.s.c3[i];
            r.utok[tid] = utok;
            r.gtok[tid] = gtok;
            r.node[tid] = sz.s.node[i];
            if constexpr (LM) fl.lm[0][tid] = sz.s.lm[i];
            if constexpr (BIAS) {
                const int s = bs.state[i];             // a state that other code wrote into cannot lead outside ret
                bl.open[0][tid] = bs.open[i];
                bl.state[0][tid] = (unsigned)s < (unsigned)bz.g.n_states ? s : 0;
            }
            // the logits of the tokens behind pu and pg in the chunk's first frame: the values the one-shot loop loads one frame
            // ahead.  Behind a token of -1 that loop holds 0.f (the root's is never written) and never reads it (section 26).
            if constexpr (MODE == ADVANCE) {
                r.xu[tid] = (unsigned)utok < (unsigned)V ? x[(size_t)b * V + utok] : 0.f;
                r.xg[tid] = (unsigned)gtok < (unsigned)V ? x[(size_t)b * V + gtok] : 0.f;
            }
        }
    } else {
        nodes = ws.node + (size_t)b * T2 * W;
    }
    if (MODE == ONESHOT && tid == 0) {
        GBeam& r = bm[0];
        r.pb[0] = 0.f;
        r.pu[0] = r.pg[0] = -INFINITY;
        r.h0[0] = ROOT_HASH;
        r.h1[0] = r.h2[0] = 0;
        r.len[0] = 0;
        r.c1[0] = r.c2[0] = r.c3[0] = -1;
        r.utok[0] = r.gtok[0] = -1;
        r.node[0] = -1;
        if constexpr (LM) fl.lm[0][0] = 0.f;
        if constexpr (BIAS) {
            bl.open[0][0] = 0.f;
            bl.state[0][0] = 0;
        }
    }
    int q_n = 0, q_id = 0;
    int2 q_g = make_int2(-1, -1);
    float q_lse = 0.f, q_lpb = 0.f, q_lp = 0.f;
    auto load_row = [&](int t) {
        const size_t row = (size_t)t * B + b;
        q_n = ws.n[row];
        q_lse = ws.lse[row];
        q_lpb = ws.lpb[row];
        if (tid < K) {                                 // entries past n are never used
            q_id = ws.cid[row * K + tid];
            q_lp = ws.clp[row * K + tid];
            q_g = cgr[row * K + tid];
        }
    };
    if (len_b > 0) load_row(0);
    __syncthreads();
    for (int t = 0; MODE != RESULT && t < len_b; ++t) {
        const GBeam& o = bm[cur];
        GBeam& nx = bm[cur ^ 1];
        const int n = min(q_n, K);
        const float lse = q_lse, lpb = q_lpb;
        // A: the frame's candidates and their spellings; a candidate that spells nothing (a < 0) keeps its rank and scores -inf
        if (tid < n) {
            cid[tid] = q_id;
            clp[tid] = q_lp;
            ca[tid] = q_g.x;
            cb[tid] = q_g.x < 0 ? -1 : q_g.y;
            cmate[tid] = -1;
        }
        if (tid < m) {
            btot[tid] = lae3(o.pb[tid], o.pu[tid], o.pg[tid]);
            bpu[tid] = lae(o.pb[tid], o.pu[tid]);
            bpg[tid] = lae(o.pb[tid], o.pg[tid]);
            par1[tid] = par2[tid] = -1;
            cu[tid] = cg[tid] = -1;
        }
        hist[0][tid] = 0;
        __syncthreads();
        // the next frame's loads: its candidate row, and the logit of every token that can be behind a pu or a pg after this
        // frame (the beam's utok and gtok, and this frame's candidates)
        float gxu = 0.f, gxg = 0.f, gxc = 0.f;
        if (t + 1 < len_b) {
            load_row(t + 1);
            const float* xr = x + ((size_t)(t + 1) * B + b) * V;
            if (tid < m) {
                if (o.utok[tid] >= 0) gxu = xr[o.utok[tid]];
                if (o.gtok[tid] >= 0) gxg = xr[o.gtok[tid]];
            }
            if (tid < n) gxc = xr[cid[tid]];
        }
        // the score of the extension of beam slot j by candidate r.  A token cannot follow itself without a blank: the unigram
        // (a) after a string that ends in a starts from pb + pg, the bigram (a, b) after one that ends in ab from pb + pu.
        auto ext_val = [&](int j, int r) -> float {
            const int a = ca[r], b2 = cb[r];
            if (a < 0) return -INFINITY;
            const float base = b2 < 0 ? (o.c1[j] == a ? bpg[j] : btot[j]) : (o.c2[j] == a && o.c1[j] == b2 ? bpu[j] : btot[j]);
            return base + clp[r];
        };
        // B: extension scores; for every stay the beam slots of s[:-1] and s[:-2] and the candidates that lead from them to s
        const int E = m + m * n;
        ngram::Step st1, st2;
        ctx::Step cs;
        // the look-ups of extension q: one step for a unigram candidate, two for a bigram candidate (both contexts are known from
        // the parent's last characters and a, so the second does not wait for the first), none for one that spells nothing.
        // The automaton's step on a starts here too; its step on b needs the state after a and is issued once that is known.
        auto issue = [&](int q) {
            if constexpr (LM || BIAS) {
                const int j = q / n, r = q - j * n, a = ca[r], b2 = cb[r];
                if (a < 0) return;
                if constexpr (BIAS) cs = ctx::step_issue(bz.g, bl.state[cur][j], a);
                if constexpr (LM) {
                    const int x0 = lm_ctx(o, j, 0, fz.bos), x1 = lm_ctx(o, j, 1, fz.bos), x2 = lm_ctx(o, j, 2, fz.bos);
                    st1 = ngram::step_issue(fz.lm, x0, x1, x2, a);
                    if (b2 >= 0) st2 = ngram::step_issue(fz.lm, a, x0, x1, b2);
                }
            }
        };
        if constexpr (LM || BIAS) {
            // thread k takes extension k (and k + 256, ...): the first one's loads are in flight during the matching loops below
            if (tid < m * n) issue(tid);
        } else {
            for (int q = tid; q < m * n; q += THREADS) {
                const int j = q / n, r = q - j * n;
                tot[m + q] = ext_val(j, r);
                mt[q] = NO_MATE;
            }
        }
        for (int p = tid; p < m * m; p += THREADS) {
            const int i = p / m, j = p - i * m;
            if (o.len[i] > 0 && o.h0[j] == o.h1[i] && o.len[j] == o.len[i] - 1 && o.c1[j] == o.c2[i]) par1[i] = j;
            if (o.len[i] > 1 && o.h0[j] == o.h2[i] && o.len[j] == o.len[i] - 2 && o.c1[j] == o.c3[i]) par2[i] = j;
        }
        for (int p = tid; p < m * n; p += THREADS) {
            const int i = p / n, r = p - i * n;
            if (ca[r] < 0) continue;
            if (cb[r] < 0) { if (ca[r] == o.c1[i]) cu[i] = r; }
            else if (ca[r] == o.c2[i] && cb[r] == o.c1[i]) cg[i] = r;
        }
        for (int p = tid; p < n * n; p += THREADS) {
            const int r2 = p / n, r = p - r2 * n;
            if (cb[r2] >= 0 && ca[r] == cb[r2] && ca[r] >= 0 && cb[r] < 0) cmate[r2] = r;
        }
        if constexpr (LM && !BIAS) {
            for (int q = tid; q < m * n; q += THREADS) {
                const int j = q / n, r = q - j * n, a = ca[r], b2 = cb[r];
                mt[q] = NO_MATE;
                if (a < 0) { tot[m + q] = -INFINITY; continue; }
                if (q >= THREADS) issue(q);
                float nl = fl.lm[cur][j] + ngram::step_finish(fz.lm, st1);       // the steps in string order: (lm + a) + b
                if (b2 >= 0) nl += ngram::step_finish(fz.lm, st2);
                fl.elm[q] = nl;
                tot[m + q] = ext_val(j, r) + (fz.alpha * nl + fz.beta * (float)(o.len[j] + (b2 < 0 ? 1 : 2)));
            }
        }
        if constexpr (BIAS) {
            for (int q = tid; q < m * n; q += THREADS) {
                const int j = q / n, r = q - j * n, a = ca[r], b2 = cb[r];
                mt[q] = NO_MATE;
                if (a < 0) { tot[m + q] = -INFINITY; continue; }
                if (q >= THREADS) issue(q);
                // the automaton first: the step on b leaves as soon as the state after a is known and flies during the model's
                int s1;
                float bo = bl.open[cur][j] + ctx::step_finish(bz.g, cs, &s1);    // the steps in string order: (open + a) + b
                if (b2 >= 0) cs = ctx::step_issue(bz.g, s1, b2);
                float v = ext_val(j, r);
                if constexpr (LM) {
                    float nl = fl.lm[cur][j] + ngram::step_finish(fz.lm, st1);
                    if (b2 >= 0) nl += ngram::step_finish(fz.lm, st2);
                    fl.elm[q] = nl;
                    v += bonus_rounded(fz.alpha, nl, fz.beta, (float)(o.len[j] + (b2 < 0 ? 1 : 2)));
                }
                if (b2 >= 0) bo += ctx::step_finish(bz.g, cs, &s1);
                bl.eopen[q] = bo;
                bl.estate[q] = s1;
                tot[m + q] = v + bo;
            }
        }
        __syncthreads();
        // C1: two extensions that spell one string: slot j holds s' + a, its parent slot j2 holds s', candidate r2 is the bigram
        // (a, b) and candidate r the unigram (b).  Spellings are unique, so an entry is in at most one such pair; the earlier
        // entry takes the sum (the unigram part first) and remembers the other one.
        for (int p = tid; p < m * n; p += THREADS) {
            const int j = p / n, r2 = p - j * n, j2 = par1[j];
            if (j2 < 0 || cb[r2] < 0 || ca[r2] != o.c1[j] || cmate[r2] < 0) continue;
            const int qu = j * n + cmate[r2], qg = j2 * n + r2;
            const int lo = min(qu, qg), hi = max(qu, qg);
            float s;
            if constexpr (LM && !BIAS) {
                // the acoustic parts again (phase B's sums, bit for bit), merged, then the string's bonus: both routes carry
                // the same lm and length
                s = lae(ext_val(j, cmate[r2]), ext_val(j2, r2)) + (fz.alpha * fl.elm[lo] + fz.beta * (float)(o.len[j] + 1));
            } else if constexpr (LM) {
                s = lae(ext_val(j, cmate[r2]), ext_val(j2, r2)) + bonus_fused(fz.alpha, fl.elm[lo], fz.beta, (float)(o.len[j] + 1));
            } else if constexpr (BIAS) {
                s = lae(ext_val(j, cmate[r2]), ext_val(j2, r2));
            } else {
                s = lae(tot[m + qu], tot[m + qg]);
            }
            if constexpr (BIAS) s += bl.eopen[lo];       // both routes carry the same bias_open and state as well
            tot[m + lo] = s;
            tot[m + hi] = -INFINITY;
            mt[lo] = (unsigned short)hi;
        }
        __syncthreads();
        // C2: stays, merged with the unigram extension of s[:-1] and the bigram extension of s[:-2] (one entry, at the stay's position)
        if (tid < m) {
            const int i = tid;
            const float npb = btot[i] + lpb;
            float npu = o.utok[i] >= 0 ? o.pu[i] + (o.xu[i] - lse) : -INFINITY;
            float npg = o.gtok[i] >= 0 ? o.pg[i] + (o.xg[i] - lse) : -INFINITY;
            if (par1[i] >= 0 && cu[i] >= 0) {
                npu = lae(npu, ext_val(par1[i], cu[i]));
                tot[m + par1[i] * n + cu[i]] = -INFINITY;
            }
            if (par2[i] >= 0 && cg[i] >= 0) {
                npg = lae(npg, ext_val(par2[i], cg[i]));
                tot[m + par2[i] * n + cg[i]] = -INFINITY;
            }
            spb[i] = npb;
            spu[i] = npu;
            spg[i] = npg;
            if constexpr (LM && !BIAS) tot[i] = lae3(npb, npu, npg) + (fz.alpha * fl.lm[cur][i] + fz.beta * (float)o.len[i]);
            else if constexpr (LM) tot[i] = lae3(npb, npu, npg) + bonus_rounded(fz.alpha, fl.lm[cur][i], fz.beta, (float)o.len[i]);
            else tot[i] = lae3(npb, npu, npg);
            if constexpr (BIAS) tot[i] += bl.open[cur][i];
        }
        __syncthreads();
        // D, E: beam_kernel's, line for line (see the note there)
        // D: radix select of the W best valid entries, 8 bits of the key per pass from the top: key >> sh > tau >> sh, and the
        // first `need` (canonical order) with key >> sh == tau >> sh.  It stops early once the boundary digit's entries are all kept.
        const int chunk = (E + THREADS - 1) / THREADS, e0 = min(E, tid * chunk), e1 = min(E, e0 + chunk);
        unsigned prefix = 0;
        int need = W, all = 0, sh = 0;
        for (int shift = 24, pass = 0; shift >= 0; shift -= 8, ++pass) {
            unsigned* h = hist[pass & 1];
            hist[(pass + 1) & 1][tid] = 0;           // the next pass's histogram; the last reader of it was the pass before
            for (int e = e0; e < e1; ++e) {
                const float f = tot[e];
                if (!valid(f)) continue;
                const unsigned key = order_key(f);
                if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&h[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) {
                int c[4], sum = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { c[k] = (int)h[255 - 4 * lane - k]; sum += c[k]; }
                int incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int u = __shfl_up(incl, off);
                    if (lane >= off) incl += u;
                }
                const int count = __shfl(incl, 63);
                if (shift == 24 && count <= W) {
                    if (lane == 0) s_all = 1;
                } else {
                    if (lane == 0) s_all = 0;
                    const unsigned long long hit = __ballot(incl >= need);
                    const int L = __ffsll((long long)hit) - 1;
                    if (lane == L) {
                        int acc = incl - sum;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (acc + c[k] >= need) {
                                s_digit = 255 - 4 * lane - k;
                                s_need = need - acc;
                                s_done = acc + c[k] == need;
                                break;
                            }
                            acc += c[k];
                        }
                    }
                }
            }
            __syncthreads();
            if (s_all) { all = 1; break; }
            prefix |= (unsigned)s_digit << shift;
            need = s_need;
            sh = shift;
            if (s_done) break;          // (s_digit / s_need / s_done are rewritten after the next pass's first barrier)
        }
        const unsigned tau = all ? 0u : prefix;
        const int need_eq = all ? 0 : need;
        // E: compact the kept entries in canonical order
        int gt = 0, eq = 0;
        for (int e = e0; e < e1; ++e) {
            const float f = tot[e];
            if (!valid(f)) continue;
            const unsigned key = order_key(f) >> sh;
            gt += key > tau >> sh;
            eq += key == tau >> sh;
        }
        int packed_total;
        const int packed = block_excl_scan((gt << 16) | eq, wsum, &packed_total);
        int g = packed >> 16, q = packed & 0xffff;
        for (int e = e0; e < e1; ++e) {
            const float f = tot[e];
            if (!valid(f)) continue;
            const unsigned key = order_key(f) >> sh;
            int slot = -1;
            if (key > tau >> sh) slot = g + min(q, need_eq), ++g;
            else if (key == tau >> sh) { if (q < need_eq) slot = g + q; ++q; }
            if (slot >= 0) { sv_pos[slot] = e; sv_tot[slot] = f; }
        }
        const int M = (packed_total >> 16) + min(packed_total & 0xffff, need_eq);
        if (tid < m) {
            xnext[tid] = gxu;
            xnext[m + tid] = gxg;
        }
        if (tid < n) xnext[2 * m + tid] = gxc;
        __syncthreads();
        // F: rank the survivors (score descending, canonical position on ties) into the next beam
        if (tid < M) {
            const float f = sv_tot[tid];
            const int rank = rank_of(sv_tot, M, f, tid);
            const int e = sv_pos[tid];
            if (e < m) {
                // a stay whose pu (pg) was empty so far learns the token from the candidate that spells s[-1] (s[-2:])
                const bool ku = o.utok[e] >= 0, kg = o.gtok[e] >= 0;
                nx.pb[rank] = spb[e];
                nx.pu[rank] = spu[e];
                nx.pg[rank] = spg[e];
                nx.h0[rank] = o.h0[e];
                nx.h1[rank] = o.h1[e];
                nx.h2[rank] = o.h2[e];
                nx.len[rank] = o.len[e];
                nx.c1[rank] = o.c1[e];
                nx.c2[rank] = o.c2[e];
                nx.c3[rank] = o.c3[e];
                nx.node[rank] = o.node[e];
                nx.utok[rank] = ku ? o.utok[e] : (cu[e] >= 0 ? cid[cu[e]] : -1);
                nx.gtok[rank] = kg ? o.gtok[e] : (cg[e] >= 0 ? cid[cg[e]] : -1);
                nx.xu[rank] = ku ? xnext[e] : (cu[e] >= 0 ? xnext[2 * m + cu[e]] : 0.f);
                nx.xg[rank] = kg ? xnext[m + e] : (cg[e] >= 0 ? xnext[2 * m + cg[e]] : 0.f);
                if constexpr (LM) fl.lm[cur ^ 1][rank] = fl.lm[cur][e];
                if constexpr (BIAS) {
                    bl.open[cur ^ 1][rank] = bl.open[cur][e];
                    bl.state[cur ^ 1][rank] = bl.state[cur][e];
                }
            } else {
                const int q2 = e - m, j = q2 / n, r = q2 - j * n, a = ca[r], b2 = cb[r];
                const int mate = mt[q2];
                // the other extension of the pair, if any: (jm, rm); f is then the sum and the parts are phase B's again
                const int jm = mate == NO_MATE ? -1 : mate / n, rm = mate == NO_MATE ? -1 : mate - jm * n;
                // (with the language model or the bias f is the ranking score, and the own part is phase B's sum again as well)
                const float own = !LM && !BIAS && jm < 0 ? f : ext_val(j, r);
                const float oth = jm < 0 ? -INFINITY : ext_val(jm, rm);
                const int id = 2 * ((f0 + t) * W + rank);
                nx.pb[rank] = -INFINITY;
                if constexpr (LM) fl.lm[cur ^ 1][rank] = fl.elm[q2];
                if constexpr (BIAS) {
                    bl.open[cur ^ 1][rank] = bl.eopen[q2];
                    bl.state[cur ^ 1][rank] = bl.estate[q2];
                }
                if (b2 < 0) {                           // s + a
                    nx.pu[rank] = own;
                    nx.pg[rank] = oth;
                    nx.utok[rank] = cid[r];
                    nx.gtok[rank] = jm < 0 ? -1 : cid[rm];
                    nx.xu[rank] = xnext[2 * m + r];
                    nx.xg[rank] = jm < 0 ? 0.f : xnext[2 * m + rm];
                    nx.h0[rank] = hash_append(o.h0[j], a);
                    nx.h1[rank] = o.h0[j];
                    nx.h2[rank] = o.h1[j];
                    nx.len[rank] = o.len[j] + 1;
                    nx.c1[rank] = a;
                    nx.c2[rank] = o.c1[j];
                    nx.c3[rank] = o.c2[j];
                    nx.node[rank] = id;
                    nodes[id] = make_int2(o.node[j], a);
                } else {                                // s + a + b: two nodes
                    const unsigned long long ha = hash_append(o.h0[j], a);
                    nx.pg[rank] = own;
                    nx.pu[rank] = oth;
                    nx.gtok[rank] = cid[r];
                    nx.utok[rank] = jm < 0 ? -1 : cid[rm];
                    nx.xg[rank] = xnext[2 * m + r];
                    nx.xu[rank] = jm < 0 ? 0.f : xnext[2 * m + rm];
                    nx.h0[rank] = hash_append(ha, b2);
                    nx.h1[rank] = ha;
                    nx.h2[rank] = o.h0[j];
                    nx.len[rank] = o.len[j] + 2;
                    nx.c1[rank] = b2;
                    nx.c2[rank] = a;
                    nx.c3[rank] = o.c1[j];
                    nx.node[rank] = id + 1;
                    nodes[id] = make_int2(o.node[j], a);
                    nodes[id + 1] = make_int2(id, b2);
                }
            }
        }
        __syncthreads();
        cur ^= 1;
        m = M;
    }
    __threadfence();
    __syncthreads();
    const GBeam& o = bm[cur];
    if constexpr (MODE == ADVANCE) {
        // the beam goes back where it came from; slots past m keep what they held
        if (tid < m) {
            const size_t i = (size_t)b * W + tid;
            sz.s.pb[i] = o.pb[tid];
            sz.s.pu[i] = o.pu[tid];
            sz.s.pg[i] = o.pg[tid];
            sz.s.h0[i] = o.h0[tid];
            sz.s.h1[i] = o.h1[tid];
            sz.s.h2[i] = o.h2[tid];
            sz.s.len[i] = o.len[tid];
            sz.s.c1[i] = o.c1[tid];
            sz.s.c2[i] = o.c2[tid];
            sz.s.c3[i] = o.c3[tid];
            sz.s.utok[i] = o.utok[tid];
            sz.s.gtok[i] = o.gtok[tid];
            sz.s.node[i] = o.node[tid];
            if constexpr (LM) sz.s.lm[i] = fl.lm[cur][tid];
            if constexpr (BIAS) {
                bs.open[i] = bl.open[cur][tid];
                bs.state[i] = bl.state[cur][tid];
            }
        }
        stream_end(sz.s.hdr + (size_t)b * HDR_WORDS, m, f0 + len_b);
        return;
    }
    // the N-best strings, sorted by score: the ids by fill_blank and walk_chain (RESULT: a string longer than the row pitch is cut there, and its
    // length is reported in full)
    int table_n = 0, cm = 0;                           // cm: the committed characters (RESULT only)
    if constexpr (MODE == RESULT) {
        table_n = 2 * sz.max_frames * W;
        if (m > 0) cm = max(sz.s.hdr[(size_t)b * HDR_WORDS + H_COMMITTED], 0);
    }
    int32_t* ids = out_ids + (size_t)b * W * T2;
    if constexpr (LM || BIAS) {
        // the end terms, then the final order: score descending, ties to the earlier slot (as beam_kernel<true, .>)
        float* o_ctc;
        float* o_lm;
        if constexpr (BIAS) { o_ctc = bz.out_ctc; o_lm = bz.out_lm; }
        else { o_ctc = fz.out_ctc; o_lm = fz.out_lm; }
        float ctc = 0.f, lmv = 0.f, bv = 0.f, sc = 0.f;
        if (tid < m) {
            ctc = lae3(o.pb[tid], o.pu[tid], o.pg[tid]);
            sc = ctc;
            if constexpr (LM) {
                lmv = fl.lm[cur][tid];
                if (fz.eos >= 0)
                    lmv += ngram::step(fz.lm, lm_ctx(o, tid, 0, fz.bos), lm_ctx(o, tid, 1, fz.bos), lm_ctx(o, tid, 2, fz.bos), fz.eos);
                if constexpr (BIAS) sc = ctc + bonus_rounded(fz.alpha, lmv, fz.beta, (float)o.len[tid]);
                else sc = ctc + (fz.alpha * lmv + fz.beta * (float)o.len[tid]);
            }
            if constexpr (BIAS) {
                bv = bl.open[cur][tid] + bz.g.ret[bl.state[cur][tid]];        // the advance of an unfinished match goes back
                sc += bv;
            }
            sv_tot[tid] = sc;
        }
        __syncthreads();
        if (tid < m) {
            const int rank = rank_of(sv_tot, m, sc, tid);
            sv_pos[rank] = tid;
            out_score[b * W + rank] = sc;
            o_ctc[b * W + rank] = ctc;
            o_lm[b * W + rank] = lmv;
            if constexpr (BIAS) bz.out_bias[b * W + rank] = bv;
        }
        __syncthreads();
        fill_blank(ids, T2, W, m, o.len, sv_pos, blank, cm);
        if (tid < W) {
            if (tid < m) {
                const int h = sv_pos[tid], L = tail_len<MODE>(o.len[h], cm);
                out_len[b * W + tid] = L;
                walk_chain<MODE>(ids + (size_t)tid * T2, T2, L, o.node[h], nodes, table_n);
            } else {
                out_len[b * W + tid] = 0;
                out_score[b * W + tid] = -INFINITY;
                o_ctc[b * W + tid] = -INFINITY;
                o_lm[b * W + tid] = 0.f;
                if constexpr (BIAS) bz.out_bias[b * W + tid] = 0.f;
            }
        }
        return;
    }
    fill_blank(ids, T2, W, m, o.len, nullptr, blank, cm);
    if (tid < W) {
        if (tid < m) {
            const int L = tail_len<MODE>(o.len[tid], cm);
            out_len[b * W + tid] = L;
            out_score[b * W + tid] = lae3(o.pb[tid], o.pu[tid], o.pg[tid]);
            walk_chain<MODE>(ids + (size_t)tid * T2, T2, L, o.node[tid], nodes, table_n);
        } else {
            out_len[b * W + tid] = 0;
            out_score[b * W + tid] = -INFINITY;
        }
    }
}

// asr_gram_ctc_beam_bias_stream_reset: the header and the root beam (what gram_beam_kernel<., ONESHOT> starts from) of every utterance, or of those with mask[b] != 0
__global__ __launch_bounds__(256) void gram_stream_reset_kernel(GState s, int B, int W, int F, int variant,
                                                                const int32_t* __restrict__ mask, GBiasState bs) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B || (mask && mask[b] == 0)) return;
    int* h = s.hdr + (size_t)b * HDR_WORDS;
    h[H_MAGIC] = STATE_MAGIC;
    h[H_B] = B;
    h[H_W] = W;
    h[H_F] = F;
    h[H_VARIANT] = variant;
    h[H_M] = 1;
    h[H_FRAMES] = 0;
    h[HDR_WORDS - 1] = 0;
    const size_t i = (size_t)b * W;
    s.pb[i] = 0.f;
    s.pu[i] = s.pg[i] = -INFINITY;
    s.h0[i] = ROOT_HASH;
    s.h1[i] = s.h2[i] = 0;
    s.len[i] = 0;
    s.c1[i] = s.c2[i] = s.c3[i] = -1;
    s.utok[i] = s.gtok[i] = -1;
    s.node[i] = -1;
    if (variant & 1) s.lm[i] = 0.f;
    if (variant & 2) {
        bs.open[i] = 0.f;
        bs.state[i] = 0;
    }
}

// ================================================================================================= the searches' host side
// All host code of the searches: the argument packs, the checks, one driver per entry family over the search
// family (Ctc / Gram), one dispatch from the variant to the kernel, and then the extern "C" entries, each of which packs its
// arguments and forwards.  Return codes are behaviour, down to which one wins when two apply; the order is stated where a driver
// runs its checks, and where the two families or two entries of one family differ, the difference is a parameter or a comment there.

// the language model and the phrase graph as the entries get them; filled once at the extern "C" boundary and passed by value
struct LmArgs {
    const float* uni;
    int vlm;
    const int32_t* keys;
    const float* vals;
    int slots, max_probe, order;
};

struct GraphArgs {
    const int32_t* keys;
    const int32_t* vals;
    int slots, max_probe;
    const float* ret;
    int n_states;
};

// what a search returns; ctc and lm with a model or a graph, bias with a graph, and all null in advance
struct Outs {
    int32_t* ids;
    int32_t* len;
    float* score;
    float* ctc;
    float* lm;
    float* bias;
};

static int make_lm(LmArgs a, ngram::Lm* lm) {
    if (!a.uni || a.vlm <= 0 || a.order < 1 || a.slots < 0) return ASR_ERR_BAD_ARG;
    if (a.order > ngram::MAX_ORDER) return ASR_ERR_UNSUPPORTED;
    if (a.slots > 0 && ((a.slots & (a.slots - 1)) != 0 || a.max_probe <= 0 || !a.keys || !a.vals)) return ASR_ERR_BAD_ARG;
    lm->uni = (const float2*)a.uni;
    lm->keys = a.slots > 0 ? (const int4*)a.keys : nullptr;
    lm->vals = (const float2*)a.vals;
    lm->mask = a.slots > 0 ? (unsigned)a.slots - 1u : 0u;
    lm->max_probe = a.max_probe;
    lm->order = a.order;
    lm->vlm = a.vlm;
    return ASR_OK;
}

static int make_graph(GraphArgs a, ctx::Graph* g) {
    if (!a.ret || a.n_states < 1 || a.slots < 0) return ASR_ERR_BAD_ARG;
    if (a.slots > 0 && ((a.slots & (a.slots - 1)) != 0 || a.max_probe <= 0 || !a.keys || !a.vals)) return ASR_ERR_BAD_ARG;
    g->keys = a.slots > 0 ? (const int2*)a.keys : nullptr;
    g->vals = (const int2*)a.vals;
    g->ret = a.ret;
    g->mask = a.slots > 0 ? (unsigned)a.slots - 1u : 0u;
    g->max_probe = a.max_probe;
    g->n_states = a.n_states;
    return ASR_OK;
}

// The one-shot entries' common checks: BAD_ARG for a null pointer, a dimension or a blank out of range, else UNSUPPORTED beyond
// the kernels' limits (`per_frame` prefix table nodes per frame and beam slot), else OK.  The driver returns a BAD_ARG at once,
// but an UNSUPPORTED only after its own argument checks and the model's and the graph's codes.
static int oneshot_check(const float* logits, const void* workspace, const Outs& out, int T, int B, int V, int blank, int beam_width,
                         int top_k, int per_frame) {
    if (!logits || !workspace || !out.ids || !out.len || !out.score || T <= 0 || B <= 0 || V <= 0 || blank < 0 || blank >= V ||
        beam_width <= 0 || top_k <= 0)
        return ASR_ERR_BAD_ARG;
    if (beam_width > MAX_BEAM || top_k > MAX_TOPK || beam_width * top_k > MAX_EXT) return ASR_ERR_UNSUPPORTED;
    if ((long long)per_frame * T * beam_width > 0x7fffffffLL) return ASR_ERR_UNSUPPORTED;    // prefix table node ids are int32
    return ASR_OK;
}

// The dimension and limit part of every streaming entry of both searches: BAD_ARG without a state (`has_state`) or for a
// dimension that is not positive, else UNSUPPORTED beyond the kernels' limits, else OK.  As with oneshot_check, an UNSUPPORTED
// waits for the model's and the graph's codes.
static int stream_dims(bool has_state, int B, int W, int F, int per_frame) {
    if (!has_state || B <= 0 || W <= 0 || F <= 0) return ASR_ERR_BAD_ARG;
    if (W > MAX_BEAM) return ASR_ERR_UNSUPPORTED;
    if ((long long)per_frame * F * W > 0x7fffffffLL) return ASR_ERR_UNSUPPORTED;      // prefix table node ids are int32
    return ASR_OK;
}

// the workspace of asr_ctc_beam_search with a prefix table of 2 * T * W nodes per utterance (a bigram extension adds two), then
// the candidates' spellings (T * B, K) int2
static size_t gram_ws_layout(int T, int B, int W, int K, char* base, Ws* ws, int2** cgr) {
    size_t off = ws_layout(T, B, 2 * W, K, base, ws);
    if (cgr) *cgr = (int2*)(base + off);
    off += align256((size_t)T * B * K * 8);
    return off;
}

// the streams' variant words (the states' headers and layouts)
static int ctc_variant(bool with_lm, bool with_bias) { return (with_lm ? 1 : 0) | (with_bias ? 2 : 0); }
static int gram_variant(bool with_lm, bool with_bias) { return GRAM_VARIANT | ctc_variant(with_lm, with_bias); }

// The two search families as the drivers see them: prefix table nodes per frame and beam slot, the variant word, and the
// workspace and state layouts (sz and bs may be null for the size alone).  Ctc has no spellings (*cgr = null) and keeps its
// graph fields inside State (bs untouched).
struct Ctc {
    static constexpr bool GRAM = false;
    static constexpr int PER_FRAME = 1;
    using Args = StrmArgs;
    static int variant(bool with_lm, bool with_bias) { return ctc_variant(with_lm, with_bias); }
    static size_t ws(int T, int B, int W, int K, char* base, Ws* ws, int2** cgr) {
        if (cgr) *cgr = nullptr;
        return ws_layout(T, B, W, K, base, ws);
    }
    static size_t state(int B, int W, int F, int variant, char* base, Args* sz, GBiasState*) {
        return state_layout(B, W, F, variant, base, sz ? &sz->s : nullptr);
    }
};

struct Gram {
    static constexpr bool GRAM = true;
    static constexpr int PER_FRAME = 2;
    using Args = GStrmArgs;
    static int variant(bool with_lm, bool with_bias) { return gram_variant(with_lm, with_bias); }
    static size_t ws(int T, int B, int W, int K, char* base, Ws* ws, int2** cgr) { return gram_ws_layout(T, B, W, K, base, ws, cgr); }
    static size_t state(int B, int W, int F, int variant, char* base, Args* sz, GBiasState* bs) {
        return gram_state_layout(B, W, F, variant, base, sz ? &sz->s : nullptr, bs);
    }
};

// everything a beam kernel of either family is launched with, in the widest form; launch_beam_as narrows it to the instantiation
template <class Fam>
struct Launch {
    hipStream_t st;
    const float* x;
    const int32_t* lengths;
    int T, B, V, W, K, blank;
    Ws ws;
    int2* cgr;                                       // Gram-CTC: the candidates' spellings
    Outs out;
    Fuse<true> fz;
    Bias<true> bz;
    typename Fam::Args sz;                           // unused in ONESHOT
    GBiasState bs;                                   // Gram-CTC streams with a graph
};

// the search's side of the model arguments (a.fz.lm is make_lm's; a negative bos / eos means none) and the outputs' places
template <class Fam>
static void fill_fuse(Launch<Fam>* a, int bos, int eos, float alpha, float beta, const Outs& out) {
    a->out = out;
    a->fz.bos = bos < 0 ? -1 : bos;
    a->fz.eos = eos < 0 ? -1 : eos;
    a->fz.alpha = alpha;
    a->fz.beta = beta;
    a->fz.out_ctc = a->bz.out_ctc = out.ctc;
    a->fz.out_lm = a->bz.out_lm = out.lm;
    a->bz.out_bias = out.bias;
}

template <class Fam, bool LM, bool BIAS, int MODE>
static void launch_beam_as(const Launch<Fam>& a) {
    Fuse<LM> f;
    Bias<BIAS> g;
    if constexpr (LM) f = a.fz;
    if constexpr (BIAS) g = a.bz;
    if constexpr (Fam::GRAM) {
        GStrm<MODE> sz;
        GBiasStrm<BIAS && MODE != ONESHOT> gs;
        if constexpr (MODE != ONESHOT) static_cast<GStrmArgs&>(sz) = a.sz;
        if constexpr (BIAS && MODE != ONESHOT) static_cast<GBiasState&>(gs) = a.bs;
        hipLaunchKernelGGL((gram_beam_kernel<LM, BIAS, MODE>), dim3(a.B), dim3(THREADS), 0, a.st, a.x, a.lengths, a.T, a.B, a.V, a.W, a.K,
                           a.blank, a.ws, (const int2*)a.cgr, a.out.ids, a.out.len, a.out.score, f, sz, g, gs);
    } else {
        Strm<MODE> sz;
        if constexpr (MODE != ONESHOT) static_cast<StrmArgs&>(sz) = a.sz;
        hipLaunchKernelGGL((beam_kernel<LM, BIAS, MODE>), dim3(a.B), dim3(THREADS), 0, a.st, a.x, a.lengths, a.T, a.B, a.V, a.W, a.K,
                           a.blank, a.ws, a.out.ids, a.out.len, a.out.score, f, g, sz);
    }
}

// The one place a variant word becomes a kernel: bit 0 the model, bit 1 the graph.  Both families in all three modes come through
// here, so the instantiations are beam_kernel and gram_beam_kernel <LM, BIAS, MODE> over everything, 12 each.
template <class Fam, int MODE>
static void launch_beam(int variant, const Launch<Fam>& a) {
    switch (variant & 3) {
        case 0: launch_beam_as<Fam, false, false, MODE>(a); break;
        case 1: launch_beam_as<Fam, true, false, MODE>(a); break;
        case 2: launch_beam_as<Fam, false, true, MODE>(a); break;
        default: launch_beam_as<Fam, true, true, MODE>(a);
    }
}

// cand_kernel over the (T, B, V) logits into a.ws, then for Gram-CTC gram_rows_kernel over the candidate rows into a.cgr
// (nothing to spell where a row can have no candidate)
template <class Fam>
static int launch_cand(const Launch<Fam>& a, float min_logp, const int32_t* gram) {
    const long long rows = (long long)a.T * a.B;
    hipLaunchKernelGGL(cand_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, a.st, a.x, a.lengths, a.T, a.B, a.V, a.blank, a.K,
                       min_logp, a.ws);
    ASR_LAUNCH_CHECK();
    if (Fam::GRAM && a.K > 0) {
        hipLaunchKernelGGL(gram_rows_kernel, dim3((unsigned)((rows * a.K + 255) / 256)), dim3(256), 0, a.st, a.lengths, a.T, a.B, a.K,
                           a.ws, (const int2*)gram, a.cgr);
        ASR_LAUNCH_CHECK();
    }
    return ASR_OK;
}

// the workspace of a one-shot search (`table`) or of a stream's advance, whose prefix table is the state's
template <class Fam>
static size_t ws_bytes(int T, int B, int V, int beam_width, int top_k, bool table) {
    if (T <= 0 || B <= 0 || V <= 0 || beam_width <= 0 || top_k <= 0) return 0;
    return Fam::ws(T, B, table ? beam_width : 0, min(top_k, V - 1), nullptr, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------- the one-shot driver
// Which one-shot entry calls: PLAIN has neither model nor graph nor the ctc / lm outputs; WITH_LM requires the model, so its
// vlm / bos / eos test runs whatever uni is (a null uni is then make_lm's BAD_ARG); WITH_BIAS requires the graph and takes the
// model only if uni != NULL, so without one its vlm, bos and eos are not looked at.
enum Kind { PLAIN, WITH_LM, WITH_BIAS };

// Order of the codes: the common BAD_ARGs, the entry's outputs, the model (its vlm / bos / eos BAD_ARG first), the graph,
// Gram-CTC's missing inventory (UNSUPPORTED), the limits' UNSUPPORTED, the workspace.
template <class Fam>
static int oneshot(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank, int beam_width, int top_k,
                   float min_logp, const int32_t* gram, Kind kind, LmArgs lm, int bos, int eos, float alpha, float beta,
                   GraphArgs graph, void* workspace, size_t workspace_bytes, Outs out) {
    const int lim = oneshot_check(logits, workspace, out, T, B, V, blank, beam_width, top_k, Fam::PER_FRAME);
    if (lim == ASR_ERR_BAD_ARG) return lim;
    if (kind != PLAIN && (!out.ctc || !out.lm)) return ASR_ERR_BAD_ARG;
    if (kind == WITH_BIAS && !out.bias) return ASR_ERR_BAD_ARG;
    const bool with_lm = kind == WITH_LM || lm.uni != nullptr;
    Launch<Fam> a{};
    int rc;
    if (with_lm) {
        if (lm.vlm < V || bos >= lm.vlm || eos >= lm.vlm) return ASR_ERR_BAD_ARG;
        rc = make_lm(lm, &a.fz.lm);
        if (rc != ASR_OK) return rc;
    }
    if (kind == WITH_BIAS) {
        rc = make_graph(graph, &a.bz.g);
        if (rc != ASR_OK) return rc;
    }
    if (Fam::GRAM && !gram) return ASR_ERR_UNSUPPORTED;
    if (lim != ASR_OK) return lim;
    a.st = (hipStream_t)stream, a.x = logits, a.lengths = lengths;
    a.T = T, a.B = B, a.V = V, a.W = beam_width, a.K = min(top_k, V - 1), a.blank = blank;
    if (workspace_bytes < Fam::ws(T, B, beam_width, a.K, (char*)workspace, &a.ws, &a.cgr)) return ASR_ERR_WORKSPACE;
    fill_fuse(&a, bos, eos, alpha, beta, out);
    rc = launch_cand(a, min_logp, gram);
    if (rc != ASR_OK) return rc;
    launch_beam<Fam, ONESHOT>(Fam::variant(with_lm, kind == WITH_BIAS), a);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

// ---------------------------------------------------------------------------------------------- the stream drivers
template <class Fam>
static size_t stream_state_bytes(int B, int beam_width, int max_frames, int with_lm, int with_bias) {
    if (stream_dims(true, B, beam_width, max_frames, Fam::PER_FRAME) == ASR_ERR_BAD_ARG) return 0;
    return Fam::state(B, beam_width, max_frames, Fam::variant(with_lm, with_bias), nullptr, nullptr, nullptr);
}

// The header and the root beam of every utterance, or of those with mask[b] != 0.  The two states differ, so each family has
// its kernel; `bos` is the CTC stream's alone (Gram-CTC gives it to advance and result), and nothing here can test it: there
// is no vlm.
template <class Fam>
static int stream_reset(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames, int with_lm,
                        int with_bias, int bos, const int32_t* mask) {
    const int rc = stream_dims(state != nullptr, B, beam_width, max_frames, Fam::PER_FRAME);
    if (rc != ASR_OK) return rc;
    const int variant = Fam::variant(with_lm, with_bias);
    typename Fam::Args sz;
    GBiasState bs{};
    if (state_bytes < Fam::state(B, beam_width, max_frames, variant, (char*)state, &sz, &bs)) return ASR_ERR_WORKSPACE;
    const dim3 grid((unsigned)((B + 255) / 256));
    if constexpr (Fam::GRAM) {
        hipLaunchKernelGGL(gram_stream_reset_kernel, grid, dim3(256), 0, (hipStream_t)stream, sz.s, B, beam_width, max_frames, variant,
                           mask, bs);
    } else {
        hipLaunchKernelGGL(stream_reset_kernel, grid, dim3(256), 0, (hipStream_t)stream, sz.s, B, beam_width, max_frames, variant,
                           bos < 0 ? -1 : bos, mask);
    }
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

// The checks on dimensions, state size and the model / graph arguments that advance and result share, in this order: the
// dimensions' BAD_ARG, the model, the graph, the limits' UNSUPPORTED, the state size (WORKSPACE).  A model or a graph is there
// if its uni / ret is.  Fills a->fz.lm, a->bz.g, a->sz and a->bs.
template <class Fam>
static int stream_open(int B, int W, int F, LmArgs lm, int bos, GraphArgs graph, void* state, size_t state_bytes, Launch<Fam>* a) {
    const int lim = stream_dims(state != nullptr, B, W, F, Fam::PER_FRAME);
    if (lim == ASR_ERR_BAD_ARG) return lim;
    const bool with_lm = lm.uni != nullptr, with_bias = graph.ret != nullptr;
    if (with_lm) {
        // Gram-CTC's advance and result take bos, and it is tested here.  The CTC stream's bos went to reset (above), so its
        // advance and result have none to test.
        if (Fam::GRAM && bos >= lm.vlm) return ASR_ERR_BAD_ARG;
        const int rc = make_lm(lm, &a->fz.lm);
        if (rc != ASR_OK) return rc;
    }
    if (with_bias) {
        const int rc = make_graph(graph, &a->bz.g);
        if (rc != ASR_OK) return rc;
    } else if (graph.keys || graph.vals || graph.slots != 0 || graph.n_states != 0) {
        return ASR_ERR_BAD_ARG;                      // a graph without its ret: section 22's check, not "no graph"
    }
    if (lim != ASR_OK) return lim;
    a->sz.max_frames = F;
    a->sz.variant = Fam::variant(with_lm, with_bias);
    a->sz.out_frames = nullptr;
    if (state_bytes < Fam::state(B, W, F, a->sz.variant, (char*)state, &a->sz, &a->bs)) return ASR_ERR_WORKSPACE;
    return ASR_OK;
}

// Order of the codes: the entry's BAD_ARGs, stream_open's, Gram-CTC's missing inventory, the top_k limits, the frames the state
// has room for (all three UNSUPPORTED), the workspace.  So a state that is too small beats a top_k that is too large.
// `bos`: Gram-CTC's; the CTC entry passes -1.
template <class Fam>
static int stream_advance(void* stream, const float* logits, const int32_t* lengths, int Tc, int B, int V, int blank, int beam_width,
                          int top_k, float min_logp, const int32_t* gram, LmArgs lm, int bos, GraphArgs graph, float alpha,
                          float beta, int frames_before, int max_frames, void* state, size_t state_bytes, void* workspace,
                          size_t workspace_bytes) {
    if (!logits || !workspace || Tc <= 0 || V <= 0 || blank < 0 || blank >= V || top_k <= 0 || frames_before < 0)
        return ASR_ERR_BAD_ARG;
    if (lm.uni && lm.vlm < V) return ASR_ERR_BAD_ARG;
    Launch<Fam> a{};
    int rc = stream_open(B, beam_width, max_frames, lm, bos, graph, state, state_bytes, &a);
    if (rc != ASR_OK) return rc;
    if (Fam::GRAM && !gram) return ASR_ERR_UNSUPPORTED;
    if (top_k > MAX_TOPK || beam_width * top_k > MAX_EXT) return ASR_ERR_UNSUPPORTED;
    if ((long long)frames_before + Tc > max_frames) return ASR_ERR_UNSUPPORTED;
    a.st = (hipStream_t)stream, a.x = logits, a.lengths = lengths;
    a.T = Tc, a.B = B, a.V = V, a.W = beam_width, a.K = min(top_k, V - 1), a.blank = blank;
    if (workspace_bytes < Fam::ws(Tc, B, 0, a.K, (char*)workspace, &a.ws, &a.cgr)) return ASR_ERR_WORKSPACE;
    fill_fuse(&a, bos, -1, alpha, beta, Outs{});     // the contexts start in reset (CTC) or with bos; they end in result
    rc = launch_cand(a, min_logp, gram);
    if (rc != ASR_OK) return rc;
    launch_beam<Fam, ADVANCE>(a.sz.variant, a);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

// Order of the codes: the outputs, of which ctc / lm / bias are required only by the variants that write them, eos against vlm,
// then stream_open's.  `bos`: Gram-CTC's; the CTC entry passes -1.
template <class Fam>
static int stream_result(void* stream, LmArgs lm, int bos, int eos, GraphArgs graph, float alpha, float beta, int B, int beam_width,
                         int max_frames, int blank, int Lcap, const void* state, size_t state_bytes, Outs out, int32_t* out_frames) {
    if (!out.ids || !out.len || !out.score || !out_frames || Lcap <= 0 || blank < 0) return ASR_ERR_BAD_ARG;
    if ((lm.uni || graph.ret) && (!out.ctc || !out.lm)) return ASR_ERR_BAD_ARG;
    if (graph.ret && !out.bias) return ASR_ERR_BAD_ARG;
    if (lm.uni && eos >= lm.vlm) return ASR_ERR_BAD_ARG;
    Launch<Fam> a{};
    const int rc = stream_open(B, beam_width, max_frames, lm, bos, graph, const_cast<void*>(state), state_bytes, &a);
    if (rc != ASR_OK) return rc;
    a.sz.out_frames = out_frames;
    a.st = (hipStream_t)stream;
    a.T = Lcap, a.B = B, a.W = beam_width, a.blank = blank;     // no logits, no candidates: the tail only
    fill_fuse(&a, bos, eos, alpha, beta, out);
    launch_beam<Fam, RESULT>(a.sz.variant, a);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

}  // namespace beam
}  // namespace asr

using namespace asr;
using namespace asr::beam;

// ---------------------------------------------------------------------------------------------- the entries
// Each packs its arguments and forwards; what an entry does not take is a null pack (no model, no graph), -1 (no bos) or a null
// output.  The *_workspace_bytes of one search family are one size.
static const LmArgs NO_LM{};
static const GraphArgs NO_GRAPH{};

extern "C" int asr_ngram_score(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals, int slots,
                               int max_probe, int order, const int32_t* ids, const int32_t* lengths, int N, int Lmax, int bos,
                               int eos, float* out_tok, float* out_sum) {
    if (!ids || !out_tok || !out_sum || N <= 0 || Lmax <= 0 || bos >= vlm || eos >= vlm) return ASR_ERR_BAD_ARG;
    ngram::Lm lm;
    const int rc = make_lm({uni, vlm, keys, vals, slots, max_probe, order}, &lm);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(ngram_score_kernel, dim3(N), dim3(THREADS), 0, (hipStream_t)stream, lm, ids, lengths, Lmax, bos < 0 ? -1 : bos,
                       eos < 0 ? -1 : eos, out_tok, out_sum);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_ctx_score(void* stream, const int32_t* g_keys, const int32_t* g_vals, int g_slots, int g_max_probe,
                             const float* g_ret, int g_n_states, int V, const int32_t* ids, const int32_t* lengths, int N,
                             int Lmax, int finalize, float* out_tok, float* out_sum) {
    if (!ids || !out_tok || !out_sum || N <= 0 || Lmax <= 0 || V <= 0) return ASR_ERR_BAD_ARG;
    ctx::Graph g;
    const int rc = make_graph({g_keys, g_vals, g_slots, g_max_probe, g_ret, g_n_states}, &g);
    if (rc != ASR_OK) return rc;
    hipLaunchKernelGGL(ctx_score_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, g, V, ids, lengths, N,
                       Lmax, finalize, out_tok, out_sum);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

// ---- CTC, one-shot
extern "C" size_t asr_ctc_beam_workspace_bytes(int T, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Ctc>(T, B, V, beam_width, top_k, true);
}

extern "C" size_t asr_ctc_beam_lm_workspace_bytes(int T, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Ctc>(T, B, V, beam_width, top_k, true);
}

extern "C" size_t asr_ctc_beam_bias_workspace_bytes(int T, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Ctc>(T, B, V, beam_width, top_k, true);
}

extern "C" int asr_ctc_beam_search(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                   int beam_width, int top_k, float min_logp, void* workspace, size_t workspace_bytes,
                                   int32_t* out_ids, int32_t* out_len, float* out_score) {
    return oneshot<Ctc>(stream, logits, lengths, T, B, V, blank, beam_width, top_k, min_logp, nullptr, PLAIN, NO_LM, -1, -1, 0.f, 0.f,
                        NO_GRAPH, workspace, workspace_bytes, {out_ids, out_len, out_score, nullptr, nullptr, nullptr});
}

extern "C" int asr_ctc_beam_search_lm(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                      int beam_width, int top_k, float min_logp, const float* uni, int vlm, const int32_t* keys,
                                      const float* vals, int slots, int max_probe, int order, int bos, int eos, float alpha,
                                      float beta, void* workspace, size_t workspace_bytes, int32_t* out_ids, int32_t* out_len,
                                      float* out_score, float* out_ctc, float* out_lm) {
    return oneshot<Ctc>(stream, logits, lengths, T, B, V, blank, beam_width, top_k, min_logp, nullptr, WITH_LM,
                        {uni, vlm, keys, vals, slots, max_probe, order}, bos, eos, alpha, beta, NO_GRAPH, workspace, workspace_bytes,
                        {out_ids, out_len, out_score, out_ctc, out_lm, nullptr});
}

extern "C" int asr_ctc_beam_search_bias(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                        int beam_width, int top_k, float min_logp, const float* uni, int vlm, const int32_t* keys,
                                        const float* vals, int slots, int max_probe, int order, int bos, int eos, float alpha,
                                        float beta, void* workspace, size_t workspace_bytes, int32_t* out_ids, int32_t* out_len,
                                        float* out_score, float* out_ctc, float* out_lm, const int32_t* g_keys,
                                        const int32_t* g_vals, int g_slots, int g_max_probe, const float* g_ret, int g_n_states,
                                        float* out_bias) {
    return oneshot<Ctc>(stream, logits, lengths, T, B, V, blank, beam_width, top_k, min_logp, nullptr, WITH_BIAS,
                        {uni, vlm, keys, vals, slots, max_probe, order}, bos, eos, alpha, beta,
                        {g_keys, g_vals, g_slots, g_max_probe, g_ret, g_n_states}, workspace, workspace_bytes,
                        {out_ids, out_len, out_score, out_ctc, out_lm, out_bias});
}

// ---- CTC, streaming
extern "C" size_t asr_ctc_beam_stream_state_bytes(int B, int beam_width, int max_frames, int with_lm, int with_bias) {
    return stream_state_bytes<Ctc>(B, beam_width, max_frames, with_lm, with_bias);
}

extern "C" size_t asr_ctc_beam_stream_workspace_bytes(int Tc, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Ctc>(Tc, B, V, beam_width, top_k, false);
}

extern "C" int asr_ctc_beam_stream_reset(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames,
                                         int with_lm, int with_bias, int bos, const int32_t* mask) {
    return stream_reset<Ctc>(stream, state, state_bytes, B, beam_width, max_frames, with_lm, with_bias, bos, mask);
}

extern "C" int asr_ctc_beam_stream_advance(void* stream, const float* logits, const int32_t* lengths, int Tc, int B, int V,
                                           int blank, int beam_width, int top_k, float min_logp, const float* uni, int vlm,
                                           const int32_t* keys, const float* vals, int slots, int max_probe, int order,
                                           const int32_t* g_keys, const int32_t* g_vals, int g_slots, int g_max_probe,
                                           const float* g_ret, int g_n_states, float alpha, float beta, int frames_before,
                                           int max_frames, void* state, size_t state_bytes, void* workspace,
                                           size_t workspace_bytes) {
    return stream_advance<Ctc>(stream, logits, lengths, Tc, B, V, blank, beam_width, top_k, min_logp, nullptr,
                               {uni, vlm, keys, vals, slots, max_probe, order}, -1,
                               {g_keys, g_vals, g_slots, g_max_probe, g_ret, g_n_states}, alpha, beta, frames_before, max_frames, state,
                               state_bytes, workspace, workspace_bytes);
}

extern "C" int asr_ctc_beam_stream_result(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals, int slots,
                                          int max_probe, int order, const int32_t* g_keys, const int32_t* g_vals, int g_slots,
                                          int g_max_probe, const float* g_ret, int g_n_states, float alpha, float beta, int eos,
                                          int B, int beam_width, int max_frames, int blank, int Lcap, const void* state,
                                          size_t state_bytes, int32_t* out_ids, int32_t* out_len, float* out_score, float* out_ctc,
                                          float* out_lm, float* out_bias, int32_t* out_frames) {
    return stream_result<Ctc>(stream, {uni, vlm, keys, vals, slots, max_probe, order}, -1, eos,
                              {g_keys, g_vals, g_slots, g_max_probe, g_ret, g_n_states}, alpha, beta, B, beam_width, max_frames, blank,
                              Lcap, state, state_bytes, {out_ids, out_len, out_score, out_ctc, out_lm, out_bias}, out_frames);
}

// ---- Gram-CTC, one-shot
extern "C" size_t asr_gram_ctc_beam_workspace_bytes(int T, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Gram>(T, B, V, beam_width, top_k, true);
}

extern "C" size_t asr_gram_ctc_beam_lm_workspace_bytes(int T, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Gram>(T, B, V, beam_width, top_k, true);
}

extern "C" size_t asr_gram_ctc_beam_bias_workspace_bytes(int T, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Gram>(T, B, V, beam_width, top_k, true);
}

extern "C" int asr_gram_ctc_beam_search(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                        int beam_width, int top_k, float min_logp, const int32_t* gram, void* workspace,
                                        size_t workspace_bytes, int32_t* out_ids, int32_t* out_len, float* out_score) {
    return oneshot<Gram>(stream, logits, lengths, T, B, V, blank, beam_width, top_k, min_logp, gram, PLAIN, NO_LM, -1, -1, 0.f, 0.f,
                         NO_GRAPH, workspace, workspace_bytes, {out_ids, out_len, out_score, nullptr, nullptr, nullptr});
}

extern "C" int asr_gram_ctc_beam_search_lm(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                           int beam_width, int top_k, float min_logp, const int32_t* gram, const float* uni, int vlm,
                                           const int32_t* keys, const float* vals, int slots, int max_probe, int order, int bos,
                                           int eos, float alpha, float beta, void* workspace, size_t workspace_bytes,
                                           int32_t* out_ids, int32_t* out_len, float* out_score, float* out_ctc, float* out_lm) {
    return oneshot<Gram>(stream, logits, lengths, T, B, V, blank, beam_width, top_k, min_logp, gram, WITH_LM,
                         {uni, vlm, keys, vals, slots, max_probe, order}, bos, eos, alpha, beta, NO_GRAPH, workspace, workspace_bytes,
                         {out_ids, out_len, out_score, out_ctc, out_lm, nullptr});
}

extern "C" int asr_gram_ctc_beam_search_bias(void* stream, const float* logits, const int32_t* lengths, int T, int B, int V, int blank,
                                             int beam_width, int top_k, float min_logp, const int32_t* gram, const float* uni, int vlm,
                                             const int32_t* keys, const float* vals, int slots, int max_probe, int order, int bos,
                                             int eos, float alpha, float beta, void* workspace, size_t workspace_bytes,
                                             int32_t* out_ids, int32_t* out_len, float* out_score, float* out_ctc, float* out_lm,
                                             const int32_t* g_keys, const int32_t* g_vals, int g_slots, int g_max_probe,
                                             const float* g_ret, int g_n_states, float* out_bias) {
    return oneshot<Gram>(stream, logits, lengths, T, B, V, blank, beam_width, top_k, min_logp, gram, WITH_BIAS,
                         {uni, vlm, keys, vals, slots, max_probe, order}, bos, eos, alpha, beta,
                         {g_keys, g_vals, g_slots, g_max_probe, g_ret, g_n_states}, workspace, workspace_bytes,
                         {out_ids, out_len, out_score, out_ctc, out_lm, out_bias});
}

// ---- Gram-CTC, streaming.  The family with a graph is the family: without one (with_bias == 0,
// g_ret == NULL) it is section 26's, size for size and byte for byte, so the narrow entries are these with no graph.
extern "C" size_t asr_gram_ctc_beam_bias_stream_state_bytes(int B, int beam_width, int max_frames, int with_lm, int with_bias) {
    return stream_state_bytes<Gram>(B, beam_width, max_frames, with_lm, with_bias);
}

extern "C" size_t asr_gram_ctc_beam_stream_state_bytes(int B, int beam_width, int max_frames, int with_lm) {
    return stream_state_bytes<Gram>(B, beam_width, max_frames, with_lm, 0);
}

extern "C" size_t asr_gram_ctc_beam_stream_workspace_bytes(int Tc, int B, int V, int beam_width, int top_k) {
    return ws_bytes<Gram>(Tc, B, V, beam_width, top_k, false);
}

extern "C" int asr_gram_ctc_beam_bias_stream_reset(void* stream, void* state, size_t state_bytes, int B, int beam_width,
                                                   int max_frames, int with_lm, int with_bias, const int32_t* mask) {
    return stream_reset<Gram>(stream, state, state_bytes, B, beam_width, max_frames, with_lm, with_bias, -1, mask);
}

extern "C" int asr_gram_ctc_beam_stream_reset(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames,
                                              int with_lm, const int32_t* mask) {
    return stream_reset<Gram>(stream, state, state_bytes, B, beam_width, max_frames, with_lm, 0, -1, mask);
}

extern "C" int asr_gram_ctc_beam_bias_stream_advance(void* stream, const float* logits, const int32_t* lengths, int Tc, int B, int V,
                                                     int blank, int beam_width, int top_k, float min_logp, const int32_t* gram,
                                                     const float* uni, int vlm, const int32_t* keys, const float* vals, int slots,
                                                     int max_probe, int order, int bos, const int32_t* g_keys,
                                                     const int32_t* g_vals, int g_slots, int g_max_probe, const float* g_ret,
                                                     int g_n_states, float alpha, float beta, int frames_before, int max_frames,
                                                     void* state, size_t state_bytes, void* workspace, size_t workspace_bytes) {
    return stream_advance<Gram>(stream, logits, lengths, Tc, B, V, blank, beam_width, top_k, min_logp, gram,
                                {uni, vlm, keys, vals, slots, max_probe, order}, bos,
                                {g_keys, g_vals, g_slots, g_max_probe, g_ret, g_n_states}, alpha, beta, frames_before, max_frames, state,
                                state_bytes, workspace, workspace_bytes);
}

extern "C" int asr_gram_ctc_beam_stream_advance(void* stream, const float* logits, const int32_t* lengths, int Tc, int B, int V,
                                                int blank, int beam_width, int top_k, float min_logp, const int32_t* gram,
                                                const float* uni, int vlm, const int32_t* keys, const float* vals, int slots,
                                                int max_probe, int order, int bos, float alpha, float beta, int frames_before,
                                                int max_frames, void* state, size_t state_bytes, void* workspace,
                                                size_t workspace_bytes) {
    return stream_advance<Gram>(stream, logits, lengths, Tc, B, V, blank, beam_width, top_k, min_logp, gram,
                                {uni, vlm, keys, vals, slots, max_probe, order}, bos, NO_GRAPH, alpha, beta, frames_before, max_frames,
                                state, state_bytes, workspace, workspace_bytes);
}

extern "C" int asr_gram_ctc_beam_bias_stream_result(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals,
                                                    int slots, int max_probe, int order, int bos, int eos, const int32_t* g_keys,
                                                    const int32_t* g_vals, int g_slots, int g_max_probe, const float* g_ret,
                                                    int g_n_states, float alpha, float beta, int B, int beam_width, int max_frames,
                                                    int blank, int Lcap, const void* state, size_t state_bytes, int32_t* out_ids,
                                                    int32_t* out_len, float* out_score, float* out_ctc, float* out_lm,
                                                    float* out_bias, int32_t* out_frames) {
    return stream_result<Gram>(stream, {uni, vlm, keys, vals, slots, max_probe, order}, bos, eos,
                               {g_keys, g_vals, g_slots, g_max_probe, g_ret, g_n_states}, alpha, beta, B, beam_width, max_frames, blank,
                               Lcap, state, state_bytes, {out_ids, out_len, out_score, out_ctc, out_lm, out_bias}, out_frames);
}

extern "C" int asr_gram_ctc_beam_stream_result(void* stream, const float* uni, int vlm, const int32_t* keys, const float* vals,
                                               int slots, int max_probe, int order, int bos, int eos, float alpha, float beta, int B,
                                               int beam_width, int max_frames, int blank, int Lcap, const void* state,
                                               size_t state_bytes, int32_t* out_ids, int32_t* out_len, float* out_score,
                                               float* out_ctc, float* out_lm, int32_t* out_frames) {
    return stream_result<Gram>(stream, {uni, vlm, keys, vals, slots, max_probe, order}, bos, eos, NO_GRAPH, alpha, beta, B, beam_width,
                               max_frames, blank, Lcap, state, state_bytes, {out_ids, out_len, out_score, out_ctc, out_lm, nullptr},
                               out_frames);
}

// ------------------------------------------------------------------------------ commit: a stream of any length
// asr_ctc_beam_stream_commit / asr_gram_ctc_beam_stream_commit.  The caller names a prefix P of the tokens beyond the committed
// ones; the hypotheses that do not start with it leave the beam, P is reported as final, and the prefix table is rewritten to
// hold only what the kept hypotheses have after P, one private chain per beam slot, so that it needs as many rows as the longest
// such tail has tokens (Gram-CTC: half as many) and not as many as frames were fed.  The semantics are stated in
// include/asr_hip.h.  One kernel serves both families and every variant: it knows the header, len, node and the table, and gets
// the other per-slot arrays as a list of pointers, because all it does with them is move entries to the front.
namespace asr {
namespace beam {

constexpr int MAX_ARR4 = 12, MAX_ARR8 = 3;

struct CommitArrays {
    int* a4[MAX_ARR4];                                // the (B, W) arrays of 4-byte entries except node (len is one of them)
    unsigned long long* a8[MAX_ARR8];                 // those of 8-byte entries
    int n4, n8;
};

struct CommitOut {
    int32_t* ids;                                     // (B, pitch): the tokens this call committed (the first min(n, pitch) of a row)
    int pitch;
    int32_t* len;                                     // (B) their count n
    int32_t* committed;                               // (B) the utterance's committed count after the call
    int32_t* rows;                                    // (B) the table rows in use after the call
    int32_t* status;                                  // (B) 1 applied, 0 refused, -1 header mismatch
};

// stage: (B, W, cap) int32 with cap = per_frame * F: the tails of the live hypotheses, walked out of the table before it is rewritten
__global__ __launch_bounds__(THREADS) void commit_kernel(int* __restrict__ hdr_all, int* len_all, int* __restrict__ node_all,
                                                         int2* __restrict__ table, CommitArrays arr, int B, int W, int F, int variant,
                                                         int per_frame, const int32_t* __restrict__ prefix_ids, int prefix_pitch,
                                                         const int32_t* __restrict__ prefix_len, int compact, int max_rows,
                                                         int32_t* __restrict__ stage_all, CommitOut out) {
    __shared__ int s_L[MAX_BEAM], s_k[MAX_BEAM], s_src[MAX_BEAM], s_l[MAX_BEAM];
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int* hdr = hdr_all + (size_t)b * HDR_WORDS;
    if (!state_matches(hdr, B, W, F, variant)) {
        if (tid == 0) {
            out.len[b] = 0;
            out.committed[b] = -1;
            out.rows[b] = -1;
            out.status[b] = -1;
        }
        return;
    }
    const int cap = per_frame * F, table_n = cap * W;
    const int m = min(max(hdr[H_M], 0), W), rows0 = min(max(hdr[H_FRAMES], 0), F), c = max(hdr[H_COMMITTED], 0);
    int2* nodes = table + (size_t)b * table_n;
    int32_t* stage = stage_all + (size_t)b * table_n;
    int* len = len_all + (size_t)b * W;
    int* node = node_all + (size_t)b * W;
    // 1. every live hypothesis walks its chain into its staging row: the tokens beyond the committed ones, L of them
    int L = 0;
    if (tid < m) {
        L = min(max(len[tid] - c, 0), cap);
        int32_t* row = stage + (size_t)tid * cap;
        int nd = node[tid], p = L - 1;
        for (; p >= 0; --p) {
            if ((unsigned)nd >= (unsigned)table_n) break;        // a state that other code wrote into: the chain ends here
            const int2 e = nodes[nd];
            row[p] = e.y;
            nd = e.x;
        }
        for (; p >= 0; --p) row[p] = -1;
        s_L[tid] = L;
    }
    __threadfence_block();
    __syncthreads();
    // 2. the prefix: the caller's, or the longest one that all live hypotheses share
    int n = prefix_ids ? prefix_len[b] : -1;
    const bool automatic = n < 0;
    bool keep = tid < m;
    if (automatic) {
        if (tid < m) {
            const int32_t* mine = stage + (size_t)tid * cap;
            const int lim = min(L, s_L[0]);
            int k = 0;
            while (k < lim && mine[k] == stage[k]) ++k;
            s_k[tid] = k;
        }
        __syncthreads();
        n = m > 0 ? s_k[0] : 0;
        for (int i = 1; i < m; ++i) n = min(n, s_k[i]);
    } else if (n > prefix_pitch) {
        keep = false;                                            // a prefix longer than its row: refused
    } else if (tid < m) {
        const int32_t* mine = stage + (size_t)tid * cap;
        const int32_t* P = prefix_ids + (size_t)b * prefix_pitch;
        keep = L >= n;
        for (int k = 0; keep && k < n; ++k) keep = mine[k] == P[k];
    }
    // 3. the kept hypotheses' places, the longest tail and the rows it needs
    int total;
    const int pos = block_excl_scan(keep ? 1 : 0, wsum, &total);
    if (tid < MAX_BEAM) s_l[tid] = 0;
    __syncthreads();
    if (keep) {
        s_src[pos] = tid;
        s_l[pos] = L - n;
    }
    __syncthreads();
    int maxl = 0;
    for (int i = 0; i < total; ++i) maxl = max(maxl, s_l[i]);
    const int rows = (maxl + per_frame - 1) / per_frame;
    if (total == 0 || rows > min(max_rows, F)) {
        if (tid == 0) {
            out.len[b] = 0;
            out.committed[b] = c;
            out.rows[b] = rows0;
            out.status[b] = 0;
        }
        return;
    }
    {
        const int32_t* first = stage + (size_t)s_src[0] * cap;
        for (int k = tid; k < min(n, out.pitch); k += THREADS) out.ids[(size_t)b * out.pitch + k] = first[k];
        if (tid == 0) {
            out.len[b] = n;
            out.committed[b] = c + n;
            out.rows[b] = rows;
            out.status[b] = 1;
        }
    }
    if (!compact) return;
    // 4. the per-slot arrays: every entry is read before any is written, then the kept ones go to the front in their order and
    // the slots they leave behind, up to the old m, get 0, so that the bytes of the state depend on what is kept alone
#pragma unroll
    for (int a = 0; a < MAX_ARR4; ++a) {
        if (a < arr.n4) {
            int* p = arr.a4[a] + (size_t)b * W;
            const int v = tid < m ? p[tid] : 0;
            __syncthreads();
            if (keep) p[pos] = v;
            if (tid >= total && tid < m) p[tid] = 0;
        }
    }
#pragma unroll
    for (int a = 0; a < MAX_ARR8; ++a) {
        if (a < arr.n8) {
            unsigned long long* p = arr.a8[a] + (size_t)b * W;
            const unsigned long long v = tid < m ? p[tid] : 0;
            __syncthreads();
            if (keep) p[pos] = v;
            if (tid >= total && tid < m) p[tid] = 0;
        }
    }
    // (pos < total <= the slots that get 0, and every slot below `total` is one kept entry's target: no slot is written twice)
    // 5. the table: tail position j of kept slot q is node j * W + q; the rows that were in use hold nothing else.  The chains were
    // read in step 1 and only the staging rows are read here.
    __threadfence();
    __syncthreads();
    const int fill = max(rows0, rows) * per_frame;
    for (int k = tid; k < fill * W; k += THREADS) {
        const int j = k / W, q = k - j * W;
        int2 e = make_int2(0, 0);
        if (q < total && j < s_l[q]) e = make_int2(j > 0 ? k - W : -1, stage[(size_t)s_src[q] * cap + n + j]);
        nodes[k] = e;
    }
    if (tid < m) node[tid] = tid < total ? (s_l[tid] > 0 ? (s_l[tid] - 1) * W + tid : -1) : 0;
    if (tid == 0) {
        hdr[H_M] = total;
        hdr[H_FRAMES] = rows;
        hdr[H_COMMITTED] = c + n;
    }
}

// the staging rows of commit_kernel
static size_t commit_ws_bytes(int B, int W, int F, int per_frame) { return align256((size_t)B * W * F * per_frame * 4); }

// what the two commit entries check besides their state, in the order of the other streaming entries
static int commit_check(int lim, const int32_t* prefix_ids, int prefix_pitch, const int32_t* prefix_len, int max_rows,
                        const void* workspace, const CommitOut& out) {
    if (lim == ASR_ERR_BAD_ARG) return lim;
    if (!workspace || !out.ids || !out.len || !out.committed || !out.rows || !out.status || out.pitch <= 0 || max_rows < 0)
        return ASR_ERR_BAD_ARG;
    if (prefix_ids && (!prefix_len || prefix_pitch <= 0)) return ASR_ERR_BAD_ARG;
    return lim;
}

}  // namespace beam
}  // namespace asr

extern "C" size_t asr_beam_stream_commit_workspace_bytes(int B, int beam_width, int max_frames, int per_frame) {
    if ((per_frame != 1 && per_frame != 2) || stream_dims(true, B, beam_width, max_frames, per_frame) != ASR_OK) return 0;
    return commit_ws_bytes(B, beam_width, max_frames, per_frame);
}

extern "C" int asr_ctc_beam_stream_commit(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames,
                                          int with_lm, int with_bias, const int32_t* prefix_ids, int prefix_pitch,
                                          const int32_t* prefix_len, int compact, int max_rows, void* workspace,
                                          size_t workspace_bytes, int32_t* out_ids, int out_pitch, int32_t* out_len,
                                          int32_t* out_committed, int32_t* out_rows, int32_t* out_status) {
    const CommitOut out{out_ids, out_pitch, out_len, out_committed, out_rows, out_status};
    const int rc = commit_check(stream_dims(state != nullptr, B, beam_width, max_frames, 1), prefix_ids, prefix_pitch, prefix_len,
                                max_rows, workspace, out);
    if (rc != ASR_OK) return rc;
    const int variant = ctc_variant(with_lm, with_bias);
    State s;
    if (state_bytes < state_layout(B, beam_width, max_frames, variant, (char*)state, &s)) return ASR_ERR_WORKSPACE;
    if (workspace_bytes < commit_ws_bytes(B, beam_width, max_frames, 1)) return ASR_ERR_WORKSPACE;
    CommitArrays arr{};
    for (void* p : {(void*)s.pb, (void*)s.pnb, (void*)s.len, (void*)s.last, (void*)s.plast, (void*)s.lm, (void*)s.c0, (void*)s.c1,
                    (void*)s.c2, (void*)s.open, (void*)s.state})
        if (p) arr.a4[arr.n4++] = (int*)p;
    arr.a8[arr.n8++] = s.hash;
    arr.a8[arr.n8++] = s.phash;
    hipLaunchKernelGGL(commit_kernel, dim3(B), dim3(THREADS), 0, (hipStream_t)stream, s.hdr, s.len, s.node, s.table, arr, B, beam_width,
                       max_frames, variant, 1, prefix_ids, prefix_pitch, prefix_len, compact, max_rows, (int32_t*)workspace, out);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_gram_ctc_beam_stream_commit(void* stream, void* state, size_t state_bytes, int B, int beam_width, int max_frames,
                                               int with_lm, int with_bias, const int32_t* prefix_ids, int prefix_pitch,
                                               const int32_t* prefix_len, int compact, int max_rows, void* workspace,
                                               size_t workspace_bytes, int32_t* out_ids, int out_pitch, int32_t* out_len,
                                               int32_t* out_committed, int32_t* out_rows, int32_t* out_status) {
    const CommitOut out{out_ids, out_pitch, out_len, out_committed, out_rows, out_status};
    const int rc = commit_check(stream_dims(state != nullptr, B, beam_width, max_frames, 2), prefix_ids, prefix_pitch, prefix_len,
                                max_rows, workspace, out);
    if (rc != ASR_OK) return rc;
    const int variant = gram_variant(with_lm, with_bias);
    GState s;
    GBiasState bs;
    if (state_bytes < gram_state_layout(B, beam_width, max_frames, variant, (char*)state, &s, &bs)) return ASR_ERR_WORKSPACE;
    if (workspace_bytes < commit_ws_bytes(B, beam_width, max_frames, 2)) return ASR_ERR_WORKSPACE;
    CommitArrays arr{};
    for (void* p : {(void*)s.pb, (void*)s.pu, (void*)s.pg, (void*)s.len, (void*)s.c1, (void*)s.c2, (void*)s.c3, (void*)s.utok,
                    (void*)s.gtok, (void*)s.lm, (void*)bs.open, (void*)bs.state})
        if (p) arr.a4[arr.n4++] = (int*)p;
    arr.a8[arr.n8++] = s.h0;
    arr.a8[arr.n8++] = s.h1;
    arr.a8[arr.n8++] = s.h2;
    hipLaunchKernelGGL(commit_kernel, dim3(B), dim3(THREADS), 0, (hipStream_t)stream, s.hdr, s.len, s.node, s.table, arr, B, beam_width,
                       max_frames, variant, 2, prefix_ids, prefix_pitch, prefix_len, compact, max_rows, (int32_t*)workspace, out);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
