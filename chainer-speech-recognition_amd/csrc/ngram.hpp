// Back-off n-gram language model over token ids on the device (orders 1-4, natural log, ARPA semantics): the table layout and
// the step look-up shared by asr_ngram_score and the fused beam search of ctc_beam.hip.  The layout, the hash and the order of
// the f32 additions are stated in include/asr_hip.h; asr/lm.py builds the image and restates the hash on uint64.
//
//   uni  (vlm, 2) f32   (logp, backoff) of every id: dense, so a back-off chain always ends here
//   keys (slots, 4) i32 the n-gram's tokens, oldest first, padded with -1; an unused slot is all -1
//   vals (slots, 2) f32 (logp, backoff) of the n-gram in the same slot
// slots is a power of two, linear probing, and no look-up needs more than max_probe probes: a probe sequence ends at a match, at
// an unused slot or after max_probe slots, so a damaged table gives wrong numbers but cannot make a kernel spin.
//
// One step P(w | c2 c1 c0) needs up to three n-gram keys and two context keys (the third context is a unigram).  All of their
// first probe addresses are known up front: step_issue starts every load, step_finish compares and combines, and only a
// linear-probe continuation (rare at load <= 0.5) is a dependent load.
#pragma once
#include "common.hpp"

namespace asr {
namespace ngram {

constexpr int MAX_ORDER = 4;
constexpr int NQ = 5;            // hash look-ups of a step: 2-, 3-, 4-gram ending in w, then the 2- and 3-token contexts

struct Lm {
    const float2* uni;
    const int4* keys;            // nullptr: no n-gram above order 1
    const float2* vals;
    unsigned mask;               // slots - 1
    int max_probe, order, vlm;
};

__host__ __device__ inline unsigned slot_of(int a, int b, int c, int d, unsigned mask) {
    unsigned long long h = 0x9E3779B97F4A7C15ull;
    h = (h ^ (unsigned long long)(unsigned)a) * 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    h = (h ^ (unsigned long long)(unsigned)b) * 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    h = (h ^ (unsigned long long)(unsigned)c) * 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    h = (h ^ (unsigned long long)(unsigned)d) * 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return (unsigned)h & mask;
}

struct Step {
    int4 q[NQ], k[NQ];
    float2 v[NQ];
    unsigned s[NQ];
    bool on[NQ];
    float2 uw;                   // the unigram entry of w
    float b1;                    // the back-off weight of the one-token context
    int L;                       // context length in use
    bool bad;                    // w outside the model's ids: the step is NaN
};

__device__ inline bool same(const int4& a, const int4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

// start every load of P(w | c2 c1 c0): c0 is the newest context token, -1 (or an id outside the model) ends the context there
__device__ inline Step step_issue(const Lm& lm, int c0, int c1, int c2, int w) {
    Step st;
    auto in = [&](int c) { return c >= 0 && c < lm.vlm; };
    const bool tab = lm.keys != nullptr;
    const bool h0 = lm.order >= 2 && in(c0), h1 = h0 && lm.order >= 3 && in(c1), h2 = h1 && lm.order >= 4 && in(c2);
    st.L = (int)h0 + (int)h1 + (int)h2;
    st.bad = !in(w);
    st.q[0] = make_int4(c0, w, -1, -1);  st.on[0] = tab && h0 && !st.bad;
    st.q[1] = make_int4(c1, c0, w, -1);  st.on[1] = tab && h1 && !st.bad;
    st.q[2] = make_int4(c2, c1, c0, w);  st.on[2] = tab && h2 && !st.bad;
    st.q[3] = make_int4(c1, c0, -1, -1); st.on[3] = tab && h1 && !st.bad;
    st.q[4] = make_int4(c2, c1, c0, -1); st.on[4] = tab && h2 && !st.bad;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        st.s[i] = slot_of(st.q[i].x, st.q[i].y, st.q[i].z, st.q[i].w, lm.mask);
        st.k[i] = make_int4(-1, -1, -1, -1);
        st.v[i] = make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        if (st.on[i]) {
            st.k[i] = lm.keys[st.s[i]];
            st.v[i] = lm.vals[st.s[i]];
        }
    }
    st.uw = st.bad ? make_float2(0.f, 0.f) : lm.uni[w];
    st.b1 = h0 ? lm.uni[c0].y : 0.f;
    return st;
}

// The f32 sum, in this order: 0, + the back-off weight of every context longer than the one that hit, longest first (0 where the
// context is not in the model), + the log-probability of the hit (the unigram's when no n-gram hit).
__device__ inline float step_finish(const Lm& lm, Step& st) {
    if (st.bad) return __int_as_float(0x7fc00000);
    bool found[NQ], pend[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) { found[i] = false; pend[i] = st.on[i]; }
    for (int p = 1;; ++p) {
        bool any = false;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            if (!pend[i]) continue;
            if (same(st.k[i], st.q[i])) { found[i] = true; pend[i] = false; }
            else if (st.k[i].x == -1 || p >= lm.max_probe) pend[i] = false;
            else { st.s[i] = (st.s[i] + 1) & lm.mask; any = true; }
        }
        if (!any) break;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            if (pend[i]) {
                st.k[i] = lm.keys[st.s[i]];
                st.v[i] = lm.vals[st.s[i]];
            }
        }
    }
    int hit = 0;
    if (st.L >= 3 && found[2]) hit = 3;
    else if (st.L >= 2 && found[1]) hit = 2;
    else if (st.L >= 1 && found[0]) hit = 1;
    float acc = 0.f;
    if (st.L >= 3 && hit < 3) acc += found[4] ? st.v[4].y : 0.f;
    if (st.L >= 2 && hit < 2) acc += found[3] ? st.v[3].y : 0.f;
    if (st.L >= 1 && hit < 1) acc += st.b1;
    acc += hit == 3 ? st.v[2].x : hit == 2 ? st.v[1].x : hit == 1 ? st.v[0].x : st.uw.x;
    return acc;
}

__device__ inline float step(const Lm& lm, int c0, int c1, int c2, int w) {
    Step st = step_issue(lm, c0, c1, c2, w);
    return step_finish(lm, st);
}

}  // namespace ngram
}  // namespace asr
