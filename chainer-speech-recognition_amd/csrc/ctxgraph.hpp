// Contextual phrase biasing on the device: the image of an Aho-Corasick automaton over a phrase list and the step look-up shared
// by asr_ctx_score and the biased beam search of ctc_beam.hip.  The layout, the hash and the order of the
// f32 additions are stated in include/asr_hip.h; asr/bias.py builds the image.
//
//   keys (slots, 2) i32  (state, token) of a stored transition; an unused slot is -1 -1
//   vals (slots, 2) i32  (next state, the bits of the f32 delta) of the transition in the same slot
//   ret  (n_states) f32  -adv(state): what a match that is abandoned in `state` gives back
// The automaton is sparse and defaults to the root: (0, c) is stored where goto(0, c) != 0, (s, c) with s != 0 where
// goto(s, c) != goto(0, c).  The table follows the n-gram image's rules (ngram.hpp): a power of two of slots, linear probing,
// keys compared in full, and a probe sequence ends at a match, at an unused slot or after max_probe slots, so a damaged table
// gives wrong numbers but cannot make a kernel spin.  A `next` outside [0, n_states) counts as the root: `next` indexes ret.
//
// One step needs the two keys (s, c) and (0, c); both first probe addresses are known up front: step_issue starts every load,
// step_finish compares and combines, and only a linear-probe continuation is a dependent load.
#pragma once
#include "common.hpp"
#include "ngram.hpp"

namespace asr {
namespace ctx {

struct Graph {
    const int2* keys;            // nullptr: no stored transition (every step falls back to the root)
    const int2* vals;
    const float* ret;
    unsigned mask;               // slots - 1
    int max_probe, n_states;
};

// the n-gram image's hash over the key words (state, token, -1, -1)
__host__ __device__ inline unsigned slot_of(int s, int c, unsigned mask) { return ngram::slot_of(s, c, -1, -1, mask); }

struct Step {
    int2 q[2], k[2], v[2];       // 0: (s, c), 1: (0, c)
    unsigned s[2];
    float r;                     // ret[s]
    bool on;
};

// start every load of the step from state s (inside [0, n_states)) on token c
__device__ inline Step step_issue(const Graph& g, int s, int c) {
    Step st;
    st.on = g.keys != nullptr;
    st.r = g.ret[s];             // first, so that it flies with the probes instead of after their wait
    st.q[0] = make_int2(s, c);
    st.q[1] = make_int2(0, c);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        st.s[i] = slot_of(st.q[i].x, c, g.mask);
        st.k[i] = make_int2(-1, -1);
        st.v[i] = make_int2(0, 0);
    }
    if (st.on) {                 // s == 0: the same slot twice
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            st.k[i] = g.keys[st.s[i]];
            st.v[i] = g.vals[st.s[i]];
        }
    }
    return st;
}

// -> delta, *next.  Hit at (s, c): (next, delta); miss there, hit at (0, c): (next0, ret[s] + delta0); miss at both: (0, ret[s]).
__device__ inline float step_finish(const Graph& g, Step& st, int* next) {
    bool found[2] = {false, false}, pend[2] = {st.on, st.on};
    for (int p = 1;; ++p) {
        bool any = false;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (!pend[i]) continue;
            if (st.k[i].x == st.q[i].x && st.k[i].y == st.q[i].y) { found[i] = true; pend[i] = false; }
            else if (st.k[i].x == -1 || p >= g.max_probe) pend[i] = false;
            else { st.s[i] = (st.s[i] + 1) & g.mask; any = true; }
        }
        if (!any) break;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (pend[i]) {
                st.k[i] = g.keys[st.s[i]];
                st.v[i] = g.vals[st.s[i]];
            }
        }
    }
    int nx = 0;
    float d = st.r;
    if (found[0]) {
        nx = st.v[0].x;
        d = __int_as_float(st.v[0].y);
    } else if (found[1]) {
        nx = st.v[1].x;
        d = st.r + __int_as_float(st.v[1].y);
    }
    *next = (nx < 0 || nx >= g.n_states) ? 0 : nx;
    return d;
}

__device__ inline float step(const Graph& g, int s, int c, int* next) {
    Step st = step_issue(g, s, c);
    return step_finish(g, st, next);
}

}  // namespace ctx
}  // namespace asr
