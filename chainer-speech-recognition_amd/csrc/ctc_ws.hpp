// Workspace of the CTC / Gram-CTC kernels (csrc/ctc.hip), shared with the fused layer-norm + CTC backward (csrc/ctc_ln.hip).
#pragma once
#include "common.hpp"

namespace asr {
namespace ctc {

struct Workspace {
    int* path_label;   // (B, Sp)  -1 = dead / outside the path
    int* path_mask;    // (B, Sp)  bit j set: edge from s - k_j into s
    int* path_len;     // (B)
    float* lse;        // (T, B)
    float* lp;         // (B, T, Sp)
    double* alpha;     // (B, T, Sp)
    double* beta;      // (B, T, Sp)
    double* total;     // (B)
    size_t bytes;
};

static inline int path_pad(int Lmax, int gram) {
    const int S = (gram ? 3 : 2) * Lmax + 1;
    return (int)align_up((size_t)S, 64);
}

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
    w.lp = (float*)take(sizeof(float) * (size_t)B * T * Sp);
    w.alpha = (double*)take(sizeof(double) * (size_t)B * T * Sp);
    w.beta = (double*)take(sizeof(double) * (size_t)B * T * Sp);
    w.total = (double*)take(sizeof(double) * B);
    w.bytes = off;
    return w;
}

// Workspace of the N-best scoring (csrc/ctc_nbest.hip): the loss's tables for B * N lattices, "utterance" u = b * N + n, and ONE
// log-sum-exp per logit row (the N hypotheses of an utterance share its rows).
struct NbestWorkspace {
    int* path_label;   // (B*N, Sp)
    int* path_mask;    // (B*N, Sp)
    int* path_len;     // (B*N)
    int* x_len;        // (B*N)    frames of utterance b for a used slot, 0 for an unused one (the sweep then reports -inf)
    float* lse;        // (T, B)
    float* lp;         // (B*N, T, Sp)
    double* alpha;     // (B*N, T, Sp)
    double* beta;      // (B*N, T, Sp)
    double* total;     // (B*N)    log p(h_n | x_b), -inf: unused or infeasible
    float* loss;       // (B*N)    what the sweep writes beside total (unused here)
    // Gram-CTC only (gram = 1): the lattice's two label rows, looked up from the hypothesis' characters, and the spelling index
    int* lab_uni;      // (B*N, Lmax)  token that spells (s[i]), -1: none
    int* lab_big;      // (B*N, Lmax)  token that spells (s[i-1], s[i]), -1: none; [0] = -1
    int* eff_len;      // (B*N)    hyp_len clamped to Lmax; -1: unused, or a character without a unigram token
    unsigned long long* idx_key;   // (capacity)  spelling, first character in the high word; all ones (the blank's (-1, -1)): empty
    int* idx_val;      // (capacity)  the smallest token id with that spelling
    size_t idx_cap;    // the power of two >= 2 V
    size_t bytes;
};

// capacity of the spelling index: the power of two >= 2 V (load <= 0.5: every linear probe ends at an empty slot)
static inline size_t gram_index_capacity(int V) {
    size_t cap = 2;
    while (cap < 2 * (size_t)V) cap <<= 1;
    return cap;
}

// gram = 0: the CTC lattices (V is not used); gram = 1: the Gram-CTC lattices, their label rows and the spelling index of V tokens
static NbestWorkspace carve_nbest(void* base, int T, int B, int N, int Lmax, int gram, int V) {
    NbestWorkspace w;
    const size_t Sp = (size_t)path_pad(Lmax, gram), U = (size_t)B * N;
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t n) { char* r = p ? p + off : nullptr; off += align_up(n, 256); return r; };
    w.path_label = (int*)take(sizeof(int) * U * Sp);
    w.path_mask = (int*)take(sizeof(int) * U * Sp);
    w.path_len = (int*)take(sizeof(int) * U);
    w.x_len = (int*)take(sizeof(int) * U);
    w.lse = (float*)take(sizeof(float) * (size_t)T * B);
    w.lp = (float*)take(sizeof(float) * U * T * Sp);
    w.alpha = (double*)take(sizeof(double) * U * T * Sp);
    w.beta = (double*)take(sizeof(double) * U * T * Sp);
    w.total = (double*)take(sizeof(double) * U);
    w.loss = (float*)take(sizeof(float) * U);
    w.lab_uni = w.lab_big = w.eff_len = w.idx_val = nullptr;
    w.idx_key = nullptr;
    w.idx_cap = 0;
    if (gram) {
        w.idx_cap = gram_index_capacity(V);
        w.lab_uni = (int*)take(sizeof(int) * U * Lmax);
        w.lab_big = (int*)take(sizeof(int) * U * Lmax);
        w.eff_len = (int*)take(sizeof(int) * U);
        w.idx_key = (unsigned long long*)take(sizeof(unsigned long long) * w.idx_cap);
        w.idx_val = (int*)take(sizeof(int) * w.idx_cap);
    }
    w.bytes = off;
    return w;
}

}  // namespace ctc
}  // namespace asr
