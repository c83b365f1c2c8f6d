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
    size_t bytes;
};

static NbestWorkspace carve_nbest(void* base, int T, int B, int N, int Lmax) {
    NbestWorkspace w;
    const size_t Sp = (size_t)path_pad(Lmax, 0), U = (size_t)B * N;
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
    w.bytes = off;
    return w;
}

}  // namespace ctc
}  // namespace asr
