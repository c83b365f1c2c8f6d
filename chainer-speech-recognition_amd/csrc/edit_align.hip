// Edit alignment and N-best consensus on the GPU (gfx950): the Levenshtein table of decode.hip's edit_distance with the path kept.
//
//   asr_edit_align               distance, substitutions, deletions, insertions and the two position maps of one optimal alignment
//                                per (reference, hypothesis) pair
//   asr_nbest_pairwise_distance  the N x N distance matrix of every utterance's N-best list, read in place
//   asr_nbest_consensus          posterior mass of the list that agrees with a pivot hypothesis, token by token
//
// One workgroup of one wave per pair sweeps the table d[i][j] by anti-diagonals k = i + j held in LDS (three diagonals of
// ref_pitch + 1 ints, indexed by i), as edit_distance_kernel does.  Several alignments reach the same distance; the one reported
// is pinned by the trace-back rule, from (i, j) = (n, m):
//     i == 0: insertion;  j == 0: deletion;  r[i-1] == h[j-1]: match;
//     d[i][j] == d[i-1][j-1] + 1: substitution;  d[i][j] == d[i-1][j] + 1: deletion;  else insertion.
// The same priority applied while a cell is computed names the cell's predecessor, so the pinned path to (i, j) is the pinned path
// to its predecessor plus one step, and the number of substitutions on it can be carried forward with the distance: a cell is the
// word  d << 13 | S  (S <= min(n, m) <= 5460 < 2^13, d <= max(n, m) < 2^19).  With i - j = D - I and d = S + D + I the other two
// counts follow at (n, m), so the counts need no back-pointers.  The maps do: one byte per inner cell (1 substitution, 2 deletion,
// 3 insertion; matches and the borders are decided from the ids), written with byte stores (no lane reads a word that another
// lane writes) and walked back by lane 0 after the sweep's last barrier.  The table is laid out the way it is written, diagonal
// by diagonal: row k - 2 holds the cells i = max(1, k - m) .. min(n, k - 1) of diagonal k from column 0 on, so the lanes of one
// store write neighbouring bytes (with row-major cells every lane of a store is in a cache line of its own, and the stores cost
// five times the sweep: profiles/edit_align.txt).  A
// diagonal has at most min(n, m) inner cells and there are n + m - 1 of them: (ref_pitch + hyp_pitch - 1) * min(ref_pitch,
// hyp_pitch) bytes per pair, never more than twice the cells.
#include "common.hpp"
#include "../../include/asr_hip.h"

namespace asr {
namespace edit_align {

constexpr int kSBits = 13;                       // substitutions of the pinned path: the low bits of a cell
constexpr unsigned kSMask = (1u << kSBits) - 1;
constexpr int kMaxHypPitch = (1 << (32 - kSBits)) - 1;
enum : unsigned char { kSub = 1, kDel = 2, kIns = 3 };

__host__ __device__ inline size_t lds_bytes(int ref_pitch) { return (size_t)3 * ((size_t)ref_pitch + 1) * sizeof(unsigned); }
// back-pointer bytes of one pair, and where cell (i, j), i, j >= 1, of a hypothesis of m tokens lives (width = min of the pitches)
__host__ __device__ inline size_t bp_bytes(int ref_pitch, int hyp_pitch) {
    return ((size_t)ref_pitch + hyp_pitch - 1) * (size_t)(ref_pitch < hyp_pitch ? ref_pitch : hyp_pitch);
}
__device__ inline size_t bp_index(int i, int j, int m, int width) { return (size_t)(i + j - 2) * width + (i - max(1, i + j - m)); }

// Sweeps the table of r[0..n) against h[0..m) over three diagonals of `stride` words in `lds` and returns cell (n, m) to every lane.
// COUNTS: cells are d << 13 | S, else plain distances.  BP: the predecessor of every inner cell (i, j >= 1) that is not a match goes
// to bp[bp_index(i, j, m, bp_width)].  Ends behind a workgroup barrier: the back-pointers are visible to every lane.
template <bool COUNTS, bool BP>
__device__ inline unsigned sweep(const int32_t* __restrict__ r, int n, const int32_t* __restrict__ h, int m, unsigned* lds,
                                 int stride, unsigned char* __restrict__ bp, int bp_width) {
    constexpr int sh = COUNTS ? kSBits : 0;
    const int lane = threadIdx.x;
    unsigned* d0 = lds;                  // diagonal k - 2
    unsigned* d1 = lds + stride;         // diagonal k - 1
    unsigned* d2 = lds + 2 * stride;     // diagonal k
    for (int k = 0; k <= n + m; ++k) {
        const int ilo = max(0, k - m), ihi = min(n, k);
        for (int i = ilo + lane; i <= ihi; i += 64) {
            const int j = k - i;
            unsigned v;
            if (i == 0) v = (unsigned)j << sh;
            else if (j == 0) v = (unsigned)i << sh;
            else if (r[i - 1] == h[j - 1]) v = d0[i - 1];
            else {
                const unsigned sub = d0[i - 1], del = d1[i - 1], ins = d1[i];      // d[i-1][j-1], d[i-1][j], d[i][j-1]
                const unsigned ds = sub >> sh, dd = del >> sh, di = ins >> sh;
                const unsigned best = min(ds, min(dd, di));
                unsigned char code;
                if (ds == best) { v = sub + (1u << sh) + (COUNTS ? 1u : 0u); code = kSub; }
                else if (dd == best) { v = del + (1u << sh); code = kDel; }
                else { v = ins + (1u << sh); code = kIns; }
                if (BP) bp[bp_index(i, j, m, bp_width)] = code;
            }
            d2[i] = v;
        }
        __syncthreads();
        unsigned* t = d0; d0 = d1; d1 = d2; d2 = t;
    }
    return d1[n];
}

// The pinned path from (n, m) back to (0, 0), one lane.  Every reference position < n and every hypothesis position < m is visited
// once: rmap / hmap (either may be null) get their partner or -1; hit (may be null) gets 1 where the partner carries the same id.
__device__ inline void trace_back(const int32_t* __restrict__ r, int n, const int32_t* __restrict__ h, int m,
                                  const unsigned char* __restrict__ bp, int bp_width, int32_t* __restrict__ rmap,
                                  int32_t* __restrict__ hmap, unsigned char* __restrict__ hit) {
    int i = n, j = m;
    while (i > 0 || j > 0) {
        unsigned char code;
        bool same = false;
        if (i == 0) code = kIns;
        else if (j == 0) code = kDel;
        else if (r[i - 1] == h[j - 1]) { code = kSub; same = true; }
        else code = bp[bp_index(i, j, m, bp_width)];
        if (code == kSub) {
            --i; --j;
            if (rmap) rmap[i] = j;
            if (hmap) hmap[j] = i;
            if (hit) hit[i] = same ? 1 : 0;
        } else if (code == kDel) {
            --i;
            if (rmap) rmap[i] = -1;
            if (hit) hit[i] = 0;
        } else {
            --j;
            if (hmap) hmap[j] = -1;
        }
    }
}

__device__ inline int clamp_len(int len, int pitch) { return min(max(len, 0), pitch); }

template <bool PATHS>
__global__ __launch_bounds__(64) void align_kernel(const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int ref_pitch,
                                                   const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, int hyp_pitch,
                                                   int32_t* __restrict__ counts, int32_t* __restrict__ ref_to_hyp,
                                                   int32_t* __restrict__ hyp_to_ref, unsigned char* __restrict__ bp_all) {
    extern __shared__ unsigned lds[];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int n = clamp_len(ref_len[p], ref_pitch), m = clamp_len(hyp_len[p], hyp_pitch);
    const int32_t* r = ref + (size_t)p * ref_pitch;
    const int32_t* h = hyp + (size_t)p * hyp_pitch;
    unsigned char* bp = PATHS ? bp_all + (size_t)p * bp_bytes(ref_pitch, hyp_pitch) : nullptr;
    const int bp_width = min(ref_pitch, hyp_pitch);
    const unsigned cell = sweep<true, PATHS>(r, n, h, m, lds, ref_pitch + 1, bp, bp_width);
    if (lane == 0) {
        const int d = (int)(cell >> kSBits), s = (int)(cell & kSMask), del = (d - s + n - m) / 2;
        int32_t* c = counts + (size_t)p * 4;
        c[0] = d; c[1] = s; c[2] = del; c[3] = del - (n - m);
    }
    if (PATHS) {
        int32_t* rmap = ref_to_hyp ? ref_to_hyp + (size_t)p * ref_pitch : nullptr;
        int32_t* hmap = hyp_to_ref ? hyp_to_ref + (size_t)p * hyp_pitch : nullptr;
        if (rmap) for (int i = n + lane; i < ref_pitch; i += 64) rmap[i] = -1;        // the padding; the path writes the rest
        if (hmap) for (int j = m + lane; j < hyp_pitch; j += 64) hmap[j] = -1;
        if (lane == 0) trace_back(r, n, h, m, bp, bp_width, rmap, hmap, nullptr);
    }
}

// one workgroup per (b, i <= j): i == j is the diagonal, written and left
__global__ __launch_bounds__(64) void pairwise_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ lens, int N, int pitch,
                                                      int32_t* __restrict__ dist) {
    extern __shared__ unsigned lds[];
    const int per = N * (N + 1) / 2;
    const int b = blockIdx.x / per;
    int q = blockIdx.x - b * per, i = 0;
    while (q >= N - i) { q -= N - i; ++i; }
    const int j = i + q;
    int32_t* out = dist + (size_t)b * N * N;
    if (i == j) {
        if (threadIdx.x == 0) out[(size_t)i * N + i] = 0;
        return;
    }
    const int li = lens[(size_t)b * N + i], lj = lens[(size_t)b * N + j];
    unsigned d = 0;
    if (li >= 0 && lj >= 0) {                                       // a negative length: the slot is unused, row and column 0
        const int32_t* r = ids + ((size_t)b * N + i) * pitch;
        const int32_t* h = ids + ((size_t)b * N + j) * pitch;
        d = sweep<false, false>(r, min(li, pitch), h, min(lj, pitch), lds, pitch + 1, nullptr, 0);
    }
    if (threadIdx.x == 0) {
        out[(size_t)i * N + j] = (int32_t)d;
        out[(size_t)j * N + i] = (int32_t)d;
    }
}

// one workgroup per (b, j): hypothesis j against the pivot of utterance b as the reference; hit (B, N, pitch) bytes
__global__ __launch_bounds__(64) void consensus_align_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ pivot, int N, int pitch,
                                                             unsigned char* __restrict__ bp_all, unsigned char* __restrict__ hit_all) {
    extern __shared__ unsigned lds[];
    const int b = blockIdx.x / N, j = blockIdx.x - b * N;
    const int pv = pivot[b];
    if (pv < 0 || pv >= N) return;
    const int lp = lens[(size_t)b * N + pv], lj = lens[(size_t)b * N + j];
    if (lp < 0 || lj < 0) return;                                   // conf_kernel reads neither
    const int n = min(lp, pitch), m = min(lj, pitch);
    const int32_t* r = ids + ((size_t)b * N + pv) * pitch;
    const int32_t* h = ids + ((size_t)b * N + j) * pitch;
    unsigned char* bp = bp_all + (size_t)blockIdx.x * bp_bytes(pitch, pitch);
    sweep<false, true>(r, n, h, m, lds, pitch + 1, bp, pitch);
    if (threadIdx.x == 0) trace_back(r, n, h, m, bp, pitch, nullptr, nullptr, hit_all + (size_t)blockIdx.x * pitch);
}

// conf[b][l] = sum over the used slots j, in index order, of post[b][j] where slot j agrees with the pivot at l: one thread per l
__global__ __launch_bounds__(256) void conf_kernel(const int32_t* __restrict__ lens, const int32_t* __restrict__ pivot,
                                                   const float* __restrict__ post, int N, int pitch,
                                                   const unsigned char* __restrict__ hit_all, float* __restrict__ conf) {
    const int b = blockIdx.y, l = blockIdx.x * 256 + threadIdx.x;
    if (l >= pitch) return;
    const int pv = pivot[b];
    const int lp = pv >= 0 && pv < N ? lens[(size_t)b * N + pv] : -1;
    float acc = 0.0f;
    if (l < min(lp, pitch)) {
        for (int j = 0; j < N; ++j) {
            if (lens[(size_t)b * N + j] < 0) continue;
            if (hit_all[((size_t)b * N + j) * pitch + l]) acc += post[(size_t)b * N + j];
        }
    }
    conf[(size_t)b * pitch + l] = acc;
}

}  // namespace edit_align
}  // namespace asr

using namespace asr;
using namespace asr::edit_align;

extern "C" size_t asr_edit_align_workspace_bytes(int pairs, int ref_pitch, int hyp_pitch) {
    if (pairs <= 0 || ref_pitch <= 0 || hyp_pitch <= 0) return 0;
    return (size_t)pairs * bp_bytes(ref_pitch, hyp_pitch);
}

extern "C" int asr_edit_align(void* stream, const int32_t* ref, const int32_t* ref_len, int ref_pitch, const int32_t* hyp,
                              const int32_t* hyp_len, int hyp_pitch, int pairs, int32_t* counts, int32_t* ref_to_hyp,
                              int32_t* hyp_to_ref, void* workspace, size_t workspace_bytes) {
    if (!ref || !ref_len || !hyp || !hyp_len || !counts || pairs <= 0 || ref_pitch <= 0 || hyp_pitch <= 0) return ASR_ERR_BAD_ARG;
    const size_t lds = lds_bytes(ref_pitch);
    if (lds > 64 * 1024 || hyp_pitch > kMaxHypPitch) return ASR_ERR_UNSUPPORTED;      // ref_pitch <= 5460: S fits its 13 bits
    if (ref_to_hyp || hyp_to_ref) {
        if (!workspace) return ASR_ERR_BAD_ARG;
        if (workspace_bytes < asr_edit_align_workspace_bytes(pairs, ref_pitch, hyp_pitch)) return ASR_ERR_WORKSPACE;
        hipLaunchKernelGGL(align_kernel<true>, dim3(pairs), dim3(64), lds, (hipStream_t)stream, ref, ref_len, ref_pitch, hyp, hyp_len,
                           hyp_pitch, counts, ref_to_hyp, hyp_to_ref, (unsigned char*)workspace);
    } else {
        hipLaunchKernelGGL(align_kernel<false>, dim3(pairs), dim3(64), lds, (hipStream_t)stream, ref, ref_len, ref_pitch, hyp, hyp_len,
                           hyp_pitch, counts, nullptr, nullptr, nullptr);
    }
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" int asr_nbest_pairwise_distance(void* stream, const int32_t* ids, const int32_t* lens, int B, int N, int pitch,
                                           int32_t* dist) {
    if (!ids || !lens || !dist || B <= 0 || N <= 0 || pitch <= 0) return ASR_ERR_BAD_ARG;
    const size_t lds = lds_bytes(pitch);
    const long long blocks = (long long)B * ((long long)N * (N + 1) / 2);
    if (lds > 64 * 1024 || blocks > 0x7fffffffLL) return ASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pairwise_kernel, dim3((unsigned)blocks), dim3(64), lds, (hipStream_t)stream, ids, lens, N, pitch, dist);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}

extern "C" size_t asr_nbest_consensus_workspace_bytes(int B, int N, int pitch) {
    if (B <= 0 || N <= 0 || pitch <= 0) return 0;
    return (size_t)B * N * bp_bytes(pitch, pitch) + (size_t)B * N * pitch;       // back-pointers, then the agreement bytes
}

extern "C" int asr_nbest_consensus(void* stream, const int32_t* ids, const int32_t* lens, const int32_t* pivot, const float* post,
                                   int B, int N, int pitch, float* conf, void* workspace, size_t workspace_bytes) {
    if (!ids || !lens || !pivot || !post || !conf || !workspace || B <= 0 || N <= 0 || pitch <= 0) return ASR_ERR_BAD_ARG;
    const size_t lds = lds_bytes(pitch);
    if (lds > 64 * 1024 || (long long)B * N > 0x7fffffffLL || B > 65535) return ASR_ERR_UNSUPPORTED;
    if (workspace_bytes < asr_nbest_consensus_workspace_bytes(B, N, pitch)) return ASR_ERR_WORKSPACE;
    unsigned char* bp = (unsigned char*)workspace;
    unsigned char* hit = bp + (size_t)B * N * bp_bytes(pitch, pitch);
    hipLaunchKernelGGL(consensus_align_kernel, dim3((unsigned)(B * N)), dim3(64), lds, (hipStream_t)stream, ids, lens, pivot, N, pitch, bp,
                       hit);
    ASR_LAUNCH_CHECK();
    hipLaunchKernelGGL(conf_kernel, dim3((unsigned)((pitch + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, lens, pivot,
                       post, N, pitch, hit, conf);
    ASR_LAUNCH_CHECK();
    return ASR_OK;
}
