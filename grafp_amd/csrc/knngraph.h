// knngraph.h -- what the three generations of the encoder's dynamic k-NN graph share: knn_graph.hip (exact-f32 MFMA),
// knn_pre.hip (bf16 pre-filter + exact rescoring), knn_split.hip (split / raw bf16 Gram, certified order + exact
// recomputation).  Device helpers and two host helpers, no state.
//
// THE arithmetic contract (oracle/csrc/knn_graph.c; all three files return its indices bit for bit):
//   * norm:      ss = fmaf(v_c, v_c, ss) over c ascending from 0; den = max(sqrtf(ss), 1e-12); xn_c = v_c / den (IEEE
//                division); sq = fmaf(xn_c, xn_c, sq) over c ascending.  sqrtf, not __fsqrt_rn: only the former is
//                correctly rounded here (with -fhip-fp32-correctly-rounded-divide-sqrt); the intrinsic is 1 ulp off for
//                ~15 % of arguments.
//   * Gram:      g = fmaf(xn_i[c], xn_j[c], g) over c ascending from 0 (v_mfma_f32_32x32x2_f32 is bitwise this chain).
//   * distance:  (sq_i + (-2 g)) + sq_j, written fmaf(-2, g, sq_i) + sq_j (the product is exact).
//   * order:     ascending (distance, index): ties go to the lowest index.
// The build's -ffp-contract=off fuses nothing by itself: every fmaf below is spelled out.
#pragma once
#include <math.h>

#include "elemio.h"

namespace grafp {

constexpr int KNN_TQ = 128;  // query nodes per workgroup (32 per wave)
constexpr int KNN_TR = 128;  // candidate nodes per block

// Where a thread of a 256-thread scan workgroup stands: clip b, first query q0 of the workgroup's tile (XCD-remapped),
// and the lane's place in its wave.  A lane's query is q0 + wave * 32 + l31; its half-wave sees the candidate rows
// mfma_row(., half).  Kernels that need `wave` in a scalar register take readfirstlane of it themselves.
struct KnnCoords {
    int b, q0, tid, wave, lane, half, l31;
};
__device__ __forceinline__ KnnCoords knn_coords(int nblocks, int tiles_per_clip) {
    const int bid = xcd_remap(blockIdx.x, nblocks);
    const int tid = threadIdx.x, lane = tid & 63;
    return {bid / tiles_per_clip, (bid % tiles_per_clip) * KNN_TQ, tid, tid >> 6, lane, lane >> 5, lane & 31};
}

// ---- the norm chains of ONE node, xb[c * sc] over c = 0 .. C-1: loads run 8 channels ahead of the dependent chain ------
template <typename T>
__device__ __forceinline__ float knn_node_den(const T *xb, int64_t sc, int C) {
    float ss = 0.0f;
    int c = 0;
    for (; c + 8 <= C; c += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ld_as_f32(xb + (size_t)(c + u) * sc);
#pragma unroll
        for (int u = 0; u < 8; ++u) ss = __builtin_fmaf(v[u], v[u], ss);
    }
    for (; c < C; ++c) {
        const float v = ld_as_f32(xb + (size_t)c * sc);
        ss = __builtin_fmaf(v, v, ss);
    }
    return fmaxf(sqrtf(ss), 1e-12f);
}
// the quotient pass: put(c, v_c / den) for every channel (v_c itself when !normalize); returns sq
template <typename T, typename F>
__device__ __forceinline__ float knn_node_quotients(const T *xb, int64_t sc, int C, int normalize, float den, F &&put) {
    float q = 0.0f;
    int c = 0;
    for (; c + 8 <= C; c += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ld_as_f32(xb + (size_t)(c + u) * sc);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (normalize) v[u] = __fdiv_rn(v[u], den);
            put(c + u, v[u]);
            q = __builtin_fmaf(v[u], v[u], q);
        }
    }
    for (; c < C; ++c) {
        float v = ld_as_f32(xb + (size_t)c * sc);
        if (normalize) v = __fdiv_rn(v, den);
        put(c, v);
        q = __builtin_fmaf(v, v, q);
    }
    return q;
}

// ---- the K best (distance, index) of a lane, ascending ---------------------------------------------------------------
template <int K>
struct TopK {
    float d[K];
    int i[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            d[t] = INFINITY;
            i[t] = 0x7fffffff;
        }
    }
    // Sorted insert as a carry chain of plain selects (branch-free).  `take` compares the ORIGINAL new
    // value with each OLD slot: in a sorted list that predicate is monotone (false...false,true...true),
    // so the first true slot receives the new element and every later slot receives its predecessor.
    // Candidates arrive in ascending index order within a lane, so strict '<' keeps the lower index on
    // ties, and a displaced (older) element always moves down regardless of ties.
    __device__ __forceinline__ void push_ascending(float v, int vi) {
        const float v0 = v;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const bool take = v0 < d[t];
            const float od = d[t];
            const int oi = i[t];
            d[t] = take ? v : od;
            i[t] = take ? vi : oi;
            v = take ? od : v;
            vi = take ? oi : vi;
        }
    }
    // arbitrary order: full (distance, index) lexicographic comparison
    __device__ __forceinline__ void push_lex(float v, int vi) {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const bool lt = v < d[t] || (v == d[t] && vi < i[t]);
            const float lo = lt ? v : d[t], hi = lt ? d[t] : v;
            const int ilo = lt ? vi : i[t], ihi = lt ? i[t] : vi;
            d[t] = lo; i[t] = ilo;
            v = hi; vi = ihi;
        }
    }
    // the two half-waves of a scan saw disjoint candidate subsets of the same query: each takes the other's list
    __device__ __forceinline__ void merge_halves() {
        float od[K];
        int oi[K];
#pragma unroll
        for (int t = 0; t < K; ++t) {
            od[t] = __shfl_xor(d[t], 32);
            oi[t] = __shfl_xor(i[t], 32);
        }
#pragma unroll
        for (int t = 0; t < K; ++t) push_lex(od[t], oi[t]);
    }
    template <typename I>
    __device__ __forceinline__ void store(I *o) const {      // o: the query's K output slots
#pragma unroll
        for (int t = 0; t < K; ++t) o[t] = (I)i[t];
    }
};

}  // namespace grafp
