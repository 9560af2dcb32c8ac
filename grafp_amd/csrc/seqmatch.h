// seqmatch.h -- what the sequence-matching kernels share: seq_rerank.hip (row-level rerank), identify.hip and
// identify_pq.hip (track-aware identification), selfmatch.hip and crossmatch.hip (shared audio inside a library, and of
// recordings against one).  Device helpers, and at the end what their host launches share (the speed ratios of the
// tempo kernels, the launch with reserved LDS); no state; compiles with and without the packed-f32 instructions
// (Makefile NOPK).
//
// THE arithmetic order of a span score (restated for the CPU in oracle/csrc/seq_rerank.c and tests/_identify_ref.py):
// a span is m pairs of 128-float rows (x[t], y[t]), t = 0..m-1.  Lane l of a 32-lane half-wave owns dims 4l..4l+3 and
// runs ONE fmaf chain over (t ascending, e = 0..3): acc = fmaf(x[t][4l+e], y[t][4l+e], acc), from acc = 0; the 32 lane
// sums are combined by the butterfly s = 16, 8, 4, 2, 1 (acc[l] + acc[l ^ s]); score = sum / m (IEEE division, by the
// caller).  All three kernels score through span_sum, so a span that two of them see gets the same bits.
#pragma once
#include "common.h"

namespace grafp {

constexpr int SEQ_D = 128;                                  // floats per fingerprint row
constexpr unsigned long long SEQ_NONE = ~0ull;              // the empty key: sorts last

// monotone map f32 -> u32 (larger float = larger integer), and back
__device__ __forceinline__ unsigned int f32_ord(float f) {
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_f32(unsigned int o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// the track t in [lo, T) with first[t] <= r < first[t+1] (first[lo] <= r < first[T] = n)
__device__ __forceinline__ int track_of(const int64_t *__restrict__ first, int lo, int T, int64_t r) {
    int hi = T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One stage (merge size k2, partner distance j) of an ascending bitonic sort by a workgroup of kThreads, over
// keys[0, cnt) whose slot 0 is slot g0 of the whole array; ends with a barrier.  kIdx: (key, idx) pairs ordered by key,
// then idx.  Int is int for arrays in LDS, int64_t for selfmatch's arrays in global memory.
template <int kThreads, bool kIdx, typename Int>
__device__ __forceinline__ void bitonic_stage(unsigned long long *keys, unsigned short *idx, Int cnt, Int g0, Int k2,
                                              Int j, int tid) {
    for (Int e = tid; e < cnt; e += kThreads) {
        const Int partner = e ^ j;
        if (partner > e) {
            const unsigned long long a = keys[e], b = keys[partner];
            const bool asc = ((g0 + e) & k2) == 0;
            bool gt = a > b;
            if (kIdx) gt = gt || (a == b && idx[e] > idx[partner]);
            if (gt == asc) {
                keys[e] = b;
                keys[partner] = a;
                if (kIdx) {
                    const unsigned short t = idx[e];
                    idx[e] = idx[partner];
                    idx[partner] = t;
                }
            }
        }
    }
    __syncthreads();
}

// ascending bitonic sort of P (a power of two) keys, or (key, idx) pairs, by the whole workgroup
template <int kThreads, bool kIdx, typename Int>
__device__ __forceinline__ void block_sort(unsigned long long *keys, unsigned short *idx, Int P, int tid) {
    for (Int k2 = 2; k2 <= P; k2 <<= 1)
        for (Int j = k2 >> 1; j > 0; j >>= 1) bitonic_stage<kThreads, kIdx, Int>(keys, idx, P, 0, k2, j, tid);
}

// The un-divided span score (the order stated at the top): x and y point at this lane's float4 of the first row pair,
// rows are SEQ_D floats apart.  Every lane of a half-wave passes the same m; m <= 0 still runs the butterfly.
// kUnroll row pairs are loaded ahead of the fmaf chain; the loop is bound by the latency of these scattered 512-byte
// row reads, so the count decides how many are in flight per wave (and the registers they take).  Every kernel uses
// the count its own loop had before the loops were merged here: 4 in seq_rerank_kernel, identify_kernel<true> and
// self_match_kernel, 1 in identify_kernel<false> (both rows of a pair come from global memory there).
// x_step: float4s between the x rows of two consecutive pairs (a query against a thinned library steps D rows).
template <int kUnroll>
__device__ __forceinline__ float span_sum(const float4 *x, const float4 *y, int m, int x_step = SEQ_D / 4) {
    float acc = 0.0f;
#pragma unroll kUnroll
    for (int t = 0; t < m; ++t) {
        const float4 q = x[(int64_t)t * x_step], r = y[(int64_t)t * (SEQ_D / 4)];
        acc = __builtin_fmaf(q.x, r.x, acc);
        acc = __builtin_fmaf(q.y, r.y, acc);
        acc = __builtin_fmaf(q.z, r.z, acc);
        acc = __builtin_fmaf(q.w, r.w, acc);
    }
#pragma unroll
    for (int s = 16; s > 0; s >>= 1) acc += __shfl_xor(acc, s);      // stays inside the 32-lane half
    return acc;
}

// The speed ratios of identify_tempo.hip and crossmatch_tempo.hip: an integer num in [SEQ_TEMPO_MIN, SEQ_TEMPO_MAX] stands
// for num / SEQ_TEMPO_DEN track seconds per recording second; a call names up to SEQ_MAX_RATIOS of them, ascending.
constexpr int SEQ_TEMPO_DEN = 256, SEQ_TEMPO_MIN = 128, SEQ_TEMPO_MAX = 512;
constexpr int SEQ_MAX_RATIOS = 64;
struct TempoRatios {
    int32_t num[SEQ_MAX_RATIOS];                           // travels in the kernel arguments
};

// host: checks a call's ratios and copies them into the table (name: the operation, for the message)
inline int tempo_ratios(const char *name, const int32_t *ratio_num, int n_ratios, TempoRatios &ratios) {
    GRAFP_REQUIRE(n_ratios >= 1 && n_ratios <= SEQ_MAX_RATIOS, "%s: n_ratios=%d not in [1, %d]", name, n_ratios,
                  SEQ_MAX_RATIOS);
    ratios = {};
    for (int j = 0; j < n_ratios; ++j) {
        GRAFP_REQUIRE(ratio_num[j] >= SEQ_TEMPO_MIN && ratio_num[j] <= SEQ_TEMPO_MAX, "%s: ratio_num[%d]=%d not in [%d, %d]",
                      name, j, (int)ratio_num[j], SEQ_TEMPO_MIN, SEQ_TEMPO_MAX);
        GRAFP_REQUIRE(j == 0 || ratio_num[j] > ratio_num[j - 1], "%s: ratio_num must be strictly ascending (%d after %d)",
                      name, (int)ratio_num[j], j ? (int)ratio_num[j - 1] : 0);
        ratios.num[j] = ratio_num[j];
    }
    return GRAFP_OK;
}

// slots of one item's merge of R lists of `top` entries (identify_tempo.hip: one list per ratio; merge_lists.hip: one per
// shard): the power of two >= max(64, R * top), at most 4096 (host: R <= 64, top <= 64), 10 bytes of LDS each
__host__ __device__ inline int merge_slots(int R, int top) {
    int P = 64;
    while (P < R * top) P <<= 1;
    return P;
}

// host: reserves `lds` bytes of dynamic LDS for a kernel and launches it (name: for the messages)
template <typename... Params, typename... Args>
inline int seq_launch(const char *name, void (*kernel)(Params...), dim3 grid, int threads, size_t lds,
                      hipStream_t stream, Args... args) {
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("%s: cannot reserve %zu bytes of LDS", name, lds);
        return GRAFP_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, stream, args...);
    GRAFP_CHECK_LAUNCH(name);
    return GRAFP_OK;
}

}  // namespace grafp
