// match_tempo.h -- what crossmatch_tempo.hip (recordings held outside the library, ops.cross_match_tempo) and
// selfmatch_tempo.hip (tracks of the library itself, ops.self_match_tempo) share: match_source along sloped alignments
// on a grid of (source, ratio), and the exact merge of the per-ratio lists.  The contract, the workspace layout (header,
// R copies of the per-source regions, six (R, n_src, top) list arrays) and why the merge is exact are stated at the top of
// crossmatch_tempo.hip; the two files differ in the Source of selfmatch_core.h alone and keep thin __global__ wrappers
// around the bodies below.
// Compiles with and without the packed-f32 instructions; every user is built without (Makefile NOPK).
#pragma once
#include "selfmatch_core.h"
#include "span_rows.h"

namespace grafp {

constexpr int XT_UNROLL = 4;                               // row pairs in flight in the score loop (cross_match_kernel's)
constexpr int XT_MERGE_THREADS = 256;

// slots of one source's merge: the power of two >= max(64, R * top), at most 4096 (host: R <= 64, top <= 64)
__host__ __device__ inline int xt_merge_slots(int R, int top) {
    int P = 64;
    while (P < R * top) P <<= 1;
    return P;
}

// Where the list arrays start (8-byte units from ws), or -1 when the regions and the lists end past the workspace.
__device__ __forceinline__ int64_t xt_lists_at(const unsigned long long *ws, int n_src, int R, int top,
                                               int64_t head_units, int64_t cap_units) {
    const int64_t total = reinterpret_cast<const int64_t *>(ws)[n_src];          // units of one copy of the regions
    const int64_t at = head_units + (int64_t)R * total;
    return at + 3 * (int64_t)R * n_src * top <= cap_units ? at : -1;
}

// Pass 1 of one (source, ratio): grid (n_src, R), SM_THREADS threads, SM_LDS bytes of dynamic LDS.  The five phases of
// match_source on MatchTempoGrid in ratio blockIdx.y's copy of the source's region; the `top` list goes to the list
// arrays in match_source's own output form.
template <typename Source>
__device__ __forceinline__ void xt_match_pass(const Source &source, const float *__restrict__ rows, int64_t n,
                                              const int64_t *__restrict__ first, int T, const TempoRatios &ratios, int R,
                                              const int64_t *__restrict__ ids, int k, int top, int min_votes,
                                              int min_overlap, unsigned long long *__restrict__ ws, int64_t head_units,
                                              int64_t cap_units) {
    const int n_src = gridDim.x, j = blockIdx.y;
    const int64_t lists_at = xt_lists_at(ws, n_src, R, top, head_units, cap_units);
    if (lists_at < 0) return;                                        // the merge writes padding
    const int64_t total = reinterpret_cast<const int64_t *>(ws)[n_src], lists = (int64_t)R * n_src * top;
    int32_t *lt = reinterpret_cast<int32_t *>(ws + lists_at) + (int64_t)j * n_src * top;   // this ratio's (n_src, top)
    int32_t *ws_track = lt, *ws_delta = lt + lists, *ws_start = lt + 2 * lists, *ws_len = lt + 3 * lists;
    float *ws_score = reinterpret_cast<float *>(lt + 4 * lists);
    int32_t *ws_votes = lt + 5 * lists;
    if (source.len(blockIdx.x) > SM_TEMPO_MAX_ROWS) {                // (refused by ops; i * num would leave an int32)
        if ((int)threadIdx.x < top)
            sm_pad((size_t)blockIdx.x * top + threadIdx.x, -1, ws_track, ws_delta, ws_start, ws_len, ws_score, ws_votes);
        return;
    }
    const TempoRowSpan<XT_UNROLL> span{reinterpret_cast<const float4 *>(rows)};
    match_source(MatchTempoGrid{ratios.num[j]}, source, span, n, first, T, ids, k, top, min_votes, min_overlap, ws,
                 head_units + (int64_t)j * total, cap_units, ws_track, ws_delta, ws_start, ws_len, ws_score, ws_votes);
}

// Pass 2 of one source: grid (n_src), XT_MERGE_THREADS threads, 10 * xt_merge_slots(R, top) bytes of dynamic LDS.
__device__ __forceinline__ void xt_merge(const TempoRatios &ratios, int R, int top,
                                         const unsigned long long *__restrict__ ws, int64_t head_units,
                                         int64_t cap_units, int32_t *__restrict__ out_track,
                                         int32_t *__restrict__ out_delta, int32_t *__restrict__ out_start,
                                         int32_t *__restrict__ out_len, float *__restrict__ out_score,
                                         int32_t *__restrict__ out_votes, int32_t *__restrict__ out_ratio) {
    extern __shared__ __attribute__((aligned(16))) unsigned char xt_smem[];       // 10 * P bytes (the launch's P)
    __shared__ int order[SEQ_MAX_RATIOS];                  // order[p]: the ratio of preference rank p
    const int src = blockIdx.x, n_src = gridDim.x, tid = threadIdx.x;
    const int total = R * top;
    const int P = xt_merge_slots(R, top);
    const int64_t lists_at = xt_lists_at(ws, n_src, R, top, head_units, cap_units);
    if (lists_at < 0) {                                   // a workspace below the plan's layout: nothing was matched
        if (tid < top) {
            const size_t o = (size_t)src * top + tid;
            sm_pad(o, -1, out_track, out_delta, out_start, out_len, out_score, out_votes);
            out_ratio[o] = 0;
        }
        return;
    }
    const int64_t lists = (int64_t)R * n_src * top;
    const int32_t *ws_track = reinterpret_cast<const int32_t *>(ws + lists_at);
    const float *ws_score = reinterpret_cast<const float *>(ws_track + 4 * lists);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(xt_smem);
    unsigned short *idx = reinterpret_cast<unsigned short *>(xt_smem + (size_t)8 * P);
    if (tid < R) {
        const int num = ratios.num[tid], d = num < SEQ_TEMPO_DEN ? SEQ_TEMPO_DEN - num : num - SEQ_TEMPO_DEN;
        int rank = 0;
        for (int j = 0; j < R; ++j) {
            const int nj = ratios.num[j], dj = nj < SEQ_TEMPO_DEN ? SEQ_TEMPO_DEN - nj : nj - SEQ_TEMPO_DEN;
            rank += (dj < d || (dj == d && nj < num)) ? 1 : 0;         // (the ratios are distinct)
        }
        order[rank] = tid;
    }
    __syncthreads();
    // the list entry of merge slot e < total
    auto entry = [&](int e) -> int64_t {
        const int p = e / top;
        return ((int64_t)order[p] * n_src + src) * top + (e - p * top);
    };
    for (int e = tid; e < P; e += XT_MERGE_THREADS) {
        unsigned long long key = SEQ_NONE;
        if (e < total) {
            const int64_t w = entry(e);
            const int b = ws_track[w];
            if (b >= 0) key = ((unsigned long long)b << 32) | ~f32_ord(ws_score[w]);
        }
        keys[e] = key;
        idx[e] = (unsigned short)e;
    }
    __syncthreads();
    // best entry per partner (P / 256 <= 16 slots per thread: one mask bit each)
    block_sort<XT_MERGE_THREADS, true>(keys, idx, P, tid);
    unsigned int head = 0;
    for (int e = tid, it = 0; e < P; e += XT_MERGE_THREADS, ++it) {
        const unsigned long long key = keys[e];
        if (key != SEQ_NONE && (e == 0 || (keys[e - 1] >> 32) != (key >> 32))) head |= 1u << it;
    }
    __syncthreads();
    for (int e = tid, it = 0; e < P; e += XT_MERGE_THREADS, ++it) {
        const unsigned long long key = keys[e];
        keys[e] = ((head >> it) & 1u) ? ((key << 32) | (key >> 32)) : SEQ_NONE;
    }
    __syncthreads();
    // the `top` partners: score descending, partner ascending
    block_sort<XT_MERGE_THREADS, true>(keys, idx, P, tid);
    if (tid < top) {
        const unsigned long long key = keys[tid];          // top <= 64 <= P
        const size_t o = (size_t)src * top + tid;
        if (key != SEQ_NONE) {
            const int e = idx[tid];
            const int64_t w = entry(e);
            out_track[o] = (int)(key & 0xffffffffull);
            out_delta[o] = ws_track[lists + w];
            out_start[o] = ws_track[2 * lists + w];
            out_len[o] = ws_track[3 * lists + w];
            out_score[o] = ord_f32(~(unsigned int)(key >> 32));
            out_votes[o] = ws_track[5 * lists + w];
            out_ratio[o] = ratios.num[order[e / top]];
        } else {
            sm_pad(o, -1, out_track, out_delta, out_start, out_len, out_score, out_votes);
            out_ratio[o] = 0;
        }
    }
}

// host: the launch-time checks both operations share (name: the operation, for the messages).  `longest` bounds a
// source's rows as far as the host knows them (longer ones than SM_TEMPO_MAX_ROWS are padding).  The host knows the header
// and the lists' size and refuses a smaller ws_bytes; whether the regions fit only the kernels can tell.
inline int xt_check_launch(const char *name, int64_t n, int64_t longest, int k, int top, int min_votes, int min_overlap,
                           int n_src, const int32_t *ratio_num, int n_ratios, const void *ws, size_t ws_bytes,
                           TempoRatios &ratios) {
    int st = tempo_ratios(name, ratio_num, n_ratios, ratios);
    if (st != GRAFP_OK) return st;
    st = sm_check_launch(name, k, top, min_votes, min_overlap, n_src, ws, ws_bytes);
    if (st != GRAFP_OK) return st;
    GRAFP_REQUIRE(n_ratios * top <= 4096, "%s: %d ratios x top=%d exceed the 4096 slots of the merge", name, n_ratios,
                  top);
    if (longest > SM_TEMPO_MAX_ROWS) longest = SM_TEMPO_MAX_ROWS;
    GRAFP_REQUIRE(n + 2 * longest < (1ll << 32),
                  "%s: n=%lld rows and sources of up to %lld reach past the 2^32 alignments of a key", name,
                  (long long)n, (long long)longest);
    const size_t head = (size_t)sm_head_bytes(n_src), lists = (size_t)24 * n_src * n_ratios * top;
    if (ws_bytes < head + lists) {
        set_error("%s: workspace of %zu bytes, at least %zu needed for the header and the lists alone", name, ws_bytes,
                  head + lists);
        return GRAFP_ERR_WORKSPACE;
    }
    return GRAFP_OK;
}

// host: pass 1 and pass 2 after the caller's plan kernel, on its stream
template <typename... Params, typename... MParams, typename... Args>
inline int xt_launch_passes(const char *name, void (*pass)(Params...), void (*merge)(MParams...), int n_src,
                            const TempoRatios &ratios, int n_ratios, int top, void *ws, size_t ws_bytes,
                            int32_t *out_track, int32_t *out_delta, int32_t *out_start, int32_t *out_len,
                            float *out_score, int32_t *out_votes, int32_t *out_ratio, hipStream_t stream,
                            Args... pass_args) {
    unsigned long long *ws8 = reinterpret_cast<unsigned long long *>(ws);
    const int64_t head_units = sm_head_bytes(n_src) / 8, cap_units = (int64_t)(ws_bytes / 8);
    const int st = sm_launch(name, pass, dim3(n_src, n_ratios), stream, pass_args..., ws8, head_units, cap_units);
    if (st != GRAFP_OK) return st;
    hipLaunchKernelGGL(merge, dim3(n_src), dim3(XT_MERGE_THREADS), (size_t)10 * xt_merge_slots(n_ratios, top), stream,
                       ratios, n_ratios, top, ws8, head_units, cap_units, out_track, out_delta, out_start, out_len,
                       out_score, out_votes, out_ratio);
    GRAFP_CHECK_LAUNCH(name);
    return GRAFP_OK;
}

}  // namespace grafp
