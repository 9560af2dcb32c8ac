// crossmatch_tempo.hip -- what recordings held OUTSIDE a track-indexed fingerprint library share with it when they play
// faster or slower than the catalogue (grafp_amd/library.py's match(tempo=...), ops.cross_match_tempo), gfx950.
//
// crossmatch.hip's operation along sloped alignments.  A ratio is an integer num in [128, 512] that stands for num / 256
// track seconds per recording second; at ratio num source row i (counted from the source's row 0; a source may have up
// to 4 194 303 rows) sits w(i) = (i * num + 128) >> 8 library rows after source row 0: integer arithmetic, the same on
// host and device.  For one source of L rows and every ratio j of the call's R <= 64 ascending ratios:
//   * row i with a hit r in [0, n) names the track b holding r and the alignment a = r - w_j(i) (the library row on which
//     source row 0 would sit); a candidate is a unique (b, a, j), its votes the hits that map to it (duplicates vote
//     twice, nothing is dropped); an alignment run that crosses a track boundary continues as a candidate of the next
//     track (inside one run r = a + w_j(i) never decreases with i);
//   * its span is [i_lo, i_hi], the smallest and largest voting i, m = i_hi - i_lo + 1; it is eligible iff votes >=
//     min_votes and m >= min_overlap, and then scores (sum_{i = i_lo .. i_hi} <q[i], row[a + w_j(i)]>) / m in span_sum's
//     order (seqmatch.h), the library rows gathered (below 256 a row may be read twice, above it rows are skipped).  All
//     those rows lie inside track b, because w_j never decreases and the two end rows do;
//   * per partner b the best eligible candidate over all ratios: highest score, then the ratio nearer to 1 (smaller
//     |num - 256|, then smaller num), then the smaller a; the `top` partners by score descending, then b ascending.
//     delta = a - first[b], and a seventh output names the ratio (num; padding 0).
// With the one ratio 256 the first six outputs are cross_match_kernel's bit for bit.
//
// Plan, cross_match_tempo_plan_kernel: plan_sources of selfmatch_core.h fills the header once; ratio j's copy of the
// per-source regions starts j * off[n_src] units after ratio 0's, and the six (R, n_src, top) list arrays of 4 bytes
// follow the R copies: head + R * (grafp_self_match_workspace - head) + 24 * n_src * R * top bytes in all.
// Pass 1, cross_match_tempo_kernel, grid (n_src, R): one workgroup runs the five phases of match_source for one
// (source, ratio) on MatchTempoGrid -- the key of a hit is (r - w(i) + 2 L) << 32 | i, w(L - 1) <= 2 L - 2 -- in that
// ratio's copy of the source's region; the span of phase 3 gathers its rows (TempoRowSpan of span_rows.h).  Its `top`
// list goes to the list arrays in match_source's own output form.
// Pass 2, cross_match_tempo_merge_kernel, one workgroup per source: the R * top <= 4096 entries are merged in LDS (10
// bytes per slot, the power of two >= max(64, R * top) slots) exactly as identify_tempo_merge_kernel merges its lists
// (identify_tempo.hip states why that is exact with lists of length top): slots in ratio-preference order, a sort of
// (b << 32 | ~ord(score), slot) puts every partner's best entry first, the heads become ~ord(score) << 32 | b and a second
// sort ranks the partners.  One ratio's list holds a partner once, with the smaller a already taken by its pass 1.
// The host knows the header and the lists' size and refuses a smaller ws_bytes; whether the regions fit it cannot know
// (the source table is device memory), so both passes compare what the plan laid out with ws_bytes: a workspace below
// grafp_cross_match_tempo_workspace writes nothing outside ws and every output is padding.  No -2 mark.
// All three kernels go out on the caller's stream with no host synchronisation; no atomics on floats.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as crossmatch.hip.
#include "selfmatch_core.h"
#include "span_rows.h"

namespace grafp {

constexpr int XT_UNROLL = 4;                               // row pairs in flight in the score loop (cross_match_kernel's)
constexpr int XT_MERGE_THREADS = 256;

size_t self_match_workspace(const int64_t *src_rows, int n_src, int k, int min_votes);      // selfmatch.hip

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

__global__ __launch_bounds__(SM_PLAN_THREADS) void cross_match_tempo_plan_kernel(const int64_t *__restrict__ src_first,
                                                                                 int n_src, int k, int min_votes,
                                                                                 int64_t *__restrict__ off) {
    plan_sources(TableSource{nullptr, src_first}, n_src, k, min_votes, off);
}

__global__ __launch_bounds__(SM_THREADS) void cross_match_tempo_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, TempoRatios ratios, int R,
    const float *__restrict__ q_rows, const int64_t *__restrict__ src_first, const int64_t *__restrict__ ids, int k,
    int top, int min_votes, int min_overlap, unsigned long long *__restrict__ ws, int64_t head_units,
    int64_t cap_units) {
    const int n_src = gridDim.x, j = blockIdx.y;
    const int64_t lists_at = xt_lists_at(ws, n_src, R, top, head_units, cap_units);
    if (lists_at < 0) return;                                        // the merge writes padding
    const int64_t total = reinterpret_cast<const int64_t *>(ws)[n_src], lists = (int64_t)R * n_src * top;
    int32_t *lt = reinterpret_cast<int32_t *>(ws + lists_at) + (int64_t)j * n_src * top;   // this ratio's (n_src, top)
    int32_t *ws_track = lt, *ws_delta = lt + lists, *ws_start = lt + 2 * lists, *ws_len = lt + 3 * lists;
    float *ws_score = reinterpret_cast<float *>(lt + 4 * lists);
    int32_t *ws_votes = lt + 5 * lists;
    const TableSource source{q_rows, src_first};
    if (source.len(blockIdx.x) > SM_TEMPO_MAX_ROWS) {                // (refused by ops; i * num would leave an int32)
        if ((int)threadIdx.x < top)
            sm_pad((size_t)blockIdx.x * top + threadIdx.x, -1, ws_track, ws_delta, ws_start, ws_len, ws_score, ws_votes);
        return;
    }
    const TempoRowSpan<XT_UNROLL> span{reinterpret_cast<const float4 *>(rows)};
    match_source(MatchTempoGrid{ratios.num[j]}, source, span, n, first, T, ids, k, top, min_votes, min_overlap, ws,
                 head_units + (int64_t)j * total, cap_units, ws_track, ws_delta, ws_start, ws_len, ws_score, ws_votes);
}

__global__ __launch_bounds__(XT_MERGE_THREADS) void cross_match_tempo_merge_kernel(
    TempoRatios ratios, int R, int top, const unsigned long long *__restrict__ ws, int64_t head_units,
    int64_t cap_units, int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta,
    int32_t *__restrict__ out_start, int32_t *__restrict__ out_len, float *__restrict__ out_score,
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

size_t cross_match_tempo_workspace(const int64_t *src_rows, int n_src, int k, int min_votes, int n_ratios, int top) {
    if (n_ratios < 1 || n_ratios > SEQ_MAX_RATIOS || top < 1 || top > SM_MAX_TOP) return 0;
    const size_t dense = self_match_workspace(src_rows, n_src, k, min_votes);
    if (dense == 0) return 0;
    const size_t head = (size_t)sm_head_bytes(n_src);
    return head + (size_t)n_ratios * (dense - head) + (size_t)24 * n_src * n_ratios * top;
}

int cross_match_tempo_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                             int64_t n_qrows, const int64_t *src_first, int n_src, const int64_t *ids, int k, int top,
                             int min_votes, int min_overlap, const int32_t *ratio_num, int n_ratios, void *ws,
                             size_t ws_bytes, int32_t *out_track, int32_t *out_delta, int32_t *out_start,
                             int32_t *out_len, float *out_score, int32_t *out_votes, int32_t *out_ratio,
                             hipStream_t stream) {
    TempoRatios ratios;
    int st = tempo_ratios("cross_match_tempo", ratio_num, n_ratios, ratios);
    if (st != GRAFP_OK) return st;
    st = sm_check_launch("cross_match_tempo", k, top, min_votes, min_overlap, n_src, ws, ws_bytes);
    if (st != GRAFP_OK) return st;
    GRAFP_REQUIRE(n_ratios * top <= 4096, "cross_match_tempo: %d ratios x top=%d exceed the 4096 slots of the merge",
                  n_ratios, top);
    // the longest source has at most min(n_qrows, SM_TEMPO_MAX_ROWS) rows (longer ones are padding)
    const int64_t longest = n_qrows < SM_TEMPO_MAX_ROWS ? n_qrows : SM_TEMPO_MAX_ROWS;
    GRAFP_REQUIRE(n + 2 * longest < (1ll << 32),
                  "cross_match_tempo: n=%lld rows and sources of up to %lld reach past the 2^32 alignments of a key",
                  (long long)n, (long long)longest);
    const size_t head = (size_t)sm_head_bytes(n_src), lists = (size_t)24 * n_src * n_ratios * top;
    if (ws_bytes < head + lists) {
        set_error("cross_match_tempo: workspace of %zu bytes, at least %zu needed for the header and the lists alone",
                  ws_bytes, head + lists);
        return GRAFP_ERR_WORKSPACE;
    }
    if (n_src == 0) return GRAFP_OK;
    unsigned long long *ws8 = reinterpret_cast<unsigned long long *>(ws);
    const int64_t head_units = (int64_t)(head / 8), cap_units = (int64_t)(ws_bytes / 8);
    hipLaunchKernelGGL(cross_match_tempo_plan_kernel, dim3(1), dim3(SM_PLAN_THREADS), 0, stream, src_first, n_src, k,
                       min_votes, reinterpret_cast<int64_t *>(ws));
    GRAFP_CHECK_LAUNCH("cross_match_tempo_plan_kernel");
    st = sm_launch("cross_match_tempo", cross_match_tempo_kernel, dim3(n_src, n_ratios), stream, rows, n, first, T, ratios,
                   n_ratios, q_rows, src_first, ids, k, top, min_votes, min_overlap, ws8, head_units, cap_units);
    if (st != GRAFP_OK) return st;
    hipLaunchKernelGGL(cross_match_tempo_merge_kernel, dim3(n_src), dim3(XT_MERGE_THREADS),
                       (size_t)10 * xt_merge_slots(n_ratios, top), stream, ratios, n_ratios, top, ws8, head_units,
                       cap_units, out_track, out_delta, out_start, out_len, out_score, out_votes, out_ratio);
    GRAFP_CHECK_LAUNCH("cross_match_tempo_merge_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
