// identify_tempo.hip -- track-aware sequence identification of recordings that play faster or slower than the
// catalogue (grafp_amd/library.py's tempo=, ops.identify_tempo), gfx950.
//
// A ratio is an integer num in [128, 512] that stands for num / 256 track seconds per recording second (> 256: the
// recording plays the track fast).  At ratio num query row s sits w(s) = (s * num + 128) >> 8 library rows after query
// row 0: integer arithmetic, the same on host and device, w(s) <= 510 for s <= 255.  Two ratios 1/256 apart differ by at
// most one row over the 256 rows an item may have, which is why the denominator is 256.
// For one item (ql query rows with their top-k library ids) and every ratio j of the call's R <= 64 ascending ratios:
//   * a hit (s, r), 0 <= r < n, names the track t holding r and the alignment a = r - w_j(s) (the row where query row 0
//     sits); a candidate is a unique (t, a, j), its votes the hits that map to it;
//   * the pairs of (t, a, j) are the s in [0, ql) with first[t] <= a + w_j(s) < first[t+1], o of them: a contiguous range
//     of s because w_j never decreases.  Below 256 two consecutive s may share a library row, above it rows are skipped;
//   * eligible iff o >= 1 and o >= min(need, max(1, (L_t * 256) / num)), need = min_overlap (<= 0: ql), L_t the rows of t:
//     the cap is the number of pairs a track of L_t rows can always hold at that ratio (at 256: identify.hip's rule);
//   * score = (sum over the pairs, s ascending, <q[s], row[a + w_j(s)]>) / o in span_sum's order (seqmatch.h).  No row
//     outside track t is read;
//   * per track the best candidate: highest score, then the ratio nearer to 1 (smaller |num - 256|, then smaller num),
//     then the smaller a; the `top` tracks by score descending, then track ascending.  offset = a - first[t], and a
//     fifth output names the ratio (num; padding 0).
// With the one ratio 256 the first four outputs are identify.hip's bit for bit.
//
// Pass 1, identify_tempo_kernel, grid (n_items, R): one workgroup runs the five phases of identify_core.h's
// identify_item (stated at the top of identify.hip, with its LDS plan and limits) for one (item, ratio) on TempoGrid --
// the key of a hit is (r - w(s) + 511) << 32 | s, so inside a run of one alignment r never decreases with s and phase 2's
// walk carries over; the span of phase 3 gathers its library rows (TempoRowSpan of span_rows.h).  Its `top` list goes to
// the workspace instead of the outputs: four (R, n_items, top) arrays of 4 bytes, track / offset / score / votes in
// identify_item's own output form, 16 bytes per entry in all.  The host keeps n + 511 below 2^32.
// Pass 2, identify_tempo_merge_kernel, one workgroup per item: the R * top <= 4096 entries are merged in LDS (10 bytes
// per slot, the power of two >= max(64, R * top) slots).  The merge
// is exact with lists of length top: a track ahead of t in ratio j's list has a final score at least its score there,
// so it is ahead of t in the final order too, and every final winner is inside its own ratio's list.  The entries are
// laid out in ratio-preference order (slot = rank(j) * top + i); sorting (t << 32 | ~ord(score), slot) puts the best
// entry of every track first with the ratio tie rule given by the slot (one ratio's list holds a track once, and its
// pass 1 already took the smaller a); the heads become ~ord(score) << 32 | t and a second sort ranks the tracks.
// Both passes go out on the caller's stream with no host synchronisation.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as identify.hip.
#include "identify_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop: query rows in LDS / in global memory (identify.hip's counts)
constexpr int IDR_UNROLL_QLDS = 4, IDR_UNROLL_QGLOBAL = 1;

template <bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_tempo_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, TempoRatios ratios,
    const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k, const int64_t *__restrict__ item_row,
    const int *__restrict__ item_len, int max_len, int Pmax, int top, int min_overlap, int32_t *__restrict__ ws_track,
    int32_t *__restrict__ ws_offset, float *__restrict__ ws_score, int32_t *__restrict__ ws_votes) {
    const TempoRowSpan<kQLds ? IDR_UNROLL_QLDS : IDR_UNROLL_QGLOBAL> span{reinterpret_cast<const float4 *>(rows)};
    const size_t list = (size_t)blockIdx.y * gridDim.x * top;          // this ratio's (n_items, top) lists
    identify_item<kQLds>(TempoGrid{ratios.num[blockIdx.y]}, span, n, first, T, q_rows, ids, k, item_row, item_len,
                         max_len, Pmax, top, min_overlap, ws_track + list, ws_offset + list, ws_score + list,
                         ws_votes + list);
}

__global__ __launch_bounds__(ID_THREADS) void identify_tempo_merge_kernel(
    TempoRatios ratios, int R, int top, const int32_t *__restrict__ ws_track, const int32_t *__restrict__ ws_offset,
    const float *__restrict__ ws_score, const int32_t *__restrict__ ws_votes, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_offset, float *__restrict__ out_score, int32_t *__restrict__ out_votes,
    int32_t *__restrict__ out_ratio) {
    extern __shared__ __attribute__((aligned(16))) unsigned char idr_smem[];      // 10 * P bytes (the launch's P)
    __shared__ int order[SEQ_MAX_RATIOS];                 // order[p]: the ratio of preference rank p
    const int item = blockIdx.x, n_items = gridDim.x, tid = threadIdx.x;
    const int total = R * top;
    const int P = merge_slots(R, top);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(idr_smem);
    unsigned short *idx = reinterpret_cast<unsigned short *>(idr_smem + (size_t)8 * P);
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
    // the ws entry of merge slot e < total
    auto entry = [&](int e) -> size_t {
        const int p = e / top;
        return ((size_t)order[p] * n_items + item) * top + (e - p * top);
    };
    for (int e = tid; e < P; e += ID_THREADS) {
        unsigned long long key = SEQ_NONE;
        if (e < total) {
            const size_t w = entry(e);
            const int t = ws_track[w];
            if (t >= 0) key = ((unsigned long long)t << 32) | ~f32_ord(ws_score[w]);
        }
        keys[e] = key;
        idx[e] = (unsigned short)e;
    }
    __syncthreads();
    // best entry per track (P / 256 <= 16 slots per thread: one mask bit each)
    block_sort<ID_THREADS, true>(keys, idx, P, tid);
    unsigned int head = 0;
    for (int e = tid, it = 0; e < P; e += ID_THREADS, ++it) {
        const unsigned long long key = keys[e];
        if (key != SEQ_NONE && (e == 0 || (keys[e - 1] >> 32) != (key >> 32))) head |= 1u << it;
    }
    __syncthreads();
    for (int e = tid, it = 0; e < P; e += ID_THREADS, ++it) {
        const unsigned long long key = keys[e];
        keys[e] = ((head >> it) & 1u) ? ((key << 32) | (key >> 32)) : SEQ_NONE;
    }
    __syncthreads();
    // the `top` tracks: score descending, track ascending
    block_sort<ID_THREADS, true>(keys, idx, P, tid);
    if (tid < top) {
        const unsigned long long key = keys[tid];          // top <= 64 <= P
        const size_t o = (size_t)item * top + tid;
        if (key != SEQ_NONE) {
            const int e = idx[tid];
            const size_t w = entry(e);
            out_track[o] = (int)(key & 0xffffffffull);
            out_offset[o] = ws_offset[w];
            out_score[o] = ord_f32(~(unsigned int)(key >> 32));
            out_votes[o] = ws_votes[w];
            out_ratio[o] = ratios.num[order[e / top]];
        } else {
            out_track[o] = -1;
            out_offset[o] = INT_MIN;
            out_score[o] = -INFINITY;
            out_votes[o] = 0;
            out_ratio[o] = 0;
        }
    }
}

size_t identify_tempo_workspace(int n_items, int n_ratios, int top) {
    if (n_items < 0 || n_ratios < 1 || n_ratios > SEQ_MAX_RATIOS || top < 1 || top > 64) return 0;
    return (size_t)16 * n_items * n_ratios * top;
}

int identify_tempo_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                          const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                          int max_len, int top, int min_overlap, const int32_t *ratio_num, int n_ratios, void *ws,
                          int32_t *out_track, int32_t *out_offset, float *out_score, int32_t *out_votes,
                          int32_t *out_ratio, hipStream_t stream) {
    TempoRatios ratios;
    int st = tempo_ratios("identify_tempo", ratio_num, n_ratios, ratios);
    if (st != GRAFP_OK) return st;
    GRAFP_REQUIRE(n + ID_TEMPO_SHIFT < (1ll << 32),
                  "identify_tempo: n=%lld rows reach past the 2^32 alignments of a key", (long long)n);
    st = id_check_launch("identify_tempo", max_len, k);
    if (st != GRAFP_OK || n_items == 0) return st;
    GRAFP_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, "identify_tempo: the workspace is missing or not 16-byte aligned");
    const size_t lists = (size_t)n_ratios * n_items * top;
    int32_t *ws_track = reinterpret_cast<int32_t *>(ws), *ws_offset = ws_track + lists;
    float *ws_score = reinterpret_cast<float *>(ws_offset + lists);
    int32_t *ws_votes = reinterpret_cast<int32_t *>(ws_score + lists);
    const IdentifyPlan plan = identify_plan(max_len, k);
    st = id_launch("identify_tempo", identify_tempo_kernel<true>, identify_tempo_kernel<false>, plan,
                   dim3(n_items, n_ratios), stream, rows, n, first, T, ratios, q_rows, ids, k, item_row, item_len,
                   max_len, plan.Pmax, top, min_overlap, ws_track, ws_offset, ws_score, ws_votes);
    if (st != GRAFP_OK) return st;
    hipLaunchKernelGGL(identify_tempo_merge_kernel, dim3(n_items), dim3(ID_THREADS), (size_t)10 * merge_slots(n_ratios, top),
                       stream, ratios, n_ratios, top,
                       ws_track, ws_offset, ws_score, ws_votes, out_track, out_offset, out_score, out_votes, out_ratio);
    GRAFP_CHECK_LAUNCH("identify_tempo_merge_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
