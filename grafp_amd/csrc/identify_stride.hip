// identify_stride.hip -- track-aware sequence identification of items that hold every Q-th segment of the recording
// (grafp_amd/library.py's query_stride, ops.identify_stride), gfx950.
//
// The query is embedded at a coarse hop and the library stays dense: item row s is the recording's segment s * Q, so it
// sits s * Q library rows after item row 0.  That is identify_tempo.hip's contract at the single ratio num = 256 * Q,
// where w(s) = (s * 256 Q + 128) >> 8 = s * Q exactly, restated for Q = query_stride in [1, 32].  For one item (ql kept
// rows with their top-k library ids):
//   * a hit (s, r), 0 <= r < n, names the track t holding r and the alignment a = r - s * Q (the library row on which
//     kept row 0 sits); a candidate is a unique (t, a), its votes the hits that map to it;
//   * the pairs of (t, a) are the s in [0, ql) with first[t] <= a + s * Q < first[t+1], o of them: a contiguous range;
//   * eligible iff o >= 1 and o >= min(need, max(1, L_t / Q)), need = min_overlap in pairs (<= 0: ql), L_t the rows of t:
//     the cap is the number of pairs a track of L_t rows can always hold at that stride;
//   * score = (sum over the pairs, s ascending, <q[s], row[a + s * Q]>) / o in span_sum's order (seqmatch.h): the query
//     pointer steps one row per pair, the library pointer Q.  No row outside track t is read;
//   * per track the best candidate (highest score, then the smaller a), the `top` tracks by score descending, then
//     track ascending; offset = a - first[t].
// The pairs of the true alignment are row pairs the dense call scores too, Q times fewer of them.  With Q = 1 every
// output equals identify.hip's bit for bit, with Q = 2 the first four outputs of identify_tempo.hip at the ratio 512.
// The five phases, the LDS layout and the limits are identify_core.h's identify_item (stated at the top of
// identify.hip) on StrideGrid: the key of a hit is (r - s * Q + 255 * Q) << 32 | s, so inside a run of one alignment r
// ascends with s and phase 2's walk carries over.  One workgroup per item, no workspace, no host synchronisation.  The
// host keeps n + 255 * Q below 2^32.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as identify.hip.
#include "identify_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop: query rows in LDS / in global memory (identify.hip's counts)
constexpr int IDS_UNROLL_QLDS = 4, IDS_UNROLL_QGLOBAL = 1;

template <bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_stride_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, int Q,
    const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k, const int64_t *__restrict__ item_row,
    const int *__restrict__ item_len, int max_len, int Pmax, int top, int min_overlap, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_offset, float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    const StepRowSpan<kQLds ? IDS_UNROLL_QLDS : IDS_UNROLL_QGLOBAL> span{reinterpret_cast<const float4 *>(rows), Q};
    identify_item<kQLds>(StrideGrid{Q}, span, n, first, T, q_rows, ids, k, item_row, item_len, max_len, Pmax, top,
                         min_overlap, out_track, out_offset, out_score, out_votes);
}

int identify_stride_launch(const float *rows, int64_t n, const int64_t *first, int T, int query_stride,
                           const float *q_rows, const int64_t *ids, int k, const int64_t *item_row,
                           const int *item_len, int n_items, int max_len, int top, int min_overlap, int32_t *out_track,
                           int32_t *out_offset, float *out_score, int32_t *out_votes, hipStream_t stream) {
    GRAFP_REQUIRE(query_stride >= 1 && query_stride <= ID_MAX_QUERY_STRIDE,
                  "identify_stride: query_stride=%d not in [1, %d]", query_stride, ID_MAX_QUERY_STRIDE);
    GRAFP_REQUIRE(n + (int64_t)(ID_MAX_LEN - 1) * query_stride < (1ll << 32),
                  "identify_stride: n=%lld rows at query_stride=%d reach past the 2^32 alignments of a key",
                  (long long)n, query_stride);
    const int st = id_check_launch("identify_stride", max_len, k);
    if (st != GRAFP_OK || n_items == 0) return st;
    const IdentifyPlan plan = identify_plan(max_len, k);
    return id_launch("identify_stride", identify_stride_kernel<true>, identify_stride_kernel<false>, plan,
                     dim3(n_items), stream, rows, n, first, T, query_stride, q_rows, ids, k, item_row, item_len,
                     max_len, plan.Pmax, top, min_overlap, out_track, out_offset, out_score, out_votes);
}

}  // namespace grafp
