// identify_thin.hip -- track-aware sequence identification against a library that keeps every D-th fingerprint row of
// each track (grafp_amd/library.py's row_stride, ops.identify_thin), gfx950.
//
// The catalogue is stored at a coarse hop and the query stays dense: library row j of track t is that track's dense
// segment j * D, a track of S dense segments has ceil(S / D) rows, and first[] counts kept rows.  The fine position of
// library row r is r * D.  For one item (ql dense query rows with their top-k ids of kept rows):
//   * a hit (s, r) names the track t holding r and the fine alignment a = r * D - s (where query row 0 would sit); a
//     candidate is a unique (t, a), its votes the hits that map to it;
//   * the pairs of (t, a) are the s in [0, ql) with (a + s) mod D == 0 and first[t] <= (a + s) / D < first[t+1]:
//     s0, s0 + D, ..., o of them.  The candidate is eligible iff o >= 1 and o >= min(max(1, need_q / D), L_t) with
//     need_q = min_overlap (<= 0: the item's ql), and
//     score = (sum over the pairs, s ascending, <q[s], row[(a + s) / D]>) / o
//     in span_sum's order (seqmatch.h): the query pointer steps D rows per pair, the library pointer one.  No row
//     outside track t is read;
//   * per track the best candidate (highest score, then the smaller a), the `top` tracks by score descending, then
//     track ascending; offset = a - first[t] * D, in dense segments from the track's start.
// Whatever the true alignment is, every D-th query row lands exactly on a kept row, so the alignment is still resolved
// to one fine hop and the pairs of the true alignment are row pairs the dense library would score too.  With D = 1
// every output equals identify.hip's bit for bit.
// The five phases, the LDS layout and the limits are identify_core.h's identify_item (stated at the top of
// identify.hip) on ThinGrid: the key of a hit is (r * D - s + 255) << 32 | s, so inside a run of one alignment r ascends
// with s and phase 2's walk carries over.  The host keeps n * D + 255 below 2^32.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as identify.hip.
#include "identify_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop: query rows in LDS / in global memory (identify.hip's counts)
constexpr int IDT_UNROLL_QLDS = 4, IDT_UNROLL_QGLOBAL = 1;

template <bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_thin_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, int D,
    const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k, const int64_t *__restrict__ item_row,
    const int *__restrict__ item_len, int max_len, int Pmax, int top, int min_overlap, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_offset, float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    const StridedRowSpan<kQLds ? IDT_UNROLL_QLDS : IDT_UNROLL_QGLOBAL> span{reinterpret_cast<const float4 *>(rows),
                                                                           D * (SEQ_D / 4)};
    identify_item<kQLds>(ThinGrid{D}, span, n, first, T, q_rows, ids, k, item_row, item_len, max_len, Pmax, top,
                         min_overlap, out_track, out_offset, out_score, out_votes);
}

int identify_thin_launch(const float *rows, int64_t n, const int64_t *first, int T, int row_stride,
                         const float *q_rows, const int64_t *ids, int k, const int64_t *item_row, const int *item_len,
                         int n_items, int max_len, int top, int min_overlap, int32_t *out_track, int32_t *out_offset,
                         float *out_score, int32_t *out_votes, hipStream_t stream) {
    GRAFP_REQUIRE(row_stride >= 1 && row_stride <= ID_MAX_STRIDE, "identify_thin: row_stride=%d not in [1, %d]",
                  row_stride, ID_MAX_STRIDE);
    GRAFP_REQUIRE(n * row_stride + ID_SHIFT < (1ll << 32),
                  "identify_thin: n=%lld rows at row_stride=%d reach past the 2^32 fine positions of a key",
                  (long long)n, row_stride);
    const int st = id_check_launch("identify_thin", max_len, k);
    if (st != GRAFP_OK || n_items == 0) return st;
    const IdentifyPlan plan = identify_plan(max_len, k);
    return id_launch("identify_thin", identify_thin_kernel<true>, identify_thin_kernel<false>, plan, dim3(n_items),
                     stream, rows, n, first, T, row_stride, q_rows, ids, k, item_row, item_len, max_len, plan.Pmax, top,
                     min_overlap, out_track, out_offset, out_score, out_votes);
}

}  // namespace grafp
