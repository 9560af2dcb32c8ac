// identify_half.hip -- track-aware sequence identification against a library held as bf16 rows (grafp_amd/library.py's
// half form, ops.identify_half), gfx950.
//
// The same operation as identify.hip, on rows that exist only as bf16.  Library row r is U[r] = the f32 value of its
// bf16 row (exact: a bf16 is the upper half of its f32), and every output is bit for bit what identify_kernel writes when
// it is handed the (n, 128) f32 array U.  Candidates, eligibility, the per-track best, the ranking, the ties, the LDS
// layout and phases 1, 2, 4 and 5 are identify_core.h's identify_item, shared with identify.hip; only the span rows of
// phase 3 differ (Bf16RowSpan of span_rows.h: 256 bytes per row instead of 512, one access per half-wave).
// Against a flat library over the f32 rows X that U was rounded from (round to nearest even) a score moves by at most
// 2^-8 max||q|| max||x||: each component moves by at most 2^-8 relative, Cauchy-Schwarz bounds a product's change, and a
// score is a mean of such products.
// One workgroup per item, no workspace; both query-row plans of identify_plan through id_launch.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as identify.hip.
#include "identify_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop: query rows in LDS / in global memory (identify.hip's counts: the same two streams,
// the library's at half the bytes)
constexpr int IDH_UNROLL_QLDS = 4, IDH_UNROLL_QGLOBAL = 1;

template <bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_half_kernel(
    const unsigned short *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T,
    const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k, const int64_t *__restrict__ item_row,
    const int *__restrict__ item_len, int max_len, int Pmax, int top, int min_overlap, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_offset, float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    const Bf16RowSpan<kQLds ? IDH_UNROLL_QLDS : IDH_UNROLL_QGLOBAL> span{reinterpret_cast<const uint2 *>(rows)};
    identify_item<kQLds>(DenseGrid{}, span, n, first, T, q_rows, ids, k, item_row, item_len, max_len, Pmax, top, min_overlap,
                         out_track, out_offset, out_score, out_votes);
}

int identify_half_launch(const unsigned short *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                         const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                         int max_len, int top, int min_overlap, int32_t *out_track, int32_t *out_offset,
                         float *out_score, int32_t *out_votes, hipStream_t stream) {
    const int st = id_check_launch("identify_half", max_len, k);
    if (st != GRAFP_OK || n_items == 0) return st;
    const IdentifyPlan plan = identify_plan(max_len, k);
    return id_launch("identify_half", identify_half_kernel<true>, identify_half_kernel<false>, plan, dim3(n_items), stream,
                     rows, n, first, T, q_rows, ids, k, item_row, item_len, max_len, plan.Pmax, top, min_overlap,
                     out_track, out_offset, out_score, out_votes);
}

}  // namespace grafp
