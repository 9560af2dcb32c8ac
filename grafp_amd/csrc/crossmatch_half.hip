// crossmatch_half.hip -- what recordings held outside a library share with it, the library held as bf16 rows
// (grafp_amd/library.py's match() on the half form, ops.cross_match_half), gfx950.
//
// The operation of crossmatch.hip on rows that exist only as bf16: library row r is U[r] = the f32 value of its bf16 row
// (exact), and all six outputs are bit for bit what cross_match_kernel writes when it is handed the (n, 128) f32 array U.
// The phases, the LDS piece, the workspace layout and its sizes are match_source, plan_sources and sm_units of
// selfmatch_core.h, so grafp_self_match_workspace sizes these launches too; only the span rows differ (Bf16RowSpan of
// span_rows.h).  It sits beside cross_match_kernel the way cross_match_pq_kernel does, in a translation unit of its own.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as crossmatch.hip.
#include "selfmatch_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop: cross_match_kernel's count (the same two global streams)
constexpr int XMH_UNROLL = 4;

__global__ __launch_bounds__(SM_PLAN_THREADS) void cross_match_half_plan_kernel(const int64_t *__restrict__ src_first,
                                                                                int n_src, int k, int min_votes,
                                                                                int64_t *__restrict__ off) {
    plan_sources(TableSource{nullptr, src_first}, n_src, k, min_votes, off);
}

__global__ __launch_bounds__(SM_THREADS) void cross_match_half_kernel(
    const unsigned short *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T,
    const float *__restrict__ q_rows, const int64_t *__restrict__ src_first, const int64_t *__restrict__ ids, int k,
    int top, int min_votes, int min_overlap, unsigned long long *__restrict__ ws, int64_t head_units, int64_t cap_units,
    int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta, int32_t *__restrict__ out_start,
    int32_t *__restrict__ out_len, float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    const TableSource source{q_rows, src_first};
    const Bf16RowSpan<XMH_UNROLL> span{reinterpret_cast<const uint2 *>(rows)};
    match_source(MatchDenseGrid{}, source, span, n, first, T, ids, k, top, min_votes, min_overlap, ws, head_units, cap_units, out_track,
                 out_delta, out_start, out_len, out_score, out_votes);
}

int cross_match_half_launch(const unsigned short *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                            const int64_t *src_first, int n_src, const int64_t *ids, int k, int top, int min_votes,
                            int min_overlap, void *ws, size_t ws_bytes, int32_t *out_track, int32_t *out_delta,
                            int32_t *out_start, int32_t *out_len, float *out_score, int32_t *out_votes,
                            hipStream_t stream) {
    const int st = sm_check_launch("cross_match_half", k, top, min_votes, min_overlap, n_src, ws, ws_bytes);
    if (st != GRAFP_OK || n_src == 0) return st;
    hipLaunchKernelGGL(cross_match_half_plan_kernel, dim3(1), dim3(SM_PLAN_THREADS), 0, stream, src_first, n_src, k,
                       min_votes, reinterpret_cast<int64_t *>(ws));
    GRAFP_CHECK_LAUNCH("cross_match_half_plan_kernel");
    return sm_launch("cross_match_half_kernel", cross_match_half_kernel, dim3(n_src), stream, rows, n, first, T, q_rows,
                     src_first, ids, k, top, min_votes, min_overlap, reinterpret_cast<unsigned long long *>(ws),
                     sm_head_bytes(n_src) / 8, (int64_t)(ws_bytes / 8), out_track, out_delta, out_start, out_len,
                     out_score, out_votes);
}

}  // namespace grafp
