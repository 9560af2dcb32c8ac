// crossmatch.hip -- what recordings held OUTSIDE a track-indexed fingerprint library share with it
// (grafp_amd/library.py's match(), ops.cross_match and ops.cross_match_pq), gfx950.
//
// The operation of selfmatch.hip with the sources taken from outside: the library is n rows of T tracks laid end to end
// (track t owns rows [first[t], first[t+1])), held as resident (n, 128) f32 rows or as IVF-PQ codes; q_rows (n_q, 128)
// f32 holds S sources laid end to end (source s owns rows [src_first[s], src_first[s+1])), and ids (n_q, k) the top-k
// library hits of every source row.  For one source of L rows:
//   * row i (i < L) with hit r in [0, n) names the track b holding r and j = r - first[b]; it votes for the candidate
//     (b, delta = j - i).  NOTHING is dropped (no library row is the source's own); duplicate ids vote twice; an
//     alignment run that crosses a track boundary continues as a candidate of the next track;
//   * a candidate's span is [i_lo, i_hi], the smallest and largest voting i, m = i_hi - i_lo + 1 rows; it is eligible
//     iff votes >= min_votes and m >= min_overlap, and then scores
//     (sum_{i = i_lo .. i_hi} <q_rows[src_first[s] + i], lib[first[b] + i + delta]>) / m
//     (span_sum's order, IEEE division; all those library rows lie inside track b, because the two end rows do);
//   * per partner b the eligible candidate with the highest score is kept (ties: the smaller delta), and the `top`
//     partners are written by score descending, then b ascending.
// One workgroup of 512 threads per source; the phases, the LDS piece, the workspace layout and its sizes are
// match_source, plan_sources and sm_units of selfmatch_core.h, shared with selfmatch.hip, so grafp_self_match_workspace
// sizes these launches too and a source whose region ends past ws_bytes gets -2 in its first out_track slot.  A source
// equal to library track a, with its hits inside a blanked, gets the bits self_match_kernel writes for a.
// Five kernels: cross_match_kernel scores against the f32 rows (RowSpan), cross_match_pq_kernel<M>, M = 16, 32, 64, 128,
// against rows decoded from the codes while they are scored (PqSpan of span_rows.h: centroids[list_id[r]][j] + codeword,
// one f32 add per element, list ids clamped), bit for bit what cross_match_kernel writes on the decoded rows.
// Built WITHOUT packed-f32 instructions (Makefile NOPK, as selfmatch.hip).
#include "selfmatch_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop: the source rows come from global memory (L2-resident: every candidate of the
// source reads them), as the library rows do.  f32: self_match_kernel's count, the same two global streams.  PQ: rows
// decoded ahead of the fmaf chain; measured at M = 64 on 3 300 sources of 303 rows that each score a 303-row span
// (tools/selfmatch_bench.py --cross): 1 -> 8.53 ms, 2 (identify_pq.hip's count for query rows in global
// memory) -> 7.83 ms, 4 -> 7.40 ms, 8 -> 7.31 ms at 120 instead of 90 VGPRs.
constexpr int XM_UNROLL = 4, XM_UNROLL_PQ = 4;

__global__ __launch_bounds__(SM_PLAN_THREADS) void cross_match_plan_kernel(const int64_t *__restrict__ src_first,
                                                                           int n_src, int k, int min_votes,
                                                                           int64_t *__restrict__ off) {
    plan_sources(TableSource{nullptr, src_first}, n_src, k, min_votes, off);
}

__global__ __launch_bounds__(SM_THREADS) void cross_match_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T,
    const float *__restrict__ q_rows, const int64_t *__restrict__ src_first, const int64_t *__restrict__ ids, int k,
    int top, int min_votes, int min_overlap, unsigned long long *__restrict__ ws, int64_t head_units, int64_t cap_units,
    int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta, int32_t *__restrict__ out_start,
    int32_t *__restrict__ out_len, float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    const TableSource source{q_rows, src_first};
    const RowSpan<XM_UNROLL> span{reinterpret_cast<const float4 *>(rows)};
    match_source(MatchDenseGrid{}, source, span, n, first, T, ids, k, top, min_votes, min_overlap, ws, head_units, cap_units, out_track,
                 out_delta, out_start, out_len, out_score, out_votes);
}

template <int kM>
__global__ __launch_bounds__(SM_THREADS) void cross_match_pq_kernel(
    const int32_t *__restrict__ list_id, const unsigned char *__restrict__ codes, int64_t n,
    const float *__restrict__ centroids, int nlist, const float *__restrict__ codebooks,
    const int64_t *__restrict__ first, int T, const float *__restrict__ q_rows, const int64_t *__restrict__ src_first,
    const int64_t *__restrict__ ids, int k, int top, int min_votes, int min_overlap,
    unsigned long long *__restrict__ ws, int64_t head_units, int64_t cap_units, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_delta, int32_t *__restrict__ out_start, int32_t *__restrict__ out_len,
    float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    const TableSource source{q_rows, src_first};
    const PqSpan<kM, XM_UNROLL_PQ> span{list_id, codes, centroids, codebooks, nlist};
    match_source(MatchDenseGrid{}, source, span, n, first, T, ids, k, top, min_votes, min_overlap, ws, head_units, cap_units, out_track,
                 out_delta, out_start, out_len, out_score, out_votes);
}

static int cross_match_plan(const int64_t *src_first, int n_src, int k, int min_votes, void *ws, hipStream_t stream) {
    hipLaunchKernelGGL(cross_match_plan_kernel, dim3(1), dim3(SM_PLAN_THREADS), 0, stream, src_first, n_src, k,
                       min_votes, reinterpret_cast<int64_t *>(ws));
    GRAFP_CHECK_LAUNCH("cross_match_plan_kernel");
    return GRAFP_OK;
}

int cross_match_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                       const int64_t *src_first, int n_src, const int64_t *ids, int k, int top, int min_votes,
                       int min_overlap, void *ws, size_t ws_bytes, int32_t *out_track, int32_t *out_delta,
                       int32_t *out_start, int32_t *out_len, float *out_score, int32_t *out_votes, hipStream_t stream) {
    int st = sm_check_launch("cross_match", k, top, min_votes, min_overlap, n_src, ws, ws_bytes);
    if (st != GRAFP_OK || n_src == 0) return st;
    if ((st = cross_match_plan(src_first, n_src, k, min_votes, ws, stream)) != GRAFP_OK) return st;
    return sm_launch("cross_match_kernel", cross_match_kernel, dim3(n_src), stream, rows, n, first, T, q_rows, src_first,
                     ids, k, top, min_votes, min_overlap, reinterpret_cast<unsigned long long *>(ws),
                     sm_head_bytes(n_src) / 8, (int64_t)(ws_bytes / 8), out_track, out_delta, out_start, out_len,
                     out_score, out_votes);
}

int cross_match_pq_launch(const int32_t *list_id, const unsigned char *codes, int64_t n, const float *centroids,
                          int nlist, const float *codebooks, int M, const int64_t *first, int T, const float *q_rows,
                          const int64_t *src_first, int n_src, const int64_t *ids, int k, int top, int min_votes,
                          int min_overlap, void *ws, size_t ws_bytes, int32_t *out_track, int32_t *out_delta,
                          int32_t *out_start, int32_t *out_len, float *out_score, int32_t *out_votes,
                          hipStream_t stream) {
    GRAFP_REQUIRE(M == 16 || M == 32 || M == 64 || M == 128, "cross_match_pq: M=%d not one of 16, 32, 64, 128", M);
    int st = sm_check_launch("cross_match_pq", k, top, min_votes, min_overlap, n_src, ws, ws_bytes);
    if (st != GRAFP_OK || n_src == 0) return st;
    if ((st = cross_match_plan(src_first, n_src, k, min_votes, ws, stream)) != GRAFP_OK) return st;
#define GRAFP_XMPQ_CASE(m)                                                                                             \
    case m:                                                                                                            \
        return sm_launch("cross_match_pq_kernel", cross_match_pq_kernel<m>, dim3(n_src), stream, list_id, codes, n,    \
                         centroids, nlist, codebooks, first, T, q_rows, src_first, ids, k, top, min_votes,             \
                         min_overlap, reinterpret_cast<unsigned long long *>(ws), sm_head_bytes(n_src) / 8,            \
                         (int64_t)(ws_bytes / 8), out_track, out_delta, out_start, out_len, out_score, out_votes)
    switch (M) {
        GRAFP_XMPQ_CASE(16);
        GRAFP_XMPQ_CASE(32);
        GRAFP_XMPQ_CASE(64);
        default:
            GRAFP_XMPQ_CASE(128);
    }
#undef GRAFP_XMPQ_CASE
}

}  // namespace grafp
