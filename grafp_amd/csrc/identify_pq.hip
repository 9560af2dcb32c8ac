// identify_pq.hip -- track-aware sequence identification against a library held as IVF-PQ codes (grafp_amd/library.py's
// compact form, ops.identify_pq), gfx950.
//
// The same operation as identify.hip, on rows that exist only as codes.  Library row r is
//   dec[r][j] = centroids[list_id[r]][j] + codebooks[m][codes[r][m]][c],  m = j / dsub, c = j % dsub, dsub = 128 / M
// (one f32 add per element, never an fma: the f32 form of oracle/ivfpq.py::reconstruct), and every output is bit for bit
// what identify_kernel writes when it is handed the (n, 128) f32 array dec.  Candidates, eligibility, the per-track best,
// the ranking, the ties, the LDS layout and phases 1, 2, 4 and 5 are identify_core.h's identify_item, shared with
// identify.hip; only the span rows of phase 3 differ (PqSpan of span_rows.h).
//
// Per row a lane of the half-wave (it owns dims 4l..4l+3) reads its float4 of the row's coarse centroid, the code
// byte(s) of the sub-spaces that hold its dims and the codewords those bytes name:
//   M = 16  (dsub 8): 1 byte  (sub-space l / 2), one float4 of the 8-float codeword
//   M = 32  (dsub 4): 1 byte  (sub-space l),     the whole float4 codeword
//   M = 64  (dsub 2): 2 bytes (2l, 2l + 1; the half-wave reads the row's 64 code bytes as one coalesced access), two float2
//   M = 128 (dsub 1): 4 bytes (4l .. 4l + 3; 128 bytes per half-wave), four floats
// The codebooks (M * 256 * dsub floats = 128 KiB for any M) and the centroids are read from global memory: every
// workgroup gathers from the same 128 KiB, so they stay in L2.  The chain of a row is list id / code byte -> centroid /
// codeword address -> add -> fmaf, one dependent load longer than span_sum's; the loop is unrolled by kUnroll rows so
// that the list ids and code bytes of the next rows are issued ahead of the fmaf chain of this one.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as identify.hip.
#include "identify_core.h"
#include "span_rows.h"

namespace grafp {

// rows decoded ahead of the fmaf chain: query rows in LDS / in global memory
constexpr int IDPQ_UNROLL_QLDS = 4, IDPQ_UNROLL_QGLOBAL = 2;

template <int kM, bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_pq_kernel(
    const int32_t *__restrict__ list_id, const unsigned char *__restrict__ codes, int64_t n,
    const float *__restrict__ centroids, int nlist, const float *__restrict__ codebooks,
    const int64_t *__restrict__ first, int T, const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k,
    const int64_t *__restrict__ item_row, const int *__restrict__ item_len, int max_len, int Pmax, int top,
    int min_overlap, int32_t *__restrict__ out_track, int32_t *__restrict__ out_offset, float *__restrict__ out_score,
    int32_t *__restrict__ out_votes) {
    const PqSpan<kM, kQLds ? IDPQ_UNROLL_QLDS : IDPQ_UNROLL_QGLOBAL> span{list_id, codes, centroids, codebooks, nlist};
    identify_item<kQLds>(DenseGrid{}, span, n, first, T, q_rows, ids, k, item_row, item_len, max_len, Pmax, top, min_overlap,
                         out_track, out_offset, out_score, out_votes);
}

int identify_pq_launch(const int32_t *list_id, const unsigned char *codes, int64_t n, const float *centroids, int nlist,
                       const float *codebooks, int M, const int64_t *first, int T, const float *q_rows,
                       const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                       int max_len, int top, int min_overlap, int32_t *out_track, int32_t *out_offset, float *out_score,
                       int32_t *out_votes, hipStream_t stream) {
    GRAFP_REQUIRE(M == 16 || M == 32 || M == 64 || M == 128, "identify_pq: M=%d not one of 16, 32, 64, 128", M);
    const int st = id_check_launch("identify_pq", max_len, k);
    if (st != GRAFP_OK || n_items == 0) return st;
    const IdentifyPlan plan = identify_plan(max_len, k);
    decltype(&identify_pq_kernel<16, true>) q_lds, q_global;
#define GRAFP_IDPQ_CASE(m)                                                                                             \
    case m:                                                                                                            \
        q_lds = identify_pq_kernel<m, true>, q_global = identify_pq_kernel<m, false>;                                  \
        break
    switch (M) {
        GRAFP_IDPQ_CASE(16);
        GRAFP_IDPQ_CASE(32);
        GRAFP_IDPQ_CASE(64);
        default:
            GRAFP_IDPQ_CASE(128);
    }
#undef GRAFP_IDPQ_CASE
    return id_launch("identify_pq", q_lds, q_global, plan, dim3(n_items), stream, list_id, codes, n, centroids, nlist,
                     codebooks, first, T, q_rows, ids, k, item_row, item_len, max_len, plan.Pmax, top, min_overlap,
                     out_track, out_offset, out_score, out_votes);
}

}  // namespace grafp
