// selfmatch.hip -- shared audio inside a track-indexed fingerprint library (grafp_amd/library.py, ops.self_match),
// gfx950.
//
// The library is the resident (n, 128) f32 rows of T tracks laid end to end (track t owns rows [first[t], first[t+1])),
// and ids (n, k) the top-k hits of every row from searching the library against itself.  For one source track a of
// L rows:
//   * row first[a] + i (i < L) with hit r in [0, n) outside track a names the track b holding r and j = r - first[b];
//     it votes for the candidate (b, delta = j - i).  Hits inside a are dropped; duplicate ids vote twice;
//   * a candidate's span is [i_lo, i_hi], the smallest and largest voting i, m = i_hi - i_lo + 1 rows; it is eligible
//     iff votes >= min_votes and m >= min_overlap, and then scores
//     (sum_{i = i_lo .. i_hi} <row[first[a] + i], row[first[b] + i + delta]>) / m;
//   * per partner b the eligible candidate with the highest score is kept (ties: the smaller delta), and the `top`
//     partners are written by score descending, then b ascending.
// Arithmetic order of a score: span_sum of seqmatch.h, then score = sum / m (IEEE division) -- shared with
// identify_kernel, so a span identify would also score gets the same bits.
//
// One workgroup of 512 threads per source track.  Its hit keys (a_g + L) << 32 | i, with a_g = r - i the global row
// where the source's row 0 would sit, number N0 = L * k; they are sorted ascending by a bitonic network over
// P1 = pow2(max(64, N0)) slots:
//   * P1 <= SM_PIECE (16 384 keys, the 128 KiB of dynamic LDS): entirely in LDS;
//   * otherwise in the caller's workspace, in LDS-sized pieces: every stage with a partner distance below SM_PIECE runs
//     on a piece loaded into LDS (all such stages of one merge level in one visit), only the longer distances run on
//     global memory -- so a 10-minute track (6 250 rows, 200 k hits at k = 32) is sorted, not refused or cut.
// Phases, each ended by a barrier:
//   1. hit keys (own-track and out-of-range ids become empty keys, which sort last), then the sort;
//   2. the first slot of every alignment run walks it (as identify does): the track is looked up once per run, a run
//      that crosses a track boundary continues as a candidate of the next track.  Votes and the span are counted on the
//      way; only ELIGIBLE candidates (most are single random votes) are appended to the record list in the workspace:
//      {b, a_g + L, i_lo, m, votes, score};
//   3. the records are scored, one per half-wave (coalesced 512-byte row reads);
//   4. keys b << 32 | record are sorted; the first slot of every partner run walks it for its best record (highest
//      score, then smaller a_g = smaller delta) and writes ~ord(score) << 32 | slot;
//   5. those are sorted and the first `top` are the answer (the slot leads back to the partner run, walked again).
// The sorts of phases 4-5 run in LDS when both key arrays fit next to each other, otherwise in the workspace.
// Workspace: a header of n_src + 1 int64 region starts written by the plan kernel (an exclusive scan of the
// per-source sizes sm_units), then one region per source: records (24 bytes x ceil(N0 / min_votes)), the phase 4 and 5
// keys (pow2(max(64, records)) each), and the hit keys when they do not fit in LDS.  self_match_workspace sums the same
// sizes on the host from the sources' row counts, so the caller's buffer is exactly what the launch lays out.  A source
// whose region ends past ws_bytes writes -2 to its first out_track slot and nothing else.
// The phases are match_source of selfmatch_core.h, shared with crossmatch.hip (the same operation for recordings held
// outside the library, against f32 rows or IVF-PQ codes); this file supplies the source (SelfSource: tracks of the
// library, own-track hits dropped), the span rows (RowSpan: the resident f32 rows) and the launch.
// Built WITHOUT packed-f32 instructions (Makefile NOPK, as identify.hip): its sums are plain fmaf chains, and the packed
// operand-select form is the hazard of DESIGN.md section 12.7b.
#include "selfmatch_core.h"
#include "span_rows.h"

namespace grafp {

constexpr int SM_UNROLL = 4;                                // row pairs in flight in the score loop (span_sum)

__global__ __launch_bounds__(SM_PLAN_THREADS) void self_match_plan_kernel(const int64_t *__restrict__ first,
                                                                          const int *__restrict__ tracks, int n_src,
                                                                          int k, int min_votes, int64_t *__restrict__ off) {
    plan_sources(SelfSource{nullptr, first, tracks}, n_src, k, min_votes, off);
}

__global__ __launch_bounds__(SM_THREADS) void self_match_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, const int64_t *__restrict__ ids,
    int k, const int *__restrict__ tracks, int top, int min_votes, int min_overlap, unsigned long long *__restrict__ ws,
    int64_t head_units, int64_t cap_units, int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta,
    int32_t *__restrict__ out_start, int32_t *__restrict__ out_len, float *__restrict__ out_score,
    int32_t *__restrict__ out_votes) {
    const SelfSource source{rows, first, tracks};
    const RowSpan<SM_UNROLL> span{reinterpret_cast<const float4 *>(rows)};
    match_source(MatchDenseGrid{}, source, span, n, first, T, ids, k, top, min_votes, min_overlap, ws, head_units, cap_units, out_track,
                 out_delta, out_start, out_len, out_score, out_votes);
}

size_t self_match_workspace(const int64_t *src_rows, int n_src, int k, int min_votes) {
    if (n_src < 0 || (n_src > 0 && !src_rows) || k < 1 || min_votes < 1) return 0;
    int64_t units = 0;                                    // exactly the regions plan_sources lays out
    for (int s = 0; s < n_src; ++s) units += sm_units(src_rows[s], k, min_votes);
    return (size_t)(sm_head_bytes(n_src) + 8 * units);
}

int self_match_launch(const float *rows, int64_t n, const int64_t *first, int T, const int64_t *ids, int k,
                      const int *tracks, int n_src, int top, int min_votes, int min_overlap, void *ws,
                      size_t ws_bytes, int32_t *out_track, int32_t *out_delta, int32_t *out_start, int32_t *out_len,
                      float *out_score, int32_t *out_votes, hipStream_t stream) {
    const int st = sm_check_launch("self_match", k, top, min_votes, min_overlap, n_src, ws, ws_bytes);
    if (st != GRAFP_OK || n_src == 0) return st;
    hipLaunchKernelGGL(self_match_plan_kernel, dim3(1), dim3(SM_PLAN_THREADS), 0, stream, first, tracks, n_src, k,
                       min_votes, reinterpret_cast<int64_t *>(ws));
    GRAFP_CHECK_LAUNCH("self_match_plan_kernel");
    return sm_launch("self_match_kernel", self_match_kernel, dim3(n_src), stream, rows, n, first, T, ids, k, tracks,
                     top, min_votes, min_overlap, reinterpret_cast<unsigned long long *>(ws), sm_head_bytes(n_src) / 8,
                     (int64_t)(ws_bytes / 8), out_track, out_delta, out_start, out_len, out_score, out_votes);
}

}  // namespace grafp
