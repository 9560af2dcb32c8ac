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
// The pass 1 body, the merge and the launch checks are match_tempo.h's, shared with selfmatch_tempo.hip (the same operation
// for the tracks of the library itself); this file supplies the source (TableSource) and the three kernels.
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
#include "match_tempo.h"

namespace grafp {

size_t self_match_workspace(const int64_t *src_rows, int n_src, int k, int min_votes);      // selfmatch.hip

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
    xt_match_pass(TableSource{q_rows, src_first}, rows, n, first, T, ratios, R, ids, k, top, min_votes, min_overlap, ws,
                  head_units, cap_units);
}

__global__ __launch_bounds__(XT_MERGE_THREADS) void cross_match_tempo_merge_kernel(
    TempoRatios ratios, int R, int top, const unsigned long long *__restrict__ ws, int64_t head_units,
    int64_t cap_units, int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta,
    int32_t *__restrict__ out_start, int32_t *__restrict__ out_len, float *__restrict__ out_score,
    int32_t *__restrict__ out_votes, int32_t *__restrict__ out_ratio) {
    xt_merge(ratios, R, top, ws, head_units, cap_units, out_track, out_delta, out_start, out_len, out_score, out_votes,
             out_ratio);
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
    // the longest source has at most min(n_qrows, SM_TEMPO_MAX_ROWS) rows (longer ones are padding)
    const int st = xt_check_launch("cross_match_tempo", n, n_qrows, k, top, min_votes, min_overlap, n_src, ratio_num,
                                   n_ratios, ws, ws_bytes, ratios);
    if (st != GRAFP_OK || n_src == 0) return st;
    hipLaunchKernelGGL(cross_match_tempo_plan_kernel, dim3(1), dim3(SM_PLAN_THREADS), 0, stream, src_first, n_src, k,
                       min_votes, reinterpret_cast<int64_t *>(ws));
    GRAFP_CHECK_LAUNCH("cross_match_tempo_plan_kernel");
    return xt_launch_passes("cross_match_tempo", cross_match_tempo_kernel, cross_match_tempo_merge_kernel, n_src, ratios,
                            n_ratios, top, ws, ws_bytes, out_track, out_delta, out_start, out_len, out_score, out_votes,
                            out_ratio, stream, rows, n, first, T, ratios, n_ratios, q_rows, src_first, ids, k, top,
                            min_votes, min_overlap);
}

}  // namespace grafp
