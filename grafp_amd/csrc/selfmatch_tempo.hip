// selfmatch_tempo.hip -- tracks of a track-indexed fingerprint library that share audio at another speed: a sped-up or
// slowed-down re-release, a varispeed remaster (grafp_amd/library.py's self_matches(tempo=...), ops.self_match_tempo),
// gfx950.
//
// selfmatch.hip's operation along sloped alignments, which is crossmatch_tempo.hip's with the library's own tracks as the
// sources.  A ratio is an integer num in [128, 512] that stands for num / 256 rows of the partner per row of the source;
// at ratio num row i of a source sits w(i) = (i * num + 128) >> 8 rows after the source's row 0: integer arithmetic, the
// same on host and device.  For source track a of L rows (library rows first[a] + i; at most 4 194 303 of them) and every
// ratio j of the call's R <= 64 strictly ascending ratios:
//   * a hit r of row i counts when it lies in [0, n) and outside [first[a], first[a + 1]) (own-track hits are dropped as
//     in self_match); it names the track b holding r and the alignment a_g = r - w_j(i) (the library row on which the
//     source's row 0 would sit); a candidate is a unique (b, a_g, j), its votes the hits that map to it (duplicate ids
//     vote twice); an alignment run that crosses a track boundary continues as a candidate of the next track;
//   * its span is [i_lo, i_hi], the smallest and largest voting i, m = i_hi - i_lo + 1; it is eligible iff votes >=
//     min_votes and m >= min_overlap, and then scores (sum_{i = i_lo .. i_hi} <row[first[a] + i], row[a_g + w_j(i)]>) / m
//     in span_sum's order (seqmatch.h), the partner's rows gathered.  All those rows lie inside track b, because w_j
//     never decreases and the two end rows do;
//   * per partner b the best eligible candidate over all ratios: highest score, then the ratio nearer to 1 (smaller
//     |num - 256|, then smaller num), then the smaller a_g; the `top` partners by score descending, then b ascending.
//     Seven (n_src, top) outputs: track b, delta = a_g - first[b], start = i_lo, length = m, score, votes, ratio = num,
//     padded with -1 / INT_MIN / -1 / 0 / -inf / 0 / 0.
// With the one ratio 256 the first six outputs are self_match_kernel's bit for bit.  For any ratios all seven are
// cross_match_tempo's on q_rows = the source tracks' own rows laid end to end and those rows' hits with every hit inside
// the source's own track replaced by -1: both run match_source on MatchTempoGrid and TempoRowSpan and the same merge
// (match_tempo.h), and a dropped hit and a -1 are the same empty key.
//
// Plan, self_match_tempo_plan_kernel: plan_sources on SelfSource fills the header once.  The workspace is
// crossmatch_tempo.hip's exactly -- header, R copies of the per-source regions (ratio j's starts j * off[n_src] units
// after ratio 0's), six (R, n_src, top) list arrays -- so grafp_cross_match_tempo_workspace, fed the source tracks' row
// counts, is its size.
// Pass 1, self_match_tempo_kernel, grid (n_src, R): xt_match_pass of match_tempo.h on SelfSource.
// Pass 2, self_match_tempo_merge_kernel, one workgroup per source: xt_merge, the R * top <= 4096 list entries.
// A workspace below the plan's layout writes nothing outside ws and every output is padding (no -2 mark); a source of
// more than SM_TEMPO_MAX_ROWS rows is padding (ops refuses it first); the host keeps n + 2 * longest < 2^32 with longest
// bounded by n, the only bound it has on a track's rows.
// All three kernels go out on the caller's stream with no host synchronisation; no atomics on floats.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as selfmatch.hip and crossmatch_tempo.hip.
#include "match_tempo.h"

namespace grafp {

__global__ __launch_bounds__(SM_PLAN_THREADS) void self_match_tempo_plan_kernel(const int64_t *__restrict__ first,
                                                                                const int *__restrict__ tracks,
                                                                                int n_src, int k, int min_votes,
                                                                                int64_t *__restrict__ off) {
    plan_sources(SelfSource{nullptr, first, tracks}, n_src, k, min_votes, off);
}

__global__ __launch_bounds__(SM_THREADS) void self_match_tempo_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, TempoRatios ratios, int R,
    const int64_t *__restrict__ ids, int k, const int *__restrict__ tracks, int top, int min_votes, int min_overlap,
    unsigned long long *__restrict__ ws, int64_t head_units, int64_t cap_units) {
    xt_match_pass(SelfSource{rows, first, tracks}, rows, n, first, T, ratios, R, ids, k, top, min_votes, min_overlap, ws,
                  head_units, cap_units);
}

__global__ __launch_bounds__(XT_MERGE_THREADS) void self_match_tempo_merge_kernel(
    TempoRatios ratios, int R, int top, const unsigned long long *__restrict__ ws, int64_t head_units,
    int64_t cap_units, int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta,
    int32_t *__restrict__ out_start, int32_t *__restrict__ out_len, float *__restrict__ out_score,
    int32_t *__restrict__ out_votes, int32_t *__restrict__ out_ratio) {
    xt_merge(ratios, R, top, ws, head_units, cap_units, out_track, out_delta, out_start, out_len, out_score, out_votes,
             out_ratio);
}

int self_match_tempo_launch(const float *rows, int64_t n, const int64_t *first, int T, const int64_t *ids, int k,
                            const int *tracks, int n_src, int top, int min_votes, int min_overlap,
                            const int32_t *ratio_num, int n_ratios, void *ws, size_t ws_bytes, int32_t *out_track,
                            int32_t *out_delta, int32_t *out_start, int32_t *out_len, float *out_score,
                            int32_t *out_votes, int32_t *out_ratio, hipStream_t stream) {
    TempoRatios ratios;
    // a track has at most n rows (the table is device memory)
    const int st = xt_check_launch("self_match_tempo", n, n, k, top, min_votes, min_overlap, n_src, ratio_num, n_ratios,
                                   ws, ws_bytes, ratios);
    if (st != GRAFP_OK || n_src == 0) return st;
    hipLaunchKernelGGL(self_match_tempo_plan_kernel, dim3(1), dim3(SM_PLAN_THREADS), 0, stream, first, tracks, n_src, k,
                       min_votes, reinterpret_cast<int64_t *>(ws));
    GRAFP_CHECK_LAUNCH("self_match_tempo_plan_kernel");
    return xt_launch_passes("self_match_tempo", self_match_tempo_kernel, self_match_tempo_merge_kernel, n_src, ratios,
                            n_ratios, top, ws, ws_bytes, out_track, out_delta, out_start, out_len, out_score, out_votes,
                            out_ratio, stream, rows, n, first, T, ratios, n_ratios, ids, k, tracks, top, min_votes,
                            min_overlap);
}

}  // namespace grafp
