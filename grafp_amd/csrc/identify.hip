// identify.hip -- track-aware sequence identification against a track-indexed fingerprint library
// (grafp_amd/library.py, ops.identify), gfx950.
//
// The library is the resident (n, 128) f32 fingerprint rows of T tracks laid end to end; track t owns rows
// [first[t], first[t+1]).  For one item (ql query segments q[0..ql), whose top-k library ids are already known from one
// batched search):
//   * every hit (s, r), r >= 0, names the track t that holds row r and the alignment a = r - s (the global row where
//     query segment 0 would sit); a candidate is a unique (t, a), its votes the number of hits that map to it;
//   * the overlap of (t, a) is the s in [0, ql) with a + s inside track t, o rows; the candidate is eligible iff
//     o >= min(min_overlap, L_t) (min_overlap <= 0: the item's ql) and is scored over those rows only --
//     score = (sum_s <q[s], row[a + s]>) / o.  No row outside track t is ever read for a candidate of t;
//   * the best candidate per track (highest score, then the smaller a) is kept, and the `top` tracks are written by
//     score descending, then track ascending.
// Arithmetic order of a score: span_sum of seqmatch.h, then score = sum / o (IEEE division) -- shared with
// seq_rerank_kernel, so a run wholly inside one track scores bit-equal to seq_rerank's score of the same start row.
//
// One workgroup of 256 threads per item.  All per-item state lives in dynamic LDS sized by the launch's largest item,
// Pmax = next power of two >= max(64, max_len * k) slots of 16 bytes:
//   keys  u64[Pmax]  hit keys (a + 255) << 32 | s, then candidates, then rank keys
//   aux   u32[Pmax]  the track of a candidate, then its a + 255
//   votes u16[Pmax]  votes of a candidate (<= ql * k <= 8192)
//   idx   u16[Pmax]  compacted candidate slots, then the slot that travels with a rank key
// plus the item's query rows (max_len * 512 bytes) when the total fits the 160 KiB of a CU; otherwise the query rows are
// read from global memory (L2-resident: every candidate of the item reads them).  Limits: ql <= 256, k <= 32,
// max_len * k <= 8192 (128 KiB of slots).
// Phases, each ended by a barrier:
//   1. hit keys -> bitonic sort (a, s): equal alignments form runs, s ascending inside a run, so r = a + s ascends too;
//   2. the first thread of every alignment run looks the track up ONCE (binary search of first[] in global memory) and
//      walks its run: votes are counted while r stays below the track's end; a run that crosses a track boundary
//      continues as a new candidate of the next track (one more lookup).  Each candidate is written to the slot of its
//      first hit (slot order = a ascending for one track); every other slot of the run becomes empty;
//   3. candidates are compacted and scored one per half-wave (coalesced 512-byte row reads); the rank key
//      t << 32 | ~ord(score) replaces the candidate in its own slot;
//   4. bitonic sort of (rank key, slot): the first entry of every track run is that track's best (ties: lower slot =
//      smaller a); it becomes ~ord(score) << 32 | t, every other entry empty;
//   5. bitonic sort of those; the first `top` entries are the result.
// The five phases are identify_item of identify_core.h, shared with identify_pq.hip (the same operation on a library held
// as IVF-PQ codes), identify_thin.hip (a library that keeps every D-th row of a track) and identify_tempo.hip (recordings
// that play faster or slower than the catalogue: one run of the phases per speed ratio); this file supplies the row grid
// (DenseGrid: one row per segment), the span rows of phase 3 (RowSpan of span_rows.h: the resident f32 rows) and the launch.
// Built WITHOUT packed-f32 instructions (Makefile NOPK, as corpus.hip): its sums are plain fmaf chains, and the packed
// operand-select form is the hazard of DESIGN.md section 12.7b.
#include "identify_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop (seqmatch.h, span_sum): query rows in LDS / in global memory
constexpr int ID_UNROLL_QLDS = 4, ID_UNROLL_QGLOBAL = 1;

template <bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T,
    const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k, const int64_t *__restrict__ item_row,
    const int *__restrict__ item_len, int max_len, int Pmax, int top, int min_overlap, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_offset, float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    const RowSpan<kQLds ? ID_UNROLL_QLDS : ID_UNROLL_QGLOBAL> span{reinterpret_cast<const float4 *>(rows)};
    identify_item<kQLds>(DenseGrid{}, span, n, first, T, q_rows, ids, k, item_row, item_len, max_len, Pmax, top, min_overlap,
                         out_track, out_offset, out_score, out_votes);
}

int identify_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                    const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items, int max_len,
                    int top, int min_overlap, int32_t *out_track, int32_t *out_offset, float *out_score,
                    int32_t *out_votes, hipStream_t stream) {
    const int st = id_check_launch("identify", max_len, k);
    if (st != GRAFP_OK || n_items == 0) return st;
    const IdentifyPlan plan = identify_plan(max_len, k);
    return id_launch("identify", identify_kernel<true>, identify_kernel<false>, plan, dim3(n_items), stream, rows, n,
                     first, T, q_rows, ids, k, item_row, item_len, max_len, plan.Pmax, top, min_overlap, out_track,
                     out_offset, out_score, out_votes);
}

}  // namespace grafp
