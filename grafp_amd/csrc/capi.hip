// capi.hip -- ABI version and thread-local error message.
#include <stdarg.h>
#include <stdio.h>

#include "common.h"

namespace grafp {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace grafp

extern "C" int grafp_abi_version(void) { return GRAFP_ABI_VERSION; }
extern "C" const char *grafp_last_error(void) { return grafp::g_err; }

// Test utility: `blocks` workgroups of `threads` threads that do nothing but hold their CU slots for `clocks` shader
// cycles (tests/test_gpu_kernels.py runs the BatchNorm rendezvous next to it -- the stand-in for a collective's kernels
// occupying CUs while backward runs).
namespace grafp {
__global__ void occupy_kernel(long long clocks, int *sink) {
    const long long t0 = __builtin_readcyclecounter();
    int spins = 0;
    while ((long long)__builtin_readcyclecounter() - t0 < clocks) {
        __builtin_amdgcn_s_sleep(32);
        ++spins;
    }
    if (sink && spins < 0) *sink = spins;
}
}  // namespace grafp
extern "C" int grafp_debug_occupy(int blocks, int threads, int64_t clocks, grafp_stream_t stream) {
    GRAFP_REQUIRE(blocks > 0 && threads > 0 && threads <= 1024 && clocks >= 0, "debug_occupy: bad arguments");
    hipLaunchKernelGGL(grafp::occupy_kernel, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, (long long)clocks,
                       (int *)nullptr);
    GRAFP_CHECK_LAUNCH("occupy_kernel");
    return GRAFP_OK;
}

// Device-resident training corpus (corpus.hip): argument checks here, kernels and launch plans there.
namespace grafp {
int resample_launch(const float *in, const int64_t *in_start, const int64_t *in_len, const int64_t *out_start,
                    int n_tracks, int64_t max_in_len, int orig, int nw, int width, int K, const float *taps, float *out,
                    hipStream_t stream);
int resample_plan(int orig, int nw, int K, int *info);
int draw_pairs_launch(const float *bank, const int64_t *track_start, const int64_t *track_len, const float *norm,
                      int n_tracks, const int32_t *row_track, const float *uniforms, int B, int A, int clip,
                      int offset_mod, float silence, float *x_i, float *x_j, int32_t *silent_rows, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_resample_plan(int orig, int new_rate, int width, int K, int *info) {
    GRAFP_REQUIRE(info, "resample_plan: null pointer");
    for (int i = 0; i < 8; ++i) info[i] = 0;
    GRAFP_REQUIRE(orig > 0 && new_rate > 0 && width >= 0 && K == 2 * width + orig,
                  "resample_plan: bad filter orig=%d new=%d width=%d K=%d", orig, new_rate, width, K);
    return grafp::resample_plan(orig, new_rate, K, info);
}

extern "C" int grafp_resample_f32(const float *in, const int64_t *in_start, const int64_t *in_len,
                                  const int64_t *out_start, int n_tracks, int64_t max_in_len, int orig, int new_rate,
                                  int width, int K, const float *taps, float *out, grafp_stream_t stream) {
    GRAFP_REQUIRE(in && in_start && in_len && out_start && out, "resample: null pointer");
    GRAFP_REQUIRE(n_tracks > 0 && n_tracks <= 65535 && max_in_len >= 0, "resample: bad sizes n_tracks=%d max_in_len=%lld",
                  n_tracks, (long long)max_in_len);
    GRAFP_REQUIRE(orig > 0 && new_rate > 0 && width >= 0 && K == 2 * width + orig,
                  "resample: bad filter orig=%d new=%d width=%d K=%d", orig, new_rate, width, K);
    return grafp::resample_launch(in, in_start, in_len, out_start, n_tracks, max_in_len, orig, new_rate, width, K, taps,
                                  out, (hipStream_t)stream);
}

extern "C" int grafp_draw_pairs_f32(const float *bank, const int64_t *track_start, const int64_t *track_len,
                                    const float *norm, int n_tracks, const int32_t *row_track, const float *uniforms,
                                    int B, int A, int clip, int offset_mod, float silence, float *x_i, float *x_j,
                                    int32_t *silent_rows, grafp_stream_t stream) {
    GRAFP_REQUIRE(bank && track_start && track_len && norm && row_track && uniforms && x_i && x_j,
                  "draw_pairs: null pointer");
    GRAFP_REQUIRE(n_tracks > 0 && B > 0 && A > 0 && clip > 0 && offset_mod > clip,
                  "draw_pairs: bad sizes n_tracks=%d B=%d A=%d clip=%d offset_mod=%d", n_tracks, B, A, clip, offset_mod);
    GRAFP_REQUIRE(x_i != x_j, "draw_pairs: the two views must not alias");
    return grafp::draw_pairs_launch(bank, track_start, track_len, norm, n_tracks, row_track, uniforms, B, A, clip,
                                    offset_mod, silence, x_i, x_j, silent_rows, (hipStream_t)stream);
}

// The size, `top` and alignment checks that the identify entries, and those that the cross-match entries, repeat (name:
// the operation, for the message).  nlist: null for a library of f32 rows, which align16 covers with the query rows;
// else the library is held as IVF-PQ codes, nlist joins the sizes, align16 covers the centroids, the codebooks and the
// query rows and align4 the codes and the list ids.
static int check_aligned(const char *name, const int *nlist, uintptr_t align16, uintptr_t align4) {
    if (nlist)
        GRAFP_REQUIRE((align16 & 15) == 0 && (align4 & 3) == 0,
                      "%s: centroids, codebooks and query rows must be 16-byte aligned, codes and list ids 4-byte", name);
    else
        GRAFP_REQUIRE((align16 & 15) == 0, "%s: rows must be 16-byte aligned", name);
    return GRAFP_OK;
}

static int check_identify(const char *name, int64_t n, const int *nlist, int n_tracks, int64_t n_qrows, int n_items,
                          int top, uintptr_t align16, uintptr_t align4) {
    const bool sizes = n >= 1 && n < 0x7fffff00ll && n_tracks >= 1 && n_qrows >= 1 && n_items >= 0;
    if (nlist)
        GRAFP_REQUIRE(sizes && *nlist >= 1, "%s: bad sizes n=%lld nlist=%d n_tracks=%d n_qrows=%lld n_items=%d", name,
                      (long long)n, *nlist, n_tracks, (long long)n_qrows, n_items);
    else
        GRAFP_REQUIRE(sizes, "%s: bad sizes n=%lld n_tracks=%d n_qrows=%lld n_items=%d", name, (long long)n, n_tracks,
                      (long long)n_qrows, n_items);
    GRAFP_REQUIRE(top >= 1 && top <= 64, "%s: top=%d not in [1, 64]", name, top);
    return check_aligned(name, nlist, align16, align4);
}

static int check_cross_match(const char *name, int64_t n, const int *nlist, int n_tracks, int64_t n_qrows, int n_src,
                             uintptr_t align16, uintptr_t align4) {
    // n + the longest source < 2^32 (the width of a hit key's alignment half) follows from the two row bounds
    const bool sizes = n >= 1 && n < 0x7fffff00ll && n_tracks >= 1 && n_qrows >= 0 && n_qrows < 0x7fffff00ll && n_src >= 0;
    if (nlist)
        GRAFP_REQUIRE(sizes && *nlist >= 1, "%s: bad sizes n=%lld nlist=%d n_tracks=%d n_qrows=%lld n_src=%d", name,
                      (long long)n, *nlist, n_tracks, (long long)n_qrows, n_src);
    else
        GRAFP_REQUIRE(sizes, "%s: bad sizes n=%lld n_tracks=%d n_qrows=%lld n_src=%d", name, (long long)n, n_tracks,
                      (long long)n_qrows, n_src);
    return check_aligned(name, nlist, align16, align4);
}

// Track-aware sequence identification (identify.hip): argument checks here, the kernel and its LDS plan there.
namespace grafp {
int identify_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                    const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items, int max_len,
                    int top, int min_overlap, int32_t *out_track, int32_t *out_offset, float *out_score,
                    int32_t *out_votes, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_identify_f32(const float *index_rows, int64_t n, const int64_t *track_first_row, int n_tracks,
                                  const float *q_rows, int64_t n_qrows, const int64_t *topk_ids, int k,
                                  const int64_t *item_row, const int *item_len, int n_items, int max_len, int top,
                                  int min_overlap, int32_t *out_track, int32_t *out_offset, float *out_score,
                                  int32_t *out_votes, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && q_rows && topk_ids && item_row && item_len && out_track &&
                  out_offset && out_score && out_votes, "identify: null pointer");
    const int st = check_identify("identify", n, nullptr, n_tracks, n_qrows, n_items, top,
                                  (uintptr_t)index_rows | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::identify_launch(index_rows, n, track_first_row, n_tracks, q_rows, topk_ids, k, item_row, item_len,
                                  n_items, max_len, top, min_overlap, out_track, out_offset, out_score, out_votes,
                                  (hipStream_t)stream);
}

// Identification against a library that keeps every row_stride-th row of each track (identify_thin.hip): argument checks
// here and there (the stride and the 2^32 bound of the alignment key sit next to the kernel).
namespace grafp {
int identify_thin_launch(const float *rows, int64_t n, const int64_t *first, int T, int row_stride,
                         const float *q_rows, const int64_t *ids, int k, const int64_t *item_row, const int *item_len,
                         int n_items, int max_len, int top, int min_overlap, int32_t *out_track, int32_t *out_offset,
                         float *out_score, int32_t *out_votes, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_identify_thin_f32(const float *index_rows, int64_t n, const int64_t *track_first_row,
                                       int n_tracks, int row_stride, const float *q_rows, int64_t n_qrows,
                                       const int64_t *topk_ids, int k, const int64_t *item_row, const int *item_len,
                                       int n_items, int max_len, int top, int min_overlap, int32_t *out_track,
                                       int32_t *out_offset, float *out_score, int32_t *out_votes,
                                       grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && q_rows && topk_ids && item_row && item_len && out_track &&
                  out_offset && out_score && out_votes, "identify_thin: null pointer");
    const int st = check_identify("identify_thin", n, nullptr, n_tracks, n_qrows, n_items, top,
                                  (uintptr_t)index_rows | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::identify_thin_launch(index_rows, n, track_first_row, n_tracks, row_stride, q_rows, topk_ids, k,
                                       item_row, item_len, n_items, max_len, top, min_overlap, out_track, out_offset,
                                       out_score, out_votes, (hipStream_t)stream);
}

// Identification of items that hold every query_stride-th segment of the recording (identify_stride.hip): argument
// checks here and there (the stride and the 2^32 bound of the alignment key sit next to the kernel).
namespace grafp {
int identify_stride_launch(const float *rows, int64_t n, const int64_t *first, int T, int query_stride,
                           const float *q_rows, const int64_t *ids, int k, const int64_t *item_row,
                           const int *item_len, int n_items, int max_len, int top, int min_overlap, int32_t *out_track,
                           int32_t *out_offset, float *out_score, int32_t *out_votes, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_identify_stride_f32(const float *index_rows, int64_t n, const int64_t *track_first_row,
                                         int n_tracks, int query_stride, const float *q_rows, int64_t n_qrows,
                                         const int64_t *topk_ids, int k, const int64_t *item_row, const int *item_len,
                                         int n_items, int max_len, int top, int min_overlap, int32_t *out_track,
                                         int32_t *out_offset, float *out_score, int32_t *out_votes,
                                         grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && q_rows && topk_ids && item_row && item_len && out_track &&
                  out_offset && out_score && out_votes, "identify_stride: null pointer");
    const int st = check_identify("identify_stride", n, nullptr, n_tracks, n_qrows, n_items, top,
                                  (uintptr_t)index_rows | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::identify_stride_launch(index_rows, n, track_first_row, n_tracks, query_stride, q_rows, topk_ids, k,
                                         item_row, item_len, n_items, max_len, top, min_overlap, out_track, out_offset,
                                         out_score, out_votes, (hipStream_t)stream);
}

// Identification of recordings that play faster or slower than the catalogue (identify_tempo.hip): the checks shared
// with grafp_identify_f32 here, the ratio checks, the 2^32 bound of the alignment key and the two launches there.
namespace grafp {
int identify_tempo_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                          const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                          int max_len, int top, int min_overlap, const int32_t *ratio_num, int n_ratios, void *ws,
                          int32_t *out_track, int32_t *out_offset, float *out_score, int32_t *out_votes,
                          int32_t *out_ratio, hipStream_t stream);
size_t identify_tempo_workspace(int n_items, int n_ratios, int top);
}  // namespace grafp

extern "C" size_t grafp_identify_tempo_workspace(int n_items, int n_ratios, int top) {
    return grafp::identify_tempo_workspace(n_items, n_ratios, top);
}

extern "C" int grafp_identify_tempo_f32(const float *index_rows, int64_t n, const int64_t *track_first_row,
                                        int n_tracks, const float *q_rows, int64_t n_qrows, const int64_t *topk_ids,
                                        int k, const int64_t *item_row, const int *item_len, int n_items, int max_len,
                                        int top, int min_overlap, const int32_t *ratio_num, int n_ratios, void *ws,
                                        int32_t *out_track, int32_t *out_offset, float *out_score, int32_t *out_votes,
                                        int32_t *out_ratio, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && q_rows && topk_ids && item_row && item_len && ratio_num &&
                  out_track && out_offset && out_score && out_votes && out_ratio, "identify_tempo: null pointer");
    const int st = check_identify("identify_tempo", n, nullptr, n_tracks, n_qrows, n_items, top,
                                  (uintptr_t)index_rows | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::identify_tempo_launch(index_rows, n, track_first_row, n_tracks, q_rows, topk_ids, k, item_row,
                                        item_len, n_items, max_len, top, min_overlap, ratio_num, n_ratios, ws, out_track,
                                        out_offset, out_score, out_votes, out_ratio, (hipStream_t)stream);
}

// identify_tempo with a ratio window per item (identify_tempo_items.hip): the checks shared with grafp_identify_f32 here;
// the ratio checks, the table's sizes, the 2^32 bound of the alignment key and the two launches there.
namespace grafp {
int identify_tempo_items_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                                const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                                int max_len, int top, int min_overlap, const int32_t *ratio_num, int n_ratios,
                                const int32_t *work, int n_work, const int32_t *item_scan, int max_cnt, void *ws,
                                int32_t *out_track, int32_t *out_offset, float *out_score, int32_t *out_votes,
                                int32_t *out_ratio, hipStream_t stream);
size_t identify_tempo_items_workspace(int n_work, int top);
}  // namespace grafp

extern "C" size_t grafp_identify_tempo_items_workspace(int n_work, int top) {
    return grafp::identify_tempo_items_workspace(n_work, top);
}

extern "C" int grafp_identify_tempo_items_f32(const float *index_rows, int64_t n, const int64_t *track_first_row,
                                              int n_tracks, const float *q_rows, int64_t n_qrows,
                                              const int64_t *topk_ids, int k, const int64_t *item_row,
                                              const int *item_len, int n_items, int max_len, int top, int min_overlap,
                                              const int32_t *ratio_num, int n_ratios, const int32_t *work, int n_work,
                                              const int32_t *item_scan, int max_cnt, void *ws, int32_t *out_track,
                                              int32_t *out_offset, float *out_score, int32_t *out_votes,
                                              int32_t *out_ratio, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && q_rows && topk_ids && item_row && item_len && ratio_num &&
                  out_track && out_offset && out_score && out_votes && out_ratio, "identify_tempo_items: null pointer");
    const int st = check_identify("identify_tempo_items", n, nullptr, n_tracks, n_qrows, n_items, top,
                                  (uintptr_t)index_rows | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::identify_tempo_items_launch(index_rows, n, track_first_row, n_tracks, q_rows, topk_ids, k, item_row,
                                              item_len, n_items, max_len, top, min_overlap, ratio_num, n_ratios, work,
                                              n_work, item_scan, max_cnt, ws, out_track, out_offset, out_score,
                                              out_votes, out_ratio, (hipStream_t)stream);
}

// Identification against a library held as IVF-PQ codes (identify_pq.hip): argument checks here, the kernels there.
namespace grafp {
int identify_pq_launch(const int32_t *list_id, const unsigned char *codes, int64_t n, const float *centroids, int nlist,
                       const float *codebooks, int M, const int64_t *first, int T, const float *q_rows,
                       const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                       int max_len, int top, int min_overlap, int32_t *out_track, int32_t *out_offset, float *out_score,
                       int32_t *out_votes, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_identify_pq_f32(const int32_t *list_id, const uint8_t *codes, int64_t n, const float *centroids,
                                     int nlist, const float *codebooks, int M, const int64_t *track_first_row,
                                     int n_tracks, const float *q_rows, int64_t n_qrows, const int64_t *topk_ids, int k,
                                     const int64_t *item_row, const int *item_len, int n_items, int max_len, int top,
                                     int min_overlap, int32_t *out_track, int32_t *out_offset, float *out_score,
                                     int32_t *out_votes, grafp_stream_t stream) {
    GRAFP_REQUIRE(list_id && codes && centroids && codebooks && track_first_row && q_rows && topk_ids && item_row &&
                  item_len && out_track && out_offset && out_score && out_votes, "identify_pq: null pointer");
    const int st = check_identify("identify_pq", n, &nlist, n_tracks, n_qrows, n_items, top,
                                  (uintptr_t)centroids | (uintptr_t)codebooks | (uintptr_t)q_rows,
                                  (uintptr_t)codes | (uintptr_t)list_id);
    if (st != GRAFP_OK) return st;
    return grafp::identify_pq_launch(list_id, codes, n, centroids, nlist, codebooks, M, track_first_row, n_tracks, q_rows,
                                     topk_ids, k, item_row, item_len, n_items, max_len, top, min_overlap, out_track,
                                     out_offset, out_score, out_votes, (hipStream_t)stream);
}

// Identification against a library held as bf16 rows (identify_half.hip): grafp_identify_f32's checks here, the kernels
// there.
namespace grafp {
int identify_half_launch(const unsigned short *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                         const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                         int max_len, int top, int min_overlap, int32_t *out_track, int32_t *out_offset,
                         float *out_score, int32_t *out_votes, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_identify_half_f32(const void *index_rows_bf16, int64_t n, const int64_t *track_first_row,
                                       int n_tracks, const float *q_rows, int64_t n_qrows, const int64_t *topk_ids,
                                       int k, const int64_t *item_row, const int *item_len, int n_items, int max_len,
                                       int top, int min_overlap, int32_t *out_track, int32_t *out_offset,
                                       float *out_score, int32_t *out_votes, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows_bf16 && track_first_row && q_rows && topk_ids && item_row && item_len && out_track &&
                  out_offset && out_score && out_votes, "identify_half: null pointer");
    const int st = check_identify("identify_half", n, nullptr, n_tracks, n_qrows, n_items, top,
                                  (uintptr_t)index_rows_bf16 | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::identify_half_launch((const unsigned short *)index_rows_bf16, n, track_first_row, n_tracks, q_rows,
                                       topk_ids, k, item_row, item_len, n_items, max_len, top, min_overlap, out_track,
                                       out_offset, out_score, out_votes, (hipStream_t)stream);
}

// Shared audio inside a track-indexed library (selfmatch.hip): argument checks here, the kernels and the plan there.
namespace grafp {
size_t self_match_workspace(const int64_t *src_rows, int n_src, int k, int min_votes);
int self_match_launch(const float *rows, int64_t n, const int64_t *first, int T, const int64_t *ids, int k,
                      const int *tracks, int n_src, int top, int min_votes, int min_overlap, void *ws,
                      size_t ws_bytes, int32_t *out_track, int32_t *out_delta, int32_t *out_start, int32_t *out_len,
                      float *out_score, int32_t *out_votes, hipStream_t stream);
}  // namespace grafp

extern "C" size_t grafp_self_match_workspace(const int64_t *src_rows, int n_src, int k, int min_votes) {
    return grafp::self_match_workspace(src_rows, n_src, k, min_votes);
}

extern "C" int grafp_self_match_f32(const float *index_rows, int64_t n, const int64_t *track_first_row, int n_tracks,
                                    const int64_t *topk_ids, int k, const int *src_tracks, int n_src, int top,
                                    int min_votes, int min_overlap, void *ws, size_t ws_bytes, int32_t *out_track, int32_t *out_delta, int32_t *out_start, int32_t *out_len,
                                    float *out_score, int32_t *out_votes, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && topk_ids && src_tracks && out_track && out_delta && out_start &&
                  out_len && out_score && out_votes, "self_match: null pointer");
    GRAFP_REQUIRE(n >= 1 && n < 0x7fffff00ll && n_tracks >= 1 && n_src >= 0,
                  "self_match: bad sizes n=%lld n_tracks=%d n_src=%d", (long long)n, n_tracks, n_src);
    GRAFP_REQUIRE(((uintptr_t)index_rows & 15) == 0, "self_match: rows must be 16-byte aligned");
    return grafp::self_match_launch(index_rows, n, track_first_row, n_tracks, topk_ids, k, src_tracks, n_src, top,
                                    min_votes, min_overlap, ws, ws_bytes, out_track, out_delta, out_start, out_len,
                                    out_score, out_votes, (hipStream_t)stream);
}

// What recordings held outside a library share with it (crossmatch.hip): argument checks here, the kernels there.
namespace grafp {
int cross_match_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                       const int64_t *src_first, int n_src, const int64_t *ids, int k, int top, int min_votes,
                       int min_overlap, void *ws, size_t ws_bytes, int32_t *out_track, int32_t *out_delta,
                       int32_t *out_start, int32_t *out_len, float *out_score, int32_t *out_votes, hipStream_t stream);
int cross_match_pq_launch(const int32_t *list_id, const unsigned char *codes, int64_t n, const float *centroids,
                          int nlist, const float *codebooks, int M, const int64_t *first, int T, const float *q_rows,
                          const int64_t *src_first, int n_src, const int64_t *ids, int k, int top, int min_votes,
                          int min_overlap, void *ws, size_t ws_bytes, int32_t *out_track, int32_t *out_delta,
                          int32_t *out_start, int32_t *out_len, float *out_score, int32_t *out_votes,
                          hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_cross_match_f32(const float *index_rows, int64_t n, const int64_t *track_first_row, int n_tracks,
                                     const float *q_rows, int64_t n_qrows, const int64_t *src_first_row, int n_src,
                                     const int64_t *topk_ids, int k, int top, int min_votes, int min_overlap, void *ws,
                                     size_t ws_bytes, int32_t *out_track, int32_t *out_delta, int32_t *out_start,
                                     int32_t *out_len, float *out_score, int32_t *out_votes, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && q_rows && src_first_row && topk_ids && out_track && out_delta &&
                  out_start && out_len && out_score && out_votes, "cross_match: null pointer");
    const int st = check_cross_match("cross_match", n, nullptr, n_tracks, n_qrows, n_src,
                                     (uintptr_t)index_rows | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::cross_match_launch(index_rows, n, track_first_row, n_tracks, q_rows, src_first_row, n_src, topk_ids,
                                     k, top, min_votes, min_overlap, ws, ws_bytes, out_track, out_delta, out_start,
                                     out_len, out_score, out_votes, (hipStream_t)stream);
}

extern "C" int grafp_cross_match_pq_f32(const int32_t *list_id, const uint8_t *codes, int64_t n, const float *centroids,
                                        int nlist, const float *codebooks, int M, const int64_t *track_first_row,
                                        int n_tracks, const float *q_rows, int64_t n_qrows,
                                        const int64_t *src_first_row, int n_src, const int64_t *topk_ids, int k,
                                        int top, int min_votes, int min_overlap, void *ws, size_t ws_bytes,
                                        int32_t *out_track, int32_t *out_delta, int32_t *out_start, int32_t *out_len,
                                        float *out_score, int32_t *out_votes, grafp_stream_t stream) {
    GRAFP_REQUIRE(list_id && codes && centroids && codebooks && track_first_row && q_rows && src_first_row &&
                  topk_ids && out_track && out_delta && out_start && out_len && out_score && out_votes,
                  "cross_match_pq: null pointer");
    const int st = check_cross_match("cross_match_pq", n, &nlist, n_tracks, n_qrows, n_src,
                                     (uintptr_t)centroids | (uintptr_t)codebooks | (uintptr_t)q_rows,
                                     (uintptr_t)codes | (uintptr_t)list_id);
    if (st != GRAFP_OK) return st;
    return grafp::cross_match_pq_launch(list_id, codes, n, centroids, nlist, codebooks, M, track_first_row, n_tracks,
                                        q_rows, src_first_row, n_src, topk_ids, k, top, min_votes, min_overlap, ws,
                                        ws_bytes, out_track, out_delta, out_start, out_len, out_score, out_votes,
                                        (hipStream_t)stream);
}

// What recordings held outside a library of bf16 rows share with it (crossmatch_half.hip): grafp_cross_match_f32's checks
// here, the kernels there.
namespace grafp {
int cross_match_half_launch(const unsigned short *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                            const int64_t *src_first, int n_src, const int64_t *ids, int k, int top, int min_votes,
                            int min_overlap, void *ws, size_t ws_bytes, int32_t *out_track, int32_t *out_delta,
                            int32_t *out_start, int32_t *out_len, float *out_score, int32_t *out_votes,
                            hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_cross_match_half_f32(const void *index_rows_bf16, int64_t n, const int64_t *track_first_row,
                                          int n_tracks, const float *q_rows, int64_t n_qrows,
                                          const int64_t *src_first_row, int n_src, const int64_t *topk_ids, int k,
                                          int top, int min_votes, int min_overlap, void *ws, size_t ws_bytes,
                                          int32_t *out_track, int32_t *out_delta, int32_t *out_start, int32_t *out_len,
                                          float *out_score, int32_t *out_votes, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows_bf16 && track_first_row && q_rows && src_first_row && topk_ids && out_track && out_delta &&
                  out_start && out_len && out_score && out_votes, "cross_match_half: null pointer");
    const int st = check_cross_match("cross_match_half", n, nullptr, n_tracks, n_qrows, n_src,
                                     (uintptr_t)index_rows_bf16 | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::cross_match_half_launch((const unsigned short *)index_rows_bf16, n, track_first_row, n_tracks, q_rows,
                                          src_first_row, n_src, topk_ids, k, top, min_votes, min_overlap, ws, ws_bytes,
                                          out_track, out_delta, out_start, out_len, out_score, out_votes,
                                          (hipStream_t)stream);
}

// What recordings that play faster or slower than the catalogue share with a library (crossmatch_tempo.hip): the checks
// shared with grafp_cross_match_f32 here; the ratio checks, the workspace floor and the three launches there.
namespace grafp {
int cross_match_tempo_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                             int64_t n_qrows, const int64_t *src_first, int n_src, const int64_t *ids, int k, int top,
                             int min_votes, int min_overlap, const int32_t *ratio_num, int n_ratios, void *ws,
                             size_t ws_bytes, int32_t *out_track, int32_t *out_delta, int32_t *out_start,
                             int32_t *out_len, float *out_score, int32_t *out_votes, int32_t *out_ratio,
                             hipStream_t stream);
size_t cross_match_tempo_workspace(const int64_t *src_rows, int n_src, int k, int min_votes, int n_ratios, int top);
}  // namespace grafp

extern "C" size_t grafp_cross_match_tempo_workspace(const int64_t *src_rows, int n_src, int k, int min_votes,
                                                    int n_ratios, int top) {
    return grafp::cross_match_tempo_workspace(src_rows, n_src, k, min_votes, n_ratios, top);
}

extern "C" int grafp_cross_match_tempo_f32(const float *index_rows, int64_t n, const int64_t *track_first_row,
                                           int n_tracks, const float *q_rows, int64_t n_qrows,
                                           const int64_t *src_first_row, int n_src, const int64_t *topk_ids, int k,
                                           int top, int min_votes, int min_overlap, const int32_t *ratio_num,
                                           int n_ratios, void *ws, size_t ws_bytes, int32_t *out_track,
                                           int32_t *out_delta, int32_t *out_start, int32_t *out_len, float *out_score,
                                           int32_t *out_votes, int32_t *out_ratio, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && q_rows && src_first_row && topk_ids && ratio_num && out_track &&
                  out_delta && out_start && out_len && out_score && out_votes && out_ratio,
                  "cross_match_tempo: null pointer");
    const int st = check_cross_match("cross_match_tempo", n, nullptr, n_tracks, n_qrows, n_src,
                                     (uintptr_t)index_rows | (uintptr_t)q_rows, 0);
    if (st != GRAFP_OK) return st;
    return grafp::cross_match_tempo_launch(index_rows, n, track_first_row, n_tracks, q_rows, n_qrows, src_first_row,
                                           n_src, topk_ids, k, top, min_votes, min_overlap, ratio_num, n_ratios, ws,
                                           ws_bytes, out_track, out_delta, out_start, out_len, out_score, out_votes,
                                           out_ratio, (hipStream_t)stream);
}

// Tracks that share audio at another speed inside a library (selfmatch_tempo.hip): the checks of grafp_self_match_f32
// here; the ratio checks, the workspace floor and the three launches there.
namespace grafp {
int self_match_tempo_launch(const float *rows, int64_t n, const int64_t *first, int T, const int64_t *ids, int k,
                            const int *tracks, int n_src, int top, int min_votes, int min_overlap,
                            const int32_t *ratio_num, int n_ratios, void *ws, size_t ws_bytes, int32_t *out_track,
                            int32_t *out_delta, int32_t *out_start, int32_t *out_len, float *out_score,
                            int32_t *out_votes, int32_t *out_ratio, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_self_match_tempo_f32(const float *index_rows, int64_t n, const int64_t *track_first_row,
                                          int n_tracks, const int64_t *topk_ids, int k, const int *src_tracks, int n_src,
                                          int top, int min_votes, int min_overlap, const int32_t *ratio_num,
                                          int n_ratios, void *ws, size_t ws_bytes, int32_t *out_track,
                                          int32_t *out_delta, int32_t *out_start, int32_t *out_len, float *out_score,
                                          int32_t *out_votes, int32_t *out_ratio, grafp_stream_t stream) {
    GRAFP_REQUIRE(index_rows && track_first_row && topk_ids && src_tracks && ratio_num && out_track && out_delta &&
                  out_start && out_len && out_score && out_votes && out_ratio, "self_match_tempo: null pointer");
    GRAFP_REQUIRE(n >= 1 && n < 0x7fffff00ll && n_tracks >= 1 && n_src >= 0,
                  "self_match_tempo: bad sizes n=%lld n_tracks=%d n_src=%d", (long long)n, n_tracks, n_src);
    GRAFP_REQUIRE(((uintptr_t)index_rows & 15) == 0, "self_match_tempo: rows must be 16-byte aligned");
    return grafp::self_match_tempo_launch(index_rows, n, track_first_row, n_tracks, topk_ids, k, src_tracks, n_src, top,
                                          min_votes, min_overlap, ratio_num, n_ratios, ws, ws_bytes, out_track,
                                          out_delta, out_start, out_len, out_score, out_votes, out_ratio,
                                          (hipStream_t)stream);
}

// The merge of the lists that the shards of a library return for the same items (merge_lists.hip): the limits, the host
// tables and the launch are all there.
namespace grafp {
int merge_track_lists_launch(const int32_t *track, const float *score, const int32_t *payload, int n_lists, int n_items,
                             int top, int n_payload, const int32_t *track_base, const int32_t *pad, int32_t *out_track,
                             float *out_score, int32_t *out_payload, hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_merge_track_lists_f32(const int32_t *track, const float *score, const int32_t *payload, int n_lists,
                                           int n_items, int top, int n_payload, const int32_t *track_base,
                                           const int32_t *pad, int32_t *out_track, float *out_score,
                                           int32_t *out_payload, grafp_stream_t stream) {
    return grafp::merge_track_lists_launch(track, score, payload, n_lists, n_items, top, n_payload, track_base, pad,
                                           out_track, out_score, out_payload, (hipStream_t)stream);
}

// The front end of live multi-channel monitoring (stream_frontend.hip): argument checks here, the kernels there.  The
// per-channel tables are device data: the caller (ops.stream_logmel) checks them on the host before it uploads them.
namespace grafp {
int stream_logmel_launch(const float *bank, const int64_t *buf_start, const int32_t *buf_len, const int64_t *buf_base,
                         const int64_t *frame_lo, const int64_t *frame_hi, const int32_t *group_first, int n_channels,
                         int n_groups, int hop, int n_mels, int ring_len, const float *window, const float *twiddle,
                         const float *fb, const int32_t *band_lo, const int32_t *band_hi, float *ring,
                         hipStream_t stream);
int stream_segments_launch(const float *ring, const int64_t *seg_lo, const int32_t *seg_first, int n_channels,
                           int n_segments, int n_mels, int ring_len, int size, int step, float *seg,
                           hipStream_t stream);
}  // namespace grafp

extern "C" int grafp_stream_logmel_f32(const float *bank, const int64_t *buf_start, const int32_t *buf_len,
                                       const int64_t *buf_base, const int64_t *frame_lo, const int64_t *frame_hi,
                                       const int32_t *group_first, int n_channels, int n_groups, int n_fft, int hop,
                                       int n_mels, int ring_len, const float *window, const float *twiddle,
                                       const float *fb, const int32_t *band_lo, const int32_t *band_hi, float *ring,
                                       grafp_stream_t stream) {
    GRAFP_REQUIRE(bank && buf_start && buf_len && buf_base && frame_lo && frame_hi && group_first && window && twiddle &&
                  fb && band_lo && band_hi && ring, "stream_logmel: null pointer");
    GRAFP_REQUIRE(n_fft == 1024 && n_mels >= 1 && n_mels <= 64,
                  "stream_logmel: only n_fft=1024 and n_mels<=64 are supported (got %d and %d)", n_fft, n_mels);
    GRAFP_REQUIRE(n_channels >= 1 && n_groups >= 0 && hop >= 1, "stream_logmel: bad n_channels=%d n_groups=%d hop=%d",
                  n_channels, n_groups, hop);
    GRAFP_REQUIRE(ring_len >= 2 && (ring_len & (ring_len - 1)) == 0,
                  "stream_logmel: ring_len=%d is no power of two >= 2", ring_len);
    if (n_groups == 0) return GRAFP_OK;
    return grafp::stream_logmel_launch(bank, buf_start, buf_len, buf_base, frame_lo, frame_hi, group_first, n_channels,
                                       n_groups, hop, n_mels, ring_len, window, twiddle, fb, band_lo, band_hi, ring,
                                       (hipStream_t)stream);
}

extern "C" int grafp_stream_segments_f32(const float *ring, const int64_t *seg_lo, const int32_t *seg_first,
                                         int n_channels, int n_segments, int n_mels, int ring_len, int size, int step,
                                         float *seg, grafp_stream_t stream) {
    GRAFP_REQUIRE(ring && seg_lo && seg_first && seg, "stream_segments: null pointer");
    GRAFP_REQUIRE(n_channels >= 1 && n_segments >= 0 && n_mels >= 1 && size >= 1 && step >= 1,
                  "stream_segments: bad n_channels=%d n_segments=%d n_mels=%d size=%d step=%d", n_channels, n_segments,
                  n_mels, size, step);
    GRAFP_REQUIRE(ring_len >= size && (ring_len & (ring_len - 1)) == 0,
                  "stream_segments: ring_len=%d is no power of two >= size=%d", ring_len, size);
    if (n_segments == 0) return GRAFP_OK;
    return grafp::stream_segments_launch(ring, seg_lo, seg_first, n_channels, n_segments, n_mels, ring_len, size, step,
                                         seg, (hipStream_t)stream);
}
