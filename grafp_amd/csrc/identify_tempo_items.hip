// identify_tempo_items.hip -- identify_tempo.hip with a ratio window per item (ops.identify_tempo_items; the tempo lock
// of grafp_amd/monitor.py's StreamMonitor), gfx950.
//
// The call names one ascending grid of R <= 64 ratios, as identify_tempo.hip does, and item i is identified over
// ratio_num[lo_i : lo_i + cnt_i] only, 1 <= cnt_i, 0 <= lo_i, lo_i + cnt_i <= R.  Row i of the five outputs is, bit for
// bit, row 0 of identify_tempo.hip called with item i alone and that sub-list of ratios: the candidates, eligibility,
// scores and the tie rule (the ratio nearer to 1, then the smaller num, then the smaller alignment) stated at the top of
// identify_tempo.hip, applied among the item's own ratios.  With every cnt_i = R it is identify_tempo.hip's launch.
//
// The host lays the windows out as a WORK TABLE: n_work = sum of cnt_i entries (item, ratio index) of two int32, ordered
// by item and then by ratio, and the exclusive scan item_scan (n_items + 1 int32) of the cnt_i; both on the device.
// Pass 1, identify_tempo_items_kernel, grid (n_work): workgroup w reads its entry and runs identify_core.h's
// identify_item for that (item, ratio) on TempoGrid with TempoRowSpan, exactly the work of one workgroup of
// identify_tempo_kernel; its `top` list is row w of the workspace, four (n_work, top) arrays of 4 bytes, 16 bytes per entry
// in all.  An entry whose item is outside [0, n_items) or whose ratio index is outside [0, R) is skipped by a compare: its
// list is empty and nothing else is read.
// Pass 2, identify_tempo_items_merge_kernel, one workgroup per item: identify_tempo_merge_kernel's merge of the item's
// cnt_i lists [item_scan[i], item_scan[i + 1]), the preference ranks taken over the item's own ratios, in
// merge_slots(cnt_i, top) slots (the launch reserves those of max_cnt, the caller's largest cnt_i).  The merge is stated
// a second time here: moved into a header it compiles identify_tempo_merge_kernel to other code.
// A scan or a window out of range (a count outside [1, max_cnt], lists outside [0, n_work), ratios outside [0, R)) gives
// an empty row instead of a read.
// Both passes go out on the caller's stream with no host synchronisation.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as identify_tempo.hip.
#include "identify_core.h"
#include "span_rows.h"

namespace grafp {

// row pairs in flight in the score loop: query rows in LDS / in global memory (identify_tempo.hip's counts)
constexpr int IDI_UNROLL_QLDS = 4, IDI_UNROLL_QGLOBAL = 1;

template <bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_tempo_items_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, TempoRatios ratios, int R,
    const int32_t *__restrict__ work, int n_items, const float *__restrict__ q_rows, const int64_t *__restrict__ ids,
    int k, const int64_t *__restrict__ item_row, const int *__restrict__ item_len, int max_len, int Pmax, int top,
    int min_overlap, int32_t *__restrict__ ws_track, int32_t *__restrict__ ws_offset, float *__restrict__ ws_score,
    int32_t *__restrict__ ws_votes) {
    const int w = blockIdx.x;
    const int item = work[2 * (size_t)w], j = work[2 * (size_t)w + 1];       // (the same in every thread)
    if (item < 0 || item >= n_items || j < 0 || j >= R) {
        if ((int)threadIdx.x < top) {
            const size_t o = (size_t)w * top + threadIdx.x;
            ws_track[o] = -1;
            ws_offset[o] = INT_MIN;
            ws_score[o] = -INFINITY;
            ws_votes[o] = 0;
        }
        return;
    }
    const TempoRowSpan<kQLds ? IDI_UNROLL_QLDS : IDI_UNROLL_QGLOBAL> span{reinterpret_cast<const float4 *>(rows)};
    identify_item<kQLds>(TempoGrid{ratios.num[j]}, span, n, first, T, q_rows, ids, k, item_row, item_len, max_len, Pmax,
                         top, min_overlap, ws_track, ws_offset, ws_score, ws_votes, item, w);
}

__global__ __launch_bounds__(ID_THREADS) void identify_tempo_items_merge_kernel(
    TempoRatios ratios, int n_ratios, int max_cnt, int top, const int32_t *__restrict__ work,
    const int32_t *__restrict__ item_scan, int n_work, const int32_t *__restrict__ ws_track,
    const int32_t *__restrict__ ws_offset, const float *__restrict__ ws_score, const int32_t *__restrict__ ws_votes,
    int32_t *__restrict__ out_track, int32_t *__restrict__ out_offset, float *__restrict__ out_score,
    int32_t *__restrict__ out_votes, int32_t *__restrict__ out_ratio) {
    const int item = blockIdx.x, tid = threadIdx.x;
    const int b = item_scan[item], cnt = item_scan[item + 1] - b;
    bool ok = b >= 0 && cnt >= 1 && cnt <= max_cnt && b <= n_work - cnt;    // (max_cnt <= R <= 64: no overflow)
    const int lo = ok ? work[2 * (size_t)b + 1] : 0;
    ok = ok && lo >= 0 && lo <= n_ratios - cnt;
    if (!ok) {
        if (tid < top) {
            const size_t o = (size_t)item * top + tid;
            out_track[o] = -1;
            out_offset[o] = INT_MIN;
            out_score[o] = -INFINITY;
            out_votes[o] = 0;
            out_ratio[o] = 0;
        }
        return;
    }
    // identify_tempo_merge_kernel's merge from here on, with R = cnt, ratio j = ratios.num[lo + j], list j = row b + j
    const int R = cnt;
    extern __shared__ __attribute__((aligned(16))) unsigned char idr_smem[];      // 10 * P bytes (the launch's P)
    __shared__ int order[SEQ_MAX_RATIOS];                 // order[p]: the ratio of preference rank p
    const int total = R * top;
    const int P = merge_slots(R, top);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(idr_smem);
    unsigned short *idx = reinterpret_cast<unsigned short *>(idr_smem + (size_t)8 * P);
    if (tid < R) {
        const int num = ratios.num[lo + tid], d = num < SEQ_TEMPO_DEN ? SEQ_TEMPO_DEN - num : num - SEQ_TEMPO_DEN;
        int rank = 0;
        for (int j = 0; j < R; ++j) {
            const int nj = ratios.num[lo + j], dj = nj < SEQ_TEMPO_DEN ? SEQ_TEMPO_DEN - nj : nj - SEQ_TEMPO_DEN;
            rank += (dj < d || (dj == d && nj < num)) ? 1 : 0;         // (the ratios are distinct)
        }
        order[rank] = tid;
    }
    __syncthreads();
    // the ws entry of merge slot e < total
    auto entry = [&](int e) -> size_t {
        const int p = e / top;
        return (size_t)(b + order[p]) * top + (e - p * top);
    };
    for (int e = tid; e < P; e += ID_THREADS) {
        unsigned long long key = SEQ_NONE;
        if (e < total) {
            const size_t w = entry(e);
            const int t = ws_track[w];
            if (t >= 0) key = ((unsigned long long)t << 32) | ~f32_ord(ws_score[w]);
        }
        keys[e] = key;
        idx[e] = (unsigned short)e;
    }
    __syncthreads();
    // best entry per track (P / 256 <= 16 slots per thread: one mask bit each)
    block_sort<ID_THREADS, true>(keys, idx, P, tid);
    unsigned int head = 0;
    for (int e = tid, it = 0; e < P; e += ID_THREADS, ++it) {
        const unsigned long long key = keys[e];
        if (key != SEQ_NONE && (e == 0 || (keys[e - 1] >> 32) != (key >> 32))) head |= 1u << it;
    }
    __syncthreads();
    for (int e = tid, it = 0; e < P; e += ID_THREADS, ++it) {
        const unsigned long long key = keys[e];
        keys[e] = ((head >> it) & 1u) ? ((key << 32) | (key >> 32)) : SEQ_NONE;
    }
    __syncthreads();
    // the `top` tracks: score descending, track ascending
    block_sort<ID_THREADS, true>(keys, idx, P, tid);
    if (tid < top) {
        const unsigned long long key = keys[tid];          // top <= 64 <= P
        const size_t o = (size_t)item * top + tid;
        if (key != SEQ_NONE) {
            const int e = idx[tid];
            const size_t w = entry(e);
            out_track[o] = (int)(key & 0xffffffffull);
            out_offset[o] = ws_offset[w];
            out_score[o] = ord_f32(~(unsigned int)(key >> 32));
            out_votes[o] = ws_votes[w];
            out_ratio[o] = ratios.num[lo + order[e / top]];
        } else {
            out_track[o] = -1;
            out_offset[o] = INT_MIN;
            out_score[o] = -INFINITY;
            out_votes[o] = 0;
            out_ratio[o] = 0;
        }
    }
}

size_t identify_tempo_items_workspace(int n_work, int top) {
    if (n_work < 0 || top < 1 || top > 64) return 0;
    return (size_t)16 * n_work * top;
}

int identify_tempo_items_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                                const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items,
                                int max_len, int top, int min_overlap, const int32_t *ratio_num, int n_ratios,
                                const int32_t *work, int n_work, const int32_t *item_scan, int max_cnt, void *ws,
                                int32_t *out_track, int32_t *out_offset, float *out_score, int32_t *out_votes,
                                int32_t *out_ratio, hipStream_t stream) {
    TempoRatios ratios;
    int st = tempo_ratios("identify_tempo_items", ratio_num, n_ratios, ratios);
    if (st != GRAFP_OK) return st;
    GRAFP_REQUIRE(n + ID_TEMPO_SHIFT < (1ll << 32),
                  "identify_tempo_items: n=%lld rows reach past the 2^32 alignments of a key", (long long)n);
    GRAFP_REQUIRE(max_cnt >= 1 && max_cnt <= n_ratios, "identify_tempo_items: max_cnt=%d not in [1, n_ratios=%d]", max_cnt,
                  n_ratios);
    GRAFP_REQUIRE(n_work >= n_items && (int64_t)n_work <= (int64_t)n_items * max_cnt,
                  "identify_tempo_items: n_work=%d is not between n_items=%d and n_items * max_cnt=%lld", n_work, n_items,
                  (long long)n_items * max_cnt);
    st = id_check_launch("identify_tempo_items", max_len, k);
    if (st != GRAFP_OK || n_items == 0) return st;
    GRAFP_REQUIRE(work && item_scan, "identify_tempo_items: null pointer");
    GRAFP_REQUIRE(ws && ((uintptr_t)ws & 15) == 0,
                  "identify_tempo_items: the workspace is missing or not 16-byte aligned");
    const size_t lists = (size_t)n_work * top;
    int32_t *ws_track = reinterpret_cast<int32_t *>(ws), *ws_offset = ws_track + lists;
    float *ws_score = reinterpret_cast<float *>(ws_offset + lists);
    int32_t *ws_votes = reinterpret_cast<int32_t *>(ws_score + lists);
    const IdentifyPlan plan = identify_plan(max_len, k);
    st = id_launch("identify_tempo_items", identify_tempo_items_kernel<true>, identify_tempo_items_kernel<false>, plan,
                   dim3(n_work), stream, rows, n, first, T, ratios, n_ratios, work, n_items, q_rows, ids, k, item_row,
                   item_len, max_len, plan.Pmax, top, min_overlap, ws_track, ws_offset, ws_score, ws_votes);
    if (st != GRAFP_OK) return st;
    hipLaunchKernelGGL(identify_tempo_items_merge_kernel, dim3(n_items), dim3(ID_THREADS),
                       (size_t)10 * merge_slots(max_cnt, top), stream, ratios, n_ratios, max_cnt, top, work, item_scan,
                       n_work, ws_track, ws_offset, ws_score, ws_votes, out_track, out_offset, out_score, out_votes,
                       out_ratio);
    GRAFP_CHECK_LAUNCH("identify_tempo_items_merge_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
