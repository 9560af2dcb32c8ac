// identify_core.h -- the one body of the track-aware identification kernels: identify.hip (library rows held as f32),
// identify_pq.hip (library rows held as IVF-PQ codes, decoded while they are scored) and identify_thin.hip (f32 rows,
// every D-th row of each track kept).  What the kernels compute, the LDS layout and the five phases are stated at the
// top of identify.hip; the arithmetic order of a score at the top of seqmatch.h.  The dense kernels differ in ONE thing:
// where y[t] of the span sum (phase 3) comes from.  That is the Span parameter of identify_item:
//     float span(const float4 *x, int64_t row, int l, int m)
// x: lane l's float4 of the first query row of the span, row: the library row that pairs with it, m: pairs (the same in
// every lane of the half-wave; <= 0: no row is read, the butterfly still runs).  It returns the un-divided span score in
// span_sum's order.  Rows [row, row + m) lie inside [0, n).
// The library rows sit on a ROW GRID, the Grid parameter of identify_item: which fine position (dense segment, counted
// over the whole library) a row holds, and so which query rows of an alignment pair with which library rows.
//     int64_t fine(int64_t r)    the fine position of library row r (and of a track's first row)
//     int64_t row(int64_t p)     the library row at fine position p = a + s of a pair (p >= 0, on the grid)
//     int need(int need_q)       the pairs a candidate needs, from the query rows the caller asks for
//     void pairs(a, f0, f1, ql, lo, o)   the pairs of alignment a with the track of rows [f0, f1): query rows
//                                lo, lo + step, ... (o of them; o < 1: none), library rows row(a + lo), + 1, ...
//   DenseGrid   one row per fine position (identify.hip, identify_pq.hip): a = r - s, pairs are consecutive rows
//   ThinGrid    every D-th position of each track is kept (identify_thin.hip): a = r * D - s, the query steps D rows
//               per pair and the library one (the Span functor carries the query step)
// A grid also says where the query rows sit, for a recording that does not run at the catalogue's speed:
//     int at(int s)              rows after query row 0 at which query row s sits (s on the two grids above)
//     int shift()                the key shift: fine(r) - at(s) + shift() >= 0 for every hit
//     int64_t cap(int64_t L)     the pairs a track of L rows can always hold (caps need in the eligibility rule)
//     float score(span, q4, a, lo, l, m)   the span call of phase 3: m pairs from query row lo on
//   TempoGrid   one row per fine position, query row s sits w(s) = (s * num + 128) >> 8 rows after row 0
//               (identify_tempo.hip): a = r - w(s), the library rows of the pairs are gathered (TempoRowSpan)
//   StrideGrid  one row per fine position, the item holds every Q-th segment of the recording: query row s sits s * Q
//               rows after row 0 (identify_stride.hip): a = r - s * Q, the library steps Q rows per pair (StepRowSpan)
// Compiles with and without the packed-f32 instructions; every user is built without (Makefile NOPK).
#pragma once
#include <limits.h>
#include <math.h>

#include "common.h"
#include "seqmatch.h"

namespace grafp {

constexpr int ID_THREADS = 256;
constexpr int ID_MAX_LEN = 256;
constexpr int ID_MAX_K = 32;
constexpr int ID_MAX_KEYS = 8192;
constexpr int ID_SHIFT = ID_MAX_LEN - 1;                 // a + ID_SHIFT >= 0 for every hit
constexpr int ID_TEMPO_SHIFT = 511;                      // TempoGrid: w(255) = 510 at num = SEQ_TEMPO_MAX
constexpr int ID_MAX_STRIDE = 32;                        // ThinGrid: the largest row stride
constexpr int ID_MAX_QUERY_STRIDE = 32;                  // StrideGrid: the largest query stride
constexpr size_t ID_LDS = 160 * 1024 - 256;      // dynamic LDS budget (the static s_ncand sits next to it)

// The launch plan of one identify kernel: slots per item, dynamic LDS bytes, and whether the query rows sit in LDS.
struct IdentifyPlan {
    int Pmax;
    size_t lds;
    bool q_lds;
};
inline IdentifyPlan identify_plan(int max_len, int k) {
    IdentifyPlan p;
    p.Pmax = 64;
    while (p.Pmax < max_len * k) p.Pmax <<= 1;
    const size_t slots = (size_t)16 * p.Pmax, qbytes = (size_t)max_len * SEQ_D * sizeof(float);
    p.q_lds = slots + qbytes <= ID_LDS;
    p.lds = p.q_lds ? slots + qbytes : slots;
    return p;
}

// the limit check every identify launch shares (name: the operation, for the message)
inline int id_check_launch(const char *name, int max_len, int k) {
    GRAFP_REQUIRE(max_len >= 1 && max_len <= ID_MAX_LEN && k >= 1 && k <= ID_MAX_K && max_len * k <= ID_MAX_KEYS,
                  "%s: max_len=%d k=%d exceed %d segments, %d hits per segment or %d keys per item", name, max_len, k,
                  ID_MAX_LEN, ID_MAX_K, ID_MAX_KEYS);
    return GRAFP_OK;
}

// reserves the plan's dynamic LDS for the kernel the plan chooses (query rows in LDS / in global memory) and launches it
// on `grid` (blockIdx.x = the item); the caller places plan.Pmax among args where the kernel expects it
template <typename... Params, typename... Args>
inline int id_launch(const char *name, void (*kernel_q_lds)(Params...), void (*kernel_q_global)(Params...),
                     const IdentifyPlan &plan, dim3 grid, hipStream_t stream, Args... args) {
    return seq_launch(name, plan.q_lds ? kernel_q_lds : kernel_q_global, grid, ID_THREADS, plan.lds, stream, args...);
}

struct DenseGrid {
    __device__ __forceinline__ int64_t fine(int64_t r) const { return r; }
    __device__ __forceinline__ int64_t row(int64_t p) const { return p; }
    __device__ __forceinline__ int need(int need_q) const { return need_q; }
    __device__ __forceinline__ void pairs(int64_t a, int64_t f0, int64_t f1, int ql, int &lo, int &o) const {
        lo = (int)(f0 - a > 0 ? f0 - a : 0);
        const int hi = (int)(f1 - a < ql ? f1 - a : ql);
        o = hi - lo;
    }
    __device__ __forceinline__ int at(int s) const { return s; }
    __device__ __forceinline__ int shift() const { return ID_SHIFT; }
    __device__ __forceinline__ int64_t cap(int64_t L) const { return L; }
    template <typename Span>
    __device__ __forceinline__ float score(const Span &span, const float4 *q4, int64_t a, int lo, int l, int m) const {
        return span(q4 + lo * (SEQ_D / 4) + l, row(a + lo), l, m);
    }
};

// Every D-th fine position of each track, D in [1, ID_MAX_STRIDE]; the host keeps n * D + ID_SHIFT below 2^32, so
// fine(r) - s + ID_SHIFT fits the upper half of a key.  Query row s pairs with a row of the track iff (a + s) mod D == 0
// (mathematical mod: a may be negative) and f0 <= (a + s) / D < f1; everything is compared in 64 bits before it is
// narrowed, so that a table the caller vouched for wrongly yields no pairs instead of a query row outside the item.
struct ThinGrid {
    int D;
    __device__ __forceinline__ int64_t fine(int64_t r) const { return r * D; }
    __device__ __forceinline__ int64_t row(int64_t p) const { return p / D; }
    __device__ __forceinline__ int need(int need_q) const { return need_q / D > 1 ? need_q / D : 1; }
    __device__ __forceinline__ void pairs(int64_t a, int64_t f0, int64_t f1, int ql, int &lo, int &o) const {
        const int64_t s0 = ((-a) % D + D) % D;             // the first s >= 0 on the grid
        const int64_t sf = f0 * D - a;                     // the s of the track's first row (on the grid too)
        const int64_t lo64 = sf > s0 ? sf : s0;
        const int64_t end = (f1 - 1) * D - a + 1;          // one past the s of the track's last row
        const int64_t hi64 = end < ql ? end : ql;
        const bool any = hi64 > lo64;                      // then 0 <= lo64 < hi64 <= ql
        lo = any ? (int)lo64 : 0;
        o = any ? (int)((hi64 - lo64 + D - 1) / D) : 0;
    }
    __device__ __forceinline__ int at(int s) const { return s; }
    __device__ __forceinline__ int shift() const { return ID_SHIFT; }
    __device__ __forceinline__ int64_t cap(int64_t L) const { return L; }
    template <typename Span>
    __device__ __forceinline__ float score(const Span &span, const float4 *q4, int64_t a, int lo, int l, int m) const {
        return span(q4 + lo * (SEQ_D / 4) + l, row(a + lo), l, m);
    }
};

// One row per fine position; the recording runs at num / 256 of the catalogue's speed, so query row s sits
// w(s) = (s * num + 128) >> 8 rows after query row 0 (num in [SEQ_TEMPO_MIN, SEQ_TEMPO_MAX]; w(s) <= 510 for s <= 255).
// w never decreases, so the pairs of an alignment are a contiguous range of s: w(s) >= x iff s * num + 128 >= 256 * x.
// The host keeps n + ID_TEMPO_SHIFT below 2^32.  Its Span gathers: span(x, a, lo, num, l, m) reads row a + w(lo + t).
struct TempoGrid {
    int num;
    __device__ __forceinline__ int64_t fine(int64_t r) const { return r; }
    __device__ __forceinline__ int64_t row(int64_t p) const { return p; }
    __device__ __forceinline__ int need(int need_q) const { return need_q; }
    __device__ __forceinline__ int at(int s) const { return (s * num + SEQ_TEMPO_DEN / 2) >> 8; }
    __device__ __forceinline__ int shift() const { return ID_TEMPO_SHIFT; }
    __device__ __forceinline__ int64_t cap(int64_t L) const {
        const int64_t c = L * SEQ_TEMPO_DEN / num;
        return c > 1 ? c : 1;
    }
    // the first s in [0, ql] with w(s) >= x (ql: none)
    __device__ __forceinline__ int first_at(int64_t x, int ql) const {
        if (x <= 0) return 0;
        const int64_t s = (x * SEQ_TEMPO_DEN - SEQ_TEMPO_DEN / 2 + num - 1) / num;
        return s < ql ? (int)s : ql;
    }
    __device__ __forceinline__ void pairs(int64_t a, int64_t f0, int64_t f1, int ql, int &lo, int &o) const {
        lo = first_at(f0 - a, ql);
        o = first_at(f1 - a, ql) - lo;
    }
    template <typename Span>
    __device__ __forceinline__ float score(const Span &span, const float4 *q4, int64_t a, int lo, int l, int m) const {
        return span(q4 + lo * (SEQ_D / 4) + l, a, lo, num, l, m);
    }
};

// One row per fine position; the item's rows are every Q-th segment of the recording, Q in [1, ID_MAX_QUERY_STRIDE], so
// query row s sits s * Q rows after query row 0 (TempoGrid's w at num = 256 * Q, exactly) and a = r - s * Q.  The pairs
// of an alignment are a contiguous range of s: s * Q >= x iff s >= ceil(x / Q).  The host keeps n + shift() below 2^32.
// Everything is compared in 64 bits before it is narrowed (as ThinGrid): a table the caller vouched for wrongly yields
// no pairs instead of a query row outside the item.  Its Span steps the library Q rows per pair (StepRowSpan).
struct StrideGrid {
    int Q;
    __device__ __forceinline__ int64_t fine(int64_t r) const { return r; }
    __device__ __forceinline__ int64_t row(int64_t p) const { return p; }
    __device__ __forceinline__ int need(int need_q) const { return need_q; }
    __device__ __forceinline__ int at(int s) const { return s * Q; }
    __device__ __forceinline__ int shift() const { return (ID_MAX_LEN - 1) * Q; }
    __device__ __forceinline__ int64_t cap(int64_t L) const { return L / Q > 1 ? L / Q : 1; }
    // the first s in [0, ql] with s * Q >= x (ql: none)
    __device__ __forceinline__ int first_at(int64_t x, int ql) const {
        if (x <= 0) return 0;
        const int64_t s = (x + Q - 1) / Q;
        return s < ql ? (int)s : ql;
    }
    __device__ __forceinline__ void pairs(int64_t a, int64_t f0, int64_t f1, int ql, int &lo, int &o) const {
        lo = first_at(f0 - a, ql);
        o = first_at(f1 - a, ql) - lo;
    }
    template <typename Span>
    __device__ __forceinline__ float score(const Span &span, const float4 *q4, int64_t a, int lo, int l, int m) const {
        return span(q4 + lo * (SEQ_D / 4) + l, a + (int64_t)lo * Q, l, m);
    }
};

// One item by one workgroup of ID_THREADS threads (blockIdx.x = the item); the four outputs are (gridDim.x, top).
// identify_tempo_items.hip, whose workgroups take (item, ratio) entries from a work table, names the two indices itself:
// `item` indexes item_row / item_len, `list` is the row of the four (lists, top) outputs that takes the result.
template <bool kQLds, typename Grid, typename Span>
__device__ __forceinline__ void identify_item(
    const Grid &grid, const Span &span, int64_t n, const int64_t *__restrict__ first, int T,
    const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k, const int64_t *__restrict__ item_row,
    const int *__restrict__ item_len, int max_len, int Pmax, int top, int min_overlap, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_offset, float *__restrict__ out_score, int32_t *__restrict__ out_votes,
    const int item = blockIdx.x, const int list = blockIdx.x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char id_smem[];
    __shared__ int s_ncand;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(id_smem);
    unsigned int *aux = reinterpret_cast<unsigned int *>(id_smem + (size_t)8 * Pmax);
    unsigned short *votes = reinterpret_cast<unsigned short *>(id_smem + (size_t)12 * Pmax);
    unsigned short *idx = reinterpret_cast<unsigned short *>(id_smem + (size_t)14 * Pmax);
    float *sq = reinterpret_cast<float *>(id_smem + (size_t)16 * Pmax);

    const int tid = threadIdx.x;
    const int64_t r0 = item_row[item];
    int ql = item_len[item] < max_len ? item_len[item] : max_len;
    if (ql < 0) ql = 0;
    const int total = ql * k;
    int P = 64;
    while (P < total) P <<= 1;                             // <= Pmax (host: max_len * k <= ID_MAX_KEYS)
    if (tid == 0) s_ncand = 0;
    if (kQLds) {
        const float4 *src = reinterpret_cast<const float4 *>(q_rows + r0 * SEQ_D);
        float4 *dst = reinterpret_cast<float4 *>(sq);
        for (int i = tid; i < ql * (SEQ_D / 4); i += ID_THREADS) dst[i] = src[i];
    }
    // 1. hit keys; ids outside [0, n) are no hits
    for (int e = tid; e < P; e += ID_THREADS) {
        unsigned long long key = SEQ_NONE;
        if (e < total) {
            const int s = e / k;
            const int64_t r = ids[(r0 + s) * k + (e - s * k)];
            if (r >= 0 && r < n) key = ((unsigned long long)(grid.fine(r) - grid.at(s) + grid.shift()) << 32) | (unsigned int)s;
        }
        keys[e] = key;
    }
    __syncthreads();
    block_sort<ID_THREADS, false>(keys, nullptr, P, tid);

    // 2. one walker per alignment run (P / 256 <= 32 slots per thread: one mask bit each)
    unsigned int head = 0;
    for (int e = tid, it = 0; e < P; e += ID_THREADS, ++it) {
        const unsigned long long key = keys[e];
        if (key != SEQ_NONE && (e == 0 || (keys[e - 1] >> 32) != (key >> 32))) head |= 1u << it;
    }
    __syncthreads();
    for (int e = tid, it = 0; e < P; e += ID_THREADS, ++it) {
        if (!((head >> it) & 1u)) continue;
        const unsigned long long hi = keys[e] >> 32;
        const int64_t a = (int64_t)hi - grid.shift();
        int start = e, nv = 0, t = 0;
        int64_t end = -1;
        for (int f = e; f < P; ++f) {
            const unsigned long long key = keys[f];
            if ((key >> 32) != hi) break;                   // the next run, or the empty tail
            const int64_t r = grid.row(a + grid.at((int)(unsigned int)key));
            if (r >= end) {                                 // first hit, or the run crossed into a later track
                if (nv) {
                    keys[start] = hi << 32;
                    aux[start] = (unsigned int)t;
                    votes[start] = (unsigned short)nv;
                }
                t = track_of(first, end < 0 ? 0 : (t + 1 < T ? t + 1 : T - 1), T, r);   // (clamp: bad tables)
                end = first[t + 1];
                start = f;
                nv = 0;
            }
            if (f != start) keys[f] = SEQ_NONE;
            ++nv;
        }
        keys[start] = hi << 32;
        aux[start] = (unsigned int)t;
        votes[start] = (unsigned short)nv;
    }
    __syncthreads();
    for (int e = tid; e < P; e += ID_THREADS)
        if (keys[e] != SEQ_NONE) idx[atomicAdd(&s_ncand, 1)] = (unsigned short)e;
    __syncthreads();
    const int ncand = s_ncand;

    // 3. scores: one candidate per half-wave at a time
    const int hw = tid >> 5, l = tid & 31;
    const int need = grid.need(min_overlap > 0 ? min_overlap : ql);
    const float4 *q4 = kQLds ? reinterpret_cast<const float4 *>(sq) : reinterpret_cast<const float4 *>(q_rows + r0 * SEQ_D);
    for (int c = hw; c < ncand; c += ID_THREADS / 32) {
        const int e = idx[c];
        const int64_t a = (int64_t)(keys[e] >> 32) - grid.shift();
        const int t = (int)aux[e];
        int64_t f0 = first[t], f1 = first[t + 1];
        f0 = f0 < 0 ? 0 : f0;                               // (a valid table needs neither clamp)
        f1 = f1 > n ? n : f1;
        const int64_t L = f1 - f0;
        int lo, o;
        grid.pairs(a, f0, f1, ql, lo, o);
        const int64_t cap = grid.cap(L);
        const bool ok = o >= 1 && o >= (need < cap ? need : cap);
        const float acc = grid.score(span, q4, a, lo, l, ok ? o : 0);                         // (not ok: nothing read)
        const float score = acc / (float)o;
        // every lane of the half-wave has read keys[e] and aux[e] before the shuffles above
        if (l == 0) {
            keys[e] = ok ? (((unsigned long long)t << 32) | ~f32_ord(score)) : SEQ_NONE;
            aux[e] = (unsigned int)(a + grid.shift());
        }
    }
    __syncthreads();

    // 4. best candidate per track
    for (int e = tid; e < P; e += ID_THREADS) idx[e] = (unsigned short)e;
    __syncthreads();
    block_sort<ID_THREADS, true>(keys, idx, P, tid);
    head = 0;
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

    // 5. the `top` tracks: score descending, track ascending
    block_sort<ID_THREADS, true>(keys, idx, P, tid);
    if (tid < top) {
        const unsigned long long key = keys[tid];          // top <= 64 <= P
        const size_t o = (size_t)list * top + tid;
        if (key != SEQ_NONE) {
            const int t = (int)(key & 0xffffffffull);
            const int slot = idx[tid];
            out_track[o] = t;
            out_offset[o] = (int32_t)((int64_t)aux[slot] - grid.shift() - grid.fine(first[t]));
            out_score[o] = ord_f32(~(unsigned int)(key >> 32));
            out_votes[o] = (int32_t)votes[slot];
        } else {
            out_track[o] = -1;
            out_offset[o] = INT_MIN;
            out_score[o] = -INFINITY;
            out_votes[o] = 0;
        }
    }
}

}  // namespace grafp
