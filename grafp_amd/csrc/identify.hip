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
// Built WITHOUT packed-f32 instructions (Makefile NOPK, as corpus.hip): its sums are plain fmaf chains, and the packed
// operand-select form is the hazard of DESIGN.md section 12.7b.
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
constexpr size_t ID_LDS = 160 * 1024 - 256;      // dynamic LDS budget (the static s_ncand sits next to it)
// row pairs in flight in the score loop (seqmatch.h, span_sum): query rows in LDS / in global memory
constexpr int ID_UNROLL_QLDS = 4, ID_UNROLL_QGLOBAL = 1;

template <bool kQLds>
__global__ __launch_bounds__(ID_THREADS) void identify_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T,
    const float *__restrict__ q_rows, const int64_t *__restrict__ ids, int k, const int64_t *__restrict__ item_row,
    const int *__restrict__ item_len, int max_len, int Pmax, int top, int min_overlap, int32_t *__restrict__ out_track,
    int32_t *__restrict__ out_offset, float *__restrict__ out_score, int32_t *__restrict__ out_votes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char id_smem[];
    __shared__ int s_ncand;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(id_smem);
    unsigned int *aux = reinterpret_cast<unsigned int *>(id_smem + (size_t)8 * Pmax);
    unsigned short *votes = reinterpret_cast<unsigned short *>(id_smem + (size_t)12 * Pmax);
    unsigned short *idx = reinterpret_cast<unsigned short *>(id_smem + (size_t)14 * Pmax);
    float *sq = reinterpret_cast<float *>(id_smem + (size_t)16 * Pmax);

    const int item = blockIdx.x, tid = threadIdx.x;
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
            if (r >= 0 && r < n) key = ((unsigned long long)(r - s + ID_SHIFT) << 32) | (unsigned int)s;
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
        const int64_t a = (int64_t)hi - ID_SHIFT;
        int start = e, nv = 0, t = 0;
        int64_t end = -1;
        for (int f = e; f < P; ++f) {
            const unsigned long long key = keys[f];
            if ((key >> 32) != hi) break;                   // the next run, or the empty tail
            const int64_t r = a + (int64_t)(unsigned int)key;
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
    const int need_q = min_overlap > 0 ? min_overlap : ql;
    const float4 *rw4 = reinterpret_cast<const float4 *>(rows);
    const float4 *q4 = kQLds ? reinterpret_cast<const float4 *>(sq) : reinterpret_cast<const float4 *>(q_rows + r0 * SEQ_D);
    for (int c = hw; c < ncand; c += ID_THREADS / 32) {
        const int e = idx[c];
        const int64_t a = (int64_t)(keys[e] >> 32) - ID_SHIFT;
        const int t = (int)aux[e];
        int64_t f0 = first[t], f1 = first[t + 1];
        f0 = f0 < 0 ? 0 : f0;                               // (a valid table needs neither clamp)
        f1 = f1 > n ? n : f1;
        const int64_t L = f1 - f0;
        const int lo = (int)(f0 - a > 0 ? f0 - a : 0);
        const int hi = (int)(f1 - a < ql ? f1 - a : ql);
        const int o = hi - lo;
        const bool ok = o >= 1 && o >= (need_q < L ? need_q : L);
        const float acc = span_sum<kQLds ? ID_UNROLL_QLDS : ID_UNROLL_QGLOBAL>(
            q4 + lo * (SEQ_D / 4) + l, rw4 + (a + lo) * (SEQ_D / 4) + l, ok ? o : 0);   // (not ok: no row is read)
        const float score = acc / (float)o;
        // every lane of the half-wave has read keys[e] and aux[e] before the shuffles above
        if (l == 0) {
            keys[e] = ok ? (((unsigned long long)t << 32) | ~f32_ord(score)) : SEQ_NONE;
            aux[e] = (unsigned int)(a + ID_SHIFT);
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
        const size_t o = (size_t)item * top + tid;
        if (key != SEQ_NONE) {
            const int t = (int)(key & 0xffffffffull);
            const int slot = idx[tid];
            out_track[o] = t;
            out_offset[o] = (int32_t)((int64_t)aux[slot] - ID_SHIFT - first[t]);
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

int identify_launch(const float *rows, int64_t n, const int64_t *first, int T, const float *q_rows,
                    const int64_t *ids, int k, const int64_t *item_row, const int *item_len, int n_items, int max_len,
                    int top, int min_overlap, int32_t *out_track, int32_t *out_offset, float *out_score,
                    int32_t *out_votes, hipStream_t stream) {
    GRAFP_REQUIRE(max_len >= 1 && max_len <= ID_MAX_LEN && k >= 1 && k <= ID_MAX_K && max_len * k <= ID_MAX_KEYS,
                  "identify: max_len=%d k=%d exceed %d segments, %d hits per segment or %d keys per item", max_len, k,
                  ID_MAX_LEN, ID_MAX_K, ID_MAX_KEYS);
    if (n_items == 0) return GRAFP_OK;
    int Pmax = 64;
    while (Pmax < max_len * k) Pmax <<= 1;
    const size_t slots = (size_t)16 * Pmax, qbytes = (size_t)max_len * SEQ_D * sizeof(float);
    const bool q_lds = slots + qbytes <= ID_LDS;
    const size_t lds = q_lds ? slots + qbytes : slots;
    const void *fn = q_lds ? (const void *)identify_kernel<true> : (const void *)identify_kernel<false>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("identify: cannot reserve %zu bytes of LDS", lds);
        return GRAFP_ERR_LAUNCH;
    }
    if (q_lds)
        hipLaunchKernelGGL(identify_kernel<true>, dim3(n_items), dim3(ID_THREADS), lds, stream, rows, n, first, T,
                           q_rows, ids, k, item_row, item_len, max_len, Pmax, top, min_overlap, out_track, out_offset,
                           out_score, out_votes);
    else
        hipLaunchKernelGGL(identify_kernel<false>, dim3(n_items), dim3(ID_THREADS), lds, stream, rows, n, first, T,
                           q_rows, ids, k, item_row, item_len, max_len, Pmax, top, min_overlap, out_track, out_offset,
                           out_score, out_votes);
    GRAFP_CHECK_LAUNCH("identify_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
