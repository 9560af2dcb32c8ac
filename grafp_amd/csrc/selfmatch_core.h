// selfmatch_core.h -- the one body of the shared-audio kernels: selfmatch.hip (the sources are tracks of the library,
// ops.self_match) and crossmatch.hip (the sources are recordings held outside the library, ops.cross_match and
// ops.cross_match_pq), crossmatch_tempo.hip (such recordings played faster or slower than the catalogue,
// ops.cross_match_tempo) and selfmatch_tempo.hip (tracks of the library that share audio at another speed,
// ops.self_match_tempo; match_tempo.h holds what the two tempo files share).  What a source's votes, spans, scores and partners are, the five phases and the workspace layout
// are stated at the top of selfmatch.hip; the arithmetic order of a score at the top of seqmatch.h.  The kernels differ
// in THREE things, the parameters of match_source:
//   * Source -- where source s comes from:
//         const float *x                the array its rows are read from, (.., 128) f32
//         int64_t row0(int s)           its first row in x AND in ids (ids holds one row of k hits per row of x)
//         int64_t len(int s)            its rows
//         static constexpr bool kDropOwn    whether hits inside the library rows [row0, row0 + len) are no hits
//     SelfSource (x = the library, row0 = first[tracks[s]], own-track hits dropped) and TableSource (x = q_rows,
//     row0 = src_first[s], nothing dropped) below;
//   * Span -- where the library rows of a span score come from (span_rows.h): RowSpan for f32 rows, PqSpan for rows
//     decoded from IVF-PQ codes, TempoRowSpan for f32 rows gathered along a slope;
//   * Grid -- where the rows of a source sit along the library, for a source that does not run at the catalogue's speed
//     (the manner of identify_core.h's DenseGrid / TempoGrid):
//         int64_t at(int64_t i)         library rows after source row 0 at which source row i sits
//         int64_t shift(int64_t L)      the key shift of a source of L rows: r - at(i) + shift(L) >= 0 for every hit
//         float score(span, x, a, lo, l, m)   the span call of phase 3: m pairs from source row lo on, alignment a
//     MatchDenseGrid (at = i, shift = L, span(x, a + lo, l, m)) for the three files above and MatchTempoGrid (at = w(i) =
//     (i * num + 128) >> 8, shift = 2 L, span(x, a, lo, num, l, m): TempoRowSpan) for the two tempo files.  Inside one
//     alignment run r = a + at(i) never decreases with i on either grid, which is all phase 2's walk needs.
// The workspace depends on a source's row count, k and min_votes only (sm_units), so plan_sources, the host's
// self_match_workspace and the -2 mark of a source that does not fit serve every kernel.
// Compiles with and without the packed-f32 instructions; every user is built without (Makefile NOPK).
#pragma once
#include <limits.h>
#include <math.h>

#include "common.h"
#include "seqmatch.h"

namespace grafp {

constexpr int SM_THREADS = 512;
constexpr int SM_MAX_K = 32;
constexpr int SM_MAX_TOP = 64;
constexpr int64_t SM_PIECE = 16384;                         // keys per LDS piece
constexpr size_t SM_LDS = (size_t)SM_PIECE * 8;            // 128 KiB of dynamic LDS
constexpr int SM_PLAN_THREADS = 1024;

__host__ __device__ inline int64_t sm_pow2(int64_t x) {
    int64_t p = 64;
    while (p < x) p <<= 1;
    return p;
}
// record capacity of a source of N0 hit slots: eligible candidates own disjoint sets of >= min_votes hits
__host__ __device__ inline int64_t sm_cap(int64_t N0, int min_votes) { return (N0 + min_votes - 1) / min_votes; }
// 8-byte units of a source's workspace region: records (3 units each), two key arrays for phases 4-5, and the hit keys
// when they exceed one LDS piece.  0 for a source without rows or with more hits than int32 counts.
__host__ __device__ inline int64_t sm_units(int64_t L, int k, int min_votes) {
    const int64_t N0 = L * k;
    if (L <= 0 || N0 > INT_MAX) return 0;
    const int64_t cap = sm_cap(N0, min_votes), P1 = sm_pow2(N0);
    return 3 * cap + 2 * sm_pow2(cap) + (P1 > SM_PIECE ? P1 : 0);
}

// bytes of the workspace header (n_src + 1 int64 region starts), rounded up to 256
__host__ __device__ inline int64_t sm_head_bytes(int n_src) { return ((int64_t)(n_src + 1) * 8 + 255) / 256 * 256; }

// the sources of self-match: tracks of the library itself
struct SelfSource {
    const float *x;                              // the library rows
    const int64_t *__restrict__ first;           // (T + 1) track table
    const int *__restrict__ tracks;              // (n_src) source tracks
    static constexpr bool kDropOwn = true;
    __device__ __forceinline__ int64_t row0(int s) const { return first[tracks[s]]; }
    __device__ __forceinline__ int64_t len(int s) const { return first[tracks[s] + 1] - first[tracks[s]]; }
};

// the sources of cross-match: source s is rows [src_first[s], src_first[s + 1]) of q_rows
struct TableSource {
    const float *x;                              // q_rows
    const int64_t *__restrict__ src_first;       // (n_src + 1) source table
    static constexpr bool kDropOwn = false;
    __device__ __forceinline__ int64_t row0(int s) const { return src_first[s]; }
    __device__ __forceinline__ int64_t len(int s) const { return src_first[s + 1] - src_first[s]; }
};

// the source runs at the catalogue's speed: row i sits i rows after row 0, a span is m consecutive library rows
struct MatchDenseGrid {
    __device__ __forceinline__ int64_t at(int64_t i) const { return i; }
    __device__ __forceinline__ int64_t shift(int64_t L) const { return L; }
    template <typename Span>
    __device__ __forceinline__ float score(const Span &span, const float4 *x, int64_t a, int lo, int l, int m) const {
        return span(x, a + lo, l, m);
    }
};

// The source runs at num / 256 of the catalogue's speed: row i sits w(i) = (i * num + 128) >> 8 rows after row 0 (num in
// [SEQ_TEMPO_MIN, SEQ_TEMPO_MAX] of seqmatch.h; i * num + 128 stays inside an int32 for the SM_TEMPO_MAX_ROWS a source
// may have, and w(L - 1) <= 2 L - 2, hence the shift).  Its Span gathers: span(x, a, lo, num, l, m) reads row a + w(lo + t).
constexpr int64_t SM_TEMPO_MAX_ROWS = 4194303;             // (2^31 - 128) / 512
struct MatchTempoGrid {
    int num;
    __device__ __forceinline__ int64_t at(int64_t i) const { return ((int)i * num + SEQ_TEMPO_DEN / 2) >> 8; }
    __device__ __forceinline__ int64_t shift(int64_t L) const { return 2 * L; }
    template <typename Span>
    __device__ __forceinline__ float score(const Span &span, const float4 *x, int64_t a, int lo, int l, int m) const {
        return span(x, a, lo, num, l, m);
    }
};

// one bitonic stage over keys[0, cnt) whose slot 0 is global slot g0
__device__ __forceinline__ void sm_stage(unsigned long long *keys, int64_t cnt, int64_t g0, int64_t k2, int64_t j,
                                         int tid) {
    bitonic_stage<SM_THREADS, false, int64_t>(keys, nullptr, cnt, g0, k2, j, tid);
}

// ascending sort of P (a power of two >= 64) keys: in place in LDS (in_lds, P <= SM_PIECE), or in global memory with
// every stage of partner distance below the piece size run on LDS pieces
__device__ __forceinline__ void sm_sort(unsigned long long *keys, int64_t P, unsigned long long *lds, bool in_lds,
                                        int tid) {
    if (in_lds) {
        block_sort<SM_THREADS, false>(keys, nullptr, P, tid);
        return;
    }
    const int64_t pc = P < SM_PIECE ? P : SM_PIECE;
    for (int64_t k2 = 2; k2 <= P; k2 <<= 1) {
        if (k2 > pc)
            for (int64_t j = k2 >> 1; j >= pc; j >>= 1) sm_stage(keys, P, 0, k2, j, tid);
        if (k2 > pc || k2 == 2) {
            // one visit per piece: every remaining stage of this level (all levels up to pc on the first visit)
            for (int64_t base = 0; base < P; base += pc) {
                for (int64_t e = tid; e < pc; e += SM_THREADS) lds[e] = keys[base + e];
                __syncthreads();
                for (int64_t kk = (k2 > pc ? k2 : 2); kk <= (k2 > pc ? k2 : pc); kk <<= 1)
                    for (int64_t j = (kk < pc ? kk : pc) >> 1; j > 0; j >>= 1) sm_stage(lds, pc, base, kk, j, tid);
                for (int64_t e = tid; e < pc; e += SM_THREADS) keys[base + e] = lds[e];
                __syncthreads();
            }
        }
    }
}

// the rank of record c among its partner's: the score, then the smaller alignment key -- ONE 64-bit value, so that the
// choice is one compare.  (Stated as `o > bo || (o == bo && a_c < a_best)` the generated gfx950 code kept the old record
// when the second clause held: equal scores went to whichever record the walkers of phase 2 had stored first, DESIGN.md
// section 12.25.)
__device__ __forceinline__ unsigned long long sm_rank(const unsigned int *rec, unsigned int c) {
    const unsigned int *rc = rec + 6 * (int64_t)c;
    return ((unsigned long long)f32_ord(__uint_as_float(rc[5])) << 32) | (unsigned int)~rc[1];
}

// the best record of the partner run that starts at slot e of the sorted phase 4 keys
__device__ __forceinline__ unsigned int sm_best(const unsigned long long *k4, int64_t P, int64_t e,
                                                const unsigned int *rec) {
    const unsigned long long b = k4[e] >> 32;
    unsigned int best = (unsigned int)k4[e];
    unsigned long long br = sm_rank(rec, best);
    for (int64_t f = e + 1; f < P; ++f) {
        const unsigned long long key = k4[f];
        if ((key >> 32) != b) break;
        const unsigned int c = (unsigned int)key;
        const unsigned long long cr = sm_rank(rec, c);
        if (cr > br) {                                       // (two records of one partner never share an alignment)
            best = c;
            br = cr;
        }
    }
    return best;
}

// an empty result slot (track -1; -2 marks a source whose region does not fit the workspace)
__device__ __forceinline__ void sm_pad(size_t o, int32_t track, int32_t *__restrict__ out_track,
                                       int32_t *__restrict__ out_delta, int32_t *__restrict__ out_start,
                                       int32_t *__restrict__ out_len, float *__restrict__ out_score,
                                       int32_t *__restrict__ out_votes) {
    out_track[o] = track;
    out_delta[o] = INT_MIN;
    out_start[o] = -1;
    out_len[o] = 0;
    out_score[o] = -INFINITY;
    out_votes[o] = 0;
}

// exclusive scan of the per-source region sizes into the workspace header (one workgroup of SM_PLAN_THREADS)
template <typename Source>
__device__ __forceinline__ void plan_sources(const Source &source, int n_src, int k, int min_votes,
                                             int64_t *__restrict__ off) {
    __shared__ int64_t part[SM_PLAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (n_src + SM_PLAN_THREADS - 1) / SM_PLAN_THREADS;
    const int s0 = tid * per < n_src ? tid * per : n_src, s1 = s0 + per < n_src ? s0 + per : n_src;
    int64_t sum = 0;
    for (int s = s0; s < s1; ++s) sum += sm_units(source.len(s), k, min_votes);
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < SM_PLAN_THREADS; d <<= 1) {
        const int64_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;
    for (int s = s0; s < s1; ++s) {
        off[s] = run;
        run += sm_units(source.len(s), k, min_votes);
    }
    if (tid == SM_PLAN_THREADS - 1) off[n_src] = part[tid];
}

// One source by one workgroup of SM_THREADS threads (blockIdx.x = the source), SM_LDS bytes of dynamic LDS.  The source's
// region is ws + head_units + off[src]: a caller with one copy of the regions per grid passes that copy's start.
template <typename Grid, typename Source, typename Span>
__device__ __forceinline__ void match_source(
    const Grid &grid, const Source &source, const Span &span, int64_t n, const int64_t *__restrict__ first, int T,
    const int64_t *__restrict__ ids, int k, int top, int min_votes, int min_overlap, unsigned long long *__restrict__ ws,
    int64_t head_units, int64_t cap_units, int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta,
    int32_t *__restrict__ out_start, int32_t *__restrict__ out_len, float *__restrict__ out_score,
    int32_t *__restrict__ out_votes) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sm_lds[];
    __shared__ int s_nc;
    const int src = blockIdx.x, tid = threadIdx.x;
    const int64_t fa = source.row0(src), L64 = source.len(src);
    const int64_t o0 = reinterpret_cast<const int64_t *>(ws)[src], o1 = reinterpret_cast<const int64_t *>(ws)[src + 1];
    const int64_t N0 = L64 * k;
    // no rows, or a region past the workspace (ws_bytes below grafp_self_match_workspace): padding; the latter marks -2
    if (L64 <= 0 || N0 > INT_MAX || head_units + o1 > cap_units) {
        if (tid < top) {
            const size_t o = (size_t)src * top + tid;
            sm_pad(o, (L64 > 0 && tid == 0) ? -2 : -1, out_track, out_delta, out_start, out_len, out_score, out_votes);
        }
        return;
    }
    const int64_t cap = sm_cap(N0, min_votes), P2max = sm_pow2(cap), P1 = sm_pow2(N0);
    unsigned long long *region = ws + head_units + o0;
    unsigned int *rec = reinterpret_cast<unsigned int *>(region);
    unsigned long long *k4g = region + 3 * cap, *k5g = k4g + P2max, *k1g = k5g + P2max;
    const bool l1 = P1 <= SM_PIECE;
    unsigned long long *K1 = l1 ? sm_lds : k1g;
    if (tid == 0) s_nc = 0;

    // 1. hit keys; ids outside [0, n), and inside the source where it is part of the library, are no hits
    for (int64_t e = tid; e < P1; e += SM_THREADS) {
        unsigned long long key = SEQ_NONE;
        if (e < N0) {
            const int i = (int)e / k;                     // e < N0 <= INT_MAX
            const int64_t r = ids[(fa + i) * k + ((int)e - i * k)];
            if (r >= 0 && r < n && (!Source::kDropOwn || r < fa || r >= fa + L64))
                key = ((unsigned long long)(r - grid.at(i) + grid.shift(L64)) << 32) | (unsigned int)i;
        }
        K1[e] = key;
    }
    __syncthreads();
    if (l1) sm_sort(sm_lds, P1, sm_lds, true, tid);      // (branches, not a selected pointer: LDS stays ds_ access)
    else sm_sort(k1g, P1, sm_lds, false, tid);

    // 2. one walker per alignment run; eligible candidates become records
    for (int64_t e = tid; e < P1; e += SM_THREADS) {
        const unsigned long long key = K1[e];
        if (key == SEQ_NONE || (e > 0 && (K1[e - 1] >> 32) == (key >> 32))) continue;
        const unsigned long long hi = key >> 32;
        const int64_t ag = (int64_t)hi - grid.shift(L64);
        int t = 0, nv = 0;
        int64_t end = -1;
        unsigned int ilo = 0, ihi = 0;
        for (int64_t f = e;; ++f) {
            const unsigned long long kf = f < P1 ? K1[f] : SEQ_NONE;
            const bool more = kf != SEQ_NONE && (kf >> 32) == hi;
            const int64_t r = ag + grid.at((int64_t)(unsigned int)kf);
            if (!more || r >= end) {                          // the run ends, or crosses into a later track
                if (nv >= min_votes && (int)(ihi - ilo) + 1 >= min_overlap) {
                    const int c = atomicAdd(&s_nc, 1);
                    if (c < cap) {
                        unsigned int *rc = rec + 6 * (int64_t)c;
                        rc[0] = (unsigned int)t;
                        rc[1] = (unsigned int)hi;
                        rc[2] = ilo;
                        rc[3] = ihi - ilo + 1;
                        rc[4] = (unsigned int)nv;
                        rc[5] = 0;
                    }
                }
                if (!more) break;
                t = track_of(first, end < 0 ? 0 : (t + 1 < T ? t + 1 : T - 1), T, r);
                end = first[t + 1];
                nv = 0;
                ilo = (unsigned int)kf;
            }
            ihi = (unsigned int)kf;
            ++nv;
        }
    }
    __syncthreads();
    const int nc = s_nc < cap ? s_nc : (int)cap;
    if (nc == 0) {
        if (tid < top) {
            const size_t o = (size_t)src * top + tid;
            sm_pad(o, -1, out_track, out_delta, out_start, out_len, out_score, out_votes);
        }
        return;
    }

    // 3. scores: one record per half-wave at a time
    const int hw = tid >> 5, l = tid & 31;
    const float4 *x4 = reinterpret_cast<const float4 *>(source.x);
    for (int c = hw; c < nc; c += SM_THREADS / 32) {
        const unsigned int *rc = rec + 6 * (int64_t)c;
        const int64_t ag = (int64_t)rc[1] - grid.shift(L64);
        const int ilo = (int)rc[2], m = (int)rc[3];
        const float acc = grid.score(span, x4 + (fa + ilo) * (SEQ_D / 4) + l, ag, ilo, l, m);
        if (l == 0) rec[6 * (int64_t)c + 5] = __float_as_uint(acc / (float)m);
    }
    __syncthreads();

    // 4. records grouped by partner; the first slot of every partner run finds the run's best
    const int64_t P2 = sm_pow2(nc);
    const bool l2 = 2 * P2 <= SM_PIECE;
    unsigned long long *K4 = l2 ? sm_lds : k4g, *K5 = l2 ? sm_lds + P2 : k5g;
    for (int64_t e = tid; e < P2; e += SM_THREADS)
        K4[e] = e < nc ? (((unsigned long long)rec[6 * e] << 32) | (unsigned int)e) : SEQ_NONE;
    __syncthreads();
    if (l2) sm_sort(sm_lds, P2, sm_lds, true, tid);
    else sm_sort(k4g, P2, sm_lds, false, tid);
    for (int64_t e = tid; e < P2; e += SM_THREADS) {
        const unsigned long long key = K4[e];
        unsigned long long out = SEQ_NONE;
        if (key != SEQ_NONE && (e == 0 || (K4[e - 1] >> 32) != (key >> 32))) {
            const unsigned int best = sm_best(K4, P2, e, rec);
            out = ((unsigned long long)~f32_ord(__uint_as_float(rec[6 * (int64_t)best + 5])) << 32) | (unsigned int)e;
        }
        K5[e] = out;
    }
    __syncthreads();

    // 5. the `top` partners: score descending, partner ascending (slot order within K4 is partner order)
    if (l2) sm_sort(sm_lds + P2, P2, sm_lds, true, tid);
    else sm_sort(k5g, P2, sm_lds, false, tid);
    if (tid < top) {
        const size_t o = (size_t)src * top + tid;
        const unsigned long long key = K5[tid];              // top <= 64 <= P2
        if (key != SEQ_NONE) {
            const unsigned int c = sm_best(K4, P2, (int64_t)(unsigned int)key, rec);
            const unsigned int *rc = rec + 6 * (int64_t)c;
            const int b = (int)rc[0];
            out_track[o] = b;
            out_delta[o] = (int32_t)((int64_t)rc[1] - grid.shift(L64) - first[b]);
            out_start[o] = (int32_t)rc[2];
            out_len[o] = (int32_t)rc[3];
            out_score[o] = __uint_as_float(rc[5]);
            out_votes[o] = (int32_t)rc[4];
        } else {
            sm_pad(o, -1, out_track, out_delta, out_start, out_len, out_score, out_votes);
        }
    }
}

// the launch-time checks every kernel shares (name: the operation, for the message).  The header must fit; a source
// whose region falls past ws_bytes is marked -2 by the kernel (no write outside ws).
inline int sm_check_launch(const char *name, int k, int top, int min_votes, int min_overlap, int n_src, const void *ws,
                           size_t ws_bytes) {
    GRAFP_REQUIRE(k >= 1 && k <= SM_MAX_K, "%s: k=%d hits per row exceeds %d", name, k, SM_MAX_K);
    GRAFP_REQUIRE(top >= 1 && top <= SM_MAX_TOP, "%s: top=%d not in [1, %d]", name, top, SM_MAX_TOP);
    GRAFP_REQUIRE(min_votes >= 1 && min_overlap >= 1, "%s: min_votes=%d and min_overlap=%d must be >= 1", name,
                  min_votes, min_overlap);
    const size_t head = (size_t)sm_head_bytes(n_src);
    if (!ws || ws_bytes < head) {
        set_error("%s: workspace of %zu bytes, at least %zu needed for the header alone", name, ws_bytes, head);
        return GRAFP_ERR_WORKSPACE;
    }
    return GRAFP_OK;
}

// reserves the dynamic LDS of one match kernel and launches it on `grid` (blockIdx.x = the source)
template <typename... Params, typename... Args>
inline int sm_launch(const char *name, void (*kernel)(Params...), dim3 grid, hipStream_t stream, Args... args) {
    return seq_launch(name, kernel, grid, SM_THREADS, SM_LDS, stream, args...);
}

}  // namespace grafp
