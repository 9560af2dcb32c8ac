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
// Workspace: a header of n_src + 1 int64 region starts written by self_match_plan_kernel (an exclusive scan of the
// per-source sizes sm_units), then one region per source: records (24 bytes x ceil(N0 / min_votes)), the phase 4 and 5
// keys (pow2(max(64, records)) each), and the hit keys when they do not fit in LDS.  self_match_workspace sums the same
// sizes on the host from the sources' row counts, so the caller's buffer is exactly what the launch lays out.  A source
// whose region ends past ws_bytes writes -2 to its first out_track slot and nothing else.
// Built WITHOUT packed-f32 instructions (Makefile NOPK, as identify.hip): its sums are plain fmaf chains, and the packed
// operand-select form is the hazard of DESIGN.md section 12.7b.
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
constexpr int SM_UNROLL = 4;                                // row pairs in flight in the score loop (span_sum)

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

// the best record of the partner run that starts at slot e of the sorted phase 4 keys
__device__ __forceinline__ unsigned int sm_best(const unsigned long long *k4, int64_t P, int64_t e,
                                                const unsigned int *rec) {
    const unsigned long long b = k4[e] >> 32;
    unsigned int best = (unsigned int)k4[e], bo = f32_ord(__uint_as_float(rec[6 * (int64_t)best + 5]));
    for (int64_t f = e + 1; f < P; ++f) {
        const unsigned long long key = k4[f];
        if ((key >> 32) != b) break;
        const unsigned int c = (unsigned int)key, o = f32_ord(__uint_as_float(rec[6 * (int64_t)c + 5]));
        if (o > bo || (o == bo && rec[6 * (int64_t)c + 1] < rec[6 * (int64_t)best + 1])) {
            best = c;
            bo = o;
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

// exclusive scan of the per-source region sizes into the workspace header (one workgroup)
__global__ __launch_bounds__(SM_PLAN_THREADS) void self_match_plan_kernel(const int64_t *__restrict__ first,
                                                                          const int *__restrict__ tracks, int n_src,
                                                                          int k, int min_votes, int64_t *__restrict__ off) {
    __shared__ int64_t part[SM_PLAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (n_src + SM_PLAN_THREADS - 1) / SM_PLAN_THREADS;
    const int s0 = tid * per < n_src ? tid * per : n_src, s1 = s0 + per < n_src ? s0 + per : n_src;
    int64_t sum = 0;
    for (int s = s0; s < s1; ++s) sum += sm_units(first[tracks[s] + 1] - first[tracks[s]], k, min_votes);
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
        run += sm_units(first[tracks[s] + 1] - first[tracks[s]], k, min_votes);
    }
    if (tid == SM_PLAN_THREADS - 1) off[n_src] = part[tid];
}

__global__ __launch_bounds__(SM_THREADS) void self_match_kernel(
    const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ first, int T, const int64_t *__restrict__ ids,
    int k, const int *__restrict__ tracks, int top, int min_votes, int min_overlap, unsigned long long *__restrict__ ws,
    int64_t head_units, int64_t cap_units, int32_t *__restrict__ out_track, int32_t *__restrict__ out_delta,
    int32_t *__restrict__ out_start, int32_t *__restrict__ out_len, float *__restrict__ out_score,
    int32_t *__restrict__ out_votes) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sm_lds[];
    __shared__ int s_nc;
    const int src = blockIdx.x, tid = threadIdx.x;
    const int a = tracks[src];
    const int64_t fa = first[a], L64 = first[a + 1] - fa;
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

    // 1. hit keys; ids outside [0, n) and inside the source track are no hits
    for (int64_t e = tid; e < P1; e += SM_THREADS) {
        unsigned long long key = SEQ_NONE;
        if (e < N0) {
            const int i = (int)e / k;                     // e < N0 <= INT_MAX
            const int64_t r = ids[(fa + i) * k + ((int)e - i * k)];
            if (r >= 0 && r < n && (r < fa || r >= fa + L64))
                key = ((unsigned long long)(r - i + L64) << 32) | (unsigned int)i;
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
        const int64_t ag = (int64_t)hi - L64;
        int t = 0, nv = 0;
        int64_t end = -1;
        unsigned int ilo = 0, ihi = 0;
        for (int64_t f = e;; ++f) {
            const unsigned long long kf = f < P1 ? K1[f] : SEQ_NONE;
            const bool more = kf != SEQ_NONE && (kf >> 32) == hi;
            const int64_t r = ag + (int64_t)(unsigned int)kf;
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
    const float4 *rw4 = reinterpret_cast<const float4 *>(rows);
    for (int c = hw; c < nc; c += SM_THREADS / 32) {
        const unsigned int *rc = rec + 6 * (int64_t)c;
        const int64_t ag = (int64_t)rc[1] - L64;
        const int ilo = (int)rc[2], m = (int)rc[3];
        const float4 *x = rw4 + (fa + ilo) * (SEQ_D / 4) + l;
        const float4 *y = rw4 + (ag + ilo) * (SEQ_D / 4) + l;
        const float acc = span_sum<SM_UNROLL>(x, y, m);
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
            out_delta[o] = (int32_t)((int64_t)rc[1] - L64 - first[b]);
            out_start[o] = (int32_t)rc[2];
            out_len[o] = (int32_t)rc[3];
            out_score[o] = __uint_as_float(rc[5]);
            out_votes[o] = (int32_t)rc[4];
        } else {
            sm_pad(o, -1, out_track, out_delta, out_start, out_len, out_score, out_votes);
        }
    }
}

size_t self_match_workspace(const int64_t *src_rows, int n_src, int k, int min_votes) {
    if (n_src < 0 || (n_src > 0 && !src_rows) || k < 1 || min_votes < 1) return 0;
    int64_t units = 0;                                    // exactly the regions self_match_plan_kernel lays out
    for (int s = 0; s < n_src; ++s) units += sm_units(src_rows[s], k, min_votes);
    return (size_t)(sm_head_bytes(n_src) + 8 * units);
}

int self_match_launch(const float *rows, int64_t n, const int64_t *first, int T, const int64_t *ids, int k,
                      const int *tracks, int n_src, int top, int min_votes, int min_overlap, void *ws,
                      size_t ws_bytes, int32_t *out_track, int32_t *out_delta, int32_t *out_start, int32_t *out_len,
                      float *out_score, int32_t *out_votes, hipStream_t stream) {
    GRAFP_REQUIRE(k >= 1 && k <= SM_MAX_K, "self_match: k=%d hits per row exceeds %d", k, SM_MAX_K);
    GRAFP_REQUIRE(top >= 1 && top <= SM_MAX_TOP, "self_match: top=%d not in [1, %d]", top, SM_MAX_TOP);
    GRAFP_REQUIRE(min_votes >= 1 && min_overlap >= 1, "self_match: min_votes=%d and min_overlap=%d must be >= 1",
                  min_votes, min_overlap);
    // the header must fit; a source whose region falls past ws_bytes is marked -2 by the kernel (no write outside ws)
    const size_t head = (size_t)sm_head_bytes(n_src);
    if (!ws || ws_bytes < head) {
        set_error("self_match: workspace of %zu bytes, at least %zu needed for the header alone", ws_bytes, head);
        return GRAFP_ERR_WORKSPACE;
    }
    if (n_src == 0) return GRAFP_OK;
    const int64_t head_units = (int64_t)head / 8;
    hipLaunchKernelGGL(self_match_plan_kernel, dim3(1), dim3(SM_PLAN_THREADS), 0, stream, first, tracks, n_src, k,
                       min_votes, reinterpret_cast<int64_t *>(ws));
    GRAFP_CHECK_LAUNCH("self_match_plan_kernel");
    if (hipFuncSetAttribute((const void *)self_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SM_LDS) !=
        hipSuccess) {
        set_error("self_match: cannot reserve %zu bytes of LDS", SM_LDS);
        return GRAFP_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(self_match_kernel, dim3(n_src), dim3(SM_THREADS), SM_LDS, stream, rows, n, first, T, ids, k,
                       tracks, top, min_votes, min_overlap, reinterpret_cast<unsigned long long *>(ws), head_units,
                       (int64_t)(ws_bytes / 8), out_track, out_delta, out_start, out_len, out_score, out_votes);
    GRAFP_CHECK_LAUNCH("self_match_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
