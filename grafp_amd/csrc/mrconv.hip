// mrconv.hip -- edge gather + max-relative aggregation (K6+K7 of SURVEY.md section 2a), gfx950.
//
// Replaces, for the live 'mr' graph conv (/root/reference/encoder/gcn_lib/torch_vertex.py:19-34):
//   x_i = batched_index_select(x, centre)   torch_nn.py:79-98   (a (B,C,N,k) copy of x itself)
//   x_j = batched_index_select(x, nn_idx)                       (a (B,C,N,k) gather)
//   rel = max_k(x_j - x_i) ; out = interleave(x, rel)           torch_vertex.py:29-32
// The reference moves ~4 full-tensor copies per call through HBM (201 MB twice at B=256 stage 0); here a
// workgroup stages a slab of channel rows of one clip in LDS, gathers neighbours from LDS and writes
// the interleaved (B,2C,N) result once.  HBM-bound: 4CN + 8kN read, 8CN written per clip.
//
// Backward recomputes the arg-max neighbour (first maximum, as torch.max on CPU) and scatter-adds into
// an LDS accumulator row, so dx is written once, coalesced, with no global atomics.
#include <math.h>

#define GRAFP_STORE_FAMILY 3        // (common.h: GRAFP_ST_NT experiment builds)
#include "elemio.h"

namespace grafp {

constexpr int MR_THREADS = 256;

__device__ __forceinline__ int clampi(int64_t v, int n) {
    return v < 0 ? 0 : (v >= n ? n - 1 : (int)v);
}

// What is specific to max-relative in the element access of elemio.h: how many slabs of raw pieces a thread keeps in flight
// (the same bytes for both element types).  Outputs are streamed, or stored plain when the result fits the Infinity Cache
// beside its reader's other operand (plain_stores, "GRAFP_MR_PLAIN_MAX_MB").
template <typename T> constexpr int MR_NPAR = sizeof(T) == 4 ? 2 : 4;

// The backward scatter accumulates in 64-bit FIXED POINT with integer LDS atomics (ds_add_f32 runs at 0.33 lane-ops per
// clock per CU on gfx950, ds_add_u64 at 10: tools/microbench/lds_atomic_bench.hip; and the sum no longer depends on the
// order of the atomics: the gradient is deterministic).  Per slab the scale is 2^(39 - e), m = max |addend| < 2^e: an
// addend becomes the integer v = rint(g scale), |v| < 2^39, carried as TWO signed 32-bit fields of one 64-bit word,
// v = hi 2^20 + lo (|lo| < 2^20, |hi| < 2^19): a node receives at most N <= 2048 addends, so neither field's sum leaves
// its 31 bits, the 64-bit add keeps the borrows right, and building / reading the word costs 9 + 7 VALU instructions
// instead of the ~35 of the f32 <-> i64 conversions (both kernels were VALU-bound on them: 60 VALU instructions per
// element, 300 us per call where the bytes take 130).
__device__ __forceinline__ unsigned long long mr_fix_encode(float g, float scale) {
    const float v = __builtin_rintf(g * scale);
    const float hf = __builtin_truncf(v * 9.5367431640625e-7f);                 // 2^-20
    const float lf = __builtin_fmaf(hf, -1048576.0f, v);                        // exact
    const int hi = (int)hf, lo = (int)lf;
    return ((unsigned long long)(unsigned)(hi + (lo >> 31)) << 32) | (unsigned long long)(unsigned)lo;
}
__device__ __forceinline__ float mr_fix_decode(unsigned long long a) {
    const int lo = (int)(unsigned)a;
    const int hi = (int)(unsigned)(a >> 32) - (lo >> 31);
    return (float)__builtin_fma((double)hi, 1048576.0, (double)lo);             // the sum exactly, rounded once
}
// The fixed-point scale of a slab, in the two halves around the barrier every backward kernel has anyway: each thread brings
// the largest sign-stripped bit pattern of its g_odd (an integer maximum: NaN / inf sort last), mr_scale_publish leaves the
// four waves' maxima in s_max, and after the barrier mr_scale_read gives every thread the same scale.
struct MrScale {
    float scale, inv_scale;
    bool poisoned;                                  // a non-finite gradient in the slab: its whole output is NaN
    __device__ __forceinline__ unsigned long long encode(float g) const { return mr_fix_encode(g, scale); }
    // the output element: identity branch minus the centre term, plus what was scattered to it
    __device__ __forceinline__ float out(float base, unsigned long long acc) const {
        return poisoned ? NAN : base + mr_fix_decode(acc) * inv_scale;
    }
};
__device__ __forceinline__ void mr_scale_publish(unsigned m, unsigned *s_max, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((tid & 63) == 0) s_max[tid >> 6] = m;
}
__device__ __forceinline__ MrScale mr_scale_read(const unsigned *s_max) {
    const unsigned mbits = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    MrScale s;
    s.poisoned = mbits >= 0x7f800000u;
    int ex = 0;
    (void)frexpf(__uint_as_float(mbits), &ex);                // m < 2^ex
    int sh = mbits ? 39 - ex : 0;
    sh = sh > 100 ? 100 : sh;
    s.scale = ldexpf(1.0f, sh);
    s.inv_scale = ldexpf(1.0f, -sh);
    return s;
}

// The routing rule of the backward pass, written once: a node's g_odd goes to the FIRST maximum of x[j] - x[n] over its K
// edges.  Edge 0 wins unconditionally -- a NaN difference there stays the winner, as the first NaN does in torch.max --
// and a later edge only on v > best (never a NaN).  The forward record and both recomputing backward kernels call this,
// so they cannot route differently.  True when edge k is the winner so far.
__device__ __forceinline__ bool mr_first_max(int k, float v, float &best) {
    const bool wins = k == 0 || v > best;
    if (wins) best = v;
    return wins;
}

// Activations are addressed as base + b*sb + c*sc + n (N contiguous): (B,C,N) has sb = C*N, sc = N; the
// GEMM-friendly (C,B,N) has sb = N, sc = B*N.  dynamic LDS: rows[CC*N] f32 | sidx[K*N] i32 (bwd: + acc[CC*N] i64, base f32).
// A workgroup owns CC channel rows of one clip; thread t walks the slab's elements t*V, t*V + 256*V, ... as a
// running (channel, node) pair -- no integer division in any loop.  V = 4 when N % 4 == 0 and the strides and
// base pointers are 4-element aligned (always true for the encoder's shapes), else 1.
#define MR_WALK(V, tid, N, c, n)                    \
    int c = ((tid) * (V)) / (N), n = ((tid) * (V)) - c * (N)
#define MR_NEXT(V, N, c, n)                         \
    do {                                            \
        n += MR_THREADS * (V);                      \
        while (n >= (N)) { n -= (N); ++c; }         \
    } while (0)

template <typename I>
__device__ __forceinline__ void stage_idx(int *sidx, const I *__restrict__ idxb, int N, int K, int tid) {
    for (int n = tid; n < N; n += MR_THREADS)
        for (int k = 0; k < K; ++k) sidx[k * N + n] = clampi((int64_t)idxb[(size_t)n * K + k], N);
}

// A thread's ITEMS 4-element pieces inside a slab of the persistent kernels: (channel offset, node) of piece it.
template <int ITEMS>
__device__ __forceinline__ void mr_pieces(int tid, int N, int (&pc)[ITEMS], int (&pn)[ITEMS]) {
    MR_WALK(4, tid, N, c, n);
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        pc[it] = c;
        pn[it] = n;
        MR_NEXT(4, N, c, n);
    }
}

template <typename T, int V, typename I>
__global__ __launch_bounds__(MR_THREADS) void mrconv_fwd_kernel(const T *__restrict__ x, int64_t x_sb, int64_t x_sc,
                                                                const I *__restrict__ idx, T *__restrict__ out,
                                                                int64_t o_sb, int64_t o_sc, int C, int N, int K,
                                                                int CC) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.y, c0 = blockIdx.x * CC, tid = threadIdx.x;
    const int cc = min(CC, C - c0);
    float *rows = reinterpret_cast<float *>(smem);
    int *sidx = reinterpret_cast<int *>(rows + (size_t)CC * N);
    const T *xb = x + (size_t)b * x_sb + (size_t)c0 * x_sc;
    {
        MR_WALK(V, tid, N, c, n);
        while (c < cc) {
            float v[4];
            if (V == 4) ElemIO<T>::load(xb + (size_t)c * x_sc + n, v); else v[0] = ld_as_f32(xb + (size_t)c * x_sc + n);
#pragma unroll
            for (int e = 0; e < V; ++e) rows[c * N + n + e] = v[e];
            MR_NEXT(V, N, c, n);
        }
    }
    stage_idx<I>(sidx, idx + (size_t)b * N * K, N, K, tid);
    __syncthreads();

    T *ob = out + (size_t)b * o_sb + (size_t)(2 * c0) * o_sc;
    MR_WALK(V, tid, N, c, n);
    while (c < cc) {
        const float *row = rows + c * N;
        float xi[4], m[4];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            xi[e] = row[n + e];
            m[e] = -INFINITY;
        }
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) m[e] = fmaxf(m[e], row[sidx[k * N + n + e]] - xi[e]);
        if (V == 4) {
            ElemIO<T>::store(ob + (size_t)(2 * c) * o_sc + n, xi, false);
            ElemIO<T>::store(ob + (size_t)(2 * c + 1) * o_sc + n, m, false);
        } else {
            ElemIO<T>::st1(ob + (size_t)(2 * c) * o_sc + n, xi[0]);
            ElemIO<T>::st1(ob + (size_t)(2 * c + 1) * o_sc + n, m[0]);
        }
        MR_NEXT(V, N, c, n);
    }
}

// Persistent 4-wide variant (N % 4 == 0, 4-element aligned strides/pointers -- every shape of the encoder): a
// workgroup stages the clip's edges ONCE and then walks several channel slabs of the clip, with the rows of the next
// slab already in flight (registers) while the current one is gathered out of LDS.  The one-slab-per-workgroup
// kernel above re-staged the 12 N bytes of edges for every 4 channel rows and exposed every load to latency.
constexpr int MRP_ITEMS = 4;                      // 4-element pieces per thread per slab: slab = 4096 elements
constexpr int MRP_SLAB = MRP_ITEMS * MR_THREADS * 4;

// WK: also write which neighbour won (first maximum, the rule of the backward pass) -- 2 bits per element, the four
// elements of a piece in one byte of arg (B, C, N / 4); K <= 4.  The backward pass then needs neither x nor the gather.
template <typename T, typename I, bool WK>
__global__ __launch_bounds__(MR_THREADS) void mrconv_fwd_p_kernel(const T *__restrict__ x, int64_t x_sb, int64_t x_sc,
                                                                  const I *__restrict__ idx, T *__restrict__ out,
                                                                  int64_t o_sb, int64_t o_sc, int C, int N, int K,
                                                                  int CC, unsigned char *__restrict__ arg, int plain) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.y, tid = threadIdx.x;
    float *rows = reinterpret_cast<float *>(smem);                 // [CC*N] (<= MRP_SLAB floats)
    int *sidx = reinterpret_cast<int *>(rows + MRP_SLAB);          // [K][N]
    const int nslab = (C + CC - 1) / CC;
    const T *xb = x + (size_t)b * x_sb;
    T *ob = out + (size_t)b * o_sb;
    int pc[MRP_ITEMS], pn[MRP_ITEMS];
    mr_pieces(tid, N, pc, pn);
    // SEVERAL slabs in flight per workgroup: with one, 5 workgroups x 8 KB per CU = 10 MB on the whole chip, and bytes
    // in flight / HBM latency (~3.5 us under load) is what the kernel ran at (3.5 TB/s).  The pieces wait in registers
    // as they were loaded (bf16: 8 bytes per piece instead of four floats), so the same 32 registers hold FOUR slabs of
    // bf16 -- all a workgroup has with the usual 16 slabs per clip -- or two of f32.
    typedef typename ElemIO<T>::Raw4 Raw;
    constexpr int NPAR = MR_NPAR<T>;
    Raw pv[NPAR][MRP_ITEMS];
    auto fetch = [&](int par, int slab) {
        const int c0 = slab * CC, cc = min(CC, C - c0);
#pragma unroll
        for (int it = 0; it < MRP_ITEMS; ++it)
            if (pc[it] < cc) pv[par][it] = GRAFP_LD_ONCE(32, reinterpret_cast<const Raw *>(xb + (size_t)(c0 + pc[it]) * x_sc + pn[it]));
    };
    int slab = blockIdx.x;
    const int G = gridDim.x;
#pragma unroll
    for (int par = 0; par < NPAR; ++par)
        if (slab + par * G < nslab) fetch(par, slab + par * G);
    stage_idx<I>(sidx, idx + (size_t)b * N * K, N, K, tid);
    while (slab < nslab) {
#pragma unroll
        for (int par = 0; par < NPAR; ++par) {
            if (slab < nslab) {                    // workgroup-uniform
                const int c0 = slab * CC, cc = min(CC, C - c0);
                __syncthreads();                   // previous slab fully consumed (and sidx staged, first time round)
                float xi[MRP_ITEMS][4];
#pragma unroll
                for (int it = 0; it < MRP_ITEMS; ++it) ElemIO<T>::unpack(pv[par][it], xi[it]);
#pragma unroll
                for (int it = 0; it < MRP_ITEMS; ++it)
                    if (pc[it] < cc)                   // one 16-byte LDS write per piece (N % 4 == 0: aligned)
                        *reinterpret_cast<float4 *>(rows + pc[it] * N + pn[it]) =
                            make_float4(xi[it][0], xi[it][1], xi[it][2], xi[it][3]);
                __syncthreads();
                if (slab + NPAR * G < nslab) fetch(par, slab + NPAR * G);
#pragma unroll
                for (int it = 0; it < MRP_ITEMS; ++it) {
                    if (pc[it] < cc) {
                        const float *row = rows + pc[it] * N;
                        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                        float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        unsigned bk = 0;
                        for (int k = 0; k < K; ++k) {
                            const int4 j4 = *reinterpret_cast<const int4 *>(sidx + k * N + pn[it]);
                            const float v[4] = {row[j4.x] - xi[it][0], row[j4.y] - xi[it][1], row[j4.z] - xi[it][2],
                                                row[j4.w] - xi[it][3]};
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                m[e] = fmaxf(m[e], v[e]);
                                if (WK && mr_first_max(k, v[e], best[e]))
                                    bk = (bk & ~(3u << (2 * e))) | ((unsigned)k << (2 * e));
                            }
                        }
                        if (WK) arg[((size_t)b * C + c0 + pc[it]) * (N / 4) + pn[it] / 4] = (unsigned char)bk;
                        T *o = ob + (size_t)(2 * (c0 + pc[it])) * o_sc + pn[it];
                        ElemIO<T>::store(o, xi[it], plain != 0);
                        ElemIO<T>::store(o + o_sc, m, plain != 0);
                    }
                }
                slab += G;
            }
        }
    }
}

// BWD_ITEMS * 256 * V elements per workgroup: the odd-channel gradients stay in registers between the
// accumulator initialisation and the scatter phase.
// Measured: small slabs (ITEMS = 2: 2048 elements, ~36 KB of LDS, 4 workgroups per CU) beat 8192-element ones by
// 25 %; ITEMS = 8 remains for N too long for a small slab to hold a whole channel row.

template <typename T, int V, typename I, int BWD_ITEMS>
__global__ __launch_bounds__(MR_THREADS) void mrconv_bwd_kernel(const T *__restrict__ x, int64_t x_sb, int64_t x_sc,
                                                                const I *__restrict__ idx,
                                                                const T *__restrict__ gout, int64_t g_sb, int64_t g_sc,
                                                                T *__restrict__ dx, int C, int N, int K, int CC) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned s_max[MR_THREADS / 64];
    const int b = blockIdx.y, c0 = blockIdx.x * CC, tid = threadIdx.x;
    const int cc = min(CC, C - c0);
    // 64-bit fixed-point scatter accumulator + integer LDS atomics (see mr_fix_encode): deterministic, and
    // ds_add_u64 is 30x the rate of ds_add_f32 on gfx950
    const size_t slab_al = ((size_t)CC * N + 1) & ~(size_t)1;
    long long *acc = reinterpret_cast<long long *>(smem);
    float *rows = reinterpret_cast<float *>(acc + slab_al);
    float *base = rows + slab_al;                                 // g_even - g_odd (identity branch minus the centre terms)
    int *sidx = reinterpret_cast<int *>(base + slab_al);
    const T *xb = x + (size_t)b * x_sb + (size_t)c0 * x_sc;
    const T *gb = gout + (size_t)b * g_sb + (size_t)(2 * c0) * g_sc;
    float godd[BWD_ITEMS][4];
    unsigned m = 0;
    {   // stage x; base <- g_even - g_odd
        MR_WALK(V, tid, N, c, n);
#pragma unroll
        for (int it = 0; it < BWD_ITEMS; ++it) {
            if (c < cc) {
                float v[4], ge[4];
                if (V == 4) {
                    ElemIO<T>::load(xb + (size_t)c * x_sc + n, v);
                    ElemIO<T>::load(gb + (size_t)(2 * c) * g_sc + n, ge);
                    ElemIO<T>::load(gb + (size_t)(2 * c + 1) * g_sc + n, godd[it]);
                } else {
                    v[0] = ld_as_f32(xb + (size_t)c * x_sc + n);
                    ge[0] = ld_as_f32(gb + (size_t)(2 * c) * g_sc + n);
                    godd[it][0] = ld_as_f32(gb + (size_t)(2 * c + 1) * g_sc + n);
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    rows[c * N + n + e] = v[e];
                    acc[c * N + n + e] = 0;
                    base[c * N + n + e] = ge[e] - godd[it][e];
                    m = max(m, __float_as_uint(godd[it][e]) & 0x7fffffffu);
                }
            }
            MR_NEXT(V, N, c, n);
        }
    }
    mr_scale_publish(m, s_max, tid);
    stage_idx<I>(sidx, idx + (size_t)b * N * K, N, K, tid);
    __syncthreads();
    const MrScale fx = mr_scale_read(s_max);
    if (!fx.poisoned) {   // route g_odd[c][m] to the arg-max neighbour of m (first maximum)
        MR_WALK(V, tid, N, c, n);
#pragma unroll
        for (int it = 0; it < BWD_ITEMS; ++it) {
            if (c < cc) {
                const float *row = rows + c * N;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float xi = row[n + e];
                    float best = 0.0f;
                    int bj = 0;
                    for (int k = 0; k < K; ++k) {
                        const int j = sidx[k * N + n + e];
                        if (mr_first_max(k, row[j] - xi, best)) bj = j;
                    }
                    atomicAdd(reinterpret_cast<unsigned long long *>(&acc[c * N + bj]), fx.encode(godd[it][e]));
                }
            }
            MR_NEXT(V, N, c, n);
        }
    }
    __syncthreads();
    T *db = dx + (size_t)b * x_sb + (size_t)c0 * x_sc;
    MR_WALK(V, tid, N, c, n);
    while (c < cc) {
        if (V == 4) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[e] = fx.out(base[c * N + n + e], (unsigned long long)acc[c * N + n + e]);
            ElemIO<T>::store(db + (size_t)c * x_sc + n, v, false);
        } else {
            ElemIO<T>::st1(db + (size_t)c * x_sc + n, fx.out(base[c * N + n], (unsigned long long)acc[c * N + n]));
        }
        MR_NEXT(V, N, c, n);
    }
}

// Persistent 4-wide backward (same conditions as mrconv_fwd_p_kernel): edges staged once per workgroup, slabs of
// 2048 elements (2 pieces per thread), the next slab's x / g_even / g_odd in flight while the current one scatters.
constexpr int MRB_ITEMS = 2;
constexpr int MRB_SLAB = MRB_ITEMS * MR_THREADS * 4;

template <typename T, typename I>
__global__ __launch_bounds__(MR_THREADS) void mrconv_bwd_p_kernel(const T *__restrict__ x, int64_t x_sb, int64_t x_sc,
                                                                  const I *__restrict__ idx,
                                                                  const T *__restrict__ gout, int64_t g_sb,
                                                                  int64_t g_sc, T *__restrict__ dx, int C, int N, int K,
                                                                  int CC) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned s_max[MR_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    long long *acc = reinterpret_cast<long long *>(smem);          // [CC*N] fixed-point scatter accumulator
    float *rows = reinterpret_cast<float *>(acc + MRB_SLAB);       // [CC*N] x
    int *sidx = reinterpret_cast<int *>(rows + MRB_SLAB);          // [K][N]
    const int nslab = (C + CC - 1) / CC;
    const T *xb = x + (size_t)b * x_sb;
    const T *gb = gout + (size_t)b * g_sb;
    T *db = dx + (size_t)b * x_sb;
    int pc[MRB_ITEMS], pn[MRB_ITEMS];
    mr_pieces(tid, N, pc, pn);
    float pv[MRB_ITEMS][4], pe[MRB_ITEMS][4], po[MRB_ITEMS][4];     // x, g_even, g_odd of the slab in flight
    auto fetch = [&](int slab) {
        const int c0 = slab * CC, cc = min(CC, C - c0);
#pragma unroll
        for (int it = 0; it < MRB_ITEMS; ++it)
            if (pc[it] < cc) {
                const int c = c0 + pc[it];
                ElemIO<T>::load(xb + (size_t)c * x_sc + pn[it], pv[it]);
                ElemIO<T>::load(gb + (size_t)(2 * c) * g_sc + pn[it], pe[it]);
                ElemIO<T>::load(gb + (size_t)(2 * c + 1) * g_sc + pn[it], po[it]);
            }
    };
    int slab = blockIdx.x;
    if (slab < nslab) fetch(slab);
    stage_idx<I>(sidx, idx + (size_t)b * N * K, N, K, tid);
    for (; slab < nslab; slab += gridDim.x) {
        const int c0 = slab * CC, cc = min(CC, C - c0);
        __syncthreads();                       // previous slab written out (and sidx staged, first time round)
        float xi[MRB_ITEMS][4], godd[MRB_ITEMS][4], base[MRB_ITEMS][4];
        unsigned m = 0;
#pragma unroll
        for (int it = 0; it < MRB_ITEMS; ++it)
            if (pc[it] < cc) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    rows[pc[it] * N + pn[it] + e] = pv[it][e];
                    acc[pc[it] * N + pn[it] + e] = 0;
                    base[it][e] = pe[it][e] - po[it][e];       // identity branch minus the centre terms
                    xi[it][e] = pv[it][e];
                    godd[it][e] = po[it][e];
                    m = max(m, __float_as_uint(po[it][e]) & 0x7fffffffu);
                }
            }
        mr_scale_publish(m, s_max, tid);
        __syncthreads();
        if (slab + gridDim.x < nslab) fetch(slab + gridDim.x);
        const MrScale fx = mr_scale_read(s_max);
        // route g_odd[c][m] to the arg-max neighbour of m (first maximum)
#pragma unroll
        for (int it = 0; it < MRB_ITEMS; ++it) {
            if (pc[it] < cc) {
                const float *row = rows + pc[it] * N;
                float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                int bj[4];
                for (int k = 0; k < K; ++k) {
                    const int4 j4 = *reinterpret_cast<const int4 *>(sidx + k * N + pn[it]);
                    const int jj[4] = {j4.x, j4.y, j4.z, j4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (mr_first_max(k, row[jj[e]] - xi[it][e], best[e])) bj[e] = jj[e];
                }
                if (!fx.poisoned) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        atomicAdd(reinterpret_cast<unsigned long long *>(&acc[pc[it] * N + bj[e]]), fx.encode(godd[it][e]));
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < MRB_ITEMS; ++it)
            if (pc[it] < cc) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v[e] = fx.out(base[it][e], (unsigned long long)acc[pc[it] * N + pn[it] + e]);
                ElemIO<T>::store(db + (size_t)(c0 + pc[it]) * x_sc + pn[it], v, false);
            }
    }
}

// Backward from the recorded arg-max (mrconv_fwd_p_kernel<WK>): no x, no gather.  Per element: one byte-quarter, one
// fixed-point LDS atomic.  LDS: i64 accumulator slab | edges [K][N].  A thread owns 4 CONSECUTIVE elements, so every
// per-element LDS access of a wave strides 16 or 32 bytes per lane (PMC, first version: 70 % of the LDS-active cycles
// were bank conflicts, the LDS busy 60 % of the kernel): the accumulator is zeroed and read back as 16-byte vectors and
// the K edges of the thread's four nodes come as K 16-byte reads, selected in registers.
template <typename T, typename I>
__global__ __launch_bounds__(MR_THREADS) void mrconv_bwd_a_kernel(const unsigned char *__restrict__ arg,
                                                                  const I *__restrict__ idx,
                                                                  const T *__restrict__ gout, int64_t g_sb,
                                                                  int64_t g_sc, T *__restrict__ dx, int64_t d_sb,
                                                                  int64_t d_sc, int C, int N, int K, int CC, int plain) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned s_max[MR_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(smem);     // [CC*N] fixed-point scatter accumulator
    int *sidx = reinterpret_cast<int *>(acc + MRB_SLAB);                         // [K][N]
    const int nslab = (C + CC - 1) / CC;
    // this thread's pieces inside a slab: element offset pc * N + pn, node pn
    int off[MRB_ITEMS], pn[MRB_ITEMS], pc[MRB_ITEMS];
    mr_pieces(tid, N, pc, pn);
#pragma unroll
    for (int it = 0; it < MRB_ITEMS; ++it) off[it] = pc[it] * N + pn[it];
    // running pointers of the pieces: slab s -> s + gridDim.x moves them by a constant
    const T *ge_p[MRB_ITEMS];
    T *dx_p[MRB_ITEMS];
    const unsigned char *ar_p[MRB_ITEMS];
    const int64_t cstep = (int64_t)gridDim.x * CC;
#pragma unroll
    for (int it = 0; it < MRB_ITEMS; ++it) {
        const int64_t c = (int64_t)blockIdx.x * CC + pc[it];
        ge_p[it] = gout + (size_t)b * g_sb + (size_t)(2 * c) * g_sc + pn[it];
        dx_p[it] = dx + (size_t)b * d_sb + (size_t)c * d_sc + pn[it];
        ar_p[it] = arg + ((size_t)b * C + c) * (N / 4) + pn[it] / 4;
    }
    const int64_t ge_step = 2 * cstep * g_sc, dx_step = cstep * d_sc, ar_step = cstep * (N / 4);
    // g_even, g_odd of the slabs in flight, as loaded (bf16: four slabs in the registers two took unpacked; see
    // mrconv_fwd_p_kernel -- the kernel runs at bytes in flight / latency)
    typedef typename ElemIO<T>::Raw4 Raw;
    constexpr int NPAR = MR_NPAR<T>;
    Raw pe[NPAR][MRB_ITEMS], po[NPAR][MRB_ITEMS];
    unsigned pa[NPAR][MRB_ITEMS];
    auto fetch = [&](int par, int slab) {                          // slabs are fetched in order, each G after the last
        const int cc = min(CC, C - slab * CC);
#pragma unroll
        for (int it = 0; it < MRB_ITEMS; ++it) {
            if (pc[it] < cc) {
                pe[par][it] = GRAFP_LD_ONCE(16, reinterpret_cast<const Raw *>(ge_p[it]));
                po[par][it] = GRAFP_LD_ONCE(16, reinterpret_cast<const Raw *>(ge_p[it] + g_sc));
                pa[par][it] = *ar_p[it];
            }
            ge_p[it] += ge_step;
            ar_p[it] += ar_step;
        }
    };
    int slab = blockIdx.x;
    const int G = gridDim.x;
#pragma unroll
    for (int par = 0; par < NPAR; ++par)
        if (slab + par * G < nslab) fetch(par, slab + par * G);
    stage_idx<I>(sidx, idx + (size_t)b * N * K, N, K, tid);
    while (slab < nslab) {
#pragma unroll
        for (int par = 0; par < NPAR; ++par) {
            if (slab < nslab) {                    // workgroup-uniform
                const int cc = min(CC, C - slab * CC);
                __syncthreads();                   // previous slab written out (and the edges staged, first time round)
                float godd[MRB_ITEMS][4], base[MRB_ITEMS][4];
                unsigned ak[MRB_ITEMS];
                unsigned m = 0;
#pragma unroll
                for (int it = 0; it < MRB_ITEMS; ++it)
                    if (pc[it] < cc) {
                        ak[it] = pa[par][it];
                        *reinterpret_cast<uint4 *>(acc + off[it]) = make_uint4(0, 0, 0, 0);
                        *reinterpret_cast<uint4 *>(acc + off[it] + 2) = make_uint4(0, 0, 0, 0);
                        float ge[4];
                        ElemIO<T>::unpack(pe[par][it], ge);
                        ElemIO<T>::unpack(po[par][it], godd[it]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            base[it][e] = ge[e] - godd[it][e];               // identity branch minus the centre terms
                            m = max(m, __float_as_uint(godd[it][e]) & 0x7fffffffu);
                        }
                    }
                mr_scale_publish(m, s_max, tid);
                __syncthreads();
                if (slab + NPAR * G < nslab) fetch(par, slab + NPAR * G);
                const MrScale fx = mr_scale_read(s_max);
                if (!fx.poisoned) {
#pragma unroll
                    for (int it = 0; it < MRB_ITEMS; ++it)
                        if (pc[it] < cc) {
                            unsigned long long *arow = acc + (off[it] - pn[it]);
                            // the winner's edge of each of the 4 nodes: K vector reads, selected in registers
                            int bj[4] = {0, 0, 0, 0};
                            for (int k = 0; k < K; ++k) {
                                const int4 j4 = *reinterpret_cast<const int4 *>(sidx + k * N + pn[it]);
                                const int jj[4] = {j4.x, j4.y, j4.z, j4.w};
#pragma unroll
                                for (int e = 0; e < 4; ++e) bj[e] = ((ak[it] >> (2 * e)) & 3u) == (unsigned)k ? jj[e] : bj[e];
                            }
#pragma unroll
                            for (int e = 0; e < 4; ++e) atomicAdd(arow + bj[e], fx.encode(godd[it][e]));
                        }
                }
                __syncthreads();
#pragma unroll
                for (int it = 0; it < MRB_ITEMS; ++it) {
                    if (pc[it] < cc) {
                        float v[4];
                        const uint4 a01 = *reinterpret_cast<const uint4 *>(acc + off[it]);
                        const uint4 a23 = *reinterpret_cast<const uint4 *>(acc + off[it] + 2);
                        const unsigned long long a[4] = {((unsigned long long)a01.y << 32) | a01.x,
                                                         ((unsigned long long)a01.w << 32) | a01.z,
                                                         ((unsigned long long)a23.y << 32) | a23.x,
                                                         ((unsigned long long)a23.w << 32) | a23.z};
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fx.out(base[it][e], a[e]);
                        ElemIO<T>::store(dx_p[it], v, plain != 0);
                    }
                    dx_p[it] += dx_step;
                }
                slab += G;
            }
        }
    }
}

// ---- host: the launch choice, made once: a pure function of (strides, shape, alignment, direction, record wanted) that the
// forward and backward launchers, the two record entries, grafp_mrconv_arg_supported and grafp_mrconv_plan all ask ----------
enum { MR_PATH_PERSISTENT = 0, MR_PATH_VEC4 = 1, MR_PATH_SCALAR = 2, MR_PATH_RECORD = 3 };
struct MrLaunch {
    int path;          // persistent 4-wide | generic 4-wide | generic scalar | persistent with the arg-max record (fwd<WK> / bwd_a)
    int items;         // pieces (elements, scalar) a thread holds per slab; 0 = the generic forward, whose threads stride
    int cc;            // channel rows per slab
    int nslab, per_clip;   // slabs per clip; workgroups per clip (grid.x): one per slab for the generic kernels
    size_t lds;        // dynamic LDS bytes
};
constexpr size_t MR_LDS_LIMIT = 160 * 1024;                   // of a gfx950 workgroup
constexpr int MR_FWD_ELEMS = 4096;   // generic forward; measured: 28 KB of LDS per workgroup (5 per CU) beats the 76 KB slab by 35 %
static_assert(MRB_SLAB <= MRP_SLAB, "a row that fits the backward slab fits the forward one");

static inline int mr_clamp_cc(int cc, int C) { return cc < 1 ? 1 : (cc > C ? C : cc); }

// x_s*: strides of x (forward) and of dx; o_s*: strides of out (forward) or grad_out (backward).  aligned: every activation
// pointer of the call is 4-element aligned.  with_arg: the caller wants the arg-max record; where the shape cannot have one
// the answer is the launch of the plain call, which fwd_arg / bwd_arg refuse.  Shape and dtype are checked (mr_check_args).
static int mr_choose(int64_t x_sb, int64_t x_sc, int64_t o_sb, int64_t o_sc, int N, int K, int C, int B,
                     bool aligned, bool backward, bool with_arg, MrLaunch *L) {
    const bool v4 = aligned && N % 4 == 0 && x_sb % 4 == 0 && x_sc % 4 == 0 && o_sb % 4 == 0 && o_sc % 4 == 0;
    const size_t edges = (size_t)K * N;
    // dynamic LDS of each kernel, in 4-byte words: fwd_p rows | edges; bwd_p i64 accumulator + rows | edges; bwd_a i64
    // accumulator | edges; generic: rows (+ i64 accumulator + identity term, slab rounded to even) | edges
    const size_t lds_fwd_p = (MRP_SLAB + edges) * 4, lds_bwd_p = (3 * (size_t)MRB_SLAB + edges) * 4,
                 lds_bwd_a = (2 * (size_t)MRB_SLAB + edges) * 4;
    auto lds_generic = [&](int cc) {
        const size_t slab = (size_t)cc * N;
        return (backward ? 4 * ((slab + 1) & ~(size_t)1) + edges : slab + edges) * 4;
    };
    // the record: 2 bits per edge number, written by the persistent forward and read by bwd_a -- both must be able to run
    const bool record = with_arg && v4 && K <= 4 && N <= MRB_SLAB && lds_fwd_p <= MR_LDS_LIMIT && lds_bwd_a <= MR_LDS_LIMIT;
    const int slab = backward ? MRB_SLAB : MRP_SLAB;
    const size_t lds_p = !backward ? lds_fwd_p : (record ? lds_bwd_a : lds_bwd_p);
    if (record || (v4 && N <= slab && lds_p <= MR_LDS_LIMIT)) {
        // whole channel rows per slab, shared among 4 workgroups per clip, more while the grid has fewer than 1024 workgroups
        *L = {record ? MR_PATH_RECORD : MR_PATH_PERSISTENT, backward ? MRB_ITEMS : MRP_ITEMS, std::min(slab / N, C), 0, 0, lds_p};
        L->nslab = (C + L->cc - 1) / L->cc;
        L->per_clip = L->nslab < 4 ? L->nslab : 4;
        while ((int64_t)L->per_clip * B < 1024 && L->per_clip < L->nslab) ++L->per_clip;
        return GRAFP_OK;
    }
    // generic: one slab of whole channel rows per workgroup; backward, it covers exactly items * 256 * V elements (the
    // odd-channel gradients wait in registers)
    int items = 0, cc = mr_clamp_cc(MR_FWD_ELEMS / N, C);
    if (backward) {
        const int per_item = MR_THREADS * (v4 ? 4 : 1);
        items = N <= 2 * per_item ? 2 : 8;
        cc = mr_clamp_cc(items * per_item / N, C);
        GRAFP_REQUIRE((size_t)cc * N <= (size_t)items * per_item, "mrconv_bwd: N=%d exceeds the %d nodes a workgroup covers", N,
                      items * per_item);
        while (cc > 1 && lds_generic(cc) > MR_LDS_LIMIT) --cc;
    }
    GRAFP_REQUIRE(lds_generic(cc) <= MR_LDS_LIMIT, "mrconv_%s: N=%d K=%d needs %zu B of LDS (> 160 KiB)",
                  backward ? "bwd" : "fwd", N, K, lds_generic(cc));
    *L = {v4 ? MR_PATH_VEC4 : MR_PATH_SCALAR, items, cc, (C + cc - 1) / cc, (C + cc - 1) / cc, lds_generic(cc)};
    return GRAFP_OK;
}

// what every entry asks of its arguments; op names the entry in the message
static int mr_check_args(const char *op, bool pointers, int dtype, int B, int C, int N, int K) {
    GRAFP_REQUIRE(pointers, "%s: null pointer", op);
    GRAFP_REQUIRE(B > 0 && C > 0 && N > 0 && K > 0, "%s: bad shape B=%d C=%d N=%d K=%d", op, B, C, N, K);
    GRAFP_REQUIRE(dtype == GRAFP_F32 || dtype == GRAFP_BF16, "%s: dtype %d not in {f32, bf16}", op, dtype);
    return GRAFP_OK;
}

static bool mr_aligned(int dtype, const void *a, const void *b, const void *c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % (dtype == GRAFP_F32 ? 16 : 8)) == 0;
}

// one launch: per_clip x B workgroups of MR_THREADS with L.lds bytes of dynamic LDS (above the 64 KiB a kernel gets unasked)
template <typename Kern, typename... Args>
static int mr_launch(const char *name, Kern kern, const MrLaunch &L, int B, grafp_stream_t stream, Args... args) {
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds);
    hipLaunchKernelGGL(kern, dim3(L.per_clip, B), dim3(MR_THREADS), L.lds, (hipStream_t)stream, args...);
    GRAFP_CHECK_LAUNCH(name);
    return GRAFP_OK;
}

}  // namespace grafp

// arg != nullptr: the forward of grafp_mrconv_fwd_arg (op names the entry)
static int mrconv_fwd_impl(const char *op, const void *x, int dtype, int64_t x_sb, int64_t x_sc, const void *idx, int idx32,
                           int B, int C, int N, int K, void *out, int64_t o_sb, int64_t o_sc, grafp_stream_t stream,
                           unsigned char *arg = nullptr) {
    using namespace grafp;
    if (int e = mr_check_args(op, x && idx && out, dtype, B, C, N, K)) return e;
    MrLaunch L;
    if (int e = mr_choose(x_sb, x_sc, o_sb, o_sc, N, K, C, B, mr_aligned(dtype, x, out), false, arg != nullptr, &L)) return e;
    GRAFP_REQUIRE(!arg || L.path == MR_PATH_RECORD,
                  "mrconv_fwd_arg: shape / alignment outside grafp_mrconv_arg_supported (N=%d K=%d)", N, K);
    int rc = GRAFP_OK;
    for_elem_idx(dtype, idx32, [&](auto te, auto ti) {
        using T = typename decltype(te)::type;
        using I = typename decltype(ti)::type;
        if (L.path == MR_PATH_PERSISTENT || L.path == MR_PATH_RECORD) {
            const int plain = plain_stores((size_t)2 * B * C * N * sizeof(T), "GRAFP_MR_PLAIN_MAX_MB", 140);
            for_bool(arg != nullptr, [&](auto wk) {
                rc = mr_launch("mrconv_fwd_p_kernel", mrconv_fwd_p_kernel<T, I, decltype(wk)::value>, L, B, stream, (const T *)x,
                               x_sb, x_sc, (const I *)idx, (T *)out, o_sb, o_sc, C, N, K, L.cc, arg, plain);
            });
        } else {
            for_bool(L.path == MR_PATH_VEC4, [&](auto vec) {
                rc = mr_launch("mrconv_fwd_kernel", mrconv_fwd_kernel<T, decltype(vec)::value ? 4 : 1, I>, L, B, stream,
                               (const T *)x, x_sb, x_sc, (const I *)idx, (T *)out, o_sb, o_sc, C, N, K, L.cc);
            });
        }
    });
    return rc;
}

// arg != nullptr: the backward of grafp_mrconv_bwd_arg, which reads the record and not x
static int mrconv_bwd_impl(const char *op, const void *x, const unsigned char *arg, int dtype, int64_t x_sb, int64_t x_sc,
                           const void *idx, int idx32, const void *grad_out, int64_t g_sb, int64_t g_sc, int B, int C, int N,
                           int K, void *dx, grafp_stream_t stream) {
    using namespace grafp;
    if (int e = mr_check_args(op, (x || arg) && idx && grad_out && dx, dtype, B, C, N, K)) return e;
    MrLaunch L;
    if (int e = mr_choose(x_sb, x_sc, g_sb, g_sc, N, K, C, B, mr_aligned(dtype, x, grad_out, dx), true, arg != nullptr, &L)) return e;
    GRAFP_REQUIRE(!arg || L.path == MR_PATH_RECORD,
                  "mrconv_bwd_arg: shape / alignment outside grafp_mrconv_arg_supported (N=%d K=%d)", N, K);
    int rc = GRAFP_OK;
    for_elem_idx(dtype, idx32, [&](auto te, auto ti) {
        using T = typename decltype(te)::type;
        using I = typename decltype(ti)::type;
        if (L.path == MR_PATH_RECORD) {
            const int plain = plain_stores((size_t)B * C * N * sizeof(T), "GRAFP_MR_PLAIN_MAX_MB", 140);
            rc = mr_launch("mrconv_bwd_a_kernel", mrconv_bwd_a_kernel<T, I>, L, B, stream, arg, (const I *)idx,
                           (const T *)grad_out, g_sb, g_sc, (T *)dx, x_sb, x_sc, C, N, K, L.cc, plain);
        } else if (L.path == MR_PATH_PERSISTENT) {
            rc = mr_launch("mrconv_bwd_p_kernel", mrconv_bwd_p_kernel<T, I>, L, B, stream, (const T *)x, x_sb, x_sc,
                           (const I *)idx, (const T *)grad_out, g_sb, g_sc, (T *)dx, C, N, K, L.cc);
        } else {
            for_bool(L.path == MR_PATH_VEC4, [&](auto vec) {
                for_bool(L.items == 2, [&](auto two) {
                    rc = mr_launch("mrconv_bwd_kernel",
                                   mrconv_bwd_kernel<T, decltype(vec)::value ? 4 : 1, I, decltype(two)::value ? 2 : 8>, L, B,
                                   stream, (const T *)x, x_sb, x_sc, (const I *)idx, (const T *)grad_out, g_sb, g_sc, (T *)dx,
                                   C, N, K, L.cc);
                });
            });
        }
    });
    return rc;
}

extern "C" int grafp_mrconv_fwd_strided(const void *x, int dtype, int64_t x_sb, int64_t x_sc, const int64_t *idx, int B,
                                        int C, int N, int K, void *out, int64_t o_sb, int64_t o_sc,
                                        grafp_stream_t stream) {
    return mrconv_fwd_impl("mrconv_fwd", x, dtype, x_sb, x_sc, idx, 0, B, C, N, K, out, o_sb, o_sc, stream);
}
extern "C" int grafp_mrconv_fwd_strided_i32(const void *x, int dtype, int64_t x_sb, int64_t x_sc, const int32_t *idx,
                                            int B, int C, int N, int K, void *out, int64_t o_sb, int64_t o_sc,
                                            grafp_stream_t stream) {
    return mrconv_fwd_impl("mrconv_fwd", x, dtype, x_sb, x_sc, idx, 1, B, C, N, K, out, o_sb, o_sc, stream);
}
extern "C" int grafp_mrconv_bwd_strided(const void *x, int dtype, int64_t x_sb, int64_t x_sc, const int64_t *idx,
                                        const void *grad_out, int64_t g_sb, int64_t g_sc, int B, int C, int N, int K,
                                        void *dx, grafp_stream_t stream) {
    return mrconv_bwd_impl("mrconv_bwd", x, nullptr, dtype, x_sb, x_sc, idx, 0, grad_out, g_sb, g_sc, B, C, N, K, dx, stream);
}
extern "C" int grafp_mrconv_bwd_strided_i32(const void *x, int dtype, int64_t x_sb, int64_t x_sc, const int32_t *idx,
                                            const void *grad_out, int64_t g_sb, int64_t g_sc, int B, int C, int N,
                                            int K, void *dx, grafp_stream_t stream) {
    return mrconv_bwd_impl("mrconv_bwd", x, nullptr, dtype, x_sb, x_sc, idx, 1, grad_out, g_sb, g_sc, B, C, N, K, dx, stream);
}

extern "C" int grafp_mrconv_plan(int dtype, int64_t x_sb, int64_t x_sc, int64_t o_sb, int64_t o_sc, int B, int C, int N,
                                 int K, int aligned, int backward, int with_arg, int *info) {
    using namespace grafp;
    if (int e = mr_check_args("mrconv_plan", info != nullptr, dtype, B, C, N, K)) return e;
    MrLaunch L;
    if (int e = mr_choose(x_sb, x_sc, o_sb, o_sc, N, K, C, B, aligned != 0, backward != 0, with_arg != 0, &L)) return e;
    const int out[8] = {L.path, L.items, L.cc, L.nslab, L.per_clip, (int)L.lds, 0, 0};
    for (int i = 0; i < 8; ++i) info[i] = out[i];
    return GRAFP_OK;
}

// the shapes whose forward can record the arg-max and whose backward can run from it (pointer alignment aside)
extern "C" int grafp_mrconv_arg_supported(int dtype, int64_t x_sb, int64_t x_sc, int64_t o_sb, int64_t o_sc, int N, int K) {
    using namespace grafp;
    MrLaunch L;
    return (dtype == GRAFP_F32 || dtype == GRAFP_BF16) && N > 0 && K >= 1 &&
           mr_choose(x_sb, x_sc, o_sb, o_sc, N, K, 1, 1, true, false, true, &L) == GRAFP_OK && L.path == MR_PATH_RECORD;
}
extern "C" int grafp_mrconv_fwd_arg(const void *x, int dtype, int64_t x_sb, int64_t x_sc, const void *idx, int idx_is_i32,
                                    int B, int C, int N, int K, void *out, int64_t o_sb, int64_t o_sc, uint8_t *arg,
                                    grafp_stream_t stream) {
    GRAFP_REQUIRE(arg, "mrconv_fwd_arg: null pointer");
    return mrconv_fwd_impl("mrconv_fwd_arg", x, dtype, x_sb, x_sc, idx, idx_is_i32, B, C, N, K, out, o_sb, o_sc, stream, arg);
}
extern "C" int grafp_mrconv_bwd_arg(const uint8_t *arg, int dtype, const void *idx, int idx_is_i32, const void *grad_out,
                                    int64_t g_sb, int64_t g_sc, int B, int C, int N, int K, void *dx, int64_t d_sb,
                                    int64_t d_sc, grafp_stream_t stream) {
    GRAFP_REQUIRE(arg, "mrconv_bwd_arg: null pointer");
    return mrconv_bwd_impl("mrconv_bwd_arg", nullptr, arg, dtype, d_sb, d_sc, idx, idx_is_i32, grad_out, g_sb, g_sc, B, C, N, K, dx,
                           stream);
}

extern "C" int grafp_mrconv_fwd_f32(const float *x, const int64_t *idx, int B, int C, int N, int K, float *out,
                                    grafp_stream_t stream) {
    return grafp_mrconv_fwd_strided(x, GRAFP_F32, (int64_t)C * N, N, idx, B, C, N, K, out, (int64_t)2 * C * N, N, stream);
}

extern "C" int grafp_mrconv_bwd_f32(const float *x, const int64_t *idx, const float *grad_out, int B, int C, int N,
                                    int K, float *dx, grafp_stream_t stream) {
    return grafp_mrconv_bwd_strided(x, GRAFP_F32, (int64_t)C * N, N, idx, grad_out, (int64_t)2 * C * N, N, B, C, N, K, dx,
                                    stream);
}
