// bn.hip -- fused [conv bias] + BatchNorm + activation + residual on the (C, M = B*N) activation layout, gfx950.
//
// Replaces, around every 1x1 convolution of the GraFPrint encoder, the chain the reference runs as separate
// library/elementwise launches: `+ bias` (Conv2d bias), BatchNorm2d (batch statistics in train mode,
// /root/reference/encoder/gcn_lib/torch_vertex.py:152-162, torch_nn.py:56-60, encoder/graph_encoder.py:52-55,131-133),
// ReLU / LeakyReLU(0.2), and the residual add (`torch_vertex.py:193`, `graph_encoder.py:65`).
// With channels as ROWS of a (C, M) matrix a channel's statistics are a reduction over one contiguous row:
//   forward  = stats pass (1 read) + apply pass (1 read [+1 residual read] + 1 write)
//   backward = reduce pass (2 reads) + dx pass (2 reads + 1 write); the activation mask is recomputed, not stored.
// HBM-bound: 12 (f32) / 6 (bf16) bytes per element forward.  Statistics use shifted sums (shift = first element
// of the row) in f32, which removes the E[x^2] - E[x]^2 cancellation for rows with |mean| >> std.
// A conv bias in front of a train-mode BatchNorm cancels in the output; it only shifts the running mean, and its
// gradient is exactly zero -- so it is folded in here instead of costing an elementwise launch + a reduction.
// Six kernels (two-pass: stats, apply, bwd_reduce, bwd_dx, on vectors or element by element; single pass: fwd1, bwd1) in
// 24 instantiations.  What they have in common is written once, in front of them: the chunk a workgroup or slot covers
// (BnChunk), the two walks over a chunk (bn_walk, bn1_walk), the shifted sums (bn_shifted_sums), the statistics of a view
// and the running-statistics advance from partial pairs in global memory or LDS (bn_view_stats, bn_advance_running), the
// forward element (BnNorm, bn_act_res), the two backward elements (BnGrad, BnGradFolded) and, for the single pass, the
// rendezvous (bn1_rendezvous).  A kernel states only its own per-element body.
#include <math.h>

#include <type_traits>

#define GRAFP_STORE_FAMILY 1        // (common.h: GRAFP_ST_NT experiment builds)
#include "elemio.h"

namespace grafp {

constexpr int BN_THREADS = 256;

// dY of the BatchNorm backward is read twice by the two launches that follow it (data gradient and weight gradient of
// the convolution in front): its store hint is plain_stores("GRAFP_BN_BWD_PLAIN_MAX_MB") of elemio.h.

template <int THREADS = 256>
__device__ __forceinline__ float2 block_sum2(float a, float b, float2 *scratch, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    __syncthreads();
    if ((tid & 63) == 0) scratch[tid >> 6] = make_float2(a, b);
    __syncthreads();
    float2 r = scratch[0];
    for (int w = 1; w < THREADS / 64; ++w) {
        r.x += scratch[w].x;
        r.y += scratch[w].y;
    }
    return r;
}

__device__ __forceinline__ float act_grad(float u, int act, float slope) {
    return act == 0 ? 1.0f : (u > 0.0f ? 1.0f : (act == 1 ? 0.0f : slope));
}

// The forward folds the normalisation into ONE fma per element, z = act(fma(x, g, off)) with g = gamma invstd and
// off = beta + (pb - mean) g.  off is rounded at the magnitude of (mean - pb) g, so a row whose mean lies hundreds of
// standard deviations from zero -- a constant non-zero row: invstd = 1/sqrt(eps) -- would lose that much of a result of
// magnitude beta (measured on a row constant at 3.0: 9.4e-5 against float64).  Such rows subtract first,
// fma((x + pb) - mean, g, beta) (x + pb rounds as the statistics' shift did, so the difference is exact where it
// cancels).  The choice is uniform over a row and view; rows of ordinary statistics keep the folded form and its bits.
constexpr float BN_FOLD_MAX = 64.0f;      // folded form up to |(mean - pb) g| = 64: 2 ulp(64) = 1.5e-5 absolute at most
struct BnNorm {
    float g, off, pb, mean, be;
    __device__ __forceinline__ bool centred() const { return fabsf((mean - pb) * g) > BN_FOLD_MAX; }
    template <bool CENTRED>
    __device__ __forceinline__ float pre(float x) const {
        return CENTRED ? __builtin_fmaf((x + pb) - mean, g, be) : __builtin_fmaf(x, g, off);
    }
    __device__ __forceinline__ static BnNorm make(float ga, float be, float pb, float mean, float invstd) {
        const float g = ga * invstd;
        return {g, be + (pb - mean) * g, pb, mean, be};      // z = act(x*g + off) + r
    }
};
// the N elements of a piece: normalise, activate, add the shortcut
template <bool CENTRED, int N>
__device__ __forceinline__ void bn_act_res(const BnNorm &nrm, int act, float slope, bool res, float (&v)[N], const float (&r)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        v[i] = act_fwd(nrm.template pre<CENTRED>(v[i]), act, slope);
        if (res) v[i] += r[i];
    }
}

// ---- what the six kernels share: the arithmetic of each formula below is written here only --------------------------------
// (two loops are still spelled in their kernels, around the shared arithmetic: the unrolled-by-4 loop of bn_apply_kernel
//  next to its bn_walk, and the last walk of bn_fwd1_kernel, which repeats bn1_walk's position for the reason given there)
// Chunk `i` of a row (a workgroup's own: i = blockIdx.x; a row-mate's: its slot): view grp, chunk sl of that view,
// columns [lo, hi) of the row.  Sg chunks of `chunk` elements per view of Mg columns; the last one may be shorter.
struct BnChunk {
    int grp, sl;
    int64_t lo, hi;
    __device__ __forceinline__ BnChunk(int i, int Sg, int64_t chunk, int64_t Mg) {
        grp = i / Sg;
        sl = i - grp * Sg;
        const int64_t gend = (int64_t)(grp + 1) * Mg;
        lo = (int64_t)grp * Mg + (int64_t)sl * chunk;
        hi = (lo + chunk < gend) ? lo + chunk : gend;
    }
};

// N = 1 or ElemIO<T>::W elements, as the walks hand them out
template <typename T, int N> __device__ __forceinline__ void bn_load(const T *p, float (&v)[N]) {
    if constexpr (N == 1) v[0] = ElemIO<T>::ld1(p);
    else ElemIO<T>::load(p, v);
}
template <typename T, int N> __device__ __forceinline__ void bn_store(T *p, const float (&v)[N]) {
    if constexpr (N == 1) ElemIO<T>::st1(p, v[0]);
    else ElemIO<T>::store(p, v, false);
}

// The strided walk of the two-pass kernels: the workgroup's threads cover [.., hi) W elements at a time from the thread's
// first position m.  body(m, n) gets a whole vector (n = W) while one fits, else the remaining elements one by one (n = 1).
template <int W, typename Body> __device__ __forceinline__ void bn_walk(int64_t m, int64_t hi, Body body) {
    for (; m < hi; m += (int64_t)BN_THREADS * W) {
        if (W > 1 && m + W <= hi) {
            body(m, std::integral_constant<int, W>{});
        } else {
            for (int i = 0; i < W && m + i < hi; ++i) body(m + i, std::integral_constant<int, 1>{});
        }
    }
}
// The register-resident walk of the single-pass kernels: item `it` of a thread is the vector at m; body(it, m).
template <int ITEMS, int THREADS, int W, typename Body>
__device__ __forceinline__ void bn1_walk(int64_t lo, int64_t hi, Body body) {
    const int tid = threadIdx.x;        // read HERE: as a parameter its range is unknown when this function is first optimised
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int64_t m = lo + ((int64_t)it * THREADS + tid) * W;
        if (m < hi) body(it, m);
    }
}

// Forward statistics are shifted sums: a = sum d, q = sum d^2 with d = (x + pb) - shift, shift = the view's first element.
template <typename T> __device__ __forceinline__ float bn_shift(const T *row, int g, int64_t Mg, float pb) {
    return ElemIO<T>::ld1(row + (int64_t)g * Mg) + pb;
}
template <int N>
__device__ __forceinline__ void bn_shifted_sums(const float (&v)[N], float pb, float shift, float &a, float &q) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float d = (v[i] + pb) - shift;
        a += d;
        q = __builtin_fmaf(d, d, q);
    }
}

// Partial pairs, one per chunk of a row: in global memory (two-pass: `part`) or in LDS (single pass: `sp`).  A reader is
// anything that returns pair i of the row as a float2.
struct BnPart {
    const float *part;
    size_t row0;            // c * S
    __device__ __forceinline__ float2 operator()(int i) const {
        return make_float2(part[(row0 + i) * 2 + 0], part[(row0 + i) * 2 + 1]);
    }
};
__device__ __forceinline__ void bn_put_pair(float *part, size_t i, float2 r) {
    part[i * 2 + 0] = r.x;
    part[i * 2 + 1] = r.y;
}
template <typename Pairs> __device__ __forceinline__ float2 bn_sum_pairs(Pairs pair, int i0, int i1) {
    float a = 0.0f, b = 0.0f;
    for (int i = i0; i < i1; ++i) {         // index order: the same sum in every workgroup that forms it
        const float2 p = pair(i);
        a += p.x;
        b += p.y;
    }
    return make_float2(a, b);
}
// (mean, biased variance) of view g from its Sg pairs of shifted sums
template <typename Pairs>
__device__ __forceinline__ float2 bn_view_mean_var(Pairs pair, int g, int Sg, int64_t Mg, float shift) {
    const float2 t = bn_sum_pairs(pair, g * Sg, (g + 1) * Sg);
    const float dm = t.x / (float)Mg;
    const float var = relu_keep_nan(t.y / (float)Mg - dm * dm);
    return make_float2(shift + dm, var);
}
template <typename Pairs>
__device__ __forceinline__ void bn_view_stats(Pairs pair, int g, int Sg, int64_t Mg, float shift, float eps, float &mean,
                                              float &invstd) {
    const float2 mv = bn_view_mean_var(pair, g, Sg, Mg, shift);
    mean = mv.x;
    invstd = 1.0f / sqrtf(mv.y + eps);
}
// running statistics advance once per view, in order -- exactly what G sequential forward calls do
template <typename T, typename Pairs>
__device__ __forceinline__ void bn_advance_running(Pairs pair, int G, int Sg, int64_t Mg, const T *row, float pb,
                                                   float momentum, float *running_mean, float *running_var) {
    float rm = *running_mean, rv = *running_var;
    for (int g = 0; g < G; ++g) {
        const float2 mv = bn_view_mean_var(pair, g, Sg, Mg, bn_shift(row, g, Mg, pb));
        const float unbiased = Mg > 1 ? mv.y * ((float)Mg / (float)(Mg - 1)) : mv.y;
        rm = (1.0f - momentum) * rm + momentum * mv.x;
        rv = (1.0f - momentum) * rv + momentum * unbiased;
    }
    *running_mean = rm;
    *running_var = rv;
}

// One element of the backward: (x, dz) -> (dy, xhat), dy = dz * act'(pre-activation).  Two forms, built once per
// (row, view) from the same seven values.  Their bits differ, and they stay two:
// BnGrad, the two-pass kernels': subtract the mean first, as the statistics did.
struct BnGrad {
    float pb, mean, invstd, ga, be;
    int act;
    float slope;
    __device__ __forceinline__ float2 operator()(float x, float dz) const {
        const float xh = ((x + pb) - mean) * invstd;
        return make_float2(dz * act_grad(__builtin_fmaf(xh, ga, be), act, slope), xh);
    }
};
// BnGradFolded, the single-pass kernel's.  That kernel is partly bound by its vector instructions (27 per element against
// ~50 lane-operations per element that 5 TB/s leave a CU), so the per-element arithmetic is folded into the fewest fused
// operations:
//   xhat = fma(x, invstd, (pb - mean) invstd);  pre-activation = fma(x, gamma invstd, beta + (pb - mean) gamma invstd)
//   -- the very expression the forward pass thresholds, so the ReLU decision is the forward one by construction;
//   masked gradient = pre > 0 ? dz : dz * neg   (neg: 1 without activation, 0 for ReLU, the slope for LeakyReLU)
struct BnGradFolded {
    float invstd, xh0, zg, zoff, neg;
    __device__ __forceinline__ BnGradFolded(float pb, float mean, float invstd_, float ga, float be, int act, float slope)
        : invstd(invstd_), xh0((pb - mean) * invstd_), zg(ga * invstd_), zoff(be + (pb - mean) * zg),
          neg(act == 0 ? 1.0f : (act == 1 ? 0.0f : slope)) {}
    __device__ __forceinline__ float2 operator()(float x, float dz) const {
        const float xh = __builtin_fmaf(x, invstd, xh0);
        return make_float2(__builtin_fmaf(x, zg, zoff) > 0.0f ? dz : dz * neg, xh);
    }
};
// the partial sums of the backward over N elements, in either form: sd = sum dy, sdx = sum dy * xhat
template <typename Grad, int N>
__device__ __forceinline__ void bn_grad_sums(const Grad &gr, const float (&x)[N], const float (&dz)[N], float &sd, float &sdx) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float2 e = gr(x[i], dz[i]);
        sd += e.x;
        sdx = __builtin_fmaf(e.x, e.y, sdx);
    }
}

// ---- forward pass 1: partial shifted sums --------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const T *__restrict__ x, int64_t M, int64_t Mg,
                                                              int64_t chunk, int Sg,
                                                              const float *__restrict__ pre_bias,
                                                              float *__restrict__ part) {
    __shared__ float2 scratch[BN_THREADS / 64];
    const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, S = gridDim.x;
    const BnChunk ck(s, Sg, chunk, Mg);
    const T *row = x + (size_t)c * M;
    const float pb = pre_bias ? pre_bias[c] : 0.0f;
    const float shift = bn_shift(row, ck.grp, Mg, pb);
    float a = 0.0f, q = 0.0f;
    constexpr int W = VEC ? ElemIO<T>::W : 1;
    bn_walk<W>(ck.lo + (int64_t)tid * W, ck.hi, [&](int64_t m, auto n) {
        float v[decltype(n)::value];
        bn_load(row + m, v);
        bn_shifted_sums(v, pb, shift, a, q);
    });
    const float2 r = block_sum2(a, q, scratch, tid);
    if (tid == 0) bn_put_pair(part, (size_t)c * S + s, r);
}

// ---- forward pass 2: finalise statistics (train) or take running ones (eval), then apply -----------
template <typename T, bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const T *__restrict__ x, int64_t M, int64_t Mg,
                                                              int64_t chunk, int Sg, int G,
                                                              const float *__restrict__ pre_bias,
                                                              const float *__restrict__ gamma,
                                                              const float *__restrict__ beta,
                                                              const T *__restrict__ residual, int act, float slope,
                                                              float eps, float momentum, int training,
                                                              float *__restrict__ running_mean,
                                                              float *__restrict__ running_var,
                                                              const float *__restrict__ part, T *__restrict__ out,
                                                              float *__restrict__ save_mean,
                                                              float *__restrict__ save_invstd) {
    const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, S = gridDim.x;
    const BnChunk ck(s, Sg, chunk, Mg);
    const T *row = x + (size_t)c * M;
    const float pb = pre_bias ? pre_bias[c] : 0.0f;
    float mean, invstd;
    if (training) {
        const BnPart pair = {part, (size_t)c * S};
        bn_view_stats(pair, ck.grp, Sg, Mg, bn_shift(row, ck.grp, Mg, pb), eps, mean, invstd);
        if (s == 0 && tid == 0 && running_mean)
            bn_advance_running(pair, G, Sg, Mg, row, pb, momentum, running_mean + c, running_var + c);
    } else {
        mean = running_mean[c];
        invstd = 1.0f / sqrtf(running_var[c] + eps);
    }
    if (ck.sl == 0 && tid == 0) {
        save_mean[c * G + ck.grp] = mean;
        save_invstd[c * G + ck.grp] = invstd;
    }
    const BnNorm nrm = BnNorm::make(gamma[c], beta[c], pb, mean, invstd);
    const T *rrow = residual ? residual + (size_t)c * M : nullptr;
    T *orow = out + (size_t)c * M;
    constexpr int W = VEC ? ElemIO<T>::W : 1;
    int64_t m = ck.lo + (int64_t)tid * W;
    const int64_t hi = ck.hi;
    auto apply = [&](auto cen_c) {
        constexpr bool CEN = decltype(cen_c)::value;
        if (VEC) {
            // four vectors in flight per thread (one load -> use -> store per iteration left the kernel latency-bound at
            // ~4.7 TB/s; this is the eval-mode / fingerprinting path)
            constexpr int U = 4;
            const int64_t step = (int64_t)BN_THREADS * W;
            for (; m + (U - 1) * step + W <= hi; m += U * step) {
                typename ElemIO<T>::Raw rx[U], rr[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    rx[u] = *reinterpret_cast<const typename ElemIO<T>::Raw *>(row + m + u * step);
                    if (rrow) rr[u] = *reinterpret_cast<const typename ElemIO<T>::Raw *>(rrow + m + u * step);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float v[ElemIO<T>::W], r[ElemIO<T>::W];
                    ElemIO<T>::unpack(rx[u], v);
                    if (rrow) ElemIO<T>::unpack(rr[u], r);
                    bn_act_res<CEN>(nrm, act, slope, rrow != nullptr, v, r);
                    bn_store(orow + m + u * step, v);
                }
            }
        }
        bn_walk<W>(m, hi, [&](int64_t p, auto n) {      // from where the unrolled loop stopped
            float v[decltype(n)::value], r[decltype(n)::value];
            bn_load(row + p, v);
            if (rrow) bn_load(rrow + p, r);
            bn_act_res<CEN>(nrm, act, slope, rrow != nullptr, v, r);
            bn_store(orow + p, v);
        });
    };
    if (nrm.centred()) apply(std::true_type{});
    else apply(std::false_type{});
}

// ---- backward pass 1: partial sums of dy and dy * xhat ----------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce_kernel(const T *__restrict__ x, const T *__restrict__ dz,
                                                                   int64_t M, int64_t Mg, int64_t chunk, int Sg,
                                                                   int G, const float *__restrict__ pre_bias,
                                                                   const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta,
                                                                   const float *__restrict__ save_mean,
                                                                   const float *__restrict__ save_invstd, int act,
                                                                   float slope, float *__restrict__ part) {
    __shared__ float2 scratch[BN_THREADS / 64];
    const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, S = gridDim.x;
    const BnChunk ck(s, Sg, chunk, Mg);
    const T *row = x + (size_t)c * M, *grow = dz + (size_t)c * M;
    const float pb = pre_bias ? pre_bias[c] : 0.0f;
    const BnGrad gr = {pb, save_mean[c * G + ck.grp], save_invstd[c * G + ck.grp], gamma[c], beta[c], act, slope};
    float sd = 0.0f, sdx = 0.0f;
    constexpr int W = VEC ? ElemIO<T>::W : 1;
    bn_walk<W>(ck.lo + (int64_t)tid * W, ck.hi, [&](int64_t m, auto n) {
        float v[decltype(n)::value], d[decltype(n)::value];
        bn_load(row + m, v);
        bn_load(grow + m, d);
        bn_grad_sums(gr, v, d, sd, sdx);
    });
    const float2 r = block_sum2(sd, sdx, scratch, tid);
    if (tid == 0) bn_put_pair(part, (size_t)c * S + s, r);
}

// ---- backward pass 2: dgamma, dbeta, dx ---------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_dx_kernel(const T *__restrict__ x, const T *__restrict__ dz,
                                                               int64_t M, int64_t Mg, int64_t chunk, int Sg, int G,
                                                               const float *__restrict__ pre_bias,
                                                               const float *__restrict__ gamma,
                                                               const float *__restrict__ beta,
                                                               const float *__restrict__ save_mean,
                                                               const float *__restrict__ save_invstd, int act,
                                                               float slope, int training,
                                                               const float *__restrict__ part, T *__restrict__ dx,
                                                               float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                               float *__restrict__ dpre_bias) {
    const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, S = gridDim.x;
    const BnChunk ck(s, Sg, chunk, Mg);
    const T *row = x + (size_t)c * M, *grow = dz + (size_t)c * M;
    T *orow = dx + (size_t)c * M;
    const float pb = pre_bias ? pre_bias[c] : 0.0f;
    const BnGrad gr = {pb, save_mean[c * G + ck.grp], save_invstd[c * G + ck.grp], gamma[c], beta[c], act, slope};
    const BnPart pair = {part, (size_t)c * S};
    const float2 sg = bn_sum_pairs(pair, ck.grp * Sg, (ck.grp + 1) * Sg);
    if (s == 0 && tid == 0) {          // parameter gradients sum over all groups (fixed order)
        const float2 t = bn_sum_pairs(pair, 0, S);
        dgamma[c] = t.y;
        dbeta[c] = t.x;
        // gradient of a bias added BEFORE the normalisation: cancels exactly under batch statistics; with running
        // statistics (eval) dx = ga*invstd*dy, so it is ga*invstd*sum(dy)
        if (dpre_bias) dpre_bias[c] = training ? 0.0f : gr.ga * gr.invstd * t.x;
    }
    // train: dx = ga*invstd * (dy - mean_g(dy) - xhat * mean_g(dy*xhat)) within the group; eval: dx = ga*invstd*dy
    const float k = gr.ga * gr.invstd;
    const float m1 = training ? sg.x / (float)Mg : 0.0f, m2 = training ? sg.y / (float)Mg : 0.0f;
    constexpr int W = VEC ? ElemIO<T>::W : 1;
    bn_walk<W>(ck.lo + (int64_t)tid * W, ck.hi, [&](int64_t m, auto n) {
        constexpr int N = decltype(n)::value;
        float v[N], d[N];
        bn_load(row + m, v);
        bn_load(grow + m, d);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float2 e = gr(v[i], d[i]);
            v[i] = training ? k * ((e.x - m1) - e.y * m2) : k * e.x;      // (eval: no xh * 0, which is NaN for a non-finite x)
        }
        bn_store(orow + m, v);
    });
}

// ---- single-pass variants: the chunk stays in registers across a row-wide rendezvous --------------------------
// The two-kernel forms above read X twice (forward) or X and dZ twice (backward).  Here a workgroup keeps its chunk
// (8 / 4 16-byte vectors per thread and operand, bf16 left packed) in VGPRs, publishes its partial sums, waits until
// all S workgroups of ITS ROW have published (the S workgroups of a row have consecutive block ids and are dispatched together -- the
// forward-progress assumption of a decoupled look-back scan), reduces the partials in the fixed order the two-kernel
// form uses, and finishes from registers: forward 3 -> 2 passes over HBM, backward 5 -> 3.
// `sync` = one counter line per row followed by S 8-byte slots per row, ALL ONES on entry and again on exit.
// Cross-XCD visibility: slots and counters move with agent-scope relaxed atomics, i.e. sc1 write-through stores and
// L2-bypassing loads (the per-XCD L2s are not coherent for plain accesses); no L2 writeback/invalidate.  The wait
// is bounded: a workgroup whose row-mates do not show up recomputes their partial sums itself (no trap, no hang).
constexpr int BN1_ITEMS_FWD = 8;                       // 16-byte vectors per thread, kept RAW (bf16 stays packed)
constexpr int BN1_ITEMS_BWD = 4;                       // per operand (x and dz); measured: fwd 8 / bwd 4 beat 4/4 and 8/8
constexpr int BN1_THREADS = 256;
constexpr int BN1_MIN_CHUNK = BN1_THREADS * BN1_ITEMS_BWD * 4;   // smallest chunk (f32 backward): bounds the slots per row
constexpr int BN1_MAX_S = 256;                         // workgroups per row
constexpr int BN1_SYNC_STRIDE = 64;                    // ints between row counters: one 256-byte line each, so the
                                                       // polls and arrivals of different rows never share a channel queue

constexpr unsigned BN1_EMPTY = 0xffffffffu;            // "not published yet" (a NaN pattern real sums are steered away from)

// Publishes this workgroup's partial pair into slot s of its row and waits until slots [w_lo, w_hi) of the row are filled:
// a workgroup needs the partials of ITS group (view) only -- the statistics of the views are independent -- and just
// chunk 0, which also writes the per-row results over all views, needs every slot.  With two views the wait is for the
// slowest of half as many workgroups (the rate of these kernels falls with the chunks per row: 5.2 TB/s at 16, 3.7 at 128).
// No read-modify-write sits on the critical path: a slot is ONE 8-byte write-through store, the wait is wave 0 polling
// the row's S slots with L2-bypassing loads (the successful poll already holds the data).  Returns with sp[0..S) set.
// The wait is BOUNDED and never traps: after `spin_limit` polls the slots that are still empty are left marked in sp
// (BN1_EMPTY in .x) and the caller (bn1_rendezvous) recomputes exactly those partials from global memory itself (same
// thread mapping, same summation order => the same bits), so a workgroup never depends on row-mates that are not resident
// -- other kernels holding CUs (RCCL all-reduces overlapping backward, several ranks on one device, CU masks) cost time,
// not correctness.  Returns the number of slots the caller has to fill in (workgroup-uniform).
__device__ __forceinline__ int bn1_publish_and_wait(float a, float b, unsigned long long *slots_row, int s, int w_lo,
                                                    int w_hi, float2 *sp, int *n_missing, int spin_limit, int tid) {
    if (tid == 0) {
        unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
        if (ua == BN1_EMPTY) ua = 0xfffffffeu;          // still a NaN, but not the marker
        __hip_atomic_store(slots_row + s, (unsigned long long)ua | ((unsigned long long)ub << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        *n_missing = 0;
    }
    if (tid < 64) {
        int spins = 0;
        for (;;) {
            int missing = 0;
            for (int i = w_lo + tid; i < w_hi; i += 64) {
                const unsigned long long v = __hip_atomic_load(slots_row + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((unsigned)v == BN1_EMPTY) ++missing;
                sp[i] = make_float2(__uint_as_float((unsigned)v), __uint_as_float((unsigned)(v >> 32)));
            }
            if (__all(missing == 0)) break;
            if (++spins > spin_limit) {
                if (missing) atomicAdd(n_missing, missing);
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    __syncthreads();
    return *n_missing;
}

// After a workgroup has its copy of the partials it checks out of the row (fire and forget: the returned count is
// only looked at when the workgroup is done); the last one out empties the slots and re-arms the counter, so the
// whole `sync` buffer is all-ones again when the kernel ends.
__device__ __forceinline__ int bn1_checkout(int *counter) {
    return __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void bn1_rearm(int old, int S, int *counter, unsigned long long *slots_row) {
    if (old == S - 2) {                                  // counter starts at -1: the S-th checkout sees S - 2
        for (int i = 0; i < S; ++i)
            __hip_atomic_store(slots_row + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(counter, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The packed operands are kept across the rendezvous and unpacked AGAIN afterwards.  Without this fence the compiler
// keeps the unpacked / derived floats of the first phase alive instead (common subexpressions): 118 VGPRs for 4 + 4
// vectors, 188 for 8 + 8 -- two to four workgroups per CU, and every one of them that waits for its row-mates is a
// slot that moves no data.  The empty asm makes the registers opaque at no cost.
__device__ __forceinline__ void bn_opaque(float4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
__device__ __forceinline__ void bn_opaque(uint4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// What the two single-pass kernels share between their first phase and the reduction of `sp`: where the row's slots and
// counter live in `sync`, which slots this workgroup waits for, publish-and-wait, and the recompute of the slots that
// stayed empty -- partial(i) returns THIS THREAD's share of the pair of chunk i, straight from the row (same thread mapping
// and summation order as the first phase of the workgroup that owns the chunk => the same bits).  Returns with sp[w_lo, w_hi)
// valid for every thread; the caller checks out BEFORE it reduces sp and re-arms as its last statement.
struct Bn1Row {
    unsigned long long *slots;
    int *counter;
};
template <int THREADS, typename Partial>
__device__ __forceinline__ Bn1Row bn1_rendezvous(float2 r, int *sync, int c, int s, int grp, int Sg, float2 *sp,
                                                 int *n_missing, float2 *scratch, int spin_limit, int tid, Partial partial) {
    const int S = gridDim.x;
    const Bn1Row rw = {reinterpret_cast<unsigned long long *>(sync + (size_t)gridDim.y * BN1_SYNC_STRIDE) + (size_t)c * S,
                       sync + (size_t)c * BN1_SYNC_STRIDE};
    const int w_lo = s == 0 ? 0 : grp * Sg, w_hi = s == 0 ? S : (grp + 1) * Sg;     // chunk 0 also writes the per-row results
    if (bn1_publish_and_wait(r.x, r.y, rw.slots, s, w_lo, w_hi, sp, n_missing, spin_limit, tid) > 0) {
        // row-mates that did not show up in time
        for (int i = w_lo; i < w_hi; ++i) {
            if (__float_as_uint(sp[i].x) != BN1_EMPTY) continue;            // LDS value: workgroup-uniform branch
            const float2 p = partial(i);
            const float2 r2 = block_sum2<THREADS>(p.x, p.y, scratch, tid);
            if (tid == 0) sp[i] = r2;
        }
        __syncthreads();
    }
    return rw;
}

template <typename T, bool RES>
__global__ __launch_bounds__(BN1_THREADS) void bn_fwd1_kernel(const T *__restrict__ x, int64_t M, int64_t Mg, int Sg,
                                                             int G, const float *__restrict__ pre_bias,
                                                             const float *__restrict__ gamma,
                                                             const float *__restrict__ beta,
                                                             const T *__restrict__ residual, int act, float slope,
                                                             float eps, float momentum,
                                                             float *__restrict__ running_mean,
                                                             float *__restrict__ running_var,
                                                             int *__restrict__ sync, T *__restrict__ out,
                                                             float *__restrict__ save_mean,
                                                             float *__restrict__ save_invstd, int spin_limit) {
    constexpr int W = ElemIO<T>::W, ITEMS = BN1_ITEMS_FWD, CHUNK = BN1_THREADS * ITEMS * W;
    using Raw = typename ElemIO<T>::Raw;
    __shared__ float2 scratch[BN1_THREADS / 64];
    __shared__ float2 sp[BN1_MAX_S];
    __shared__ int n_missing;
    const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, S = gridDim.x;
    const BnChunk ck(s, Sg, CHUNK, Mg);
    const T *row = x + (size_t)c * M;
    const float pb = pre_bias ? pre_bias[c] : 0.0f;
    const float shift = bn_shift(row, ck.grp, Mg, pb);
    Raw raw[ITEMS];
    float a = 0.0f, q = 0.0f;
    bn1_walk<ITEMS, BN1_THREADS, W>(ck.lo, ck.hi, [&](int it, int64_t m) { raw[it] = *reinterpret_cast<const Raw *>(row + m); });
    bn1_walk<ITEMS, BN1_THREADS, W>(ck.lo, ck.hi, [&](int it, int64_t) {
        float v[W];
        ElemIO<T>::unpack(raw[it], v);
        bn_shifted_sums(v, pb, shift, a, q);
    });
    // the shortcut rows do not depend on the statistics: fetch them now, so their latency passes during the rendezvous
    // (RES is a template parameter: the 32 extra registers only exist in the instantiation that needs them)
    const T *rrow = RES ? residual + (size_t)c * M : nullptr;
    Raw rres[RES ? ITEMS : 1];
    if (RES) bn1_walk<ITEMS, BN1_THREADS, W>(ck.lo, ck.hi, [&](int it, int64_t m) { rres[it] = *reinterpret_cast<const Raw *>(rrow + m); });
    const float2 r = block_sum2<BN1_THREADS>(a, q, scratch, tid);
    const Bn1Row rw = bn1_rendezvous<BN1_THREADS>(r, sync, c, s, ck.grp, Sg, sp, &n_missing, scratch, spin_limit, tid, [&](int i) {
        const BnChunk c2(i, Sg, CHUNK, Mg);
        const float sh2 = bn_shift(row, c2.grp, Mg, pb);
        float a2 = 0.0f, q2 = 0.0f;
        bn1_walk<ITEMS, BN1_THREADS, W>(c2.lo, c2.hi, [&](int, int64_t m) {
            float v[W];
            ElemIO<T>::load(row + m, v);
            bn_shifted_sums(v, pb, sh2, a2, q2);
        });
        return make_float2(a2, q2);
    });
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) bn_opaque(raw[it]);
    int checkout = 0;
    if (tid == 0) checkout = bn1_checkout(rw.counter);
    const auto pair = [&](int i) { return sp[i]; };
    float mean, invstd;
    bn_view_stats(pair, ck.grp, Sg, Mg, shift, eps, mean, invstd);
    if (ck.sl == 0 && tid == 0) {
        save_mean[c * G + ck.grp] = mean;
        save_invstd[c * G + ck.grp] = invstd;
    }
    if (s == 0 && tid == 0 && running_mean)
        bn_advance_running(pair, G, Sg, Mg, row, pb, momentum, running_mean + c, running_var + c);
    const BnNorm nrm = BnNorm::make(gamma[c], beta[c], pb, mean, invstd);
    T *orow = out + (size_t)c * M;
    // (this walk keeps its own spelling: through bn1_walk the positions m are the first phase's own expressions and stay
    //  live across the rendezvous, 14 VGPRs; written here they are formed again)
    auto apply = [&](auto cen_c) {
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int64_t m = ck.lo + ((int64_t)it * BN1_THREADS + tid) * W;
            if (m < ck.hi) {
                float v[W], rr[W];
                ElemIO<T>::unpack(raw[it], v);
                if (RES) ElemIO<T>::unpack(rres[it], rr);
                bn_act_res<decltype(cen_c)::value>(nrm, act, slope, RES, v, rr);
                ElemIO<T>::store(orow + m, v, false);
            }
        }
    };
    if (nrm.centred()) apply(std::true_type{});
    else apply(std::false_type{});
    if (tid == 0) bn1_rearm(checkout, S, rw.counter, rw.slots);
}

template <typename T, int ITEMS, int THREADS = BN1_THREADS>
__global__ __launch_bounds__(THREADS) void bn_bwd1_kernel(const T *__restrict__ x, const T *__restrict__ dz,
                                                             int64_t M, int64_t Mg, int Sg, int G,
                                                             const float *__restrict__ pre_bias,
                                                             const float *__restrict__ gamma,
                                                             const float *__restrict__ beta,
                                                             const float *__restrict__ save_mean,
                                                             const float *__restrict__ save_invstd, int act,
                                                             float slope,
                                                             int *__restrict__ sync, T *__restrict__ dx,
                                                             float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                             float *__restrict__ dpre_bias, int spin_limit,
                                                             int plain_stores) {
    constexpr int W = ElemIO<T>::W, CHUNK = THREADS * ITEMS * W;
    using Raw = typename ElemIO<T>::Raw;
    __shared__ float2 scratch[THREADS / 64];
    __shared__ float2 sp[BN1_MAX_S];
    __shared__ int n_missing;
    const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x, S = gridDim.x;
    const BnChunk ck(s, Sg, CHUNK, Mg);
    const T *row = x + (size_t)c * M, *grow = dz + (size_t)c * M;
    T *orow = dx + (size_t)c * M;
    const float pb = pre_bias ? pre_bias[c] : 0.0f;
    const float ga = gamma[c], be = beta[c];
    const BnGradFolded gr(pb, save_mean[c * G + ck.grp], save_invstd[c * G + ck.grp], ga, be, act, slope);
    Raw rx[ITEMS], rd[ITEMS];
    bn1_walk<ITEMS, THREADS, W>(ck.lo, ck.hi, [&](int it, int64_t m) {
        rx[it] = GRAFP_LD_ONCE(1, reinterpret_cast<const Raw *>(row + m));
        rd[it] = GRAFP_LD_ONCE(4, reinterpret_cast<const Raw *>(grow + m));
    });
    float sd = 0.0f, sdx = 0.0f;
    bn1_walk<ITEMS, THREADS, W>(ck.lo, ck.hi, [&](int it, int64_t) {
        float v[W], d[W];
        ElemIO<T>::unpack(rx[it], v);
        ElemIO<T>::unpack(rd[it], d);
        bn_grad_sums(gr, v, d, sd, sdx);
    });
    const float2 r = block_sum2<THREADS>(sd, sdx, scratch, tid);
    const Bn1Row rw = bn1_rendezvous<THREADS>(r, sync, c, s, ck.grp, Sg, sp, &n_missing, scratch, spin_limit, tid, [&](int i) {
        const BnChunk c2(i, Sg, CHUNK, Mg);
        const BnGradFolded gr2(pb, save_mean[c * G + c2.grp], save_invstd[c * G + c2.grp], ga, be, act, slope);
        float sd2 = 0.0f, sdx2 = 0.0f;
        bn1_walk<ITEMS, THREADS, W>(c2.lo, c2.hi, [&](int, int64_t m) {
            float v[W], d[W];
            ElemIO<T>::load(row + m, v);
            ElemIO<T>::load(grow + m, d);
            bn_grad_sums(gr2, v, d, sd2, sdx2);
        });
        return make_float2(sd2, sdx2);
    });
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        bn_opaque(rx[it]);
        bn_opaque(rd[it]);
    }
    int checkout = 0;
    if (tid == 0) checkout = bn1_checkout(rw.counter);
    const auto pair = [&](int i) { return sp[i]; };
    const float2 sg = bn_sum_pairs(pair, ck.grp * Sg, (ck.grp + 1) * Sg);
    if (s == 0 && tid == 0) {
        const float2 t = bn_sum_pairs(pair, 0, S);
        dgamma[c] = t.y;
        dbeta[c] = t.x;
        if (dpre_bias) dpre_bias[c] = 0.0f;          // training mode only: cancels in the normalisation
    }
    const float k = ga * gr.invstd;
    const float m1 = sg.x / (float)Mg, m2 = sg.y / (float)Mg;
    const float km1 = -(k * m1), km2 = -(k * m2);               // dx = k dy - k m1 - k m2 xh: two fmaf per element
    bn1_walk<ITEMS, THREADS, W>(ck.lo, ck.hi, [&](int it, int64_t m) {
        float v[W], d[W];
        ElemIO<T>::unpack(rx[it], v);
        ElemIO<T>::unpack(rd[it], d);
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float2 e = gr(v[i], d[i]);
            v[i] = __builtin_fmaf(e.y, km2, __builtin_fmaf(e.x, k, km1));
        }
        ElemIO<T>::store(orow + m, v, plain_stores != 0);
    });
    if (tid == 0) bn1_rearm(checkout, S, rw.counter, rw.slots);
}

// single-pass plan: Sg chunks per group, or 0 when the shape does not qualify
static int bn1_plan(int64_t Mg, int G, int W, int items, int threads = BN1_THREADS) {
    if (Mg % W) return 0;
    const int64_t chunk = (int64_t)threads * items * W;
    const int64_t Sg = (Mg + chunk - 1) / chunk;
    if (Sg * G > BN1_MAX_S) return 0;
    return (int)Sg;
}

struct BnPlan {
    int Sg;
    int64_t chunk;
};
static BnPlan bn_plan(int C, int64_t Mg, int G, int W) {
    const int64_t per_block = (int64_t)BN_THREADS * W * 4;      // >= 4 vector iterations per thread
    int64_t S = (Mg + per_block - 1) / per_block;
    const int64_t cap = 4096 / ((int64_t)C * G) > 1 ? 4096 / ((int64_t)C * G) : 1;   // ~4096 workgroups overall
    if (S > cap) S = cap;
    if (S < 1) S = 1;
    int64_t chunk = (Mg + S - 1) / S;
    chunk = (chunk + W - 1) / W * W;                             // chunk boundaries stay vector-aligned
    BnPlan p;
    p.chunk = chunk;
    p.Sg = (int)((Mg + chunk - 1) / chunk);
    return p;
}

// The launch a call takes: ONE function for grafp_bn_fwd_1pass, grafp_bn_bwd_1pass and grafp_bn_plan, so the query cannot
// drift from the launches.  vec = bn_vec_ok of the call's pointers; have_sync = a rendezvous buffer was passed.
enum { BN_PATH_1PASS = 0, BN_PATH_2PASS_VEC = 1, BN_PATH_2PASS_SCALAR = 2 };
struct BnLaunch {
    int path;
    int items;          // single pass: 16-byte vectors a thread holds per operand; two-pass: 0 (threads stride over the chunk)
    int threads;
    int Sg;             // chunks per view
    int64_t chunk;      // elements per chunk (the last chunk of a view may be shorter)
};
static int bn_vec_width(int dtype) { return dtype == GRAFP_F32 ? 4 : 8; }      // ElemIO<T>::W of the dtype's T
static BnLaunch bn_choose(int dtype, int C, int64_t Mg, int G, bool training, bool backward, bool vec, bool have_sync) {
    const bool f32 = dtype == GRAFP_F32;
    const int W = bn_vec_width(dtype);
    BnLaunch L;
    if (have_sync && training && !backward) {
        const int Sg = vec ? bn1_plan(Mg, G, W, BN1_ITEMS_FWD) : 0;
        if (Sg > 0) {
            L = {BN_PATH_1PASS, BN1_ITEMS_FWD, BN1_THREADS, Sg, (int64_t)BN1_THREADS * BN1_ITEMS_FWD * W};
            return L;
        }
    }
    if (have_sync && training && backward) {
        // from 16 chunks per row the rendezvous runs over fewer, larger chunks: 8 vectors per thread and operand instead
        // of 4 (tools/bn_bench.py, threshold swept 0 ... 128: 16 is best at 256, 512 and 2048 clip-views; with the
        // operands fenced across the wait -- bn_opaque -- this variant needs 122 VGPRs, 4 workgroups per CU)
        int items = BN1_ITEMS_BWD;
        int Sg = vec ? bn1_plan(Mg, G, W, items) : 0;
        const int items8_from = GRAFP_TUNE_INT("GRAFP_BN_BWD_ITEMS8_FROM", 16);
        if (vec && !f32 && (Sg == 0 || Sg * G > items8_from)) {
            items = 2 * BN1_ITEMS_BWD;
            Sg = bn1_plan(Mg, G, 8, items);
        }
        // ... and from 32 chunks per view on 512-thread workgroups: half the chunks again with the same registers per
        // thread and the same waves per CU (two workgroups instead of four).  tools/bn_bench.py at 2048 clip-views: 64
        // chunks per view (stage 0) 783 -> 703 us, 32 (stage 1) 681 -> 650; from 16 chunks (stage 2) it loses 1 %, and
        // 1024-thread workgroups -- ONE per CU, whose phases overlap nobody's -- lose 10-20 % everywhere.
        const int t512_from = GRAFP_TUNE_INT("GRAFP_BN_BWD_T512_FROM", 32);
        if (vec && !f32 && t512_from > 0 && items == 2 * BN1_ITEMS_BWD && Sg >= t512_from) {
            const int Sg2 = bn1_plan(Mg, G, 8, items, 512);
            if (Sg2 > 0) {
                L = {BN_PATH_1PASS, items, 512, Sg2, (int64_t)512 * items * W};
                return L;
            }
        }
        if (Sg > 0) {
            L = {BN_PATH_1PASS, items, BN1_THREADS, Sg, (int64_t)BN1_THREADS * items * W};
            return L;
        }
    }
    const BnPlan p = bn_plan(C, Mg, G, vec ? W : 1);
    L = {vec ? BN_PATH_2PASS_VEC : BN_PATH_2PASS_SCALAR, 0, BN_THREADS, p.Sg, p.chunk};
    return L;
}

// W = ElemIO<T>::W: whole 16-byte pieces at 16-byte aligned addresses
static bool bn_vec_ok(int W, const void *a, const void *b, const void *c, const void *d, int64_t Mg) {
    const uintptr_t m = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d;
    return (Mg % W) == 0 && (m & 15) == 0;
}

}  // namespace grafp

// polls (~1 us each) before a workgroup stops waiting for its row-mates and recomputes their partial sums itself; a
// per-call argument of the *_1pass entry points (negative = this default; 0 = never wait)
static inline int bn_spin(int spin_limit) { return spin_limit < 0 ? (1 << 12) : spin_limit; }

// what grafp_bn_fwd_1pass, grafp_bn_bwd_1pass and grafp_bn_plan ask of their arguments; op names the entry in the message
static int bn_check_args(const char *op, bool pointers, int dtype, int C, int64_t M, int groups, int act) {
    GRAFP_REQUIRE(pointers, "%s: null pointer", op);
    GRAFP_REQUIRE(C > 0 && M > 0 && C <= 65535, "%s: bad shape C=%d M=%lld", op, C, (long long)M);
    GRAFP_REQUIRE(groups >= 1 && groups <= 8 && M % groups == 0, "%s: groups=%d must be in [1,8] and divide M=%lld", op, groups, (long long)M);
    GRAFP_REQUIRE(dtype == GRAFP_F32 || dtype == GRAFP_BF16, "%s: dtype %d not in {f32, bf16}", op, dtype);
    GRAFP_REQUIRE(act >= 0 && act <= 2, "%s: act %d not in {0 none, 1 relu, 2 leaky}", op, act);
    return GRAFP_OK;
}

extern "C" size_t grafp_bn_workspace(int C, int64_t M) {
    if (C <= 0 || M <= 0) return 0;
    const size_t two_pass = (size_t)4096 + (size_t)C * 8;          // >= C * G * Sg partial pairs for any G <= 8
    return two_pass * 2 * sizeof(float);
}

extern "C" size_t grafp_bn_sync_bytes(int C, int64_t M) {
    if (C <= 0 || M <= 0) return 0;
    // a counter line per row + at most (M / chunk + groups) <= M / chunk + 8 slots per row
    return (size_t)C * grafp::BN1_SYNC_STRIDE * sizeof(int) + (size_t)C * ((size_t)(M / grafp::BN1_MIN_CHUNK) + 8) * 8;
}

static int bn_check_ws(const char *op, const void *ws, size_t ws_bytes, int C, int64_t M) {
    if (!ws || ws_bytes < grafp_bn_workspace(C, M)) {
        grafp::set_error("%s: workspace %zu bytes < required %zu", op, ws_bytes, grafp_bn_workspace(C, M));
        return GRAFP_ERR_WORKSPACE;
    }
    return GRAFP_OK;
}

extern "C" int grafp_bn_fwd_1pass(const void *x, int dtype, int C, int64_t M, int groups, const float *pre_bias,
                                  const float *gamma, const float *beta, const void *residual, int act, float slope,
                                  float eps, float momentum, int training, float *running_mean, float *running_var,
                                  void *out, float *save_mean, float *save_invstd, void *ws, size_t ws_bytes,
                                  int32_t *sync, int spin_limit, grafp_stream_t stream) {
    using namespace grafp;
    const int spin = bn_spin(spin_limit);
    if (int e = bn_check_args("bn_fwd", x && gamma && beta && out && save_mean && save_invstd, dtype, C, M, groups, act)) return e;
    GRAFP_REQUIRE(training || (running_mean && running_var), "bn_fwd: eval mode needs running statistics");
    if (int e = bn_check_ws("bn_fwd", ws, ws_bytes, C, M)) return e;
    const int G = groups;
    const int64_t Mg = M / G;
    hipStream_t s = (hipStream_t)stream;
    float *part = (float *)ws;
    const bool vec = bn_vec_ok(bn_vec_width(dtype), x, out, residual, nullptr, Mg);
    const BnLaunch p = bn_choose(dtype, C, Mg, G, training != 0, false, vec, sync != nullptr);
    if (p.path == BN_PATH_1PASS) {
        const int Sg = p.Sg;
        for_elem(dtype, [&](auto te) {
            using T = typename decltype(te)::type;
            for_bool(residual != nullptr, [&](auto res) {
                hipLaunchKernelGGL((bn_fwd1_kernel<T, decltype(res)::value>), dim3(Sg * G, C), dim3(BN1_THREADS), 0, s,
                                   (const T *)x, M, Mg, Sg, G, pre_bias, gamma, beta, (const T *)residual, act, slope,
                                   eps, momentum, running_mean, running_var, (int *)sync, (T *)out, save_mean,
                                   save_invstd, spin);
            });
        });
        GRAFP_CHECK_LAUNCH("bn_fwd1_kernel");
        return GRAFP_OK;
    }
    const dim3 grid(p.Sg * G, C);
    for_elem(dtype, [&](auto te) {
        using T = typename decltype(te)::type;
        for_bool(vec, [&](auto v) {
            constexpr bool VEC = decltype(v)::value;
            if (training)
                hipLaunchKernelGGL((bn_stats_kernel<T, VEC>), grid, dim3(BN_THREADS), 0, s, (const T *)x, M, Mg, p.chunk,
                                   p.Sg, pre_bias, part);
            hipLaunchKernelGGL((bn_apply_kernel<T, VEC>), grid, dim3(BN_THREADS), 0, s, (const T *)x, M, Mg, p.chunk, p.Sg,
                               G, pre_bias, gamma, beta, (const T *)residual, act, slope, eps, momentum, training,
                               running_mean, running_var, part, (T *)out, save_mean, save_invstd);
        });
    });
    GRAFP_CHECK_LAUNCH("bn_stats_kernel / bn_apply_kernel");
    return GRAFP_OK;
}

extern "C" int grafp_bn_fwd(const void *x, int dtype, int C, int64_t M, int groups, const float *pre_bias, const float *gamma,
                            const float *beta, const void *residual, int act, float slope, float eps, float momentum,
                            int training, float *running_mean, float *running_var, void *out, float *save_mean,
                            float *save_invstd, void *ws, size_t ws_bytes, grafp_stream_t stream) {
    return grafp_bn_fwd_1pass(x, dtype, C, M, groups, pre_bias, gamma, beta, residual, act, slope, eps, momentum, training,
                              running_mean, running_var, out, save_mean, save_invstd, ws, ws_bytes, nullptr, -1, stream);
}

extern "C" int grafp_bn_bwd_1pass(const void *x, const void *dz, int dtype, int C, int64_t M, int groups,
                                  const float *pre_bias, const float *gamma, const float *beta, const float *save_mean,
                                  const float *save_invstd, int act, float slope, int training, void *dx,
                                  float *dgamma, float *dbeta, float *dpre_bias, void *ws, size_t ws_bytes,
                                  int32_t *sync, int spin_limit, grafp_stream_t stream) {
    using namespace grafp;
    const int spin = bn_spin(spin_limit);
    if (int e = bn_check_args("bn_bwd", x && dz && gamma && beta && save_mean && save_invstd && dx && dgamma && dbeta, dtype, C, M,
                              groups, act))
        return e;
    if (int e = bn_check_ws("bn_bwd", ws, ws_bytes, C, M)) return e;
    const int G = groups;
    const int64_t Mg = M / G;
    hipStream_t s = (hipStream_t)stream;
    float *part = (float *)ws;
    const bool f32 = dtype == GRAFP_F32;
    const bool ok = bn_vec_ok(bn_vec_width(dtype), x, dz, dx, nullptr, Mg);
    const BnLaunch p = bn_choose(dtype, C, Mg, G, training != 0, true, ok, sync != nullptr);
    if (p.path == BN_PATH_1PASS) {
        // one launch of the single-pass kernel <T, ITEMS, THREADS> over sg chunks per view
        auto launch1 = [&](auto te, auto items_c, auto threads_c, int sg, int plain) {
            using T = typename decltype(te)::type;
            constexpr int THREADS = decltype(threads_c)::value;
            hipLaunchKernelGGL((bn_bwd1_kernel<T, decltype(items_c)::value, THREADS>), dim3(sg * G, C), dim3(THREADS), 0, s,
                               (const T *)x, (const T *)dz, M, Mg, sg, G, pre_bias, gamma, beta, save_mean, save_invstd, act,
                               slope, (int *)sync, (T *)dx, dgamma, dbeta, dpre_bias, spin, plain);
        };
        using Items1 = std::integral_constant<int, BN1_ITEMS_BWD>;
        using Items2 = std::integral_constant<int, 2 * BN1_ITEMS_BWD>;
        using T256 = std::integral_constant<int, BN1_THREADS>;
        using T512 = std::integral_constant<int, 512>;
        const int plain = plain_stores((size_t)C * (size_t)M * (f32 ? 4 : 2), "GRAFP_BN_BWD_PLAIN_MAX_MB", 140);
        if (f32) launch1(TypeTag<float>{}, Items1{}, T256{}, p.Sg, plain);
        else if (p.threads == 512) launch1(TypeTag<unsigned short>{}, Items2{}, T512{}, p.Sg, plain);
        else if (p.items == BN1_ITEMS_BWD) launch1(TypeTag<unsigned short>{}, Items1{}, T256{}, p.Sg, plain);
        else launch1(TypeTag<unsigned short>{}, Items2{}, T256{}, p.Sg, plain);
        GRAFP_CHECK_LAUNCH("bn_bwd1_kernel");
        return GRAFP_OK;
    }
    const dim3 grid(p.Sg * G, C);
    for_elem(dtype, [&](auto te) {
        using T = typename decltype(te)::type;
        for_bool(ok, [&](auto v) {
            constexpr bool VEC = decltype(v)::value;
            hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, VEC>), grid, dim3(BN_THREADS), 0, s, (const T *)x, (const T *)dz, M,
                               Mg, p.chunk, p.Sg, G, pre_bias, gamma, beta, save_mean, save_invstd, act, slope, part);
            hipLaunchKernelGGL((bn_bwd_dx_kernel<T, VEC>), grid, dim3(BN_THREADS), 0, s, (const T *)x, (const T *)dz, M, Mg,
                               p.chunk, p.Sg, G, pre_bias, gamma, beta, save_mean, save_invstd, act, slope, training, part,
                               (T *)dx, dgamma, dbeta, dpre_bias);
        });
    });
    GRAFP_CHECK_LAUNCH("bn_bwd_reduce_kernel / bn_bwd_dx_kernel");
    return GRAFP_OK;
}

extern "C" int grafp_bn_bwd(const void *x, const void *dz, int dtype, int C, int64_t M, int groups, const float *pre_bias,
                            const float *gamma, const float *beta, const float *save_mean, const float *save_invstd,
                            int act, float slope, int training, void *dx, float *dgamma, float *dbeta,
                            float *dpre_bias, void *ws, size_t ws_bytes, grafp_stream_t stream) {
    return grafp_bn_bwd_1pass(x, dz, dtype, C, M, groups, pre_bias, gamma, beta, save_mean, save_invstd, act, slope,
                              training, dx, dgamma, dbeta, dpre_bias, ws, ws_bytes, nullptr, -1, stream);
}

extern "C" int grafp_bn_plan(int dtype, int C, int64_t M, int groups, int training, int backward, int aligned,
                             int have_sync, int *info) {
    using namespace grafp;
    if (int e = bn_check_args("bn_plan", info != nullptr, dtype, C, M, groups, 0)) return e;
    const int64_t Mg = M / groups;
    const BnLaunch p = bn_choose(dtype, C, Mg, groups, training != 0, backward != 0,
                                 aligned != 0 && Mg % bn_vec_width(dtype) == 0, have_sync != 0);
    info[0] = p.path;
    info[1] = p.items;
    info[2] = p.threads;
    info[3] = p.Sg;
    info[4] = p.chunk > 0x7fffffff ? 0x7fffffff : (int)p.chunk;
    for (int i = 5; i < 8; ++i) info[i] = 0;
    return GRAFP_OK;
}
