// stretch.hip -- time-stretch augmentation of the second training view (grafp_amd/modules/transformations.py), gfx950.
//
// One launch stretches every clip of a batch by its OWN ratio, read on the device (so the launch can be captured into a
// HIP graph and every replay reads fresh ratios).  The tempo moves and the pitch stays: key-locked DJ decks, programmes
// squeezed by a few per cent.  speed.hip is the other kind, where the pitch moves with the tempo.
//
// THE RULE (WSOLA, waveform-similarity overlap-add; tests/_stretch_ref.stretch_f64 is it in float64).
//   Frame N = 512, synthesis hop HS = 256, search range delta in [-128, 127] (256 candidates),
//   window w[n] = sin^2(pi n / N), so that w[n] + w[n + HS] = 1.
//   For clip b:
//   rho = ratio[b] clamped to [0.5, 2]; a NaN counts as 1.  rho is input samples per output sample: above 1 the clip
//         plays fast (speed.hip's conventions).
//   xz  = x inside [0, T_in), 0 outside.
//   Frames i = 0 .. F - 1, F = ceil(T_out / HS) + 1.  Frame i covers the outputs [(i - 1) HS, (i + 1) HS): every output
//         lies under exactly two frames, there is no fade-in.
//   a_i = x_offset + floor((i - 1) * HS * (double)rho + 0.5)           (the nominal input position; the product is exact
//         in f64 and must not be formed in f32: past frame 1024 an f32 product is rounded to 1/32 sample and falls on
//         the other side of the floor at some frames -- at rho = 0.97 at frame 1065 and every 25th after it)
//   delta_0 = 0.  For i >= 1, with p_i = a_i + delta_i:
//         t[n]     = xz[p_{i-1} + HS + n], n < N                       (the natural continuation of the previous frame)
//         c(delta) = sum over n < N of t[n] * xz[a_i + delta + n]
//         delta_i  = the candidate with the largest c; ties go to the smaller |delta|, then to the negative one.
//   out[b][m] = w[n + HS] * xz[p_{i-1} + n + HS] + w[n] * xz[p_i + n],  m = (i - 1) HS + n, 0 <= n < HS, m < T_out.
//         Every output is written once, in order: no atomics, no read-modify-write.
//   rho == 1.0f exactly: out[b][m] = xz[x_offset + m], a bit copy, and every delta is 0 (the window sum is 1 only in
//         exact arithmetic, and the unnormalised correlation need not peak at delta = 0).
//   shift[b][i] = delta_i (optional second output): where the splices are.
//
// THE ROUTE (tests/_stretch_ref.stretch_f32 restates the output arithmetic operation by operation):
//   * One workgroup of 256 threads per clip.  The frames are sequential (delta_i needs delta_{i-1}); inside a frame the
//     256 candidates run in parallel.
//   * Per frame two LDS buffers: R[k] = xz[a_i - 128 + k], k < 1024, and the template Tm[n] = t[n].  R holds the search
//     region (k < 767) and, whatever delta_i turns out to be, the next template R[128 + delta_i + HS + n] (k <= 1022):
//     the template never comes from global memory inside the chain delta_{i-1} -> delta_i.  R of frame i + 1 does not
//     depend on any delta; it is loaded into registers before the correlations and stored after them.
//   * Correlations: lane l of every wave owns the four candidates 4 l .. 4 l + 3; wave v sums the products of
//     n in [128 v, 128 v + 128).  Per step of four n a thread reads one 16-byte slot of R (it keeps the previous one: a
//     sliding window of eight samples in registers) and one of Tm (the same address in every lane: a broadcast) for
//     16 fmaf.  Each candidate's partial sum is one fmaf chain over ascending n starting from 0; the four partial sums
//     are added as ((P0 + P1) + P2) + P3.  The order is fixed: two launches give the same bits.
//   * Arg-max: wave 0 adds the partial sums, each lane picks among its four, then a 64-lane butterfly on
//     (c, |delta|, delta); one LDS word carries delta_i to the other waves.
//   * Output: thread n computes sn = sinf(n * pi/N), cs = cosf(n * pi/N) once; out = (cs * cs) * Tm[n] + (sn * sn) *
//     R[128 + delta_i + n], two products and one sum, each rounded (Tm[n] IS xz[p_{i-1} + HS + n]).
//   No workspace, no host synchronisation, no mutable global.  Where the time goes: DESIGN.md section 12.27.
//
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as speed.hip is: DESIGN.md section 12.7b.
#include <math.h>

#include "clipwarp.h"
#include "common.h"

namespace grafp {

constexpr int ST_N = 512;                                  // frame
constexpr int ST_HS = 256;                                 // synthesis hop
constexpr int ST_D = 128;                                  // candidates delta = -ST_D .. ST_D - 1
constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int ST_R = 1024;                                 // samples of R: 128 + 127 + HS + N = 1023 are read at most
constexpr int ST_KSLICE = ST_N / ST_WAVES;                 // n per wave
constexpr float ST_PI_N = 0.00613592315154256491887f;      // pi / N

static_assert(ST_THREADS == 2 * ST_D && ST_THREADS == ST_HS, "one thread per candidate slot and per output of a hop");
static_assert(ST_D + (ST_D - 1) + ST_HS + ST_N <= ST_R, "the next template lies inside R for every delta");
static_assert(4 * 63 + 3 + ST_N <= ST_R, "the last candidate's last product lies inside R");

typedef float st_slot __attribute__((ext_vector_type(4)));    // one 16-byte LDS slot, read whole (ds_read_b128)

// the rule's order on candidates: larger c, then smaller |delta|, then the negative one.  (A NaN c never wins.)
__device__ __forceinline__ bool st_better(float c, int d, float bc, int bd) {
    if (c != bc) return c > bc;
    const int a = d < 0 ? -d : d, ba = bd < 0 ? -bd : bd;
    return a != ba ? a < ba : d < bd;
}

__global__ __launch_bounds__(ST_THREADS) void time_stretch_kernel(const float *__restrict__ x, int64_t x_stride, int T_in,
                                                                  int64_t x_offset, const float *__restrict__ ratio,
                                                                  float *__restrict__ out, int64_t out_stride, int T_out,
                                                                  int32_t *__restrict__ shift, int64_t shift_stride,
                                                                  int frames) {
    __shared__ __attribute__((aligned(16))) float R[ST_R];
    __shared__ __attribute__((aligned(16))) float Tm[ST_N];
    __shared__ __attribute__((aligned(16))) float P[ST_WAVES][2 * ST_D];
    __shared__ int s_delta;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *xb = x + (int64_t)b * x_stride;
    float *ob = out + (int64_t)b * out_stride;
    int32_t *sb = shift ? shift + (int64_t)b * shift_stride : nullptr;
    const float rho = warp_ratio(ratio[b]);

    if (rho == 1.0f) {                                     // workgroup-uniform: the whole workgroup copies
        warp_copy<ST_THREADS>(xb, T_in, x_offset, ob, 0, T_out, tid);
        if (sb)
            for (int i = tid; i < frames; i += ST_THREADS) sb[i] = 0;
        return;
    }

    const double rd = (double)rho;
    auto pos = [&](int i) -> int64_t { return x_offset + (int64_t)floor((double)((int64_t)(i - 1) * ST_HS) * rd + 0.5); };
    auto xz = [&](int64_t s) -> float { return (s >= 0 && s < T_in) ? xb[s] : 0.0f; };

    // frame 0: delta = 0, so frame 1's template is xz[a_0 + HS + n]; R of frame 1
    const int64_t t0 = pos(0) + ST_HS, r1 = pos(1) - ST_D;
    Tm[tid] = xz(t0 + tid);
    Tm[tid + ST_THREADS] = xz(t0 + tid + ST_THREADS);
#pragma unroll
    for (int k = 0; k < ST_R / ST_THREADS; ++k) R[tid + k * ST_THREADS] = xz(r1 + tid + k * ST_THREADS);
    if (sb && tid == 0) sb[0] = 0;
    const float ang = (float)tid * ST_PI_N;
    const float sn = sinf(ang), cs = cosf(ang);
    const float w_new = sn * sn, w_old = cs * cs;          // w[n] and w[n + HS]
    __syncthreads();

    const st_slot *R4 = reinterpret_cast<const st_slot *>(R) + wv * (ST_KSLICE / 4) + lane;
    const st_slot *T4 = reinterpret_cast<const st_slot *>(Tm) + wv * (ST_KSLICE / 4);
    for (int i = 1; i < frames; ++i) {
        // R of the next frame: in flight during the correlations
        float nx[ST_R / ST_THREADS];
        const bool more = i + 1 < frames;
        if (more) {
            const int64_t rn = pos(i + 1) - ST_D;
#pragma unroll
            for (int k = 0; k < ST_R / ST_THREADS; ++k) nx[k] = xz(rn + tid + k * ST_THREADS);
        }

        // candidates 4 lane .. 4 lane + 3 over this wave's slice of n
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
        st_slot lo = R4[0];
#pragma unroll 8
        for (int q = 0; q < ST_KSLICE / 4; ++q) {
            const st_slot hi = R4[q + 1];
            const st_slot t = T4[q];
            c0 = __builtin_fmaf(t.x, lo.x, c0); c0 = __builtin_fmaf(t.y, lo.y, c0);
            c0 = __builtin_fmaf(t.z, lo.z, c0); c0 = __builtin_fmaf(t.w, lo.w, c0);
            c1 = __builtin_fmaf(t.x, lo.y, c1); c1 = __builtin_fmaf(t.y, lo.z, c1);
            c1 = __builtin_fmaf(t.z, lo.w, c1); c1 = __builtin_fmaf(t.w, hi.x, c1);
            c2 = __builtin_fmaf(t.x, lo.z, c2); c2 = __builtin_fmaf(t.y, lo.w, c2);
            c2 = __builtin_fmaf(t.z, hi.x, c2); c2 = __builtin_fmaf(t.w, hi.y, c2);
            c3 = __builtin_fmaf(t.x, lo.w, c3); c3 = __builtin_fmaf(t.y, hi.x, c3);
            c3 = __builtin_fmaf(t.z, hi.y, c3); c3 = __builtin_fmaf(t.w, hi.z, c3);
            lo = hi;
        }
        reinterpret_cast<float4 *>(P[wv])[lane] = make_float4(c0, c1, c2, c3);
        __syncthreads();

        if (wv == 0) {
            float4 s = reinterpret_cast<const float4 *>(P[0])[lane];
#pragma unroll
            for (int v = 1; v < ST_WAVES; ++v) {
                const float4 p = reinterpret_cast<const float4 *>(P[v])[lane];
                s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
            }
            float bc = s.x;
            int bd = 4 * lane - ST_D;
            if (st_better(s.y, 4 * lane + 1 - ST_D, bc, bd)) { bc = s.y; bd = 4 * lane + 1 - ST_D; }
            if (st_better(s.z, 4 * lane + 2 - ST_D, bc, bd)) { bc = s.z; bd = 4 * lane + 2 - ST_D; }
            if (st_better(s.w, 4 * lane + 3 - ST_D, bc, bd)) { bc = s.w; bd = 4 * lane + 3 - ST_D; }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float oc = __shfl_xor(bc, o, 64);
                const int od = __shfl_xor(bd, o, 64);
                if (st_better(oc, od, bc, bd)) { bc = oc; bd = od; }
            }
            if (lane == 0) {
                s_delta = bd;
                if (sb) sb[i] = bd;
            }
        }
        __syncthreads();

        const int p = ST_D + s_delta;                      // R index of xz[p_i]: 0 .. 255
        const int64_t m = (int64_t)(i - 1) * ST_HS + tid;
        if (m < T_out) ob[m] = w_old * Tm[tid] + w_new * R[p + tid];
        const float n0 = R[p + ST_HS + tid], n1 = R[p + ST_HS + tid + ST_THREADS];
        __syncthreads();
        Tm[tid] = n0;
        Tm[tid + ST_THREADS] = n1;
        if (more) {
#pragma unroll
            for (int k = 0; k < ST_R / ST_THREADS; ++k) R[tid + k * ST_THREADS] = nx[k];
        }
        __syncthreads();
    }
}

}  // namespace grafp

extern "C" int grafp_time_stretch_f32(const float *x, int64_t x_stride, int B, int T_in, int64_t x_offset,
                                      const float *ratio, float *out, int64_t out_stride, int T_out, int32_t *shift,
                                      int64_t shift_stride, grafp_stream_t stream) {
    using namespace grafp;
    const int st = warp_check("time_stretch", x, x_stride, B, T_in, x_offset, ratio, out, out_stride, T_out, 1 << 30);
    if (st != GRAFP_OK) return st;
    const int frames = (T_out + ST_HS - 1) / ST_HS + 1;
    GRAFP_REQUIRE(!shift || shift_stride >= frames, "time_stretch: shift row stride %lld below the %d frames",
                  (long long)shift_stride, frames);
    GRAFP_REQUIRE((int64_t)B <= 0x7fffffff, "time_stretch: %d clips exceed the grid", B);      // one workgroup per clip
    hipLaunchKernelGGL(time_stretch_kernel, dim3((unsigned)B), dim3(ST_THREADS), 0, (hipStream_t)stream, x, x_stride, T_in,
                       x_offset, ratio, out, out_stride, T_out, shift, shift_stride, frames);
    GRAFP_CHECK_LAUNCH("time_stretch_kernel");
    return GRAFP_OK;
}
