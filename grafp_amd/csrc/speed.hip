// speed.hip -- speed augmentation of the second training view (grafp_amd/modules/transformations.py), gfx950.
//
// One launch resamples every clip of a batch by its OWN ratio, read on the device (so the launch can be captured into a
// HIP graph and every replay reads fresh ratios).  Radio, turntables and re-uploads change speed by resampling, which
// moves the pitch with the tempo; this is that, per clip.
//
// THE RULE.  For clip b:
//   rho = ratio[b] clamped to [0.5, 2]; a NaN counts as 1.  rho is input samples per output sample: above 1 the clip
//         plays fast and its pitch rises.
//   c   = 0.99 * min(1, 1 / rho)                          (the cut-off, as a fraction of the input's Nyquist rate)
//   p   = x_offset + m * rho                              (the input position of output m)
//   out[b][m] = sum over k = ceil(p - 6/c) .. floor(p + 6/c), k ascending, of xz[b][k] * h(k - p)
//   xz  = x inside [0, T_in), 0 outside
//   h(u) = c * sinc(pi t) * cos^2(pi t / 12),  t = clip(c u, -6, 6)
//   the sum is ONE fmaf chain starting from 0; no atomics: a clip's samples do not depend on the rest of the launch.
//   rho == 1.0f exactly: out[b][m] = xz[b][x_offset + m], a bit copy (the 0.99 roll-off filter is not the identity).
// This is the filter family of corpus.hip's resample_kernel (torchaudio's sinc_interp_hann, width 6, rolloff 0.99)
// evaluated at an arbitrary position instead of on a polyphase grid: 13 taps up to rho = 1, 25 at rho = 2.
//
// THE ROUTE (tests/_speed_ref.speed_f32 restates it operation by operation):
//   * p is formed in f64 from the f32 rho (m * rho is exact there); ip = floor(p) and f = (float)(p - ip) leave it.
//     Only the small integer j = k - ip and f go to f32: u = (float)j - f, t = c * u.  (An f32 m * rho is off by 1e-3
//     sample at m = 16 000.)
//   * candidates j = -W .. W + 1 with W = floor(6 / c); a tap is used iff |t| <= 6 -- the rule's range, decided in f32.
//     (Where the two decisions differ, at |t| = 6 to rounding, h is 0 to 1e-13: the window has a double zero there.)
//   * sin(pi t) = (-1)^n sinf(pi * (t - n)), n = rintf(t): the subtraction is exact, sinf sees |arg| <= pi/2;
//     sinc = that / (pi * t), 1 at t == 0; window = cosf(t * (pi/12)) squared; h = ((c * sinc) * w) * w.
//
// A workgroup owns SP_TILE consecutive outputs of one clip and stages the input span they touch (at most
// (SP_TILE - 1) * 2 + 2 * 12 + 3 samples) in LDS once.  Bound by the tap arithmetic (sinf, cosf and an IEEE division per
// tap), not by HBM: DESIGN.md section 12.23.
//
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as corpus.hip is: DESIGN.md section 12.7b.
#include <math.h>

#include "clipwarp.h"
#include "common.h"

namespace grafp {

constexpr int SP_THREADS = 256;
constexpr int SP_PER_THREAD = 4;
constexpr int SP_TILE = SP_THREADS * SP_PER_THREAD;      // outputs per workgroup
constexpr int SP_WMAX = 13;                               // floor(6 / c) is 12 at rho = 2, the largest
constexpr int SP_STAGE = (SP_TILE - 1) * 2 + 2 * SP_WMAX + 4;
constexpr float SP_PI = 3.14159265358979323846f;
constexpr float SP_PI_12 = 0.26179938779914943654f;

__global__ __launch_bounds__(SP_THREADS) void speed_change_kernel(const float *__restrict__ x, int64_t x_stride, int T_in,
                                                                  int64_t x_offset, const float *__restrict__ ratio,
                                                                  float *__restrict__ out, int64_t out_stride, int T_out,
                                                                  int tiles) {
    __shared__ float win[SP_STAGE];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles, tid = threadIdx.x;
    const float *xb = x + (int64_t)b * x_stride;
    float *ob = out + (int64_t)b * out_stride;
    const float rho = warp_ratio(ratio[b]);
    const int m0 = tile * SP_TILE;
    const int m_end = min(T_out, m0 + SP_TILE);            // > m0: the grid covers T_out exactly

    if (rho == 1.0f)                                       // wave-uniform: the whole workgroup copies
        return warp_copy<SP_THREADS>(xb, T_in, x_offset, ob, m0, m_end, tid);

    const float c = 0.99f * fminf(1.0f, 1.0f / rho);
    const int W = min(SP_WMAX, (int)(6.0f / c + 1e-3f));   // floor(6 / c); the nudge keeps an integer 6 / c from rounding
    //                                                        below itself (taps past |t| = 6 are skipped below anyway)
    const double rd = (double)rho, od = (double)x_offset;
    const int64_t s0 = (int64_t)floor(od + (double)m0 * rd) - W;
    // the span ends with the last output's last candidate: <= (SP_TILE - 1) * 2 + 1 + 2 * W + 1 < SP_STAGE
    const int span = min(SP_STAGE, (int)((int64_t)floor(od + (double)(m_end - 1) * rd) - s0) + W + 2);
    for (int i = tid; i < span; i += SP_THREADS) {
        const int64_t s = s0 + i;
        win[i] = (s >= 0 && s < T_in) ? xb[s] : 0.0f;
    }
    __syncthreads();

    for (int m = m0 + tid; m < m_end; m += SP_THREADS) {
        const double p = od + (double)m * rd;
        const double fl = floor(p);
        const float f = (float)(p - fl);
        const float *w = win + ((int64_t)fl - s0);         // candidate j lives at w[j]; j >= -W keeps it >= win
        float acc = 0.0f;
        for (int j = -W; j <= W + 1; ++j) {
            const float t = c * ((float)j - f);
            if (fabsf(t) <= 6.0f) {
                const float n = rintf(t);
                float s = sinf(SP_PI * (t - n));
                if ((int)n & 1) s = -s;
                const float sinc = t == 0.0f ? 1.0f : s / (SP_PI * t);
                const float cw = cosf(t * SP_PI_12);
                acc = __builtin_fmaf(w[j], c * sinc * cw * cw, acc);
            }
        }
        ob[m] = acc;
    }
}

}  // namespace grafp

extern "C" int grafp_speed_change_f32(const float *x, int64_t x_stride, int B, int T_in, int64_t x_offset,
                                      const float *ratio, float *out, int64_t out_stride, int T_out,
                                      grafp_stream_t stream) {
    using namespace grafp;
    const int st = warp_check("speed_change", x, x_stride, B, T_in, x_offset, ratio, out, out_stride, T_out, 0);
    if (st != GRAFP_OK) return st;
    const int64_t tiles = ((int64_t)T_out + SP_TILE - 1) / SP_TILE;
    GRAFP_REQUIRE(tiles * B <= 0x7fffffff, "speed_change: %d clips of %d outputs exceed the grid", B, T_out);
    hipLaunchKernelGGL(speed_change_kernel, dim3((unsigned)(tiles * B)), dim3(SP_THREADS), 0, (hipStream_t)stream, x,
                       x_stride, T_in, x_offset, ratio, out, out_stride, T_out, (int)tiles);
    GRAFP_CHECK_LAUNCH("speed_change_kernel");
    return GRAFP_OK;
}
