// corpus.hip -- the device-resident training corpus (grafp_amd/data.py), gfx950.
//
// Replaces the per-item CPU work of the reference's NeuralfpDataset.__getitem__ (modules/data.py:45-89): the whole-track
// resample to cfg['fs'] runs ONCE per track at load time (resample_kernel), and every training step draws its (x_i, x_j)
// crops for the whole batch in one launch (draw_pairs_kernel).  The tracks live in one ragged bank (flat f32 buffer +
// per-track start and length), the layout of the augmentation banks of augment.hip.
//
//   * resample_kernel: torchaudio.transforms.Resample's default (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99)
//     as a polyphase filter: output j*new + p = sum_k tap[p][k] * x[j*orig + k - width], k < K = 2*width + orig, zeros
//     outside the track.  A workgroup owns JT tiles of 64 consecutive output blocks j and stages the input window they
//     touch ((64*JT - 1)*orig + K samples) in LDS once; lane = block j, and a wave computes RS_P consecutive phases of its
//     64 blocks: per tap index k ONE LDS read feeds RS_P fmaf (the taps are wave-uniform, stored [phase block][k][RS_P],
//     and compile to scalar loads).  Every output is one fmaf chain in increasing k, so a track's samples do not depend
//     on what else is in the launch.  2*K flops per output sample (K = 475 for 44.1 -> 16 kHz): compute-bound.
//   * draw_pairs_kernel: one workgroup per batch row.  Attempt a reads the 1.05 s window of track (t0 + a) mod n into LDS
//     once, takes max|x_i| and max|x_j| from it, and either rejects the attempt (silence) or writes both views, divided by
//     the track's quantile norm, straight from LDS.  HBM-bound: window read once, two views written once.
//
// Built WITHOUT packed-f32 instructions (Makefile: -target-feature -packed-fp32-ops for this file only): the packed
// form whose low lane reads the high register of a pair is the hazard of DESIGN.md section 12.7b, and the scalar
// v_fma_f32 already issues at the full f32 vector rate (64 flop/clk/SIMD).
#include <math.h>

#include "common.h"

namespace grafp {

constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_P = GRAFP_RESAMPLE_PHASES;      // phases per wave item
constexpr int RS_KU = 4;                         // tap indices per unrolled step (taps padded to a multiple)
constexpr int RS_LDS_FLOATS = 160 * 1024 / 4;    // the whole LDS of a CU

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float *__restrict__ x,
                                                              const int64_t *__restrict__ in_start,
                                                              const int64_t *__restrict__ in_len,
                                                              const int64_t *__restrict__ out_start, int orig, int nw,
                                                              int width, int K4, int n_pb, int JT,
                                                              const float *__restrict__ taps, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float win[];
    const int tr = blockIdx.y, tid = threadIdx.x;
    const int64_t L = in_len[tr];
    const int64_t out_len = (L * nw + orig - 1) / orig;
    const int64_t n_j = (out_len + nw - 1) / nw;
    const int64_t j0 = (int64_t)blockIdx.x * 64 * JT;
    if (j0 >= n_j) return;
    const float *xt = x + in_start[tr];
    float *ot = out + out_start[tr];
    const int64_t s0 = j0 * orig - width;
    const int W = (64 * JT - 1) * orig + K4;
    for (int i = tid; i < W; i += RS_THREADS) {
        const int64_t s = s0 + i;
        win[i] = (s >= 0 && s < L) ? xt[s] : 0.0f;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int item = wave; item < JT * n_pb; item += RS_WAVES) {
        const int t = item / n_pb, pb = item - t * n_pb;
        if (j0 + (int64_t)t * 64 >= n_j) break;          // wave-uniform: items are ordered by tile
        const float *w = win + (t * 64 + lane) * orig;
        const float *tp = taps + (size_t)pb * K4 * RS_P;
        float acc[RS_P];
#pragma unroll
        for (int q = 0; q < RS_P; ++q) acc[q] = 0.0f;
        for (int k = 0; k < K4; k += RS_KU) {
            float xv[RS_KU];
#pragma unroll
            for (int u = 0; u < RS_KU; ++u) xv[u] = w[k + u];
#pragma unroll
            for (int u = 0; u < RS_KU; ++u)
#pragma unroll
                for (int q = 0; q < RS_P; ++q) acc[q] = __builtin_fmaf(tp[(k + u) * RS_P + q], xv[u], acc[q]);
        }
        const int64_t j = j0 + t * 64 + lane;
#pragma unroll
        for (int q = 0; q < RS_P; ++q) {
            const int p = pb * RS_P + q;
            const int64_t o = j * nw + p;
            if (p < nw && o < out_len) ot[o] = acc[q];
        }
    }
}

// orig == new: the track is returned unchanged (bit for bit)
__global__ __launch_bounds__(256) void copy_tracks_kernel(const float *__restrict__ x, const int64_t *__restrict__ in_start,
                                                          const int64_t *__restrict__ in_len,
                                                          const int64_t *__restrict__ out_start, float *__restrict__ out) {
    const int tr = blockIdx.y;
    const int64_t L = in_len[tr];
    const float *xt = x + in_start[tr];
    float *ot = out + out_start[tr];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) ot[i] = xt[i];
}

constexpr int DP_THREADS = 1024;
constexpr int DP_MAX_WINDOW = RS_LDS_FLOATS - 2 * DP_THREADS / 64 * 2;      // next to the reduction scratch

__device__ __forceinline__ float2 dp_block_max2(float a, float b, float2 *scratch, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a = fmaxf(a, __shfl_xor(a, o));
        b = fmaxf(b, __shfl_xor(b, o));
    }
    if ((tid & 63) == 0) scratch[tid >> 6] = make_float2(a, b);
    __syncthreads();
    float2 r = scratch[0];
    for (int w = 1; w < DP_THREADS / 64; ++w) {
        r.x = fmaxf(r.x, scratch[w].x);
        r.y = fmaxf(r.y, scratch[w].y);
    }
    return r;
}

__device__ __forceinline__ int64_t dp_pick(float u, int64_t n) {      // min(floor(u * n), n - 1), n >= 1
    const int64_t r = (int64_t)floor((double)u * (double)n);
    return r < n - 1 ? r : n - 1;
}

__global__ __launch_bounds__(DP_THREADS) void draw_pairs_kernel(const float *__restrict__ bank,
                                                                const int64_t *__restrict__ track_start,
                                                                const int64_t *__restrict__ track_len,
                                                                const float *__restrict__ norm, int n_tracks,
                                                                const int32_t *__restrict__ row_track,
                                                                const float *__restrict__ uniforms, int A, int clip,
                                                                int offset_mod, float silence, float *__restrict__ x_i,
                                                                float *__restrict__ x_j, int32_t *__restrict__ silent_rows) {
    extern __shared__ __attribute__((aligned(16))) float win[];
    __shared__ float2 scratch[2][DP_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = row_track[b];
    const int nc = offset_mod - clip;
    for (int a = 0; a < A; ++a) {
        const int tr = (int)(((t0 % n_tracks) + n_tracks + a) % n_tracks);
        const int64_t len = track_len[tr];
        const float *y = bank + track_start[tr];
        const float *u = uniforms + ((size_t)b * A + a) * 3;
        const int64_t r = len - offset_mod >= 1 ? dp_pick(u[0], len - offset_mod) : 0;
        const int ri = (int)dp_pick(u[1], nc), rj = (int)dp_pick(u[2], nc);
        __syncthreads();                                  // the previous attempt's readers are done with win
        for (int i = tid; i < offset_mod; i += DP_THREADS) win[i] = r + i < len ? y[r + i] : 0.0f;
        __syncthreads();
        float mi = 0.0f, mj = 0.0f;
        for (int i = tid; i < clip; i += DP_THREADS) {
            mi = fmaxf(mi, fabsf(win[ri + i]));
            mj = fmaxf(mj, fabsf(win[rj + i]));
        }
        const float2 m = dp_block_max2(mi, mj, scratch[a & 1], tid);
        const bool silent = m.x < silence || m.y < silence;
        if (!silent || a == A - 1) {
            const float nv = norm[tr];
            float *oi = x_i + (size_t)b * clip, *oj = x_j + (size_t)b * clip;
            for (int i = tid; i < clip; i += DP_THREADS) {
                oi[i] = win[ri + i] / nv;
                oj[i] = win[rj + i] / nv;
            }
            if (silent && tid == 0 && silent_rows) atomicAdd(silent_rows, 1);
            return;
        }
    }
}

// The launch plan of a rate pair, written once: resample_launch and grafp_resample_plan (capi.hip) read it.  Tiles of 64
// output blocks per workgroup: enough wave items for the 16 waves, as long as the window fits the LDS.
// info = {JT, n_pb, K4, W, LDS bytes, output blocks j per workgroup, input samples per workgroup tile, 0}
int resample_plan(int orig, int nw, int K, int *info) {
    const int K4 = (K + RS_KU - 1) / RS_KU * RS_KU;
    const int n_pb = (nw + RS_P - 1) / RS_P;
    int JT = (RS_WAVES + n_pb - 1) / n_pb;
    while (JT > 1 && (int64_t)(64 * JT - 1) * orig + K4 > RS_LDS_FLOATS) --JT;
    const int64_t W = (int64_t)(64 * JT - 1) * orig + K4;
    GRAFP_REQUIRE(W <= RS_LDS_FLOATS, "resample: rate ratio %d/%d needs a %lld-sample window (LDS holds %d)", nw, orig,
                  (long long)W, RS_LDS_FLOATS);
    info[0] = JT; info[1] = n_pb; info[2] = K4; info[3] = (int)W; info[4] = (int)(W * sizeof(float));
    info[5] = 64 * JT; info[6] = 64 * JT * orig; info[7] = 0;
    return GRAFP_OK;
}

int resample_launch(const float *in, const int64_t *in_start, const int64_t *in_len, const int64_t *out_start,
                    int n_tracks, int64_t max_in_len, int orig, int nw, int width, int K, const float *taps, float *out,
                    hipStream_t stream) {
    if (orig == nw) {
        const int64_t blocks = (max_in_len + 255) / 256;
        const dim3 grid((unsigned)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096), n_tracks);
        hipLaunchKernelGGL(copy_tracks_kernel, grid, dim3(256), 0, stream, in, in_start, in_len, out_start, out);
        GRAFP_CHECK_LAUNCH("copy_tracks_kernel");
        return GRAFP_OK;
    }
    GRAFP_REQUIRE(taps, "resample: null taps");
    int plan[8];
    if (int e = resample_plan(orig, nw, K, plan)) return e;
    const int JT = plan[0], n_pb = plan[1], K4 = plan[2];
    const int64_t max_out = (max_in_len * nw + orig - 1) / orig;
    const int64_t n_j = (max_out + nw - 1) / nw;
    const int64_t tiles = (n_j + 64 * JT - 1) / (64 * JT);
    GRAFP_REQUIRE(tiles <= 0x7fffffff, "resample: track too long");
    if (tiles == 0) return GRAFP_OK;
    const size_t lds = (size_t)plan[4];
    if (hipFuncSetAttribute((const void *)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("resample: cannot reserve %zu bytes of LDS", lds);
        return GRAFP_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, n_tracks), dim3(RS_THREADS), lds, stream, in, in_start,
                       in_len, out_start, orig, nw, width, K4, n_pb, JT, taps, out);
    GRAFP_CHECK_LAUNCH("resample_kernel");
    return GRAFP_OK;
}

int draw_pairs_launch(const float *bank, const int64_t *track_start, const int64_t *track_len, const float *norm,
                      int n_tracks, const int32_t *row_track, const float *uniforms, int B, int A, int clip,
                      int offset_mod, float silence, float *x_i, float *x_j, int32_t *silent_rows, hipStream_t stream) {
    GRAFP_REQUIRE(offset_mod <= DP_MAX_WINDOW, "draw_pairs: window of %d samples exceeds the LDS (%d)", offset_mod,
                  DP_MAX_WINDOW);
    const size_t lds = (size_t)offset_mod * sizeof(float);
    if (hipFuncSetAttribute((const void *)draw_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("draw_pairs: cannot reserve %zu bytes of LDS", lds);
        return GRAFP_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(draw_pairs_kernel, dim3(B), dim3(DP_THREADS), lds, stream, bank, track_start, track_len, norm,
                       n_tracks, row_track, uniforms, A, clip, offset_mod, silence, x_i, x_j, silent_rows);
    GRAFP_CHECK_LAUNCH("draw_pairs_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
