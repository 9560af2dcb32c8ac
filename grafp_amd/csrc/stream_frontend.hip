// stream_frontend.hip -- the front end of live multi-channel monitoring (grafp_amd/monitor.py).
//
// Every channel of a monitor is an open-ended stream.  A push brings one ragged chunk per channel; the host keeps, per
// channel, the few samples a later frame still reads (the "carry") and says which frames became computable.  Two
// launches, whatever the number of channels:
//   stream_logmel1024_kernel  the new frames [frame_lo, frame_hi) of every channel into the channel's spectrogram ring
//                             (frame f at column f & (R - 1)); the arithmetic is lm1k_pair of logmel_core.h, the body
//                             of logmel1024_kernel, so a frame has the bits grafp_logmel_f32 gives on the whole stream;
//   stream_segments_kernel    the new segments [seg_lo, seg_hi) of every channel, read through the ring, packed channel
//                             by channel: the values of grafp_unfold_segments_f32 on the whole spectrogram.
// A workgroup finds its channel in a prefix table (workgroups, resp. segments, per channel) by bisection; there is no
// launch per channel and no grid dimension of C.
//
// Positions: a channel's buffer holds the stream's samples [base, base + len); absolute positions, f * hop and frame
// numbers are 64-bit (a feed that runs for weeks does not wrap), the sample index inside the buffer is 32-bit.
#include "common.h"
#include "logmel_core.h"

namespace grafp {

// largest c in [0, C) with first[c] <= v (first: C + 1 non-decreasing entries, first[0] = 0, v < first[C])
__device__ __forceinline__ int sf_find(const int32_t *__restrict__ first, int C, int v) {
    int lo = 0, hi = C;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

struct SfRingDst {
    float *__restrict__ plane;                 // the channel's (n_mels, R) ring
    int R, col;                                // col = f0 & (R - 1): even, so f1's column is the next one
    __device__ __forceinline__ float *row(int m) const { return plane + (size_t)m * R + col; }
};

__global__ __launch_bounds__(256, 2) void stream_logmel1024_kernel(
    const float *__restrict__ bank, const int64_t *__restrict__ buf_start, const int32_t *__restrict__ buf_len,
    const int64_t *__restrict__ buf_base, const int64_t *__restrict__ frame_lo, const int64_t *__restrict__ frame_hi,
    const int32_t *__restrict__ group_first, int C, int hop, int n_mels, int R, const float *__restrict__ window,
    const float2 *__restrict__ twiddle, const float *__restrict__ fb, const int *__restrict__ band_lo,
    const int *__restrict__ band_hi, float *__restrict__ ring) {
    __shared__ float2 lds[LM1K_PAIRS][32 * LM1K_ROW];
    __shared__ float wband[64][LM1K_BW];
    const int tid = threadIdx.x, l = tid & 31, g = tid >> 5;
    lm1k_stage_filters(wband, n_mels, fb, band_lo, band_hi, tid);
    __syncthreads();                              // (the only workgroup barrier; before any half-wave leaves)
    const int c = sf_find(group_first, C, (int)blockIdx.x);          // workgroup-uniform: one channel per workgroup
    const int64_t f0 = frame_lo[c] + 2 * (int64_t)(((int)blockIdx.x - group_first[c]) * LM1K_PAIRS + g);
    const int64_t hi = frame_hi[c];
    if (f0 >= hi) return;                         // (a whole half-wave; nobody waits for it)
    const int T = buf_len[c];                     // the buffer ends where the stream does so far: the reflection's T
    if (T <= 0) return;
    const float *x = bank + buf_start[c];
    // position of frame f0's centre relative to the buffer: the host keeps it within a hop of the buffer, so it is 32-bit
    const int f0hop = (int)(f0 * (int64_t)hop - buf_base[c]);
    const SfRingDst dst{ring + (size_t)c * n_mels * R, R, (int)(f0 & (int64_t)(R - 1))};
    lm1k_pair<true>(x, T, dst, f0hop, hop, f0 + 1 < hi, n_mels, window, twiddle[l], fb, band_lo, band_hi, wband, lds[g],
                    l);
}

// one workgroup per new segment
__global__ __launch_bounds__(256) void stream_segments_kernel(const float *__restrict__ ring,
                                                              const int64_t *__restrict__ seg_lo,
                                                              const int32_t *__restrict__ seg_first, int C, int n_mels,
                                                              int R, int size, int step, float *__restrict__ seg) {
    const int sg = blockIdx.x;
    const int c = sf_find(seg_first, C, sg);
    const int64_t fr0 = (seg_lo[c] + (sg - seg_first[c])) * (int64_t)step;
    const float *plane = ring + (size_t)c * n_mels * R;
    float *o = seg + (size_t)sg * n_mels * size;
    for (int i = threadIdx.x; i < n_mels * size; i += 256) {
        const int m = i / size, j = i - m * size;
        o[i] = plane[(size_t)m * R + (int)((fr0 + j) & (int64_t)(R - 1))];
    }
}

// ---- launches (argument checks: capi.hip) ----------------------------------------------------------------------------
int stream_logmel_launch(const float *bank, const int64_t *buf_start, const int32_t *buf_len, const int64_t *buf_base,
                         const int64_t *frame_lo, const int64_t *frame_hi, const int32_t *group_first, int n_channels,
                         int n_groups, int hop, int n_mels, int ring_len, const float *window, const float *twiddle,
                         const float *fb, const int32_t *band_lo, const int32_t *band_hi, float *ring,
                         hipStream_t stream) {
    hipLaunchKernelGGL(stream_logmel1024_kernel, dim3(n_groups), dim3(256), 0, stream, bank, buf_start, buf_len,
                       buf_base, frame_lo, frame_hi, group_first, n_channels, hop, n_mels, ring_len, window,
                       reinterpret_cast<const float2 *>(twiddle), fb, band_lo, band_hi, ring);
    GRAFP_CHECK_LAUNCH("stream_logmel1024_kernel");
    return GRAFP_OK;
}

int stream_segments_launch(const float *ring, const int64_t *seg_lo, const int32_t *seg_first, int n_channels,
                           int n_segments, int n_mels, int ring_len, int size, int step, float *seg,
                           hipStream_t stream) {
    hipLaunchKernelGGL(stream_segments_kernel, dim3(n_segments), dim3(256), 0, stream, ring, seg_lo, seg_first,
                       n_channels, n_mels, ring_len, size, step, seg);
    GRAFP_CHECK_LAUNCH("stream_segments_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
