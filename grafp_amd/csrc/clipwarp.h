// clipwarp.h -- what the per-clip warps of the second training view share: speed.hip (resampling, the pitch moves) and
// stretch.hip (WSOLA, the pitch stays).  Both warp every clip of a batch by its own ratio, read on the device.
// Compiles with and without the packed-f32 instructions; both users are built without (Makefile NOPK).
#pragma once
#include "common.h"

namespace grafp {

// the ratio rule: clamped to [0.5, 2]; a NaN counts as 1
__device__ __forceinline__ float warp_ratio(float r) {
    if (!(r == r)) return 1.0f;
    return r < 0.5f ? 0.5f : (r > 2.0f ? 2.0f : r);
}

// ratio == 1.0f exactly: outputs [m0, m_end) of one clip are a bit copy, ob[m] = xz[x_offset + m] (x_offset >= 0)
template <int THREADS>
__device__ __forceinline__ void warp_copy(const float *__restrict__ xb, int T_in, int64_t x_offset, float *__restrict__ ob,
                                          int m0, int m_end, int tid) {
    for (int m = m0 + tid; m < m_end; m += THREADS) {
        const int64_t s = x_offset + m;
        ob[m] = s < T_in ? xb[s] : 0.0f;
    }
}

// the host checks the two entry points share (name: the operation, for the message; max_out: a cap on T_out, 0 = none)
inline int warp_check(const char *name, const float *x, int64_t x_stride, int B, int T_in, int64_t x_offset,
                      const float *ratio, const float *out, int64_t out_stride, int T_out, int max_out) {
    GRAFP_REQUIRE(x && ratio && out, "%s: null pointer", name);
    GRAFP_REQUIRE(B > 0 && T_in > 0 && T_out > 0 && (!max_out || T_out <= max_out), "%s: bad sizes B=%d T_in=%d T_out=%d",
                  name, B, T_in, T_out);
    GRAFP_REQUIRE(x_stride >= T_in && out_stride >= T_out, "%s: row strides %lld / %lld below the row lengths %d / %d", name,
                  (long long)x_stride, (long long)out_stride, T_in, T_out);
    GRAFP_REQUIRE(x != out, "%s: out must not alias x", name);
    GRAFP_REQUIRE(x_offset >= 0 && x_offset <= ((int64_t)1 << 40), "%s: x_offset=%lld out of range", name, (long long)x_offset);
    return GRAFP_OK;
}

}  // namespace grafp
