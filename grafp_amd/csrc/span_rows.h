// span_rows.h -- where the library rows of a span score come from: the Span functors that identify_core.h's identify_item
// and selfmatch_core.h's match_source take,
//     float span(const float4 *x, int64_t row, int l, int m)
// x: lane l's float4 of the first query (source) row of the span, row: the library row that pairs with it, m: pairs (the
// same in every lane of the half-wave; <= 0: no row is read, the butterfly still runs).  Returns the un-divided span
// score in span_sum's order (seqmatch.h).
//   RowSpan<kUnroll>      the library's resident (n, 128) f32 rows     identify.hip, selfmatch.hip, crossmatch.hip
//   StridedRowSpan<kUnroll>   the same rows, the x rows of consecutive pairs x_step float4s apart    identify_thin.hip
//   TempoRowSpan<kUnroll>     the same rows, gathered along a sloped alignment (its own call, see there)  identify_tempo.hip, identify_tempo_items.hip
//   StepRowSpan<kUnroll>      the same rows, the library rows of consecutive pairs Q rows apart (its own loop)  identify_stride.hip
//   PqSpan<kM, kUnroll>   rows decoded from IVF-PQ codes while scored  identify_pq.hip, crossmatch.hip
//   Bf16RowSpan<kUnroll>  the half form's resident (n, 128) bf16 rows, widened in registers  identify_half.hip, crossmatch_half.hip
// Library row r of the half form is U[r] = the f32 value of its bf16 row (the bits shifted up by 16: exact), so
// Bf16RowSpan returns the bits RowSpan returns on the (n, 128) f32 array U.
// Library row r of the compact form is
//   dec[r][j] = centroids[list_id[r]][j] + codebooks[m][codes[r][m]][c],  m = j / dsub, c = j % dsub, dsub = 128 / M
// (one f32 add per element, never an fma), so PqSpan returns the bits RowSpan returns on the (n, 128) f32 array dec.
// kUnroll: row pairs loaded (rows decoded) ahead of the fmaf chain; every kernel states its own count.
// Compiles with and without the packed-f32 instructions; every user is built without (Makefile NOPK).
#pragma once
#include "common.h"
#include "seqmatch.h"

namespace grafp {

template <int kUnroll>
struct RowSpan {
    const float4 *rw4;
    __device__ __forceinline__ float operator()(const float4 *x, int64_t row, int l, int m) const {
        return span_sum<kUnroll>(x, rw4 + row * (SEQ_D / 4) + l, m);
    }
};

template <int kUnroll>
struct StridedRowSpan {
    const float4 *rw4;
    int x_step;                                  // float4s between the x rows of two consecutive pairs
    __device__ __forceinline__ float operator()(const float4 *x, int64_t row, int l, int m) const {
        return span_sum<kUnroll>(x, rw4 + row * (SEQ_D / 4) + l, m, x_step);
    }
};

// The pairs of a recording that runs at num / 256 of the catalogue's speed (TempoGrid of identify_core.h): pair t is
// query row lo + t with library row a + w(lo + t), w(s) = (s * num + 128) >> 8, so the library rows are gathered (one
// row may be read twice, rows may be skipped).  span_sum's order; at num = 256 the rows and so the bits are RowSpan's.
template <int kUnroll>
struct TempoRowSpan {
    const float4 *rw4;
    __device__ __forceinline__ float operator()(const float4 *x, int64_t a, int lo, int num, int l, int m) const {
        float acc = 0.0f;
#pragma unroll kUnroll
        for (int t = 0; t < m; ++t) {
            const int64_t row = a + (((lo + t) * num + 128) >> 8);
            const float4 q = x[(int64_t)t * (SEQ_D / 4)], r = rw4[row * (SEQ_D / 4) + l];
            acc = __builtin_fmaf(q.x, r.x, acc);
            acc = __builtin_fmaf(q.y, r.y, acc);
            acc = __builtin_fmaf(q.z, r.z, acc);
            acc = __builtin_fmaf(q.w, r.w, acc);
        }
#pragma unroll
        for (int s = 16; s > 0; s >>= 1) acc += __shfl_xor(acc, s);      // stays inside the 32-lane half
        return acc;
    }
};

// The pairs of an item that holds every Q-th segment of the recording (StrideGrid of identify_core.h): pair t is query
// row x + t with library row `row` + t * Q, each still one whole 512-byte row per half-wave.  span_sum's order; at Q = 1
// the rows and so the bits are RowSpan's, at Q = 2 TempoRowSpan's at num = 512.
template <int kUnroll>
struct StepRowSpan {
    const float4 *rw4;
    int Q;                                       // library rows between two consecutive pairs
    __device__ __forceinline__ float operator()(const float4 *x, int64_t row, int l, int m) const {
        const float4 *y = rw4 + row * (SEQ_D / 4) + l;
        const int64_t y_step = (int64_t)Q * (SEQ_D / 4);
        float acc = 0.0f;
#pragma unroll kUnroll
        for (int t = 0; t < m; ++t) {
            const float4 q = x[(int64_t)t * (SEQ_D / 4)], r = y[t * y_step];
            acc = __builtin_fmaf(q.x, r.x, acc);
            acc = __builtin_fmaf(q.y, r.y, acc);
            acc = __builtin_fmaf(q.z, r.z, acc);
            acc = __builtin_fmaf(q.w, r.w, acc);
        }
#pragma unroll
        for (int s = 16; s > 0; s >>= 1) acc += __shfl_xor(acc, s);      // stays inside the 32-lane half
        return acc;
    }
};

// The rows of a library held as bf16 (the half form): lane l reads the 8 bytes that hold its dims 4l..4l+3 -- a half-wave
// reads the row's 256 bytes as one access -- and widens them by shifts (a bf16 is the upper half of its f32).  span_sum's
// order on the widened values, so the bits are RowSpan's on the f32 array of those values.
template <int kUnroll>
struct Bf16RowSpan {
    const uint2 *rh2;                            // the (n, 128) bf16 rows, SEQ_D / 4 uint2 each
    __device__ __forceinline__ float operator()(const float4 *x, int64_t row, int l, int m) const {
        const uint2 *y = rh2 + row * (SEQ_D / 4) + l;
        float acc = 0.0f;
#pragma unroll kUnroll
        for (int t = 0; t < m; ++t) {
            const float4 q = x[(int64_t)t * (SEQ_D / 4)];
            const uint2 w = y[(int64_t)t * (SEQ_D / 4)];
            acc = __builtin_fmaf(q.x, __uint_as_float(w.x << 16), acc);
            acc = __builtin_fmaf(q.y, __uint_as_float(w.x & 0xffff0000u), acc);
            acc = __builtin_fmaf(q.z, __uint_as_float(w.y << 16), acc);
            acc = __builtin_fmaf(q.w, __uint_as_float(w.y & 0xffff0000u), acc);
        }
#pragma unroll
        for (int s = 16; s > 0; s >>= 1) acc += __shfl_xor(acc, s);      // stays inside the 32-lane half
        return acc;
    }
};

template <int kM, int kUnroll>
struct PqSpan {
    const int32_t *__restrict__ list_id;        // (n)
    const unsigned char *__restrict__ codes;    // (n, kM), library row order
    const float *__restrict__ centroids;        // (nlist, 128)
    const float *__restrict__ codebooks;        // (kM, 256, 128 / kM)
    int nlist;

    // lane l's four floats of the codewords of row `cr`
    __device__ __forceinline__ float4 codeword(const unsigned char *cr, int l) const {
        constexpr int dsub = SEQ_D / kM;
        if (kM == 16) {
            const int m = l >> 1;
            return *reinterpret_cast<const float4 *>(codebooks + ((size_t)m * 256 + cr[m]) * dsub + (l & 1) * 4);
        } else if (kM == 32) {
            return *reinterpret_cast<const float4 *>(codebooks + ((size_t)l * 256 + cr[l]) * dsub);
        } else if (kM == 64) {
            const unsigned int cc = reinterpret_cast<const unsigned short *>(cr)[l];
            const float2 w0 = *reinterpret_cast<const float2 *>(codebooks + ((size_t)(2 * l) * 256 + (cc & 255u)) * dsub);
            const float2 w1 = *reinterpret_cast<const float2 *>(codebooks + ((size_t)(2 * l + 1) * 256 + (cc >> 8)) * dsub);
            return make_float4(w0.x, w0.y, w1.x, w1.y);
        } else {
            const unsigned int cc = reinterpret_cast<const unsigned int *>(cr)[l];
            return make_float4(codebooks[(size_t)(4 * l) * 256 + (cc & 255u)],
                               codebooks[(size_t)(4 * l + 1) * 256 + ((cc >> 8) & 255u)],
                               codebooks[(size_t)(4 * l + 2) * 256 + ((cc >> 16) & 255u)],
                               codebooks[(size_t)(4 * l + 3) * 256 + (cc >> 24)]);
        }
    }

    __device__ __forceinline__ float operator()(const float4 *x, int64_t row, int l, int m) const {
        const float4 *c4 = reinterpret_cast<const float4 *>(centroids);
        float acc = 0.0f;
#pragma unroll kUnroll
        for (int t = 0; t < m; ++t) {
            const int64_t r = row + t;
            int lid = list_id[r];
            lid = lid < 0 ? 0 : (lid < nlist ? lid : nlist - 1);       // (valid list ids need no clamp)
            const float4 q = x[(int64_t)t * (SEQ_D / 4)];
            const float4 c = c4[(size_t)lid * (SEQ_D / 4) + l];
            const float4 w = codeword(codes + r * kM, l);
            acc = __builtin_fmaf(q.x, c.x + w.x, acc);
            acc = __builtin_fmaf(q.y, c.y + w.y, acc);
            acc = __builtin_fmaf(q.z, c.z + w.z, acc);
            acc = __builtin_fmaf(q.w, c.w + w.w, acc);
        }
#pragma unroll
        for (int s = 16; s > 0; s >>= 1) acc += __shfl_xor(acc, s);      // stays inside the 32-lane half
        return acc;
    }
};

}  // namespace grafp
