// elemio.h -- how ONE f32 or bf16 element, or a vector of them, is read, widened, narrowed and stored (gfx950 only).
// Said once for the training path's element-wise kernels, the GEMM epilogues and the k-NN operand copies (DESIGN.md
// section 12.13).  bf16 is carried as unsigned short; a packed PAIR is one 32-bit word, element 0 in the low half.
//
// GRAFP_ST_NT (common.h) depends on GRAFP_STORE_FAMILY, which a .hip file defines BEFORE its first include: the streaming
// arm of ElemIO::store therefore belongs to the including file's family in the experiment builds, as it always did.
#pragma once
#include <type_traits>

#include "common.h"
#include "tuning.h"

namespace grafp {

// ---- widening: exact ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ float ld_as_f32(const float *p) { return *p; }
__device__ __forceinline__ float ld_as_f32(const unsigned short *p) { return __uint_as_float(((unsigned)*p) << 16); }

// ---- narrowing: round to nearest even, NaN stays NaN ----------------------------------------------------------------------
// The PAIR form, v_cvt_pk_bf16_f32: one instruction per pair instead of the six per value of the integer form (a seventh
// of the BatchNorm backward's vector instructions).  What activations and gradients are stored with.
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    const f2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
}
// The SCALAR form, in integer arithmetic: exact for f32 denormals whatever the float mode, so the operand copies of the
// index-valued kernels (knn_pre.hip, knn_search.hip), whose results are a bit contract, and every one-element tail use it.
__device__ __forceinline__ unsigned short f32_to_bf16(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// ---- 4 elements (Raw4: 16 B of f32 / 8 B of bf16) and 16 bytes (Raw: W = 4 f32 / 8 bf16) as they sit in registers --------
// load / unpack / store pick the piece by the length of `v`; pack is the inverse of unpack for the 4-element piece.
// The CALLER guarantees that the address is aligned to the piece (its launcher checks base pointers, strides and row
// lengths and otherwise takes the one-element kernels).
// store: `plain` is wave-uniform and comes from plain_stores() below or is a constant; false = the streaming hint (outputs
// are read by a later launch: a plain-store copy of a 67-268 MB tensor runs at 3.7-4.9 TB/s on MI355X, the same copy with
// `nt` stores at 6.2-6.7 TB/s, tools/microbench/copy_bench.hip).
template <typename T> struct ElemIO;
template <> struct ElemIO<float> {
    static constexpr int W = 4;
    using Raw4 = float4;
    using Raw = float4;
    __device__ static void unpack(const float4 &t, float (&v)[4]) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    __device__ static float4 pack(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }
    __device__ static void load(const float *p, float (&v)[4]) { unpack(*reinterpret_cast<const float4 *>(p), v); }
    __device__ static void store(float *p, const float (&v)[4], bool plain) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 t = {v[0], v[1], v[2], v[3]};
        if (plain) store16_hint(p, __builtin_bit_cast(st_u32x4, t), true);
        else GRAFP_ST_NT(t, reinterpret_cast<f4 *>(p));
    }
    __device__ static float ld1(const float *p) { return *p; }
    __device__ static void st1(float *p, float v) { *p = v; }
};
template <> struct ElemIO<unsigned short> {
    static constexpr int W = 8;
    using Raw4 = uint2;
    using Raw = uint4;
    __device__ static void unpack(const uint2 &t, float (&v)[4]) {
        v[0] = bf16_lo(t.x); v[1] = bf16_hi(t.x);
        v[2] = bf16_lo(t.y); v[3] = bf16_hi(t.y);
    }
    __device__ static void unpack(const uint4 &t, float (&v)[8]) {
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = bf16_lo(w[i]);
            v[2 * i + 1] = bf16_hi(w[i]);
        }
    }
    __device__ static uint2 pack(const float (&v)[4]) { return make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])); }
    __device__ static void load(const unsigned short *p, float (&v)[4]) { unpack(*reinterpret_cast<const uint2 *>(p), v); }
    __device__ static void load(const unsigned short *p, float (&v)[8]) { unpack(*reinterpret_cast<const uint4 *>(p), v); }
    __device__ static void store(unsigned short *p, const float (&v)[4], bool plain) {
        const st_u32x2 t = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
        if (plain) store8_hint(p, t, true);
        else GRAFP_ST_NT(t, reinterpret_cast<st_u32x2 *>(p));
    }
    __device__ static void store(unsigned short *p, const float (&v)[8], bool plain) {
        const st_u32x4 t = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
        if (plain) store16_hint(p, t, true);
        else GRAFP_ST_NT(t, reinterpret_cast<st_u32x4 *>(p));
    }
    __device__ static float ld1(const unsigned short *p) { return ld_as_f32(p); }
    __device__ static void st1(unsigned short *p, float v) { *p = f32_to_bf16(v); }
};

// ---- host: the run-time store hint ----------------------------------------------------------------------------------------
// A result that fits the 256 MB Infinity Cache beside its readers' other operand is written with PLAIN stores (it stays
// cached for the launches that read it next); a larger one keeps the streaming hint, which wins there by sparing the
// producers' working set.  A pure function of the bytes written; `env` names the threshold in measurement builds.
// Same-box A/B of the whole step (tools/step_lib_ab.py, profiles/r06_c_*, r06_d_*): plain stores in the BatchNorm backward
// -1.15 % at 128 pairs, -1.05 % at 256, +0.45 % at 512, +1.2 % at 1024; in max-relative -0.5 % at 128 and 256, +0.5 % at
// 512 and 1024.  The threshold between them from tools/step_env_graph_ab.py (profiles/r06_e_bn_plain_threshold.txt,
// r06_e_mr_plain_threshold.txt; tensors up to 70 / 140 / 280 MB / all plain: 128 pairs -0.8 / -0.7 / -0.8 / -0.8 %, 256
// pairs -0.8 / -1.2 / -0.6 / -0.7 %, 512 pairs +0.2 / -0.1 / +0.8 / +1.1 %): 140 MB.
static int plain_stores(size_t bytes, const char *env, int default_mb) {
    (void)env;
    return bytes <= ((size_t)GRAFP_TUNE_INT(env, default_mb) << 20) ? 1 : 0;
}

// ---- host: the {f32, bf16} x {int32, int64} x {true, false} choices of a launcher ------------------------------------------
// f is a generic lambda that receives a tag per choice: `typename decltype(tag)::type` is the type, `decltype(tag)::value`
// the constant.  The caller has checked that dtype is GRAFP_F32 or GRAFP_BF16.
template <typename T> struct TypeTag { using type = T; };
template <typename F> static inline void for_elem(int dtype, F &&f) {
    if (dtype == GRAFP_F32) f(TypeTag<float>{});
    else f(TypeTag<unsigned short>{});
}
template <typename F> static inline void for_elem_idx(int dtype, int idx32, F &&f) {
    for_elem(dtype, [&](auto te) {
        if (idx32) f(te, TypeTag<int32_t>{});
        else f(te, TypeTag<int64_t>{});
    });
}
template <typename F> static inline void for_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace grafp
