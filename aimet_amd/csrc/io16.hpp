// io16.hpp -- fp16 / bf16 <-> fp32 element conversions of the 16-bit I/O kernels, exactly as
// torch's .to(torch.float32) (exact) and .to(torch.float16 / torch.bfloat16) (round to nearest
// even; bf16 NaN -> 0x7FC0) compute them.
#pragma once

#include <hip/hip_fp16.h>

#include <cstdint>

#include "vec_types.hpp"

namespace aimet_amd
{

enum IoType
{
    IO_F32  = 0,
    IO_F16  = 1,
    IO_BF16 = 2
};

template <int IO>
__device__ __forceinline__ float to_f32(unsigned short u)
{
    if constexpr (IO == IO_F16)
        return __half2float(__ushort_as_half(u));
    else
        return __uint_as_float((uint32_t) u << 16);
}

// MAYBE_NAN = false: the caller knows f is not NaN (a QDQ output with finite delta and offset is
// delta * (integer + offset): finite or +-inf), so the bf16 NaN canonicalisation is skipped
template <int IO, bool MAYBE_NAN = true>
__device__ __forceinline__ unsigned short from_f32(float f)
{
    // The empty asm pins f as an fp32 VGPR value: without it the backend folds
    // fptrunc(fmul(a, b)) into v_fma_mix{lo,hi}_f16(a, b, 0), which rounds the exact product
    // straight to fp16 (no fp32 rounding first: differs from torch's two-step cast near fp16
    // rounding boundaries) and adds +0 (turns a -0 result into +0).
    asm("" : "+v"(f));
    if constexpr (IO == IO_F16)
        return __half_as_ushort(__float2half_rn(f));
    else
    {
        // c10::BFloat16 round_to_nearest_even (c10/util/BFloat16.h): RNE = gfx950's
        // v_cvt_pk_bf16_f32; torch maps every NaN to 0x7FC0
        const unsigned short h = __builtin_bit_cast(unsigned short, (__bf16) f);
        if constexpr (!MAYBE_NAN)
            return h;
        return f != f ? (unsigned short) 0x7FC0 : h;
    }
}

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// One I/O dtype as a kernel sees it: element type, 16-byte vector type and its width, and the
// roundings. The values match aimet_amd/_native.py's IO_CODES.
template <int IO>
struct Io
{
    using elem_t = unsigned short;
    using vec_t  = u16x8;
    static constexpr int width = 8;
    static __device__ __forceinline__ float load(elem_t e)
    {
        return to_f32<IO>(e);
    }
    static __device__ __forceinline__ elem_t store(float f)
    {
        return from_f32<IO>(f);
    }
    // f is not NaN (from_f32's MAYBE_NAN)
    static __device__ __forceinline__ elem_t store_number(float f)
    {
        return from_f32<IO, false>(f);
    }
    static __device__ __forceinline__ float round(float f)   // [f]_T
    {
        return to_f32<IO>(from_f32<IO>(f));
    }
};
template <>
struct Io<IO_F32>
{
    using elem_t = float;
    using vec_t  = f4;
    static constexpr int width = 4;
    static __device__ __forceinline__ float load(float e)
    {
        return e;
    }
    static __device__ __forceinline__ float store(float f)
    {
        return f;
    }
    static __device__ __forceinline__ float store_number(float f)
    {
        return f;
    }
    static __device__ __forceinline__ float round(float f)
    {
        return f;
    }
};

// elements before the first 16-byte boundary at or after p (aligned to its element), at most n
template <class T>
__device__ __forceinline__ int head_of(const T* p, int n)
{
    const int h = (int) (((16u - (unsigned) (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(T));
    return h < n ? h : n;
}

}   // namespace aimet_amd
