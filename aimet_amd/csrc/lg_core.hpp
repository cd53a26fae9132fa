// lg_core.hpp -- the learned-grid (range-learning) element arithmetic, written once for every
// kernel that quantize-dequantizes on a trainable range (learned_grid.hip, lg_block.hip): the
// encoding of a range (LgEnc::of, enc_of), the Markstein quotient (lg_recip, lg_quot), the forward's
// element (lg_qdq*) with its fused 16-bit store (lg_store4), the backward's element and its sums
// (lg_bwd_term*, lg_bwd_elems*, load_grad4) and the range gradients of one set of sums
// (range_grads_one). Reference: quantsim_straight_through_grad.py:121-328.
//
// Everything sits in an unnamed namespace, as it did inside learned_grid.hip: the kernels of that
// file take LgEnc and LgRange by value, so their symbols -- and their machine code -- are what they
// were before these lines moved here.
#pragma once

#include <cmath>

#include "common.hpp"
#include "io16.hpp"
#include "stream_map.hpp"

namespace aimet_amd
{
namespace
{

// The quotient x / d without the IEEE division's ~10 instructions. y = lg_recip(d) = RN(1/d) is
// computed once per encoding; then q0 = RN(x * y) is a faithful quotient, r = x - d * q0 is exact
// (fma), and RN(q0 + r * y) is the correctly rounded quotient (Markstein's theorem) while nothing
// under- or overflows: |d| in [2^-40, 2^40] (else y = NaN and the kernels divide) and |q| in
// [2^-60, 2^60), so |x| and r stay far from the subnormal range. Bit-identical to x / d there:
// tools/studies/markstein_div_check.c (754 M operand pairs, quotients at half-integers +-3 ulp and
// all-ones mantissas included; the same bounds fail only for |x| < 2^-100). Outside that range the
// consumers below need less than the exact quotient (lg_rint_quot, lg_quot), so no element takes
// a slow path: 3 VALU plus one compare per element (the 16-bit kernels are VALU co-bound).
__device__ __forceinline__ float lg_recip(float d)
{
    const float a = __builtin_fabsf(d);
    return (a >= 0x1p-40f && a <= 0x1p40f) ? 1.0f / d : __builtin_nanf("");
}

// torch's NaN: the op chain passes a NaN input through (quieted)
__device__ __forceinline__ float quiet_nan(float x)
{
    return __uint_as_float(__float_as_uint(x) | 0x00400000u);
}

// torch's clamp(v, lo, hi) = minimum(maximum(v, lo), hi): a NaN passes through (gfx950's
// v_maximum3 / v_minimum3, IEEE 754-2019). It differs from torch only in the sign of a zero
// (maximum(-0, +0) = +0), which every use below adds an offset to, where -0 + o == +0 + o.
__device__ __forceinline__ float t_clamp(float v, float lo, float hi)
{
    return __builtin_elementwise_minimum(__builtin_elementwise_maximum(v, lo), hi);
}

// the reference's forward with the division: encodings that lg_recip refuses (or a non-finite
// offset)
__device__ __forceinline__ float lg_qdq_div(float x, float d, float o, float steps)
{
    return (t_clamp(__builtin_rintf(x / d) - o, 0.0f, steps) + o) * d;
}

__device__ __forceinline__ bool lg_fast_enc(float o, float rd)
{
    return rd == rd && __builtin_fabsf(o) <= 0x1p32f;
}

// The forward's element for an encoding lg_fast_enc accepts, never NaN: x is first clamped to
// +-2^59 |d| (med3), inside which |x * y| < 2^60 and the Markstein quotient needs no range test;
// a clamped x gives rint(q) ~ +-2^59, beyond every clamp bound on the same side as the division's
// (+-inf included). A NaN x is the caller's to map (torch's clamp passes it through).
__device__ __forceinline__ float lg_qdq_fast(float x, float d, float o, float steps, float rd, float xmax)
{
    const float xc = __builtin_amdgcn_fmed3f(x, -xmax, xmax);
    const float q0 = xc * rd;
    const float q  = __builtin_fmaf(__builtin_fmaf(-q0, d, xc), rd, q0);
    return (__builtin_amdgcn_fmed3f(__builtin_rintf(q) - o, 0.0f, steps) + o) * d;
}

// x_round = round(x / delta) - offset ; x_quant = clamp(x_round, 0, steps) ; y = (x_quant + offset) * delta
// (rd = lg_recip(d)); a NaN x gives NaN as torch's clamp does
__device__ __forceinline__ float lg_qdq(float x, float d, float o, float steps, float rd)
{
    if (!lg_fast_enc(o, rd))
        return lg_qdq_div(x, d, o, steps);
    const float y = lg_qdq_fast(x, d, o, steps, rd, 0x1p59f * __builtin_fabsf(d));
    return x != x ? quiet_nan(x) : y;
}
template <int N>
__device__ __forceinline__ void lg_qdq_n(const float* x, float d, float o, float steps, float rd, float* y)
{
    if (!lg_fast_enc(o, rd))
    {
#pragma unroll
        for (int k = 0; k < N; ++k)
            y[k] = lg_qdq_div(x[k], d, o, steps);
        return;
    }
    const float xmax = 0x1p59f * __builtin_fabsf(d);
#pragma unroll
    for (int k = 0; k < N; ++k)
    {
        const float v = lg_qdq_fast(x[k], d, o, steps, rd, xmax);
        y[k]          = x[k] != x[k] ? quiet_nan(x[k]) : v;
    }
}

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// torch's maximum / minimum: a NaN operand is returned
__device__ __forceinline__ float t_maximum(float a, float b)
{
    return a != a ? a : (b != b ? b : fmaxf(a, b));
}
__device__ __forceinline__ float t_minimum(float a, float b)
{
    return a != a ? a : (b != b ? b : fminf(a, b));
}

// get_computed_encodings (quantsim_straight_through_grad.py:121-160) of channel c, element by
// element as the reference's torch ops on the C-vectors: computed in the forward kernel itself
// when `emin` is set (the thread holding the first element of a channel's first row stores
// them for the backward), else read from precomputed delta / offset
struct LgEnc
{
    const float* emin;
    const float* emax;
    float* delta_out;
    float* offset_out;
    float* range_out;   // optional [2][C]: the range as the forward read it (saved for the backward)
    float steps, half_floor, neg_half_ceil;
    int mode;        // 0 symmetric signed, 1 symmetric unsigned, 2 asymmetric
    uint32_t K;      // elements per row (the store condition)
    uint32_t C;
    __device__ __forceinline__ void of(float mn, float mx, float& d, float& o) const
    {
        if (mode == 0)
        {
            d = mx / half_floor;
            o = neg_half_ceil;
        }
        else
        {
            d = (mx - mn) / steps;
            if (mode == 1)
                o = mn / d;
            else
                o = -t_minimum(steps, t_maximum(0.0f, __builtin_rintf(-mn / d)));
        }
    }
    // delta / offset of channel c for element e (flat index): from the range or the tables
    __device__ __forceinline__ void get(uint32_t c, uint32_t e, const float* delta, const float* offset, float& d,
                                        float& o) const
    {
        if (emin == nullptr)
        {
            d = delta[c];
            o = offset[c];
            return;
        }
        const float mn = emin[c], mx = emax[c];
        of(mn, mx, d, o);
        if (e == c * K)
        {
            delta_out[c]  = d;
            offset_out[c] = o;
            if (range_out)
            {
                range_out[c]     = mn;
                range_out[C + c] = mx;
            }
        }
    }
};

// OUT = IO_F32: y float32. OUT = IO_F16 / IO_BF16: y written in 16 bits with torch's rounding --
// the float32 result cast as autocast casts a weight for its matmul, fused into the store.
template <int OUT>
__device__ __forceinline__ void lg_store4(void* __restrict__ y, uint32_t q, f4 r)
{
    if constexpr (OUT == IO_F32)
        store_stream(r, static_cast<f4*>(y) + q);
    else
    {
        const u16x4 h = {from_f32<OUT>(r.x), from_f32<OUT>(r.y), from_f32<OUT>(r.z), from_f32<OUT>(r.w)};
        store_stream(h, static_cast<u16x4*>(y) + q);
    }
}

// four gradient elements of quad i: float32, or 16-bit upcast (exact)
template <int GIO>
__device__ __forceinline__ f4 load_grad4(const void* __restrict__ g, uint32_t i)
{
    if constexpr (GIO == IO_F32)
        return load_stream(static_cast<const f4*>(g) + i);
    else
    {
        const u16x4 h = load_stream(static_cast<const u16x4*>(g) + i);
        return f4 {to_f32<GIO>(h.x), to_f32<GIO>(h.y), to_f32<GIO>(h.z), to_f32<GIO>(h.w)};
    }
}

struct Sums
{
    float a, b, d;
};

// One element of the backward (calculate_forward_pass + the gradient expressions of
// QuantizeDequantizeFunc.backward / asymmetric_gradients / symmetric_gradients), with
// q = RN(x / dl) (lg_quot, rcp = lg_recip(dl)), the reference's x / delta:
//   m = mask (0 / 1) ; grad_x = m * grad ;
//   MODE 1 (symmetric_gradients): A += (x_quant + offset) * grad ; B += (m * (x / delta)) * grad
//     (the reference's two sums, :311-314);
//   MODE 2 (asymmetric_gradients): A += (x_quant + offset - (x * m) / delta) * grad, the
//     reference's one grad_scale sum (:283-286, B stays 0), and D += grad where !m (grad_offset
//     without its delta factor, applied to the sum);
//   MODE 0 (no range gradients requested): A, B as MODE 1 and D as MODE 2.
// Where !m, (x * m) / delta is 0 * x (NaN for a non-finite x) and m * (x / delta) is 0 * (x /
// delta) (NaN also when the quotient overflows), as the reference evaluates them. mask is
// x_quant == x_round with x_quant = med3(x_round, 0, steps) (one compare instead of two; false
// for a NaN round); a NaN x makes the sums NaN through those 0 * NaN terms, as the reference's,
// so x_quant need not pass the NaN through. Every kernel forms the same values.
template <int MODE>
__device__ __forceinline__ void lg_bwd_term_m(float x, float q, float g, float o, float steps, float& gx, Sums& s)
{
    const float xr = __builtin_rintf(q) - o;
    const float xq = __builtin_amdgcn_fmed3f(xr, 0.0f, steps);
    const bool in  = xq == xr;
    const float m  = in ? 1.0f : 0.0f;
    gx = m * g;
    if constexpr (MODE == 2)
    {
        s.a += ((xq + o) - m * (in ? q : x)) * g;
        s.d += in ? 0.0f : g;
    }
    else
    {
        s.a += (xq + o) * g;
        s.b += (m * q) * g;
        if constexpr (MODE == 0)
            s.d += in ? 0.0f : g;
    }
}
__device__ __forceinline__ void lg_bwd_term(float x, float q, float g, float o, float steps, int mode, float& gx,
                                            Sums& s)
{
    if (mode == 2)
        lg_bwd_term_m<2>(x, q, g, o, steps, gx, s);
    else if (mode == 1)
        lg_bwd_term_m<1>(x, q, g, o, steps, gx, s);
    else
        lg_bwd_term_m<0>(x, q, g, o, steps, gx, s);
}

// RN(x / d) for the backward from y = lg_recip(d) (not NaN), no branch: the Markstein quotient
// while |q0| < 2^60 -- RN(x / d) itself except for |x| < 2^-100, where it is off by a few ulps of
// a quotient below 2^-59 -- else q0 = RN(x * y) (infinite exactly when x is, or when x / d is
// within an ulp of overflowing). rint(q) and the mask are therefore the division's (grad_x is
// bit-exact); B's terms can differ only in those two corners, at the encoding gradients' tolerance.
__device__ __forceinline__ float lg_quot(float x, float d, float y)
{
    const float q0 = x * y;
    const float q  = __builtin_fmaf(__builtin_fmaf(-q0, d, x), y, q0);
    return __builtin_fabsf(q0) < 0x1p60f ? q : q0;
}

__device__ __forceinline__ void lg_bwd_elem(float x, float g, float dl, float o, float steps, float rcp, float& gx,
                                            Sums& s, int mode)
{
    lg_bwd_term(x, lg_fast_enc(o, rcp) ? lg_quot(x, dl, rcp) : x / dl, g, o, steps, mode, gx, s);
}

// lg_bwd_elem over N elements in order (the same sums)
template <int N>
__device__ __forceinline__ void lg_bwd_elems(const float* x, const float* g, float dl, float o, float steps,
                                             float rcp, float* gx, Sums& s, int mode)
{
    float q[N];
    if (lg_fast_enc(o, rcp))
    {
#pragma unroll
        for (int k = 0; k < N; ++k)
            q[k] = lg_quot(x[k], dl, rcp);
    }
    else
    {
#pragma unroll
        for (int k = 0; k < N; ++k)
            q[k] = x[k] / dl;
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
        lg_bwd_term(x[k], q[k], g[k], o, steps, mode, gx[k], s);
}

// lg_bwd_elems for an encoding lg_fast_enc accepts: no division code in the caller's vector path
// (its registers are then the streaming loads' and the sums', not the division's temporaries)
template <int N, int MODE>
__device__ __forceinline__ void lg_bwd_elems_fast(const float* x, const float* g, float dl, float o, float steps,
                                                  float rcp, float* gx, Sums& s)
{
#pragma unroll
    for (int k = 0; k < N; ++k)
        lg_bwd_term_m<MODE>(x[k], lg_quot(x[k], dl, rcp), g[k], o, steps, gx[k], s);
}

// the encoding gradients of channel c from its sums {A, B, D} (asymmetric / symmetric_gradients,
// the reference's torch expressions element by element); gmin == nullptr: not requested
struct LgRange
{
    const float* emin;
    const float* emax;
    const float* delta;
    float* gmin;
    float* gmax;
    float steps, half_floor;
    int sym;
};

__device__ __forceinline__ void range_grads_one(float A, float B, float D, uint32_t c, const LgRange& r)
{
    const float gss = A - B;
    if (r.sym)
    {
        const float g = gss / r.half_floor;
        r.gmax[c]     = g;
        r.gmin[c]     = -g;
        return;
    }
    const float mn = r.emin[c], mx = r.emax[c];
    const float term1 = gss / r.steps;
    const float w     = mx - mn;
    const float term2 = (r.steps / (w * w)) * (r.delta[c] * D);
    r.gmin[c]         = -term1 + mx * term2;
    r.gmax[c]         = term1 - mn * term2;
}

// (bw, sym, strict, unsign) as a grid: the one place that turns the quantizer's flags into LgEnc's
// steps, mode and constants; validates the range and table pointers
LgEnc enc_of(const float* emin, const float* emax, int64_t C, int64_t K, int bw, int sym, int strict, int unsign,
             float* delta, float* offset, float* range_out)
{
    AIMET_REQUIRE(bw > 0 && bw < 32, "invalid bitwidth");
    require_device_ptr(emin, "encoding_min");
    require_device_ptr(emax, "encoding_max");
    require_device_ptr(delta, "delta");
    require_device_ptr(offset, "offset");
    double steps = std::ldexp(1.0, bw) - 1;
    if (sym && strict)
        steps -= 1;
    const double half = steps / 2;
    if (range_out)
        require_device_ptr(range_out, "range_out");
    return LgEnc {emin, emax, delta, offset, range_out, (float) steps, (float) std::floor(half),
                  (float) -std::ceil(half), (sym && !unsign) ? 0 : (sym ? 1 : 2), (uint32_t) K, (uint32_t) C};
}

}   // namespace
}   // namespace aimet_amd
