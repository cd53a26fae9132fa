// rnn_math.hpp -- the sigmoid and tanh of the fused recurrent step (rnn_cell.hip), written out in
// float32 operations so that they can be restated operation for operation elsewhere
// (tests/rnn_oracle.py in numpy float32; tools/studies/rnn_math_host.cpp compiles this header for
// the host). Every operation below is one IEEE float32 add, subtract, multiply, divide, floor,
// compare or integer step, in the order the parentheses give: the library is built with
// -ffp-contract=off and the correctly rounded divide, and nothing here calls a math library.
//
//  * exp_r: Cephes expf. x clamped to [-87, 88.5] (results stay normal and finite);
//    n = floor(x * log2(e) + 0.5); r = (x - n * C1) - n * C2 with ln 2 = C1 + C2 in two parts;
//    e^r = ((P(r) * r^2) + r) + 1 with a degree-5 P; the scale 2^n as two exact power-of-two factors.
//  * sigmoid_r(x) = 1 / (1 + exp_r(-x)).
//  * tanh_r: below |x| = 0.625 the odd Cephes polynomial x + x * z * Q(z), z = x^2; above,
//    1 - 2 / (exp_r(2 |x|) + 1) with the sign of x (|x| clamped to 44, where the result is 1).
// Measured against torch's CPU functions over every float32 input: profiles/r16/rnn_math_sweep.txt.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define AIMET_RNN_HD __host__ __device__ __forceinline__
#else
#define AIMET_RNN_HD inline
#endif

namespace aimet_amd
{
namespace rnn_math
{

// 2^n for -126 <= n <= 127, from its bits
AIMET_RNN_HD float pow2i(int n)
{
    const uint32_t bits = (uint32_t) (n + 127) << 23;
    float f;
    __builtin_memcpy(&f, &bits, sizeof f);
    return f;
}

AIMET_RNN_HD float exp_r(float x)
{
    x             = x < -87.0f ? -87.0f : x;   // a NaN passes both clamps and comes out a NaN
    x             = x > 88.5f ? 88.5f : x;
    const float z = __builtin_floorf((1.44269504088896341f * x) + 0.5f);
    x             = x - (z * 0.693359375f);
    x             = x - (z * -2.12194440e-4f);
    const int n   = z == z ? (int) z : 0;      // -126 .. 128
    const float x2 = x * x;
    float p       = (1.9875691500e-4f * x) + 1.3981999507e-3f;
    p             = (p * x) + 8.3334519073e-3f;
    p             = (p * x) + 4.1665795894e-2f;
    p             = (p * x) + 1.6666665459e-1f;
    p             = (p * x) + 5.0000001201e-1f;
    const float r = ((p * x2) + x) + 1.0f;
    const int a   = n >> 1;                    // floor(n / 2): both factors within [2^-63, 2^64]
    return (r * pow2i(a)) * pow2i(n - a);
}

AIMET_RNN_HD float sigmoid_r(float x)
{
    return 1.0f / (1.0f + exp_r(-x));
}

AIMET_RNN_HD float tanh_r(float x)
{
    float a = __builtin_fabsf(x);
    if (a < 0.625f)
    {
        const float z = x * x;
        float q       = (-5.70498872745e-3f * z) + 2.06390887954e-2f;
        q             = (q * z) - 5.37397155531e-2f;
        q             = (q * z) + 1.33314422036e-1f;
        q             = (q * z) - 3.33332819422e-1f;
        return ((q * z) * x) + x;
    }
    a             = a > 44.0f ? 44.0f : a;
    const float t = 1.0f - (2.0f / (exp_r(a + a) + 1.0f));
    return x < 0.0f ? -t : t;
}

}   // namespace rnn_math
}   // namespace aimet_amd
