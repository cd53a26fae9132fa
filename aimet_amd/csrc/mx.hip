// mx.hip -- OCP Microscaling (MX) fake-quantization for gfx950: MXFP8 (E4M3, E5M2), MXFP6 (E3M2,
// E2M3) and MXFP4 (E2M1). A block of 32 values along one axis shares a power-of-two scale (E8M0)
// that is computed from the data at every call; there is nothing to calibrate. Written in torch ops
// this is about a dozen element-wise and reduction launches per tensor; here it is one.
//
// The arithmetic contract. Formats (M mantissa bits, element exponents emin..emax, subnormals, no
// Inf / NaN element is ever produced):
//     E4M3  M 3  emin  -6  emax  8  max normal 448        E3M2  M 2  emin -2  emax 4  max normal 28
//     E5M2  M 2  emin -14  emax 15  max normal 57344      E2M3  M 3  emin  0  emax 2  max normal 7.5
//                                                         E2M1  M 1  emin  0  emax 2  max normal 6
// A block v_0..v_31 (fp16 / bf16 converted to float32, exact):
//   * any v_i NaN or +-Inf: all 32 outputs NaN, scale byte 0xFF;
//   * a = max|v_i|; a == 0: s = -127 (every output zero); else s = clamp(floor(log2 a) - emax, -127, 127),
//     a float32 denormal a counting with its true exponent (so s = -127); X = 2^s, scale byte s + 127;
//   * y_i = v_i / X (exact wherever it matters: what float32 underflow can touch is below half the
//     smallest element subnormal 2^(emin - M) and becomes 0 either way; input denormals are not flushed);
//   * E = max(floor(log2|y_i|), emin), step = 2^(E - M), p_i = RNE(y_i / step) * step (a carry into
//     the next binade is fine), then p_i = sign * min(|p_i|, max normal): saturating;
//   * out_i = p_i * X, exact in float32 (denormal results included); fp16 / bf16 I/O rounds it once
//     with io16.hpp's RNE store.
// Every step is exact, so the kernels equal a float64 restatement bit for bit. The gradient is the
// straight-through identity (no kernel).
//
// How it is computed: the block maximum is taken on the sign-cleared bit patterns as integers (an
// all-ones exponent field is then the NaN / Inf test, and the exponent field is floor(log2 a)). s is in
// [-127, 125] (emax >= 2), so 2^-s is always a normal float32 and y = v * 2^-s is one multiply. The
// grid rounding builds 2^(M - E) and 2^(E - M) from y's exponent field (as fp8.hip does), rint is the
// only rounding. 2^s itself is a denormal for s = -127, so out = (p * 2^(s >> 1)) * 2^(s - (s >> 1)):
// two normal factors, the first product exact. Plain float and integer operations; gfx950's
// scaled-convert instructions are not used.
//
// MI355X design. A tensor is [outer][K][inner], the block along K, K % 32 == 0. Streaming, HBM-bound
// (fp32 8 B/element, 16-bit 4 B/element), no LDS, 64-bit offsets, grid-stride, in place allowed (a
// lane reads all it owns before it writes).
//   * row form (inner == 1): the tensor is a flat run of blocks. A lane owns 8 consecutive elements
//     (two 16-B loads for fp32, one for 16-bit), 4 adjacent lanes are a block; the block maximum
//     crosses the 4 lanes in two DPP quad_perm steps (reduce.hpp: quad_all); 8 values are quantized in
//     registers and stored with the width they were loaded with. A base that is not 16-B aligned
//     (a sliced view) takes the same lane map with element accesses.
//   * column form (inner > 1): lanes run along the flattened (outer K/32, inner) index, so neighbouring
//     lanes touch neighbouring addresses; a lane walks its block's 32 k at stride `inner` into 32
//     registers, takes the maximum and quantizes with no cross-lane traffic, and writes back at the same
//     stride. inner = 9 (a 3x3 kernel) and inner = H W run the same kernel: only how much of a wave
//     falls in one (outer, block) differs.
//   * quantize / dequantize (row form): the same lane map and block body; a lane's 8 codes of w bits
//     are w bytes of the block's little-endian bit string (element i at bits [w i, w i + w): FP4 element
//     0 is the low nibble, 8 FP6 codes are exactly 6 bytes), lane 0 of a block stores the scale byte.
//     A code is sign, exponent, mantissa in the OCP encodings. A NaN block stores 0xFF and zero codes.
#include "common.hpp"
#include "io16.hpp"
#include "reduce.hpp"
#include "stream_map.hpp"

namespace aimet_amd
{

namespace
{

LaunchCounter g_launches;

struct MxFormat
{
    int M, emin, emax, w;
    uint32_t eb_min;   // exponent field of 2^emin, in place
    uint32_t down;     // bits of 2^(M - E) are down - (exponent field of 2^E, in place)
    uint32_t up;       // bits of 2^(E - M) are (exponent field of 2^E, in place) - up
    uint32_t rebias;   // (exponent field of 2^(emin - 1)), in place: float bits <-> element code
    float maxn;        // max normal
};

MxFormat mx_format(int format)
{
    static const int tab[5][4]   = {{3, -6, 8, 8}, {2, -14, 15, 8}, {2, -2, 4, 6}, {3, 0, 2, 6}, {1, 0, 2, 4}};
    static const float maxn[5]   = {448.0f, 57344.0f, 28.0f, 7.5f, 6.0f};
    AIMET_REQUIRE(format >= 0 && format < 5, "MX format must be 0 (E4M3), 1 (E5M2), 2 (E3M2), 3 (E2M3) or 4 (E2M1)");
    const int* t = tab[format];
    MxFormat f;
    f.M = t[0], f.emin = t[1], f.emax = t[2], f.w = t[3];
    f.eb_min = (uint32_t) (f.emin + 127) << 23;
    f.down   = (uint32_t) (254 + f.M) << 23;
    f.up     = (uint32_t) f.M << 23;
    f.rebias = (uint32_t) (f.emin + 126) << 23;
    f.maxn   = maxn[format];
    return f;
}

constexpr uint32_t kAbsMask = 0x7fffffffu;
constexpr uint32_t kExpMask = 0x7f800000u;

__device__ __forceinline__ float pow2(int e)   // -126 <= e <= 127
{
    return __uint_as_float((uint32_t) (e + 127) << 23);
}

// A block's scale as the kernels use it: 2^-s and the two halves of 2^s.
struct MxScale
{
    float inv, x1, x2;
    bool nan;
};

// From the scale byte s + 127. The encoder's s is in [-127, 125]; a stored byte may say 126 or 127,
// where 2^-s is no normal float, but only the halves of 2^s are used to decode.
__device__ __forceinline__ MxScale mx_scale(int byte)
{
    const int s = byte - 127, s1 = s >> 1;
    return MxScale {__uint_as_float((uint32_t) (254 - byte) << 23), pow2(s1), pow2(s - s1), byte == 0xFF};
}

// s + 127 from max|v_i| as bits; 0xFF for a block with a NaN or an Inf. A zero or denormal maximum has
// exponent field 0 and clamps to s = -127 like every a < 2^(emax - 127).
__device__ __forceinline__ int mx_scale_byte(uint32_t amax_bits, const MxFormat& f)
{
    if (amax_bits >= kExpMask)
        return 0xFF;
    const int s = (int) (amax_bits >> 23) - 127 - f.emax;
    return (s < -127 ? -127 : s) + 127;
}

// p: v / X on the element grid, signed and saturated
__device__ __forceinline__ float mx_grid(float v, const MxScale& sc, const MxFormat& f)
{
    const float ay = __builtin_fabsf(v * sc.inv);
    uint32_t eb    = __float_as_uint(ay) & kExpMask;
    eb             = eb < f.eb_min ? f.eb_min : eb;
    const float r  = __builtin_rintf(ay * __uint_as_float(f.down - eb));
    float g        = r * __uint_as_float(eb - f.up);
    g              = g > f.maxn ? f.maxn : g;
    return __builtin_copysignf(g, v);
}

__device__ __forceinline__ float mx_out(float p, const MxScale& sc)
{
    return (p * sc.x1) * sc.x2;
}

// the OCP code of a grid value: sign, exponent (bias 1 - emin), mantissa
__device__ __forceinline__ uint32_t mx_encode(float p, const MxFormat& f)
{
    const uint32_t bits = __float_as_uint(p), gb = bits & kAbsMask;
    const uint32_t mag  = gb < f.eb_min ? (uint32_t) (__uint_as_float(gb) * __uint_as_float(f.down - f.eb_min))
                                        : (gb - f.rebias) >> (23 - f.M);
    return (bits >> 31) << (f.w - 1) | mag;
}

// and back. The encoder never emits E4M3's NaN or E5M2's Inf / NaN codes; they decode as numbers.
__device__ __forceinline__ float mx_decode(uint32_t code, const MxFormat& f)
{
    const uint32_t mag = code & ((1u << (f.w - 1)) - 1u);
    const float g      = mag < (1u << f.M) ? (float) mag * __uint_as_float(f.eb_min - f.up)
                                           : __uint_as_float((mag << (23 - f.M)) + f.rebias);
    return (code >> (f.w - 1)) & 1u ? -g : g;
}

__device__ __forceinline__ float quiet_nan()
{
    return __uint_as_float(0x7fc00000u);
}

// ---- a lane's 8 consecutive elements -------------------------------------------------------------
template <int IO, bool VEC>
__device__ __forceinline__ void load8(const typename Io<IO>::elem_t* p, float (&v)[8])
{
    if constexpr (!VEC)
    {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = Io<IO>::load(p[k]);
    }
    else if constexpr (IO == IO_F32)
    {
        const f4 a = load_stream(reinterpret_cast<const f4*>(p)), b = load_stream(reinterpret_cast<const f4*>(p) + 1);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    }
    else
    {
        const u16x8 a = load_stream(reinterpret_cast<const u16x8*>(p));
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = Io<IO>::load(a[k]);
    }
}

template <int IO, bool VEC>
__device__ __forceinline__ void store8(typename Io<IO>::elem_t* p, const float (&v)[8])
{
    if constexpr (!VEC)
    {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            p[k] = Io<IO>::store(v[k]);
    }
    else if constexpr (IO == IO_F32)
    {
        store_stream(f4 {v[0], v[1], v[2], v[3]}, reinterpret_cast<f4*>(p));
        store_stream(f4 {v[4], v[5], v[6], v[7]}, reinterpret_cast<f4*>(p) + 1);
    }
    else
    {
        u16x8 a;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            a[k] = Io<IO>::store(v[k]);
        store_stream(a, reinterpret_cast<u16x8*>(p));
    }
}

// the scale byte of the block the lane's 8 values belong to (4 adjacent lanes, all of them active)
__device__ __forceinline__ int row_scale_byte(const float (&v)[8], const MxFormat& f)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
    {
        const uint32_t b = __float_as_uint(v[k]) & kAbsMask;
        m                = b > m ? b : m;
    }
    m = quad_all(m, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
    return mx_scale_byte(m, f);
}

// Lane slot i owns elements [8 i, 8 i + 8); n8 = elements / 8 is a multiple of 4 and the grid's
// stride a multiple of 256, so the 4 lanes of a block enter and leave the loop together.
#define MX_ROW_LOOP(i, n8)                                                                                \
    for (int64_t i = (int64_t) blockIdx.x * kBlock + threadIdx.x, stride_ = (int64_t) gridDim.x * kBlock; \
         i < (n8); i += stride_)

template <int IO, bool VEC>
__global__ __launch_bounds__(kBlock) void mx_row_qdq_kernel(const typename Io<IO>::elem_t* in,
                                                            typename Io<IO>::elem_t* out, int64_t n8, MxFormat f)
{
    MX_ROW_LOOP(i, n8)
    {
        float v[8];
        load8<IO, VEC>(in + i * 8, v);
        const MxScale sc = mx_scale(row_scale_byte(v, f));
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = sc.nan ? quiet_nan() : mx_out(mx_grid(v[k], sc, f), sc);
        store8<IO, VEC>(out + i * 8, v);
    }
}

// codes must be 8-byte aligned: a lane's w bytes start at a multiple of w
template <int IO, bool VEC>
__global__ __launch_bounds__(kBlock) void mx_row_pack_kernel(const typename Io<IO>::elem_t* in,
                                                             uint8_t* __restrict__ scales,
                                                             uint8_t* __restrict__ codes, int64_t n8, MxFormat f)
{
    MX_ROW_LOOP(i, n8)
    {
        float v[8];
        load8<IO, VEC>(in + i * 8, v);
        const int byte   = row_scale_byte(v, f);
        const MxScale sc = mx_scale(byte);
        uint64_t word    = 0;
        if (!sc.nan)
        {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                word |= (uint64_t) mx_encode(mx_grid(v[k], sc, f), f) << (f.w * k);
        }
        uint8_t* dst = codes + i * f.w;
        if (f.w == 8)
            *reinterpret_cast<uint2*>(dst) = uint2 {(uint32_t) word, (uint32_t) (word >> 32)};
        else if (f.w == 6)
        {
            uint16_t* d = reinterpret_cast<uint16_t*>(dst);
            d[0] = (uint16_t) word, d[1] = (uint16_t) (word >> 16), d[2] = (uint16_t) (word >> 32);
        }
        else
            *reinterpret_cast<uint32_t*>(dst) = (uint32_t) word;
        if ((i & 3) == 0)
            scales[i >> 2] = (uint8_t) byte;
    }
}

template <int IO, bool VEC>
__global__ __launch_bounds__(kBlock) void mx_row_unpack_kernel(const uint8_t* __restrict__ scales,
                                                               const uint8_t* __restrict__ codes,
                                                               typename Io<IO>::elem_t* __restrict__ out, int64_t n8,
                                                               MxFormat f)
{
    MX_ROW_LOOP(i, n8)
    {
        const uint8_t* src = codes + i * f.w;
        uint64_t word;
        if (f.w == 8)
        {
            const uint2 u = *reinterpret_cast<const uint2*>(src);
            word          = (uint64_t) u.y << 32 | u.x;
        }
        else if (f.w == 6)
        {
            const uint16_t* s = reinterpret_cast<const uint16_t*>(src);
            word              = (uint64_t) s[2] << 32 | (uint64_t) s[1] << 16 | s[0];
        }
        else
            word = *reinterpret_cast<const uint32_t*>(src);
        const MxScale sc    = mx_scale(scales[i >> 2]);
        const uint32_t mask = (1u << f.w) - 1u;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = sc.nan ? quiet_nan() : mx_out(mx_decode((uint32_t) (word >> (f.w * k)) & mask, f), sc);
        store8<IO, VEC>(out + i * 8, v);
    }
}

// Lane slot j = (outer block ob, inner index ii): elements (ob * 32 + k) * inner + ii, k = 0..31.
template <int IO>
__global__ __launch_bounds__(kBlock) void mx_col_qdq_kernel(const typename Io<IO>::elem_t* in,
                                                            typename Io<IO>::elem_t* out, int64_t slots, int64_t inner,
                                                            MxFormat f)
{
    const int64_t stride = (int64_t) gridDim.x * kBlock;
    for (int64_t j = (int64_t) blockIdx.x * kBlock + threadIdx.x; j < slots; j += stride)
    {
        const int64_t ob   = j / inner;
        const int64_t base = ob * 32 * inner + (j - ob * inner);
        float v[32];
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k)
        {
            v[k]             = Io<IO>::load(in[base + k * inner]);
            const uint32_t b = __float_as_uint(v[k]) & kAbsMask;
            m                = b > m ? b : m;
        }
        const MxScale sc = mx_scale(mx_scale_byte(m, f));
#pragma unroll
        for (int k = 0; k < 32; ++k)
            out[base + k * inner] = Io<IO>::store(sc.nan ? quiet_nan() : mx_out(mx_grid(v[k], sc, f), sc));
    }
}

// ---- host side ---------------------------------------------------------------------------------
size_t check_io(int io)
{
    AIMET_REQUIRE(io == IO_F32 || io == IO_F16 || io == IO_BF16,
                  "io_dtype must be 0 (float32), 1 (float16) or 2 (bfloat16)");
    return io == IO_F32 ? 4 : 2;
}

void check_shape(int64_t outer, int64_t K, int64_t inner)
{
    AIMET_REQUIRE(outer > 0 && K > 0 && inner > 0, "MX: outer, K and inner must be positive");
    AIMET_REQUIRE(K % 32 == 0, "MX: the block axis must be a multiple of 32");
    AIMET_REQUIRE(K < (int64_t(1) << 40) && inner < (int64_t(1) << 40) / K &&
                      outer < (int64_t(1) << 40) / (K * inner),
                  "MX: tensor too large (outer K inner must stay below 2^40)");
}

void check_tensor(const void* p, size_t esize, const char* what)
{
    require_device_ptr(p, what);
    AIMET_REQUIRE((reinterpret_cast<uintptr_t>(p) & (esize - 1)) == 0, "MX: misaligned pointer");
}

// f(Io tag, vector tag) for the runtime dtype and alignment
template <class F>
void with_io(int io, bool vec, F&& f)
{
    auto with_vec = [&](auto tag) {
        if (vec)
            f(tag, std::true_type {});
        else
            f(tag, std::false_type {});
    };
    if (io == IO_F32)
        with_vec(std::integral_constant<int, IO_F32> {});
    else if (io == IO_F16)
        with_vec(std::integral_constant<int, IO_F16> {});
    else
        with_vec(std::integral_constant<int, IO_BF16> {});
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_mx_qdq(const void* in, void* out, int64_t outer, int64_t K, int64_t inner, int io_dtype, int format,
                 void* stream)
{
    return guarded([&] {
        const MxFormat f   = mx_format(format);
        const size_t esize = check_io(io_dtype);
        check_shape(outer, K, inner);
        check_tensor(in, esize, "input");
        check_tensor(out, esize, "output");
        const int64_t n     = outer * K * inner;
        const char *i0 = static_cast<const char*>(in), *o0 = static_cast<const char*>(out);
        AIMET_REQUIRE(o0 == i0 || o0 + n * (int64_t) esize <= i0 || i0 + n * (int64_t) esize <= o0,
                      "MX: the output must be the input or not overlap it");
        hipStream_t s = as_stream(stream);
        if (inner == 1)
            with_io(io_dtype, aligned16(in, out), [&](auto io, auto vec) {
                using E = typename Io<decltype(io)::value>::elem_t;
                mx_row_qdq_kernel<decltype(io)::value, decltype(vec)::value>
                    <<<stream_blocks(n / 8, kBlock), kBlock, 0, s>>>(static_cast<const E*>(in), static_cast<E*>(out),
                                                                     n / 8, f);
            });
        else
            with_io(io_dtype, false, [&](auto io, auto) {
                using E = typename Io<decltype(io)::value>::elem_t;
                mx_col_qdq_kernel<decltype(io)::value><<<stream_blocks(n / 32, kBlock), kBlock, 0, s>>>(
                    static_cast<const E*>(in), static_cast<E*>(out), n / 32, inner, f);
            });
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_mx_quantize(const void* in, uint8_t* scales, uint8_t* codes, int64_t rows, int64_t K, int io_dtype,
                      int format, void* stream)
{
    return guarded([&] {
        const MxFormat f   = mx_format(format);
        const size_t esize = check_io(io_dtype);
        check_shape(rows, K, 1);
        check_tensor(in, esize, "input");
        check_tensor(scales, 1, "scales");
        check_tensor(codes, 8, "codes");
        const int64_t n = rows * K;
        with_io(io_dtype, aligned16(in), [&](auto io, auto vec) {
            using E = typename Io<decltype(io)::value>::elem_t;
            mx_row_pack_kernel<decltype(io)::value, decltype(vec)::value>
                <<<stream_blocks(n / 8, kBlock), kBlock, 0, as_stream(stream)>>>(static_cast<const E*>(in), scales,
                                                                                 codes, n / 8, f);
        });
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_mx_dequantize(const uint8_t* scales, const uint8_t* codes, void* out, int64_t rows, int64_t K, int io_dtype,
                        int format, void* stream)
{
    return guarded([&] {
        const MxFormat f   = mx_format(format);
        const size_t esize = check_io(io_dtype);
        check_shape(rows, K, 1);
        check_tensor(scales, 1, "scales");
        check_tensor(codes, 8, "codes");
        check_tensor(out, esize, "output");
        const int64_t n = rows * K;
        with_io(io_dtype, aligned16(out), [&](auto io, auto vec) {
            using E = typename Io<decltype(io)::value>::elem_t;
            mx_row_unpack_kernel<decltype(io)::value, decltype(vec)::value>
                <<<stream_blocks(n / 8, kBlock), kBlock, 0, as_stream(stream)>>>(scales, codes, static_cast<E*>(out),
                                                                                 n / 8, f);
        });
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_mx_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
