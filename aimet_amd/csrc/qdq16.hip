// qdq16.hip -- fp16 / bf16 I/O variants of the QDQ and STE ops.
//
// Reference: a half / bfloat16 tensor is upcast (`tensor.to(torch.float32)`), quantize-dequantized
// by the fp32 kernel and cast back (`.to(orig dtype)`): v1/tensor_quantizer.py:1116-1139 and
// :1141-1168, i.e. three full passes (2+4, 4+4, 4+2 B/elem = 20 B/elem). Here the conversions
// happen in registers: 2 B in + 2 B out per element (4 B/elem), one 16-B vector of
// eight elements per lane. Results are identical to the three-pass sequence: the upcast is exact,
// the fp32 arithmetic is the same (common.hpp), and the downcast is round-to-nearest-even as
// torch's (c10::Half via the hardware cvt, c10::BFloat16 round_to_nearest_even with NaN -> 0x7FC0).
// The STE backward compares float(x) with the float32 bounds (torch type promotion) and returns
// grad * mask in the grad dtype.
// The ops run on the kernels and the launch policy of stream_map.hpp, at a fixed 256 lanes.
#include "common.hpp"
#include "io16.hpp"
#include "stream_map.hpp"

#include <cstdlib>

namespace aimet_amd
{
namespace
{

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int kLanes16 = 256;   // fixed: aimet_qdq_tile_lanes does not apply

// thr = qdq_round_thr(p, rcp) (common.hpp), hoisted by the callers out of their element loops
template <bool STOCHASTIC>
__device__ __forceinline__ float qdq(float x, const QdqParams& p, uint64_t seed, uint64_t idx, float rcp, float thr)
{
    float q;
    if constexpr (STOCHASTIC)
        q = quantize_stochastic(x, p, seed, idx);
    else
        q = qdq_round_fast(glibc_fmaxf(glibc_fminf(x, p.max), p.min), p, rcp, thr);
    return dequantize(q, p);
}

// per-tensor (CH = false, params in SGPRs) / per-channel (CH = true; vector form: K % 8 == 0 and
// n < 2^32, the 32-bit map; scalar form: int64, any K)
template <int IO, bool CH, bool STOCHASTIC>
struct Qdq16
{
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = 8;
    const unsigned short* __restrict__ in;
    unsigned short* __restrict__ out;
    QdqParams params;
    ChannelMap map;
    int64_t C, K;
    const float* __restrict__ table;
    uint64_t seed;
    __device__ __forceinline__ void vec(int64_t i) const
    {
        QdqParams p = params;
        if constexpr (CH)
            p = load_params(table, map.C, map.channel((uint32_t) (i * 8)));
        u16x8 v = load_stream(reinterpret_cast<const u16x8*>(in) + i), r;
        const uint64_t e = (uint64_t) i * 8;
        const float rcp  = 1.0f / p.delta;
        const float thr  = qdq_round_thr(p, rcp);
        if (__builtin_isfinite(p.delta) && __builtin_isfinite(p.offset))
        {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                r[k] = from_f32<IO, false>(qdq<STOCHASTIC>(to_f32<IO>(v[k]), p, seed, e + k, rcp, thr));
        }
        else
        {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                r[k] = from_f32<IO>(qdq<STOCHASTIC>(to_f32<IO>(v[k]), p, seed, e + k, rcp, thr));
        }
        store_stream(r, reinterpret_cast<u16x8*>(out) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        QdqParams q = params;
        if constexpr (CH)
            q = load_params(table, (uint32_t) C, (uint32_t) ((i / K) % C));
        const float rcp = 1.0f / q.delta;
        out[i] = from_f32<IO>(qdq<STOCHASTIC>(to_f32<IO>(in[i]), q, seed, (uint64_t) i, rcp, qdq_round_thr(q, rcp)));
    }
};

template <int IO>
__device__ __forceinline__ unsigned short ste16(unsigned short x, unsigned short g, float mn, float mx)
{
    const float xf = to_f32<IO>(x);
    return from_f32<IO>(to_f32<IO>(g) * ((mn <= xf && xf <= mx) ? 1.0f : 0.0f));
}

template <int IO, bool CH>
struct Ste16
{
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = 8;
    const unsigned short* __restrict__ x;
    const unsigned short* __restrict__ g;
    unsigned short* __restrict__ gi;
    float smin, smax;
    ChannelMap map;
    int64_t C, K;
    const float* __restrict__ mins;
    const float* __restrict__ maxs;
    __device__ __forceinline__ void vec(int64_t i) const
    {
        float mn = smin, mx = smax;
        if constexpr (CH)
        {
            const uint32_t c = map.channel((uint32_t) (i * 8));
            mn               = mins[c];
            mx               = maxs[c];
        }
        u16x8 a = load_stream(reinterpret_cast<const u16x8*>(x) + i),
              b = load_stream(reinterpret_cast<const u16x8*>(g) + i), r;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            r[k] = ste16<IO>(a[k], b[k], mn, mx);
        store_stream(r, reinterpret_cast<u16x8*>(gi) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        float mn = smin, mx = smax;
        if constexpr (CH)
        {
            const int64_t c = (i / K) % C;
            mn              = mins[c];
            mx              = maxs[c];
        }
        gi[i] = ste16<IO>(x[i], g[i], mn, mx);
    }
};

// vector part plus scalar tail (per-tensor), or everything scalar (K % 8 != 0)
template <bool CH>
bool vec_ok16(bool aligned, int64_t n, int64_t K)
{
    return aligned && (!CH || (K % 8 == 0 && n < (int64_t(1) << 32)));
}

template <int IO, bool CH, bool STO>
void launch_qdq16(const void* in, void* out, int64_t n, const QdqParams& p, int64_t C, int64_t K, const float* table,
                  uint64_t seed, hipStream_t s)
{
    Qdq16<IO, CH, STO> op {static_cast<const unsigned short*>(in), static_cast<unsigned short*>(out), p,
                           ChannelMap(C, K), C, K, table, seed};
    launch_stream<kLanes16, true>(op, n, vec_ok16<CH>(aligned16(in, out), n, K), s);
}

template <int IO, bool CH>
void launch_ste16(const void* x, const void* g, void* gi, int64_t n, float mn, float mx, int64_t C, int64_t K,
                  const float* mins, const float* maxs, hipStream_t s)
{
    Ste16<IO, CH> op {static_cast<const unsigned short*>(x), static_cast<const unsigned short*>(g),
                      static_cast<unsigned short*>(gi), mn, mx, ChannelMap(C, K), C, K, mins, maxs};
    launch_stream<kLanes16, true>(op, n, vec_ok16<CH>(aligned16(x, g, gi), n, K), s);
}

template <bool CH>
void dispatch_qdq16(int io, bool sto, const void* in, void* out, int64_t n, const QdqParams& p, int64_t C, int64_t K,
                    const float* table, uint64_t seed, hipStream_t s)
{
    if (io == IO_F16)
        sto ? launch_qdq16<IO_F16, CH, true>(in, out, n, p, C, K, table, seed, s)
            : launch_qdq16<IO_F16, CH, false>(in, out, n, p, C, K, table, seed, s);
    else
        sto ? launch_qdq16<IO_BF16, CH, true>(in, out, n, p, C, K, table, seed, s)
            : launch_qdq16<IO_BF16, CH, false>(in, out, n, p, C, K, table, seed, s);
}

void check_io(int io)
{
    AIMET_REQUIRE(io == IO_F16 || io == IO_BF16, "io_dtype must be 1 (float16) or 2 (bfloat16)");
}

void check_round_mode(int round_mode)
{
    AIMET_REQUIRE(round_mode == AIMET_ROUND_NEAREST || round_mode == AIMET_ROUND_STOCHASTIC, "Unknown rounding mode.");
}

}   // namespace

QdqParams tensor_params(const aimet_tf_encoding& enc);   // qdq.hip

}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_qdq_per_tensor_16(const void* in, void* out, int64_t n, int io_dtype, const aimet_tf_encoding* enc,
                            int round_mode, uint64_t seed, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(enc != nullptr, "encoding is null");
        AIMET_REQUIRE(n >= 0, "negative element count");
        check_io(io_dtype);
        check_round_mode(round_mode);
        if (n == 0)
            return;
        require_device_ptr(in, "input");
        require_device_ptr(out, "output");
        dispatch_qdq16<false>(io_dtype, round_mode == AIMET_ROUND_STOCHASTIC, in, out, n, tensor_params(*enc), 1, 1,
                              nullptr, seed, as_stream(stream));
    });
}

int aimet_qdq_per_channel_16(const void* in, void* out, int64_t outer, int64_t C, int64_t K, int io_dtype,
                             const float* table, int round_mode, uint64_t seed, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(outer >= 0 && C > 0 && K >= 0, "invalid per-channel shape");
        check_io(io_dtype);
        check_round_mode(round_mode);
        const int64_t n = outer * C * K;
        if (n == 0)
            return;
        require_device_ptr(in, "input");
        require_device_ptr(out, "output");
        require_device_ptr(table, "table");
        dispatch_qdq16<true>(io_dtype, round_mode == AIMET_ROUND_STOCHASTIC, in, out, n, QdqParams {}, C, K, table,
                             seed, as_stream(stream));
    });
}

int aimet_ste_backward_16(const void* x, const void* grad, void* grad_in, int64_t outer, int64_t C, int64_t K,
                          int io_dtype, const float* mins, const float* maxs, float enc_min, float enc_max,
                          void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(outer >= 0 && C > 0 && K >= 0, "invalid shape");
        check_io(io_dtype);
        const int64_t n = outer * C * K;
        if (n == 0)
            return;
        require_device_ptr(x, "x");
        require_device_ptr(grad, "grad");
        require_device_ptr(grad_in, "grad_in");
        const bool ch = mins != nullptr;
        if (ch)
        {
            require_device_ptr(mins, "mins");
            require_device_ptr(maxs, "maxs");
        }
        hipStream_t s = as_stream(stream);
        if (io_dtype == IO_F16)
            ch ? launch_ste16<IO_F16, true>(x, grad, grad_in, n, 0, 0, C, K, mins, maxs, s)
               : launch_ste16<IO_F16, false>(x, grad, grad_in, n, enc_min, enc_max, 1, 1, nullptr, nullptr, s);
        else
            ch ? launch_ste16<IO_BF16, true>(x, grad, grad_in, n, 0, 0, C, K, mins, maxs, s)
               : launch_ste16<IO_BF16, false>(x, grad, grad_in, n, enc_min, enc_max, 1, 1, nullptr, nullptr, s);
    });
}

}   // extern "C"
