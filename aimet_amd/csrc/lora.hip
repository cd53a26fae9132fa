// lora.hip -- the element-wise tail of a quantized PEFT LoRA layer (aimet_torch/peft.py LoraLayer:
// mul_scale and add_lora_to_res with the output quantizers around them), each in ONE launch.
//
// The reference runs every adapted linear as five wrapped children,
//   r0 = Q_base(u)   a = Q_A(a_raw)   m = Q_mul(a * s)   b = Q_B(v)   out = Q_add(r0 + b),
// which on the [T, out] tensors is three QDQ launches and an add going forward (5 reads + 4 writes
// per element) and three STE launches going back (9 passes). Here
//   aimet_lora_merge            out = Q_out(Q_u(u) + Q_v(v))          2 reads + 1 write
//   aimet_lora_merge_backward   grad_u, grad_v from grad, u, v        3 reads + 2 writes
//   aimet_lora_scale            out = Q_out(Q_a(a) * scale)           1 read  + 1 write
//   aimet_lora_scale_backward   grad_a from grad, a                   2 reads + 1 write
// with results equal, bit for bit, to the children called one by one. That fixes where a value is
// rounded to the I/O dtype T (float32: nowhere; fp16 / bf16: wherever the literal route
// materialises a tensor), written [.]_T below; all arithmetic is float32, one rounding per
// operation (-ffp-contract=off keeps the dequantize multiply and the add apart):
//   Q(x)      = [delta * (round(clamp(x, min, max) / delta - offset) + offset)]_T, the gated
//               parameters of fill_encoding_info, qdq_round_fast of common.hpp (identical to the
//               per-tensor QDQ kernels); a NULL encoding: Q(x) = x
//   merge     s = [Q_u(u) + Q_v(v)]_T          (torch's 16-bit add: float32 sum of the two rounded
//             out = Q_out(s)                    operands, rounded once)
//   scale     p = [Q_a(a) * scale]_T
//             out = Q_out(p)
//   backward  the straight-through masks of QuantizeDequantize.backward on the recomputed s or p:
//             m_out = (min_out <= s <= max_out), m_u = (min_u <= u <= max_u), ... compared with
//             the RAW encoding min / max (not the gated ones) rounded to float32 and then, for
//             16-bit I/O, to T (what quantizers._scalar_bound returns: the reference's 0-dim bound
//             takes the tensor's dtype). The launcher does that rounding from the encoding it is given.
//             merge:  g1 = [grad * m_out]_T, grad_u = [g1 * m_u]_T, grad_v = [g1 * m_v]_T
//             scale:  g1 = [grad * m_out]_T, g2 = [g1 * scale]_T, grad_a = [g2 * m_a]_T
//             one multiply by the 0/1 mask each, as aimet_ste_backward* (a masked negative gradient
//             is -0, a NaN gradient stays NaN); a NULL encoding is no multiply at all (the gradient's
//             bits pass through). grad_u or grad_v NULL: that operand needs no gradient.
//
// `scale` is a host float. The rule that makes the fused route equal the literal one: the literal
// route multiplies a tensor of dtype T by a 0-dim float32 tensor ON THE DEVICE; torch computes that
// product in T's common dtype, i.e. it casts the 0-dim operand to T before the float32 multiply. So
// for 16-bit I/O the caller passes float(T(float32(scale))) -- 16/12 becomes bf16 1.3359375 -- and
// for float32 float32(scale) (aimet_amd.peft._host_scale; tests/test_peft_gpu.py settles it with a
// scale bf16 cannot represent).
//
// Outputs may not overlap inputs or each other; the launcher refuses that (AIMET_ERR_INVALID_ARGUMENT),
// the kernels do not look. The ops run on stream_map.hpp: one 16-B vector (4 floats / 8 halves) per
// lane at a fixed 256 lanes, the scalar kernel for the tail or for a base that is not 16-B aligned.
#include "common.hpp"
#include "io16.hpp"
#include "stream_map.hpp"

#include <cmath>

namespace aimet_amd
{

QdqParams tensor_params(const aimet_tf_encoding& enc);   // qdq.hip

namespace
{

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int kLoraLanes = 256;   // fixed: aimet_qdq_tile_lanes does not apply

LaunchCounter g_launches;

// element type, vector type and the roundings of one I/O dtype
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
    static __device__ __forceinline__ float round(float f)   // [f]_T
    {
        return to_f32<IO>(from_f32<IO>(f));
    }
    // f is not NaN (io16.hpp: from_f32's MAYBE_NAN)
    static __device__ __forceinline__ elem_t store_number(float f)
    {
        return from_f32<IO, false>(f);
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
    static __device__ __forceinline__ float round(float f)
    {
        return f;
    }
    static __device__ __forceinline__ float store_number(float f)
    {
        return f;
    }
};

// one quantizer as the kernels see it (kernel arguments: SGPRs)
struct Quant
{
    int on;          // 0: a NULL encoding
    QdqParams p;     // gated (fill_encoding_info)
    float lo, hi;    // the STE bounds: the raw min / max in the I/O dtype
};

// the per-thread constants of an enabled quantizer's rounding
struct Rounder
{
    float rcp, thr;
    __device__ __forceinline__ explicit Rounder(const Quant& q) : rcp(1.0f / q.p.delta), thr(qdq_round_thr(q.p, rcp)) {}
};

// FIN: every enabled quantizer of the launch has a finite delta and offset, so a QDQ's result is
// delta * (integer + offset), never NaN, and its rounding to bf16 needs no NaN case (as in qdq16.hip)
template <int IO, bool FIN>
__device__ __forceinline__ typename Io<IO>::elem_t quant_stored(float x, const Quant& q, const Rounder& r)
{
    if (!q.on)
        return Io<IO>::store(x);
    const float o = glibc_fmaxf(glibc_fminf(x, q.p.max), q.p.min);
    const float y = dequantize(qdq_round_fast(o, q.p, r.rcp, r.thr), q.p);
    return FIN ? Io<IO>::store_number(y) : Io<IO>::store(y);
}

template <int IO, bool FIN>
__device__ __forceinline__ float quant(float x, const Quant& q, const Rounder& r)
{
    return q.on ? Io<IO>::load(quant_stored<IO, FIN>(x, q, r)) : x;
}

// g * (lo <= x <= hi) in the I/O dtype; a disabled quantizer passes g's bits on
template <int IO>
__device__ __forceinline__ typename Io<IO>::elem_t gate(typename Io<IO>::elem_t g, float x, const Quant& q)
{
    if (!q.on)
        return g;
    return Io<IO>::store(Io<IO>::load(g) * ((q.lo <= x && x <= q.hi) ? 1.0f : 0.0f));
}

template <int IO, bool FIN>
struct Merge
{
    using io           = Io<IO>;
    using T            = typename io::elem_t;
    using V            = typename io::vec_t;
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = io::width;
    const T* __restrict__ u;
    const T* __restrict__ v;
    T* __restrict__ out;
    Quant qu, qv, qo;
    __device__ __forceinline__ T one(T a, T b, const Rounder& ru, const Rounder& rv, const Rounder& ro) const
    {
        const float s = io::round(quant<IO, FIN>(io::load(a), qu, ru) + quant<IO, FIN>(io::load(b), qv, rv));
        return quant_stored<IO, FIN>(s, qo, ro);
    }
    __device__ __forceinline__ void vec(int64_t i) const
    {
        const Rounder ru(qu), rv(qv), ro(qo);
        const V a = load_stream(reinterpret_cast<const V*>(u) + i), b = load_stream(reinterpret_cast<const V*>(v) + i);
        V r;
#pragma unroll
        for (int k = 0; k < width; ++k)
            r[k] = one(a[k], b[k], ru, rv, ro);
        store_stream(r, reinterpret_cast<V*>(out) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        out[i] = one(u[i], v[i], Rounder(qu), Rounder(qv), Rounder(qo));
    }
};

template <int IO, bool FIN>
struct MergeBackward
{
    using io           = Io<IO>;
    using T            = typename io::elem_t;
    using V            = typename io::vec_t;
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = io::width;
    const T* __restrict__ u;
    const T* __restrict__ v;
    const T* __restrict__ g;
    T* __restrict__ gu;   // or null
    T* __restrict__ gv;   // or null
    Quant qu, qv, qo;
    __device__ __forceinline__ void one(T a, T b, T grad, const Rounder& ru, const Rounder& rv, T& da, T& db) const
    {
        const float x = io::load(a), y = io::load(b);
        const float s = io::round(quant<IO, FIN>(x, qu, ru) + quant<IO, FIN>(y, qv, rv));
        const T g1    = gate<IO>(grad, s, qo);
        da            = gate<IO>(g1, x, qu);
        db            = gate<IO>(g1, y, qv);
    }
    __device__ __forceinline__ void vec(int64_t i) const
    {
        const Rounder ru(qu), rv(qv);
        const V a = load_stream(reinterpret_cast<const V*>(u) + i), b = load_stream(reinterpret_cast<const V*>(v) + i),
                c = load_stream(reinterpret_cast<const V*>(g) + i);
        V ra, rb;
#pragma unroll
        for (int k = 0; k < width; ++k)
        {
            T da, db;
            one(a[k], b[k], c[k], ru, rv, da, db);
            ra[k] = da;
            rb[k] = db;
        }
        if (gu)
            store_stream(ra, reinterpret_cast<V*>(gu) + i);
        if (gv)
            store_stream(rb, reinterpret_cast<V*>(gv) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        T da, db;
        one(u[i], v[i], g[i], Rounder(qu), Rounder(qv), da, db);
        if (gu)
            gu[i] = da;
        if (gv)
            gv[i] = db;
    }
};

template <int IO, bool FIN>
struct Scale
{
    using io           = Io<IO>;
    using T            = typename io::elem_t;
    using V            = typename io::vec_t;
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = io::width;
    const T* __restrict__ a;
    T* __restrict__ out;
    float scale;
    Quant qa, qo;
    __device__ __forceinline__ T one(T x, const Rounder& ra, const Rounder& ro) const
    {
        const float p = io::round(quant<IO, FIN>(io::load(x), qa, ra) * scale);
        return quant_stored<IO, FIN>(p, qo, ro);
    }
    __device__ __forceinline__ void vec(int64_t i) const
    {
        const Rounder ra(qa), ro(qo);
        const V x = load_stream(reinterpret_cast<const V*>(a) + i);
        V r;
#pragma unroll
        for (int k = 0; k < width; ++k)
            r[k] = one(x[k], ra, ro);
        store_stream(r, reinterpret_cast<V*>(out) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        out[i] = one(a[i], Rounder(qa), Rounder(qo));
    }
};

template <int IO, bool FIN>
struct ScaleBackward
{
    using io           = Io<IO>;
    using T            = typename io::elem_t;
    using V            = typename io::vec_t;
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = io::width;
    const T* __restrict__ a;
    const T* __restrict__ g;
    T* __restrict__ ga;
    float scale;
    Quant qa, qo;
    __device__ __forceinline__ T one(T x, T grad, const Rounder& ra) const
    {
        const float xf = io::load(x);
        const float p  = io::round(quant<IO, FIN>(xf, qa, ra) * scale);
        const T g1     = gate<IO>(grad, p, qo);
        const T g2     = io::store(io::load(g1) * scale);
        return gate<IO>(g2, xf, qa);
    }
    __device__ __forceinline__ void vec(int64_t i) const
    {
        const Rounder ra(qa);
        const V x = load_stream(reinterpret_cast<const V*>(a) + i), c = load_stream(reinterpret_cast<const V*>(g) + i);
        V r;
#pragma unroll
        for (int k = 0; k < width; ++k)
            r[k] = one(x[k], c[k], ra);
        store_stream(r, reinterpret_cast<V*>(ga) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        ga[i] = one(a[i], g[i], Rounder(qa));
    }
};

// ---- host side ---------------------------------------------------------------------------------
// float32 -> the I/O dtype and back, round to nearest even: the second rounding of _scalar_bound
float round_to_io(float f, int io)
{
    if (io == IO_F32 || f != f)
        return f;
    if (io == IO_F16)
    {
        if (!std::isfinite(f) || f == 0.0f)
            return f;
        int e;
        std::frexp(f, &e);                         // |f| in [2^(e-1), 2^e): 11 significant bits,
        const int ulp = std::max(e - 11, -24);     // or the subnormal spacing 2^-24
        const float r = (float) std::ldexp(std::nearbyint(std::ldexp((double) f, -ulp)), ulp);
        return std::fabs(r) > 65504.0f ? std::copysign(HUGE_VALF, f) : r;
    }
    uint32_t b;
    std::memcpy(&b, &f, 4);
    b = (b + 0x7FFFu + ((b >> 16) & 1u)) & 0xFFFF0000u;   // an overflow rounds to inf, as it should
    std::memcpy(&f, &b, 4);
    return f;
}

Quant make_quant(const aimet_tf_encoding* enc, int io)
{
    Quant q {};
    q.p = QdqParams {0.0f, 0.0f, 1.0f, 0.0f};
    if (enc)
    {
        q.on = 1;
        q.p  = tensor_params(*enc);
        q.lo = round_to_io((float) enc->min, io);
        q.hi = round_to_io((float) enc->max, io);
    }
    return q;
}

size_t elem_size(int io)
{
    return io == IO_F32 ? 4 : 2;
}

void check_io(int io)
{
    AIMET_REQUIRE(io == IO_F32 || io == IO_F16 || io == IO_BF16,
                  "io_dtype must be 0 (float32), 1 (float16) or 2 (bfloat16)");
}

bool overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + bytes && y < x + bytes;
}

// every output apart from every input and from the other outputs
void require_separate(std::initializer_list<const void*> outs, std::initializer_list<const void*> ins, size_t bytes)
{
    for (auto o = outs.begin(); o != outs.end(); ++o)
    {
        for (const void* i : ins)
            AIMET_REQUIRE(!overlap(*o, i, bytes), "lora: an output overlaps an input");
        for (auto p = o + 1; p != outs.end(); ++p)
            AIMET_REQUIRE(!overlap(*o, *p, bytes), "lora: two outputs overlap");
    }
}

template <class... P>
bool aligned_elem(size_t esz, const P*... p)
{
    return ((reinterpret_cast<uintptr_t>(p) | ...) & (esz - 1)) == 0;
}

// f(std::integral_constant<int, IO>)
template <class F>
void with_io(int io, F&& f)
{
    switch (io)
    {
    case IO_F32: f(std::integral_constant<int, IO_F32> {}); break;
    case IO_F16: f(std::integral_constant<int, IO_F16> {}); break;
    default: f(std::integral_constant<int, IO_BF16> {}); break;
    }
}

bool finite(const Quant& q)
{
    return !q.on || (std::isfinite(q.p.delta) && std::isfinite(q.p.offset));
}

template <class T>
const T* as(const void* p)
{
    return static_cast<const T*>(p);
}
template <class T>
T* as(void* p)
{
    return static_cast<T*>(p);
}
template <class T, class A>
const A& as(const A& a)   // a quantizer or the scale
{
    return a;
}

// OpT<IO, FIN> {fields...} over n elements; pointers among the fields take the I/O dtype's element type
template <template <int, bool> class OpT, class... A>
void launch(int io, bool fin, int64_t n, bool vec, void* stream, A... fields)
{
    with_io(io, [&](auto IO) {
        constexpr int I = decltype(IO)::value;
        using T         = typename Io<I>::elem_t;
        if (fin)
            launch_stream<kLoraLanes, true>(OpT<I, true> {as<T>(fields)...}, n, vec, as_stream(stream));
        else
            launch_stream<kLoraLanes, true>(OpT<I, false> {as<T>(fields)...}, n, vec, as_stream(stream));
    });
    g_launches.add(1);
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_lora_merge(const void* u, const void* v, void* out, int64_t n, int io_dtype, const aimet_tf_encoding* enc_u,
                     const aimet_tf_encoding* enc_v, const aimet_tf_encoding* enc_out, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(n >= 0, "negative element count");
        check_io(io_dtype);
        if (n == 0)
            return;
        require_device_ptr(u, "u");
        require_device_ptr(v, "v");
        require_device_ptr(out, "out");
        const size_t esz = elem_size(io_dtype);
        AIMET_REQUIRE(aligned_elem(esz, u, v, out), "lora: misaligned pointer");
        require_separate({out}, {u, v}, (size_t) n * esz);
        const Quant qu = make_quant(enc_u, io_dtype), qv = make_quant(enc_v, io_dtype),
                    qo = make_quant(enc_out, io_dtype);
        launch<Merge>(io_dtype, finite(qu) && finite(qv) && finite(qo), n, aligned16(u, v, out), stream, u, v, out, qu,
                      qv, qo);
    });
}

int aimet_lora_merge_backward(const void* u, const void* v, const void* grad, void* grad_u, void* grad_v, int64_t n,
                              int io_dtype, const aimet_tf_encoding* enc_u, const aimet_tf_encoding* enc_v,
                              const aimet_tf_encoding* enc_out, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(n >= 0, "negative element count");
        check_io(io_dtype);
        if (n == 0 || (!grad_u && !grad_v))
            return;
        require_device_ptr(u, "u");
        require_device_ptr(v, "v");
        require_device_ptr(grad, "grad");
        if (grad_u)
            require_device_ptr(grad_u, "grad_u");
        if (grad_v)
            require_device_ptr(grad_v, "grad_v");
        const size_t esz = elem_size(io_dtype);
        AIMET_REQUIRE(aligned_elem(esz, u, v, grad, grad_u, grad_v), "lora: misaligned pointer");
        require_separate({grad_u, grad_v}, {u, v, grad}, (size_t) n * esz);
        const Quant qu = make_quant(enc_u, io_dtype), qv = make_quant(enc_v, io_dtype),
                    qo = make_quant(enc_out, io_dtype);
        launch<MergeBackward>(io_dtype, finite(qu) && finite(qv) && finite(qo), n,
                              aligned16(u, v, grad, grad_u, grad_v), stream, u, v, grad, grad_u, grad_v, qu, qv, qo);
    });
}

int aimet_lora_scale(const void* a, void* out, int64_t n, int io_dtype, float scale, const aimet_tf_encoding* enc_a,
                     const aimet_tf_encoding* enc_out, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(n >= 0, "negative element count");
        check_io(io_dtype);
        if (n == 0)
            return;
        require_device_ptr(a, "a");
        require_device_ptr(out, "out");
        const size_t esz = elem_size(io_dtype);
        AIMET_REQUIRE(aligned_elem(esz, a, out), "lora: misaligned pointer");
        require_separate({out}, {a}, (size_t) n * esz);
        const Quant qa = make_quant(enc_a, io_dtype), qo = make_quant(enc_out, io_dtype);
        launch<Scale>(io_dtype, finite(qa) && finite(qo), n, aligned16(a, out), stream, a, out, scale, qa, qo);
    });
}

int aimet_lora_scale_backward(const void* a, const void* grad, void* grad_a, int64_t n, int io_dtype, float scale,
                              const aimet_tf_encoding* enc_a, const aimet_tf_encoding* enc_out, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(n >= 0, "negative element count");
        check_io(io_dtype);
        if (n == 0)
            return;
        require_device_ptr(a, "a");
        require_device_ptr(grad, "grad");
        require_device_ptr(grad_a, "grad_a");
        const size_t esz = elem_size(io_dtype);
        AIMET_REQUIRE(aligned_elem(esz, a, grad, grad_a), "lora: misaligned pointer");
        require_separate({grad_a}, {a, grad}, (size_t) n * esz);
        const Quant qa = make_quant(enc_a, io_dtype), qo = make_quant(enc_out, io_dtype);
        launch<ScaleBackward>(io_dtype, finite(qa) && finite(qo), n, aligned16(a, grad, grad_a), stream, a, grad,
                              grad_a, scale, qa, qo);
    });
}

int aimet_lora_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
