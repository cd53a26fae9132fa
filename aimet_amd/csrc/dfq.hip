// dfq.hip -- data-free quantization on the device: batch-norm fold, cross-layer scaling (CLS) and
// high-bias fold (HBF), in place on fp32 parameters (aimet_common/batch_norm_fold.py:71-97,
// aimet_common/cross_layer_equalization.py:600-729; the reference runs them in numpy on the host,
// one layer at a time, every parameter copied device -> host -> device).
//
// Every kernel gives one workgroup to one channel. In CLS channel c owns row c of the first weight
// and column c of the next and nothing else touches them, so the workgroup reduces its ranges,
// computes its scale and rescales its data without any hand-off: one launch per set, the second
// read served by the cache. The reductions are LDS trees of a fixed shape: no atomics, equal inputs
// give equal bits. Arithmetic: each product, quotient and root rounded on its own in fp32
// (-ffp-contract=off, correctly rounded divide and sqrt), denormals kept, as numpy on the host.
#include <cmath>
#include <vector>

#include "common.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kDfqBlock = 256;

LaunchCounter g_launches;

// One channel's elements: nseg segments of len floats, segment j at base + j * stride.
struct Span
{
    float* base;
    int64_t nseg, len, stride;
};

// A weight seen from one side: channel c's span starts at data + c * chan_stride.
struct Side
{
    float* data;
    int64_t chan_stride, nseg, len, stride;

    __device__ __forceinline__ Span channel(int64_t c) const
    {
        return Span {data + c * chan_stride, nseg, len, stride};
    }
};

// np.max semantics: a NaN stays
__device__ __forceinline__ float nan_max(float m, float v)
{
    return (v > m || v != v) ? v : m;
}

// f(x) for every element of the span, the workgroup's lanes striding over it; WRITE stores x back.
// A one-segment span goes in 16-byte accesses between a scalar head and tail.
template <bool WRITE, class F>
__device__ __forceinline__ void span_apply(const Span& sp, F&& f)
{
    const int t = threadIdx.x;
    if (sp.nseg == 1)
    {
        float* p        = sp.base;
        const int64_t n = sp.len;
        int64_t head    = (int64_t) (((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
        if (head > n)
            head = n;
        for (int64_t i = t; i < head; i += kDfqBlock)
        {
            float x = p[i];
            f(x);
            if (WRITE)
                p[i] = x;
        }
        float4* v        = reinterpret_cast<float4*>(p + head);
        const int64_t nv = (n - head) >> 2;
        for (int64_t i = t; i < nv; i += kDfqBlock)
        {
            float4 x = v[i];
            f(x.x);
            f(x.y);
            f(x.z);
            f(x.w);
            if (WRITE)
                v[i] = x;
        }
        for (int64_t i = head + nv * 4 + t; i < n; i += kDfqBlock)
        {
            float x = p[i];
            f(x);
            if (WRITE)
                p[i] = x;
        }
    }
    else
    {
        const int64_t n = sp.nseg * sp.len;
        for (int64_t e = t; e < n; e += kDfqBlock)
        {
            const int64_t j = sp.len == 1 ? e : e / sp.len;
            float* q        = sp.base + j * sp.stride + (e - j * sp.len);
            float x         = *q;
            f(x);
            if (WRITE)
                *q = x;
        }
    }
}

// Fixed-shape tree over the workgroup's 256 partials; every lane gets the result.
template <class Op>
__device__ __forceinline__ float block_reduce(float v, float* lds, Op op)
{
    const int t = threadIdx.x;
    lds[t]      = v;
    __syncthreads();
    for (int s = kDfqBlock / 2; s > 0; s >>= 1)
    {
        if (t < s)
            lds[t] = op(lds[t], lds[t + s]);
        __syncthreads();
    }
    const float r = lds[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float span_absmax(const Span& sp, float* lds)
{
    float m = 0.0f;
    span_apply<false>(sp, [&](float& x) { m = nan_max(m, __builtin_fabsf(x)); });
    return block_reduce(m, lds, [](float a, float b) { return nan_max(a, b); });
}

__device__ __forceinline__ void span_scale(const Span& sp, float s)
{
    span_apply<true>(sp, [&](float& x) { x = x * s; });
}

// np.nan_to_num(s, nan=1, posinf=1), then s[s == 0] = 1
__device__ __forceinline__ float sanitize_scale(float s)
{
    if (s != s || s == __builtin_inff())
        s = 1.0f;
    return s == 0.0f ? 1.0f : s;
}

__global__ __launch_bounds__(kDfqBlock) void dfq_cls_pair_kernel(Side a, float* bias0, Side b, float* scale_out)
{
    __shared__ float lds[kDfqBlock];
    const int64_t c = blockIdx.x;
    const Span s0 = a.channel(c), s1 = b.channel(c);
    const float r0  = span_absmax(s0, lds);
    const float r1  = span_absmax(s1, lds);
    const float s   = sanitize_scale(r0 / __builtin_sqrtf(r0 * r1));
    const float rcp = 1.0f / s;
    span_scale(s0, rcp);
    span_scale(s1, s);
    if (threadIdx.x == 0)
    {
        scale_out[c] = s;
        if (bias0)
            bias0[c] = bias0[c] * rcp;
    }
}

__global__ __launch_bounds__(kDfqBlock) void dfq_cls_triple_kernel(Side a, float* bias0, Side b, float* bias1, Side d,
                                                                   float* s12_out, float* s23_out)
{
    __shared__ float lds[kDfqBlock];
    const int64_t c = blockIdx.x;
    const Span s0 = a.channel(c), s1 = b.channel(c), s2 = d.channel(c);
    const float r0    = span_absmax(s0, lds);
    const float r1    = span_absmax(s1, lds);
    const float r2    = span_absmax(s2, lds);
    const float p     = (r0 * r1) * r2;
    const float root  = (float) cbrt((double) p);
    const float s12   = sanitize_scale(r0 / root);
    const float s23   = sanitize_scale(root / r2);
    const float rcp12 = 1.0f / s12, rcp23 = 1.0f / s23;
    span_scale(s0, rcp12);
    span_apply<true>(s1, [&](float& x) { x = x * s12 * rcp23; });
    span_scale(s2, s23);
    if (threadIdx.x == 0)
    {
        s12_out[c] = s12;
        s23_out[c] = s23;
        if (bias0)
            bias0[c] = bias0[c] * rcp12;
        if (bias1)
            bias1[c] = bias1[c] * rcp23;
    }
}

struct BnJob
{
    Side w;   // backward: the spans of the output channels; forward: data only
    float* bias;
    const float *gamma, *beta, *mean, *var;
    float eps;
    int32_t forward;
    int64_t cout, cin, k;
};

// conv -> bn for output channel o, `scale` what was folded in; false, with the status word set and
// nothing touched, when sqrt(var + eps) is zero
__device__ __forceinline__ bool bn_fold_backward(const BnJob& j, int64_t o, int32_t* status, float& scale)
{
    const float sigma = __builtin_sqrtf(j.var[o] + j.eps);
    if (sigma == 0.0f)
    {
        if (threadIdx.x == 0)
            status[blockIdx.y] = 1;
        return false;
    }
    scale = j.gamma[o] / sigma;
    span_scale(j.w.channel(o), scale);
    if (threadIdx.x == 0)
        j.bias[o] = j.beta[o] - (j.mean[o] - j.bias[o]) * scale;
    return true;
}

// A backward fold that also moves the output channel's learned quantization range onto the scaled
// weight: (min, max) * c, the ends swapped for a negative c.
struct BnScaleJob
{
    BnJob fold;
    float *enc_min, *enc_max;
};

__global__ __launch_bounds__(kDfqBlock) void dfq_bn_fold_scale_kernel(const BnScaleJob* jobs, int32_t* status)
{
    const BnScaleJob j = jobs[blockIdx.y];
    const int64_t o    = blockIdx.x;
    if (o >= j.fold.cout)
        return;
    float c;
    if (bn_fold_backward(j.fold, o, status, c) && threadIdx.x == 0)
    {
        const float lo = j.enc_min[o] * c, hi = j.enc_max[o] * c;
        j.enc_min[o]   = c >= 0.0f ? lo : hi;
        j.enc_max[o]   = c >= 0.0f ? hi : lo;
    }
}

__global__ __launch_bounds__(kDfqBlock) void dfq_bn_fold_kernel(const BnJob* jobs, int32_t* status)
{
    __shared__ float lds[kDfqBlock];
    const BnJob j   = jobs[blockIdx.y];
    const int64_t o = blockIdx.x;
    if (o >= j.cout)
        return;
    if (!j.forward)
    {
        float scale;
        bn_fold_backward(j, o, status, scale);
        return;
    }
    // bn -> conv: row o of a [cout][cin][k] weight; a lane owns the input channels i = t, t + 256, ...
    float* row     = j.w.data + o * j.cin * j.k;
    float sum_beta = 0.0f, sum_mu = 0.0f;
    bool bad       = false;
    for (int64_t i = threadIdx.x; i < j.cin; i += kDfqBlock)
    {
        const float sigma = __builtin_sqrtf(j.var[i] + j.eps);
        if (sigma == 0.0f)
        {
            bad = true;
            continue;
        }
        const float scale = j.gamma[i] / sigma;
        float* seg        = row + i * j.k;
        float w2d         = 0.0f;
        for (int64_t q = 0; q < j.k; ++q)
            w2d = w2d + seg[q];
        sum_beta = sum_beta + w2d * j.beta[i];
        sum_mu   = sum_mu + w2d * (j.mean[i] * scale);
        for (int64_t q = 0; q < j.k; ++q)
            seg[q] = seg[q] * scale;
    }
    if (bad)
        status[blockIdx.y] = 1;
    auto add      = [](float x, float y) { return x + y; };
    sum_beta      = block_reduce(sum_beta, lds, add);
    sum_mu        = block_reduce(sum_mu, lds, add);
    if (threadIdx.x == 0)
        j.bias[o] = (sum_beta - sum_mu) + j.bias[o];
}

__device__ __forceinline__ float hbf_absorb(const float* gamma, const float* beta, const float* scale, int relu,
                                            int64_t c)
{
    const float bq = beta[c] / scale[c];
    if (!relu)
        return bq;
    const float gq = gamma[c] / scale[c];
    const float v  = bq - 3.0f * __builtin_fabsf(gq);
    return (0.0f > v || v != v) ? (v != v ? v : 0.0f) : v;   // np.maximum(0, v): a NaN stays
}

// One workgroup per output channel o of the second layer. bias1 is rewritten from beta, gamma and
// scale alone (absorb never reads a bias), so no workgroup waits for another.
__global__ __launch_bounds__(kDfqBlock) void dfq_bias_fold_kernel(const float* gamma, const float* beta,
                                                                  const float* scale, int64_t C, int relu,
                                                                  float* bias1, const float* w2, int64_t cin,
                                                                  int64_t k, int64_t out_stride, int64_t in_stride,
                                                                  float* bias2)
{
    __shared__ float lds[kDfqBlock];
    const int64_t o = blockIdx.x;
    for (int64_t c = o * kDfqBlock + threadIdx.x; c < C; c += (int64_t) gridDim.x * kDfqBlock)
        bias1[c] = bias1[c] - hbf_absorb(gamma, beta, scale, relu, c);
    if (cin == 1)
    {
        if (threadIdx.x == 0)
        {
            const float* seg = w2 + o * out_stride;
            float w2d        = 0.0f;
            for (int64_t q = 0; q < k; ++q)
                w2d = w2d + seg[q];
            bias2[o] = bias2[o] + w2d * hbf_absorb(gamma, beta, scale, relu, o);
        }
        return;
    }
    float acc = 0.0f;
    for (int64_t c = threadIdx.x; c < cin; c += kDfqBlock)
    {
        const float* seg = w2 + o * out_stride + c * in_stride;
        float w2d        = 0.0f;
        for (int64_t q = 0; q < k; ++q)
            w2d = w2d + seg[q];
        acc = acc + w2d * hbf_absorb(gamma, beta, scale, relu, c);
    }
    acc = block_reduce(acc, lds, [](float x, float y) { return x + y; });
    if (threadIdx.x == 0)
        bias2[o] = bias2[o] + acc;
}

// ---- host side -------------------------------------------------------------------------------------
bool conv_layout(const aimet_dfq_weight& w)
{
    return w.out_stride == w.cin * w.k && w.in_stride == w.k;
}
bool transposed_layout(const aimet_dfq_weight& w)
{
    return w.out_stride == w.k && w.in_stride == w.cout * w.k;
}

void check_weight(const aimet_dfq_weight* w, const char* what)
{
    AIMET_REQUIRE(w != nullptr, std::string(what) + " is null");
    AIMET_REQUIRE(w->cout > 0 && w->cin > 0 && w->k > 0, std::string(what) + ": cout, cin and k must be positive");
    AIMET_REQUIRE(w->cout < (int64_t(1) << 31) && w->cin < (int64_t(1) << 31) && w->k < (int64_t(1) << 31) &&
                      w->cout * w->cin < (int64_t(1) << 40) / w->k,
                  std::string(what) + ": too large");
    AIMET_REQUIRE(conv_layout(*w) || transposed_layout(*w),
                  std::string(what) + ": strides must be (cin*k, k) or, for a transposed weight, (k, cout*k)");
    require_device_ptr(w->data, what);
}

// the elements of output channel o / of input channel i, contiguous runs merged
Side out_side(const aimet_dfq_weight& w)
{
    if (w.in_stride == w.k)
        return Side {w.data, w.out_stride, 1, w.cin * w.k, w.cin * w.k};
    return Side {w.data, w.out_stride, w.cin, w.k, w.in_stride};
}
Side in_side(const aimet_dfq_weight& w)
{
    if (w.out_stride == w.k)
        return Side {w.data, w.in_stride, 1, w.cout * w.k, w.cout * w.k};
    return Side {w.data, w.in_stride, w.cout, w.k, w.out_stride};
}

BnJob checked_bn_job(const aimet_dfq_bn_fold_job& j)
{
    check_weight(&j.w, "BN fold weight");
    AIMET_REQUIRE(!j.forward || conv_layout(j.w), "BN fold: forward fold needs a Conv / Linear layout");
    require_device_ptr(j.bias, "BN fold bias");
    require_device_ptr(j.gamma, "BN gamma");
    require_device_ptr(j.beta, "BN beta");
    require_device_ptr(j.mean, "BN running mean");
    require_device_ptr(j.var, "BN running var");
    return BnJob {out_side(j.w), j.bias, j.gamma, j.beta, j.mean, j.var, j.eps, j.forward ? 1 : 0,
                  j.w.cout,      j.w.cin, j.w.k};
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_dfq_bn_fold(const aimet_dfq_bn_fold_job* jobs, int64_t count, int32_t* status_dev, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(count >= 0 && count <= 65535, "BN fold: 0..65535 jobs per launch");
        if (count == 0)
            return;
        AIMET_REQUIRE(jobs != nullptr, "BN fold: job table is null");
        require_device_ptr(status_dev, "status");
        std::vector<BnJob> table((size_t) count);
        int64_t max_cout = 0;
        for (int64_t n = 0; n < count; ++n)
        {
            const aimet_dfq_bn_fold_job& j = jobs[n];
            for (int64_t m = 0; m < n; ++m)
                AIMET_REQUIRE(jobs[m].w.data != j.w.data, "BN fold: two jobs of one launch on the same weight");
            table[(size_t) n] = checked_bn_job(j);
            max_cout          = std::max(max_cout, j.w.cout);
        }
        hipStream_t s = as_stream(stream);
        auto dev      = Scratch<BnJob>::upload(table, s);
        dfq_bn_fold_kernel<<<dim3((unsigned) max_cout, (unsigned) count), kDfqBlock, 0, s>>>(dev.get(), status_dev);
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_bnre_fold_scale(const aimet_bnre_fold_scale_job* jobs, int64_t count, int32_t* status_dev, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(count >= 0 && count <= 65535, "BN fold to scale: 0..65535 jobs per launch");
        if (count == 0)
            return;
        AIMET_REQUIRE(jobs != nullptr, "BN fold to scale: job table is null");
        require_device_ptr(status_dev, "status");
        std::vector<BnScaleJob> table((size_t) count);
        int64_t max_cout = 0;
        for (int64_t n = 0; n < count; ++n)
        {
            const aimet_bnre_fold_scale_job& j = jobs[n];
            AIMET_REQUIRE(!j.fold.forward, "BN fold to scale: only a BatchNorm behind the layer folds to scale");
            require_device_ptr(j.enc_min, "BN fold to scale encoding min");
            require_device_ptr(j.enc_max, "BN fold to scale encoding max");
            for (int64_t m = 0; m < n; ++m)
                AIMET_REQUIRE(jobs[m].fold.w.data != j.fold.w.data && jobs[m].enc_min != j.enc_min &&
                                  jobs[m].enc_max != j.enc_max,
                              "BN fold to scale: two jobs of one launch on the same weight or range");
            table[(size_t) n] = BnScaleJob {checked_bn_job(j.fold), j.enc_min, j.enc_max};
            max_cout          = std::max(max_cout, j.fold.w.cout);
        }
        hipStream_t s = as_stream(stream);
        auto dev      = Scratch<BnScaleJob>::upload(table, s);
        dfq_bn_fold_scale_kernel<<<dim3((unsigned) max_cout, (unsigned) count), kDfqBlock, 0, s>>>(dev.get(),
                                                                                                    status_dev);
        AIMET_LAUNCH_CHECK();
        bnre_count_launches(1);
    });
}

int aimet_dfq_cls_pair(const aimet_dfq_weight* w0, float* bias0, const aimet_dfq_weight* w1, float* scale_dev,
                       void* stream)
{
    return guarded([&] {
        check_weight(w0, "CLS first weight");
        check_weight(w1, "CLS second weight");
        AIMET_REQUIRE(w0->cout == w1->cin, "CLS pair: the second weight needs as many input channels as the first has "
                                           "output channels");
        AIMET_REQUIRE(w0->data != w1->data, "CLS pair: the two weights are the same tensor");
        if (bias0)
            require_device_ptr(bias0, "CLS first bias");
        require_device_ptr(scale_dev, "CLS scale");
        dfq_cls_pair_kernel<<<(unsigned) w0->cout, kDfqBlock, 0, as_stream(stream)>>>(out_side(*w0), bias0,
                                                                                     in_side(*w1), scale_dev);
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_dfq_cls_triple(const aimet_dfq_weight* w0, float* bias0, const aimet_dfq_weight* w1, float* bias1,
                         const aimet_dfq_weight* w2, float* s12_dev, float* s23_dev, void* stream)
{
    return guarded([&] {
        check_weight(w0, "CLS first weight");
        check_weight(w1, "CLS depthwise weight");
        check_weight(w2, "CLS third weight");
        AIMET_REQUIRE(w1->cin == 1 && conv_layout(*w1), "CLS triple: the middle weight must be depthwise (C x 1 x k)");
        AIMET_REQUIRE(w0->cout == w1->cout && w1->cout == w2->cin, "CLS triple: channel counts differ");
        AIMET_REQUIRE(w0->data != w1->data && w1->data != w2->data && w0->data != w2->data,
                      "CLS triple: two weights are the same tensor");
        if (bias0)
            require_device_ptr(bias0, "CLS first bias");
        if (bias1)
            require_device_ptr(bias1, "CLS depthwise bias");
        require_device_ptr(s12_dev, "CLS scale 12");
        require_device_ptr(s23_dev, "CLS scale 23");
        dfq_cls_triple_kernel<<<(unsigned) w0->cout, kDfqBlock, 0, as_stream(stream)>>>(
            out_side(*w0), bias0, out_side(*w1), bias1, in_side(*w2), s12_dev, s23_dev);
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_dfq_bias_fold(const float* gamma, const float* beta, const float* scale, int64_t C, int relu_between,
                        float* bias1, const aimet_dfq_weight* w2, float* bias2, void* stream)
{
    return guarded([&] {
        check_weight(w2, "HBF second weight");
        AIMET_REQUIRE(C > 0 && C < (int64_t(1) << 31), "HBF: invalid channel count");
        AIMET_REQUIRE(w2->cin == 1 ? w2->cout == C : w2->cin == C,
                      "HBF: the second weight does not have C input channels (or, depthwise, C output channels)");
        require_device_ptr(gamma, "HBF gamma");
        require_device_ptr(beta, "HBF beta");
        require_device_ptr(scale, "HBF scale");
        require_device_ptr(bias1, "HBF first bias");
        require_device_ptr(bias2, "HBF second bias");
        dfq_bias_fold_kernel<<<(unsigned) w2->cout, kDfqBlock, 0, as_stream(stream)>>>(
            gamma, beta, scale, C, relu_between ? 1 : 0, bias1, w2->data, w2->cin, w2->k, w2->out_stride,
            w2->in_stride, bias2);
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_dfq_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
