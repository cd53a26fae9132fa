// quant_analyzer.hip -- the reduction behind QuantAnalyzer's per-layer MSE (aimet_torch/v1/quant_analyzer.py
// export_per_layer_mse_loss; the reference takes torch's fp32 mse_loss of two partial forwards per layer
// and batch and reads every value back with .item()).
//
//  * aimet_qa_sq_err: acc[0] += scale * sum (ref_i - x_i)^2, acc[1] += scale * sum ref_i^2 over two
//    tensors of one dtype (fp32, fp16, bf16). Every element is widened to double before the
//    subtraction; squares and sums are double, so neither 1e30-scale activations nor long sums leave
//    the format. One HBM read of each tensor, nothing else: 16-byte loads on both inputs between a
//    scalar head and tail when the two bases are equally misaligned to 16 bytes, element loads on
//    both otherwise (a view at an odd offset; layer outputs from the allocator are aligned).
//    A workgroup leaves two doubles; a second, one-workgroup launch folds them (a lane its run of
//    consecutive partials in index order, then a fixed tree), multiplies by scale once and adds into
//    acc. No atomics: the order of every addition is fixed by n, the dtype and the two base
//    alignments, so two runs on the same pointers give the same bits.
//
//  * aimet_amp_sqnr_add: acc[0] += (sum ref_i^2 / n) / (sum (ref_i - x_i)^2 / n + eps), the per-batch
//    ratio of mixed precision's SQNR callback (aimet_torch/amp/mixed_precision_algo.py _compute_sqnr;
//    the reference clones, subtracts, squares twice, takes two means and reads the ratio back). The
//    same first launch; its fold also takes the two means, the ratio and the add, so a batch costs
//    one read of each tensor and an evaluation one read-back.

#include <limits>

#include "common.hpp"
#include "io16.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kQaBlock          = 256;
constexpr int64_t kQaVecPerLane = 2;   // 16-byte loads per input a lane has before the grid grows no further
constexpr int64_t kQaMaxElems   = int64_t(1) << 40;

LaunchCounter g_launches;       // aimet_qa_sq_err
LaunchCounter g_amp_launches;   // aimet_amp_sqnr_add

// Fixed-shape tree over the workgroup's 256 pairs; every lane returns with lds[0], lds[kQaBlock] the sums.
__device__ __forceinline__ void block_sum2(double a, double b, double* lds)
{
    const int t       = threadIdx.x;
    lds[t]            = a;
    lds[kQaBlock + t] = b;
    __syncthreads();
    for (int s = kQaBlock / 2; s > 0; s >>= 1)
    {
        if (t < s)
        {
            lds[t]            = lds[t] + lds[t + s];
            lds[kQaBlock + t] = lds[kQaBlock + t] + lds[kQaBlock + t + s];
        }
        __syncthreads();
    }
}

template <int IO>
struct Elem
{
    using type = unsigned short;
};
template <>
struct Elem<IO_F32>
{
    using type = float;
};

template <int IO>
__device__ __forceinline__ double widen(typename Elem<IO>::type v)
{
    if constexpr (IO == IO_F32)
        return (double) v;
    else
        return (double) to_f32<IO>(v);
}

// one element: d += (r - x)^2, q += r^2, one rounding per accumulation
__device__ __forceinline__ void add_pair(double r, double x, double& d, double& q)
{
    const double e = r - x;
    d              = __builtin_fma(e, e, d);
    q              = __builtin_fma(r, r, q);
}

template <int IO>
__device__ __forceinline__ void add_vec(const uint4 r, const uint4 x, double (&d)[4], double (&q)[4])
{
    const uint32_t rw[4] = {r.x, r.y, r.z, r.w}, xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        if constexpr (IO == IO_F32)
            add_pair((double) __uint_as_float(rw[k]), (double) __uint_as_float(xw[k]), d[k], q[k]);
        else
        {
            add_pair(widen<IO>((unsigned short) (rw[k] & 0xFFFFu)), widen<IO>((unsigned short) (xw[k] & 0xFFFFu)), d[k],
                     q[k]);
            add_pair(widen<IO>((unsigned short) (rw[k] >> 16)), widen<IO>((unsigned short) (xw[k] >> 16)), d[k], q[k]);
        }
    }
}

// ref and x equally misaligned: `head` elements up to the 16-byte boundary, nv 16-byte vectors, the
// rest (fewer than a vector). Workgroup b takes vectors b * 256 + t, then strides by the grid;
// workgroup 0 also takes head and tail.
template <int IO>
__global__ __launch_bounds__(kQaBlock) void qa_sq_err_vec_kernel(const typename Elem<IO>::type* __restrict__ ref,
                                                                 const typename Elem<IO>::type* __restrict__ x, int64_t n,
                                                                 int64_t head, int64_t nv, double* __restrict__ part)
{
    constexpr int EPV = 16 / (int) sizeof(typename Elem<IO>::type);
    __shared__ double lds[2 * kQaBlock];
    const int t = threadIdx.x;
    double d[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    const uint4* rv      = reinterpret_cast<const uint4*>(ref + head);
    const uint4* xv      = reinterpret_cast<const uint4*>(x + head);
    const int64_t stride = (int64_t) gridDim.x * kQaBlock;
#pragma unroll 4
    for (int64_t i = (int64_t) blockIdx.x * kQaBlock + t; i < nv; i += stride)
        add_vec<IO>(rv[i], xv[i], d, q);
    if (blockIdx.x == 0)
    {
        if (t < head)
            add_pair(widen<IO>(ref[t]), widen<IO>(x[t]), d[0], q[0]);
        const int64_t rest = head + nv * EPV + t;   // fewer than EPV elements
        if (rest < n)
            add_pair(widen<IO>(ref[rest]), widen<IO>(x[rest]), d[1], q[1]);
    }
    block_sum2((d[0] + d[1]) + (d[2] + d[3]), (q[0] + q[1]) + (q[2] + q[3]), lds);
    if (t == 0)
    {
        part[2 * (int64_t) blockIdx.x]     = lds[0];
        part[2 * (int64_t) blockIdx.x + 1] = lds[kQaBlock];
    }
}

// differently misaligned bases: element loads on both
template <int IO>
__global__ __launch_bounds__(kQaBlock) void qa_sq_err_elem_kernel(const typename Elem<IO>::type* __restrict__ ref,
                                                                  const typename Elem<IO>::type* __restrict__ x, int64_t n,
                                                                  double* __restrict__ part)
{
    __shared__ double lds[2 * kQaBlock];
    const int t = threadIdx.x;
    double d[2] = {0.0, 0.0}, q[2] = {0.0, 0.0};
    const int64_t stride = (int64_t) gridDim.x * kQaBlock;
    int64_t i            = (int64_t) blockIdx.x * kQaBlock + t;
    for (; i + stride < n; i += 2 * stride)
    {
        const auto r0 = ref[i], x0 = x[i], r1 = ref[i + stride], x1 = x[i + stride];
        add_pair(widen<IO>(r0), widen<IO>(x0), d[0], q[0]);
        add_pair(widen<IO>(r1), widen<IO>(x1), d[1], q[1]);
    }
    if (i < n)
        add_pair(widen<IO>(ref[i]), widen<IO>(x[i]), d[0], q[0]);
    block_sum2(d[0] + d[1], q[0] + q[1], lds);
    if (t == 0)
    {
        part[2 * (int64_t) blockIdx.x]     = lds[0];
        part[2 * (int64_t) blockIdx.x + 1] = lds[kQaBlock];
    }
}

// acc[j] += scale * (part[0][j] + part[1][j] + ...): lane t adds partials t * per .. in index order
__global__ __launch_bounds__(kQaBlock) void qa_fold_kernel(const double* __restrict__ part, int64_t nparts, int64_t per,
                                                           double scale, double* __restrict__ acc)
{
    __shared__ double lds[2 * kQaBlock];
    const int64_t lo = (int64_t) threadIdx.x * per;
    const int64_t hi = lo + per < nparts ? lo + per : nparts;
    double d = 0.0, q = 0.0;
    for (int64_t k = lo; k < hi; ++k)
    {
        d = d + part[2 * k];
        q = q + part[2 * k + 1];
    }
    block_sum2(d, q, lds);
    if (threadIdx.x == 0)
    {
        acc[0] = acc[0] + scale * lds[0];
        acc[1] = acc[1] + scale * lds[kQaBlock];
    }
}

// acc[0] += (S / n) / (N / n + eps) over the same partials, N = sum (ref - x)^2 and S = sum ref^2: the
// fold of qa_fold_kernel, then two means, the ratio and the add, each rounded once
__global__ __launch_bounds__(kQaBlock) void amp_sqnr_fold_kernel(const double* __restrict__ part, int64_t nparts,
                                                                 int64_t per, double n, double eps,
                                                                 double* __restrict__ acc)
{
    __shared__ double lds[2 * kQaBlock];
    const int64_t lo = (int64_t) threadIdx.x * per;
    const int64_t hi = lo + per < nparts ? lo + per : nparts;
    double d = 0.0, q = 0.0;
    for (int64_t k = lo; k < hi; ++k)
    {
        d = d + part[2 * k];
        q = q + part[2 * k + 1];
    }
    block_sum2(d, q, lds);
    if (threadIdx.x == 0)
    {
        const double noise = lds[0] / n, signal = lds[kQaBlock] / n;
        acc[0] = acc[0] + signal / (noise + eps);
    }
}

// The first launch of both entry points: a workgroup's (sum (ref - x)^2, sum ref^2) into part[2 * b ..].
// Returns the number of workgroups.
template <int IO>
int64_t launch_partials(const void* ref_v, const void* x_v, int64_t n, Scratch<double>& part, hipStream_t s)
{
    using T           = typename Elem<IO>::type;
    constexpr int EPV = 16 / (int) sizeof(T);
    const T* ref      = static_cast<const T*>(ref_v);
    const T* x        = static_cast<const T*>(x_v);
    const uintptr_t ra = reinterpret_cast<uintptr_t>(ref) & 15, xa = reinterpret_cast<uintptr_t>(x) & 15;
    int64_t blocks;
    if (ra == xa)
    {
        const int64_t head = std::min<int64_t>((int64_t) (((16 - ra) & 15) / sizeof(T)), n);
        const int64_t nv   = (n - head) / EPV;
        blocks             = stream_blocks(nv, kQaBlock * kQaVecPerLane);
        part               = Scratch<double>((size_t) blocks * 2, s);
        qa_sq_err_vec_kernel<IO><<<(unsigned) blocks, kQaBlock, 0, s>>>(ref, x, n, head, nv, part.get());
    }
    else
    {
        blocks = stream_blocks(n, kQaBlock * kQaVecPerLane * EPV);
        part   = Scratch<double>((size_t) blocks * 2, s);
        qa_sq_err_elem_kernel<IO><<<(unsigned) blocks, kQaBlock, 0, s>>>(ref, x, n, part.get());
    }
    AIMET_LAUNCH_CHECK();
    return blocks;
}

int64_t launch_partials(int io_dtype, const void* ref, const void* x, int64_t n, Scratch<double>& part, hipStream_t s)
{
    switch (io_dtype)
    {
    case IO_F32: return launch_partials<IO_F32>(ref, x, n, part, s);
    case IO_F16: return launch_partials<IO_F16>(ref, x, n, part, s);
    default: return launch_partials<IO_BF16>(ref, x, n, part, s);
    }
}

// what both entry points ask of their arguments
void require_pair(const void* ref, const void* x, int64_t n, int io_dtype, const double* acc_dev, const char* what)
{
    const std::string w(what);
    AIMET_REQUIRE(n > 0 && n <= kQaMaxElems, (w + ": n must be in 1 .. 2^40").c_str());
    AIMET_REQUIRE(io_dtype == IO_F32 || io_dtype == IO_F16 || io_dtype == IO_BF16,
                  (w + ": io_dtype is 0 (float32), 1 (float16) or 2 (bfloat16)").c_str());
    require_device_ptr(ref, (w + " reference").c_str());
    require_device_ptr(x, (w + " input").c_str());
    require_device_ptr(acc_dev, (w + " accumulator").c_str());
    const uintptr_t elem = io_dtype == IO_F32 ? 4 : 2;
    AIMET_REQUIRE((reinterpret_cast<uintptr_t>(ref) & (elem - 1)) == 0 &&
                      (reinterpret_cast<uintptr_t>(x) & (elem - 1)) == 0 &&
                      (reinterpret_cast<uintptr_t>(acc_dev) & 7) == 0,
                  (w + ": misaligned pointer").c_str());
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_qa_sq_err(const void* ref, const void* x, int64_t n, int io_dtype, double scale, double* acc_dev, void* stream)
{
    return guarded([&] {
        require_pair(ref, x, n, io_dtype, acc_dev, "squared error");
        hipStream_t s = as_stream(stream);
        Scratch<double> part;
        const int64_t blocks = launch_partials(io_dtype, ref, x, n, part, s);
        qa_fold_kernel<<<1, kQaBlock, 0, s>>>(part.get(), blocks, ceil_div(blocks, kQaBlock), scale, acc_dev);
        AIMET_LAUNCH_CHECK();
        g_launches.add(2);
    });
}

int aimet_amp_sqnr_add(const void* ref, const void* x, int64_t n, int io_dtype, double eps, double* acc_dev, void* stream)
{
    return guarded([&] {
        require_pair(ref, x, n, io_dtype, acc_dev, "SQNR");
        AIMET_REQUIRE(eps >= 0.0 && eps < std::numeric_limits<double>::infinity(), "SQNR: eps must be finite and >= 0");
        hipStream_t s = as_stream(stream);
        Scratch<double> part;
        const int64_t blocks = launch_partials(io_dtype, ref, x, n, part, s);
        amp_sqnr_fold_kernel<<<1, kQaBlock, 0, s>>>(part.get(), blocks, ceil_div(blocks, kQaBlock), (double) n, eps,
                                                    acc_dev);
        AIMET_LAUNCH_CHECK();
        g_amp_launches.add(2);
    });
}

int aimet_amp_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_amp_launches.read(count, reset); });
}

int aimet_qa_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
