// bias_corr.hip -- bias correction on the device (aimet_torch/bias_correction.py,
// aimet_common/bias_correction.py; the reference copies every layer output of the calibration set to
// the host and takes float32 numpy means there).
//
//  * aimet_bc_channel_sums: acc[c] += sum over a layer output of channel c, in double. One HBM read of
//    the tensor, nothing else: the ChannelSum accumulator on the traversals of channel_reduce.hpp
//    (planar long / planar short / interleaved), which leave one double per (split, channel); a
//    second, tiny launch folds the splits in order into acc. No atomics: the order of every addition
//    is fixed by the sizes (and, for the choice between 16-byte and 4-byte loads, the base alignment)
//    alone.
//  * aimet_bc_apply_empirical: bias[c] -= (q_sum[c] - ref_sum[c]) / count, rounded to fp32 once.
//  * aimet_bc_analytical: the BN-based correction of `count` layers in one launch, grid (job, output
//    channel): fp32 differences of the two weights, everything after in double.
#include <cmath>
#include <vector>

#include "channel_reduce.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kBcBlock = kReduceBlock;

LaunchCounter g_launches;

// acc[c] += part[0][c] + part[1][c] + ... , in that order
__global__ __launch_bounds__(kBcBlock) void bc_fold_kernel(const double* __restrict__ part, int64_t nsplit, int64_t C,
                                                           double* __restrict__ acc)
{
    const int64_t c = (int64_t) blockIdx.x * kBcBlock + threadIdx.x;
    if (c >= C)
        return;
    double s = 0.0;
    for (int64_t k = 0; k < nsplit; ++k)
        s = s + part[k * C + c];
    acc[c] = acc[c] + s;
}

__global__ __launch_bounds__(kBcBlock) void bc_apply_empirical_kernel(float* __restrict__ bias,
                                                                      const double* __restrict__ ref_sum,
                                                                      const double* __restrict__ q_sum, int64_t C,
                                                                      double count)
{
    const int64_t c = (int64_t) blockIdx.x * kBcBlock + threadIdx.x;
    if (c < C)
        bias[c] = (float) ((double) bias[c] - (q_sum[c] - ref_sum[c]) / count);
}

// ---- analytical -------------------------------------------------------------------------------------
struct AnaJob
{
    const float *w, *wq;
    float* bias;
    const float *gamma, *beta;
    int32_t activation;
    int64_t cout, cin, k, out_stride, in_stride;
};

__device__ __forceinline__ double norm_cdf(double v)
{
    return 0.5 * erfc(-v * 0.70710678118654752440);
}
__device__ __forceinline__ double norm_pdf(double v)
{
    return exp(-(v * v) / 2.0) / 2.50662827463100050242;   // sqrt(2 pi)
}

// E[x] of a clipped normal with mean beta and standard deviation gamma (gamma as given: a negative
// or zero gamma follows IEEE, as the reference's formula does)
__device__ __forceinline__ double expected_input(double beta, double gamma, int activation)
{
    if (activation == 0)
        return beta;
    const double lo = -beta / gamma;
    if (activation == 1)
        return beta * (1.0 - norm_cdf(lo)) + gamma * norm_pdf(lo);
    const double b = 6.0, hi = (b - beta) / gamma;
    const double z = norm_pdf(lo) - norm_pdf(hi);
    const double Z = norm_cdf(hi) - norm_cdf(lo);
    return (gamma * z + beta * Z) + b * (1.0 - norm_cdf(hi));
}

__global__ __launch_bounds__(kBcBlock) void bc_analytical_kernel(const AnaJob* jobs)
{
    __shared__ double lds[kBcBlock];
    const AnaJob j  = jobs[blockIdx.y];
    const int64_t o = blockIdx.x;
    if (o >= j.cout)
        return;
    double err = 0.0;
    for (int64_t i = threadIdx.x; i < j.cin; i += kBcBlock)
    {
        const int64_t at = o * j.out_stride + i * j.in_stride;
        double eps       = 0.0;
        for (int64_t q = 0; q < j.k; ++q)
        {
            const float d = j.wq[at + q] - j.w[at + q];
            eps           = eps + (double) d;
        }
        const int64_t ch   = j.cin == 1 ? o : i;
        const double gamma = j.gamma ? (double) j.gamma[ch] : 1.0;
        const double beta  = j.beta ? (double) j.beta[ch] : 0.0;
        err                = err + eps * expected_input(beta, gamma, j.activation);
    }
    err = block_sum(err, lds);
    if (threadIdx.x == 0)
        j.bias[o] = (float) ((double) j.bias[o] - err);
}

void fold(const double* part, int64_t nsplit, int64_t C, double* acc, hipStream_t s)
{
    bc_fold_kernel<<<(unsigned) ceil_div(C, kBcBlock), kBcBlock, 0, s>>>(part, nsplit, C, acc);
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_bc_channel_sums(const float* x, int64_t outer, int64_t C, int64_t inner, double* acc_dev, void* stream)
{
    return guarded([&] {
        require_channel_sizes("channel sums", outer, C, inner);
        require_device_ptr(x, "channel sums input");
        require_device_ptr(acc_dev, "channel sums accumulator");
        require_channel_alignment("channel sums", {x}, {acc_dev});
        hipStream_t s             = as_stream(stream);
        const auto [part, nsplit] = launch_channel_reduce<ChannelSum>(x, outer, C, inner, s);
        AIMET_LAUNCH_CHECK();
        fold(part.get(), nsplit, C, acc_dev, s);
        AIMET_LAUNCH_CHECK();
        g_launches.add(2);
    });
}

int aimet_bc_apply_empirical(float* bias, const double* ref_sum, const double* q_sum, int64_t C, double count,
                             void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(C > 0 && C < (int64_t(1) << 31), "empirical bias correction: invalid channel count");
        AIMET_REQUIRE(count > 0.0, "empirical bias correction: the element count must be positive");
        require_device_ptr(bias, "bias");
        require_device_ptr(ref_sum, "reference channel sums");
        require_device_ptr(q_sum, "quantized channel sums");
        bc_apply_empirical_kernel<<<(unsigned) ceil_div(C, kBcBlock), kBcBlock, 0, as_stream(stream)>>>(
            bias, ref_sum, q_sum, C, count);
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_bc_analytical(const aimet_bc_analytical_job* jobs, int64_t count, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(count >= 0 && count <= 65535, "analytical bias correction: 0..65535 jobs per launch");
        if (count == 0)
            return;
        AIMET_REQUIRE(jobs != nullptr, "analytical bias correction: job table is null");
        std::vector<AnaJob> table((size_t) count);
        int64_t max_cout = 0;
        for (int64_t n = 0; n < count; ++n)
        {
            const aimet_bc_analytical_job& j = jobs[n];
            const aimet_dfq_weight& w        = j.w;
            AIMET_REQUIRE(w.cout > 0 && w.cin > 0 && w.k > 0, "analytical bias correction: cout, cin and k must be positive");
            AIMET_REQUIRE(w.cout < (int64_t(1) << 31) && w.cin < (int64_t(1) << 31) && w.k < (int64_t(1) << 31) &&
                              w.cout * w.cin < (int64_t(1) << 40) / w.k,
                          "analytical bias correction: weight too large");
            AIMET_REQUIRE((w.out_stride == w.cin * w.k && w.in_stride == w.k) ||
                              (w.out_stride == w.k && w.in_stride == w.cout * w.k),
                          "analytical bias correction: strides must be (cin*k, k) or, for a transposed weight, "
                          "(k, cout*k)");
            AIMET_REQUIRE(j.activation >= 0 && j.activation <= 2, "analytical bias correction: activation is 0, 1 or 2");
            AIMET_REQUIRE((j.gamma == nullptr) == (j.beta == nullptr),
                          "analytical bias correction: gamma and beta are both given or both null");
            require_device_ptr(w.data, "analytical bias correction weight");
            require_device_ptr(j.wq, "analytical bias correction quantized weight");
            require_device_ptr(j.bias, "analytical bias correction bias");
            if (j.gamma)
            {
                require_device_ptr(j.gamma, "analytical bias correction gamma");
                require_device_ptr(j.beta, "analytical bias correction beta");
            }
            for (int64_t m = 0; m < n; ++m)
                AIMET_REQUIRE(jobs[m].bias != j.bias, "analytical bias correction: two jobs on the same bias");
            table[(size_t) n] = AnaJob {w.data, j.wq,  j.bias, j.gamma,      j.beta,     j.activation,
                                        w.cout, w.cin, w.k,    w.out_stride, w.in_stride};
            max_cout          = std::max(max_cout, w.cout);
        }
        hipStream_t s = as_stream(stream);
        auto dev      = Scratch<AnaJob>::upload(table, s);
        bc_analytical_kernel<<<dim3((unsigned) max_cout, (unsigned) count), kBcBlock, 0, s>>>(dev.get());
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_bc_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
