// bn_reest.hip -- BatchNorm re-estimation on the device (aimet_torch/bn_reestimation.py; the reference
// runs every BatchNorm in training mode at momentum 1 and adds the running buffers into float32 sums
// after every batch: a library BN kernel, a momentum update and two adds per BatchNorm and batch).
//
//  * aimet_bnre_forward: one training-mode BatchNorm forward that also adds the batch's mean and
//    unbiased variance into two double accumulators. Three launches: per-(split, channel) partials
//    D1 = sum (x - K), D2 = sum (x - K)^2 with the shift K = x[0][c][0] (difference, square and sums
//    in double; one read of x); a fold over the splits, in order, that also derives the fp32
//    coefficients a, b of y = fma(x, a, b); the normalisation (one read, one write, 16-byte
//    accesses between a scalar head and tail). 12 bytes per element. The partials are the Moments
//    accumulator on the traversals of channel_reduce.hpp (planar long / planar short / interleaved).
//    A channel of at most 15872 elements takes the resident form instead: one launch, one workgroup
//    per channel that keeps the channel in LDS between the sums and the normalisation (8 bytes per
//    element; 2.3-4.1 times faster than the three launches at 32x1024x14x14, 32x2048x7x7 and 32x1000,
//    profiles/r15/bn_reestimation_models.txt).
//  * aimet_bnre_finish: running_mean = (float) (sum_mean / count), running_var likewise, for a table
//    of BatchNorms in one launch.
// No atomics: the order of every addition is fixed by the sizes (and, for the choice between 16-byte
// and 4-byte accesses, the base alignment) alone, so equal inputs give equal bits.
#include <atomic>
#include <cmath>
#include <vector>

#include "channel_reduce.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kBlk               = kReduceBlock;
constexpr int64_t kMaxNormBlocks = int64_t(1) << 20;

// resident form: 62 KiB of a channel beside the tree's 2 KiB, so two workgroups and more fit a CU
constexpr int64_t kResidentMaxN = 15872;

LaunchCounter g_launches;
std::atomic<int> g_form {0};   // aimet_bnre_forward_form: 0 and 2 resident where it fits, 1 streaming

// The splits of channel c summed in order; the batch's mean and unbiased variance added to the
// accumulators; ab[c] = (a, b) of y = fma(x, a, b), evaluated in double and rounded once.
__global__ __launch_bounds__(kBlk) void bnre_fold_kernel(const double* __restrict__ part, int64_t nsplit, int64_t C,
                                                         const float* __restrict__ x, int64_t inner, double n,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, double eps,
                                                         double* __restrict__ sum_mean, double* __restrict__ sum_var,
                                                         float2* __restrict__ ab)
{
    const int64_t c = (int64_t) blockIdx.x * kBlk + threadIdx.x;
    if (c >= C)
        return;
    double D1 = 0.0, D2 = 0.0;
    for (int64_t k = 0; k < nsplit; ++k)
    {
        D1 = D1 + part[k * C + c];
        D2 = D2 + part[(nsplit + k) * C + c];
    }
    const double K     = (double) x[c * inner];
    const double m     = D1 / n;
    const double mean  = K + m;
    const double M2    = D2 - D1 * m;
    const double var_b = M2 / n, var_u = M2 / (n - 1.0);
    sum_mean[c]        = sum_mean[c] + mean;
    sum_var[c]         = sum_var[c] + var_u;
    const double g     = gamma ? (double) gamma[c] : 1.0;
    const double bt    = beta ? (double) beta[c] : 0.0;
    const double a     = g / sqrt(var_b + eps);
    ab[c]              = make_float2((float) a, (float) (bt - mean * a));
}

// y = fma(x, a[c], b[c]) over the tensor as one flat range of `total` floats, c = (e / inner) mod C.
// VEC: x and y are equally misaligned to 16 bytes; lane g of the grid takes the four floats at
// head + 4 g, the first workgroup also the head (< 4 floats) and the tail (< 4 floats).
template <bool VEC>
__global__ __launch_bounds__(kBlk) void bnre_normalise_kernel(const float* x, float* y, int64_t total, int64_t C,
                                                              int64_t inner, int64_t head,
                                                              const float2* __restrict__ ab)
{
    constexpr int W      = VEC ? 4 : 1;
    const int64_t nv     = (total - head) / W;
    const int64_t stride = (int64_t) gridDim.x * kBlk;
    for (int64_t g = (int64_t) blockIdx.x * kBlk + threadIdx.x; g < nv; g += stride)
    {
        const int64_t e   = head + g * W;
        const int64_t row = e / inner;
        int64_t i         = e - row * inner;
        int64_t c         = row % C;
        float2 k          = ab[c];
        if (VEC)
        {
            float4 f = *reinterpret_cast<const float4*>(x + e);
            float v[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
                v[q] = __builtin_fmaf(v[q], k.x, k.y);
                if (++i == inner && q < 3)
                {
                    i = 0;
                    c = c + 1 == C ? 0 : c + 1;
                    k = ab[c];
                }
            }
            *reinterpret_cast<float4*>(y + e) = make_float4(v[0], v[1], v[2], v[3]);
        }
        else
            y[e] = __builtin_fmaf(x[e], k.x, k.y);
    }
    if (VEC && blockIdx.x == 0)
    {
        const int64_t tail = head + nv * 4;
        const int t        = threadIdx.x;
        const int64_t e    = t < head ? t : tail + (t - head);   // lanes 0 .. head - 1 the head, the next ones the tail
        if (e < total && (t < head || e >= tail))
        {
            const float2 k = ab[(e / inner) % C];
            y[e]           = __builtin_fmaf(x[e], k.x, k.y);
        }
    }
}

// ---- resident form: workgroup c keeps channel c's n floats in LDS between the sums and the
// normalisation, so x is read from HBM once (8 bytes per element, one launch). Lane t takes the
// elements t, t + 256, ... of the channel's flat range; every lane derives the same a and b.
__global__ __launch_bounds__(kBlk) void bnre_resident_kernel(const float* x, float* y, int64_t C, int64_t inner,
                                                             FastDiv by_inner, int n,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, double eps,
                                                             double* __restrict__ sum_mean,
                                                             double* __restrict__ sum_var)
{
    extern __shared__ float held[];
    __shared__ double lds[kBlk];
    const int64_t c      = blockIdx.x;
    const int64_t stride = C * inner;
    const int64_t base   = c * inner;
    const double K       = (double) x[base];
    Moments::Lane m;
    for (int e = threadIdx.x; e < n; e += kBlk)
    {
        const uint32_t o = by_inner.div((uint32_t) e);
        const float v    = x[base + (int64_t) o * stride + (e - (int64_t) o * inner)];
        held[e]          = v;
        Moments::add(m, v, K);
    }
    const double D1    = block_sum(m.d1, lds);
    const double D2    = block_sum(m.d2, lds);
    const double mu    = D1 / (double) n;
    const double mean  = K + mu;
    const double M2    = D2 - D1 * mu;
    const double var_b = M2 / (double) n, var_u = M2 / ((double) n - 1.0);
    if (threadIdx.x == 0)
    {
        sum_mean[c] = sum_mean[c] + mean;
        sum_var[c]  = sum_var[c] + var_u;
    }
    const double g  = gamma ? (double) gamma[c] : 1.0;
    const double bt = beta ? (double) beta[c] : 0.0;
    const double ad = g / sqrt(var_b + eps);
    const float a = (float) ad, b = (float) (bt - mean * ad);
    for (int e = threadIdx.x; e < n; e += kBlk)
    {
        const uint32_t o = by_inner.div((uint32_t) e);
        y[base + (int64_t) o * stride + (e - (int64_t) o * inner)] = __builtin_fmaf(held[e], a, b);
    }
}

struct FinishJob
{
    const double *sum_mean, *sum_var;
    float *running_mean, *running_var;
    int64_t C;
    double count;
};

__global__ __launch_bounds__(kBlk) void bnre_finish_kernel(const FinishJob* jobs)
{
    const FinishJob j = jobs[blockIdx.y];
    const int64_t c   = (int64_t) blockIdx.x * kBlk + threadIdx.x;
    if (c >= j.C)
        return;
    j.running_mean[c] = (float) (j.sum_mean[c] / j.count);
    j.running_var[c]  = (float) (j.sum_var[c] / j.count);
}

}   // namespace

void bnre_count_launches(int64_t n)
{
    g_launches.add(n);
}

}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_bnre_forward(const float* x, int64_t outer, int64_t C, int64_t inner, const float* gamma, const float* beta,
                       float eps, float* y, double* sum_mean_dev, double* sum_var_dev, void* stream)
{
    return guarded([&] {
        require_channel_sizes("BN re-estimation", outer, C, inner);
        AIMET_REQUIRE(outer * inner >= 2, "BN re-estimation: a training-mode BatchNorm needs more than one value per "
                                          "channel");
        require_device_ptr(x, "BN re-estimation input");
        require_device_ptr(y, "BN re-estimation output");
        require_device_ptr(sum_mean_dev, "BN re-estimation mean accumulator");
        require_device_ptr(sum_var_dev, "BN re-estimation variance accumulator");
        if (gamma)
            require_device_ptr(gamma, "BN gamma");
        if (beta)
            require_device_ptr(beta, "BN beta");
        const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
        require_channel_alignment("BN re-estimation", {x, y}, {sum_mean_dev, sum_var_dev});
        hipStream_t s   = as_stream(stream);
        const int64_t n = outer * inner;
        const int form  = g_form.load(std::memory_order_relaxed);
        if (n <= kResidentMaxN && form != 1)
        {
            bnre_resident_kernel<<<(unsigned) C, kBlk, (size_t) n * sizeof(float), s>>>(
                x, y, C, inner, FastDiv((uint32_t) inner), (int) n, gamma, beta, (double) eps, sum_mean_dev,
                sum_var_dev);
            AIMET_LAUNCH_CHECK();
            g_launches.add(1);
            return;
        }
        const auto [part, nsplit] = launch_channel_reduce<Moments>(x, outer, C, inner, s);
        Scratch<float2> ab((size_t) C, s);
        AIMET_LAUNCH_CHECK();
        bnre_fold_kernel<<<(unsigned) ceil_div(C, kBlk), kBlk, 0, s>>>(part.get(), nsplit, C, x, inner, (double) n,
                                                                      gamma, beta, (double) eps, sum_mean_dev,
                                                                      sum_var_dev, ab.get());
        AIMET_LAUNCH_CHECK();
        const int64_t total = n * C;
        if (((xa ^ ya) & 15) == 0)
        {
            const int64_t head   = std::min<int64_t>((int64_t) (((16 - (xa & 15)) & 15) >> 2), total);
            const int64_t blocks = clamp64(ceil_div((total - head) / 4, kBlk), 1, kMaxNormBlocks);
            bnre_normalise_kernel<true><<<(unsigned) blocks, kBlk, 0, s>>>(x, y, total, C, inner, head, ab.get());
        }
        else
        {
            const int64_t blocks = clamp64(ceil_div(total, kBlk), 1, kMaxNormBlocks);
            bnre_normalise_kernel<false><<<(unsigned) blocks, kBlk, 0, s>>>(x, y, total, C, inner, 0, ab.get());
        }
        AIMET_LAUNCH_CHECK();
        g_launches.add(3);
    });
}

int aimet_bnre_finish(const aimet_bnre_finish_job* jobs, int64_t count, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(count >= 0 && count <= 65535, "BN re-estimation finish: 0..65535 jobs per launch");
        if (count == 0)
            return;
        AIMET_REQUIRE(jobs != nullptr, "BN re-estimation finish: job table is null");
        std::vector<FinishJob> table((size_t) count);
        int64_t max_c = 0;
        for (int64_t n = 0; n < count; ++n)
        {
            const aimet_bnre_finish_job& j = jobs[n];
            AIMET_REQUIRE(j.C > 0 && j.C < (int64_t(1) << 31), "BN re-estimation finish: invalid channel count");
            AIMET_REQUIRE(j.count > 0.0, "BN re-estimation finish: the batch count must be positive");
            require_device_ptr(j.sum_mean, "BN re-estimation mean accumulator");
            require_device_ptr(j.sum_var, "BN re-estimation variance accumulator");
            require_device_ptr(j.running_mean, "BN running mean");
            require_device_ptr(j.running_var, "BN running var");
            table[(size_t) n] = FinishJob {j.sum_mean, j.sum_var, j.running_mean, j.running_var, j.C, j.count};
            max_c             = std::max(max_c, j.C);
        }
        hipStream_t s = as_stream(stream);
        auto dev      = Scratch<FinishJob>::upload(table, s);
        bnre_finish_kernel<<<dim3((unsigned) ceil_div(max_c, kBlk), (unsigned) count), kBlk, 0, s>>>(dev.get());
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_bnre_forward_form(int form, int* previous)
{
    return guarded([&] {
        AIMET_REQUIRE(form >= 0 && form <= 2, "BN re-estimation form: 0 (default), 1 (streaming) or 2 (resident)");
        const int was = g_form.exchange(form, std::memory_order_relaxed);
        if (previous)
            *previous = was;
    });
}

int aimet_bnre_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
