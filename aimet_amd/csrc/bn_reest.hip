// bn_reest.hip -- BatchNorm re-estimation on the device (aimet_torch/bn_reestimation.py; the reference
// runs every BatchNorm in training mode at momentum 1 and adds the running buffers into float32 sums
// after every batch: a library BN kernel, a momentum update and two adds per BatchNorm and batch).
//
//  * aimet_bnre_forward: one training-mode BatchNorm forward that also adds the batch's mean and
//    unbiased variance into two double accumulators. Three launches: per-(split, channel) partials
//    D1 = sum (x - K), D2 = sum (x - K)^2 with the shift K = x[0][c][0] (difference, square and sums
//    in double; one read of x); a fold over the splits, in order, that also derives the fp32
//    coefficients a, b of y = fma(x, a, b); the normalisation (one read, one write, 16-byte
//    accesses between a scalar head and tail). 12 bytes per element. The partials kernels are those
//    of bias_corr.hip (planar long / planar short / interleaved) with the second sum added.
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

#include "common.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kBlk             = 256;
constexpr int64_t kPieceFloats = 4096;   // planar: floats of one segment a workgroup takes at a time
constexpr int64_t kMinPerGroup = 8192;   // elements below which a further split is not worth a workgroup
constexpr int64_t kVecInner    = 128;    // planar segments shorter than this are read flat, 4 bytes a lane
constexpr int64_t kMaxNormBlocks = int64_t(1) << 20;

// resident form: 62 KiB of a channel beside the tree's 2 KiB, so two workgroups and more fit a CU
constexpr int64_t kResidentMaxN = 15872;

std::atomic<int64_t> g_launches {0};
std::atomic<int> g_form {0};   // aimet_bnre_forward_form: 0 and 2 resident where it fits, 1 streaming

// the two shifted sums of one lane
struct Moments
{
    double d1 = 0.0, d2 = 0.0;
    __device__ __forceinline__ void add(float v, double K)
    {
        const double d = (double) v - K;
        d1             = d1 + d;
        d2             = d2 + d * d;
    }
};

// Fixed-shape tree over the workgroup's 256 partials; lane 0's return value is the sum.
__device__ __forceinline__ double block_sum(double v, double* lds)
{
    const int t = threadIdx.x;
    lds[t]      = v;
    __syncthreads();
    for (int s = kBlk / 2; s > 0; s >>= 1)
    {
        if (t < s)
            lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// part holds the D1 of every (split, channel), then the D2 of every (split, channel)
__device__ __forceinline__ void store_partials(double s1, double s2, double* part, int64_t c, int64_t C)
{
    if (threadIdx.x == 0)
    {
        const int64_t at = (int64_t) blockIdx.y * C + c;
        part[at]                             = s1;
        part[(int64_t) gridDim.y * C + at]   = s2;
    }
}

// ---- planar, long segments: workgroup (c, split) takes pieces split, split + nsplit, ... of the
// channel's outer * pieces_per_seg pieces; a piece is piece_len floats of one segment.
__global__ __launch_bounds__(kBlk) void bnre_planar_vec_kernel(const float* __restrict__ x, int64_t outer, int64_t C,
                                                               int64_t inner, int64_t pieces_per_seg,
                                                               int64_t piece_len, double* __restrict__ part)
{
    __shared__ double lds[kBlk];
    const int t          = threadIdx.x;
    const int64_t c      = blockIdx.x;
    const int64_t npiece = outer * pieces_per_seg;
    const double K       = (double) x[c * inner];
    Moments m0, m1, m2, m3;
    for (int64_t q = blockIdx.y; q < npiece; q += gridDim.y)
    {
        const int64_t o     = q / pieces_per_seg;
        const int64_t start = (q - o * pieces_per_seg) * piece_len;
        const int64_t n     = (inner - start) < piece_len ? (inner - start) : piece_len;
        const float* p      = x + (o * C + c) * inner + start;
        int64_t head        = (int64_t) (((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
        if (head > n)
            head = n;
        if (t < head)
            m0.add(p[t], K);
        const float4* v  = reinterpret_cast<const float4*>(p + head);
        const int64_t nv = (n - head) >> 2;
#pragma unroll 4
        for (int64_t i = t; i < nv; i += kBlk)
        {
            const float4 f = v[i];
            m0.add(f.x, K);
            m1.add(f.y, K);
            m2.add(f.z, K);
            m3.add(f.w, K);
        }
        const int64_t rest = head + nv * 4 + t;   // at most three floats
        if (rest < n)
            m1.add(p[rest], K);
    }
    const double s1 = block_sum((m0.d1 + m1.d1) + (m2.d1 + m3.d1), lds);
    const double s2 = block_sum((m0.d2 + m1.d2) + (m2.d2 + m3.d2), lds);
    store_partials(s1, s2, part, c, C);
}

// ---- planar, short segments: the channel's outer * inner elements as one flat range, workgroup
// (c, split) takes `chunk` of them; consecutive lanes read consecutive floats of a segment.
__global__ __launch_bounds__(kBlk) void bnre_planar_flat_kernel(const float* __restrict__ x, int64_t C, int64_t inner,
                                                                FastDiv by_inner, int64_t n, int64_t chunk,
                                                                double* __restrict__ part)
{
    __shared__ double lds[kBlk];
    const int64_t c      = blockIdx.x;
    const int64_t lo     = (int64_t) blockIdx.y * chunk;
    const int64_t hi     = lo + chunk < n ? lo + chunk : n;
    const int64_t stride = C * inner;
    const float* base    = x + c * inner;
    const double K       = (double) base[0];
    Moments m0, m1;
    int64_t e = lo + threadIdx.x;
    for (; e + kBlk < hi; e += 2 * kBlk)
    {
        const uint32_t o0 = by_inner.div((uint32_t) e), o1 = by_inner.div((uint32_t) (e + kBlk));
        const float f0 = base[(int64_t) o0 * stride + (e - (int64_t) o0 * inner)];
        const float f1 = base[(int64_t) o1 * stride + (e + kBlk - (int64_t) o1 * inner)];
        m0.add(f0, K);
        m1.add(f1, K);
    }
    if (e < hi)
    {
        const uint32_t o0 = by_inner.div((uint32_t) e);
        m0.add(base[(int64_t) o0 * stride + (e - (int64_t) o0 * inner)], K);
    }
    const double s1 = block_sum(m0.d1 + m1.d1, lds);
    const double s2 = block_sum(m0.d2 + m1.d2, lds);
    store_partials(s1, s2, part, c, C);
}

// ---- interleaved: [rows][C]. The 256 lanes are LY rows x LX column units (a unit is VEC columns);
// workgroup (bx, split) owns column units bx * LX .. and the rows split * rows_per .. ; lane (ty, tx)
// adds the rows ty, ty + LY, ... of its range, then a fixed tree over ty.
template <int VEC>
__global__ __launch_bounds__(kBlk) void bnre_interleaved_kernel(const float* __restrict__ x, int64_t rows, int64_t C,
                                                                int lx_log2, int64_t rows_per,
                                                                double* __restrict__ part)
{
    __shared__ double lds[kBlk * VEC];
    const int t = threadIdx.x, LX = 1 << lx_log2, LY = kBlk >> lx_log2;
    const int tx = t & (LX - 1), ty = t >> lx_log2;
    const int64_t unit = (int64_t) blockIdx.x * LX + tx;
    const int64_t col  = unit * VEC;
    const int64_t r0   = (int64_t) blockIdx.y * rows_per;
    const int64_t r1   = r0 + rows_per < rows ? r0 + rows_per : rows;
    Moments m[VEC];
    if (col < C)
    {
        double K[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            K[k] = (double) x[col + k];
#pragma unroll 4
        for (int64_t r = r0 + ty; r < r1; r += LY)
        {
            const float* p = x + r * C + col;
            if (VEC == 4)
            {
                const float4 f = *reinterpret_cast<const float4*>(p);
                m[0].add(f.x, K[0]);
                m[1 % VEC].add(f.y, K[1 % VEC]);
                m[2 % VEC].add(f.z, K[2 % VEC]);
                m[3 % VEC].add(f.w, K[3 % VEC]);
            }
            else
                m[0].add(*p, K[0]);
        }
    }
    for (int pass = 0; pass < 2; ++pass)
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            lds[k * kBlk + t] = pass ? m[k].d2 : m[k].d1;
        __syncthreads();
        for (int s = LY >> 1; s > 0; s >>= 1)
        {
            if (ty < s)
            {
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    lds[k * kBlk + t] = lds[k * kBlk + t] + lds[k * kBlk + t + s * LX];
            }
            __syncthreads();
        }
        if (ty == 0 && col < C)
        {
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                part[((int64_t) pass * gridDim.y + blockIdx.y) * C + col + k] = lds[k * kBlk + t];
        }
        __syncthreads();
    }
}

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
    Moments m;
    for (int e = threadIdx.x; e < n; e += kBlk)
    {
        const uint32_t o = by_inner.div((uint32_t) e);
        const float v    = x[base + (int64_t) o * stride + (e - (int64_t) o * inner)];
        held[e]          = v;
        m.add(v, K);
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

// ---- host side ---------------------------------------------------------------------------------------
int64_t clamp64(int64_t v, int64_t lo, int64_t hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

// splits of a channel of n elements when `groups` workgroups exist per split: fill the chip, but
// leave every workgroup kMinPerGroup elements
int64_t split_count(int64_t groups, int64_t n, int64_t most)
{
    return clamp64(std::min(ceil_div(kMaxStreamBlocks, groups), ceil_div(n, kMinPerGroup)), 1, std::min<int64_t>(most, 65535));
}

}   // namespace

void bnre_count_launches(int64_t n)
{
    g_launches.fetch_add(n, std::memory_order_relaxed);
}

}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_bnre_forward(const float* x, int64_t outer, int64_t C, int64_t inner, const float* gamma, const float* beta,
                       float eps, float* y, double* sum_mean_dev, double* sum_var_dev, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(outer > 0 && C > 0 && inner > 0, "BN re-estimation: outer, C and inner must be positive");
        AIMET_REQUIRE(C < (int64_t(1) << 31) && outer < (int64_t(1) << 31) && inner < (int64_t(1) << 31) &&
                          outer * inner < (int64_t(1) << 31) && outer * inner < (int64_t(1) << 46) / C,
                      "BN re-estimation: too large (2^31 elements per channel, 2^46 in all)");
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
        AIMET_REQUIRE((xa & 3) == 0 && (ya & 3) == 0 && (reinterpret_cast<uintptr_t>(sum_mean_dev) & 7) == 0 &&
                          (reinterpret_cast<uintptr_t>(sum_var_dev) & 7) == 0,
                      "BN re-estimation: misaligned pointer");
        hipStream_t s   = as_stream(stream);
        const int64_t n = outer * inner;
        const int form  = g_form.load(std::memory_order_relaxed);
        if (n <= kResidentMaxN && form != 1)
        {
            bnre_resident_kernel<<<(unsigned) C, kBlk, (size_t) n * sizeof(float), s>>>(
                x, y, C, inner, FastDiv((uint32_t) inner), (int) n, gamma, beta, (double) eps, sum_mean_dev,
                sum_var_dev);
            AIMET_LAUNCH_CHECK();
            g_launches.fetch_add(1, std::memory_order_relaxed);
            return;
        }
        int64_t nsplit;
        double* part;
        auto alloc_part = [&] { return static_cast<double*>(scratch_alloc((size_t) (2 * nsplit * C) * sizeof(double), s)); };
        if (inner == 1)
        {
            const int64_t rows  = outer;
            const bool vec      = (C & 3) == 0 && (xa & 15) == 0;
            const int64_t units = vec ? C / 4 : C;
            int lx_log2         = 0;
            while (lx_log2 < 8 && (int64_t(1) << lx_log2) < units)
                ++lx_log2;
            const int64_t LX = int64_t(1) << lx_log2, LY = kBlk / LX;
            const int64_t gx = ceil_div(units, LX);
            nsplit                 = split_count(gx, rows * LX * (vec ? 4 : 1), ceil_div(rows, LY));
            const int64_t rows_per = ceil_div(rows, nsplit);
            nsplit                 = ceil_div(rows, rows_per);
            part                   = alloc_part();
            const dim3 grid((unsigned) gx, (unsigned) nsplit);
            if (vec)
                bnre_interleaved_kernel<4><<<grid, kBlk, 0, s>>>(x, rows, C, lx_log2, rows_per, part);
            else
                bnre_interleaved_kernel<1><<<grid, kBlk, 0, s>>>(x, rows, C, lx_log2, rows_per, part);
        }
        else if (inner >= kVecInner)
        {
            const int64_t pieces_per_seg = ceil_div(inner, kPieceFloats);
            const int64_t piece_len      = ceil_div(ceil_div(inner, pieces_per_seg), 4) * 4;
            const int64_t pps            = ceil_div(inner, piece_len);
            nsplit                       = split_count(C, n, outer * pps);
            part                         = alloc_part();
            bnre_planar_vec_kernel<<<dim3((unsigned) C, (unsigned) nsplit), kBlk, 0, s>>>(x, outer, C, inner, pps,
                                                                                         piece_len, part);
        }
        else
        {
            nsplit              = split_count(C, n, ceil_div(n, kBlk));
            const int64_t chunk = ceil_div(ceil_div(n, nsplit), kBlk) * kBlk;
            nsplit              = ceil_div(n, chunk);
            part                = alloc_part();
            bnre_planar_flat_kernel<<<dim3((unsigned) C, (unsigned) nsplit), kBlk, 0, s>>>(
                x, C, inner, FastDiv((uint32_t) inner), n, chunk, part);
        }
        auto* ab     = static_cast<float2*>(scratch_alloc((size_t) C * sizeof(float2), s));
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
        {
            bnre_fold_kernel<<<(unsigned) ceil_div(C, kBlk), kBlk, 0, s>>>(part, nsplit, C, x, inner, (double) n, gamma,
                                                                          beta, (double) eps, sum_mean_dev,
                                                                          sum_var_dev, ab);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
        {
            const int64_t total = n * C;
            if (((xa ^ ya) & 15) == 0)
            {
                const int64_t head   = std::min<int64_t>((int64_t) (((16 - (xa & 15)) & 15) >> 2), total);
                const int64_t blocks = clamp64(ceil_div((total - head) / 4, kBlk), 1, kMaxNormBlocks);
                bnre_normalise_kernel<true><<<(unsigned) blocks, kBlk, 0, s>>>(x, y, total, C, inner, head, ab);
            }
            else
            {
                const int64_t blocks = clamp64(ceil_div(total, kBlk), 1, kMaxNormBlocks);
                bnre_normalise_kernel<false><<<(unsigned) blocks, kBlk, 0, s>>>(x, y, total, C, inner, 0, ab);
            }
            e = hipGetLastError();
        }
        scratch_free(part, s);
        scratch_free(ab, s);
        AIMET_HIP_CHECK(e);
        g_launches.fetch_add(3, std::memory_order_relaxed);
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
        auto* dev     = static_cast<FinishJob*>(upload_async(table.data(), table.size() * sizeof(FinishJob), s));
        bnre_finish_kernel<<<dim3((unsigned) ceil_div(max_c, kBlk), (unsigned) count), kBlk, 0, s>>>(dev);
        hipError_t e = hipGetLastError();
        scratch_free(dev, s);
        AIMET_HIP_CHECK(e);
        g_launches.fetch_add(1, std::memory_order_relaxed);
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
    return guarded([&] {
        const int64_t n = reset ? g_launches.exchange(0, std::memory_order_relaxed)
                                : g_launches.load(std::memory_order_relaxed);
        if (count)
            *count = n;
    });
}

}   // extern "C"
