// bias_corr.hip -- bias correction on the device (aimet_torch/bias_correction.py,
// aimet_common/bias_correction.py; the reference copies every layer output of the calibration set to
// the host and takes float32 numpy means there).
//
//  * aimet_bc_channel_sums: acc[c] += sum over a layer output of channel c, in double. One HBM read of
//    the tensor, nothing else. Two layouts, two kernels: planar ([outer][C][inner], NCHW) gives a
//    workgroup one (channel, split) and reads the channel's segments in 16-byte loads between a scalar
//    head and tail; interleaved ([rows][C], Linear and channels-last) gives a lane its columns and a
//    workgroup a range of rows. Both leave one double per (split, channel); a second, tiny launch
//    folds the splits in order into acc. No atomics: the order of every addition is fixed by the
//    sizes (and, for the choice between 16-byte and 4-byte loads, the base alignment) alone.
//  * aimet_bc_apply_empirical: bias[c] -= (q_sum[c] - ref_sum[c]) / count, rounded to fp32 once.
//  * aimet_bc_analytical: the BN-based correction of `count` layers in one launch, grid (job, output
//    channel): fp32 differences of the two weights, everything after in double.
#include <atomic>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kBcBlock         = 256;
constexpr int64_t kPieceFloats = 4096;   // planar: floats of one segment a workgroup takes at a time
constexpr int64_t kMinPerGroup = 8192;   // elements below which a further split is not worth a workgroup
constexpr int64_t kVecInner    = 128;    // planar segments shorter than this are read flat, 4 bytes a lane

std::atomic<int64_t> g_launches {0};

// Fixed-shape tree over the workgroup's 256 partials; lane 0's return value is the sum.
__device__ __forceinline__ double block_sum(double v, double* lds)
{
    const int t = threadIdx.x;
    lds[t]      = v;
    __syncthreads();
    for (int s = kBcBlock / 2; s > 0; s >>= 1)
    {
        if (t < s)
            lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// ---- planar, long segments: workgroup (c, split) takes pieces split, split + nsplit, ... of the
// channel's outer * pieces_per_seg pieces; a piece is piece_len floats of one segment (the last
// piece of a segment shorter).
__global__ __launch_bounds__(kBcBlock) void bc_planar_vec_kernel(const float* __restrict__ x, int64_t outer, int64_t C,
                                                                 int64_t inner, int64_t pieces_per_seg,
                                                                 int64_t piece_len, double* __restrict__ part)
{
    __shared__ double lds[kBcBlock];
    const int t          = threadIdx.x;
    const int64_t c      = blockIdx.x;
    const int64_t npiece = outer * pieces_per_seg;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
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
            a0 = a0 + (double) p[t];
        const float4* v  = reinterpret_cast<const float4*>(p + head);
        const int64_t nv = (n - head) >> 2;
#pragma unroll 4
        for (int64_t i = t; i < nv; i += kBcBlock)
        {
            const float4 f = v[i];
            a0             = a0 + (double) f.x;
            a1             = a1 + (double) f.y;
            a2             = a2 + (double) f.z;
            a3             = a3 + (double) f.w;
        }
        const int64_t rest = head + nv * 4 + t;   // at most three floats
        if (rest < n)
            a1 = a1 + (double) p[rest];
    }
    const double s = block_sum((a0 + a1) + (a2 + a3), lds);
    if (t == 0)
        part[(int64_t) blockIdx.y * C + c] = s;
}

// ---- planar, short segments: the channel's outer * inner elements as one flat range, workgroup
// (c, split) takes `chunk` of them; consecutive lanes read consecutive floats of a segment.
__global__ __launch_bounds__(kBcBlock) void bc_planar_flat_kernel(const float* __restrict__ x, int64_t C, int64_t inner,
                                                                  FastDiv by_inner, int64_t n, int64_t chunk,
                                                                  double* __restrict__ part)
{
    __shared__ double lds[kBcBlock];
    const int64_t c      = blockIdx.x;
    const int64_t lo     = (int64_t) blockIdx.y * chunk;
    const int64_t hi     = lo + chunk < n ? lo + chunk : n;
    const int64_t stride = C * inner;
    const float* base    = x + c * inner;
    double a0 = 0.0, a1 = 0.0;
    int64_t e = lo + threadIdx.x;
    for (; e + kBcBlock < hi; e += 2 * kBcBlock)
    {
        const uint32_t o0 = by_inner.div((uint32_t) e), o1 = by_inner.div((uint32_t) (e + kBcBlock));
        const float f0 = base[(int64_t) o0 * stride + (e - (int64_t) o0 * inner)];
        const float f1 = base[(int64_t) o1 * stride + (e + kBcBlock - (int64_t) o1 * inner)];
        a0             = a0 + (double) f0;
        a1             = a1 + (double) f1;
    }
    if (e < hi)
    {
        const uint32_t o0 = by_inner.div((uint32_t) e);
        a0                = a0 + (double) base[(int64_t) o0 * stride + (e - (int64_t) o0 * inner)];
    }
    const double s = block_sum(a0 + a1, lds);
    if (threadIdx.x == 0)
        part[(int64_t) blockIdx.y * C + c] = s;
}

// ---- interleaved: [rows][C]. The 256 lanes are LY rows x LX column units (a unit is VEC columns);
// workgroup (bx, split) owns column units bx * LX .. and the rows split * rows_per .. ; lane (ty, tx)
// adds the rows ty, ty + LY, ... of its range, then a fixed tree over ty.
template <int VEC>
__global__ __launch_bounds__(kBcBlock) void bc_interleaved_kernel(const float* __restrict__ x, int64_t rows, int64_t C,
                                                                  int lx_log2, int64_t rows_per,
                                                                  double* __restrict__ part)
{
    __shared__ double lds[kBcBlock * VEC];
    const int t = threadIdx.x, LX = 1 << lx_log2, LY = kBcBlock >> lx_log2;
    const int tx = t & (LX - 1), ty = t >> lx_log2;
    const int64_t unit  = (int64_t) blockIdx.x * LX + tx;
    const int64_t col   = unit * VEC;
    const int64_t r0    = (int64_t) blockIdx.y * rows_per;
    const int64_t r1    = r0 + rows_per < rows ? r0 + rows_per : rows;
    double a[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        a[k] = 0.0;
    if (col < C)
    {
#pragma unroll 4
        for (int64_t r = r0 + ty; r < r1; r += LY)
        {
            const float* p = x + r * C + col;
            if (VEC == 4)
            {
                const float4 f = *reinterpret_cast<const float4*>(p);
                a[0]           = a[0] + (double) f.x;
                a[1 % VEC]     = a[1 % VEC] + (double) f.y;
                a[2 % VEC]     = a[2 % VEC] + (double) f.z;
                a[3 % VEC]     = a[3 % VEC] + (double) f.w;
            }
            else
                a[0] = a[0] + (double) *p;
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        lds[k * kBcBlock + t] = a[k];
    __syncthreads();
    for (int s = LY >> 1; s > 0; s >>= 1)
    {
        if (ty < s)
        {
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                lds[k * kBcBlock + t] = lds[k * kBcBlock + t] + lds[k * kBcBlock + t + s * LX];
        }
        __syncthreads();
    }
    if (ty == 0 && col < C)
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            part[(int64_t) blockIdx.y * C + col + k] = lds[k * kBcBlock + t];
    }
}

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
        AIMET_REQUIRE(outer > 0 && C > 0 && inner > 0, "channel sums: outer, C and inner must be positive");
        AIMET_REQUIRE(C < (int64_t(1) << 31) && outer < (int64_t(1) << 31) && inner < (int64_t(1) << 31) &&
                          outer * inner < (int64_t(1) << 31) && outer * inner < (int64_t(1) << 46) / C,
                      "channel sums: too large (2^31 elements per channel, 2^46 in all)");
        require_device_ptr(x, "channel sums input");
        require_device_ptr(acc_dev, "channel sums accumulator");
        AIMET_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(acc_dev) & 7) == 0,
                      "channel sums: misaligned pointer");
        hipStream_t s = as_stream(stream);
        int64_t nsplit;
        double* part;
        if (inner == 1)
        {
            const int64_t rows = outer;
            const bool vec     = (C & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
            const int64_t units = vec ? C / 4 : C;
            int lx_log2         = 0;
            while (lx_log2 < 8 && (int64_t(1) << lx_log2) < units)
                ++lx_log2;
            const int64_t LX = int64_t(1) << lx_log2, LY = kBcBlock / LX;
            const int64_t gx = ceil_div(units, LX);
            AIMET_REQUIRE(gx < (int64_t(1) << 31), "channel sums: too many channels");
            nsplit                 = split_count(gx, rows * LX * (vec ? 4 : 1), ceil_div(rows, LY));
            const int64_t rows_per = ceil_div(rows, nsplit);
            nsplit                 = ceil_div(rows, rows_per);
            part                   = static_cast<double*>(scratch_alloc((size_t) (nsplit * C) * sizeof(double), s));
            const dim3 grid((unsigned) gx, (unsigned) nsplit);
            if (vec)
                bc_interleaved_kernel<4><<<grid, kBcBlock, 0, s>>>(x, rows, C, lx_log2, rows_per, part);
            else
                bc_interleaved_kernel<1><<<grid, kBcBlock, 0, s>>>(x, rows, C, lx_log2, rows_per, part);
        }
        else if (inner >= kVecInner)
        {
            const int64_t pieces_per_seg = ceil_div(inner, kPieceFloats);
            const int64_t piece_len      = ceil_div(ceil_div(inner, pieces_per_seg), 4) * 4;
            const int64_t pps            = ceil_div(inner, piece_len);
            nsplit                       = split_count(C, outer * inner, outer * pps);
            part = static_cast<double*>(scratch_alloc((size_t) (nsplit * C) * sizeof(double), s));
            bc_planar_vec_kernel<<<dim3((unsigned) C, (unsigned) nsplit), kBcBlock, 0, s>>>(x, outer, C, inner, pps,
                                                                                           piece_len, part);
        }
        else
        {
            const int64_t n     = outer * inner;
            nsplit              = split_count(C, n, ceil_div(n, kBcBlock));
            const int64_t chunk = ceil_div(ceil_div(n, nsplit), kBcBlock) * kBcBlock;
            nsplit              = ceil_div(n, chunk);
            part = static_cast<double*>(scratch_alloc((size_t) (nsplit * C) * sizeof(double), s));
            bc_planar_flat_kernel<<<dim3((unsigned) C, (unsigned) nsplit), kBcBlock, 0, s>>>(
                x, C, inner, FastDiv((uint32_t) inner), n, chunk, part);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
        {
            fold(part, nsplit, C, acc_dev, s);
            e = hipGetLastError();
        }
        scratch_free(part, s);
        AIMET_HIP_CHECK(e);
        g_launches.fetch_add(2, std::memory_order_relaxed);
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
        g_launches.fetch_add(1, std::memory_order_relaxed);
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
        auto* dev     = static_cast<AnaJob*>(upload_async(table.data(), table.size() * sizeof(AnaJob), s));
        bc_analytical_kernel<<<dim3((unsigned) max_cout, (unsigned) count), kBcBlock, 0, s>>>(dev);
        hipError_t e = hipGetLastError();
        scratch_free(dev, s);
        AIMET_HIP_CHECK(e);
        g_launches.fetch_add(1, std::memory_order_relaxed);
    });
}

int aimet_bc_launch_count(int64_t* count, int reset)
{
    return guarded([&] {
        const int64_t n = reset ? g_launches.exchange(0, std::memory_order_relaxed)
                                : g_launches.load(std::memory_order_relaxed);
        if (count)
            *count = n;
    });
}

}   // extern "C"
