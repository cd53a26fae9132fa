// channel_reduce.hpp -- the one skeleton of the per-channel reductions over a layer output
// [outer][C][inner]: bias correction's channel sums (bias_corr.hip) and BatchNorm re-estimation's
// shifted moments (bn_reest.hip).
//
// One HBM read of the tensor leaves, for each of an accumulator's N sums, one double per
// (split, channel): part[(k * nsplit + split) * C + c]. The caller folds the splits in order in a
// launch of its own and frees the scratch. Two layouts, three traversals: planar ([outer][C][inner],
// NCHW) gives a workgroup one (channel, split) and reads long segments in 16-byte loads between a
// scalar head and tail, short ones as one flat range per channel; interleaved ([rows][C], Linear and
// channels-last) gives a lane its columns and a workgroup a range of rows. No atomics: the order of
// every addition is fixed by the sizes (and, for the choice between 16-byte and 4-byte loads, the
// base alignment) alone, so equal inputs give equal bits. That order is written here and nowhere
// else: which element goes to which of a lane's accumulators, how a lane's accumulators combine, the
// LDS tree, the planner's split rule.
//
// An accumulator names a lane's running value of N sums and how an element enters it. It has
//   N                  number of sums
//   Lane               the running value, zero when value-initialised
//   Shift              a per-channel value every add takes (an empty struct: none, and no load)
//   shift(x, at)       the channel's Shift, from its first element x[at]
//   add(lane, v, K)    one element
//   get(lane, k)       sum k
#pragma once

#include <initializer_list>
#include <string>

#include "common.hpp"

namespace aimet_amd
{

constexpr int kReduceBlock     = 256;    // block_sum's tree and the traversals are written for it
constexpr int64_t kPieceFloats = 4096;   // planar: floats of one segment a workgroup takes at a time
constexpr int64_t kMinPerGroup = 8192;   // elements below which a further split is not worth a workgroup
constexpr int64_t kVecInner    = 128;    // planar segments shorter than this are read flat, 4 bytes a lane

// Fixed-shape tree over the workgroup's 256 partials; lane 0's return value is the sum.
__device__ __forceinline__ double block_sum(double v, double* lds)
{
    const int t = threadIdx.x;
    lds[t]      = v;
    __syncthreads();
    for (int s = kReduceBlock / 2; s > 0; s >>= 1)
    {
        if (t < s)
            lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// ---- accumulators --------------------------------------------------------------------------------
// the plain sum. The lane value is a bare double: wrapped in a struct it changed how the interleaved
// row loop forms its addresses (profiles/r18/channel_reduce_isa.txt).
struct ChannelSum
{
    static constexpr int N = 1;
    using Lane             = double;
    struct Shift
    {
    };
    static __device__ __forceinline__ Shift shift(const float*, int64_t)
    {
        return {};
    }
    static __device__ __forceinline__ void add(Lane& a, float v, Shift)
    {
        a = a + (double) v;
    }
    static __device__ __forceinline__ double get(const Lane& a, int)
    {
        return a;
    }
};

// the two shifted sums D1 = sum (x - K), D2 = sum (x - K)^2, K the channel's first element
struct Moments
{
    static constexpr int N = 2;
    struct Lane
    {
        double d1 = 0.0, d2 = 0.0;
    };
    using Shift = double;
    static __device__ __forceinline__ Shift shift(const float* x, int64_t at)
    {
        return (double) x[at];
    }
    static __device__ __forceinline__ void add(Lane& a, float v, double K)
    {
        const double d = (double) v - K;
        a.d1           = a.d1 + d;
        a.d2           = a.d2 + d * d;
    }
    static __device__ __forceinline__ double get(const Lane& a, int k)
    {
        return k ? a.d2 : a.d1;
    }
};

// where sum k of (split blockIdx.y, channel c) goes
__device__ __forceinline__ int64_t partial_index(int k, int64_t c, int64_t C)
{
    return ((int64_t) k * gridDim.y + blockIdx.y) * C + c;
}

// ---- planar, long segments: workgroup (c, split) takes pieces split, split + nsplit, ... of the
// channel's outer * pieces_per_seg pieces; a piece is piece_len floats of one segment (the last
// piece of a segment shorter).
template <class Acc>
__global__ __launch_bounds__(kReduceBlock) void reduce_planar_vec_kernel(const float* __restrict__ x, int64_t outer,
                                                                         int64_t C, int64_t inner,
                                                                         int64_t pieces_per_seg, int64_t piece_len,
                                                                         double* __restrict__ part)
{
    __shared__ double lds[kReduceBlock];
    const int t                 = threadIdx.x;
    const int64_t c             = blockIdx.x;
    const int64_t npiece        = outer * pieces_per_seg;
    const typename Acc::Shift K = Acc::shift(x, c * inner);
    typename Acc::Lane a0 {}, a1 {}, a2 {}, a3 {};
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
            Acc::add(a0, p[t], K);
        const float4* v  = reinterpret_cast<const float4*>(p + head);
        const int64_t nv = (n - head) >> 2;
#pragma unroll 4
        for (int64_t i = t; i < nv; i += kReduceBlock)
        {
            const float4 f = v[i];
            Acc::add(a0, f.x, K);
            Acc::add(a1, f.y, K);
            Acc::add(a2, f.z, K);
            Acc::add(a3, f.w, K);
        }
        const int64_t rest = head + nv * 4 + t;   // at most three floats
        if (rest < n)
            Acc::add(a1, p[rest], K);
    }
    // every tree, then lane 0's stores in a loop of their own: the spelling that leaves the loops
    // above as they compiled before the two callers shared them (profiles/r18/channel_reduce_isa.txt)
    double s[Acc::N];
    for (int k = 0; k < Acc::N; ++k)
        s[k] = block_sum((Acc::get(a0, k) + Acc::get(a1, k)) + (Acc::get(a2, k) + Acc::get(a3, k)), lds);
    for (int k = 0; k < Acc::N; ++k)
    {
        if (t == 0)
            part[partial_index(k, c, C)] = s[k];
    }
}

// ---- planar, short segments: the channel's outer * inner elements as one flat range, workgroup
// (c, split) takes `chunk` of them; consecutive lanes read consecutive floats of a segment.
template <class Acc>
__global__ __launch_bounds__(kReduceBlock) void reduce_planar_flat_kernel(const float* __restrict__ x, int64_t C,
                                                                          int64_t inner, FastDiv by_inner, int64_t n,
                                                                          int64_t chunk, double* __restrict__ part)
{
    __shared__ double lds[kReduceBlock];
    const int64_t c             = blockIdx.x;
    const int64_t lo            = (int64_t) blockIdx.y * chunk;
    const int64_t hi            = lo + chunk < n ? lo + chunk : n;
    const int64_t stride        = C * inner;
    const float* base           = x + c * inner;
    const typename Acc::Shift K = Acc::shift(x, c * inner);
    typename Acc::Lane a0 {}, a1 {};
    int64_t e = lo + threadIdx.x;
    for (; e + kReduceBlock < hi; e += 2 * kReduceBlock)
    {
        const uint32_t o0 = by_inner.div((uint32_t) e), o1 = by_inner.div((uint32_t) (e + kReduceBlock));
        const float f0 = base[(int64_t) o0 * stride + (e - (int64_t) o0 * inner)];
        const float f1 = base[(int64_t) o1 * stride + (e + kReduceBlock - (int64_t) o1 * inner)];
        Acc::add(a0, f0, K);
        Acc::add(a1, f1, K);
    }
    if (e < hi)
    {
        const uint32_t o0 = by_inner.div((uint32_t) e);
        Acc::add(a0, base[(int64_t) o0 * stride + (e - (int64_t) o0 * inner)], K);
    }
    double s[Acc::N];   // as in reduce_planar_vec_kernel
    for (int k = 0; k < Acc::N; ++k)
        s[k] = block_sum(Acc::get(a0, k) + Acc::get(a1, k), lds);
    for (int k = 0; k < Acc::N; ++k)
    {
        if (threadIdx.x == 0)
            part[partial_index(k, c, C)] = s[k];
    }
}

// ---- interleaved: [rows][C]. The 256 lanes are LY rows x LX column units (a unit is VEC columns);
// workgroup (bx, split) owns column units bx * LX .. and the rows split * rows_per .. ; lane (ty, tx)
// adds the rows ty, ty + LY, ... of its range, then a fixed tree over ty, one sum after the other.
template <class Acc, int VEC>
__global__ __launch_bounds__(kReduceBlock) void reduce_interleaved_kernel(const float* __restrict__ x, int64_t rows,
                                                                          int64_t C, int lx_log2, int64_t rows_per,
                                                                          double* __restrict__ part)
{
    __shared__ double lds[kReduceBlock * VEC];
    const int t = threadIdx.x, LX = 1 << lx_log2, LY = kReduceBlock >> lx_log2;
    const int tx = t & (LX - 1), ty = t >> lx_log2;
    const int64_t unit = (int64_t) blockIdx.x * LX + tx;
    const int64_t col  = unit * VEC;
    const int64_t r0   = (int64_t) blockIdx.y * rows_per;
    const int64_t r1   = r0 + rows_per < rows ? r0 + rows_per : rows;
    typename Acc::Lane a[VEC] = {};
    if (col < C)
    {
        typename Acc::Shift K[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            K[k] = Acc::shift(x, col + k);
#pragma unroll 4
        for (int64_t r = r0 + ty; r < r1; r += LY)
        {
            const float* p = x + r * C + col;
            if (VEC == 4)
            {
                const float4 f = *reinterpret_cast<const float4*>(p);
                Acc::add(a[0], f.x, K[0]);
                Acc::add(a[1 % VEC], f.y, K[1 % VEC]);
                Acc::add(a[2 % VEC], f.z, K[2 % VEC]);
                Acc::add(a[3 % VEC], f.w, K[3 % VEC]);
            }
            else
                Acc::add(a[0], *p, K[0]);
        }
    }
    for (int pass = 0; pass < Acc::N; ++pass)
    {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            lds[k * kReduceBlock + t] = Acc::get(a[k], pass);
        __syncthreads();
        for (int s = LY >> 1; s > 0; s >>= 1)
        {
            if (ty < s)
            {
#pragma unroll
                for (int k = 0; k < VEC; ++k)
                    lds[k * kReduceBlock + t] = lds[k * kReduceBlock + t] + lds[k * kReduceBlock + t + s * LX];
            }
            __syncthreads();
        }
        if (ty == 0 && col < C)
        {
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                part[partial_index(pass, col, C) + k] = lds[k * kReduceBlock + t];
        }
        if (Acc::N > 1)
            __syncthreads();   // the next pass writes lds
    }
}

// ---- host side ---------------------------------------------------------------------------------------
inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

// splits of a channel of n elements when `groups` workgroups exist per split: fill the chip, but
// leave every workgroup kMinPerGroup elements
inline int64_t split_count(int64_t groups, int64_t n, int64_t most)
{
    return clamp64(std::min(ceil_div(kMaxStreamBlocks, groups), ceil_div(n, kMinPerGroup)), 1,
                   std::min<int64_t>(most, 65535));
}

// The sizes every channel reduction takes; `what` opens the caller's error texts.
inline void require_channel_sizes(const std::string& what, int64_t outer, int64_t C, int64_t inner)
{
    AIMET_REQUIRE(outer > 0 && C > 0 && inner > 0, what + ": outer, C and inner must be positive");
    AIMET_REQUIRE(C < (int64_t(1) << 31) && outer < (int64_t(1) << 31) && inner < (int64_t(1) << 31) &&
                      outer * inner < (int64_t(1) << 31) && outer * inner < (int64_t(1) << 46) / C,
                  what + ": too large (2^31 elements per channel, 2^46 in all)");
}

// float tensors on 4-byte, double accumulators on 8-byte boundaries
inline void require_channel_alignment(const std::string& what, std::initializer_list<const float*> tensors,
                                      std::initializer_list<const double*> accumulators)
{
    uintptr_t low = 0;
    for (const float* p : tensors)
        low |= reinterpret_cast<uintptr_t>(p) & 3;
    for (const double* p : accumulators)
        low |= reinterpret_cast<uintptr_t>(p) & 7;
    AIMET_REQUIRE(low == 0, what + ": misaligned pointer");
}

enum class ChannelForm
{
    interleaved,   // inner == 1, a column a unit
    interleaved4,  // inner == 1, four columns a unit: C a multiple of four on a 16-byte base
    planar_vec,    // inner >= kVecInner
    planar_flat
};

// grid (gx, nsplit) and the form's parameters
struct ChannelPlan
{
    ChannelForm form;
    int64_t gx, nsplit;
    int lx_log2            = 0;   // interleaved: LX = 1 << lx_log2 column units across a workgroup
    int64_t rows_per       = 0;   // interleaved: rows of a split
    int64_t pieces_per_seg = 0;   // planar_vec
    int64_t piece_len      = 0;   // planar_vec
    int64_t chunk          = 0;   // planar_flat: elements of a split
};

// The traversal of [outer][C][inner] from its sizes and whether its base is 16-byte aligned.
inline ChannelPlan plan_channel_reduce(bool base16, int64_t outer, int64_t C, int64_t inner)
{
    ChannelPlan p;
    const int64_t n = outer * inner;
    if (inner == 1)
    {
        const int64_t rows  = outer;
        const bool vec      = (C & 3) == 0 && base16;
        const int64_t units = vec ? C / 4 : C;
        while (p.lx_log2 < 8 && (int64_t(1) << p.lx_log2) < units)
            ++p.lx_log2;
        const int64_t LX = int64_t(1) << p.lx_log2, LY = kReduceBlock / LX;
        p.form           = vec ? ChannelForm::interleaved4 : ChannelForm::interleaved;
        p.gx             = ceil_div(units, LX);
        p.nsplit         = split_count(p.gx, rows * LX * (vec ? 4 : 1), ceil_div(rows, LY));
        p.rows_per       = ceil_div(rows, p.nsplit);
        p.nsplit         = ceil_div(rows, p.rows_per);
    }
    else if (inner >= kVecInner)
    {
        const int64_t pieces_per_seg = ceil_div(inner, kPieceFloats);
        p.form                       = ChannelForm::planar_vec;
        p.gx                         = C;
        p.piece_len                  = ceil_div(ceil_div(inner, pieces_per_seg), 4) * 4;
        p.pieces_per_seg             = ceil_div(inner, p.piece_len);
        p.nsplit                     = split_count(C, n, outer * p.pieces_per_seg);
    }
    else
    {
        p.form   = ChannelForm::planar_flat;
        p.gx     = C;
        p.nsplit = split_count(C, n, ceil_div(n, kReduceBlock));
        p.chunk  = ceil_div(ceil_div(n, p.nsplit), kReduceBlock) * kReduceBlock;
        p.nsplit = ceil_div(n, p.chunk);
    }
    return p;
}

struct ChannelPartials
{
    Scratch<double> part;   // Acc::N * nsplit * C doubles, released on s when the caller has folded them
    int64_t nsplit;
};

// One launch on s: the partials of Acc over x. The caller checks the launch.
template <class Acc>
ChannelPartials launch_channel_reduce(const float* x, int64_t outer, int64_t C, int64_t inner, hipStream_t s)
{
    const ChannelPlan p = plan_channel_reduce((reinterpret_cast<uintptr_t>(x) & 15) == 0, outer, C, inner);
    Scratch<double> owner((size_t) (Acc::N * p.nsplit * C), s);
    double* part = owner.get();
    const dim3 grid((unsigned) p.gx, (unsigned) p.nsplit);
    switch (p.form)
    {
    case ChannelForm::interleaved4:
        reduce_interleaved_kernel<Acc, 4><<<grid, kReduceBlock, 0, s>>>(x, outer, C, p.lx_log2, p.rows_per, part);
        break;
    case ChannelForm::interleaved:
        reduce_interleaved_kernel<Acc, 1><<<grid, kReduceBlock, 0, s>>>(x, outer, C, p.lx_log2, p.rows_per, part);
        break;
    case ChannelForm::planar_vec:
        reduce_planar_vec_kernel<Acc><<<grid, kReduceBlock, 0, s>>>(x, outer, C, inner, p.pieces_per_seg, p.piece_len,
                                                                    part);
        break;
    case ChannelForm::planar_flat:
        reduce_planar_flat_kernel<Acc><<<grid, kReduceBlock, 0, s>>>(x, C, inner, FastDiv((uint32_t) inner),
                                                                     outer * inner, p.chunk, part);
        break;
    }
    return {std::move(owner), p.nsplit};
}

}   // namespace aimet_amd
