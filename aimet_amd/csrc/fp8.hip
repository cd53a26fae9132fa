// fp8.hip -- FP8 fake-quantization (aimet_torch/fp_quantization.py) for gfx950: the streaming
// quantize-dequantize, the scale table it reads, and the fused 111-candidate MSE range search.
//
// Reference: fake_cast_to_ieee_float, about a dozen elementwise torch kernels per tensor (log2,
// floor, clamp, pow, div, round, mul ...), and init_mse, which runs that chain 111 times over the
// tensor per calibration batch (per channel: after a Python loop over the channels).
//
// The format: M mantissa bits, E = 7 - M exponent bits, subnormals, no NaN / Inf code, the
// exponent bias following from the tensor's (channel's) maxval. With F = (2 - 2^-M) * 2^(2^E - 1)
// the largest value of the bias-0 format and alpha = float32(double(maxval) / F), the reference's
// bias is -log2(alpha) and its chain approximates, per element,
//     xc = clamp(x, -maxval, maxval)      q = xc / alpha           (IEEE float32 divide)
//     g  = q rounded to M fraction bits at exponent max(floor(log2|q|), 1), ties to even, |g| <= F
//     out = float32(g * alpha)
// which is what fp8_cast computes, from the float's bits (no log2 / pow), so that a numpy oracle
// follows it bit for bit ("FP8"). maxval <= 0 or not finite, or an alpha that rounds
// to 0: out = xc (the reference produces NaN there).
//
// MI355X design:
//   * scale_table: {maxval, alpha} per channel from maxvals in HBM, one small launch, nothing read
//     back: a forward stays capturable in a HIP graph.
//   * qdq: HBM-bound, 8 B/element, two ops (Fp8Tensor, Fp8Channel) on the streaming skeleton of
//     stream_map.hpp at one wave per workgroup; the channel's pair is fetched once per vector
//     (K % 4 == 0).
//   * search: ALU-bound (111 casts per element read). A single-wave workgroup owns a run of
//     1024-element tiles of one [outer][C] row; a lane keeps 16 elements of the tile in registers
//     while the 111 candidates go by, so four partial sums are live at a time (not 111) and the
//     candidate's three scalars are fetched once per 1024 casts. Each candidate's tile sum is a
//     wave butterfly, kept by lane (candidate mod 64). Per-workgroup partials go to a workspace; a second pass adds
//     them in a fixed order and takes the first minimum: no atomics, the grid depends on the shape
//     alone, results repeat bit for bit. The candidate maxima are torch.linspace's float32 values,
//     built on the device from max|x|.
#include "common.hpp"
#include "stream_map.hpp"

#include <atomic>
#include <cmath>

namespace aimet_amd
{

namespace
{

constexpr int kFp8Lanes   = 64;     // family default of the qdq ops (stream_map.hpp: launch_stream)
constexpr int kCand       = 111;    // init_mse: linspace(0.1 * mx, 1.2 * mx, 111)
constexpr int kSearchElems = 16;    // elements a lane holds while the candidates go by (4, 8 or 16)
constexpr int kSearchTile = 64 * 16;    // the unit of the grid's plan, whatever a lane holds
constexpr int64_t kSearchBlocks = 16384;   // target workgroups of a search launch

struct Fp8Format
{
    float F;          // largest value of the bias-0 format
    uint32_t down;    // bits of 2^(M - e) are down - (biased exponent field of 2^e)
    uint32_t up;      // bits of 2^(e - M) are (biased exponent field of 2^e) - up
};

inline double fp8_largest(int M)
{
    const int E = 7 - M;
    return (2.0 - std::ldexp(1.0, -M)) * std::ldexp(1.0, (1 << E) - 1);
}

inline Fp8Format fp8_format(int M)
{
    return Fp8Format {(float) fp8_largest(M), (uint32_t) (254 + M) << 23, (uint32_t) M << 23};
}

// clamp(x, -maxval, maxval): NaN passes, a NaN maxval clamps nothing
__device__ __forceinline__ float fp8_clamp(float x, float maxval)
{
    return x > maxval ? maxval : (x < -maxval ? -maxval : x);
}

// |q| rounded to M fraction bits at exponent e = max(floor(log2|q|), 1), ties to even, at most F.
// 2^(M - e) and 2^(e - M) come from the exponent field, both products are exact, rint is the
// only rounding. NaN stays NaN.
__device__ __forceinline__ float fp8_grid(float aq, const Fp8Format& f)
{
    uint32_t eb = __float_as_uint(aq) & 0x7f800000u;
    eb          = eb < (128u << 23) ? (128u << 23) : eb;
    const float r = __builtin_rintf(aq * __uint_as_float(f.down - eb));
    const float g = r * __uint_as_float(eb - f.up);
    return g > f.F ? f.F : g;
}

// the one cast everything below shares
__device__ __forceinline__ float fp8_cast(float x, float maxval, float alpha, const Fp8Format& f)
{
    const float xc = fp8_clamp(x, maxval);
    if (alpha == 0.0f)
        return xc;
    const float q = xc / alpha;
    return __builtin_copysignf(fp8_grid(__builtin_fabsf(q), f), q) * alpha;
}

// alpha of a maxval; 0 marks "no grid" (maxval <= 0, NaN, Inf, or an alpha below the subnormals)
__device__ __forceinline__ float fp8_alpha(float maxval, double F)
{
    if (!(maxval > 0.0f) || maxval > 3.4028234663852886e38f)
        return 0.0f;
    return (float) ((double) maxval / F);
}

__global__ __launch_bounds__(kBlock) void fp8_scale_table_kernel(const float* __restrict__ maxval, int64_t C, double F,
                                                                 float* __restrict__ table)
{
    const int64_t c = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (c >= C)
        return;
    const float mv   = maxval[c];
    table[2 * c]     = mv;
    table[2 * c + 1] = fp8_alpha(mv, F);
}

// ---------------------------------------------------------------------------------------------
// streaming QDQ
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f4 fp8_cast4(f4 v, float mv, float alpha, const Fp8Format& f)
{
    f4 r;
    r.x = fp8_cast(v.x, mv, alpha, f);
    r.y = fp8_cast(v.y, mv, alpha, f);
    r.z = fp8_cast(v.z, mv, alpha, f);
    r.w = fp8_cast(v.w, mv, alpha, f);
    return r;
}

// per-tensor (C == 1): table = {maxval, alpha}
struct Fp8Tensor
{
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = 4;
    const float* __restrict__ in;
    float* __restrict__ out;
    const float* __restrict__ table;
    Fp8Format f;
    __device__ __forceinline__ void vec(int64_t i) const
    {
        const f4 v = load_stream(reinterpret_cast<const f4*>(in) + i);
        store_stream(fp8_cast4(v, table[0], table[1], f), reinterpret_cast<f4*>(out) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        out[i] = fp8_cast(in[i], table[0], table[1], f);
    }
};

// vector form: K % 4 == 0 (a 16-B vector never straddles two channels), n < 2^31; scalar form:
// int64, any K and alignment
struct Fp8Channel
{
    using index_t      = uint32_t;
    using tail_index_t = int64_t;
    static constexpr int width = 4;
    const float* __restrict__ in;
    float* __restrict__ out;
    ChannelMap map;
    int64_t C, K;
    const float* __restrict__ table;
    Fp8Format f;
    __device__ __forceinline__ void vec(uint32_t i) const
    {
        const f4 v     = load_stream(reinterpret_cast<const f4*>(in) + i);
        const float2 p = reinterpret_cast<const float2*>(table)[map.channel(i * 4)];
        store_stream(fp8_cast4(v, p.x, p.y, f), reinterpret_cast<f4*>(out) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        independent_of(out, in, table);
        const int64_t c = (i / K) % C;
        out[i]          = fp8_cast(in[i], table[2 * c], table[2 * c + 1], f);
    }
};

// ---------------------------------------------------------------------------------------------
// range search
// ---------------------------------------------------------------------------------------------
// How [outer][C][K] is cut into workgroups; the workspace query and every launch share it, so it
// depends on the sizes alone.
struct SearchPlan
{
    int64_t rows;     // outer * C
    int64_t S;        // workgroups per row
    int64_t per;      // tiles per workgroup
    int64_t P;        // partials per channel: outer * S
};

SearchPlan search_plan(int64_t outer, int64_t C, int64_t K)
{
    SearchPlan p;
    p.rows = outer * C;
    const int64_t tiles = ceil_div(K, kSearchTile);
    int64_t S = std::max<int64_t>(1, std::min(tiles, kSearchBlocks / std::max<int64_t>(1, p.rows)));
    p.per     = std::max<int64_t>(1, ceil_div(tiles, S));
    p.S       = std::max<int64_t>(1, ceil_div(tiles, p.per));
    p.P       = outer * p.S;
    return p;
}

void check_search_shape(int64_t outer, int64_t C, int64_t K)
{
    AIMET_REQUIRE(outer > 0 && C > 0 && K > 0, "invalid per-channel shape");
    AIMET_REQUIRE(outer < (int64_t(1) << 31) && C < (int64_t(1) << 31) && K < (int64_t(1) << 40) &&
                      outer * C < (int64_t(1) << 31),
                  "range search: shape too large");
    const SearchPlan p = search_plan(outer, C, K);
    AIMET_REQUIRE(p.rows * p.S < (int64_t(1) << 31), "range search: too many workgroups");
}

__device__ __forceinline__ float wave_max_all(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = __builtin_fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// every lane gets the same sum: each butterfly step adds the same two values on both sides
__device__ __forceinline__ float wave_sum_all(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// workgroup b -> row (o, c) and its run of tiles [e0, e1) of the row's K elements
struct SearchBlock
{
    int64_t o, c, s, e0, e1;
    __device__ __forceinline__ SearchBlock(int64_t C, int64_t K, int64_t S, int64_t per)
    {
        const int64_t b = blockIdx.x;
        const int64_t r = b / S;
        s               = b - r * S;
        o               = r / C;
        c               = r - o * C;
        e0              = s * per * kSearchTile;
        e1              = e0 + per * kSearchTile < K ? e0 + per * kSearchTile : K;
    }
};

// part[c * P + o * S + s] = max|x| of the workgroup's elements (NaN ignored)
__global__ __launch_bounds__(64) void fp8_absmax_part_kernel(const float* __restrict__ in, int64_t C, int64_t K,
                                                             int64_t S, int64_t per, int64_t P,
                                                             float* __restrict__ part)
{
    const SearchBlock b(C, K, S, per);
    const float* row = in + (b.o * C + b.c) * K;
    float m          = 0.0f;
    for (int64_t e = b.e0 + threadIdx.x; e < b.e1; e += 64)
        m = __builtin_fmaxf(m, __builtin_fabsf(row[e]));
    m = wave_max_all(m);
    if (threadIdx.x == 0)
        part[b.c * P + b.o * S + b.s] = m;
}

// one workgroup per channel; max is the same in any order
__global__ __launch_bounds__(kBlock) void fp8_absmax_fold_kernel(const float* __restrict__ part, int64_t P,
                                                                 float* __restrict__ absmax)
{
    __shared__ float s_m[kBlock / 64];
    const int64_t c = blockIdx.x;
    float m = 0.0f;
    for (int64_t p = threadIdx.x; p < P; p += kBlock)
        m = __builtin_fmaxf(m, part[c * P + p]);
    m = wave_max_all(m);
    if ((threadIdx.x & 63) == 0)
        s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w)
            m = __builtin_fmaxf(m, s_m[w]);
        absmax[c] = m;
    }
}

// candidate i of a channel whose max|x| is mx: torch.linspace(0.1 * mx.item(), 1.2 * mx.item(), 111)
// in CPU float32 -- the ends rounded from double, the step an IEEE divide, each half of the table
// one fused multiply-add from its own end
__device__ __forceinline__ float fp8_candidate(float mx, int i)
{
    const float start = (float) (0.1 * (double) mx);
    const float end   = (float) (1.2 * (double) mx);
    const float step  = (end - start) / (float) (kCand - 1);
    return i < kCand / 2 ? __builtin_fmaf(step, (float) i, start) : __builtin_fmaf(-step, (float) (kCand - 1 - i), end);
}

// part[(c * P + o * S + s) * 111 + i] = sum over the workgroup's elements of (x - cast_i(x))^2.
// The error is computed on |x| (the cast is odd, so (x - out)^2 = (|x| - |out|)^2 exactly).
// RCP: q = xc * RN(1 / alpha) instead of the divide; it moves only elements at a rounding tie,
// where both neighbours are equally far.
template <bool RCP, int ELEMS>
__global__ __launch_bounds__(64) void fp8_search_part_kernel(const float* __restrict__ in, int64_t C, int64_t K,
                                                             int64_t S, int64_t per, int64_t P,
                                                             const float* __restrict__ absmax, Fp8Format f, double F,
                                                             float* __restrict__ part, float* __restrict__ cands)
{
    __shared__ float s_mv[kCand], s_alpha[kCand], s_rcp[kCand];
    const SearchBlock b(C, K, S, per);
    const int lane = threadIdx.x;
    const float mx = absmax[b.c];
    for (int i = lane; i < kCand; i += 64)
    {
        const float mv = fp8_candidate(mx, i);
        const float al = fp8_alpha(mv, F);
        s_mv[i]        = mv;
        s_alpha[i]     = al;
        s_rcp[i]       = 1.0f / al;
        if (cands && b.o == 0 && b.s == 0)
            cands[(int64_t) i * C + b.c] = mv;
    }
    __syncthreads();
    const float* row = in + (b.o * C + b.c) * K;
    float tot0 = 0.0f, tot1 = 0.0f;   // lane l: candidates l and 64 + l
    for (int64_t t0 = b.e0; t0 < b.e1; t0 += 64 * ELEMS)
    {
        float ax[ELEMS];
        const int64_t left = b.e1 - t0;
        const int nj       = (int) (left < 64 * ELEMS ? (left + 63) / 64 : ELEMS);
#pragma unroll
        for (int j = 0; j < ELEMS; ++j)
        {
            const int64_t e = t0 + j * 64 + lane;
            ax[j]           = e < b.e1 ? __builtin_fabsf(row[e]) : 0.0f;   // 0 casts to 0: no error
        }
        for (int i = 0; i < kCand; ++i)
        {
            const float mv = s_mv[i], al = s_alpha[i], rc = s_rcp[i];
            // four independent partial sums over groups of four held elements; a group past the
            // tile's end is skipped (uniform), a slot past it holds 0 and adds exactly 0
            float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const bool grid = al != 0.0f;   // uniform
#pragma unroll
            for (int j4 = 0; j4 < ELEMS / 4; ++j4)
                if (j4 * 4 < nj)
                {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                    {
                        const float x  = ax[j4 * 4 + k];
                        const float xc = x > mv ? mv : x;
                        const float o  = grid ? fp8_grid(RCP ? xc * rc : xc / al, f) * al : xc;
                        const float d  = x - o;
                        a4[k]          = __builtin_fmaf(d, d, a4[k]);
                    }
                }
            const float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
            const float s = wave_sum_all(acc);
            if (lane == (i & 63))
            {
                if (i < 64)
                    tot0 += s;
                else
                    tot1 += s;
            }
        }
    }
    float* dst      = part + (b.c * P + b.o * S + b.s) * kCand;
    dst[lane]       = tot0;
    if (64 + lane < kCand)
        dst[64 + lane] = tot1;
}

// One workgroup per channel. The P partials are cut into kFoldGroups runs; a lane adds one
// candidate's partials of one run in order (four loads in flight), the runs are added in order,
// then the first wave takes the first minimum. A fixed order throughout: equal inputs, equal bits.
constexpr int kFoldGroups = 8;
constexpr int kFoldLanes  = 128;   // lanes of a run, one per candidate (111 used)

__global__ __launch_bounds__(kFoldGroups* kFoldLanes) void fp8_search_fold_kernel(
    const float* __restrict__ part, int64_t C, int64_t P, const float* __restrict__ absmax, float* __restrict__ best,
    float* __restrict__ losses, int32_t* __restrict__ best_index)
{
    __shared__ float s_sum[kFoldGroups][kFoldLanes];
    const int64_t c = blockIdx.x;
    {
        const int i = threadIdx.x & (kFoldLanes - 1), g = threadIdx.x / kFoldLanes;
        const int64_t per = (P + kFoldGroups - 1) / kFoldGroups;
        const int64_t p0 = g * per, p1 = p0 + per < P ? p0 + per : P;
        float s = 0.0f;
        if (i < kCand)
        {
            const float* src = part + c * P * kCand + i;
            int64_t p = p0;
            for (; p + 4 <= p1; p += 4)
            {
                const float a = src[p * kCand], b = src[(p + 1) * kCand], d = src[(p + 2) * kCand],
                            e = src[(p + 3) * kCand];
                s += a;
                s += b;
                s += d;
                s += e;
            }
            for (; p < p1; ++p)
                s += src[p * kCand];
        }
        s_sum[g][i] = s;
    }
    __syncthreads();
    if (threadIdx.x >= 64)
        return;
    const int lane  = threadIdx.x;
    const float inf = __builtin_inff();
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
    {
        const int i = h * 64 + lane;
        float s     = s_sum[0][i];
#pragma unroll
        for (int g = 1; g < kFoldGroups; ++g)
            s += s_sum[g][i];
        if (i < kCand && losses)
            losses[c * kCand + i] = s;
        v[h] = i < kCand ? s : inf;
    }
    // argmin as torch's: the first index of the least value; a NaN loss is the least of all
    float bv = v[0];
    int bi   = lane;
    if (v[1] != v[1] ? bv == bv : v[1] < bv)
    {
        bv = v[1];
        bi = 64 + lane;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi   = __shfl_xor(bi, off, 64);
        const bool bn = bv != bv, on = ov != ov;
        const bool take = (on && !bn) || (on == bn && (ov < bv || ((ov == bv || on) && oi < bi)));
        if (take)
        {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0)
    {
        best[c] = fp8_candidate(absmax[c], bi);
        if (best_index)
            best_index[c] = bi;
    }
}

std::atomic<int> g_search_elems {0};   // aimet_fp8_search_elems; 0: kSearchElems

Fp8Format checked_format(int M)
{
    AIMET_REQUIRE(M >= 1 && M <= 6, "FP8 mantissa bits must be in 1..6");
    return fp8_format(M);
}

}   // namespace

}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_fp8_scale_table(const float* maxval_dev, int64_t C, int mantissa_bits, float* table_dev, void* stream)
{
    return guarded([&] {
        checked_format(mantissa_bits);
        AIMET_REQUIRE(C > 0, "FP8 scale table needs at least one maxval");
        require_device_ptr(maxval_dev, "maxval");
        require_device_ptr(table_dev, "table");
        fp8_scale_table_kernel<<<tile_grid(C, kBlock), kBlock, 0, as_stream(stream)>>>(
            maxval_dev, C, fp8_largest(mantissa_bits), table_dev);
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_fp8_qdq(const float* in, float* out, int64_t outer, int64_t C, int64_t K, const float* table_dev,
                  int mantissa_bits, void* stream)
{
    return guarded([&] {
        const Fp8Format f = checked_format(mantissa_bits);
        AIMET_REQUIRE(outer >= 0 && C > 0 && K >= 0, "invalid per-channel shape");
        const int64_t n = outer * C * K;
        if (n == 0)
            return;
        require_device_ptr(in, "input");
        require_device_ptr(out, "output");
        require_device_ptr(table_dev, "table");
        hipStream_t s = as_stream(stream);
        if (C == 1)
            launch_stream<kFp8Lanes>(Fp8Tensor {in, out, table_dev, f}, n, aligned16(in, out), s);
        else
            launch_stream<kFp8Lanes>(Fp8Channel {in, out, ChannelMap(C, K), C, K, table_dev, f}, n,
                                     n < (int64_t(1) << 31) && K % 4 == 0 && aligned16(in, out), s);
    });
}

int aimet_fp8_search_workspace(int64_t outer, int64_t C, int64_t K, int64_t* bytes)
{
    return guarded([&] {
        AIMET_REQUIRE(bytes != nullptr, "bytes is null");
        check_search_shape(outer, C, K);
        const SearchPlan p = search_plan(outer, C, K);
        *bytes             = (int64_t) sizeof(float) * C * p.P * kCand;
    });
}

int aimet_fp8_absmax(const float* in, int64_t outer, int64_t C, int64_t K, float* absmax_dev, void* workspace,
                     int64_t workspace_bytes, void* stream)
{
    return guarded([&] {
        check_search_shape(outer, C, K);
        const SearchPlan p = search_plan(outer, C, K);
        AIMET_REQUIRE(workspace_bytes >= (int64_t) sizeof(float) * C * p.P, "workspace too small");
        require_device_ptr(in, "input");
        require_device_ptr(absmax_dev, "absmax");
        require_device_ptr(workspace, "workspace");
        hipStream_t s = as_stream(stream);
        float* part   = static_cast<float*>(workspace);
        fp8_absmax_part_kernel<<<(unsigned) (p.rows * p.S), 64, 0, s>>>(in, C, K, p.S, p.per, p.P, part);
        AIMET_LAUNCH_CHECK();
        fp8_absmax_fold_kernel<<<(unsigned) C, kBlock, 0, s>>>(part, p.P, absmax_dev);
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_fp8_search_elems(int elems, int* previous)
{
    return guarded([&] {
        AIMET_REQUIRE(elems == 0 || elems == 4 || elems == 8 || elems == 16, "search elements: 0, 4, 8 or 16");
        const int prev = g_search_elems.exchange(elems, std::memory_order_relaxed);
        if (previous)
            *previous = prev;
    });
}

int aimet_fp8_mse_search(const float* in, int64_t outer, int64_t C, int64_t K, const float* absmax_dev,
                         int mantissa_bits, int exact_divide, float* best_maxval_dev, float* losses_dev,
                         float* candidates_dev, int32_t* best_index_dev, void* workspace, int64_t workspace_bytes,
                         void* stream)
{
    return guarded([&] {
        const Fp8Format f = checked_format(mantissa_bits);
        check_search_shape(outer, C, K);
        const SearchPlan p = search_plan(outer, C, K);
        AIMET_REQUIRE(workspace_bytes >= (int64_t) sizeof(float) * C * p.P * kCand, "workspace too small");
        require_device_ptr(in, "input");
        require_device_ptr(absmax_dev, "absmax");
        require_device_ptr(best_maxval_dev, "best maxval");
        require_device_ptr(workspace, "workspace");
        if (losses_dev)
            require_device_ptr(losses_dev, "losses");
        if (candidates_dev)
            require_device_ptr(candidates_dev, "candidates");
        if (best_index_dev)
            require_device_ptr(best_index_dev, "best index");
        hipStream_t s  = as_stream(stream);
        float* part    = static_cast<float*>(workspace);
        const double F = fp8_largest(mantissa_bits);
        const unsigned blocks = (unsigned) (p.rows * p.S);
        auto launch = [&](auto rcp, auto elems) {
            fp8_search_part_kernel<decltype(rcp)::value, decltype(elems)::value><<<blocks, 64, 0, s>>>(
                in, C, K, p.S, p.per, p.P, absmax_dev, f, F, part, candidates_dev);
        };
        auto with_elems = [&](auto rcp) {
            const int forced = g_search_elems.load(std::memory_order_relaxed);
            switch (forced ? forced : kSearchElems)
            {
            case 4: launch(rcp, std::integral_constant<int, 4> {}); break;
            case 8: launch(rcp, std::integral_constant<int, 8> {}); break;
            default: launch(rcp, std::integral_constant<int, 16> {}); break;
            }
        };
        if (exact_divide)
            with_elems(std::false_type {});
        else
            with_elems(std::true_type {});
        AIMET_LAUNCH_CHECK();
        fp8_search_fold_kernel<<<(unsigned) C, kFoldGroups * kFoldLanes, 0, s>>>(
            part, C, p.P, absmax_dev, best_maxval_dev, losses_dev, best_index_dev);
        AIMET_LAUNCH_CHECK();
    });
}

}   // extern "C"
