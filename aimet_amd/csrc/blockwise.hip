// blockwise.hip -- blockwise and LPBQ weight quantization in ONE launch: per-block min / max, the
// block encodings, the optional LPBQ scale compression and the optional quantize-dequantize of a
// weight viewed as [R][NB][BL] (R output channels, NB blocks a row, BL contiguous elements a block).
//
// Reference: the blockwise QcQuantizeOp (aimet_onnx/qc_quantize_op.py:139-160: one TF analyzer per
// block, TfEncodingAnalyzer.cpp:80-101 + getComputedEncodings), lpbq_utils.py:65-146
// (grouped_dynamic_quantize, compress_encoding_scales over one output row) and
// quantizeDequantizeBroadcast (trim_functions.cpp:633-687). There it is a host loop over one
// analyzer and one encoding object a block; here the encodings never leave the device.
//
// Per row r and block b (e = r NB + b, E = R NB), float32 compares, double encoding math:
//   mn, mx      = min / max of the block's BL elements (16-bit inputs upcast; exact in any order)
//   enc         = mse::tf_encoding(mn, mx, bw, sym, strict, unsign)       mse_core.hpp, as the host
//   LPBQ (scale_bitwidth s > 0): factor_r = max_b delta / 2^s,  q = clip(rint(delta / factor_r), 1, 2^s),
//                 delta = q factor_r,  min = delta offset,  max = (2^bw - 1 + offset) delta
//                 (lpbq.py: grouped_dynamic_quantize, scale_offset_arrays_to_encodings)
//   table[k][e] = (float) {min, max, delta, offset}[k]                    the [4][E] per-channel layout
//   out         = dequantize(quantize_nearest(x)) of common.hpp with the table's floats, 16-bit
//                 outputs rounded once (qdq16.hip's convention)
//
// Work split. A row is one work unit (LPBQ reduces over the row's blocks). A block is covered by a
// segment of SEG lanes, SEG a power of two between the elements of a 16-B vector and 64, that load
// 16 B each: lane s of the segment takes vectors s, s + SEG, ... of the block's 16-byte aligned
// body (NP passes), and the scalar elements before and after that body (a row or a block that does
// not start on 16 bytes). The segment folds its min / max with xor shuffles; one lane a block then
// computes the encoding. The row stays on chip between the min / max phase and the QDQ phase, in
// its I/O width:
//   wave path   one 64-lane wave a row, 64 / SEG blocks at a time, the row in registers: at most
//               kWaveMaxVec 16-B vectors a lane (32 VGPRs; instantiated for 1, 2, 4, 8) plus one
//               head and one tail element a vector slot. Needs in and out congruent mod 16.
//   group path  one 256-thread workgroup a row, 256 / SEG blocks at a time, the row in LDS at an
//               offset congruent to its global address (aligned 16-B LDS accesses).
//   two-pass    the group path for a row that does not fit in LDS: the QDQ phase reads the row a
//               second time (each lane the elements it writes, so in place stays safe).
// Per block 32 B of LDS hold {min, max}, the double delta and the float table column; rows of more
// than kMaxBlocks blocks are refused. Rows are taken in a grid-stride loop with 64-bit offsets.
#include "common.hpp"
#include "io16.hpp"
#include "mse_core.hpp"
#include "reduce.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kBlk        = 256;
constexpr int kWave       = 64;
constexpr int kWaveMaxVec = 8;       // 16-B vectors a lane holds on the wave path
constexpr int kMaxBlocks  = AIMET_BQ_MAX_BLOCKS;
constexpr int kMetaBytes  = 32;      // LDS per block: float4 table column, double delta, float2 min / max
constexpr int kLdsBytes   = 65536;
constexpr unsigned kMaxGrid = 1u << 16;

static_assert(kMaxBlocks * kMetaBytes + 64 < kLdsBytes, "a row's block table must fit LDS");

LaunchCounter g_launches;

struct Args
{
    const void* in;
    void* out;        // null: no QDQ
    float* table;     // [4][E]
    int32_t* q;       // [E], LPBQ
    double* factor;   // [R], LPBQ
    int64_t R, L;     // rows, elements a row (NB BL)
    int NB, BL;
    int seg, seg_log2, np;   // lanes a block, passes a block
    int bw, sym, strict, unsign, sbw;
};

struct Meta
{
    float4* prm;   // the block's table column
    double* dl;    // its uncompressed delta (LPBQ)
    float2* mm;    // its min / max
};

__device__ __forceinline__ Meta meta_at(void* base, int NB)
{
    Meta m;
    m.prm = static_cast<float4*>(base);
    m.dl  = reinterpret_cast<double*>(m.prm + NB);
    m.mm  = reinterpret_cast<float2*>(m.dl + NB);
    return m;
}

struct MinMax
{
    float mn, mx;
    __device__ __forceinline__ void reset()
    {
        mn = __builtin_huge_valf();
        mx = -__builtin_huge_valf();
    }
    __device__ __forceinline__ void take(float x)
    {
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
    // every lane of an aligned group of `seg` lanes ends with the group's min / max
    __device__ __forceinline__ void fold(int seg)
    {
        *this = wave_all(*this, [](const MinMax& m, const MinMax& o) {
            return MinMax {o.mn < m.mn ? o.mn : m.mn, o.mx > m.mx ? o.mx : m.mx};
        }, seg);
    }
};

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int IO>
__device__ __forceinline__ typename Io<IO>::elem_t qdq_elem(typename Io<IO>::elem_t x, const QdqParams& p)
{
    return Io<IO>::store(dequantize(quantize_nearest(Io<IO>::load(x), p), p));
}

template <int IO>
__device__ __forceinline__ typename Io<IO>::vec_t qdq_vec(typename Io<IO>::vec_t v, const QdqParams& p)
{
#pragma unroll
    for (int k = 0; k < Io<IO>::width; ++k)
        v[k] = qdq_elem<IO>(v[k], p);
    return v;
}

template <int IO>
__device__ __forceinline__ void take_vec(MinMax& m, typename Io<IO>::vec_t v)
{
#pragma unroll
    for (int k = 0; k < Io<IO>::width; ++k)
        m.take(Io<IO>::load(v[k]));
}

__device__ __forceinline__ QdqParams params_of(const float4& c)
{
    return QdqParams {c.x, c.y, c.z, c.w};
}

__device__ __forceinline__ void put(const Args& a, const Meta& m, int64_t E, int64_t e, int b, double mn, double mx,
                                    double delta, double offset)
{
    const float4 c = make_float4((float) mn, (float) mx, (float) delta, (float) offset);
    m.prm[b]           = c;
    a.table[e]         = c.x;
    a.table[E + e]     = c.y;
    a.table[2 * E + e] = c.z;
    a.table[3 * E + e] = c.w;
}

// The encodings of row r from the min / max in m.mm, by the `N` threads of the unit (a wave, or the
// workgroup when GROUP), thread `tid` taking blocks tid, tid + N, ...; red: 4 doubles (GROUP).
template <bool GROUP>
__device__ __forceinline__ void encode_row(const Args& a, const Meta& m, double* red, int64_t r, int tid)
{
    constexpr int N  = GROUP ? kBlk : kWave;
    const int64_t E  = a.R * a.NB, e0 = r * a.NB;
    const bool lpbq  = a.sbw > 0;
    double dmax      = 0.0;
    for (int b = tid; b < a.NB; b += N)
    {
        const float2 v            = m.mm[b];
        const aimet_tf_encoding e = mse::tf_encoding(v.x, v.y, a.bw, a.sym != 0, a.strict != 0, a.unsign != 0);
        if (lpbq)
        {
            m.dl[b]    = e.delta;
            m.prm[b].w = (float) e.offset;   // an integer of at most bw bits: exact
            dmax       = e.delta > dmax ? e.delta : dmax;
        }
        else
            put(a, m, E, e0 + b, b, e.min, e.max, e.delta, e.offset);
    }
    if (!lpbq)
        return;
    dmax = wave_all(dmax, [](double m, double o) { return o > m ? o : m; });
    if constexpr (GROUP)
    {
        if ((tid & (kWave - 1)) == 0)
            red[tid / kWave] = dmax;
        __syncthreads();
        const double m01 = red[0] > red[1] ? red[0] : red[1], m23 = red[2] > red[3] ? red[2] : red[3];
        dmax             = m01 > m23 ? m01 : m23;
    }
    const double qmax = ldexp(1.0, a.sbw), steps = ldexp(1.0, a.bw) - 1;
    const double factor = dmax / qmax;
    if (tid == 0)
        a.factor[r] = factor;
    for (int b = tid; b < a.NB; b += N)   // the blocks this thread wrote above
    {
        const double off = m.prm[b].w;
        double q         = rint(m.dl[b] / factor);   // half to even, as numpy.round
        q                = q < 1.0 ? 1.0 : (q > qmax ? qmax : q);
        const double d   = q * factor;
        a.q[e0 + b]      = (int32_t) q;
        put(a, m, E, e0 + b, b, d * off, (steps + off) * d, d, off);
    }
}

// ---- wave path: NV vector slots a lane ------------------------------------------------------------
template <int IO, int NV>
__global__ __launch_bounds__(kBlk) void bq_wave(const Args a)
{
    using X   = Io<IO>;
    using T   = typename X::elem_t;
    using Vec = typename X::vec_t;
    constexpr int V = X::width;
    extern __shared__ float4 lds4[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const Meta m   = meta_at(reinterpret_cast<char*>(lds4) + (size_t) wave * a.NB * kMetaBytes, a.NB);
    const int SEG = a.seg, s = lane & (SEG - 1), seg = lane >> a.seg_log2, nseg = kWave >> a.seg_log2;
    const int NP = a.np, BL = a.BL, NB = a.NB;
    constexpr int kRows = kBlk / kWave;
    for (int64_t r = (int64_t) blockIdx.x * kRows + wave; r < a.R; r += (int64_t) gridDim.x * kRows)
    {
        const T* src = static_cast<const T*>(a.in) + r * a.L;
        Vec v[NV];
        T hs[NV], ts[NV];
        // phase 1: the row into registers, the block min / max into LDS
        MinMax mm;
        mm.reset();
        int it = 0, p = 0;
#pragma unroll
        for (int k = 0; k < NV; ++k)
        {
            const int b       = it * nseg + seg;
            const bool active = b < NB;
            const T* bp       = src + (int64_t) (active ? b : 0) * BL;
            const int head = head_of(bp, BL), nvec = (BL - head) / V, tail = head + V * nvec;
            if (p == 0 && active)
            {
                if (s < head)
                {
                    hs[k] = bp[s];
                    mm.take(X::load(hs[k]));
                }
                if (s < BL - tail)
                {
                    ts[k] = bp[tail + s];
                    mm.take(X::load(ts[k]));
                }
            }
            const int vi = p * SEG + s;
            if (active && vi < nvec)
            {
                v[k] = __builtin_nontemporal_load(reinterpret_cast<const Vec*>(bp + head) + vi);
                take_vec<IO>(mm, v[k]);
            }
            if (++p == NP)
            {
                mm.fold(SEG);
                if (s == 0 && active)
                    m.mm[b] = make_float2(mm.mn, mm.mx);
                mm.reset();
                p = 0;
                ++it;
            }
        }
        wave_sync();
        encode_row<false>(a, m, nullptr, r, lane);
        wave_sync();
        // phase 3: QDQ from the registers
        if (a.out)
        {
            T* dst = static_cast<T*>(a.out) + r * a.L;
            it = 0, p = 0;
#pragma unroll
            for (int k = 0; k < NV; ++k)
            {
                const int b       = it * nseg + seg;
                const bool active = b < NB;
                T* bp             = dst + (int64_t) (active ? b : 0) * BL;   // congruent to src mod 16
                const int head = head_of(bp, BL), nvec = (BL - head) / V, tail = head + V * nvec;
                if (active)
                {
                    const QdqParams q = params_of(m.prm[b]);
                    if (p == 0 && s < head)
                        bp[s] = qdq_elem<IO>(hs[k], q);
                    if (p == 0 && s < BL - tail)
                        bp[tail + s] = qdq_elem<IO>(ts[k], q);
                    const int vi = p * SEG + s;
                    if (vi < nvec)
                        __builtin_nontemporal_store(qdq_vec<IO>(v[k], q), reinterpret_cast<Vec*>(bp + head) + vi);
                }
                if (++p == NP)
                    p = 0, ++it;
            }
        }
        wave_sync();   // the block table is read out before the next row overwrites it
    }
}

// ---- group path: the row in LDS (RESIDENT) or read twice -------------------------------------------
template <int IO, bool RESIDENT>
__global__ __launch_bounds__(kBlk) void bq_group(const Args a)
{
    using X   = Io<IO>;
    using T   = typename X::elem_t;
    using Vec = typename X::vec_t;
    constexpr int V = X::width;
    extern __shared__ float4 lds4[];
    const Meta m = meta_at(lds4, a.NB);
    double* red  = reinterpret_cast<double*>(reinterpret_cast<char*>(lds4) + (size_t) a.NB * kMetaBytes);   // 4
    T* rowbuf    = reinterpret_cast<T*>(red + 8);   // 16-byte aligned
    const int t = threadIdx.x;
    const int SEG = a.seg, s = t & (SEG - 1), seg = t >> a.seg_log2, nseg = kBlk >> a.seg_log2;
    const int BL = a.BL, NB = a.NB;
    for (int64_t r = blockIdx.x; r < a.R; r += gridDim.x)
    {
        const T* src = static_cast<const T*>(a.in) + r * a.L;
        // LDS element j of the row sits at row[j], as far from a 16-byte boundary as src[j] is
        T* row = rowbuf + (reinterpret_cast<uintptr_t>(src) & 15u) / sizeof(T);
        for (int b0 = 0; b0 < NB; b0 += nseg)
        {
            const int b       = b0 + seg;
            const bool active = b < NB;
            MinMax mm;
            mm.reset();
            if (active)
            {
                const T* bp    = src + (int64_t) b * BL;
                const int base = b * BL;
                const int head = head_of(bp, BL), nvec = (BL - head) / V, tail = head + V * nvec;
                for (int i = s; i < head; i += SEG)
                {
                    const T x = bp[i];
                    if constexpr (RESIDENT)
                        row[base + i] = x;
                    mm.take(X::load(x));
                }
                for (int vi = s; vi < nvec; vi += SEG)
                {
                    Vec x;
                    if constexpr (RESIDENT)
                    {
                        x = __builtin_nontemporal_load(reinterpret_cast<const Vec*>(bp + head) + vi);
                        *reinterpret_cast<Vec*>(row + base + head + V * vi) = x;
                    }
                    else
                        x = *(reinterpret_cast<const Vec*>(bp + head) + vi);
                    take_vec<IO>(mm, x);
                }
                for (int i = tail + s; i < BL; i += SEG)
                {
                    const T x = bp[i];
                    if constexpr (RESIDENT)
                        row[base + i] = x;
                    mm.take(X::load(x));
                }
            }
            mm.fold(SEG);
            if (s == 0 && active)
                m.mm[b] = make_float2(mm.mn, mm.mx);
        }
        __syncthreads();   // the row and every block's min / max are in LDS
        encode_row<true>(a, m, red, r, t);
        __syncthreads();   // the block table is complete
        if (a.out)
        {
            T* dst = static_cast<T*>(a.out) + r * a.L;
            // the destination's own split; its vectors line up with the source's when the two
            // pointers are congruent mod 16
            const bool congruent = ((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
            for (int b = seg; b < NB; b += nseg)
            {
                const QdqParams q = params_of(m.prm[b]);
                const T* bp       = src + (int64_t) b * BL;
                T* dp             = dst + (int64_t) b * BL;
                const int base    = b * BL;
                auto elem = [&](int i) -> T {
                    if constexpr (RESIDENT)
                        return row[base + i];
                    else
                        return bp[i];
                };
                const int head = head_of(dp, BL), nvec = (BL - head) / V, tail = head + V * nvec;
                for (int i = s; i < head; i += SEG)
                    dp[i] = qdq_elem<IO>(elem(i), q);
                for (int vi = s; vi < nvec; vi += SEG)
                {
                    const int i = head + V * vi;
                    Vec x;
                    if (congruent)
                    {
                        if constexpr (RESIDENT)
                            x = *reinterpret_cast<const Vec*>(row + base + i);
                        else
                            x = *reinterpret_cast<const Vec*>(bp + i);
                    }
                    else
                    {
#pragma unroll
                        for (int k = 0; k < V; ++k)
                            x[k] = elem(i + k);
                    }
                    __builtin_nontemporal_store(qdq_vec<IO>(x, q), reinterpret_cast<Vec*>(dp + i));
                }
                for (int i = tail + s; i < BL; i += SEG)
                    dp[i] = qdq_elem<IO>(elem(i), q);
            }
        }
        __syncthreads();   // row, red and the block table are read out before the next row overwrites them
    }
}

// ---- launch policy ---------------------------------------------------------------------------------
enum Path
{
    PATH_WAVE  = AIMET_BQ_PATH_WAVE,
    PATH_GROUP = AIMET_BQ_PATH_GROUP,
    PATH_TWO   = AIMET_BQ_PATH_TWO_PASS
};

struct Plan
{
    Path path;
    int seg, seg_log2, np, nv;   // nv: vector slots a lane (wave path)
    size_t lds;
};

Plan plan_of(int64_t NB, int64_t BL, int io, bool congruent)
{
    const int V = io == IO_F32 ? 4 : 8, esize = io == IO_F32 ? 4 : 2;
    const int64_t nvec = ceil_div(BL, V);   // an upper bound of the 16-B vectors of a block's body
    Plan p {};
    p.seg = V, p.seg_log2 = io == IO_F32 ? 2 : 3;
    while (p.seg < kWave && p.seg < nvec)
        p.seg <<= 1, ++p.seg_log2;
    p.np = (int) ceil_div(nvec, p.seg);
    // wave path: what a lane must hold, from the code: ceil(NB / (64 / SEG)) block rounds of NP vectors
    const int64_t slots = ceil_div(NB, kWave / p.seg) * p.np;
    const size_t meta   = (size_t) NB * kMetaBytes;
    if (slots <= kWaveMaxVec && congruent)
    {
        p.path = PATH_WAVE;
        p.nv   = 1;
        while (p.nv < slots)
            p.nv <<= 1;
        p.lds = meta * (kBlk / kWave);
        return p;
    }
    p.np             = 0;   // the group path loops over a block's vectors
    const size_t fix = meta + 64;                                  // block table, the four partial maxima
    const size_t row = (size_t) (NB * BL + V) * esize + 16;        // the row at its global misalignment
    p.path           = fix + row <= (size_t) kLdsBytes ? PATH_GROUP : PATH_TWO;
    p.lds            = p.path == PATH_GROUP ? fix + row : fix;
    return p;
}

template <int IO>
void launch(const Args& a, const Plan& p, hipStream_t s)
{
    if (p.path == PATH_WAVE)
    {
        const unsigned grid = (unsigned) std::min<int64_t>(ceil_div(a.R, kBlk / kWave), kMaxGrid);
        switch (p.nv)
        {
        case 1: bq_wave<IO, 1><<<grid, kBlk, p.lds, s>>>(a); break;
        case 2: bq_wave<IO, 2><<<grid, kBlk, p.lds, s>>>(a); break;
        case 4: bq_wave<IO, 4><<<grid, kBlk, p.lds, s>>>(a); break;
        default: bq_wave<IO, 8><<<grid, kBlk, p.lds, s>>>(a); break;
        }
        return;
    }
    const unsigned grid = (unsigned) std::min<int64_t>(a.R, kMaxGrid);
    if (p.path == PATH_GROUP)
        bq_group<IO, true><<<grid, kBlk, p.lds, s>>>(a);
    else
        bq_group<IO, false><<<grid, kBlk, p.lds, s>>>(a);
}

void check_shape(int64_t R, int64_t NB, int64_t BL, int io)
{
    AIMET_REQUIRE(io == IO_F32 || io == IO_F16 || io == IO_BF16,
                  "io_dtype must be 0 (float32), 1 (float16) or 2 (bfloat16)");
    AIMET_REQUIRE(R > 0 && NB > 0 && BL > 0, "blockwise: R, NB and BL must be positive");
    AIMET_REQUIRE(NB <= kMaxBlocks, "blockwise: more than " + std::to_string(kMaxBlocks) + " blocks a row");
    AIMET_REQUIRE(BL < (int64_t(1) << 31) / NB, "blockwise: a row of 2^31 elements or more");
    AIMET_REQUIRE(R < (int64_t(1) << 40) / (NB * BL), "blockwise: tensor too large (R NB BL must stay below 2^40)");
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_bq_encode_qdq(const void* in, void* out, int64_t R, int64_t NB, int64_t BL, int io_dtype, int32_t bw,
                        int use_symmetric, int use_strict_symmetric, int use_unsigned_symmetric, int scale_bitwidth,
                        float* table, int32_t* q, double* factor, void* stream)
{
    return guarded([&] {
        check_shape(R, NB, BL, io_dtype);
        AIMET_REQUIRE(bw >= 1 && bw <= 31, "blockwise: bitwidth must be in [1, 31]");
        AIMET_REQUIRE(scale_bitwidth >= 0 && scale_bitwidth <= 30, "blockwise: scale_bitwidth must be in [0, 30]");
        AIMET_REQUIRE(scale_bitwidth == 0 || use_symmetric, "blockwise: LPBQ (scale_bitwidth > 0) is symmetric only");
        const size_t esize = io_dtype == IO_F32 ? 4 : 2;
        require_device_ptr(in, "input");
        require_device_ptr(table, "table");
        AIMET_REQUIRE((reinterpret_cast<uintptr_t>(in) & (esize - 1)) == 0 &&
                          (reinterpret_cast<uintptr_t>(out) & (esize - 1)) == 0 &&
                          (reinterpret_cast<uintptr_t>(table) & 3) == 0,
                      "blockwise: misaligned pointer");
        if (out)
        {
            require_device_ptr(out, "output");
            const char *i0 = static_cast<const char*>(in), *o0 = static_cast<const char*>(out);
            const int64_t bytes = R * NB * BL * (int64_t) esize;
            AIMET_REQUIRE(o0 == i0 || o0 + bytes <= i0 || i0 + bytes <= o0,
                          "blockwise: the output must be the input or not overlap it");
        }
        if (scale_bitwidth > 0)
        {
            require_device_ptr(q, "per-block integer scales");
            require_device_ptr(factor, "per-channel scales");
            AIMET_REQUIRE((reinterpret_cast<uintptr_t>(q) & 3) == 0 && (reinterpret_cast<uintptr_t>(factor) & 7) == 0,
                          "blockwise: misaligned pointer");
        }
        const bool congruent =
            !out || ((reinterpret_cast<uintptr_t>(in) ^ reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
        const Plan p = plan_of(NB, BL, io_dtype, congruent);
        Args a {};
        a.in = in, a.out = out, a.table = table, a.q = q, a.factor = factor;
        a.R = R, a.L = NB * BL, a.NB = (int) NB, a.BL = (int) BL;
        a.seg = p.seg, a.seg_log2 = p.seg_log2, a.np = p.np;
        a.bw = bw, a.sym = use_symmetric != 0, a.strict = use_strict_symmetric != 0;
        a.unsign = use_unsigned_symmetric != 0, a.sbw = scale_bitwidth;
        hipStream_t s = as_stream(stream);
        if (io_dtype == IO_F32)
            launch<IO_F32>(a, p, s);
        else if (io_dtype == IO_F16)
            launch<IO_F16>(a, p, s);
        else
            launch<IO_BF16>(a, p, s);
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_bq_row_path(int64_t NB, int64_t BL, int io_dtype, int* path)
{
    return guarded([&] {
        AIMET_REQUIRE(path != nullptr, "output is null");
        check_shape(1, NB, BL, io_dtype);
        *path = plan_of(NB, BL, io_dtype, true).path;
    });
}

int aimet_bq_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
