// lg_block.hip -- learned blockwise ranges: the learned-grid (range-learning) forward and backward
// over a contiguous float32 weight viewed as [E][BL], block e with its own trainable range. One
// launch each way, for gfx950.
//
// The arithmetic is lg_core.hpp's, element by element what learned_grid.hip computes on the
// [1, E, BL] view (quantsim_straight_through_grad.py:121-328). What is new is the work split: the
// per-channel kernels give a channel a 256-lane workgroup and fold the range gradients in a second
// launch, which at BL = 64 leaves 240 of 256 lanes idle. Here nothing is larger than a wave.
//
// Work split. A block is covered by a segment of SEG lanes, SEG the power of two from 1 to 64 that
// holds the block's 16-B vectors (nvec = ceil(BL / 4)); lane s of the segment takes vectors s,
// s + SEG, ... (NP passes, more than one only when SEG = 64). A lane holds kSlots = 4 vector slots a
// trip: slot k is pass k % NP of round k / NP, and round r of a wave covers the 64 / SEG consecutive
// blocks base + r (64 / SEG) + segment. So a wave takes bw = (4 / NP) (64 / SEG) consecutive blocks a
// trip -- 16 at BL = 64, 4 KiB of x -- with every load of the trip issued before any arithmetic. The
// waves of the grid (1024 workgroups of 4, one resident round) take consecutive chunks of bw blocks,
// trip after trip, with 64-bit offsets.
//
// One encoding per block, not per lane and slot. A block's delta, offset and reciprocal cost two
// IEEE divisions and a guarded reciprocal (~45 VALU), against ~20 for a lane's four elements. Lane l
// of the wave computes the encoding of block base + l (bw <= 64 whenever SEG >= 4: one evaluation a
// wave and trip instead of one per round; SEG 2 and 1 take NENC = 2 and 4 evaluations for their 128
// and 256 blocks), from coalesced loads of the range, and stores the saved encoding -- coalesced too.
// The segments then fetch {delta, offset, reciprocal} from the computing lane by ds_bpermute.
//
// Backward. The segment's lanes sum {A, B, D} over their slots in pass order, the segment folds them
// with reduce.hpp's xor butterfly over SEG lanes (a fixed order: bit-identical runs), and lane 0 of
// the segment evaluates the range gradients (range_grads_one) and stores grad_min[e], grad_max[e]. No
// sums array, no scratch, no second launch, no atomics.
//
// Element path. A slot is always the four elements 4 vi .. 4 vi + 3 of its block, cut at BL. Where
// BL % 4 != 0 or a pointer is off its vector alignment the same kernels load, compute and store those
// elements one by one: same lanes, same order of every sum, same results.
//
// Built without packed fp32 instructions, like blockwise.hip (the element arithmetic has no use for
// them and the segment fold must stay three scalar adds a step).
#include "common.hpp"
#include "io16.hpp"
#include "lg_core.hpp"
#include "reduce.hpp"
#include "stream_map.hpp"

namespace aimet_amd
{
namespace
{

constexpr int kWave       = 64;
constexpr int kSlots      = 4;                       // 16-B vector slots a lane and trip
constexpr int kWaves      = kBlock / kWave;
constexpr int64_t kGrid   = 1024;                    // workgroups: 4 a CU (the kernels take 70 - 110 VGPRs), one resident round
constexpr int64_t kMaxBL  = AIMET_LG_BLOCK_MAX_BL;   // SEG = 64 lanes x kSlots passes x 4 elements

static_assert(kMaxBL == kWave * kSlots * 4, "a block is at most kSlots passes of a whole wave");

struct BlockShape
{
    int64_t E;
    int BL;
    int seg_log2;   // SEG = 1 << seg_log2 lanes a block
};

// where a lane stands: its segment, its place in it, the wave's first block of the first trip
struct LaneMap
{
    int lane, seg, s, sidx, nseg;
    __device__ __forceinline__ explicit LaneMap(const BlockShape& sh)
    {
        lane = threadIdx.x & (kWave - 1);
        seg  = 1 << sh.seg_log2;
        s    = lane & (seg - 1);
        sidx = lane >> sh.seg_log2;
        nseg = kWave >> sh.seg_log2;
    }
};

// slot k of a lane in the trip that starts at block `base`: its block, its vector in the block, the
// elements of that vector inside the block (4, or fewer at the end of a block whose length is not a
// multiple of 4; 0: nothing to do)
template <int NP>
struct Slot
{
    int64_t b;
    int vi, cnt;
    __device__ __forceinline__ Slot(const BlockShape& sh, const LaneMap& m, int64_t base, int k)
    {
        b              = base + (k / NP) * m.nseg + m.sidx;
        vi             = (k % NP) * m.seg + m.s;
        const int left = b < sh.E ? sh.BL - 4 * vi : 0;
        cnt            = left >= 4 ? 4 : (left > 0 ? left : 0);
    }
};

// The encodings of a wave's bw blocks, NENC a lane (block base + j 64 + lane), and their way to the
// segments. fetch(r) is called by every lane of the wave (ds_bpermute reads no inactive lane).
template <int NENC>
struct WaveEncodings
{
    float d[NENC], o[NENC], rd[NENC];
    // round r's block of this lane's segment: computed by lane (r nseg + sidx) % 64 in evaluation
    // (r nseg + sidx) / 64, which is r NENC / 4 (NENC > 1 means nseg = 16 NENC, four rounds)
    __device__ __forceinline__ void fetch(const LaneMap& m, int r, float& dl, float& of, float& rc) const
    {
        const int j   = NENC == 1 ? 0 : r * NENC / 4;
        const int src = (r * m.nseg + m.sidx) & (kWave - 1);
        dl            = __shfl(d[j], src, kWave);
        of            = __shfl(o[j], src, kWave);
        rc            = __shfl(rd[j], src, kWave);
    }
};

template <int OUT>
__device__ __forceinline__ void store_elem(void* __restrict__ y, int64_t i, float v)
{
    static_cast<typename Io<OUT>::elem_t*>(y)[i] = Io<OUT>::store(v);
}

// ---- forward -----------------------------------------------------------------------------------------
// saved[4][E] = {delta, offset, min, max as read}, written by the lane that computes the encoding
template <int OUT, int NP, int NENC, bool VEC>
__global__ __launch_bounds__(kBlock) void lg_block_fwd_kernel(const float* __restrict__ x, void* __restrict__ y,
                                                              BlockShape sh, LgEnc enc, float* __restrict__ saved)
{
    constexpr int ROUNDS = kSlots / NP;
    const LaneMap m(sh);
    const int bw         = ROUNDS * m.nseg;
    const int64_t stride = (int64_t) gridDim.x * kWaves * bw;
    for (int64_t base = ((int64_t) blockIdx.x * kWaves + (threadIdx.x >> 6)) * bw; base < sh.E; base += stride)
    {
        // the loads of the trip: the ranges first (needed first), then the slots
        float mn[NENC], mx[NENC];
#pragma unroll
        for (int j = 0; j < NENC; ++j)
        {
            const int bi    = j * kWave + m.lane;
            const int64_t b = base + bi;
            const bool own  = bi < bw && b < sh.E;
            mn[j]           = own ? enc.emin[b] : 0.0f;
            mx[j]           = own ? enc.emax[b] : 1.0f;
        }
        float xv[kSlots][4];
#pragma unroll
        for (int k = 0; k < kSlots; ++k)
        {
            const Slot<NP> t(sh, m, base, k);
            const float* p = x + t.b * sh.BL + 4 * t.vi;
            xv[k][0] = xv[k][1] = xv[k][2] = xv[k][3] = 0.0f;
            if constexpr (VEC)
            {
                if (t.cnt)
                {
                    const f4 v = load_stream(reinterpret_cast<const f4*>(p));
                    xv[k][0] = v.x, xv[k][1] = v.y, xv[k][2] = v.z, xv[k][3] = v.w;
                }
            }
            else
            {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < t.cnt)
                        xv[k][i] = p[i];
            }
        }
        WaveEncodings<NENC> we;
#pragma unroll
        for (int j = 0; j < NENC; ++j)
        {
            const int bi    = j * kWave + m.lane;
            const int64_t b = base + bi;
            enc.of(mn[j], mx[j], we.d[j], we.o[j]);
            we.rd[j] = lg_recip(we.d[j]);
            if (bi < bw && b < sh.E)
            {
                saved[b]            = we.d[j];
                saved[sh.E + b]     = we.o[j];
                saved[2 * sh.E + b] = mn[j];
                saved[3 * sh.E + b] = mx[j];
            }
        }
        float d = 0.0f, o = 0.0f, rd = 0.0f;
#pragma unroll
        for (int k = 0; k < kSlots; ++k)
        {
            const Slot<NP> t(sh, m, base, k);
            if (k % NP == 0)
                we.fetch(m, k / NP, d, o, rd);
            float yo[4];
            lg_qdq_n<4>(xv[k], d, o, enc.steps, rd, yo);
            if constexpr (VEC)
            {
                if (t.cnt)
                {
                    const f4 r = {yo[0], yo[1], yo[2], yo[3]};
                    lg_store4<OUT>(static_cast<typename Io<OUT>::elem_t*>(y) + t.b * sh.BL, (uint32_t) t.vi, r);
                }
            }
            else
            {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < t.cnt)
                        store_elem<OUT>(y, t.b * sh.BL + 4 * t.vi + i, yo[i]);
            }
        }
    }
}

// ---- backward ----------------------------------------------------------------------------------------
// MODE: lg_bwd_term's (1 symmetric, 2 asymmetric), a template parameter because the run-time form keeps
// the sums in scratch memory; range: the saved encoding's rows and the outputs
template <int GIO, int NP, int NENC, bool VEC, int MODE>
__global__ __launch_bounds__(kBlock) void lg_block_bwd_kernel(const float* __restrict__ x, const void* __restrict__ g,
                                                              float* __restrict__ gx, BlockShape sh,
                                                              const float* __restrict__ saved, float steps,
                                                              LgRange range)
{
    typedef typename Io<GIO>::elem_t G;
    constexpr int ROUNDS = kSlots / NP;
    const LaneMap m(sh);
    const int bw         = ROUNDS * m.nseg;
    const int64_t stride = (int64_t) gridDim.x * kWaves * bw;
    for (int64_t base = ((int64_t) blockIdx.x * kWaves + (threadIdx.x >> 6)) * bw; base < sh.E; base += stride)
    {
        WaveEncodings<NENC> we;
#pragma unroll
        for (int j = 0; j < NENC; ++j)
        {
            const int bi    = j * kWave + m.lane;
            const int64_t b = base + bi;
            const bool own  = bi < bw && b < sh.E;
            we.d[j]         = own ? saved[b] : 1.0f;
            we.o[j]         = own ? saved[sh.E + b] : 0.0f;
        }
        float xv[kSlots][4], gv[kSlots][4];
#pragma unroll
        for (int k = 0; k < kSlots; ++k)
        {
            const Slot<NP> t(sh, m, base, k);
            const int64_t e0 = t.b * sh.BL + 4 * t.vi;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                xv[k][i] = gv[k][i] = 0.0f;
            if constexpr (VEC)
            {
                if (t.cnt)
                {
                    const f4 a = load_stream(reinterpret_cast<const f4*>(x + e0));
                    const f4 b = load_grad4<GIO>(static_cast<const G*>(g) + t.b * sh.BL, (uint32_t) t.vi);
                    xv[k][0] = a.x, xv[k][1] = a.y, xv[k][2] = a.z, xv[k][3] = a.w;
                    gv[k][0] = b.x, gv[k][1] = b.y, gv[k][2] = b.z, gv[k][3] = b.w;
                }
            }
            else
            {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < t.cnt)
                    {
                        xv[k][i] = x[e0 + i];
                        gv[k][i] = Io<GIO>::load(static_cast<const G*>(g)[e0 + i]);
                    }
            }
        }
#pragma unroll
        for (int j = 0; j < NENC; ++j)
            we.rd[j] = lg_recip(we.d[j]);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
        {
            float dl, o, rcp;
            we.fetch(m, r, dl, o, rcp);
            Sums s {0, 0, 0};
#pragma unroll
            for (int p = 0; p < NP; ++p)
            {
                const int k = r * NP + p;
                const Slot<NP> t(sh, m, base, k);
                float gq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (VEC)
                {
                    if (t.cnt)
                    {
                        lg_bwd_elems<4>(xv[k], gv[k], dl, o, steps, rcp, gq, s, MODE);
                        if (gx)
                        {
                            const f4 rv = {gq[0], gq[1], gq[2], gq[3]};
                            store_stream(rv, reinterpret_cast<f4*>(gx + t.b * sh.BL) + t.vi);
                        }
                    }
                }
                else
                {
                    // lg_bwd_elems<4> is its four elements in order: the same sums one element at a time
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < t.cnt)
                        {
                            lg_bwd_elems<1>(&xv[k][i], &gv[k][i], dl, o, steps, rcp, &gq[i], s, MODE);
                            if (gx)
                                gx[t.b * sh.BL + 4 * t.vi + i] = gq[i];
                        }
                }
            }
            // the block's sums: the segment's lanes in the butterfly's fixed order
            const auto add = [](float a, float b) { return a + b; };
            const float A = wave_all(s.a, add, m.seg), B = wave_all(s.b, add, m.seg), D = wave_all(s.d, add, m.seg);
            const int64_t b = base + r * m.nseg + m.sidx;
            if (m.s == 0 && b < sh.E)
                range_grads_one(A, B, D, (uint32_t) b, range);
        }
    }
}

// ---- launch policy -----------------------------------------------------------------------------------
struct Plan
{
    int seg_log2, np, nenc;
    int64_t per_wave;   // blocks a wave and trip
};

Plan plan_of(int64_t BL)
{
    const int64_t nvec = ceil_div(BL, 4);
    Plan p {};
    while ((int64_t(1) << p.seg_log2) < nvec && p.seg_log2 < 6)
        ++p.seg_log2;
    const int64_t passes = ceil_div(nvec, int64_t(1) << p.seg_log2);   // > 1 only with a whole wave a block
    p.np       = passes <= 1 ? 1 : (passes == 2 ? 2 : kSlots);
    p.nenc     = p.seg_log2 == 0 ? 4 : (p.seg_log2 == 1 ? 2 : 1);
    p.per_wave = (int64_t) (kSlots / p.np) * (kWave >> p.seg_log2);
    return p;
}

unsigned grid_of(int64_t E, const Plan& p)
{
    return (unsigned) std::min(kGrid, ceil_div(E, p.per_wave * kWaves));
}

// f(integral_constant<NP>, integral_constant<NENC>, bool_constant<VEC>) for the five shapes plan_of
// gives, on the vector or the element path
template <class F>
void with_plan(const Plan& p, bool vec, F&& f)
{
    using std::integral_constant;
    const auto shape = [&](auto v) {
        if (p.nenc == 4)
            f(integral_constant<int, 1> {}, integral_constant<int, 4> {}, v);
        else if (p.nenc == 2)
            f(integral_constant<int, 1> {}, integral_constant<int, 2> {}, v);
        else if (p.np == 1)
            f(integral_constant<int, 1> {}, integral_constant<int, 1> {}, v);
        else if (p.np == 2)
            f(integral_constant<int, 2> {}, integral_constant<int, 1> {}, v);
        else
            f(integral_constant<int, 4> {}, integral_constant<int, 1> {}, v);
    };
    if (vec)
        shape(std::true_type {});
    else
        shape(std::false_type {});
}

template <class F>
void with_io(int dtype, F&& f)
{
    if (dtype == IO_F32)
        f(std::integral_constant<int, IO_F32> {});
    else if (dtype == IO_F16)
        f(std::integral_constant<int, IO_F16> {});
    else
        f(std::integral_constant<int, IO_BF16> {});
}

void check_shape(int64_t E, int64_t BL, int dtype, const char* what)
{
    AIMET_REQUIRE(dtype == IO_F32 || dtype == IO_F16 || dtype == IO_BF16,
                  std::string(what) + " must be 0 (float32), 1 (float16) or 2 (bfloat16)");
    AIMET_REQUIRE(E >= 0 && E < (int64_t(1) << 31), "learned blockwise ranges: E must be in [0, 2^31)");
    AIMET_REQUIRE(BL >= 1 && BL <= kMaxBL,
                  "learned blockwise ranges: BL must be in [1, " + std::to_string(kMaxBL) + "]");
}

// a float32 tensor or table, or one of 16-bit values: device memory, aligned to its elements
void check_ptr(const void* p, int dtype, const char* what)
{
    require_device_ptr(p, what);
    AIMET_REQUIRE((reinterpret_cast<uintptr_t>(p) & (dtype == IO_F32 ? 3u : 1u)) == 0,
                  std::string("learned blockwise ranges: misaligned ") + what);
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_lg_block_forward(const float* x, void* y, int64_t E, int64_t BL, int out_dtype, const float* emin,
                           const float* emax, int bw, int sym, int strict, int unsign, float* enc, void* stream)
{
    return guarded([&] {
        check_shape(E, BL, out_dtype, "out_dtype");
        AIMET_REQUIRE(bw > 0 && bw < 32, "invalid bitwidth");
        if (E == 0)
            return;
        check_ptr(x, IO_F32, "x");
        check_ptr(y, out_dtype, "y");
        check_ptr(emin, IO_F32, "encoding_min");
        check_ptr(emax, IO_F32, "encoding_max");
        check_ptr(enc, IO_F32, "enc");
        const LgEnc e = enc_of(emin, emax, E, BL, bw, sym, strict, unsign, enc, enc + E, enc + 2 * E);
        const Plan p  = plan_of(BL);
        const bool y_aligned = out_dtype == IO_F32 ? aligned16(y) : aligned_to<8>(y);
        const bool vec = BL % 4 == 0 && aligned16(x) && y_aligned;
        const BlockShape sh {E, (int) BL, p.seg_log2};
        with_io(out_dtype, [&](auto io) {
            with_plan(p, vec, [&](auto np, auto nenc, auto v) {
                lg_block_fwd_kernel<decltype(io)::value, decltype(np)::value, decltype(nenc)::value, decltype(v)::value>
                    <<<grid_of(E, p), kBlock, 0, as_stream(stream)>>>(x, y, sh, e, enc);
            });
        });
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_lg_block_backward(const float* x, const void* grad, int grad_dtype, float* grad_x, int64_t E, int64_t BL,
                            const float* enc, float num_steps, int mode, float* grad_min, float* grad_max,
                            void* stream)
{
    return guarded([&] {
        check_shape(E, BL, grad_dtype, "grad_dtype");
        AIMET_REQUIRE(mode >= 0 && mode <= 2,
                      "mode must be 0 (symmetric signed), 1 (symmetric unsigned) or 2 (asymmetric)");
        if (E == 0)
            return;
        check_ptr(x, IO_F32, "x");
        check_ptr(grad, grad_dtype, "grad");
        if (grad_x)
            check_ptr(grad_x, IO_F32, "grad_x");
        check_ptr(enc, IO_F32, "enc");
        check_ptr(grad_min, IO_F32, "grad_min");
        check_ptr(grad_max, IO_F32, "grad_max");
        const Plan p = plan_of(BL);
        const bool g_aligned = grad_dtype == IO_F32 ? aligned16(grad) : aligned_to<8>(grad);
        const bool vec = BL % 4 == 0 && aligned16(x, grad_x) && g_aligned;
        const BlockShape sh {E, (int) BL, p.seg_log2};
        const LgRange range {enc + 2 * E, enc + 3 * E, enc, grad_min, grad_max, num_steps,
                             (float) std::floor(num_steps / 2.0), mode != 2};
        with_io(grad_dtype, [&](auto io) {
            with_plan(p, vec, [&](auto np, auto nenc, auto v) {
                constexpr int IO = decltype(io)::value, NP = decltype(np)::value, NENC = decltype(nenc)::value;
                constexpr bool VEC = decltype(v)::value;
                if (mode == 2)
                    lg_block_bwd_kernel<IO, NP, NENC, VEC, 2>
                        <<<grid_of(E, p), kBlock, 0, as_stream(stream)>>>(x, grad, grad_x, sh, enc, num_steps, range);
                else
                    lg_block_bwd_kernel<IO, NP, NENC, VEC, 1>
                        <<<grid_of(E, p), kBlock, 0, as_stream(stream)>>>(x, grad, grad_x, sh, enc, num_steps, range);
            });
        });
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_lg_block_round(int64_t BL, int out_dtype, int64_t* blocks)
{
    return guarded([&] {
        AIMET_REQUIRE(blocks != nullptr, "output is null");
        check_shape(0, BL, out_dtype, "out_dtype");
        *blocks = kGrid * kWaves * plan_of(BL).per_wave;
    });
}

}   // extern "C"
