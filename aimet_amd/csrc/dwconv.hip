// dwconv.hip -- depthwise 2-D convolution forward and weight gradient for gfx950: the layer math
// of the AdaRound loop on MobileNet-class depthwise layers (aimet_amd.adaround_optimizer).
//
// AdaRound's per-iteration work on a depthwise layer (adaround_optimizer.py:181-218) is
// q_out = conv(x, Wq) and dL/dWq = conv_weight_grad(x, dL/dq_out) over a 32-sample batch; the
// input gradient is never needed. PyTorch's native depthwise kernels take 36 us (forward) and
// 100 us (weight gradient) per MobileNet-v2 depthwise layer-iteration (profiles/r02
// adaround_loop_kernels_v1.csv); both are HBM-bound elementwise-plus-reduction work:
//   forward:     reads x once (neighbours from L1/L2), writes y:   (|x| + |y|) * 4 B
//   weight grad: reads x and dy once:                               (|x| + |dy|) * 4 B
//
// Layout NCHW fp32, square kernel K (3 or 5), square stride / padding / dilation, groups == C
// (one filter per channel), weights [C][1][K][K].
//
// Forward: one lane per output in NCHW order (coalesced stores), y = bias + sum_kh sum_kw
// w * x in that order with fused multiply-adds (PyTorch's conv_depthwise2d_forward_kernel order).
// Weight grad: the (n, oh, ow) positions of a channel are split into S contiguous slices, one
// workgroup each; every lane keeps K*K partial sums, reduced in the workgroup by a fixed shuffle
// tree, stored per slice; a fold kernel adds the slices in order -- deterministic.
//
// The weight gradient of a given dL/dq_out (aimet_dwconv2d_grad_weight) and the AdaRound iteration
// in one pass over the cached rows (aimet_adaround_dw_step) are the same slice kernel,
// dw_slice_kernel<Form, Src, U>, with another source of the gradient: what one computes, the other
// computes with the same instructions in the same order.
#include "common.hpp"
#include "recon.hpp"
#include "stream_map.hpp"   // aligned16

namespace aimet_amd
{
namespace
{

struct DwShape
{
    uint32_t N, C, H, W, OH, OW;
    int stride, pad, dil;
    FastDiv div_ow, div_ohow, div_c;
};

template <int K>
__global__ __launch_bounds__(kBlock) void dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y,
                                                        DwShape s, uint32_t total)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= total)
        return;
    const uint32_t nc  = s.div_ohow.div(i);
    const uint32_t rem = i - nc * (s.OH * s.OW);
    const uint32_t oh  = s.div_ow.div(rem);
    const uint32_t ow  = rem - oh * s.OW;
    const uint32_t n   = s.div_c.div(nc);
    const uint32_t c   = nc - n * s.C;
    const float* xp    = x + ((size_t) n * s.C + c) * s.H * s.W;
    const float* wp    = w + c * K * K;
    float v            = bias ? bias[c] : 0.0f;
    const int ih0 = (int) oh * s.stride - s.pad, iw0 = (int) ow * s.stride - s.pad;
#pragma unroll
    for (int kh = 0; kh < K; ++kh)
    {
        const int ih = ih0 + kh * s.dil;
        if (ih < 0 || ih >= (int) s.H)
            continue;
#pragma unroll
        for (int kw = 0; kw < K; ++kw)
        {
            const int iw = iw0 + kw * s.dil;
            if (iw >= 0 && iw < (int) s.W)
                v = __builtin_fmaf(wp[kh * K + kw], xp[ih * (int) s.W + iw], v);
        }
    }
    y[i] = v;
}

// ---- forms: how a lane covers outputs and their taps ---------------------------------------------
// A unit is L consecutive outputs of one plane, starting at (oh, ow). A form holds a unit's input
// window and operand (the L values at the outputs: dL/dq, or the fp target), and owns
//   load        the window and the operand; every load reads an in-plane address (clamped) and a
//               tap outside the plane is dropped by a select on a validity bit, never by control
//               flow (per-tap branches cost ~300 scalar instructions per 4 positions)
//   forward     output j from the channel's taps: dw_fwd_kernel's FMAs in its order, from the bias
//   accumulate  acc[k] = fma(g[j], tap(j, k), acc[k]) for j = 0..L-1 in order, taps (kh, kw) in
//               order; a tap outside the plane leaves acc[k] as it is
//   clear       a unit past the slice's end: nothing valid (it is never reduced)

// one output and its K x K window
template <int K>
struct Taps
{
    static constexpr int KK = K * K, L = 1;
    static constexpr int kStepUnits = K == 3 ? 4 : 2;
    float xv[KK], o[1];
    uint32_t valid;   // bit k: tap k inside the plane

    __device__ __forceinline__ void clear()
    {
        valid = 0;
        o[0]  = 0.0f;
#pragma unroll
        for (int k = 0; k < KK; ++k)
            xv[k] = 0.0f;
    }
    __device__ __forceinline__ void load(const float* __restrict__ xp, const float* __restrict__ op, uint32_t oh,
                                         uint32_t ow, const DwShape& s)
    {
        o[0] = op[0];
        const int ih0 = (int) oh * s.stride - s.pad, iw0 = (int) ow * s.stride - s.pad;
        uint32_t m = 0;
#pragma unroll
        for (int kh = 0; kh < K; ++kh)
        {
            const int ih   = ih0 + kh * s.dil;
            const bool rin = ih >= 0 && ih < (int) s.H;
            const int ihc  = ih < 0 ? 0 : (ih >= (int) s.H ? (int) s.H - 1 : ih);
#pragma unroll
            for (int kw = 0; kw < K; ++kw)
            {
                const int iw  = iw0 + kw * s.dil;
                const bool ok = rin && iw >= 0 && iw < (int) s.W;
                const int iwc = iw < 0 ? 0 : (iw >= (int) s.W ? (int) s.W - 1 : iw);
                const float xval = xp[ihc * (int) s.W + iwc];
                xv[kh * K + kw]  = ok ? xval : 0.0f;
                m |= (ok ? 1u : 0u) << (kh * K + kw);
            }
        }
        valid = m;
    }
    __device__ __forceinline__ float forward(int, const float (&wk)[KK], float b0) const
    {
        float v = b0;
#pragma unroll
        for (int k = 0; k < KK; ++k)
        {
            const float f = __builtin_fmaf(wk[k], xv[k], v);
            v = (valid >> k) & 1u ? f : v;
        }
        return v;
    }
    __device__ __forceinline__ void accumulate(const float (&g)[1], float (&acc)[KK]) const
    {
#pragma unroll
        for (int k = 0; k < KK; ++k)
        {
            const float f = __builtin_fmaf(g[0], xv[k], acc[k]);
            acc[k] = (valid >> k) & 1u ? f : acc[k];
        }
    }
};

// K = 3, dilation 1, stride 1, OW % 4 == 0: 4 consecutive outputs of one row (a quad; OW % 4 == 0
// keeps a quad inside its row) and their 3 x 6 window, loaded once (18 loads for 36 taps); the
// index divisions are done once per quad
struct Quad
{
    static constexpr int KK = 9, L = 4;
    static constexpr int kStepUnits = 2;
    float xw[3][6], o[4];
    uint32_t rowv, colv;   // bit kh / bit c: window row / column inside the plane

    __device__ __forceinline__ void clear()
    {
        rowv = colv = 0;
    }
    __device__ __forceinline__ void load(const float* __restrict__ xp, const float* __restrict__ op, uint32_t oh,
                                         uint32_t ow, const DwShape& s)
    {
        const float4 o4 = *reinterpret_cast<const float4*>(op);
        o[0] = o4.x;
        o[1] = o4.y;
        o[2] = o4.z;
        o[3] = o4.w;
        const int H = (int) s.H, W = (int) s.W;
        const int ih0 = (int) oh - s.pad, iw0 = (int) ow - s.pad;
        int iwc[6];
        colv = 0;
#pragma unroll
        for (int c = 0; c < 6; ++c)
        {
            const int iw = iw0 + c;
            colv |= (iw >= 0 && iw < W ? 1u : 0u) << c;
            iwc[c] = iw < 0 ? 0 : (iw >= W ? W - 1 : iw);
        }
        rowv = 0;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
        {
            const int ih   = ih0 + kh;
            const bool rok = ih >= 0 && ih < H;
            rowv |= (rok ? 1u : 0u) << kh;
            const float* xr = xp + (ih < 0 ? 0 : (ih >= H ? H - 1 : ih)) * W;
#pragma unroll
            for (int c = 0; c < 6; ++c)
            {
                const float v = xr[iwc[c]];
                xw[kh][c]     = rok && ((colv >> c) & 1u) ? v : 0.0f;
            }
        }
    }
    __device__ __forceinline__ bool inside(int kh, int c) const
    {
        return ((rowv >> kh) & 1u) && ((colv >> c) & 1u);
    }
    __device__ __forceinline__ float forward(int j, const float (&wk)[9], float b0) const
    {
        float v = b0;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
            {
                const float f = __builtin_fmaf(wk[kh * 3 + kw], xw[kh][j + kw], v);
                v = inside(kh, j + kw) ? f : v;
            }
        return v;
    }
    __device__ __forceinline__ void accumulate(const float (&g)[4], float (&acc)[9]) const
    {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
                {
                    const float f = __builtin_fmaf(g[j], xw[kh][j + kw], acc[kh * 3 + kw]);
                    acc[kh * 3 + kw] = inside(kh, j + kw) ? f : acc[kh * 3 + kw];
                }
    }
};

// ---- sources: where the gradient g of a unit's outputs comes from -------------------------------
// A source names the input planes (x) and the operand planes (o), and owns
//   prologue    what a workgroup reads before its slice (Ctx)
//   plane       the plane of sample n, channel c in x and in o
//   grad        g[j] of the unit a form holds
//   units<Form> units per lane in flight: their windows and operands are loaded before any of them
//               is reduced (the accumulation order stays unit, unit + kBlock, ...)

// aimet_dwconv2d_grad_weight: the operand is dL/dq_out itself
struct GradIn
{
    const float* x;   // [N][C][H][W]
    const float* o;   // grad_y [N][C][OH][OW]
    template <class Form>
    static constexpr int units = 1;
    template <int KK>
    struct Ctx
    {
    };

    template <int KK>
    __device__ __forceinline__ Ctx<KK> prologue(uint32_t, const DwShape&) const
    {
        return {};
    }
    template <int KK>
    __device__ __forceinline__ size_t plane(const Ctx<KK>&, uint32_t n, uint32_t c, const DwShape& s) const
    {
        return (size_t) n * s.C + c;
    }
    template <class Form>
    __device__ __forceinline__ void grad(const Ctx<Form::KK>&, const Form& f, float (&g)[Form::L]) const
    {
#pragma unroll
        for (int j = 0; j < Form::L; ++j)
            g[j] = f.o[j];
    }
};

// The AdaRound iteration of a depthwise layer up to dL/dWq in ONE pass over the batch
// (aimet_adaround_dw_step). Sample n's input plane and fp target are read in place from the caches
// (row idx_all[it][n]); q = dw_fwd_kernel's sum and g = recon_grad_idx_kernel's gradient of q
// (recon_g) feed the slice kernel where GradIn reads g from memory: the partials -- and grad_w after
// dw_wgrad_fold -- are bit-identical to gather -> dw_fwd -> recon_grad_idx -> GradIn, with no batch
// copy of the input and neither q nor g in HBM (the caches are read once: |x| + |target| bytes per
// iteration instead of ~9 passes).
constexpr int kDwStepRows = 1024;   // batches up to this size keep their row table in LDS

__device__ __forceinline__ int64_t* dw_step_rows()
{
    __shared__ int64_t rows[kDwStepRows];
    return rows;
}

struct Step
{
    const float* x;           // x_cache [rows][C][H][W]
    const float* o;           // target cache [rows][C][OH][OW]
    const int64_t* idx_all;   // [iterations][N]
    const int64_t* it_cur;
    int64_t* it_next;         // workgroup (0, 0) writes it + 1 (as adaround_gather_kernel)
    const float* w;           // [C][K][K]
    const float* bias;        // nullable
    float scale;              // 2 / (N * OH * OW)
    int act;
    // (1, 2 or 8 positions per lane in flight instead of 4 measured no faster:
    // profiles/r03/dw_step_tune.jsonl); the loop is otherwise a chain of dependent loads per unit
    template <class Form>
    static constexpr int units = Form::kStepUnits;
    template <int KK>
    struct Ctx
    {
        float wk[KK], b0;
        const int64_t* rows;   // the batch's cache rows
        bool lds_rows;         // ... are in dw_step_rows()
    };

    template <int KK>
    __device__ __forceinline__ Ctx<KK> prologue(uint32_t c, const DwShape& s) const
    {
        // the channel's taps and bias first: they do not depend on the iteration counter, so their
        // loads overlap its round trip and the batch-row table's
        Ctx<KK> ctx;
#pragma unroll
        for (int k = 0; k < KK; ++k)
            ctx.wk[k] = w[c * KK + k];
        ctx.b0           = bias ? bias[c] : 0.0f;
        const int64_t it = it_cur[0];
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
            it_next[0] = it + 1;
        ctx.rows     = idx_all + it * (int64_t) s.N;
        ctx.lds_rows = s.N <= (uint32_t) kDwStepRows;
        if (ctx.lds_rows)
            for (uint32_t i = threadIdx.x; i < s.N; i += kBlock)
                dw_step_rows()[i] = ctx.rows[i];
        __syncthreads();
        return ctx;
    }
    template <int KK>
    __device__ __forceinline__ size_t plane(const Ctx<KK>& ctx, uint32_t n, uint32_t c, const DwShape& s) const
    {
        return (size_t) (ctx.lds_rows ? dw_step_rows()[n] : ctx.rows[n]) * s.C + c;
    }
    template <class Form>
    __device__ __forceinline__ void grad(const Ctx<Form::KK>& ctx, const Form& f, float (&g)[Form::L]) const
    {
#pragma unroll
        for (int j = 0; j < Form::L; ++j)   // recon_grad_idx_kernel adds the (absent) bias as + 0.0f: the same here
            g[j] = recon_g(f.forward(j, ctx.wk, ctx.b0) + 0.0f, f.o[j], scale, act);
    }
};

// workgroup reduction of the K*K sums: wave shuffles, then the waves in order, into
// partial[(c * S + slice) * K*K + k]
template <int KK>
__device__ __forceinline__ void dw_block_partial(const float (&acc)[KK], float* __restrict__ partial, uint32_t c)
{
    __shared__ float sh[KK][kBlock / 64];
#pragma unroll
    for (int k = 0; k < KK; ++k)
    {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0)
            sh[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < KK)
    {
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < kBlock / 64; ++i)
            v += sh[threadIdx.x][i];
        partial[((size_t) c * gridDim.x + blockIdx.x) * KK + threadIdx.x] = v;
    }
}

// Slice blockIdx.x of channel blockIdx.y: positions [slice * per, (slice + 1) * per) of the channel's
// N*OH*OW outputs (position p = (n * OH + oh) * OW + ow; per % L == 0), in units of L outputs, a
// lane taking units tid, tid + kBlock, ... in that order, U of them in flight.
template <class Form, class Src, int U>
__global__ __launch_bounds__(kBlock) void dw_slice_kernel(Src src, float* __restrict__ partial, DwShape s,
                                                          uint32_t per)
{
    constexpr int KK = Form::KK, L = Form::L;
    const uint32_t c  = blockIdx.y;
    const uint32_t np = s.N * s.OH * s.OW;
    const uint32_t p0 = blockIdx.x * per;
    const uint32_t p1 = p0 + per < np ? p0 + per : np;
    float acc[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k)
        acc[k] = 0.0f;
    const auto ctx    = src.template prologue<KK>(c, s);
    const uint32_t u1 = p1 / L;
    for (uint32_t ub = p0 / L + threadIdx.x; ub < u1; ub += kBlock * U)
    {
        Form f[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            f[u].clear();
            if (ub + u * kBlock < u1)
            {
                const uint32_t p   = L * (ub + u * kBlock);
                const uint32_t n   = s.div_ohow.div(p);
                const uint32_t rem = p - n * (s.OH * s.OW);
                const uint32_t oh  = s.div_ow.div(rem);
                const uint32_t ow  = rem - oh * s.OW;
                const size_t plane = src.plane(ctx, n, c, s);
                f[u].load(src.x + plane * s.H * s.W, src.o + plane * s.OH * s.OW + rem, oh, ow, s);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            if (ub + u * kBlock >= u1)
                break;
            float g[L];
            src.grad(ctx, f[u], g);
            f[u].accumulate(g, acc);
        }
    }
    dw_block_partial<KK>(acc, partial, c);
}

__global__ __launch_bounds__(kBlock) void dw_wgrad_fold(const float* __restrict__ partial, float* __restrict__ gw,
                                                        uint32_t C, uint32_t S, uint32_t KK)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;   // (c, k)
    if (i >= C * KK)
        return;
    const uint32_t c = i / KK, k = i - c * KK;
    float v          = 0.0f;
    for (uint32_t sl = 0; sl < S; ++sl)
        v += partial[((size_t) c * S + sl) * KK + k];
    gw[i] = v;
}

// the Quad form applies; `operand` (grad_y, the target cache) is read as float4
// (stride 2 measured slower in quads: 84 -> 125 us on 96 channels at 112^2, profiles/r03/dw_step_tune.jsonl)
bool dw_quads(int64_t K, int64_t stride, int64_t dil, int64_t OW, const float* operand)
{
    return K == 3 && dil == 1 && stride == 1 && OW % 4 == 0 && aligned16(operand);
}

// the slices of a channel's N*OH*OW positions, for the step and the chain alike: S slices of `per`
// positions, >= 16 positions per lane, and enough workgroups (~2048) to fill the chip
struct DwPlan
{
    bool quads;
    int64_t S;
    uint32_t per;
    int64_t KK;
    int64_t elems(int64_t C) const   // of the [C][S][K K] partials
    {
        return C * S * KK;
    }
};

DwPlan dw_plan(bool quads, int64_t N, int64_t C, int64_t OH, int64_t OW, int64_t K)
{
    const int64_t np = N * OH * OW;
    // positions per lane per slice (it sets the summation order of the weight gradient)
    constexpr int64_t ppl = 16;
    int64_t S          = ceil_div(np, (int64_t) kBlock * ppl);
    const int64_t want = ceil_div(2048, C);
    if (S < want)
        S = want < ceil_div(np, kBlock) ? want : ceil_div(np, kBlock);
    if (S < 1)
        S = 1;
    uint32_t per = (uint32_t) ceil_div(np, S);
    if (quads)
        per = (per + 3) / 4 * 4;   // slices of whole quads (np % 4 == 0 when OW % 4 == 0)
    return {quads, ceil_div(np, per), per, K * K};
}

DwShape make_shape(int64_t N, int64_t C, int64_t H, int64_t W, int64_t OH, int64_t OW, int K, int stride, int pad,
                   int dil)
{
    AIMET_REQUIRE(K == 3 || K == 5, "depthwise kernel size must be 3 or 5");
    AIMET_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "invalid depthwise shape");
    AIMET_REQUIRE(stride > 0 && pad >= 0 && dil > 0, "invalid stride / padding / dilation");
    AIMET_REQUIRE((OH - 1) * stride - 2 * pad + dil * (K - 1) + 1 <= H && (OW - 1) * stride - 2 * pad + dil * (K - 1) + 1 <= W,
                  "output size inconsistent with the input size");
    AIMET_REQUIRE(N * C * H * W < (int64_t(1) << 31) && N * C * OH * OW < (int64_t(1) << 31),
                  "depthwise tensors must have < 2^31 elements");
    DwShape s;
    s.N = (uint32_t) N, s.C = (uint32_t) C, s.H = (uint32_t) H, s.W = (uint32_t) W, s.OH = (uint32_t) OH;
    s.OW = (uint32_t) OW, s.stride = stride, s.pad = pad, s.dil = dil;
    s.div_ow   = FastDiv((uint32_t) OW);
    s.div_ohow = FastDiv((uint32_t) (OH * OW));
    s.div_c    = FastDiv((uint32_t) C);
    return s;
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

namespace
{

// The slices of `src` into `workspace` (or a scratch block of the call's own), folded into grad_w
// unless that is null. Step and chain take the quad form on the same test of their operand (the
// gradient's buffer is a 16-B aligned torch / scratch allocation wherever the target cache is one).
template <class Src>
void launch_slices(const Src& src, float* grad_w, float* workspace, const DwShape& s, int K, hipStream_t st)
{
    AIMET_REQUIRE(s.C <= 65535, "depthwise weight gradient: at most 65535 channels");
    const DwPlan p = dw_plan(dw_quads(K, s.stride, s.dil, s.OW, src.o), s.N, s.C, s.OH, s.OW, K);
    // a caller-owned workspace (aimet_dwconv2d_grad_weight_workspace elements) keeps the call
    // free of allocations, e.g. inside a HIP-graph capture
    if (workspace)
        require_device_ptr(workspace, "workspace");
    Scratch<float> own;
    if (!workspace)
        own = Scratch<float>((size_t) p.elems(s.C), st);
    float* partial = workspace ? workspace : own.get();
    const dim3 grid((unsigned) p.S, s.C);
    if (p.quads)
        dw_slice_kernel<Quad, Src, Src::template units<Quad>><<<grid, kBlock, 0, st>>>(src, partial, s, p.per);
    else if (K == 3)
        dw_slice_kernel<Taps<3>, Src, Src::template units<Taps<3>>><<<grid, kBlock, 0, st>>>(src, partial, s, p.per);
    else
        dw_slice_kernel<Taps<5>, Src, Src::template units<Taps<5>>><<<grid, kBlock, 0, st>>>(src, partial, s, p.per);
    AIMET_LAUNCH_CHECK();
    if (grad_w)   // else the Adam step folds the [C][S][K K] slices (aimet_adaround_backward_adam_parts)
    {
        dw_wgrad_fold<<<(unsigned) ceil_div(s.C * p.KK, kBlock), kBlock, 0, st>>>(partial, grad_w, s.C, (uint32_t) p.S,
                                                                                (uint32_t) p.KK);
        AIMET_LAUNCH_CHECK();
    }
}

}   // namespace

extern "C" {

int aimet_dwconv2d_forward(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t C,
                           int64_t H, int64_t W, int64_t OH, int64_t OW, int32_t K, int32_t stride, int32_t pad,
                           int32_t dilation, void* stream)
{
    return guarded([&] {
        DwShape s = make_shape(N, C, H, W, OH, OW, K, stride, pad, dilation);
        require_device_ptr(x, "x");
        require_device_ptr(w, "weight");
        require_device_ptr(y, "y");
        if (bias)
            require_device_ptr(bias, "bias");
        const uint32_t total = (uint32_t) (N * C * OH * OW);
        const unsigned grid  = (unsigned) ceil_div(total, kBlock);
        if (K == 3)
            dw_fwd_kernel<3><<<grid, kBlock, 0, as_stream(stream)>>>(x, w, bias, y, s, total);
        else
            dw_fwd_kernel<5><<<grid, kBlock, 0, as_stream(stream)>>>(x, w, bias, y, s, total);
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_dwconv2d_grad_weight_workspace(int64_t N, int64_t C, int64_t OH, int64_t OW, int32_t K, int64_t* elems)
{
    return guarded([&] {
        AIMET_REQUIRE(elems != nullptr, "elems is null");
        AIMET_REQUIRE(N > 0 && C > 0 && OH > 0 && OW > 0 && (K == 3 || K == 5), "invalid depthwise shape");
        *elems = dw_plan(false, N, C, OH, OW, K).elems(C);   // the quad form never takes more slices
    });
}

int aimet_dwconv2d_grad_weight(const float* x, const float* grad_y, float* grad_w, float* workspace, int64_t N,
                               int64_t C, int64_t H, int64_t W, int64_t OH, int64_t OW, int32_t K, int32_t stride,
                               int32_t pad, int32_t dilation, void* stream)
{
    return guarded([&] {
        DwShape s = make_shape(N, C, H, W, OH, OW, K, stride, pad, dilation);
        require_device_ptr(x, "x");
        require_device_ptr(grad_y, "grad_y");
        require_device_ptr(grad_w, "grad_w");
        launch_slices(GradIn {x, grad_y}, grad_w, workspace, s, K, as_stream(stream));
    });
}

int aimet_adaround_dw_step(const float* x_cache, const float* target_cache, const int64_t* idx_all,
                           const int64_t* it_cur, int64_t* it_next, const float* w, const float* bias, float* grad_w,
                           float* workspace, int64_t N, int64_t C, int64_t H, int64_t W, int64_t OH, int64_t OW,
                           int32_t K, int32_t stride, int32_t pad, int32_t dilation, int32_t act, void* stream)
{
    return guarded([&] {
        DwShape s = make_shape(N, C, H, W, OH, OW, K, stride, pad, dilation);
        AIMET_REQUIRE(act >= 0 && act <= 2, "act must be 0 (none), 1 (ReLU) or 2 (ReLU6)");
        require_device_ptr(x_cache, "x_cache");
        require_device_ptr(target_cache, "target_cache");
        require_device_ptr(idx_all, "idx_all");
        require_device_ptr(it_cur, "it_cur");
        require_device_ptr(it_next, "it_next");
        require_device_ptr(w, "weight");
        AIMET_REQUIRE(grad_w || workspace, "grad_w may be null only with a workspace (the slices stay there)");
        if (grad_w)
            require_device_ptr(grad_w, "grad_w");
        if (bias)
            require_device_ptr(bias, "bias");
        // aimet_adaround_recon_grad_indexed's scale: 2 / (number of dim-1 norms)
        const float scale = (float) (2.0 / (double) (N * OH * OW));
        launch_slices(Step {x_cache, target_cache, idx_all, it_cur, it_next, w, bias, scale, act}, grad_w, workspace, s,
                      K, as_stream(stream));
    });
}

int aimet_adaround_dw_step_slices(const float* target_cache, int64_t N, int64_t C, int64_t OH, int64_t OW, int32_t K,
                                  int32_t stride, int32_t dilation, int64_t* slices)
{
    return guarded([&] {
        AIMET_REQUIRE(slices != nullptr, "slices is null");
        AIMET_REQUIRE(N > 0 && C > 0 && OH > 0 && OW > 0 && (K == 3 || K == 5), "invalid depthwise shape");
        *slices = dw_plan(dw_quads(K, stride, dilation, OW, target_cache), N, C, OH, OW, K).S;
    });
}

}   // extern "C"
