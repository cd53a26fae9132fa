// seqmse.hip -- the three kernels of Sequential MSE (aimet_torch/v1/seq_mse.py) for gfx950.
//
// Reference: SequentialMse.optimize_module (seq_mse.py:467-503). Per module and per candidate it
// resets the weight quantizer, feeds it a [C,2] tensor, computes the encoding on the host, uploads
// a table, quantize-dequantizes W (8 B/element per candidate), runs two GEMMs (the FP32 one is the
// same every time) and reduces mse_loss(reduction="none").sum(0) in three passes over the output.
// MI355X design:
//   * candidate_tables: every candidate's per-channel table [n_cand][4][C] in one launch, one lane
//     per (candidate, channel), in the double arithmetic of the host path (TF analyzer on the
//     two-element statistics -> getComputedEncodings -> the fp32 table of per_channel_table_host),
//     bit for bit. A device kernel rather than a host build: min/max stay in HBM, no D2H of the
//     statistics, no H2D of n_cand tables, no synchronisation; the double divide and round/floor/
//     ceil are IEEE on gfx950 and mse_core.hpp already runs getComputedEncodings there.
//   * candidate_qdq: W is read once and stays in registers while the window's candidates are
//     written with streaming stores: 4 + 4*count B/element instead of 8*count. The CandidateQdq
//     op on the streaming skeleton of stream_map.hpp, at a fixed one wave per workgroup; the
//     element arithmetic of qdq.hip (quantize_nearest / dequantize, IEEE divide).
//   * recon_sums: sum over tokens of (xqwq - xw)^2 (or |.|) for every (candidate, channel) and
//     sum xw^2 once, reading every xqwq element once. No float atomics: per-workgroup partials go
//     to a workspace and a second small pass adds them in a fixed order, so the result is
//     bitwise reproducible. Linear layout (inner == 1): a lane owns 4 adjacent channels (16-B
//     loads, coalesced along channels) and kJT candidates of them, the four waves of a workgroup
//     take interleaved rows and are added through LDS (no cross-lane step is needed: a lane's
//     sums are already per channel). Conv2d layout (inner > 1, NCHW used as it is): a workgroup
//     owns one channel, lanes run along (image, pixel), sums go through a wave shuffle tree, then
//     LDS. xw is re-read once per group of kJT candidates (from L2 / MALL: it is 1/count of the
//     traffic).
#include "common.hpp"
#include "mse_core.hpp"
#include "stream_map.hpp"

#include <cmath>

namespace aimet_amd
{

namespace
{

constexpr int kQdqLanes   = 64;   // CandidateQdq: fixed (stream_map.hpp: launch_stream)
constexpr int kJT         = 4;    // candidates a lane accumulates at once in recon_sums
constexpr int kReconBlock = 256;
constexpr int kReconWaves = kReconBlock / 64;
constexpr int64_t kTargetBlocks = 2048;   // 256 CUs x 8 resident workgroups
constexpr int64_t kMaxGridYZ    = 65535;

// ---------------------------------------------------------------------------------------------
// (a) candidate tables
// ---------------------------------------------------------------------------------------------
// The encoding the existing path computes for candidate j of channel c: SequentialMse.
// compute_param_encodings feeds the TF analyzer the two values {cand_min, cand_max}
// (stats.hip: fp32 min / max, folded into the double running min / max), tf_encoding
// (encodings.cpp) gates them and calls getComputedEncodings.
__device__ aimet_tf_encoding candidate_encoding(const float* __restrict__ mins, const float* __restrict__ maxs,
                                                int64_t c, int j, int n_cand, int bw, bool sym, bool strict,
                                                bool unsign)
{
    // per_channel_max / num_candidates * (cand + 1) in fp32: an IEEE divide, then a multiply
    const float n = (float) n_cand, k = (float) (j + 1);
    const float cmax = maxs[c] / n * k;
    const float cmin = mins ? mins[c] / n * k : -cmax;
    const double acc_min = (double) (cmax < cmin ? cmax : cmin);
    const double acc_max = (double) (cmin > cmax ? cmin : cmax);
    // tf_encoding: std::min(0.0, accMin), std::max(0.0, accMax), std::max(hi, lo + 0.01)
    const double lo = acc_min < 0.0 ? acc_min : 0.0;
    double hi       = 0.0 < acc_max ? acc_max : 0.0;
    hi              = hi < lo + 0.01 ? lo + 0.01 : hi;
    return mse::computed_encoding(bw, lo, hi, sym, strict, unsign);
}

// per_channel_table_host (encodings.cpp), one row: fp32 torch ops, NaN-propagating minimum /
// maximum, at::round half-to-even; the step count comes from channel 0's encoding
__device__ __forceinline__ float torch_min(float a, float b)
{
    return (a != a || b != b) ? __builtin_nanf("") : (a < b ? a : b);
}
__device__ __forceinline__ float torch_max(float a, float b)
{
    return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b);
}

__global__ __launch_bounds__(kBlock) void candidate_tables_kernel(const float* __restrict__ mins,
                                                                  const float* __restrict__ maxs, int64_t C,
                                                                  int n_cand, int bw, int sym, int strict, int unsign,
                                                                  float* __restrict__ tables)
{
    const int64_t i = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= C * n_cand)
        return;
    const int j     = (int) (i / C);
    const int64_t c = i - (int64_t) j * C;
    const aimet_tf_encoding e0 = candidate_encoding(mins, maxs, 0, j, n_cand, bw, sym, strict, unsign);
    const aimet_tf_encoding e  = c == 0 ? e0 : candidate_encoding(mins, maxs, c, j, n_cand, bw, sym, strict, unsign);
    double steps = ldexp(1.0, e0.bw) - 1;
    if (e0.min == -e0.max)
        steps -= 1;
    const float fsteps = (float) steps;
    const float eps    = (float) 1e-5;
    float mn           = torch_min((float) e.min, 0.0f);
    float mx           = torch_max((float) e.max, 0.0f);
    mx                 = torch_max(mx, mn + eps);
    const float d      = (mx - mn) / fsteps;
    float* t           = tables + (int64_t) j * 4 * C + c;
    t[0]               = mn;
    t[C]               = mx;
    t[2 * C]           = d;
    t[3 * C]           = __builtin_rintf(mn / d);
}

// ---------------------------------------------------------------------------------------------
// (b) candidate QDQ: out[count][C][K] from W[C][K] and tables[first .. first + count)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float qdq_nearest(float x, const QdqParams& p)
{
    return dequantize(quantize_nearest(x, p), p);
}

// one load, `count` stores, candidate j's plane n elements after candidate j - 1's
struct CandidateQdq
{
    using index_t      = uint32_t;
    using tail_index_t = uint32_t;
    static constexpr int width = 4;
    const float* __restrict__ in;
    float* __restrict__ out;
    uint32_t n;
    FastDiv divK;
    int64_t C;
    const float* __restrict__ tables;
    int count;
    // K % 4 == 0: a 16-B vector never straddles two channels
    __device__ __forceinline__ void vec(uint32_t i) const
    {
        const f4 v     = load_stream(reinterpret_cast<const f4*>(in) + i);
        const float* t = tables + divK.div(i * 4);   // this channel's column of the first table
        f4* o          = reinterpret_cast<f4*>(out) + i;
        for (int j = 0; j < count; ++j, t += 4 * C, o += n / 4)
        {
            const QdqParams p = load_params(t, C, int64_t(0));
            f4 r;
            r.x = qdq_nearest(v.x, p);
            r.y = qdq_nearest(v.y, p);
            r.z = qdq_nearest(v.z, p);
            r.w = qdq_nearest(v.w, p);
            store_stream(r, o);
        }
    }
    __device__ __forceinline__ void scalar(uint32_t i) const
    {
        const float v  = in[i];
        const float* t = tables + divK.div(i);
        float* o       = out + i;
        for (int j = 0; j < count; ++j, t += 4 * C, o += n)
        {
            const QdqParams p = load_params(t, C, int64_t(0));
            *o                = qdq_nearest(v, p);
        }
    }
};

// ---------------------------------------------------------------------------------------------
// (c) reconstruction sums
// ---------------------------------------------------------------------------------------------
template <int VEC>
struct Vec;
template <>
struct Vec<1>
{
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
    __device__ __forceinline__ void load_stream(const float* p) { v[0] = __builtin_nontemporal_load(p); }
};
template <>
struct Vec<4>
{
    float v[4];
    __device__ __forceinline__ void set(f4 t)
    {
        v[0] = t.x;
        v[1] = t.y;
        v[2] = t.z;
        v[3] = t.w;
    }
    __device__ __forceinline__ void load(const float* p) { set(*reinterpret_cast<const f4*>(p)); }
    __device__ __forceinline__ void load_stream(const float* p)
    {
        set(__builtin_nontemporal_load(reinterpret_cast<const f4*>(p)));
    }
};

template <bool L1>
__device__ __forceinline__ float accumulate(float acc, float q, float w)
{
    const float d = q - w;
    if constexpr (L1)
        return acc + __builtin_fabsf(d);
    else
        return __builtin_fmaf(d, d, acc);
}

// How a call is cut into workgroups; the workspace query and the launch share it, so it depends on
// the sizes alone (never on pointer alignment).
struct ReconPlan
{
    int64_t tiles;    // grid x: channel tiles (Linear) or channels (Conv2d)
    int64_t groups;   // grid y: groups of kJT candidates
    int64_t R;        // grid z: chunks of rows (Linear) or of outer * inner elements (Conv2d)
    int64_t per;      // rows / elements per chunk
    int64_t stride;   // floats per partial row: count * C error sums, then C signal sums
};

ReconPlan recon_plan(int64_t outer, int64_t C, int64_t inner, int64_t count)
{
    ReconPlan p;
    p.groups = ceil_div(count, kJT);
    p.stride = count * C + C;
    int64_t total, unit;
    if (inner == 1)
    {
        p.tiles = ceil_div(C % 4 == 0 ? C / 4 : C, 64);
        total   = outer;
        unit    = kReconWaves;            // a row per wave
    }
    else
    {
        p.tiles = C;
        total   = outer * inner;
        unit    = kReconBlock * 4;        // a 16-B vector per lane
    }
    if (total <= 0)
    {
        p.R = p.per = 0;
        return p;
    }
    int64_t R = ceil_div(kTargetBlocks, p.tiles * p.groups);
    R         = std::min(R, ceil_div(total, unit * 4));   // at least four steps of a chunk's loop
    R         = std::max<int64_t>(1, std::min(R, kMaxGridYZ));
    p.per     = ceil_div(ceil_div(total, R), unit) * unit;
    p.R       = ceil_div(total, p.per);
    return p;
}

// Linear layout: xw [T][C], xq [T][count * C]; lane -> VEC adjacent channels, wave -> every
// fourth row of the chunk. part[z][j * C + c] / part[z][count * C + c].
template <int VEC, bool L1>
__global__ __launch_bounds__(kReconBlock) void recon_rows_kernel(const float* __restrict__ xw,
                                                                 const float* __restrict__ xq, int64_t T, int64_t C,
                                                                 int count, int64_t per, int want_sig,
                                                                 float* __restrict__ part, int64_t stride)
{
    __shared__ float lds[kReconWaves][kJT + 1][VEC][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c  = ((int64_t) blockIdx.x * 64 + lane) * VEC;
    const int j0     = blockIdx.y * kJT;
    const int64_t r0 = (int64_t) blockIdx.z * per;
    const int64_t r1 = r0 + per < T ? r0 + per : T;
    const int64_t N  = (int64_t) count * C;
    const bool sig   = want_sig && blockIdx.y == 0;
    float acc[kJT + 1][VEC];
#pragma unroll
    for (int a = 0; a <= kJT; ++a)
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            acc[a][v] = 0.0f;
    if (c < C)   // C % VEC == 0: the whole vector is inside the row
    {
        for (int64_t r = r0 + wave; r < r1; r += kReconWaves)
        {
            Vec<VEC> w;
            w.load(xw + r * C + c);
            const float* q0 = xq + r * N + (int64_t) j0 * C + c;
#pragma unroll
            for (int jj = 0; jj < kJT; ++jj)
                if (j0 + jj < count)
                {
                    Vec<VEC> q;
                    q.load_stream(q0 + (int64_t) jj * C);
#pragma unroll
                    for (int v = 0; v < VEC; ++v)
                        acc[jj][v] = accumulate<L1>(acc[jj][v], q.v[v], w.v[v]);
                }
            if (sig)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc[kJT][v] = __builtin_fmaf(w.v[v], w.v[v], acc[kJT][v]);
        }
    }
#pragma unroll
    for (int a = 0; a <= kJT; ++a)
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            lds[wave][a][v][lane] = acc[a][v];
    __syncthreads();
    if (wave != 0 || c >= C)
        return;
    float* prow = part + (int64_t) blockIdx.z * stride;
#pragma unroll
    for (int a = 0; a <= kJT; ++a)
    {
        const bool live = a < kJT ? (j0 + a < count) : sig;
        if (!live)
            continue;
        float* dst = a < kJT ? prow + (int64_t) (j0 + a) * C + c : prow + N + c;
#pragma unroll
        for (int v = 0; v < VEC; ++v)
        {
            float s = lds[0][a][v][lane];
#pragma unroll
            for (int w = 1; w < kReconWaves; ++w)
                s += lds[w][a][v][lane];
            dst[v] = s;
        }
    }
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    return v;   // lane 0
}

// Conv2d layout: xw [outer][C][inner], xq [outer][count * C][inner]; workgroup -> one channel,
// kJT candidates and a chunk of the channel's outer * inner elements (e = o * inner + i).
template <int VEC, bool L1>
__global__ __launch_bounds__(kReconBlock) void recon_planes_kernel(const float* __restrict__ xw,
                                                                   const float* __restrict__ xq, uint32_t E,
                                                                   FastDiv divInner, int64_t C, int count, int64_t per,
                                                                   int want_sig, float* __restrict__ part,
                                                                   int64_t stride)
{
    __shared__ float lds[kReconWaves][kJT + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c     = blockIdx.x;
    const int j0        = blockIdx.y * kJT;
    const int64_t inner = divInner.d;
    const int64_t N     = (int64_t) count * C;
    const int64_t e0    = (int64_t) blockIdx.z * per;
    const int64_t e1    = e0 + per < (int64_t) E ? e0 + per : (int64_t) E;
    const bool sig      = want_sig && blockIdx.y == 0;
    float acc[kJT + 1];
#pragma unroll
    for (int a = 0; a <= kJT; ++a)
        acc[a] = 0.0f;
    // inner % VEC == 0: a vector stays inside one image's row of the channel
    for (int64_t e = e0 + (int64_t) threadIdx.x * VEC; e < e1; e += kReconBlock * VEC)
    {
        const int64_t o = divInner.div((uint32_t) e);
        const int64_t i = e - o * inner;
        Vec<VEC> w;
        w.load(xw + (o * C + c) * inner + i);
        const float* q0 = xq + (o * N + (int64_t) j0 * C + c) * inner + i;
#pragma unroll
        for (int jj = 0; jj < kJT; ++jj)
            if (j0 + jj < count)
            {
                Vec<VEC> q;
                q.load_stream(q0 + (int64_t) jj * C * inner);
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc[jj] = accumulate<L1>(acc[jj], q.v[v], w.v[v]);
            }
        if (sig)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                acc[kJT] = __builtin_fmaf(w.v[v], w.v[v], acc[kJT]);
    }
#pragma unroll
    for (int a = 0; a <= kJT; ++a)
    {
        const float s = wave_sum(acc[a]);
        if (lane == 0)
            lds[wave][a] = s;
    }
    __syncthreads();
    const int a = threadIdx.x;
    if (a > kJT)
        return;
    const bool live = a < kJT ? (j0 + a < count) : sig;
    if (!live)
        return;
    float s = lds[0][a];
#pragma unroll
    for (int w = 1; w < kReconWaves; ++w)
        s += lds[w][a];
    float* prow = part + (int64_t) blockIdx.z * stride;
    if (a < kJT)
        prow[(int64_t) (j0 + a) * C + c] = s;
    else
        prow[N + c] = s;
}

// second pass: err[i] = sum over the R partial rows, in row order; the signal sums follow
__global__ __launch_bounds__(kBlock) void recon_fold_kernel(const float* __restrict__ part, int64_t R, int64_t stride,
                                                            int64_t N, int64_t n_sig, float* __restrict__ err,
                                                            float* __restrict__ sig)
{
    const int64_t i = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= N + n_sig)
        return;
    float s = 0.0f;
    for (int64_t r = 0; r < R; ++r)
        s += part[r * stride + i];
    if (i < N)
        err[i] = s;
    else
        sig[i - N] = s;
}

void check_recon_shape(int64_t outer, int64_t C, int64_t inner, int64_t count)
{
    AIMET_REQUIRE(outer >= 0 && C > 0 && inner > 0 && count > 0, "invalid reconstruction shape");
    AIMET_REQUIRE(count * C < (int64_t(1) << 31), "count * C must be below 2^31");
    AIMET_REQUIRE(ceil_div(count, kJT) <= kMaxGridYZ, "too many candidates in one call");
    AIMET_REQUIRE(inner == 1 || outer * inner < (int64_t(1) << 31),
                  "Conv2d layout needs outer * inner below 2^31");
}

}   // namespace

}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_seqmse_candidate_tables(const float* min_dev, const float* max_dev, int64_t C, int32_t num_candidates,
                                  int32_t bw, int sym, int strict, int unsign, float* tables_dev, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(C > 0 && num_candidates > 0, "candidate tables need at least one channel and one candidate");
        AIMET_REQUIRE(num_candidates <= (1 << 24), "too many candidates");   // exact in fp32
        AIMET_REQUIRE(bw > 0 && bw <= 32, "invalid bitwidth");
        if (min_dev)
            require_device_ptr(min_dev, "per-channel min");
        require_device_ptr(max_dev, "per-channel max");
        require_device_ptr(tables_dev, "tables");
        const unsigned blocks = tile_grid(C * num_candidates, kBlock);
        candidate_tables_kernel<<<blocks, kBlock, 0, as_stream(stream)>>>(min_dev, max_dev, C, num_candidates,
                                                                          (int32_t) (uint8_t) bw, sym != 0,
                                                                          strict != 0, unsign != 0, tables_dev);
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_seqmse_candidate_qdq(const float* w, float* out, int64_t C, int64_t K, const float* tables_dev,
                               int64_t num_candidates, int64_t first, int64_t count, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(C > 0 && K >= 0, "invalid per-channel shape");
        AIMET_REQUIRE(first >= 0 && count >= 0 && first + count <= num_candidates, "candidate window out of range");
        AIMET_REQUIRE(count < (int64_t(1) << 31), "candidate window too large");
        const int64_t n = C * K;
        AIMET_REQUIRE(n < (int64_t(1) << 31), "candidate QDQ needs fewer than 2^31 weight elements");
        if (n == 0 || count == 0)
            return;
        require_device_ptr(w, "weight");
        require_device_ptr(out, "output");
        require_device_ptr(tables_dev, "tables");
        hipStream_t s  = as_stream(stream);
        const float* t = tables_dev + first * 4 * C;
        launch_stream<kQdqLanes, true>(CandidateQdq {w, out, (uint32_t) n, FastDiv((uint32_t) K), C, t, (int) count}, n,
                                       K % 4 == 0 && aligned16(w, out), s);
    });
}

int aimet_seqmse_recon_sums_workspace(int64_t outer, int64_t C, int64_t inner, int64_t count, int64_t* bytes)
{
    return guarded([&] {
        AIMET_REQUIRE(bytes != nullptr, "bytes is null");
        check_recon_shape(outer, C, inner, count);
        const ReconPlan p = recon_plan(outer, C, inner, count);
        *bytes            = (int64_t) sizeof(float) * p.R * p.stride;
    });
}

int aimet_seqmse_recon_sums(const float* xw, const float* xqwq, int64_t outer, int64_t C, int64_t inner,
                            int64_t count, int loss_kind, float* err, float* sig, void* workspace,
                            int64_t workspace_bytes, void* stream)
{
    return guarded([&] {
        check_recon_shape(outer, C, inner, count);
        AIMET_REQUIRE(loss_kind == AIMET_SEQMSE_LOSS_MSE || loss_kind == AIMET_SEQMSE_LOSS_L1 ||
                          loss_kind == AIMET_SEQMSE_LOSS_SQNR,
                      "Unknown loss kind.");
        const bool want_sig = loss_kind == AIMET_SEQMSE_LOSS_SQNR;
        const bool l1       = loss_kind == AIMET_SEQMSE_LOSS_L1;
        require_device_ptr(err, "err");
        if (want_sig)
            require_device_ptr(sig, "sig");
        const ReconPlan p = recon_plan(outer, C, inner, count);
        AIMET_REQUIRE(workspace_bytes >= (int64_t) sizeof(float) * p.R * p.stride, "workspace too small");
        hipStream_t s = as_stream(stream);
        float* part   = static_cast<float*>(workspace);
        const int64_t N = count * C;
        if (p.R > 0)
        {
            require_device_ptr(xw, "xw");
            require_device_ptr(xqwq, "xqwq");
            require_device_ptr(workspace, "workspace");
            const dim3 grid(tile_grid(p.tiles, 1), (unsigned) p.groups, (unsigned) p.R);
            const bool al = aligned16(xw, xqwq);
            if (inner == 1)
            {
                const bool vec = C % 4 == 0 && al;
                // the plan's tiles are those of the vector kernel when C % 4 == 0; the scalar kernel
                // on misaligned pointers then needs four times as many
                const dim3 g1(tile_grid(vec ? p.tiles : ceil_div(C, 64), 1), grid.y, grid.z);
                if (vec && l1)
                    recon_rows_kernel<4, true><<<g1, kReconBlock, 0, s>>>(xw, xqwq, outer, C, (int) count, p.per,
                                                                          want_sig, part, p.stride);
                else if (vec)
                    recon_rows_kernel<4, false><<<g1, kReconBlock, 0, s>>>(xw, xqwq, outer, C, (int) count, p.per,
                                                                           want_sig, part, p.stride);
                else if (l1)
                    recon_rows_kernel<1, true><<<g1, kReconBlock, 0, s>>>(xw, xqwq, outer, C, (int) count, p.per,
                                                                          want_sig, part, p.stride);
                else
                    recon_rows_kernel<1, false><<<g1, kReconBlock, 0, s>>>(xw, xqwq, outer, C, (int) count, p.per,
                                                                           want_sig, part, p.stride);
            }
            else
            {
                const bool vec   = inner % 4 == 0 && al;
                const uint32_t E = (uint32_t) (outer * inner);
                const FastDiv divInner((uint32_t) inner);
                if (vec && l1)
                    recon_planes_kernel<4, true><<<grid, kReconBlock, 0, s>>>(xw, xqwq, E, divInner, C, (int) count,
                                                                              p.per, want_sig, part, p.stride);
                else if (vec)
                    recon_planes_kernel<4, false><<<grid, kReconBlock, 0, s>>>(xw, xqwq, E, divInner, C, (int) count,
                                                                               p.per, want_sig, part, p.stride);
                else if (l1)
                    recon_planes_kernel<1, true><<<grid, kReconBlock, 0, s>>>(xw, xqwq, E, divInner, C, (int) count,
                                                                              p.per, want_sig, part, p.stride);
                else
                    recon_planes_kernel<1, false><<<grid, kReconBlock, 0, s>>>(xw, xqwq, E, divInner, C, (int) count,
                                                                               p.per, want_sig, part, p.stride);
            }
            AIMET_LAUNCH_CHECK();
        }
        const int64_t n_out = N + (want_sig ? C : 0);
        recon_fold_kernel<<<tile_grid(n_out, kBlock), kBlock, 0, s>>>(part, p.R, p.stride, N, want_sig ? C : 0, err,
                                                                      sig);
        AIMET_LAUNCH_CHECK();
    });
}

}   // extern "C"
