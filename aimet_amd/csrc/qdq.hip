// qdq.hip -- quantize-dequantize, quantize-only and STE-backward ops for gfx950, and the batched
// per-channel plan kernel.
//
// Reference: trim_functions.cu:46-92 (one element per thread, 512-thread blocks, fast-math
// division, per-element global loads of the per-channel table, legacy default stream).
// The per-element IEEE division stays (tools/studies/qdq_variants.hip: the reciprocal fast path of
// common.hpp measures 4% slower here -- this kernel is HBM-bound, the fast path's extra VGPRs and
// branch cost more than the division; it pays off in the 16-bit and histogram kernels).
// MI355X design: HBM-bound streaming (8 B/elem fwd, 12 B/elem STE). The ops below (TensorQdq,
// ChannelQdq, ChannelQdq64, SteTensor, SteChannel) run on stream_map.hpp's two kernels, and its
// launch_stream holds the launch policy: one 16-B vector per lane, one tile per single-wave
// (64-lane) workgroup (STE: 256), non-temporal loads/stores. Scalar encoding parameters are kernel
// arguments (SGPRs), per-channel parameters are fetched once per 16-B vector (K % 4 == 0) from a
// device-resident table built once per encoding.
// The family defaults come from a sweep through the library itself, back-to-back launches from a
// HIP graph over fresh memory (tools/studies/qdq_tile_sweep.hip, profiles/r07/qdq_tile_sweep.txt),
// 64 / 128 / 256 lanes:
//   per-tensor, 6.4 M elements      5.28 / 5.04 / 5.12 TB/s     205.5 M      6.77 / 6.60 / 6.56 TB/s
//   the flagship step's 53 launches of its six sizes, byte-weighted: 6.63 / 6.42 / 6.38 TB/s
//   per-channel 256x64x12544        6.75 / 6.47 / 6.45 TB/s     STE 205.5 M  6.59 / 6.49 / 6.42 TB/s
//   batched plan, 54 ResNet-50 weights (25.5 M elements): 6.11 / 5.64 / 5.74 TB/s
// One wave per workgroup wins at every size and 128 lanes is within 1 % of 256, so there is no
// size threshold; the flagship step went from 3.594 to 3.456 ms of per-tensor QDQ kernel time
// (rocprofv3), 796.0 -> 829.0 Gelem/s. Adopted where the gain cleared three times the parent's
// run-to-run spread: per-tensor and batched (bench.py), per-channel (benchmarks/kernel_roofline.py:
// 6.46 -> 6.74 TB/s). The STE kernels' +3.4 % there fell just short, so they stay at 256 lanes.
#include "common.hpp"
#include "stream_map.hpp"

#include <atomic>
#include <cmath>
#include <vector>

namespace aimet_amd
{

namespace
{

enum class Op
{
    QDQ,        // dequantize(quantize(x))
    QUANTIZE    // quantize(x) - shift
};

template <Op OP, bool STOCHASTIC>
__device__ __forceinline__ float apply(float x, const QdqParams& p, float shift, uint64_t seed, uint64_t idx)
{
    float q = STOCHASTIC ? quantize_stochastic(x, p, seed, idx) : quantize_nearest(x, p);
    if constexpr (OP == Op::QDQ)
        return dequantize(q, p);
    else
        return q - shift;
}

// ---------------------------------------------------------------------------------------
// Per-tensor: parameters are kernel arguments (SGPRs): 6.80 TB/s for a 2 GiB in+out stream at
// 64 lanes (6.59 at 256; a grid-strided 4-vector loop with default cache policy reached 5.6:
// tools/studies/qdq_variants.hip, profiles/r01/qdq_variants.txt).
// ---------------------------------------------------------------------------------------
// Family defaults of the tile shape (stream_map.hpp: launch_stream), one 16-B vector per lane
constexpr int kTensorLanes  = 64;    // TensorQdq
constexpr int kChannelLanes = 64;    // ChannelQdq
constexpr int kBatchLanes   = 64;    // channel_batch_kernel (fixed per plan at its creation)
constexpr int kSteLanes     = 256;   // SteTensor / SteChannel (64: +3.4 % in kernel_roofline.py, short of the margin)

std::atomic<int> g_tile_lanes {0};   // aimet_qdq_tile_lanes; 0: the defaults above

template <Op OP, bool STOCHASTIC>
struct TensorQdq
{
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = 4;
    const float* __restrict__ in;
    float* __restrict__ out;
    QdqParams p;
    float shift;
    uint64_t seed;
    __device__ __forceinline__ void vec(int64_t i) const
    {
        f4 v = load_stream(reinterpret_cast<const f4*>(in) + i);
        uint64_t e = (uint64_t) i * 4;
        f4 r;
        r.x = apply<OP, STOCHASTIC>(v.x, p, shift, seed, e + 0);
        r.y = apply<OP, STOCHASTIC>(v.y, p, shift, seed, e + 1);
        r.z = apply<OP, STOCHASTIC>(v.z, p, shift, seed, e + 2);
        r.w = apply<OP, STOCHASTIC>(v.w, p, shift, seed, e + 3);
        store_stream(r, reinterpret_cast<f4*>(out) + i);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        out[i] = apply<OP, STOCHASTIC>(in[i], p, shift, seed, (uint64_t) i);
    }
};

// the scalar kernel runs from 0 when the pointers are misaligned
template <Op OP, bool STOCHASTIC>
void launch_tensor(const float* in, float* out, int64_t n, const QdqParams& p, float shift, uint64_t seed,
                   hipStream_t s)
{
    launch_stream<kTensorLanes>(TensorQdq<OP, STOCHASTIC> {in, out, p, shift, seed}, n, aligned16(in, out), s);
}

// ---------------------------------------------------------------------------------------
// Per-channel: [outer][C][K], table [4][C] = {min, max, delta, offset}.
// ---------------------------------------------------------------------------------------
template <bool STOCHASTIC>
struct ChannelQdq
{
    using index_t      = uint32_t;
    using tail_index_t = uint32_t;
    static constexpr int width = 4;
    const float* __restrict__ in;
    float* __restrict__ out;
    ChannelMap map;
    const float* __restrict__ table;
    uint64_t seed;
    // K % 4 == 0: a 16-B vector never straddles two channels.
    __device__ __forceinline__ void vec(uint32_t i) const
    {
        f4 v        = load_stream(reinterpret_cast<const f4*>(in) + i);
        QdqParams p = load_params(table, map.C, map.channel(i * 4));
        uint64_t e  = (uint64_t) i * 4;
        f4 r;
        r.x = apply<Op::QDQ, STOCHASTIC>(v.x, p, 0.f, seed, e + 0);
        r.y = apply<Op::QDQ, STOCHASTIC>(v.y, p, 0.f, seed, e + 1);
        r.z = apply<Op::QDQ, STOCHASTIC>(v.z, p, 0.f, seed, e + 2);
        r.w = apply<Op::QDQ, STOCHASTIC>(v.w, p, 0.f, seed, e + 3);
        store_stream(r, reinterpret_cast<f4*>(out) + i);
    }
    __device__ __forceinline__ void scalar(uint32_t i) const
    {
        QdqParams p = load_params(table, map.C, map.channel(i));
        out[i]      = apply<Op::QDQ, STOCHASTIC>(in[i], p, 0.f, seed, i);
    }
};

// 64-bit form (tensors of >= 2^31 elements): scalar only.
template <bool STOCHASTIC>
struct ChannelQdq64
{
    using tail_index_t = int64_t;
    static constexpr int width = 1;
    const float* __restrict__ in;
    float* __restrict__ out;
    int64_t C, K;
    const float* __restrict__ table;
    uint64_t seed;
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        independent_of(out, in, table);
        uint32_t c  = (uint32_t) ((i / K) % C);
        QdqParams p = load_params(table, (uint32_t) C, c);
        out[i]      = apply<Op::QDQ, STOCHASTIC>(in[i], p, 0.f, seed, (uint64_t) i);
    }
};

// ---------------------------------------------------------------------------------------
// STE backward: grad_in = grad * (min <= x <= max)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float ste(float x, float g, float mn, float mx)
{
    return g * ((mn <= x && x <= mx) ? 1.0f : 0.0f);
}

__device__ __forceinline__ void ste_vec(const float* x, const float* g, float* gi, int64_t i, float mn, float mx)
{
    f4 a = load_stream(reinterpret_cast<const f4*>(x) + i), b = load_stream(reinterpret_cast<const f4*>(g) + i), r;
    r.x = ste(a.x, b.x, mn, mx);
    r.y = ste(a.y, b.y, mn, mx);
    r.z = ste(a.z, b.z, mn, mx);
    r.w = ste(a.w, b.w, mn, mx);
    store_stream(r, reinterpret_cast<f4*>(gi) + i);
}

struct SteTensor
{
    using index_t      = int64_t;
    using tail_index_t = int64_t;
    static constexpr int width = 4;
    const float* __restrict__ x;
    const float* __restrict__ g;
    float* __restrict__ gi;
    float mn, mx;
    __device__ __forceinline__ void vec(int64_t i) const
    {
        ste_vec(x, g, gi, i, mn, mx);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        gi[i] = ste(x[i], g[i], mn, mx);
    }
};

// vector form: 32-bit FastDiv map; scalar form: int64, any K, alignment and size
struct SteChannel
{
    using index_t      = uint32_t;
    using tail_index_t = int64_t;
    static constexpr int width = 4;
    const float* __restrict__ x;
    const float* __restrict__ g;
    float* __restrict__ gi;
    ChannelMap map;
    int64_t C, K;
    const float* __restrict__ mins;
    const float* __restrict__ maxs;
    __device__ __forceinline__ void vec(uint32_t i) const
    {
        uint32_t c = map.channel(i * 4);
        float mn = mins[c], mx = maxs[c];
        ste_vec(x, g, gi, i, mn, mx);
    }
    __device__ __forceinline__ void scalar(int64_t i) const
    {
        int64_t c = (C == 1) ? 0 : (i / K) % C;
        gi[i]     = ste(x[i], g[i], mins[c], maxs[c]);
    }
};

// ---------------------------------------------------------------------------------------
// Batched per-channel QDQ (one launch for many tensors)
// ---------------------------------------------------------------------------------------
struct BatchDesc
{
    const float* in;
    float* out;
    const float* table;
    ChannelMap map;
    uint32_t n;           // elements
    uint32_t vec;         // 16-B vector path (K % 4 == 0, aligned)
    uint32_t block0;      // first workgroup of this tensor in the flattened grid (of the plan's tile shape)
    uint32_t pad;
};

template <int LANES, bool STOCHASTIC>
__global__ __launch_bounds__(LANES) void channel_batch_kernel(const BatchDesc* __restrict__ descs, int count,
                                                              uint64_t seed)
{
    // find the tensor of this workgroup (block0 is increasing): scalar binary search
    int lo = 0, hi = count - 1;
    const uint32_t b = blockIdx.x;
    while (lo < hi)
    {
        int mid = (lo + hi + 1) >> 1;
        if (descs[mid].block0 <= b)
            lo = mid;
        else
            hi = mid - 1;
    }
    const BatchDesc& d = descs[lo];
    const uint32_t t   = (b - d.block0) * LANES + threadIdx.x;
    if (d.vec)
    {
        if (t >= d.n / 4)
            return;
        f4 v        = load_stream(reinterpret_cast<const f4*>(d.in) + t);
        QdqParams p = load_params(d.table, d.map.C, d.map.channel(t * 4));
        uint64_t e  = ((uint64_t) lo << 40) + (uint64_t) t * 4;
        f4 r;
        r.x = apply<Op::QDQ, STOCHASTIC>(v.x, p, 0.f, seed, e + 0);
        r.y = apply<Op::QDQ, STOCHASTIC>(v.y, p, 0.f, seed, e + 1);
        r.z = apply<Op::QDQ, STOCHASTIC>(v.z, p, 0.f, seed, e + 2);
        r.w = apply<Op::QDQ, STOCHASTIC>(v.w, p, 0.f, seed, e + 3);
        store_stream(r, reinterpret_cast<f4*>(d.out) + t);
    }
    else
    {
        if (t >= d.n)
            return;
        QdqParams p = load_params(d.table, d.map.C, d.map.channel(t));
        d.out[t]    = apply<Op::QDQ, STOCHASTIC>(d.in[t], p, 0.f, seed, ((uint64_t) lo << 40) + t);
    }
}

}   // namespace

// -------------------------------------------------------------------------------------------
// Host side of the per-tensor encoding (TensorQuantizationSim.cpp:62-92), exact double math.
// -------------------------------------------------------------------------------------------
aimet_tf_encoding fill_encoding_info(int32_t bw, double mn, double mx);   // encodings.cpp

void per_channel_table_host(const aimet_tf_encoding* encs, int64_t C, float* table);   // encodings.cpp

int forced_tile_lanes()
{
    return g_tile_lanes.load(std::memory_order_relaxed);
}

QdqParams tensor_params(const aimet_tf_encoding& enc)
{
    aimet_tf_encoding e = fill_encoding_info(enc.bw, enc.min, enc.max);
    return QdqParams {(float) e.min, (float) e.max, (float) e.delta, (float) e.offset};
}

}   // namespace aimet_amd

using namespace aimet_amd;

struct aimet_qdq_plan
{
    int device          = 0;
    int count           = 0;
    int lanes           = 0;         // tile shape of block0 / blocks, fixed at creation
    uint32_t blocks     = 0;
    BatchDesc* descs    = nullptr;   // device
};

extern "C" {

int aimet_qdq_channel_plan_create(const aimet_qdq_channel_desc* descs, int64_t count, int device, aimet_qdq_plan** out)
{
    return guarded([&] {
        AIMET_REQUIRE(out != nullptr && descs != nullptr && count > 0, "empty plan");
        AIMET_REQUIRE(count < (1 << 20), "too many tensors in one plan");
        std::vector<BatchDesc> h((size_t) count);
        const int lanes = tile_lanes(kBatchLanes);
        uint64_t blocks = 0;
        for (int64_t i = 0; i < count; ++i)
        {
            const auto& d = descs[i];
            AIMET_REQUIRE(d.outer >= 0 && d.C > 0 && d.K >= 0, "invalid per-channel shape");
            int64_t n = d.outer * d.C * d.K;
            AIMET_REQUIRE(n < (int64_t(1) << 31), "batched per-channel QDQ needs < 2^31 elements per tensor");
            if (n > 0)
            {
                require_device_ptr(d.in, "input");
                require_device_ptr(d.out, "output");
                require_device_ptr(d.table, "table");
            }
            BatchDesc& b = h[(size_t) i];
            b.in         = d.in;
            b.out        = d.out;
            b.table      = d.table;
            b.map        = ChannelMap(d.C, d.K > 0 ? d.K : 1);
            b.n          = (uint32_t) n;
            b.vec        = (d.K % 4 == 0 && aligned16(d.in, d.out)) ? 1u : 0u;
            b.block0     = (uint32_t) blocks;
            b.pad        = 0;
            blocks += (uint64_t) ceil_div(b.vec ? n / 4 : n, lanes);
        }
        AIMET_REQUIRE(blocks < (uint64_t(1) << 31), "plan too large");
        auto* plan   = new aimet_qdq_plan();
        plan->device = device;
        plan->count  = (int) count;
        plan->lanes  = lanes;
        plan->blocks = (uint32_t) blocks;
        int prev     = 0;
        AIMET_HIP_CHECK(hipGetDevice(&prev));
        AIMET_HIP_CHECK(hipSetDevice(device));
        hipError_t e = hipMalloc(&plan->descs, sizeof(BatchDesc) * count);
        if (e == hipSuccess)
            e = hipMemcpy(plan->descs, h.data(), sizeof(BatchDesc) * count, hipMemcpyHostToDevice);
        (void) hipSetDevice(prev);
        if (e != hipSuccess)
        {
            if (plan->descs)
                (void) hipFree(plan->descs);
            delete plan;
            throw HipError(std::string("plan upload: ") + hipGetErrorString(e));
        }
        *out = plan;
    });
}

int aimet_qdq_channel_plan_run(aimet_qdq_plan* plan, int round_mode, uint64_t seed, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(plan != nullptr, "plan is null");
        AIMET_REQUIRE(round_mode == AIMET_ROUND_NEAREST || round_mode == AIMET_ROUND_STOCHASTIC,
                      "Unknown rounding mode.");
        if (plan->blocks == 0)
            return;
        hipStream_t s = as_stream(stream);
        with_lanes(plan->lanes, [&](auto L) {
            constexpr int LANES = decltype(L)::value;
            if (round_mode == AIMET_ROUND_STOCHASTIC)
                channel_batch_kernel<LANES, true><<<plan->blocks, LANES, 0, s>>>(plan->descs, plan->count, seed);
            else
                channel_batch_kernel<LANES, false><<<plan->blocks, LANES, 0, s>>>(plan->descs, plan->count, seed);
        });
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_qdq_channel_plan_destroy(aimet_qdq_plan* plan)
{
    return guarded([&] {
        if (!plan)
            return;
        if (plan->descs)
        {
            AIMET_HIP_CHECK(hipDeviceSynchronize());
            AIMET_HIP_CHECK(hipFree(plan->descs));
        }
        delete plan;
    });
}

int aimet_qdq_tile_lanes(int lanes, int* previous)
{
    return guarded([&] {
        AIMET_REQUIRE(lanes == 0 || lanes == 64 || lanes == 128 || lanes == 256, "tile lanes: 0, 64, 128 or 256");
        int prev = g_tile_lanes.exchange(lanes, std::memory_order_relaxed);
        if (previous)
            *previous = prev;
    });
}

int aimet_qdq_per_tensor(const float* in, float* out, int64_t n, const aimet_tf_encoding* enc, int round_mode,
                         uint64_t seed, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(enc != nullptr, "encoding is null");
        AIMET_REQUIRE(n >= 0, "negative element count");
        if (n == 0)
            return;
        require_device_ptr(in, "input");
        require_device_ptr(out, "output");
        QdqParams p = tensor_params(*enc);
        if (round_mode == AIMET_ROUND_NEAREST)
            launch_tensor<Op::QDQ, false>(in, out, n, p, 0.f, seed, as_stream(stream));
        else if (round_mode == AIMET_ROUND_STOCHASTIC)
            launch_tensor<Op::QDQ, true>(in, out, n, p, 0.f, seed, as_stream(stream));
        else
            throw RuntimeError("Unknown rounding mode.");
    });
}

int aimet_quantize_per_tensor(const float* in, float* out, int64_t n, const aimet_tf_encoding* enc, int round_mode,
                              int shift_to_signed, uint64_t seed, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(enc != nullptr, "encoding is null");
        AIMET_REQUIRE(n >= 0, "negative element count");
        if (n == 0)
            return;
        require_device_ptr(in, "input");
        require_device_ptr(out, "output");
        QdqParams p = tensor_params(*enc);
        // trim_functions.cpp:206-212: unsigned int shift = pow(2, bw-1), subtracted as float
        unsigned int shift = shift_to_signed ? (unsigned int) std::pow(2.0, (double) (enc->bw - 1)) : 0u;
        if (round_mode == AIMET_ROUND_NEAREST)
            launch_tensor<Op::QUANTIZE, false>(in, out, n, p, (float) shift, seed, as_stream(stream));
        else if (round_mode == AIMET_ROUND_STOCHASTIC)
            launch_tensor<Op::QUANTIZE, true>(in, out, n, p, (float) shift, seed, as_stream(stream));
        else
            throw RuntimeError("Unknown rounding mode.");
    });
}

int aimet_per_channel_table(const aimet_tf_encoding* encs, int64_t C, float* table, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(encs != nullptr && C > 0, "per-channel table needs at least one encoding");
        require_device_ptr(table, "table");
        std::vector<float> t(4 * (size_t) C);
        per_channel_table_host(encs, C, t.data());
        hipStream_t s = as_stream(stream);
        AIMET_HIP_CHECK(hipMemcpyAsync(table, t.data(), sizeof(float) * 4 * C, hipMemcpyHostToDevice, s));
        // pageable source: complete the copy before `t` goes out of scope (once per encoding change)
        AIMET_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aimet_make_delta_offset(const aimet_tf_encoding* encs, int64_t C, float* table, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(encs != nullptr && C > 0, "makeDeltaOffsetTensor needs at least one encoding");
        require_device_ptr(table, "table");
        std::vector<float> v(2 * (size_t) C);
        for (int64_t c = 0; c < C; ++c)
        {
            v[c]     = (float) encs[c].delta;
            v[C + c] = (float) encs[c].offset;
        }
        hipStream_t s = as_stream(stream);
        AIMET_HIP_CHECK(hipMemcpyAsync(table, v.data(), sizeof(float) * 2 * C, hipMemcpyHostToDevice, s));
        AIMET_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aimet_qdq_per_channel(const float* in, float* out, int64_t outer, int64_t C, int64_t K, const float* table,
                          int round_mode, uint64_t seed, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(outer >= 0 && C > 0 && K >= 0, "invalid per-channel shape");
        int64_t n = outer * C * K;
        if (n == 0)
            return;
        require_device_ptr(in, "input");
        require_device_ptr(out, "output");
        require_device_ptr(table, "table");
        AIMET_REQUIRE(round_mode == AIMET_ROUND_NEAREST || round_mode == AIMET_ROUND_STOCHASTIC,
                      "Unknown rounding mode.");
        bool sto      = round_mode == AIMET_ROUND_STOCHASTIC;
        hipStream_t s = as_stream(stream);
        auto launch = [&](auto STO) {
            constexpr bool STOCHASTIC = decltype(STO)::value;
            if (n >= (int64_t(1) << 31))
                launch_stream<kChannelLanes>(ChannelQdq64<STOCHASTIC> {in, out, C, K, table, seed}, n, false, s);
            else
                launch_stream<kChannelLanes>(ChannelQdq<STOCHASTIC> {in, out, ChannelMap(C, K), table, seed}, n,
                                             K % 4 == 0 && aligned16(in, out), s);
        };
        if (sto)
            launch(std::true_type {});
        else
            launch(std::false_type {});
    });
}

int aimet_ste_backward_per_tensor(const float* x, const float* g, float* gi, int64_t n, float mn, float mx,
                                  void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(n >= 0, "negative element count");
        if (n == 0)
            return;
        require_device_ptr(x, "x");
        require_device_ptr(g, "grad");
        require_device_ptr(gi, "grad_in");
        launch_stream<kSteLanes>(SteTensor {x, g, gi, mn, mx}, n, aligned16(x, g, gi), as_stream(stream));
    });
}

int aimet_ste_backward(const float* x, const float* g, float* gi, int64_t outer, int64_t C, int64_t K,
                       const float* mins, const float* maxs, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(outer >= 0 && C > 0 && K >= 0, "invalid per-channel shape");
        int64_t n = outer * C * K;
        if (n == 0)
            return;
        require_device_ptr(x, "x");
        require_device_ptr(g, "grad");
        require_device_ptr(gi, "grad_in");
        require_device_ptr(mins, "encoding min");
        require_device_ptr(maxs, "encoding max");
        launch_stream<kSteLanes>(SteChannel {x, g, gi, ChannelMap(C, K), C, K, mins, maxs}, n,
                                 n < (int64_t(1) << 31) && K % 4 == 0 && aligned16(x, g, gi), as_stream(stream));
    });
}

}   // extern "C"
