// stream_map.hpp -- the one skeleton of the streaming element-wise kernels (QDQ, STE, FP8,
// candidate QDQ, fp16 round trip: qdq.hip, qdq16.hip, fp8.hip, seqmse.hip, broadcast.hip) and the
// helpers they share.
//
// The launch policy lives here and nowhere else: one 16-B vector per lane, one tile of LANES lanes
// per workgroup, grid = ceil(vectors / LANES), non-temporal loads and stores, and a kBlock
// grid-stride scalar kernel for the ragged tail, or for the whole tensor where the vector form does
// not apply. The tile shapes were measured once through the library itself
// (tools/studies/qdq_tile_sweep.hip, profiles/r07/qdq_tile_sweep.txt); moving the kernels onto this
// skeleton left their machine code and their speed as they were (profiles/r12).
//
// An op is a small trivially copyable struct, passed by value so that its fields are kernel
// arguments (SGPRs). `__restrict__` on its pointer members states the contract (the output shares no
// storage with the inputs); independent_of() is how an op tells the optimiser. It has
//   index_t          type of the vector index (the kernel's bound check and address arithmetic)
//   tail_index_t     type of the element index of the scalar form
//   width            elements per 16-B vector (4 floats, 8 halves); 1: the op has no vector form
//   vec(i)           vector i: elements [i * width, (i + 1) * width)
//   scalar(i)        element i
// An element's index, and with it a stochastic draw, does not depend on the tile shape.
#pragma once

#include "common.hpp"

namespace aimet_amd
{

// streamed once: kept out of L2 / MALL
template <class V>
__device__ __forceinline__ V load_stream(const V* p)
{
    return __builtin_nontemporal_load(p);
}
template <class V>
__device__ __forceinline__ void store_stream(V v, V* p)
{
    __builtin_nontemporal_store(v, p);
}

// `out` shares no storage with the inputs. `__restrict__` on an op's pointer members does not reach
// the optimiser; this does. The int64 (i / K) % C forms state it: with it the compiler keeps two
// grid-stride iterations of their divide chains in flight, as it did when the pointers were
// `__restrict__` kernel parameters (6 % as a whole-tensor fallback, profiles/r12/stream_map_ab.txt).
template <class... P>
__device__ __forceinline__ void independent_of(const float* out, const P*... in)
{
    (__builtin_assume_separate_storage(out, in), ...);
}

// every pointer a multiple of A bytes (a null pointer is)
template <int A, class... P>
inline bool aligned_to(const P*... p)
{
    return ((reinterpret_cast<uintptr_t>(p) | ...) & (A - 1)) == 0;
}
template <class... P>
inline bool aligned16(const P*... p)
{
    return aligned_to<16>(p...);
}

// channel of element i of [outer][C][K] (i < 2^31)
struct ChannelMap
{
    FastDiv divK;
    FastDiv divC;
    uint32_t C;
    ChannelMap() = default;
    ChannelMap(int64_t C_, int64_t K_) : divK((uint32_t) K_), divC((uint32_t) C_), C((uint32_t) C_) {}
    __device__ __forceinline__ uint32_t channel(uint32_t i) const
    {
        uint32_t row = divK.div(i);
        return row - divC.div(row) * C;
    }
};

// column c of a per-channel table [4][C] = {min, max, delta, offset}
template <class I>
__device__ __forceinline__ QdqParams load_params(const float* __restrict__ table, I C, I c)
{
    return QdqParams {table[c], table[C + c], table[2 * C + c], table[3 * C + c]};
}

template <int LANES, class Op>
__global__ __launch_bounds__(LANES) void stream_vec_kernel(Op op, typename Op::index_t nvec)
{
    using index_t   = typename Op::index_t;
    const index_t i = (index_t) blockIdx.x * LANES + threadIdx.x;
    if (i >= nvec)
        return;
    op.vec(i);
}

template <class Op>
__global__ __launch_bounds__(kBlock) void stream_scalar_kernel(Op op, typename Op::tail_index_t begin,
                                                               typename Op::tail_index_t end)
{
    using index_t        = typename Op::tail_index_t;
    const index_t stride = (index_t) gridDim.x * kBlock;
    for (index_t i = begin + (index_t) blockIdx.x * kBlock + threadIdx.x; i < end; i += stride)
        op.scalar(i);
}

// The op over n elements: the vector kernel over [0, n / width) where `vec` holds (the caller's
// alignment / shape / size test), the scalar kernel over the rest. LANES is the family's measured
// default, overridden by aimet_qdq_tile_lanes; FIXED: exactly LANES, whatever the override says.
template <int LANES, bool FIXED = false, class Op>
void launch_stream(const Op& op, int64_t n, bool vec, hipStream_t s)
{
    int64_t done = 0;
    if constexpr (Op::width > 1)
    {
        const int64_t nvec = vec ? n / Op::width : 0;
        if (nvec > 0)
        {
            auto launch = [&](auto L) {
                constexpr int TILE = decltype(L)::value;
                stream_vec_kernel<TILE, Op>
                    <<<tile_grid(nvec, TILE), TILE, 0, s>>>(op, (typename Op::index_t) nvec);
            };
            if constexpr (FIXED)
                launch(std::integral_constant<int, LANES> {});
            else
                with_lanes(tile_lanes(LANES), launch);
            AIMET_LAUNCH_CHECK();
        }
        done = nvec * Op::width;
    }
    if (done < n)
    {
        using index_t = typename Op::tail_index_t;
        stream_scalar_kernel<Op><<<stream_blocks(n - done, kBlock), kBlock, 0, s>>>(op, (index_t) done, (index_t) n);
        AIMET_LAUNCH_CHECK();
    }
}

}   // namespace aimet_amd
