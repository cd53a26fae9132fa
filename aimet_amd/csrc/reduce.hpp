// reduce.hpp -- the shapes of the wave and workgroup reductions, written once: the 64-lane xor
// butterfly, its lane-0-to-LDS workgroup form, and the fixed 256-lane LDS tree.
//
// The shape lives here and nowhere else: which lanes meet at which step, which wave's value is
// folded when, where the barriers stand. The arithmetic does not. Every caller passes its own
// combine op(mine, other) or its own predicate better(other, mine), because those are the bit
// contract of its kernel: fminf, __builtin_fmaxf, `o > v ? o : v` and nan_max are four different
// functions of a NaN and of +-0, and a "first index wins" predicate is its kernel's tie-break.
// There is no wave_max here and there will be none.
//
//   wave_all(v, op, span)        butterfly over aligned groups of `span` lanes (64: the wave);
//                                every lane of a group gets the group's result. v is a 4- or 8-byte
//                                arithmetic value, or a trivially copyable record of 4-byte words
//                                (several values side by side: one loop, one op over the record)
//   quad_all(word, op)           the same over aligned groups of 4 lanes, one 32-bit word, two DPP steps
//   wave_best(rec, better)       butterfly that keeps `other` where better(other, rec)
//   block_fold_own<W>            wave_all, lane 0 of each wave to lds[wave], one barrier, thread 0
//                                starts from its own value and folds waves 1..W-1
//   block_fold_from<W>           the same, thread 0 starts from `init` and folds waves 0..W-1
//                                (for a float sum the two differ when wave 0 holds -0)
//   block_tree, block_tree2      256 values through LDS, strides 128..1, op(lds[t], lds[t + s])
// Neither block_fold form ends in a barrier: a caller whose LDS is used again adds its own.
#pragma once

#include <cstdint>
#include <type_traits>

#include "common.hpp"

namespace aimet_amd
{

constexpr int kTreeBlock = 256;   // block_tree's workgroup

// lane (id ^ d)'s v
template <class T>
__device__ __forceinline__ T lane_xor(const T& v, int d)
{
    if constexpr (std::is_arithmetic<T>::value)
        return __shfl_xor(v, d, 64);
    else
    {
        static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "a record of 4-byte words");
        uint32_t w[sizeof(T) / 4];
        __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
        for (size_t k = 0; k < sizeof(T) / 4; ++k)
            w[k] = __shfl_xor(w[k], d, 64);
        T r;
        __builtin_memcpy(&r, w, sizeof(T));
        return r;
    }
}

template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op, int span = 64)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        if (d < span)
            v = op(v, lane_xor(v, d));
    return v;
}

// wave_all over aligned groups of 4 lanes for one 32-bit word, as two DPP quad_perm moves
// ([1,0,3,2] then [2,3,0,1]) instead of two trips through the LDS crossbar. The four lanes of a
// group must be active together.
template <class Op>
__device__ __forceinline__ uint32_t quad_all(uint32_t v, Op op)
{
    v = op(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0xB1, 0xF, 0xF, true));
    v = op(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x4E, 0xF, 0xF, true));
    return v;
}

// a predicate as a combine: `other` where better(other, mine), else `mine`. By value and by
// assignment: a `?:` between two references selects an address and sends the record to scratch.
template <class Better>
__device__ __forceinline__ auto keep_better(Better better)
{
    return [better](auto mine, const auto& other) {
        if (better(other, mine))
            mine = other;
        return mine;
    };
}

template <class T, class Better>
__device__ __forceinline__ T wave_best(T rec, Better better)
{
    return wave_all(rec, keep_better(better));
}

// the workgroup's W wave results; valid in thread 0
template <int W, class T, class Op>
__device__ __forceinline__ T block_fold_own(T v, T* lds, Op op)
{
    v = wave_all(v, op);
    if ((threadIdx.x & 63) == 0)
        lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int w = 1; w < W; ++w)
            v = op(v, lds[w]);
    }
    return v;
}

// thread 0: ((init op wave 0) op wave 1) ...; every other thread: init
template <int W, class T, class Op>
__device__ __forceinline__ T block_fold_from(T init, T v, T* lds, Op op)
{
    v = wave_all(v, op);
    if ((threadIdx.x & 63) == 0)
        lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int w = 0; w < W; ++w)
            init = op(init, lds[w]);
    }
    return init;
}

// Two trees sharing their barriers; lds_a[0] and lds_b[0] hold the results behind the last barrier.
// No barrier follows: the callers' LDS is not written again.
template <class T, class Op>
__device__ __forceinline__ void block_tree2(T a, T b, T* lds_a, T* lds_b, Op op)
{
    const int t = threadIdx.x;
    lds_a[t]    = a;
    lds_b[t]    = b;
    __syncthreads();
    for (int s = kTreeBlock / 2; s > 0; s >>= 1)
    {
        if (t < s)
        {
            lds_a[t] = op(lds_a[t], lds_a[t + s]);
            lds_b[t] = op(lds_b[t], lds_b[t + s]);
        }
        __syncthreads();
    }
}

// One tree; every lane gets the result, and a barrier follows the read: lds is free for the next tree.
template <class T, class Op>
__device__ __forceinline__ T block_tree(T v, T* lds, Op op)
{
    const int t = threadIdx.x;
    lds[t]      = v;
    __syncthreads();
    for (int s = kTreeBlock / 2; s > 0; s >>= 1)
    {
        if (t < s)
            lds[t] = op(lds[t], lds[t + s]);
        __syncthreads();
    }
    const T r = lds[0];
    __syncthreads();
    return r;
}

}   // namespace aimet_amd
