// attn_softmax.hip -- the score quantizer, the masks, the softmax and the probability quantizer of a
// quantizable multi-head attention (aimet_torch/transformers/activation.py: matmul_1's output QDQ,
// masked_fill_ with the attention mask, masked_fill with the padding mask, nn.Softmax, softmax's
// output QDQ) in ONE launch over the [B H, L, S] score tensor: every row is read once, stays on chip
// and is written once.
//
// Per row r = bh L + l (b = bh / H), j in [0, S), all in float32, one rounding per operation:
//   x_j = QDQ(scores[r S + j]; score_enc)              quantize_nearest / dequantize of common.hpp
//   x_j = -inf  where attn_mask[((per_bh ? bh : 0) L + l) S + j] or key_padding_mask[b S + j] is set
//   m   = max_j x_j                                    (-inf for a row with every position masked)
//   e_j = x_j == -inf ? 0 : exp_r(x_j - m)             rnn_math.hpp; a masked position is exactly 0
//   s   = sum of e_j in the ORDER BELOW
//   p_j = e_j / s                                      IEEE divide; 0 / 0 = NaN for a fully masked row
//   probs[r S + j] = QDQ(p_j; prob_enc)
// A null encoding skips its QDQ, a null mask masks nothing.
//
// Summation order (part of the contract; tests/mha_oracle.py restates it). It depends on S alone:
//   S <= kWaveMaxS (1024), "wave path": one 64-lane wave per row. Lane t accumulates the elements
//     j = t, t + 64, t + 128, ... in increasing j, starting from the first (a lane without elements
//     holds +0). Then six butterfly steps over the 64 lane sums, v_t = v_t + v_(t xor d) for
//     d = 32, 16, 8, 4, 2, 1 in this order; every lane ends with the same s.
//   kWaveMaxS < S <= kMaxS (16320), "LDS path": one 256-thread workgroup per row, the row in LDS.
//     Thread t accumulates j = t, t + 256, t + 512, ... in increasing j; each of the four waves
//     (threads 64 w .. 64 w + 63) runs the same six butterfly steps on its 64 sums, giving w0..w3;
//     s = (w0 + w1) + (w2 + w3).
//   S > kMaxS (a row of 16320 floats and the four partial sums fill 64 KiB of LDS): refused, nothing
//     written.
// The maximum is exact in any order.
//
// Memory shape. Wave path: the row lives in registers, ceil(S / 64) values a lane (instantiated for
// 1, 2, 4, 8, 16); lane t reads and writes dword t of each 64-dword group, which needs no alignment
// beyond 4 bytes and leaves the lane-to-element map (the summation order) independent of the
// row's address. LDS path: 16-byte global loads and stores on the aligned body of the row, with a
// scalar head of up to three floats and a scalar tail, separately for source and destination (S is
// often odd, so consecutive rows have different alignments); the fixed-order sum then reads LDS by
// element index. 64-bit offsets throughout; rows are taken in a grid-stride loop. In place
// (probs == scores) is safe on both paths: a row is read completely before any of it is written.

#include "common.hpp"
#include "rnn_math.hpp"

namespace aimet_amd
{

QdqParams tensor_params(const aimet_tf_encoding& enc);   // qdq.hip

namespace
{

constexpr int kBlk        = 256;
constexpr int kWave       = 64;
constexpr int kWaveMaxS   = 1024;
constexpr int kMaxS       = AIMET_ATTN_SOFTMAX_MAX_S;
constexpr unsigned kMaxGrid = 1u << 16;

static_assert((kMaxS % 4) == 0 && kMaxS * 4 + 16 <= 65536, "a row and the partial sums must fit 64 KiB of LDS");

LaunchCounter g_launches;

struct Args
{
    const float* scores;
    float* probs;
    const uint8_t* attn_mask;
    const uint8_t* kpm;
    int64_t rows;   // B H L
    int64_t L, H;
    int S;
    int per_bh, score_qdq, prob_qdq;
    QdqParams sp, pp;
};

struct F4
{
    float v[4];
};

struct Row
{
    const float* src;
    float* dst;
    const uint8_t* am;    // this row's S attention-mask bytes, or null
    const uint8_t* kpm;   // this row's S padding-mask bytes, or null
};

__device__ __forceinline__ Row row_of(const Args& a, int64_t r)
{
    const int64_t bh = r / a.L, l = r - bh * a.L, b = bh / a.H;
    Row w;
    w.src = a.scores + r * a.S;
    w.dst = a.probs + r * a.S;
    w.am  = a.attn_mask ? a.attn_mask + ((a.per_bh ? bh : 0) * a.L + l) * a.S : nullptr;
    w.kpm = a.kpm ? a.kpm + b * a.S : nullptr;
    return w;
}

__device__ __forceinline__ float neg_inf()
{
    return -__builtin_huge_valf();
}

// steps 1 and 2 for element j of a row
__device__ __forceinline__ float score_of(const Args& a, const Row& w, float x, int j, float s_rcp)
{
    if (a.score_qdq)
        x = dequantize(quantize_nearest_rcp(x, a.sp, s_rcp), a.sp);
    if ((w.am && w.am[j]) || (w.kpm && w.kpm[j]))
        x = neg_inf();
    return x;
}

__device__ __forceinline__ float exp_of(float x, float m)
{
    return x == neg_inf() ? 0.0f : rnn_math::exp_r(x - m);
}

__device__ __forceinline__ float prob_of(const Args& a, float e, float s, float p_rcp)
{
    const float p = e / s;
    return a.prob_qdq ? dequantize(quantize_nearest_rcp(p, a.pp, p_rcp), a.pp) : p;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        const float o = __shfl_xor(v, d, kWave);
        v             = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = v + __shfl_xor(v, d, kWave);
    return v;
}

// ---- wave path: NI values a lane ---------------------------------------------------------------
template <int NI>
__global__ __launch_bounds__(kBlk) void attn_softmax_wave(const Args a)
{
    const int lane    = threadIdx.x & (kWave - 1);
    const int wave    = threadIdx.x / kWave;
    const int S       = a.S;
    const float s_rcp = 1.0f / a.sp.delta, p_rcp = 1.0f / a.pp.delta;
    constexpr int kRows = kBlk / kWave;
    for (int64_t r = (int64_t) blockIdx.x * kRows + wave; r < a.rows; r += (int64_t) gridDim.x * kRows)
    {
        const Row w = row_of(a, r);
        float x[NI];
        float m = neg_inf();
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            const int j = lane + i * kWave;
            x[i]        = j < S ? score_of(a, w, w.src[j], j, s_rcp) : neg_inf();
            m           = x[i] > m ? x[i] : m;
        }
        m = wave_max(m);
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            x[i] = exp_of(x[i], m);   // an element past S is -inf here and adds +0
            acc  = i == 0 ? x[0] : acc + x[i];
        }
        const float s = wave_sum(acc);
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            const int j = lane + i * kWave;
            if (j < S)
                w.dst[j] = prob_of(a, x[i], s, p_rcp);
        }
    }
}

// ---- LDS path ----------------------------------------------------------------------------------
// floats before the first 16-byte boundary at or after p (p is 4-byte aligned), at most n
__device__ __forceinline__ int head_of(const void* p, int n)
{
    const int h = (int) ((16u - (unsigned) (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
    return h < n ? h : n;
}

__global__ __launch_bounds__(kBlk) void attn_softmax_lds(const Args a)
{
    extern __shared__ float4 lds4[];
    float* row = reinterpret_cast<float*>(lds4);   // S floats
    float* red = row + ((a.S + 3) & ~3);           // 4 floats
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int S = a.S;
    const float s_rcp = 1.0f / a.sp.delta, p_rcp = 1.0f / a.pp.delta;
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x)
    {
        const Row w = row_of(a, r);
        // pass A: the row into LDS, quantized and masked; the maximum
        float m = neg_inf();
        {
            const int head = head_of(w.src, S);
            const int nvec = (S - head) >> 2;
            const int tail = head + 4 * nvec;   // first element after the vector body
            for (int j = t; j < head; j += kBlk)
            {
                const float x = score_of(a, w, w.src[j], j, s_rcp);
                row[j]        = x;
                m             = x > m ? x : m;
            }
            for (int v = t; v < nvec; v += kBlk)
            {
                const int j = head + 4 * v;
                const F4 f  = *reinterpret_cast<const F4*>(__builtin_assume_aligned(w.src + j, 16));
#pragma unroll
                for (int k = 0; k < 4; ++k)
                {
                    const float x = score_of(a, w, f.v[k], j + k, s_rcp);
                    row[j + k]    = x;
                    m             = x > m ? x : m;
                }
            }
            for (int j = tail + t; j < S; j += kBlk)
            {
                const float x = score_of(a, w, w.src[j], j, s_rcp);
                row[j]        = x;
                m             = x > m ? x : m;
            }
        }
        m = wave_max(m);
        if (lane == 0)
            red[wave] = m;
        __syncthreads();   // the row and the four maxima are in LDS
        {
            const float m01 = red[0] > red[1] ? red[0] : red[1], m23 = red[2] > red[3] ? red[2] : red[3];
            m               = m01 > m23 ? m01 : m23;
        }
        __syncthreads();   // red is free again
        // pass B: the exponentials, summed in the documented order
        float acc = 0.0f;
        for (int j = t; j < S; j += kBlk)
        {
            const float e = exp_of(row[j], m);
            row[j]        = e;
            acc           = j == t ? e : acc + e;
        }
        acc = wave_sum(acc);
        if (lane == 0)
            red[wave] = acc;
        __syncthreads();
        const float s = (red[0] + red[1]) + (red[2] + red[3]);
        // pass C: divide, quantize, store
        {
            const int head = head_of(w.dst, S);
            const int nvec = (S - head) >> 2;
            const int tail = head + 4 * nvec;
            for (int j = t; j < head; j += kBlk)
                w.dst[j] = prob_of(a, row[j], s, p_rcp);
            for (int v = t; v < nvec; v += kBlk)
            {
                const int j = head + 4 * v;
                F4 f;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    f.v[k] = prob_of(a, row[j + k], s, p_rcp);
                *reinterpret_cast<F4*>(__builtin_assume_aligned(w.dst + j, 16)) = f;
            }
            for (int j = tail + t; j < S; j += kBlk)
                w.dst[j] = prob_of(a, row[j], s, p_rcp);
        }
        __syncthreads();   // row and red are read out before the next row overwrites them
    }
}

bool aligned4(const void* p)
{
    return (reinterpret_cast<uintptr_t>(p) & 3) == 0;
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_attn_softmax(const float* scores, float* probs, int64_t B, int64_t H, int64_t L, int64_t S,
                       const uint8_t* attn_mask, int attn_mask_per_bh, const uint8_t* key_padding_mask,
                       const aimet_tf_encoding* score_enc, const aimet_tf_encoding* prob_enc, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(B > 0 && H > 0 && L > 0 && S > 0, "attention softmax: B, H, L and S must be positive");
        AIMET_REQUIRE(S <= kMaxS, "attention softmax: a row of more than " + std::to_string(kMaxS) +
                                      " elements is not resident");
        AIMET_REQUIRE(B < (int64_t(1) << 31) && H < (int64_t(1) << 31) && L < (int64_t(1) << 31) &&
                          B * H < (int64_t(1) << 40) / L,
                      "attention softmax: too many rows (B H L must stay below 2^40)");
        require_device_ptr(scores, "attention scores");
        require_device_ptr(probs, "attention probabilities");
        if (attn_mask)
            require_device_ptr(attn_mask, "attention mask");
        if (key_padding_mask)
            require_device_ptr(key_padding_mask, "key padding mask");
        AIMET_REQUIRE(aligned4(scores) && aligned4(probs), "attention softmax: misaligned pointer");
        Args a {};
        a.scores = scores, a.probs = probs, a.attn_mask = attn_mask, a.kpm = key_padding_mask;
        a.rows = B * H * L, a.L = L, a.H = H, a.S = (int) S;
        a.per_bh    = attn_mask_per_bh != 0;
        a.score_qdq = score_enc != nullptr, a.prob_qdq = prob_enc != nullptr;
        a.sp = a.pp = QdqParams {0.0f, 0.0f, 1.0f, 0.0f};
        if (score_enc)
            a.sp = tensor_params(*score_enc);
        if (prob_enc)
            a.pp = tensor_params(*prob_enc);
        hipStream_t s = as_stream(stream);
        if (S <= kWaveMaxS)
        {
            const unsigned grid = (unsigned) std::min<int64_t>(ceil_div(a.rows, kBlk / kWave), kMaxGrid);
            const int64_t ni    = ceil_div(S, kWave);
            if (ni <= 1)
                attn_softmax_wave<1><<<grid, kBlk, 0, s>>>(a);
            else if (ni <= 2)
                attn_softmax_wave<2><<<grid, kBlk, 0, s>>>(a);
            else if (ni <= 4)
                attn_softmax_wave<4><<<grid, kBlk, 0, s>>>(a);
            else if (ni <= 8)
                attn_softmax_wave<8><<<grid, kBlk, 0, s>>>(a);
            else
                attn_softmax_wave<16><<<grid, kBlk, 0, s>>>(a);
        }
        else
        {
            const unsigned grid = (unsigned) std::min<int64_t>(a.rows, kMaxGrid);
            const size_t lds    = (size_t) ((S + 3) & ~int64_t(3)) * 4 + 16;
            attn_softmax_lds<<<grid, kBlk, lds, s>>>(a);
        }
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int64_t aimet_attn_softmax_max_s(void)
{
    return kMaxS;
}

int aimet_attn_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
