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
// row's address; a lane's loads are all issued before the first is used. LDS path: 16-byte global loads and stores on the aligned body of the row, with a
// scalar head of up to three floats and a scalar tail, separately for source and destination (S is
// often odd, so consecutive rows have different alignments); the fixed-order sum then reads LDS by
// element index. 64-bit offsets throughout; rows are taken in a grid-stride loop. In place
// (probs == scores) is safe on both paths: a row is read completely before any of it is written.
//
// Backward (aimet_attn_softmax_backward): the straight-through gradient of the chain above for fixed
// encodings, one launch, from the raw scores and the gradient g arriving at the quantized
// probabilities. The row is recomputed with the forward's own device functions (score_of, exp_of,
// unq_prob, wave_row_exp, lds_row_exp), so p_j below is the forward's pre-QDQ probability bit for bit:
//   G_j  = (pmin <= p_j <= pmax) ? g_j : 0         prob_enc's STE; null prob_enc: G_j = g_j
//   d    = sum_j G_j p_j                           each product rounded, summed in the ORDER ABOVE for this S
//   t_j  = (G_j - d) p_j                           torch's _softmax_backward_data form
//   dx_j = masked(j) ? 0 : ((smin <= x_j <= smax) ? t_j : 0)     x_j the RAW score; null score_enc: no test
// smin / smax / pmin / pmax are the encodings' min / max rounded to float32 (what compute_dloss_by_dx
// compares against), not the grid ends. A masked position is exactly 0, also in a fully masked row
// (whose p is NaN).
//   Wave path: e and g both stay in registers (2 NI values a lane) with the NI keep bits (not masked and
//     the raw score in range) in one more; scores, grad_probs and grad_scores are touched once each.
//   LDS path: p in LDS, and g is READ AGAIN instead of held in a second LDS array. At S = kMaxS the row
//     of p alone fills the 64 KiB, so a second array (and the keep flags beside it) would serve short rows
//     only and long rows would need this form anyway; one form for every S is what is built. Pass D
//     reads g by element index (dword t of each 256-dword group: coalesced, and the thread-to-element
//     map is the documented order without staging g in LDS) and leaves p in LDS; pass T writes
//     grad_scores in 16-byte stores on its own aligned body (scalar head and tail) and reads g, the raw
//     score and the mask bytes of the elements it writes again -- 16-byte loads where that pointer is
//     aligned at the body, dword loads otherwise. The second reads follow the first by one row pass of the
//     same workgroup, so they are expected from L2 (12 B an element from HBM; not confirmed by a counter run).
//   grad_scores may be grad_probs (or scores) itself: on the wave path the row is in registers before
//   the first store; in pass T a thread reads exactly the elements it then writes.

#include "common.hpp"
#include "io16.hpp"
#include "reduce.hpp"
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
    // backward only: probs is grad_scores
    const float* grad;   // the gradient at the quantized probabilities
    float smin, smax, pmin, pmax;
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
    const float* g;       // backward: this row of grad_probs
};

__device__ __forceinline__ Row row_of(const Args& a, int64_t r)
{
    const int64_t bh = r / a.L, l = r - bh * a.L, b = bh / a.H;
    Row w;
    w.src = a.scores + r * a.S;
    w.dst = a.probs + r * a.S;
    w.am  = a.attn_mask ? a.attn_mask + ((a.per_bh ? bh : 0) * a.L + l) * a.S : nullptr;
    w.kpm = a.kpm ? a.kpm + b * a.S : nullptr;
    w.g   = a.grad ? a.grad + r * a.S : nullptr;
    return w;
}

__device__ __forceinline__ float neg_inf()
{
    return -__builtin_huge_valf();
}

__device__ __forceinline__ bool masked_at(const Row& w, int j)
{
    return (w.am && w.am[j]) || (w.kpm && w.kpm[j]);
}

// steps 1 and 2 for element j of a row
__device__ __forceinline__ float score_of(const Args& a, const Row& w, float x, int j, float s_rcp)
{
    if (a.score_qdq)
        x = dequantize(quantize_nearest_rcp(x, a.sp, s_rcp), a.sp);
    if (masked_at(w, j))
        x = neg_inf();
    return x;
}

__device__ __forceinline__ float exp_of(float x, float m)
{
    return x == neg_inf() ? 0.0f : rnn_math::exp_r(x - m);
}

// the probability before its QDQ
__device__ __forceinline__ float unq_prob(float e, float s)
{
    return e / s;
}

__device__ __forceinline__ float prob_of(const Args& a, float e, float s, float p_rcp)
{
    const float p = unq_prob(e, s);
    return a.prob_qdq ? dequantize(quantize_nearest_rcp(p, a.pp, p_rcp), a.pp) : p;
}

// backward: G_j, and whether element j (raw score x) passes a gradient on at all
__device__ __forceinline__ float ste_prob(const Args& a, float p, float g)
{
    return (a.prob_qdq && !(p >= a.pmin && p <= a.pmax)) ? 0.0f : g;
}

__device__ __forceinline__ bool kept(const Args& a, const Row& w, int j, float x)
{
    return !masked_at(w, j) && (!a.score_qdq || (x >= a.smin && x <= a.smax));
}

// `o > v ? o : v`: a NaN in another lane is never taken
__device__ __forceinline__ float wave_max(float v)
{
    return wave_all(v, [](float v, float o) { return o > v ? o : v; });
}

__device__ __forceinline__ float wave_sum(float v)
{
    return wave_all(v, [](float v, float o) { return v + o; });
}

// ---- wave path: NI values a lane ---------------------------------------------------------------
// Lane `lane`'s NI values of row w into x as e_j (an element past S: 0); returns s. raw(i, j, score)
// sees every raw score the lane loads.
template <int NI, class Raw>
__device__ __forceinline__ float wave_row_exp(const Args& a, const Row& w, int lane, float s_rcp, float (&x)[NI],
                                              Raw raw)
{
    const int S = a.S;
    // The lane's NI loads are issued before the first value is used, without a branch: an element
    // past S re-reads the row's last one (in bounds) and is discarded below.
#pragma unroll
    for (int i = 0; i < NI; ++i)
    {
        const int j = lane + i * kWave;
        x[i]        = w.src[j < S ? j : S - 1];
    }
    float m = neg_inf();
#pragma unroll
    for (int i = 0; i < NI; ++i)
    {
        const int j = lane + i * kWave;
        if (j < S)
        {
            raw(i, j, x[i]);
            x[i] = score_of(a, w, x[i], j, s_rcp);
        }
        else
            x[i] = neg_inf();
        m = x[i] > m ? x[i] : m;
    }
    m = wave_max(m);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
    {
        x[i] = exp_of(x[i], m);   // an element past S is -inf here and adds +0
        acc  = i == 0 ? x[0] : acc + x[i];
    }
    return wave_sum(acc);
}

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
        const float s = wave_row_exp<NI>(a, w, lane, s_rcp, x, [](int, int, float) {});
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            const int j = lane + i * kWave;
            if (j < S)
                w.dst[j] = prob_of(a, x[i], s, p_rcp);
        }
    }
}

template <int NI>
__global__ __launch_bounds__(kBlk) void attn_softmax_bwd_wave(const Args a)
{
    const int lane    = threadIdx.x & (kWave - 1);
    const int wave    = threadIdx.x / kWave;
    const int S       = a.S;
    const float s_rcp = 1.0f / a.sp.delta;
    constexpr int kRows = kBlk / kWave;
    for (int64_t r = (int64_t) blockIdx.x * kRows + wave; r < a.rows; r += (int64_t) gridDim.x * kRows)
    {
        const Row w = row_of(a, r);
        float g[NI], p[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i)   // in flight together with the scores
        {
            const int j = lane + i * kWave;
            g[i]        = j < S ? w.g[j] : 0.0f;
        }
        unsigned keep = 0;   // bit i: element i is not masked and its raw score is in range
        const float s = wave_row_exp<NI>(a, w, lane, s_rcp, p,
                                         [&](int i, int j, float x) { keep |= (unsigned) kept(a, w, j, x) << i; });
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            p[i]           = unq_prob(p[i], s);
            g[i]           = ste_prob(a, p[i], g[i]);
            const float gp = g[i] * p[i];   // past S: 0 * 0 (NaN in a fully masked row, which writes zeros)
            acc            = i == 0 ? gp : acc + gp;
        }
        const float d = wave_sum(acc);
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            const int j = lane + i * kWave;
            if (j < S)
                w.dst[j] = (keep >> i & 1u) ? (g[i] - d) * p[i] : 0.0f;
        }
    }
}

// ---- LDS path ----------------------------------------------------------------------------------
// Row w into `row` as e_j; returns s. `red` holds four floats; the caller puts a barrier between its
// last read of row / red and the next call.
__device__ __forceinline__ float lds_row_exp(const Args& a, const Row& w, float* row, float* red, float s_rcp)
{
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int S = a.S;
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
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kBlk) void attn_softmax_lds(const Args a)
{
    extern __shared__ float4 lds4[];
    float* row = reinterpret_cast<float*>(lds4);   // S floats
    float* red = row + ((a.S + 3) & ~3);           // 4 floats
    const int t = threadIdx.x;
    const int S = a.S;
    const float s_rcp = 1.0f / a.sp.delta, p_rcp = 1.0f / a.pp.delta;
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x)
    {
        const Row w   = row_of(a, r);
        const float s = lds_row_exp(a, w, row, red, s_rcp);
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

// four consecutive floats from p: one 16-byte load where p is aligned, four dword loads otherwise
__device__ __forceinline__ F4 load4(const float* p, bool vec)
{
    if (vec)
        return *reinterpret_cast<const F4*>(__builtin_assume_aligned(p, 16));
    F4 f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        f.v[k] = p[k];
    return f;
}

__device__ __forceinline__ float dx_of(const Args& a, const Row& w, int j, float p, float d)
{
    return kept(a, w, j, w.src[j]) ? (ste_prob(a, p, w.g[j]) - d) * p : 0.0f;
}

__global__ __launch_bounds__(kBlk) void attn_softmax_bwd_lds(const Args a)
{
    extern __shared__ float4 lds4[];
    float* row = reinterpret_cast<float*>(lds4);   // S floats
    float* red = row + ((a.S + 3) & ~3);           // 4 floats
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int S = a.S;
    const float s_rcp = 1.0f / a.sp.delta;
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x)
    {
        const Row w   = row_of(a, r);
        const float s = lds_row_exp(a, w, row, red, s_rcp);
        __syncthreads();   // every thread has its s before red takes the partial sums of d
        // pass D: p into LDS (thread t owns t, t + 256, ... here as in pass B) and d in the order of s
        float acc = 0.0f;
        for (int j = t; j < S; j += kBlk)
        {
            const float p  = unq_prob(row[j], s);
            row[j]         = p;
            const float gp = ste_prob(a, p, w.g[j]) * p;
            acc            = j == t ? gp : acc + gp;
        }
        acc = wave_sum(acc);
        if (lane == 0)
            red[wave] = acc;
        __syncthreads();   // p and the four partial sums are in LDS
        const float d = (red[0] + red[1]) + (red[2] + red[3]);
        // pass T: the gradient, stored on the destination's aligned body
        {
            const int head = head_of(w.dst, S);
            const int nvec = (S - head) >> 2;
            const int tail = head + 4 * nvec;
            const bool g_vec = (reinterpret_cast<uintptr_t>(w.g + head) & 15u) == 0;
            const bool x_vec = (reinterpret_cast<uintptr_t>(w.src + head) & 15u) == 0;
            for (int j = t; j < head; j += kBlk)
                w.dst[j] = dx_of(a, w, j, row[j], d);
            for (int v = t; v < nvec; v += kBlk)
            {
                const int j = head + 4 * v;
                const F4 g = load4(w.g + j, g_vec), x = load4(w.src + j, x_vec);
                F4 f;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    f.v[k] = kept(a, w, j + k, x.v[k]) ? (ste_prob(a, row[j + k], g.v[k]) - d) * row[j + k] : 0.0f;
                *reinterpret_cast<F4*>(__builtin_assume_aligned(w.dst + j, 16)) = f;
            }
            for (int j = tail + t; j < S; j += kBlk)
                w.dst[j] = dx_of(a, w, j, row[j], d);
        }
        __syncthreads();   // row and red are read out before the next row overwrites them
    }
}

bool aligned4(const void* p)
{
    return (reinterpret_cast<uintptr_t>(p) & 3) == 0;
}

// The checks both entry points share, and the kernel arguments but for the float tensors after `scores`.
Args checked_args(const float* scores, int64_t B, int64_t H, int64_t L, int64_t S, const uint8_t* attn_mask,
                  int attn_mask_per_bh, const uint8_t* key_padding_mask, const aimet_tf_encoding* score_enc,
                  const aimet_tf_encoding* prob_enc)
{
    AIMET_REQUIRE(B > 0 && H > 0 && L > 0 && S > 0, "attention softmax: B, H, L and S must be positive");
    AIMET_REQUIRE(S <= kMaxS, "attention softmax: a row of more than " + std::to_string(kMaxS) +
                                  " elements is not resident");
    AIMET_REQUIRE(B < (int64_t(1) << 31) && H < (int64_t(1) << 31) && L < (int64_t(1) << 31) &&
                      B * H < (int64_t(1) << 40) / L,
                  "attention softmax: too many rows (B H L must stay below 2^40)");
    require_device_ptr(scores, "attention scores");
    if (attn_mask)
        require_device_ptr(attn_mask, "attention mask");
    if (key_padding_mask)
        require_device_ptr(key_padding_mask, "key padding mask");
    Args a {};
    a.scores = scores, a.attn_mask = attn_mask, a.kpm = key_padding_mask;
    a.rows = B * H * L, a.L = L, a.H = H, a.S = (int) S;
    a.per_bh    = attn_mask_per_bh != 0;
    a.score_qdq = score_enc != nullptr, a.prob_qdq = prob_enc != nullptr;
    a.sp = a.pp = QdqParams {0.0f, 0.0f, 1.0f, 0.0f};
    if (score_enc)
        a.sp = tensor_params(*score_enc), a.smin = (float) score_enc->min, a.smax = (float) score_enc->max;
    if (prob_enc)
        a.pp = tensor_params(*prob_enc), a.pmin = (float) prob_enc->min, a.pmax = (float) prob_enc->max;
    return a;
}

using Kernel = void (*)(Args);

// wave[k] holds 2^k values a lane
void launch_rows(const Args& a, const Kernel (&wave)[5], Kernel lds, hipStream_t s)
{
    if (a.S <= kWaveMaxS)
    {
        const unsigned grid = (unsigned) std::min<int64_t>(ceil_div(a.rows, kBlk / kWave), kMaxGrid);
        int k               = 0;
        while ((kWave << k) < a.S)
            ++k;
        wave[k]<<<grid, kBlk, 0, s>>>(a);
    }
    else
    {
        const unsigned grid = (unsigned) std::min<int64_t>(a.rows, kMaxGrid);
        const size_t bytes  = (size_t) ((a.S + 3) & ~3) * 4 + 16;
        lds<<<grid, kBlk, bytes, s>>>(a);
    }
    AIMET_LAUNCH_CHECK();
}

LaunchCounter g_backward_launches;

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_attn_softmax(const float* scores, float* probs, int64_t B, int64_t H, int64_t L, int64_t S,
                       const uint8_t* attn_mask, int attn_mask_per_bh, const uint8_t* key_padding_mask,
                       const aimet_tf_encoding* score_enc, const aimet_tf_encoding* prob_enc, void* stream)
{
    return guarded([&] {
        Args a = checked_args(scores, B, H, L, S, attn_mask, attn_mask_per_bh, key_padding_mask, score_enc, prob_enc);
        require_device_ptr(probs, "attention probabilities");
        AIMET_REQUIRE(aligned4(scores) && aligned4(probs), "attention softmax: misaligned pointer");
        a.probs = probs;
        launch_rows(a, {attn_softmax_wave<1>, attn_softmax_wave<2>, attn_softmax_wave<4>, attn_softmax_wave<8>,
                        attn_softmax_wave<16>}, attn_softmax_lds, as_stream(stream));
        g_launches.add(1);
    });
}

int aimet_attn_softmax_backward(const float* scores, const float* grad_probs, float* grad_scores, int64_t B, int64_t H,
                                int64_t L, int64_t S, const uint8_t* attn_mask, int attn_mask_per_bh,
                                const uint8_t* key_padding_mask, const aimet_tf_encoding* score_enc,
                                const aimet_tf_encoding* prob_enc, void* stream)
{
    return guarded([&] {
        Args a = checked_args(scores, B, H, L, S, attn_mask, attn_mask_per_bh, key_padding_mask, score_enc, prob_enc);
        require_device_ptr(grad_probs, "gradient of the attention probabilities");
        require_device_ptr(grad_scores, "gradient of the attention scores");
        AIMET_REQUIRE(aligned4(scores) && aligned4(grad_probs) && aligned4(grad_scores),
                      "attention softmax: misaligned pointer");
        a.grad = grad_probs, a.probs = grad_scores;
        launch_rows(a, {attn_softmax_bwd_wave<1>, attn_softmax_bwd_wave<2>, attn_softmax_bwd_wave<4>,
                        attn_softmax_bwd_wave<8>, attn_softmax_bwd_wave<16>}, attn_softmax_bwd_lds, as_stream(stream));
        g_backward_launches.add(1);
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

int aimet_attn_backward_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_backward_launches.read(count, reset); });
}

}   // extern "C"
