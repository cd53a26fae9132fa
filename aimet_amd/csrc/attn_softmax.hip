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
//
// Range learning (aimet_attn_softmax_lg, aimet_attn_softmax_lg_backward): the same rows with both
// quantizers on learned grids, the element arithmetic of lg_core.hpp (calculate_forward_pass,
// asymmetric_gradients / symmetric_gradients; round half to even). wave_row_exp and lds_row_exp are
// templates over their argument record and find score_of by overload: Args gives the static kernels
// what they were, LgRowArgs the learned grid.
//   Forward: a quantizer's trainable range arrives as two device pointers; every thread computes delta and
//     offset with LgEnc::of, x_j = lg_qdq(scores_j), then masks, m, e_j, s, p_j as above, probs_j =
//     lg_qdq(p_j). One thread stores each quantizer's {delta, offset, min, max} for the backward. The
//     host reads nothing back. Out of place.
//   Backward, per element that is not masked (a masked one gets exactly 0 and adds to no sum):
//     q = p_j / delta_p (lg_quot), m_p its in-grid mask: G_j = m_p g_j, and the probability quantizer's
//       {A, B, D} terms of lg_bwd_term_m with gradient g_j
//     d = sum_j G_j p_j in the ORDER ABOVE, t_j = (G_j - d) p_j
//     q = scores_j / delta_s, m_s: dx_j = m_s t_j, and the score quantizer's {A, B, D} terms with gradient t_j
//   A lane carries its six sums over the rows of its grid-stride loop (rows in increasing index, a
//   row's elements in increasing j); block_fold_own makes the workgroup's partial. The partials go to a
//   scratch block and a SECOND LAUNCH of one workgroup folds them -- lane l adds partials l, l + 256, ...
//   in increasing index, then the same tree -- and applies range_grads_one on the saved range of each
//   quantizer. (The per-tensor learned-grid backward folds the same way; its fold in the last workgroup
//   to arrive measured slower than the launch, learned_grid.hip.) No atomics: equal inputs, equal bits.
//   Wave path: g, p and the raw score in registers (3 NI values a lane) and NI live bits. LDS path: p in
//   LDS and g read again as above; pass T keeps pass D's thread-to-element map with dword accesses, so
//   the order of every sum is independent of the row's alignment.

#include "common.hpp"
#include "io16.hpp"
#include "lg_core.hpp"
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

// Range learning: one quantizer's grid as a kernel holds it. delta and offset come from the device --
// LgEnc::of on the trainable range in the forward, the forward's four saved floats in the backward.
struct LgGrid
{
    float d, o, steps, rd;   // rd = lg_recip(d)
    int on;                  // 0: no quantizer
    int mode;                // lg_bwd_term's: 1 symmetric_gradients, 2 asymmetric_gradients
};

// what the row functions below read of their `a` on the range-learning kernels
struct LgRowArgs
{
    int S;
    LgGrid sq;
};

// steps 1 and 2 on a learned grid (calculate_forward_pass: round half to even)
__device__ __forceinline__ float score_of(const LgRowArgs& a, const Row& w, float x, int j, float)
{
    if (a.sq.on)
        x = lg_qdq(x, a.sq.d, a.sq.o, a.sq.steps, a.sq.rd);
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
template <int NI, class A, class Raw>
__device__ __forceinline__ float wave_row_exp(const A& a, const Row& w, int lane, float s_rcp, float (&x)[NI],
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
template <class A>
__device__ __forceinline__ float lds_row_exp(const A& a, const Row& w, float* row, float* red, float s_rcp)
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

// ---- range learning: aimet_attn_softmax_lg / aimet_attn_softmax_lg_backward ---------------------------
// The same rows on learned grids (header comment, "Range learning"). Both kernels of a pair take
// LgArgs: the tensors, masks and shape in `a` (its static-grid fields unused) and one LgEnc a
// quantizer, emin == nullptr where there is none; delta_out / offset_out / range_out are the four
// saved floats {delta, offset, min, max} -- written by the forward, read by the backward.
struct LgArgs
{
    Args a;
    LgEnc se, pe;
    float* partial;   // backward: six sums a workgroup
};

// forward: the grid from the trainable range as it stands on the device; one thread of the launch
// saves it for the backward
__device__ __forceinline__ LgGrid grid_of_range(const LgEnc& e, bool save)
{
    LgGrid g {1.0f, 0.0f, 0.0f, 1.0f, 0, 0};
    if (e.emin == nullptr)
        return g;
    const float mn = e.emin[0], mx = e.emax[0];
    e.of(mn, mx, g.d, g.o);
    if (save)
    {
        e.delta_out[0]  = g.d;
        e.offset_out[0] = g.o;
        e.range_out[0]  = mn;
        e.range_out[1]  = mx;
    }
    g.steps = e.steps, g.rd = lg_recip(g.d), g.on = 1, g.mode = e.mode == 2 ? 2 : 1;
    return g;
}

// backward: the grid the forward saved
__device__ __forceinline__ LgGrid grid_saved(const LgEnc& e)
{
    LgGrid g {1.0f, 0.0f, 0.0f, 1.0f, 0, 0};
    if (e.emin == nullptr)
        return g;
    g.d = e.delta_out[0], g.o = e.offset_out[0];
    g.steps = e.steps, g.rd = lg_recip(g.d), g.on = 1, g.mode = e.mode == 2 ? 2 : 1;
    return g;
}

__device__ __forceinline__ float lg_prob_of(const LgGrid& pq, float e, float s)
{
    const float p = unq_prob(e, s);
    return pq.on ? lg_qdq(p, pq.d, pq.o, pq.steps, pq.rd) : p;
}

template <int NI>
__global__ __launch_bounds__(kBlk) void attn_softmax_lg_wave(const LgArgs k)
{
    const int lane  = threadIdx.x & (kWave - 1);
    const int wave  = threadIdx.x / kWave;
    const int S     = k.a.S;
    const bool save = blockIdx.x == 0 && threadIdx.x == 0;
    const LgRowArgs a {S, grid_of_range(k.se, save)};
    const LgGrid pq = grid_of_range(k.pe, save);
    constexpr int kRows = kBlk / kWave;
    for (int64_t r = (int64_t) blockIdx.x * kRows + wave; r < k.a.rows; r += (int64_t) gridDim.x * kRows)
    {
        const Row w = row_of(k.a, r);
        float x[NI];
        const float s = wave_row_exp<NI>(a, w, lane, 0.0f, x, [](int, int, float) {});
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            const int j = lane + i * kWave;
            if (j < S)
                w.dst[j] = lg_prob_of(pq, x[i], s);
        }
    }
}

__global__ __launch_bounds__(kBlk) void attn_softmax_lg_lds(const LgArgs k)
{
    extern __shared__ float4 lds4[];
    float* row = reinterpret_cast<float*>(lds4);   // S floats
    float* red = row + ((k.a.S + 3) & ~3);         // 4 floats
    const int t = threadIdx.x;
    const int S = k.a.S;
    const bool save = blockIdx.x == 0 && t == 0;
    const LgRowArgs a {S, grid_of_range(k.se, save)};
    const LgGrid pq = grid_of_range(k.pe, save);
    for (int64_t r = blockIdx.x; r < k.a.rows; r += gridDim.x)
    {
        const Row w   = row_of(k.a, r);
        const float s = lds_row_exp(a, w, row, red, 0.0f);
        // pass C: divide, quantize, store (attn_softmax_lds's, on the learned grid)
        const int head = head_of(w.dst, S);
        const int nvec = (S - head) >> 2;
        const int tail = head + 4 * nvec;
        for (int j = t; j < head; j += kBlk)
            w.dst[j] = lg_prob_of(pq, row[j], s);
        for (int v = t; v < nvec; v += kBlk)
        {
            const int j = head + 4 * v;
            F4 f;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                f.v[c] = lg_prob_of(pq, row[j + c], s);
            *reinterpret_cast<F4*>(__builtin_assume_aligned(w.dst + j, 16)) = f;
        }
        for (int j = tail + t; j < S; j += kBlk)
            w.dst[j] = lg_prob_of(pq, row[j], s);
        __syncthreads();   // row and red are read out before the next row overwrites them
    }
}

// The backward's six sums: {A, B, D} of lg_bwd_term_m for the score quantizer and for the probability
// quantizer. A lane carries its own across the rows of its grid-stride loop.
struct LgSums
{
    Sums s, p;
};

__device__ __forceinline__ LgSums add_sums(LgSums x, const LgSums& y)
{
    x.s.a += y.s.a, x.s.b += y.s.b, x.s.d += y.s.d;
    x.p.a += y.p.a, x.p.b += y.p.b, x.p.d += y.p.d;
    return x;
}

// x / delta as lg_bwd_elem forms it
__device__ __forceinline__ float lg_quotient(const LgGrid& q, float x)
{
    return lg_fast_enc(q.o, q.rd) ? lg_quot(x, q.d, q.rd) : x / q.d;
}

// lg_grad's result alone (in-grid mask * g, lg_bwd_term_m's expressions), for a pass whose terms are
// already in the sums
__device__ __forceinline__ float lg_masked_grad(const LgGrid& q, float x, float g)
{
    if (!q.on)
        return g;
    const float xr = __builtin_rintf(lg_quotient(q, x)) - q.o;
    return (__builtin_amdgcn_fmed3f(xr, 0.0f, q.steps) == xr ? 1.0f : 0.0f) * g;
}

// One quantizer's backward at x for the gradient g arriving at its output: the gradient passed on
// (in-grid mask * g) and the element's terms added to t. No quantizer: g, nothing added.
__device__ __forceinline__ float lg_grad(const LgGrid& q, float x, float g, Sums& t)
{
    if (!q.on)
        return g;
    const float qt = lg_quotient(q, x);
    // Both modes' terms of the element (they share the quotient, the rounding and the mask), then one
    // select a sum: 0 + term is the term, so the sums are those of lg_bwd_term adding in place. With
    // the mode known only at run time, lg_bwd_term's branches were merged by the compiler into one add
    // at a computed address, which put the running sums in private memory.
    Sums sym {0.0f, 0.0f, 0.0f}, asym {0.0f, 0.0f, 0.0f};
    float gx;
    lg_bwd_term_m<1>(x, qt, g, q.o, q.steps, gx, sym);
    lg_bwd_term_m<2>(x, qt, g, q.o, q.steps, gx, asym);
    const bool two = q.mode == 2;
    t.a += two ? asym.a : sym.a;
    t.b += two ? asym.b : sym.b;
    t.d += two ? asym.d : sym.d;
    return gx;
}

// the workgroup's six sums (wave butterfly, then thread 0 folds waves 1..3) as its partial
__device__ __forceinline__ void publish_sums(const LgSums& acc, LgSums* fold, float* partial)
{
    const LgSums t = block_fold_own<kBlk / kWave>(acc, fold, add_sums);
    if (threadIdx.x == 0)
    {
        float* p = partial + 6 * (size_t) blockIdx.x;
        p[0] = t.s.a, p[1] = t.s.b, p[2] = t.s.d;
        p[3] = t.p.a, p[4] = t.p.b, p[5] = t.p.d;
    }
}

template <int NI>
__global__ __launch_bounds__(kBlk) void attn_softmax_lg_bwd_wave(const LgArgs k)
{
    __shared__ LgSums fold[kBlk / kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int S    = k.a.S;
    const LgRowArgs a {S, grid_saved(k.se)};
    const LgGrid pq = grid_saved(k.pe);
    Sums accs {0.0f, 0.0f, 0.0f}, accp {0.0f, 0.0f, 0.0f};   // this lane's, over all its rows
    constexpr int kRows = kBlk / kWave;
    for (int64_t r = (int64_t) blockIdx.x * kRows + wave; r < k.a.rows; r += (int64_t) gridDim.x * kRows)
    {
        const Row w = row_of(k.a, r);
        float g[NI], p[NI], xr[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i)   // in flight together with the scores
        {
            const int j = lane + i * kWave;
            g[i]        = j < S ? w.g[j] : 0.0f;
            xr[i]       = 0.0f;
        }
        unsigned live = 0;   // bit i: element i exists and is not masked
        const float s = wave_row_exp<NI>(a, w, lane, 0.0f, p, [&](int i, int j, float x) {
            xr[i] = x;
            live |= (unsigned) !masked_at(w, j) << i;
        });
        float dacc = 0.0f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            p[i]           = unq_prob(p[i], s);
            g[i]           = (live >> i & 1u) ? lg_grad(pq, p[i], g[i], accp) : 0.0f;   // G_j
            const float gp = g[i] * p[i];   // masked or past S: 0 * 0 (NaN in a fully masked row, which writes zeros)
            dacc           = i == 0 ? gp : dacc + gp;
        }
        const float d = wave_sum(dacc);
#pragma unroll
        for (int i = 0; i < NI; ++i)
        {
            const int j = lane + i * kWave;
            if (j < S)
                w.dst[j] = (live >> i & 1u) ? lg_grad(a.sq, xr[i], (g[i] - d) * p[i], accs) : 0.0f;
        }
    }
    if (k.partial)   // null: neither quantizer is present, nothing to fold
        publish_sums(LgSums {accs, accp}, fold, k.partial);
}

// LDS path: p in LDS and g read again, as attn_softmax_bwd_lds; pass T keeps pass D's thread-to-element
// map (dword t of each 256-dword group, loads and stores), so every element's terms are added by the
// same lane in the same order whatever the row's alignment, and a thread reads exactly what it writes.
__global__ __launch_bounds__(kBlk) void attn_softmax_lg_bwd_lds(const LgArgs k)
{
    extern __shared__ float4 lds4[];
    float* row = reinterpret_cast<float*>(lds4);   // S floats
    float* red = row + ((k.a.S + 3) & ~3);         // 4 floats
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const int S = k.a.S;
    const LgRowArgs a {S, grid_saved(k.se)};
    const LgGrid pq = grid_saved(k.pe);
    Sums accs {0.0f, 0.0f, 0.0f}, accp {0.0f, 0.0f, 0.0f};   // this thread's, over all its rows
    for (int64_t r = blockIdx.x; r < k.a.rows; r += gridDim.x)
    {
        const Row w   = row_of(k.a, r);
        const float s = lds_row_exp(a, w, row, red, 0.0f);
        __syncthreads();   // every thread has its s before red takes the partial sums of d
        // pass D: p into LDS, the probability quantizer's terms, and d in the order of s
        float dacc = 0.0f;
        for (int j = t; j < S; j += kBlk)
        {
            const float p  = unq_prob(row[j], s);
            row[j]         = p;
            const float G  = masked_at(w, j) ? 0.0f : lg_grad(pq, p, w.g[j], accp);
            const float gp = G * p;
            dacc           = j == t ? gp : dacc + gp;
        }
        dacc = wave_sum(dacc);
        if (lane == 0)
            red[wave] = dacc;
        __syncthreads();   // p and the four partial sums are in LDS
        const float d = (red[0] + red[1]) + (red[2] + red[3]);
        // pass T: G_j once more (its terms are pass D's), the score quantizer's terms, dx
        for (int j = t; j < S; j += kBlk)
        {
            float dx = 0.0f;
            if (!masked_at(w, j))
            {
                const float p = row[j];
                const float G = lg_masked_grad(pq, p, w.g[j]);
                dx            = lg_grad(a.sq, w.src[j], (G - d) * p, accs);
            }
            w.dst[j] = dx;
        }
        __syncthreads();   // row and red are read out before the next row overwrites them
    }
    if (k.partial)
        publish_sums(LgSums {accs, accp}, reinterpret_cast<LgSums*>(row), k.partial);   // the row is free: S > 1024 floats
}

// The backward's second launch, one workgroup: lane l adds the partials l, l + 256, ... in increasing
// index, then publish_sums' tree; thread 0 turns the six sums into the four range gradients.
__global__ __launch_bounds__(kBlk) void attn_lg_fold(const float* __restrict__ partial, unsigned nparts, LgRange rs,
                                                     LgRange rp)
{
    __shared__ LgSums fold[kBlk / kWave];
    LgSums acc {};
    for (unsigned i = threadIdx.x; i < nparts; i += kBlk)
    {
        const float* p = partial + 6 * (size_t) i;
        acc            = add_sums(acc, LgSums {{p[0], p[1], p[2]}, {p[3], p[4], p[5]}});
    }
    const LgSums t = block_fold_own<kBlk / kWave>(acc, fold, add_sums);
    if (threadIdx.x == 0)
    {
        if (rs.gmin)
            range_grads_one(t.s.a, t.s.b, t.s.d, 0, rs);
        if (rp.gmin)
            range_grads_one(t.p.a, t.p.b, t.p.d, 0, rp);
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

template <class KA>
using Kernel = void (*)(KA);

// the workgroups launch_rows starts for this shape
unsigned row_grid(const Args& a)
{
    return (unsigned) std::min<int64_t>(a.S <= kWaveMaxS ? ceil_div(a.rows, kBlk / kWave) : a.rows, kMaxGrid);
}

// wave[k] holds 2^k values a lane; ka: the kernels' argument, a: the shape in it
template <class KA>
void launch_rows(const KA& ka, const Args& a, const Kernel<KA> (&wave)[5], Kernel<KA> lds, hipStream_t s)
{
    const unsigned grid = row_grid(a);
    if (a.S <= kWaveMaxS)
    {
        int k = 0;
        while ((kWave << k) < a.S)
            ++k;
        wave[k]<<<grid, kBlk, 0, s>>>(ka);
    }
    else
    {
        const size_t bytes = (size_t) ((a.S + 3) & ~3) * 4 + 16;
        lds<<<grid, kBlk, bytes, s>>>(ka);
    }
    AIMET_LAUNCH_CHECK();
}

LaunchCounter g_backward_launches;
LaunchCounter g_lg_launches, g_lg_backward_launches;

// One quantizer of the range-learning entries as the kernels take it. forward: the grid from the
// trainable range, `saved` written; backward: the range pointers of `grid` are not read, the encoding
// is the saved one (LgEnc's pointers are not const: the forward writes through them).
LgEnc lg_enc_of(const aimet_attn_lg_grid* grid, const float* saved, bool forward)
{
    if (grid == nullptr)
        return LgEnc {};
    require_device_ptr(saved, "saved encoding");
    float* sv = const_cast<float*>(saved);
    return enc_of(forward ? grid->encoding_min : sv + 2, forward ? grid->encoding_max : sv + 3, 1, 0, grid->bitwidth,
                  grid->use_symmetric, grid->use_strict_symmetric, grid->is_unsigned_symmetric, sv, sv + 1, sv + 2);
}

// the range gradients of one quantizer from its saved encoding: range_grad[0] = min's, [1] = max's
LgRange lg_range_of(const LgEnc& e, float* range_grad)
{
    if (e.emin == nullptr)
        return LgRange {};
    require_device_ptr(range_grad, "range gradient");
    return LgRange {e.range_out, e.range_out + 1, e.delta_out, range_grad, range_grad + 1, e.steps, e.half_floor,
                    e.mode != 2};
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
        Args a = checked_args(scores, B, H, L, S, attn_mask, attn_mask_per_bh, key_padding_mask, score_enc, prob_enc);
        require_device_ptr(probs, "attention probabilities");
        AIMET_REQUIRE(aligned4(scores) && aligned4(probs), "attention softmax: misaligned pointer");
        a.probs = probs;
        launch_rows<Args>(a, a, {attn_softmax_wave<1>, attn_softmax_wave<2>, attn_softmax_wave<4>,
                                 attn_softmax_wave<8>, attn_softmax_wave<16>}, attn_softmax_lds, as_stream(stream));
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
        launch_rows<Args>(a, a, {attn_softmax_bwd_wave<1>, attn_softmax_bwd_wave<2>, attn_softmax_bwd_wave<4>,
                                 attn_softmax_bwd_wave<8>, attn_softmax_bwd_wave<16>}, attn_softmax_bwd_lds,
                          as_stream(stream));
        g_backward_launches.add(1);
    });
}

int aimet_attn_softmax_lg(const float* scores, float* probs, int64_t B, int64_t H, int64_t L, int64_t S,
                          const uint8_t* attn_mask, int attn_mask_per_bh, const uint8_t* key_padding_mask,
                          const aimet_attn_lg_grid* score_grid, float* score_saved, const aimet_attn_lg_grid* prob_grid,
                          float* prob_saved, void* stream)
{
    return guarded([&] {
        LgArgs k {};
        k.a = checked_args(scores, B, H, L, S, attn_mask, attn_mask_per_bh, key_padding_mask, nullptr, nullptr);
        require_device_ptr(probs, "attention probabilities");
        AIMET_REQUIRE(aligned4(scores) && aligned4(probs), "attention softmax: misaligned pointer");
        AIMET_REQUIRE(probs != scores, "attention softmax on learned grids is out of place: the backward reads the "
                                       "raw scores");
        k.a.probs = probs;
        k.se      = lg_enc_of(score_grid, score_saved, true);
        k.pe      = lg_enc_of(prob_grid, prob_saved, true);
        launch_rows<LgArgs>(k, k.a, {attn_softmax_lg_wave<1>, attn_softmax_lg_wave<2>, attn_softmax_lg_wave<4>,
                                     attn_softmax_lg_wave<8>, attn_softmax_lg_wave<16>}, attn_softmax_lg_lds,
                            as_stream(stream));
        g_lg_launches.add(1);
    });
}

int aimet_attn_softmax_lg_backward(const float* scores, const float* grad_probs, float* grad_scores, int64_t B,
                                   int64_t H, int64_t L, int64_t S, const uint8_t* attn_mask, int attn_mask_per_bh,
                                   const uint8_t* key_padding_mask, const aimet_attn_lg_grid* score_grid,
                                   const float* score_saved, float* score_range_grad,
                                   const aimet_attn_lg_grid* prob_grid, const float* prob_saved, float* prob_range_grad,
                                   void* stream)
{
    return guarded([&] {
        LgArgs k {};
        k.a = checked_args(scores, B, H, L, S, attn_mask, attn_mask_per_bh, key_padding_mask, nullptr, nullptr);
        require_device_ptr(grad_probs, "gradient of the attention probabilities");
        require_device_ptr(grad_scores, "gradient of the attention scores");
        AIMET_REQUIRE(aligned4(scores) && aligned4(grad_probs) && aligned4(grad_scores),
                      "attention softmax: misaligned pointer");
        k.a.grad = grad_probs, k.a.probs = grad_scores;
        k.se = lg_enc_of(score_grid, score_saved, false);
        k.pe = lg_enc_of(prob_grid, prob_saved, false);
        const LgRange rs = lg_range_of(k.se, score_range_grad), rp = lg_range_of(k.pe, prob_range_grad);
        hipStream_t s    = as_stream(stream);
        const unsigned grid = row_grid(k.a);
        Scratch<float> partial;   // stays empty where neither quantizer is present
        if (rs.gmin || rp.gmin)
            partial = Scratch<float>((size_t) 6 * grid, s);
        k.partial = partial.get();
        launch_rows<LgArgs>(k, k.a, {attn_softmax_lg_bwd_wave<1>, attn_softmax_lg_bwd_wave<2>,
                                     attn_softmax_lg_bwd_wave<4>, attn_softmax_lg_bwd_wave<8>,
                                     attn_softmax_lg_bwd_wave<16>}, attn_softmax_lg_bwd_lds, s);
        g_lg_backward_launches.add(1);
        if (partial)
        {
            attn_lg_fold<<<1, kBlk, 0, s>>>(partial.get(), grid, rs, rp);
            AIMET_LAUNCH_CHECK();
        }
    });
}

int aimet_attn_lg_launch_count(int64_t* forward, int64_t* backward, int reset)
{
    return guarded([&] {
        g_lg_launches.read(forward, reset);
        g_lg_backward_launches.read(backward, reset);
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
