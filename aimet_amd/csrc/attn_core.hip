// attn_core.hip -- the core of a quantizable multi-head attention for static-grid evaluation in ONE
// launch that never writes the [B H, L, S] scores or probabilities to memory: q k^T, matmul_1's output
// quantizer, both masks, the softmax, softmax's output quantizer, the product with v and matmul_2's
// output quantizer (aimet_torch/transformers/activation.py), both products on the fp32 matrix cores.
//
// Per query row r = (bh, l), b = bh / H, j in [0, S), float32:
//   s_j = sum_k q[bh][l][k] k[bh][j][k]                v_mfma_f32_16x16x4_f32, k order below
//   x_j = QDQ(s_j; score_enc)                           quantize_nearest / dequantize of common.hpp
//   x_j = -inf  where attn_mask[((per_bh ? bh : 0) L + l) S + j] or key_padding_mask[b S + j] is set
//   m   = max_j x_j                                     (-inf for a row with every position masked)
//   e_j = x_j == -inf ? 0 : exp_r(x_j - m)              rnn_math.hpp; a masked position is exactly 0
//   s   = sum of e_j in the ORDER BELOW
//   p_j = QDQ(e_j / s; prob_enc)                        IEEE divide; 0 / 0 = NaN for a fully masked row,
//                                                       which the QDQ maps as aimet_qdq_per_tensor does
//   out[bh][l][d] = QDQ(sum_j p_j v[bh][j][d]; out_enc)
// A null encoding skips its QDQ, a null mask masks nothing. This is aimet_attn_softmax's element
// arithmetic (attn_softmax.hip) between two matrix products; only the order of the row sum differs.
//
// Work split. An item is one bh and a tile of kRT = 64 query rows; a workgroup of four waves takes
// items in a grid-stride loop, wave w owning rows 16 w .. 16 w + 15 of the tile: a row's maximum and
// sum never leave its wave. Keys and values stream through LDS in tiles of kST = 64 keys (four
// subtiles of 16), loaded once a workgroup and read by all four waves; 16-byte global loads.
//   q     registers, for the whole item: lane (i = lane & 15, g = lane >> 4) holds
//         q[row i][16 c + 4 g .. + 3], c < D / 16, the B operand of the score product.
//   k     LDS, in the order the A operand is read: subtile st, float4 slot (4 c + g) 16 + key, so lane
//         (key = lane & 15, g) reads 16 bytes at float offset st 16 D + 256 c + 4 lane: a wave reads
//         1 KiB of consecutive addresses (no bank conflict), and it is written with the same map.
//   s^T   = k q^T, not q k^T: D[key 4 g + u][row i] puts the scores of row i at keys 4 g .. 4 g + 3 into
//         lane (i, g) -- which is where the A operand of the second product wants the probabilities
//         (A[row i][k-slot g] at step u is key 4 g + u). No transpose through LDS, no lane permute.
//         The k order of a score: steps c = 0 .. D / 16 - 1, u = 0 .. 3, the step holding the four
//         products k = 16 c + 4 g' + u, g' = 0 .. 3 (summed by the matrix core), accumulated in fp32.
//   v     LDS, [key][D + 4] floats: lane (n = lane & 15, g) reads v[key 4 g + u][16 c + n] as one dword;
//         the four lane groups fall on rows 4 apart, 4 (D + 4) = 16 mod 64 dwords: four different
//         sixteen-bank groups (no bank conflict).
//   out   D / 16 accumulators of 4 VGPRs: lane (n, g) holds out[row 4 g + u][16 c + n]; a row's 16
//         consecutive floats are stored by 16 consecutive lanes.
//
// Two passes over the key tiles, because the probability quantizer needs the normalised probability:
//   pass 1  k tile -> LDS, the score tile, score QDQ and masks, running maximum and rescaled sum.
//   pass 2  k and v tiles -> LDS, the score tile again (the same instructions on the same operands: the
//           same bits), e_j / s, probability QDQ, out += p v.
//   epilogue  output QDQ, store.
// 3 * 2 * BH * L * S * D matrix FLOPs; no atomics, no global scratch.
//
// Summation order of s (part of the contract). It depends on S alone:
//   A row's keys belong to four lanes: lane g holds the keys j with (j mod 16) / 4 == g.
//   Within key tile t (keys 64 t .. 64 t + 63) lane g adds its 16 values e_j in increasing j, starting
//     from the first, each e_j taken against the running maximum m_t = max(m_(t-1), tile maximum):
//     ts. A key past S or masked adds +0.
//   Across tiles lane g carries l: l = (m_t == m_(t-1) ? l : l * exp_r(m_(t-1) - m_t)) + ts, tiles in
//     increasing t; l starts at 0, and while m_(t-1) is -inf the product is taken as 0.
//   Then s = (l_g + l_(g xor 2)) + the same of lane g xor 1: two butterfly steps, lanes 32 then 16 apart.
//   The maximum is exact in any order. Equal inputs give equal bits.
//
// D in {32, 64, 128}; L and S arbitrary (ragged last tiles: rows past L are computed on zeros and not
// stored, keys past S are zeros in LDS, -inf as scores and exactly 0 as probabilities).
// LDS: 64 D + 64 (D + 4) floats = 17408 / 33792 / 66560 bytes for D = 32 / 64 / 128.

#include "common.hpp"
#include "rnn_math.hpp"

namespace aimet_amd
{

QdqParams tensor_params(const aimet_tf_encoding& enc);   // qdq.hip

namespace
{

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves   = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kRT      = 16 * kWaves;   // query rows an item
constexpr int kST      = 64;            // keys a tile
constexpr unsigned kMaxGrid = 1u << 16;

LaunchCounter g_launches;

struct CoreArgs
{
    const float* q;
    const float* k;
    const float* v;
    float* out;
    const uint8_t* attn_mask;
    const uint8_t* kpm;
    int64_t H, L, S;
    int64_t q_sb, q_sl, k_sb, k_sl, v_sb, v_sl;   // strides in floats: bh, row
    int64_t row_tiles, items;
    int per_bh, score_qdq, prob_qdq, out_qdq;
    QdqParams sp, pp, op;
};

__device__ __forceinline__ float neg_inf()
{
    return -__builtin_huge_valf();
}

__device__ __forceinline__ float exp_of(float x, float m)
{
    return x == neg_inf() ? 0.0f : rnn_math::exp_r(x - m);
}

template <int D>
__global__ __launch_bounds__(kThreads) void attn_core_kernel(const CoreArgs a)
{
    extern __shared__ float4 lds4[];
    constexpr int NC   = D / 16;
    constexpr int kVLd = D + 4;
    float* const kt = reinterpret_cast<float*>(lds4);   // [4 subtiles][NC][64 lanes] float4
    float* const vt = kt + kST * D;                     // [kST][kVLd]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int64_t S = a.S;
    const float s_rcp = 1.0f / a.sp.delta, p_rcp = 1.0f / a.pp.delta, o_rcp = 1.0f / a.op.delta;

    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x)
    {
        const int64_t bh = item / a.row_tiles;
        const int64_t l0 = (item - bh * a.row_tiles) * kRT + wave * 16;   // this wave's first row
        const int64_t b  = bh / a.H;
        const int64_t row = l0 + i;            // the row whose scores this lane holds
        const bool wave_live = l0 < a.L;       // a wave without rows loads its share of the tiles and waits
        const bool row_live  = row < a.L;

        f32x4 qr[NC];
        {
            const float* qp = a.q + bh * a.q_sb + row * a.q_sl + 4 * g;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                qr[c] = row_live ? *reinterpret_cast<const f32x4*>(qp + 16 * c) : f32x4 {0.0f, 0.0f, 0.0f, 0.0f};
        }
        const uint8_t* const am =
            (a.attn_mask && row_live) ? a.attn_mask + ((a.per_bh ? bh : 0) * a.L + row) * S : nullptr;
        const uint8_t* const kp = a.kpm ? a.kpm + b * S : nullptr;
        const float* const kbase = a.k + bh * a.k_sb;
        const float* const vbase = a.v + bh * a.v_sb;

        // wave w brings subtile w of the k tile at j0: lane (key i, g) its float4s, into the read order
        auto load_k = [&](int64_t j0) {
            const int64_t key = j0 + 16 * wave + i;
            const float* p    = kbase + key * a.k_sl + 4 * g;
#pragma unroll
            for (int c = 0; c < NC; ++c)
            {
                const f32x4 kv = key < S ? *reinterpret_cast<const f32x4*>(p + 16 * c) : f32x4 {0.0f, 0.0f, 0.0f, 0.0f};
                *reinterpret_cast<f32x4*>(kt + wave * 16 * D + c * 256 + lane * 4) = kv;
            }
        };
        // the v tile row by row: consecutive threads take consecutive float4s of a row
        auto load_v = [&](int64_t j0) {
#pragma unroll
            for (int idx = tid; idx < kST * (D / 4); idx += kThreads)
            {
                const int key = idx / (D / 4), c4 = idx - key * (D / 4);
                const f32x4 vv = j0 + key < S ? *reinterpret_cast<const f32x4*>(vbase + (j0 + key) * a.v_sl + 4 * c4)
                                              : f32x4 {0.0f, 0.0f, 0.0f, 0.0f};
                *reinterpret_cast<f32x4*>(vt + key * kVLd + 4 * c4) = vv;
            }
        };
        // the score tile at j0, quantized and masked: x[st][u] is row i at key j0 + 16 st + 4 g + u
        auto score_tile = [&](int64_t j0, float (&x)[4][4]) {
#pragma unroll
            for (int st = 0; st < 4; ++st)
            {
                const int64_t js = j0 + 16 * st;
                f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
                if (js < S)   // the same for every lane
                {
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                    {
                        const f32x4 kv = *reinterpret_cast<const f32x4*>(kt + st * 16 * D + c * 256 + lane * 4);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            d = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[u], qr[c][u], d, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                {
                    const int64_t j = js + 4 * g + u;
                    float s = d[u];
                    if (a.score_qdq)
                        s = dequantize(quantize_nearest_rcp(s, a.sp, s_rcp), a.sp);
                    if (j >= S || (am && am[j]) || (kp && kp[j]))
                        s = neg_inf();
                    x[st][u] = s;
                }
            }
        };

        const int64_t n_tiles = (S + kST - 1) / kST;

        // ---- pass 1: the row maximum and the row sum ----
        float m = neg_inf(), l = 0.0f;
        for (int64_t t = 0; t < n_tiles; ++t)
        {
            __syncthreads();   // the previous tile is read out
            load_k(t * kST);
            __syncthreads();
            if (!wave_live)
                continue;
            float x[4][4];
            score_tile(t * kST, x);
            float tm = neg_inf();
#pragma unroll
            for (int st = 0; st < 4; ++st)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    tm = x[st][u] > tm ? x[st][u] : tm;
            {
                float o = __shfl_xor(tm, 32, 64);
                tm      = o > tm ? o : tm;
                o       = __shfl_xor(tm, 16, 64);
                tm      = o > tm ? o : tm;
            }
            const float mn = tm > m ? tm : m;
            float ts = 0.0f;
#pragma unroll
            for (int st = 0; st < 4; ++st)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                {
                    const float e = exp_of(x[st][u], mn);
                    ts            = (st == 0 && u == 0) ? e : ts + e;
                }
            if (mn != m)
                l = m == neg_inf() ? 0.0f : l * rnn_math::exp_r(m - mn);
            l = l + ts;
            m = mn;
        }
        l = l + __shfl_xor(l, 32, 64);
        l = l + __shfl_xor(l, 16, 64);

        // ---- pass 2: the probabilities and their product with v ----
        f32x4 acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            acc[c] = f32x4 {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t t = 0; t < n_tiles; ++t)
        {
            const int64_t j0 = t * kST;
            __syncthreads();
            load_k(j0);
            load_v(j0);
            __syncthreads();
            if (!wave_live)
                continue;
            float x[4][4];
            score_tile(j0, x);
#pragma unroll
            for (int st = 0; st < 4; ++st)
            {
                const int64_t js = j0 + 16 * st;
                if (js >= S)
                    continue;
                float p[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                {
                    float pv = exp_of(x[st][u], m) / l;
                    if (a.prob_qdq)
                        pv = dequantize(quantize_nearest_rcp(pv, a.pp, p_rcp), a.pp);
                    p[u] = js + 4 * g + u < S ? pv : 0.0f;   // a key past S: 0 times the zeros in LDS
                }
                const float* vrow = vt + (16 * st + 4 * g) * kVLd + i;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[u], vrow[u * kVLd + 16 * c], acc[c], 0, 0, 0);
            }
        }

        // ---- epilogue: lane (n = i, g) holds out[row l0 + 4 g + u][16 c + n] ----
        if (wave_live)
        {
#pragma unroll
            for (int u = 0; u < 4; ++u)
            {
                const int64_t r = l0 + 4 * g + u;
                if (r >= a.L)
                    continue;
                float* o = a.out + (bh * a.L + r) * D + i;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                {
                    float y = acc[c][u];
                    if (a.out_qdq)
                        y = dequantize(quantize_nearest_rcp(y, a.op, o_rcp), a.op);
                    o[16 * c] = y;
                }
            }
        }
    }
}

template <int D>
void launch(const CoreArgs& a, unsigned grid, hipStream_t s)
{
    constexpr size_t lds_bytes = (size_t) (kST * D + kST * (D + 4)) * sizeof(float);
    auto kernel = attn_core_kernel<D>;
    if (lds_bytes > 48 * 1024)
        AIMET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes));
    kernel<<<grid, kThreads, lds_bytes, s>>>(a);
    AIMET_LAUNCH_CHECK();
}

// a [BH, rows, D] operand read in 16-byte pieces: D contiguous, rows and matrices at multiples of 4 floats
void require_operand(const float* p, int64_t sb, int64_t sl, int64_t D, const char* what)
{
    require_device_ptr(p, what);
    AIMET_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0 && sb % 4 == 0 && sl % 4 == 0 && sl >= D && sb >= 0,
                  std::string("attention core: ") + what + " must be 16-byte aligned with strides that are multiples "
                  "of 4 floats and rows at least D apart");
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_attn_core(const float* q, const float* k, const float* v, float* out, int64_t B, int64_t H, int64_t L,
                    int64_t S, int64_t D, int64_t q_bh_stride, int64_t q_row_stride, int64_t k_bh_stride,
                    int64_t k_row_stride, int64_t v_bh_stride, int64_t v_row_stride, const uint8_t* attn_mask,
                    int attn_mask_per_bh, const uint8_t* key_padding_mask, const aimet_tf_encoding* score_enc,
                    const aimet_tf_encoding* prob_enc, const aimet_tf_encoding* out_enc, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(B > 0 && H > 0 && L > 0 && S > 0, "attention core: B, H, L and S must be positive");
        AIMET_REQUIRE(D == 32 || D == 64 || D == 128, "attention core: head_dim must be 32, 64 or 128");
        AIMET_REQUIRE(B < (int64_t(1) << 31) && H < (int64_t(1) << 31) && L < (int64_t(1) << 31) &&
                          S < (int64_t(1) << 31) && B * H < (int64_t(1) << 40) / L,
                      "attention core: too many rows (B H L must stay below 2^40)");
        require_operand(q, q_bh_stride, q_row_stride, D, "q");
        require_operand(k, k_bh_stride, k_row_stride, D, "k");
        require_operand(v, v_bh_stride, v_row_stride, D, "v");
        require_device_ptr(out, "attention output");
        AIMET_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "attention core: misaligned output");
        if (attn_mask)
            require_device_ptr(attn_mask, "attention mask");
        if (key_padding_mask)
            require_device_ptr(key_padding_mask, "key padding mask");
        CoreArgs a {};
        a.q = q, a.k = k, a.v = v, a.out = out, a.attn_mask = attn_mask, a.kpm = key_padding_mask;
        a.H = H, a.L = L, a.S = S;
        a.q_sb = q_bh_stride, a.q_sl = q_row_stride, a.k_sb = k_bh_stride, a.k_sl = k_row_stride;
        a.v_sb = v_bh_stride, a.v_sl = v_row_stride;
        a.row_tiles = ceil_div(L, kRT), a.items = B * H * a.row_tiles;
        a.per_bh    = attn_mask_per_bh != 0;
        a.score_qdq = score_enc != nullptr, a.prob_qdq = prob_enc != nullptr, a.out_qdq = out_enc != nullptr;
        a.sp = a.pp = a.op = QdqParams {0.0f, 0.0f, 1.0f, 0.0f};
        if (score_enc)
            a.sp = tensor_params(*score_enc);
        if (prob_enc)
            a.pp = tensor_params(*prob_enc);
        if (out_enc)
            a.op = tensor_params(*out_enc);
        const unsigned grid = (unsigned) std::min<int64_t>(a.items, kMaxGrid);
        hipStream_t s = as_stream(stream);
        switch (D)
        {
        case 32: launch<32>(a, grid, s); break;
        case 64: launch<64>(a, grid, s); break;
        default: launch<128>(a, grid, s); break;
        }
        g_launches.add(1);
    });
}

int aimet_attn_core_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
