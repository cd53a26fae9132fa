// seqmse_block.hip -- Sequential MSE for blockwise weights: the reconstruction loss of every
// (candidate, output row, block of input features) of a Linear layer in ONE launch, on the fp32
// matrix cores of gfx950.
//
// Reference: aimet_torch/v2/seq_mse.py _compute_loss with block_size set: the weight and the input
// are split along the input features, one slice a block, and per candidate every slice runs two
// GEMMs with K = block_size whose [tokens][rows] outputs are only squared and summed. Here no
// candidate weight and no output tile leaves the chip:
//   err[c][r][b] = sum_t d^2 (or |d|),  d = sum_k xq[t][b BS + k] wq_c[r][b BS + k] - sum_k x[t][..] w[r][..]
//   sig[r][b]    = sum_t (sum_k x w)^2                                               (sqnr only)
//   wq_c         = dequantize(quantize_nearest(w)) of common.hpp with column r NB + b of candidate
//                  c's table [4][E] (aimet_seqmse_candidate_tables at C = E = R NB), rounded once
//                  to the I/O type for 16-bit I/O.
//
// Work split. A job is one block b and a tile of kRT = 16 rows; a workgroup of 8 waves takes jobs in
// a grid-stride loop (consecutive jobs share b, hence x's columns in L2) and walks all T tokens of a
// job itself: no cross-workgroup fold, no atomics, no workspace, equal inputs give equal bits.
//   prologue   the w tile is read once; the unquantized tile and the QDQ'd tile of every candidate
//              of the chunk go to LDS as fp32 in the order the B operand is read: float4 slot
//              (k / 4) * 16 + row, so that lane (row j = lane & 15, g = lane >> 4) reads the 16
//              bytes k = 16 q + 4 g .. + 3 at float offset 256 q + 4 lane: a wave reads 1 KiB of
//              consecutive addresses (no bank conflict). k is padded with zeros to 16 NQ.
//   main loop  a wave takes tiles of 16 tokens in turn. A lane (token i = lane & 15, g) loads the same
//              k quadruples of x and of xq (16-bit converted on load) into registers; they serve
//              the reference tile and every candidate. v_mfma_f32_16x16x4_f32, 4 NQ steps a tile,
//              the same k order for both products; D[token 4 g + v][row j] in 4 VGPRs, so a lane's 4
//              values belong to one row: it squares the 4 differences and adds them to its slot of
//              the candidate's running sum (LDS, one float a lane and candidate: the candidate loop
//              stays rolled, a register array indexed by it would live in scratch).
//   fold       per (candidate, row) the 8 waves x 4 lane groups are added in a fixed order.
// Candidates whose tiles do not fit the 160 KiB of LDS together are taken in equal chunks, each
// with its own pass over the tokens (x is re-read from L2; the reference tile is recomputed).
// Padded tokens, rows and k contribute exactly zero: their operands are zeros.
#include "common.hpp"
#include "io16.hpp"

namespace aimet_amd
{
namespace
{

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves    = 8;
constexpr int kThreads  = kWaves * 64;
constexpr int kRT       = 16;           // rows of w a job
constexpr int kTT       = 16;           // tokens a tile
constexpr int kMaxBS    = 256;
constexpr int kLdsBytes = 160 * 1024;   // gfx950: LDS of a CU, all of it open to one workgroup

struct BlockArgs
{
    const void* x;
    const void* xq;
    const void* w;
    const float* tables;   // candidate `first`'s table; candidate c is 4 E floats further
    float* err;            // [count][R][NB]
    float* sig;            // [R][NB] or null
    int64_t T, R, NB, ld;
    int64_t row_tiles, jobs;
    int BS, count, chunk;  // candidates a pass over the tokens
    int l1, vec_x, vec_q;  // 16-byte (fp32) / 8-byte (16-bit) loads of x / xq are aligned
};

// elements p[0 .. 3] as floats
template <int IO>
__device__ __forceinline__ f32x4 load4(const typename Io<IO>::elem_t* p, bool vec)
{
    f32x4 r;
    if (vec)
    {
        if constexpr (IO == IO_F32)
            r = *reinterpret_cast<const f32x4*>(p);
        else
        {
            const u16x4 u = *reinterpret_cast<const u16x4*>(p);
#pragma unroll
            for (int v = 0; v < 4; ++v)
                r[v] = Io<IO>::load(u[v]);
        }
    }
    else
    {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            r[v] = Io<IO>::load(p[v]);
    }
    return r;
}

// One tile's product: D += A B over the 16 NQ padded k of the block, B from the LDS tile `bt`
template <int NQ>
__device__ __forceinline__ f32x4 tile_product(const f32x4 (&a)[NQ], const float* bt, int lane)
{
    f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
        const f32x4 b = *reinterpret_cast<const f32x4*>(bt + q * 256 + lane * 4);
#pragma unroll
        for (int v = 0; v < 4; ++v)
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][v], b[v], d, 0, 0, 0);
    }
    return d;
}

template <int IO, int NQ>
__global__ __launch_bounds__(kThreads) void block_losses_kernel(BlockArgs a)
{
    using E = typename Io<IO>::elem_t;
    extern __shared__ float lds[];
    constexpr int kTile = NQ * 256;                            // floats of one [16 rows][16 NQ] tile
    float* const tiles  = lds;                                 // [chunk + 1]: the unquantized tile first
    float* const sums   = lds + (size_t) (a.chunk + 1) * kTile;   // [chunk + 1][kThreads]: sig last
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const E* const x  = static_cast<const E*>(a.x);
    const E* const xq = static_cast<const E*>(a.xq);
    const E* const w  = static_cast<const E*>(a.w);
    const int64_t En  = a.R * a.NB;
    const int64_t token_tiles = (a.T + kTT - 1) / kTT;

    for (int64_t job = blockIdx.x; job < a.jobs; job += gridDim.x)
    {
        const int64_t b  = job / a.row_tiles;
        const int64_t r0 = (job - b * a.row_tiles) * kRT;
        for (int c0 = 0; c0 < a.count; c0 += a.chunk)
        {
            const int cc       = a.count - c0 < a.chunk ? a.count - c0 : a.chunk;
            const bool do_sig  = a.sig != nullptr && c0 == 0;
            // ---- prologue: the w tile once, every candidate's QDQ of it, into the B layout ----
            for (int idx = tid; idx < 16 * 4 * NQ; idx += kThreads)
            {
                const int j = idx & 15, k = (idx >> 4) * 4;
                const int64_t r = r0 + j;
                const bool live = r < a.R && k < a.BS;
                f32x4 wv = {0.0f, 0.0f, 0.0f, 0.0f};
                if (live)
                    wv = load4<IO>(w + (r * a.NB + b) * a.BS + k, false);
                *reinterpret_cast<f32x4*>(tiles + idx * 4) = wv;
                const int64_t e = r * a.NB + b;
                for (int c = 0; c < cc; ++c)
                {
                    f32x4 qv = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (live)
                    {
                        const float* t = a.tables + (int64_t) (c0 + c) * 4 * En + e;
                        const QdqParams p {t[0], t[En], t[2 * En], t[3 * En]};
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            qv[v] = Io<IO>::round(dequantize(quantize_nearest(wv[v], p), p));
                    }
                    *reinterpret_cast<f32x4*>(tiles + (size_t) (c + 1) * kTile + idx * 4) = qv;
                }
            }
            for (int c = 0; c <= cc; ++c)
                sums[c * kThreads + tid] = 0.0f;
            __syncthreads();

            // ---- main loop: this wave's token tiles ----
            for (int64_t tt = wave; tt < token_tiles; tt += kWaves)
            {
                const int64_t t = tt * kTT + i;
                f32x4 ax[NQ], aq[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                {
                    const int k = 16 * q + 4 * g;
                    ax[q] = aq[q] = f32x4 {0.0f, 0.0f, 0.0f, 0.0f};
                    if (t < a.T && k < a.BS)
                    {
                        const int64_t off = t * a.ld + b * a.BS + k;
                        ax[q] = load4<IO>(x + off, a.vec_x != 0);
                        aq[q] = load4<IO>(xq + off, a.vec_q != 0);
                    }
                }
                const f32x4 ref = tile_product<NQ>(ax, tiles, lane);
                if (do_sig)
                {
                    float s = ref[0] * ref[0];
#pragma unroll
                    for (int v = 1; v < 4; ++v)
                        s = __builtin_fmaf(ref[v], ref[v], s);
                    sums[cc * kThreads + tid] += s;
                }
                for (int c = 0; c < cc; ++c)
                {
                    const f32x4 d = tile_product<NQ>(aq, tiles + (size_t) (c + 1) * kTile, lane) - ref;
                    float s;
                    if (a.l1)
                        s = (__builtin_fabsf(d[0]) + __builtin_fabsf(d[1])) + (__builtin_fabsf(d[2]) + __builtin_fabsf(d[3]));
                    else
                    {
                        s = d[0] * d[0];
#pragma unroll
                        for (int v = 1; v < 4; ++v)
                            s = __builtin_fmaf(d[v], d[v], s);
                    }
                    sums[c * kThreads + tid] += s;
                }
            }
            __syncthreads();

            // ---- fold: (candidate, row) over the waves and the four lane groups, in a fixed order ----
            for (int idx = tid; idx < (cc + 1) * kRT; idx += kThreads)
            {
                const int c = idx >> 4, j = idx & 15;
                const int64_t r = r0 + j;
                if (r >= a.R || (c == cc && !do_sig))
                    continue;
                float s = 0.0f;
                for (int l = j; l < kThreads; l += 16)
                    s += sums[c * kThreads + l];
                if (c < cc)
                    a.err[((int64_t) (c0 + c) * a.R + r) * a.NB + b] = s;
                else
                    a.sig[r * a.NB + b] = s;
            }
            __syncthreads();   // the tiles and sums are rewritten by the next chunk / job
        }
    }
}

template <int IO, int NQ>
void launch(const BlockArgs& a, unsigned grid, size_t lds_bytes, hipStream_t s)
{
    auto kernel = block_losses_kernel<IO, NQ>;
    if (lds_bytes > 48 * 1024)
        AIMET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes));
    kernel<<<grid, kThreads, lds_bytes, s>>>(a);
}

template <int IO>
void launch_nq(int nq, const BlockArgs& a, unsigned grid, size_t lds_bytes, hipStream_t s)
{
    switch (nq)
    {
    case 1: launch<IO, 1>(a, grid, lds_bytes, s); break;
    case 2: launch<IO, 2>(a, grid, lds_bytes, s); break;
    case 4: launch<IO, 4>(a, grid, lds_bytes, s); break;
    case 8: launch<IO, 8>(a, grid, lds_bytes, s); break;
    default: launch<IO, 16>(a, grid, lds_bytes, s); break;
    }
}

bool aligned_rows(const void* p, int64_t ld, size_t esize)
{
    return (reinterpret_cast<uintptr_t>(p) & (4 * esize - 1)) == 0 && ld % 4 == 0;
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_bq_seqmse_losses(const void* x, const void* xq, int64_t ld, const void* w, int64_t T, int64_t R,
                              int64_t NB, int64_t BS, const float* tables_dev, int64_t num_candidates, int64_t first,
                              int64_t count, int loss_kind, int io_dtype, float* err, float* sig, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(io_dtype == IO_F32 || io_dtype == IO_F16 || io_dtype == IO_BF16,
                      "io_dtype must be 0 (float32), 1 (float16) or 2 (bfloat16)");
        AIMET_REQUIRE(loss_kind == AIMET_SEQMSE_LOSS_MSE || loss_kind == AIMET_SEQMSE_LOSS_L1 ||
                          loss_kind == AIMET_SEQMSE_LOSS_SQNR,
                      "Unknown loss kind.");
        AIMET_REQUIRE(T >= 0 && R > 0 && NB > 0, "invalid blockwise loss shape");
        AIMET_REQUIRE(BS >= 4 && BS <= kMaxBS && BS % 4 == 0, "block size must be a multiple of 4 from 4 to 256");
        AIMET_REQUIRE(ld >= NB * BS, "row stride below the input features");
        AIMET_REQUIRE(first >= 0 && count >= 0 && first + count <= num_candidates, "candidate window out of range");
        AIMET_REQUIRE(count < (int64_t(1) << 24), "candidate window too large");
        if (count == 0)
            return;
        const size_t esize  = io_dtype == IO_F32 ? 4 : 2;
        const bool want_sig = loss_kind == AIMET_SEQMSE_LOSS_SQNR;
        require_device_ptr(w, "weight");
        require_device_ptr(tables_dev, "tables");
        require_device_ptr(err, "err");
        if (want_sig)
            require_device_ptr(sig, "sig");
        if (T > 0)
        {
            require_device_ptr(x, "x");
            require_device_ptr(xq, "xq");
        }
        for (const void* p : {x, xq, w})
            AIMET_REQUIRE((reinterpret_cast<uintptr_t>(p) & (esize - 1)) == 0, "misaligned pointer");

        const int64_t kq = ceil_div(BS, 16);
        const int nq     = kq <= 1 ? 1 : kq <= 2 ? 2 : kq <= 4 ? 4 : kq <= 8 ? 8 : 16;
        // LDS of one tile and of one running-sum slot; the unquantized tile and the signal slot come first
        const int64_t per       = (int64_t) sizeof(float) * (nq * 256 + kThreads);
        const int64_t fit       = kLdsBytes / per - 1;
        const int64_t chunks    = ceil_div(count, fit);
        const int64_t chunk     = ceil_div(count, chunks);
        const size_t lds_bytes  = (size_t) ((chunk + 1) * per);

        BlockArgs a;
        a.x = x, a.xq = xq, a.w = w;
        a.tables = tables_dev + first * 4 * R * NB;
        a.err = err, a.sig = want_sig ? sig : nullptr;
        a.T = T, a.R = R, a.NB = NB, a.ld = ld;
        a.row_tiles = ceil_div(R, kRT);
        a.jobs      = a.row_tiles * NB;
        a.BS = (int) BS, a.count = (int) count, a.chunk = (int) chunk;
        a.l1    = loss_kind == AIMET_SEQMSE_LOSS_L1;
        a.vec_x = aligned_rows(x, ld, esize), a.vec_q = aligned_rows(xq, ld, esize);
        const unsigned grid = (unsigned) std::min<int64_t>(a.jobs, kMaxStreamBlocks);
        hipStream_t s       = as_stream(stream);
        if (io_dtype == IO_F32)
            launch_nq<IO_F32>(nq, a, grid, lds_bytes, s);
        else if (io_dtype == IO_F16)
            launch_nq<IO_F16>(nq, a, grid, lds_bytes, s);
        else
            launch_nq<IO_BF16>(nq, a, grid, lds_bytes, s);
        AIMET_LAUNCH_CHECK();
    });
}

}   // extern "C"
