// gptvq.hip -- the two hot loops of GPTVQ (aimet_torch/gptvq/) for gfx950.
//
// Reference: generate_codebook (gptvq/utils.py:56-78, 177-241) runs, per column block, 100 Lloyd
// iterations that each materialise a [G][N][K][D] distance tensor and a [G][N][K] one-hot;
// GPTVQOptimizer.weight_update (gptvq_optimizer.py:112-169) runs ~15 launches per `vector_dim`
// columns, 2048 dependent steps for a 4096-column weight. MI355X design:
//   * kmeans: one 1024-lane workgroup per row group, every iteration inside one launch. The group's
//     vectors are staged in LDS once (a group that does not fit is walked in LDS-sized chunks that
//     are re-read from global memory / L2 every iteration). E-step: a lane holds four vectors in
//     registers while the K centroids go by as LDS broadcast reads. M-step: a masked reduction
//     without atomics. Lane t owns (centroid k = t % K, slice s = t / K) and adds, n ascending, the
//     vectors of slice s that are assigned to k (the assignment and the vector are broadcast
//     reads, eight of each in flight; a vector of another centroid adds +0.0f); then the S = max(1, 1024 / K) slice sums of a centroid are added s ascending. Both
//     orders are fixed by the sizes alone, so equal inputs give equal bits. The masked reduction
//     costs N * K / 1024 steps per lane, as the E-step does.
//   * block_update: one wave per weight row, four rows per workgroup, no LDS and no barrier. The
//     row's block of at most 128 columns lives in two registers per lane (column j in lane j % 64),
//     lane k holds centroid k (K <= 64; beyond that the lanes walk the codebook in L1). A step
//     broadcasts its D columns with v_readlane, takes the wave's first minimum with a six-stage
//     butterfly on (distance, index), and every lane updates its two columns with the rows of hinv
//     it prefetched during the previous step's reduction. err and indices stay in registers and
//     are written, like the block, once and coalesced. (The alternative, a lane per row with the
//     row in LDS, keeps 64 rows in one wave: 4096 rows are 64 waves for 1024 SIMDs. It is kept as
//     layout 2 for the measurement in benchmarks/gptvq_llama.py.)
// All arithmetic is fp32 with separately rounded products and sums (-ffp-contract=off) and IEEE
// divides; tests/gptvq_oracle.py follows the same order in numpy.
#include "common.hpp"

#include <atomic>

namespace aimet_amd
{

namespace
{

constexpr int kKmLanes    = 1024;   // k-means workgroup: 16 waves, four per SIMD
constexpr int kKmBatch    = 4;      // vectors a lane holds in the E-step
constexpr int kKmUnroll   = 8;      // vectors a lane loads at once in the M-step
constexpr int kMaxD       = 8;
constexpr int kMaxK       = 1024;
constexpr int kMaxBlock   = 128;    // BLOCK_STRIDE of the reference
constexpr int kRowsPerWg  = 4;      // block_update: waves (rows) per workgroup
constexpr int64_t kTwo31  = int64_t(1) << 31;

std::atomic<int> g_update_layout {0};

typedef float f2 __attribute__((ext_vector_type(2)));

template <int D>
__device__ __forceinline__ void load_vec(const float* p, float* v, int d_rt)
{
    if constexpr (D == 2)
    {
        const f2 t = *reinterpret_cast<const f2*>(p);
        v[0]       = t.x;
        v[1]       = t.y;
    }
    else if constexpr (D == 4)
    {
        const f4 t = *reinterpret_cast<const f4*>(p);
        v[0]       = t.x;
        v[1]       = t.y;
        v[2]       = t.z;
        v[3]       = t.w;
    }
    else if constexpr (D == 1)
        v[0] = p[0];
    else
    {
#pragma unroll
        for (int d = 0; d < kMaxD; ++d)
            v[d] = d < d_rt ? p[d] : 0.0f;
    }
}

// v[d] = p[d] for d < d_rt (scalar loads: no alignment is assumed), zero beyond
template <int DD>
__device__ __forceinline__ void load_n(const float* p, float* v, int d_rt)
{
#pragma unroll
    for (int d = 0; d < DD; ++d)
        v[d] = d < d_rt ? p[d] : 0.0f;
}

// sum over d ascending of (x_d - c_d) * (x_d - c_d), every operation rounded on its own
template <int D>
__device__ __forceinline__ float sq_dist(const float* x, const float* c, int d_rt)
{
    constexpr int DD = D ? D : kMaxD;
    float t          = x[0] - c[0];
    float acc        = t * t;
#pragma unroll
    for (int d = 1; d < DD; ++d)
        if (D || d < d_rt)
        {
            t   = x[d] - c[d];
            acc = acc + t * t;
        }
    return acc;
}

// ---------------------------------------------------------------------------------------------
// k-means
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline int64_t align16(int64_t b)
{
    return (b + 15) & ~int64_t(15);
}

// dynamic LDS: data [chunk * D] | codebook [K * D] | partials [S * K * (D + 1)] | assignments u16 [chunk]
struct KmLayout
{
    int64_t cb, part, assign, total;
};
__host__ __device__ inline KmLayout km_layout(int64_t chunk, int D, int K, int S)
{
    KmLayout l;
    l.cb     = align16(chunk * D * 4);
    l.part   = l.cb + align16((int64_t) K * D * 4);
    l.assign = l.part + align16((int64_t) S * K * (D + 1) * 4);
    l.total  = l.assign + align16(chunk * 2);
    return l;
}

template <int DT>
__global__ __launch_bounds__(kKmLanes) void kmeans_kernel(const float* __restrict__ w, int64_t ld, int rows_per_block,
                                                          FastDiv divCols, int d_rt, int K, int iterations, int N,
                                                          int chunk, float* __restrict__ codebook)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
    constexpr int DD  = DT ? DT : kMaxD;
    const int D       = DT ? DT : d_rt;
    const int S       = K < kKmLanes ? kKmLanes / K : 1;
    const KmLayout lo = km_layout(chunk, D, K, S);
    float* data       = reinterpret_cast<float*>(km_lds);
    float* cb         = reinterpret_cast<float*>(km_lds + lo.cb);
    float* part       = reinterpret_cast<float*>(km_lds + lo.part);
    uint16_t* assign  = reinterpret_cast<uint16_t*>(km_lds + lo.assign);
    const int t       = threadIdx.x;
    const int ncols   = (int) divCols.d;
    const float* wg   = w + (int64_t) blockIdx.x * rows_per_block * ld;
    float* cbg        = codebook + (int64_t) blockIdx.x * K * D;
    const bool staged_once = chunk >= N;
    // M-step ownership: centroid mk of slice ms
    const int mk = t % K, ms = t / K;
    const bool m_live = ms < S;

    for (int i = t; i < K * D; i += kKmLanes)
        cb[i] = cbg[i];

    for (int it = 0; it < iterations; ++it)
    {
        float acc[DD];
#pragma unroll
        for (int d = 0; d < DD; ++d)
            acc[d] = 0.0f;
        int cnt = 0;
        for (int n0 = 0; n0 < N; n0 += chunk)
        {
            const int cn = N - n0 < chunk ? N - n0 : chunk;
            if (!staged_once || it == 0)
            {
                // element e of the group is row e / ncols, column e % ncols of the block
                const uint32_t e0 = (uint32_t) n0 * D, e1 = e0 + (uint32_t) cn * D;
                for (uint32_t e = e0 + t; e < e1; e += kKmLanes)
                {
                    const uint32_t r = divCols.div(e);
                    data[e - e0]     = wg[(int64_t) r * ld + (e - r * ncols)];
                }
            }
            __syncthreads();   // the chunk and the codebook are in LDS
            // E-step: first minimum over k of the squared distance
            for (int base = 0; base < cn; base += kKmLanes * kKmBatch)
            {
                float x[kKmBatch][DD], best[kKmBatch];
                int idx[kKmBatch];
#pragma unroll
                for (int j = 0; j < kKmBatch; ++j)
                {
                    const int n = base + t + j * kKmLanes;
                    load_vec<DT>(data + (int64_t) (n < cn ? n : 0) * D, x[j], D);
                    best[j] = __builtin_inff();
                    idx[j]  = 0;
                }
                float c[DD];
                load_vec<DT>(cb, c, D);
                for (int k = 0; k < K; ++k)
                {
                    // the next centroid is on its way while this one is used
                    float cnext[DD];
                    load_vec<DT>(cb + (k + 1 < K ? k + 1 : k) * D, cnext, D);
#pragma unroll
                    for (int j = 0; j < kKmBatch; ++j)
                    {
                        const float dist = sq_dist<DT>(x[j], c, D);
                        if (dist < best[j])
                        {
                            best[j] = dist;
                            idx[j]  = k;
                        }
                    }
#pragma unroll
                    for (int d = 0; d < DD; ++d)
                        c[d] = cnext[d];
                }
#pragma unroll
                for (int j = 0; j < kKmBatch; ++j)
                {
                    const int n = base + t + j * kKmLanes;
                    if (n < cn)
                        assign[n] = (uint16_t) idx[j];
                }
            }
            __syncthreads();   // the assignments are in LDS
            // M-step: this lane's slice of the chunk, n ascending
            if (m_live)
            {
                // kKmUnroll vectors and assignments are loaded at once, then added in order. A vector
                // of another centroid adds +0.0f, which leaves the sum's bits as they are (a sum that
                // starts at +0.0f is never -0.0f).
                const int len = (cn + S - 1) / S;
                const int a   = ms * len;
                for (int j0 = 0; j0 < len; j0 += kKmUnroll)
                {
                    float x[kKmUnroll][DD];
                    int who[kKmUnroll];
#pragma unroll
                    for (int u = 0; u < kKmUnroll; ++u)
                    {
                        const int n   = a + j0 + u;
                        const bool ok = j0 + u < len && n < cn;
                        const int nn  = ok ? n : 0;   // both loads unconditional: no branch between them
                        load_vec<DT>(data + (int64_t) nn * D, x[u], D);
                        const int av = (int) assign[nn];
                        who[u]       = ok ? av : -1;
                    }
#pragma unroll
                    for (int u = 0; u < kKmUnroll; ++u)
                    {
                        const bool mine = who[u] == mk;
#pragma unroll
                        for (int d = 0; d < DD; ++d)
                            acc[d] = acc[d] + (mine ? x[u][d] : 0.0f);
                        cnt += mine ? 1 : 0;
                    }
                }
            }
            if (!staged_once)
                __syncthreads();   // the next chunk overwrites data and assignments
        }
        if (m_live)
        {
            float* p = part + ((int64_t) ms * K + mk) * (D + 1);
#pragma unroll
            for (int d = 0; d < DD; ++d)
                if (d < D)
                    p[d] = acc[d];
            p[D] = __int_as_float(cnt);
        }
        __syncthreads();
        // the S slice sums of (k, d), s ascending; an empty cluster becomes the zero vector
        for (int i = t; i < K * D; i += kKmLanes)
        {
            const int k = i / D, d = i - k * D;
            float sum = 0.0f;
            int count = 0;
            for (int s = 0; s < S; ++s)
            {
                const float* p = part + ((int64_t) s * K + k) * (D + 1);
                sum            = sum + p[d];
                count += __float_as_int(p[D]);
            }
            cb[i] = sum * (1.0f / (float) (count > 1 ? count : 1));
        }
        __syncthreads();
    }
    for (int i = t; i < K * D; i += kKmLanes)
        cbg[i] = cb[i];
}

// ---------------------------------------------------------------------------------------------
// block update
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float lane_bcast(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

struct UpdateArgs
{
    float* w;
    int64_t ld;
    int64_t rows;
    int rows_per_block, b0, s0, s1, len, D, K;
    const float* codebook;
    const float* hinv;
    int64_t hinv_ld;
    float* err;
    int32_t* indices;
};

// Layout 1: a wave per row. REGK: lane k keeps centroid k in registers (K <= 64).
template <int DT, bool REGK>
__global__ __launch_bounds__(kRowsPerWg * 64) void update_wave_kernel(UpdateArgs a)
{
    constexpr int DD  = DT ? DT : kMaxD;
    const int D       = DT ? DT : a.D;
    const int lane    = threadIdx.x & 63;
    const int64_t r   = (int64_t) blockIdx.x * kRowsPerWg + (threadIdx.x >> 6);
    if (r >= a.rows)
        return;
    const int L        = a.len, K = a.K;
    float* wr          = a.w + r * a.ld + a.b0;
    const float* cb    = a.codebook + (r / a.rows_per_block) * (int64_t) K * D;
    const float* hblk  = a.hinv + (int64_t) a.b0 * a.hinv_ld + a.b0;   // hinv[b0 + i][b0 + j] = hblk[i * hinv_ld + j]
    // column j of the block: register j / 64 of lane j % 64
    float x0 = lane < L ? wr[lane] : 0.0f;
    float x1 = lane + 64 < L ? wr[lane + 64] : 0.0f;
    float e0 = 0.0f, e1 = 0.0f;
    int i0 = 0, i1 = 0;
    float creg[DD];
#pragma unroll
    for (int d = 0; d < DD; ++d)
        creg[d] = 0.0f;
    if (REGK && lane < K)
        load_n<DD>(cb + lane * D, creg, D);

    // rows i .. i + D - 1 of hinv at this lane's two columns, and their diagonal
    float h0[DD], h1[DD], hd[DD];
    auto fetch = [&](int i) {
#pragma unroll
        for (int d = 0; d < DD; ++d)
            if (d < D)
            {
                const float* hr = hblk + (int64_t) (i + d) * a.hinv_ld;
                h0[d]           = lane < L ? hr[lane] : 0.0f;
                h1[d]           = lane + 64 < L ? hr[lane + 64] : 0.0f;
                hd[d]           = hr[i + d];
            }
    };
    if (a.s0 < a.s1)
        fetch(a.s0);
    for (int i = a.s0; i < a.s1; i += D)
    {
        float x[DD];
#pragma unroll
        for (int d = 0; d < DD; ++d)
            if (d < D)
            {
                const int j = i + d;
                x[d]        = lane_bcast(j < 64 ? x0 : x1, j & 63);
            }
            else
                x[d] = 0.0f;
        // this lane's candidates k = lane, lane + 64, ...: the first minimum among them
        float best = __builtin_inff();
        int idx    = kMaxK;
        if (REGK)
        {
            if (lane < K)
            {
                best = sq_dist<DT>(x, creg, D);
                idx  = lane;
            }
        }
        else
            for (int k = lane; k < K; k += 64)
            {
                float c[DD];
                load_n<DD>(cb + (int64_t) k * D, c, D);
                const float dist = sq_dist<DT>(x, c, D);
                if (dist < best || idx == kMaxK)
                {
                    best = dist;
                    idx  = k;
                }
            }
        // the wave's first minimum: butterfly on (distance, index)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1)
        {
            const float od = __shfl_xor(best, m, 64);
            const int oi   = __shfl_xor(idx, m, 64);
            if (od < best || (od == best && oi < idx))
            {
                best = od;
                idx  = oi;
            }
        }
        const int ks = __builtin_amdgcn_readfirstlane(idx);
        float q[DD], e[DD], hcur0[DD], hcur1[DD];
#pragma unroll
        for (int d = 0; d < DD; ++d)
            if (d < D)
            {
                q[d]     = REGK ? lane_bcast(creg[d], ks) : cb[(int64_t) ks * D + d];
                e[d]     = (x[d] - q[d]) / hd[d];
                hcur0[d] = h0[d];
                hcur1[d] = h1[d];
            }
        if (i + D < a.s1)
            fetch(i + D);   // in flight during the rest of this step and the next reduction
        // columns i .. i + D - 1 take q, their err and the step's index
#pragma unroll
        for (int d = 0; d < DD; ++d)
            if (d < D)
            {
                const int j = i + d;
                if (lane == (j & 63))
                {
                    if (j < 64)
                    {
                        x0 = q[d];
                        e0 = e[d];
                    }
                    else
                    {
                        x1 = q[d];
                        e1 = e[d];
                    }
                }
            }
        {
            const int st = i / D;
            if (lane == (st & 63))
            {
                if (st < 64)
                    i0 = ks;
                else
                    i1 = ks;
            }
        }
        // columns from i + D on: w -= (e_0 * h_0 + e_1 * h_1 + ...), d ascending
        float u0 = e[0] * hcur0[0], u1 = e[0] * hcur1[0];
#pragma unroll
        for (int d = 1; d < DD; ++d)
            if (d < D)
            {
                u0 = u0 + e[d] * hcur0[d];
                u1 = u1 + e[d] * hcur1[d];
            }
        if (lane >= i + D && lane < L)
            x0 = x0 - u0;
        if (lane + 64 >= i + D && lane + 64 < L)
            x1 = x1 - u1;
    }
    // the block from s0 on, err and indices of the steps of this call, each written once
    float* er   = a.err + r * L;
    int32_t* ir = a.indices + r * (L / D);
    if (lane >= a.s0 && lane < L)
        wr[lane] = x0;
    if (lane + 64 >= a.s0 && lane + 64 < L)
        wr[lane + 64] = x1;
    if (lane >= a.s0 && lane < a.s1)
        er[lane] = e0;
    if (lane + 64 >= a.s0 && lane + 64 < a.s1)
        er[lane + 64] = e1;
    const int t0 = a.s0 / D, t1 = a.s1 / D;
    if (lane >= t0 && lane < t1)
        ir[lane] = i0;
    if (lane + 64 >= t0 && lane + 64 < t1)
        ir[lane + 64] = i1;
}

// Layout 2: a lane per row, the row's block in LDS (column-major: conflict-free), everything else
// as above. For the layout measurement only.
template <int DT>
__global__ __launch_bounds__(64) void update_lane_kernel(UpdateArgs a)
{
    __shared__ float xs[kMaxBlock][64];
    constexpr int DD = DT ? DT : kMaxD;
    const int D      = DT ? DT : a.D;
    const int lane   = threadIdx.x;
    const int64_t r  = (int64_t) blockIdx.x * 64 + lane;
    if (r >= a.rows)
        return;
    const int L       = a.len, K = a.K;
    float* wr         = a.w + r * a.ld + a.b0;
    const float* cb   = a.codebook + (r / a.rows_per_block) * (int64_t) K * D;
    const float* hblk = a.hinv + (int64_t) a.b0 * a.hinv_ld + a.b0;
    float* er         = a.err + r * L;
    int32_t* ir       = a.indices + r * (L / D);
    for (int j = 0; j < L; ++j)
        xs[j][lane] = wr[j];
    for (int i = a.s0; i < a.s1; i += D)
    {
        float x[DD], q[DD], e[DD];
#pragma unroll
        for (int d = 0; d < DD; ++d)
            x[d] = d < D ? xs[i + d][lane] : 0.0f;
        float best = __builtin_inff();
        int idx    = 0;
        for (int k = 0; k < K; ++k)
        {
            float c[DD];
            load_n<DD>(cb + (int64_t) k * D, c, D);
            const float dist = sq_dist<DT>(x, c, D);
            if (dist < best)
            {
                best = dist;
                idx  = k;
            }
        }
#pragma unroll
        for (int d = 0; d < DD; ++d)
            if (d < D)
            {
                q[d]            = cb[(int64_t) idx * D + d];
                e[d]            = (x[d] - q[d]) / hblk[(int64_t) (i + d) * a.hinv_ld + i + d];
                xs[i + d][lane] = q[d];
                er[i + d]       = e[d];
            }
        ir[i / D] = idx;
        for (int j = i + D; j < L; ++j)
        {
            float u = e[0] * hblk[(int64_t) i * a.hinv_ld + j];
#pragma unroll
            for (int d = 1; d < DD; ++d)
                if (d < D)
                    u = u + e[d] * hblk[(int64_t) (i + d) * a.hinv_ld + j];
            xs[j][lane] = xs[j][lane] - u;
        }
    }
    for (int j = a.s0; j < L; ++j)
        wr[j] = xs[j][lane];
}

template <int DT>
void launch_update(const UpdateArgs& a, int layout, hipStream_t s)
{
    if (layout == 2)
        update_lane_kernel<DT><<<tile_grid(a.rows, 64), 64, 0, s>>>(a);
    else if (a.K <= 64)
        update_wave_kernel<DT, true><<<tile_grid(a.rows, kRowsPerWg), kRowsPerWg * 64, 0, s>>>(a);
    else
        update_wave_kernel<DT, false><<<tile_grid(a.rows, kRowsPerWg), kRowsPerWg * 64, 0, s>>>(a);
}

int lds_limit()
{
    int dev = 0, bytes = 0;
    AIMET_HIP_CHECK(hipGetDevice(&dev));
    AIMET_HIP_CHECK(hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    return bytes;
}

template <int DT>
void launch_kmeans(const float* w, int64_t ld, int64_t G, int rows_per_block, int ncols, int D, int K, int iterations,
                   float* codebook, hipStream_t s)
{
    const int S         = K < kKmLanes ? kKmLanes / K : 1;
    const int64_t N     = (int64_t) rows_per_block * ncols / D;
    const int64_t limit = lds_limit();
    // the largest chunk of vectors (a multiple of four: every region stays 16-B aligned) that fits
    int64_t chunk = N;
    if (km_layout(chunk, D, K, S).total > limit)
    {
        const int64_t fixed = km_layout(0, D, K, S).total;
        chunk               = (limit - fixed - 32) / (D * 4 + 2) / 4 * 4;
        AIMET_REQUIRE(chunk >= 4, "codebook too large for the k-means kernel's LDS");
    }
    const int64_t bytes = km_layout(chunk, D, K, S).total;
    auto kernel         = kmeans_kernel<DT>;
    if (bytes > 48 * 1024)
        AIMET_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes));
    kernel<<<tile_grid(G, 1), kKmLanes, (size_t) bytes, s>>>(w, ld, rows_per_block, FastDiv((uint32_t) ncols), D, K,
                                                             iterations, (int) N, (int) chunk, codebook);
}

}   // namespace

}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_gptvq_kmeans(const float* w, int64_t ld, int64_t G, int64_t rows_per_block, int64_t ncols, int32_t D,
                       int32_t K, int32_t iterations, float* codebook, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(G > 0 && rows_per_block > 0 && ncols > 0, "k-means needs at least one group, row and column");
        AIMET_REQUIRE(D >= 1 && D <= kMaxD, "vector_dim must be in 1..8");
        AIMET_REQUIRE(ncols % D == 0, "the column count must be a multiple of vector_dim");
        AIMET_REQUIRE(K >= 1 && K <= kMaxK, "the number of centroids must be in 1..1024");
        AIMET_REQUIRE(iterations >= 0, "iterations must not be negative");
        AIMET_REQUIRE(ld >= ncols, "ld is smaller than the column count");
        AIMET_REQUIRE(G < kTwo31 && rows_per_block < kTwo31 && ld < kTwo31, "k-means shape too large");
        AIMET_REQUIRE(G * rows_per_block * ld < kTwo31, "k-means needs fewer than 2^31 weight elements");
        AIMET_REQUIRE(rows_per_block * ncols < kTwo31, "k-means needs fewer than 2^31 elements per group");
        AIMET_REQUIRE(G * K * D < kTwo31, "k-means needs fewer than 2^31 codebook elements");
        require_device_ptr(w, "weight");
        require_device_ptr(codebook, "codebook");
        if (iterations == 0)
            return;
        hipStream_t s = as_stream(stream);
        switch (D)
        {
        case 1: launch_kmeans<1>(w, ld, G, (int) rows_per_block, (int) ncols, D, K, iterations, codebook, s); break;
        case 2: launch_kmeans<2>(w, ld, G, (int) rows_per_block, (int) ncols, D, K, iterations, codebook, s); break;
        case 4: launch_kmeans<4>(w, ld, G, (int) rows_per_block, (int) ncols, D, K, iterations, codebook, s); break;
        default: launch_kmeans<0>(w, ld, G, (int) rows_per_block, (int) ncols, D, K, iterations, codebook, s); break;
        }
        AIMET_LAUNCH_CHECK();
    });
}

int aimet_gptvq_update_layout(int layout, int* previous)
{
    return guarded([&] {
        AIMET_REQUIRE(layout >= 0 && layout <= 2, "layout must be 0 (default), 1 (a wave per row) or 2 (a lane per row)");
        const int old = g_update_layout.exchange(layout);
        if (previous)
            *previous = old;
    });
}

int aimet_gptvq_block_update(float* w, int64_t ld, int64_t rows, int64_t rows_per_block, int64_t b0, int64_t s0,
                             int64_t s1, int64_t block_end, int32_t D, int32_t K, const float* codebook,
                             const float* hinv, int64_t hinv_ld, float* err, int32_t* indices, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(rows > 0 && rows_per_block > 0 && rows % rows_per_block == 0,
                      "rows must be a positive multiple of rows_per_block");
        AIMET_REQUIRE(D >= 1 && D <= kMaxD, "vector_dim must be in 1..8");
        AIMET_REQUIRE(K >= 1 && K <= kMaxK, "the number of centroids must be in 1..1024");
        AIMET_REQUIRE(b0 >= 0 && block_end > b0 && block_end - b0 <= kMaxBlock, "a block holds 1..128 columns");
        const int64_t len = block_end - b0;
        AIMET_REQUIRE(len % D == 0 && s0 % D == 0 && s1 % D == 0, "block length, s0 and s1 must be multiples of vector_dim");
        AIMET_REQUIRE(0 <= s0 && s0 <= s1 && s1 <= len, "step range outside the block");
        AIMET_REQUIRE(ld >= block_end && hinv_ld >= block_end, "block_end beyond ld or hinv_ld");
        AIMET_REQUIRE(rows < kTwo31 && ld < kTwo31 && rows * ld < kTwo31, "block update needs fewer than 2^31 weight elements");
        AIMET_REQUIRE(hinv_ld < kTwo31 && hinv_ld * block_end < kTwo31, "block update needs fewer than 2^31 hinv elements");
        AIMET_REQUIRE((rows / rows_per_block) * K * D < kTwo31, "block update needs fewer than 2^31 codebook elements");
        require_device_ptr(w, "weight");
        require_device_ptr(codebook, "codebook");
        require_device_ptr(hinv, "hinv");
        require_device_ptr(err, "err");
        require_device_ptr(indices, "indices");
        if (s0 == s1)
            return;
        UpdateArgs a {w, ld, rows, (int) rows_per_block, (int) b0, (int) s0, (int) s1, (int) len, D, K,
                      codebook, hinv, hinv_ld, err, indices};
        hipStream_t s    = as_stream(stream);
        const int layout = g_update_layout.load();
        switch (D)
        {
        case 1: launch_update<1>(a, layout, s); break;
        case 2: launch_update<2>(a, layout, s); break;
        case 4: launch_update<4>(a, layout, s); break;
        default: launch_update<0>(a, layout, s); break;
        }
        AIMET_LAUNCH_CHECK();
    });
}

}   // extern "C"
