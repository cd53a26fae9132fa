// qdq_tile_sweep.hip -- lanes-per-workgroup sweep (64 / 128 / 256) of the streaming fp32 QDQ kernels,
// timed through the library itself (aimet_qdq_tile_lanes selects the shape, so every variant is the
// shipped kernel and launch path; 256 lanes is the form before the shape became a parameter).
// Build (from the repository root, after the library):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include tools/studies/qdq_tile_sweep.hip
//         -o tools/studies/qdq_tile_sweep -L aimet_amd -laimet_amd -Wl,-rpath,'$ORIGIN/../../aimet_amd'
// Run: tools/studies/qdq_tile_sweep [reps = 25] [warm = 5]
//
// Method. The flagship step runs 55 per-tensor launches back to back from a HIP graph over tensors
// that are all different (11.5 GB read per step: nothing is found in the 256 MiB Infinity Cache).
// So one sample here is a HIP graph of k launches of one size walking a 2 GiB + 2 GiB pool once
// (k = pool / size: 83 launches at 6.4 M elements, 2 at 205.5 M), and the shapes are interleaved
// 64 / 128 / 256 / 64 / ... inside one process; by the time a shape sees an address again 4 GiB
// have passed. Reported per (size, shape): median and best GB/s over the samples (8 B/elem; 12 for
// STE) and the median time of one launch. The batched plan is sampled the same way over 20 copies of
// the 54 ResNet-50 weight tensors (the table of (C, K) below), one plan per copy and shape.
// The summary weighs the six workload sizes by how often the ResNet-50 batch-256 forward has them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aimet_amd.h"

#define CK(x)                                                                                                  \
    do                                                                                                         \
    {                                                                                                          \
        hipError_t e_ = (x);                                                                                   \
        if (e_ != hipSuccess)                                                                                  \
        {                                                                                                      \
            printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);                             \
            exit(1);                                                                                           \
        }                                                                                                      \
    } while (0)
#define AK(x)                                                                                                  \
    do                                                                                                         \
    {                                                                                                          \
        if ((x) != AIMET_OK)                                                                                   \
        {                                                                                                      \
            printf("aimet error at line %d: %s\n", __LINE__, aimet_last_error());                             \
            exit(1);                                                                                           \
        }                                                                                                      \
    } while (0)

static const int kShapes[3]     = {64, 128, 256};
static const int64_t kPoolElems = int64_t(1) << 29;   // 2 GiB in + 2 GiB out

// activation sizes of the ResNet-50 batch-256 forward and how many of its 55 tensors have them
// (the other two are the input, 38.5 M, and the fc output, 0.26 M)
struct Size
{
    int64_t n;
    int count;
};
static const Size kSizes[] = {{6422528, 5},   {12845056, 11}, {25690112, 12},       {51380224, 14},
                              {102760448, 6}, {205520896, 5}, {int64_t(1) << 28, 0}};

// the 54 conv / fc weights of ResNet-50 as (C, K) = (out channels, in channels x kh x kw)
struct CK2
{
    int C, K;
};
static const CK2 kWeights[54] = {
    {64, 147},                                                                                 // conv1
    {64, 64},     {64, 576},   {256, 64},   {256, 64},                                         // layer1.0 (+ downsample)
    {64, 256},    {64, 576},   {256, 64},   {64, 256},    {64, 576},   {256, 64},              // layer1.1-2
    {128, 256},   {128, 1152}, {512, 128},  {512, 256},                                        // layer2.0
    {128, 512},   {128, 1152}, {512, 128},  {128, 512},   {128, 1152}, {512, 128},             // layer2.1-2
    {128, 512},   {128, 1152}, {512, 128},                                                     // layer2.3
    {256, 512},   {256, 2304}, {1024, 256}, {1024, 512},                                       // layer3.0
    {256, 1024},  {256, 2304}, {1024, 256}, {256, 1024},  {256, 2304}, {1024, 256},            // layer3.1-2
    {256, 1024},  {256, 2304}, {1024, 256}, {256, 1024},  {256, 2304}, {1024, 256},            // layer3.3-4
    {256, 1024},  {256, 2304}, {1024, 256},                                                    // layer3.5
    {512, 1024},  {512, 4608}, {2048, 512}, {2048, 1024},                                      // layer4.0
    {512, 2048},  {512, 4608}, {2048, 512}, {512, 2048},  {512, 4608}, {2048, 512},            // layer4.1-2
    {1000, 2048}};                                                                             // fc

__global__ __launch_bounds__(256) void fill_kernel(float* p, int64_t n)
{
    const int64_t stride = (int64_t) gridDim.x * 256;
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
    {
        uint64_t z = 0x9E3779B97F4A7C15ull * (uint64_t) (i + 1);
        z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z ^= z >> 31;
        p[i] = ((float) (uint32_t) (z >> 40) * (1.0f / 16777216.0f) - 0.5f) * 12.0f;   // U(-6, 6)
    }
}

struct Series
{
    hipGraphExec_t exec[3] = {};
    int launches           = 0;
    double bytes           = 0;   // per launch
    std::vector<float> ms[3];
};

template <class F>
static void capture(Series& s, int shape, hipStream_t st, F&& launches)
{
    AK(aimet_qdq_tile_lanes(kShapes[shape], nullptr));
    hipGraph_t g;
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    launches();
    CK(hipStreamEndCapture(st, &g));
    CK(hipGraphInstantiate(&s.exec[shape], g, nullptr, nullptr, 0));
    CK(hipGraphDestroy(g));
}

static void sample(std::vector<Series*>& all, int reps, int warm, hipStream_t st)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (Series* s: all)
        for (int r = 0; r < warm + reps; ++r)
            for (int k = 0; k < 3; ++k)   // 64 / 128 / 256 interleaved
            {
                CK(hipEventRecord(e0, st));
                CK(hipGraphLaunch(s->exec[k], st));
                CK(hipEventRecord(e1, st));
                CK(hipEventSynchronize(e1));
                float ms;
                CK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= warm)
                    s->ms[k].push_back(ms / s->launches);
            }
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
}

static float median(std::vector<float> v)
{
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

static void report(const char* what, const char* label, Series& s)
{
    for (int k = 0; k < 3; ++k)
    {
        float med = median(s.ms[k]), best = *std::min_element(s.ms[k].begin(), s.ms[k].end());
        printf("%-10s %-22s lanes %3d  x%-3d  median %9.2f us  %7.1f GB/s   best %7.1f GB/s\n", what, label,
               kShapes[k], s.launches, med * 1e3, s.bytes / med / 1e6, s.bytes / best / 1e6);
    }
}

int main(int argc, char** argv)
{
    const int reps = std::max(20, argc > 1 ? atoi(argv[1]) : 25);
    const int warm = std::max(5, argc > 2 ? atoi(argv[2]) : 5);
    float *in, *out;
    CK(hipMalloc(&in, kPoolElems * 4));
    CK(hipMalloc(&out, kPoolElems * 4));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    fill_kernel<<<2048, 256, 0, st>>>(in, kPoolElems);
    CK(hipGetLastError());
    CK(hipMemsetAsync(out, 0, kPoolElems * 4, st));
    CK(hipStreamSynchronize(st));
    const aimet_tf_encoding enc {-3.1, 5.7, 0.0, 0.0, 8};

    // ---- per-tensor QDQ --------------------------------------------------------------------
    const int nsizes = (int) (sizeof(kSizes) / sizeof(kSizes[0]));
    std::vector<Series> tensor((size_t) nsizes);
    for (int i = 0; i < nsizes; ++i)
    {
        const int64_t n    = kSizes[i].n;
        tensor[i].launches = (int) (kPoolElems / n);
        tensor[i].bytes    = 8.0 * n;
        for (int k = 0; k < 3; ++k)
            capture(tensor[i], k, st, [&] {
                for (int j = 0; j < tensor[i].launches; ++j)
                    AK(aimet_qdq_per_tensor(in + j * n, out + j * n, n, &enc, AIMET_ROUND_NEAREST, 0, st));
            });
    }

    // ---- per-channel QDQ (one launch, [256][64][12544]) and STE backward at 205.5 M -----------
    const int64_t nbig = 205520896;
    float* table64;
    {
        std::vector<float> t(4 * 64);
        for (int c = 0; c < 64; ++c)
        {
            float d    = 0.02f + 0.001f * c;
            t[c]       = d * -90.0f;
            t[64 + c]  = d * 165.0f;
            t[128 + c] = d;
            t[192 + c] = -90.0f;
        }
        CK(hipMalloc(&table64, t.size() * 4));
        CK(hipMemcpy(table64, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    }
    Series channel, ste;
    channel.launches = 2;
    channel.bytes    = 8.0 * nbig;
    ste.launches     = 1;   // x and grad are the two halves of the input pool
    ste.bytes        = 12.0 * nbig;
    for (int k = 0; k < 3; ++k)
    {
        capture(channel, k, st, [&] {
            for (int j = 0; j < 2; ++j)
                AK(aimet_qdq_per_channel(in + j * nbig, out + j * nbig, 256, 64, 12544, table64,
                                         AIMET_ROUND_NEAREST, 0, st));
        });
        capture(ste, k, st,
                [&] { AK(aimet_ste_backward_per_tensor(in, in + nbig, out, nbig, -3.1f, 5.7f, st)); });
    }

    // ---- the same form in other files: fp16 round trip (broadcast.hip) and learned-grid forward
    //      (learned_grid.hip, [4096][65536] per-channel as benchmarks/kernel_roofline.py) at 2^28 -----
    const int64_t n28 = int64_t(1) << 28;
    float* lgenc;   // delta[4096], offset[4096]
    {
        std::vector<float> t(2 * 4096);
        for (int c = 0; c < 4096; ++c)
        {
            t[c]        = 0.02f + 0.00001f * c;
            t[4096 + c] = -128.0f;
        }
        CK(hipMalloc(&lgenc, t.size() * 4));
        CK(hipMemcpy(lgenc, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    }
    Series fp16, lg;
    fp16.launches = lg.launches = 2;
    fp16.bytes = lg.bytes = 8.0 * n28;
    for (int k = 0; k < 3; ++k)
    {
        capture(fp16, k, st, [&] {
            for (int j = 0; j < 2; ++j)
                AK(aimet_qdq_fp16(in + j * n28, out + j * n28, n28, st));
        });
        capture(lg, k, st, [&] {
            for (int j = 0; j < 2; ++j)
                AK(aimet_lg_forward(in + j * n28, out + j * n28, 1, 4096, 65536, lgenc, lgenc + 4096, 255.0f, st));
        });
    }

    // ---- batched plan: 20 copies of the 54 weights, one plan per copy and shape ------------------
    int64_t wtotal = 0, channels = 0;
    for (const CK2& w: kWeights)
    {
        wtotal += (int64_t) w.C * w.K;
        channels += w.C;
    }
    const int copies = (int) std::min<int64_t>(20, kPoolElems / wtotal);
    std::vector<float*> tables;
    for (const CK2& w: kWeights)
    {
        std::vector<float> t(4 * (size_t) w.C);
        for (int c = 0; c < w.C; ++c)
        {
            float d          = 0.01f + 0.0001f * (c % 97);
            t[c]             = d * -128.0f;
            t[w.C + c]       = d * 127.0f;
            t[2 * w.C + c]   = d;
            t[3 * w.C + c]   = -128.0f;
        }
        float* dt;
        CK(hipMalloc(&dt, t.size() * 4));
        CK(hipMemcpy(dt, t.data(), t.size() * 4, hipMemcpyHostToDevice));
        tables.push_back(dt);
    }
    Series batch;
    batch.launches = copies;
    batch.bytes    = 8.0 * wtotal;
    std::vector<aimet_qdq_plan*> plans;
    for (int k = 0; k < 3; ++k)
    {
        AK(aimet_qdq_tile_lanes(kShapes[k], nullptr));   // a plan keeps the shape it is created with
        std::vector<aimet_qdq_plan*> mine;
        for (int c = 0; c < copies; ++c)
        {
            std::vector<aimet_qdq_channel_desc> d;
            int64_t off = (int64_t) c * wtotal;
            for (size_t i = 0; i < 54; ++i)
            {
                d.push_back({in + off, out + off, 1, kWeights[i].C, kWeights[i].K, tables[i]});
                off += (int64_t) kWeights[i].C * kWeights[i].K;
            }
            aimet_qdq_plan* p;
            AK(aimet_qdq_channel_plan_create(d.data(), (int64_t) d.size(), 0, &p));
            mine.push_back(p);
            plans.push_back(p);
        }
        capture(batch, k, st, [&] {
            for (aimet_qdq_plan* p: mine)
                AK(aimet_qdq_channel_plan_run(p, AIMET_ROUND_NEAREST, 0, st));
        });
    }
    AK(aimet_qdq_tile_lanes(0, nullptr));

    std::vector<Series*> all;
    for (Series& s: tensor)
        all.push_back(&s);
    all.push_back(&channel);
    all.push_back(&ste);
    all.push_back(&fp16);
    all.push_back(&lg);
    all.push_back(&batch);
    sample(all, reps, warm, st);

    printf("qdq_tile_sweep: %d samples after %d warm-ups per (size, shape); a sample = one graph of xN launches\n",
           reps, warm);
    char label[64];
    for (int i = 0; i < nsizes; ++i)
    {
        snprintf(label, sizeof label, "%lld", (long long) kSizes[i].n);
        report("per-tensor", label, tensor[i]);
    }
    report("per-chan", "256x64x12544", channel);
    report("ste", "205520896", ste);
    report("fp16", "268435456", fp16);
    report("lg-fwd", "4096x65536", lg);
    snprintf(label, sizeof label, "54 weights, %lld el", (long long) wtotal);
    report("batched", label, batch);
    printf("batched: %lld channels, %d copies\n", (long long) channels, copies);

    // byte-weighted over the workload's sizes: the time of the 53 launches of these sizes per step
    printf("\nper-tensor, the workload's 53 launches of the six sizes (count x median launch time):\n");
    double t256 = 0;
    for (int k = 2; k >= 0; --k)
    {
        double ms = 0, bytes = 0;
        for (int i = 0; i < nsizes; ++i)
        {
            ms += kSizes[i].count * (double) median(tensor[i].ms[k]);
            bytes += kSizes[i].count * tensor[i].bytes;
        }
        if (k == 2)
            t256 = ms;
        printf("  lanes %3d  %8.4f ms  %7.1f GB/s  %+6.2f %% time vs 256 lanes\n", kShapes[k], ms, bytes / ms / 1e6,
               (ms / t256 - 1.0) * 100.0);
    }

    for (aimet_qdq_plan* p: plans)
        AK(aimet_qdq_channel_plan_destroy(p));
    for (int k = 0; k < 3; ++k)
    {
        for (Series* s: all)
            CK(hipGraphExecDestroy(s->exec[k]));
    }
    for (float* t: tables)
        CK(hipFree(t));
    CK(hipFree(table64));
    CK(hipFree(lgenc));
    CK(hipFree(in));
    CK(hipFree(out));
    return 0;
}
