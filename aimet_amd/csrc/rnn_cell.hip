// rnn_cell.hip -- one fused time step of a quantized recurrent layer (aimet_torch/v1/
// qc_quantize_recurrent.py: the reference walks the sequence in Python and, per layer, direction and
// step, calls a library cell, replaces the rows of ended sequences, quantize-dequantizes or measures
// each state tensor, and appends to lists it later stacks, flips and concatenates).
//
//  * aimet_rnn_step: for up to AIMET_RNN_MAX_JOBS independent jobs (the two directions of a
//    bidirectional layer) in ONE launch: the biases added to the raw products x W_ih^T and
//    h W_hh^T, the gate non-linearities, the state update, the rows at or beyond `valid_rows` kept,
//    the QDQ of h and c (mode ACTIVE, quantizer enabled), the new state written, and h written into
//    its row of the layer's [T, B, D H] output slab. The time index of a row is an argument: `step`
//    for a forward job, len(row) - 1 - step for a reverse one (the sequence's own length with packed
//    input), so neither the input nor the output is flipped, shifted or concatenated.
//  * Arithmetic: rnn_math.hpp (sigmoid and tanh in written-out float32 operations); the cell in the
//    evaluation order of torch's CPU cells, (ig + b_ih) + (hg + b_hh) and so on; the QDQ of
//    common.hpp with the IEEE divide. tests/rnn_oracle.py restates all of it; equal inputs give equal bits.
//  * Shape: an element map. A lane takes four consecutive columns of one row (16-byte accesses that
//    need only 4-byte alignment, so any H and any base work), the last lane of a row the H mod 4
//    columns left, one at a time. No LDS, no atomics, no grid-wide synchronisation; the job table
//    travels in the kernel arguments, so a captured step loop is a chain of plain kernel nodes.

#include "common.hpp"
#include "rnn_math.hpp"

namespace aimet_amd
{

QdqParams tensor_params(const aimet_tf_encoding& enc);   // qdq.hip

namespace
{

constexpr int kBlk = 256;

LaunchCounter g_launches;

// four floats that need the alignment of one
struct F4
{
    float v[4];
};

struct StepJob
{
    const float *ig, *hg, *b_ih, *b_hh, *h_prev, *c_prev;
    float *h_next, *c_next, *out;
    const int32_t* lens;
    int64_t ig_step_stride, ig_row_stride, hg_row_stride, out_step_stride, out_row_stride;
    int reverse;
};

struct StepArgs
{
    StepJob job[AIMET_RNN_MAX_JOBS];
    int B, H, units, T, step, valid_rows;   // units: lanes per row, ceil(H / 4)
    int h_qdq, c_qdq;
    QdqParams hp, cp;
};

// w of the four floats at p (w == 4: one 16-byte access), the rest zero
__device__ __forceinline__ void load4(float (&d)[4], const float* p, int w)
{
    if (w == 4)
    {
        const F4 f = *reinterpret_cast<const F4*>(p);
        d[0] = f.v[0], d[1] = f.v[1], d[2] = f.v[2], d[3] = f.v[3];
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        d[k] = k < w ? p[k] : 0.0f;
}

__device__ __forceinline__ void store4(float* p, const float (&s)[4], int w)
{
    if (w == 4)
    {
        *reinterpret_cast<F4*>(p) = F4 {{s[0], s[1], s[2], s[3]}};
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < w)
            p[k] = s[k];
}

// gate g of this lane's columns: (ig + b_ih) and (hg + b_hh), each bias optional
__device__ __forceinline__ void load_gate(float (&gi)[4], float (&gh)[4], const float* ig, const float* hg,
                                          const float* b_ih, const float* b_hh, int at, int w)
{
    float b[4];
    load4(gi, ig + at, w);
    load4(gh, hg + at, w);
    if (b_ih)
    {
        load4(b, b_ih + at, w);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            gi[k] = gi[k] + b[k];
    }
    if (b_hh)
    {
        load4(b, b_hh + at, w);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            gh[k] = gh[k] + b[k];
    }
}

template <int MODE>
__global__ __launch_bounds__(kBlk) void rnn_step_kernel(const StepArgs a)
{
    using namespace rnn_math;
    const StepJob& j = a.job[blockIdx.y];
    const int64_t u  = (int64_t) blockIdx.x * kBlk + threadIdx.x;
    if (u >= (int64_t) a.B * a.units)
        return;
    const int b      = (int) (u / a.units);
    const int col    = (int) (u - (int64_t) b * a.units) * 4;
    const int w      = a.H - col < 4 ? a.H - col : 4;
    const int H      = a.H;
    const int64_t at = (int64_t) b * H + col;
    // the row's time index; a reverse row whose sequence has ended (index below zero) is kept, whatever
    // valid_rows says, so that no table of lengths can send an access outside the slab
    int64_t t = a.step;
    if (j.reverse)
        t = (int64_t) (j.lens ? j.lens[b] : a.T) - 1 - a.step;
    const bool live = b < a.valid_rows && t >= 0 && t < a.T;

    float h[4], c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    load4(h, j.h_prev + at, w);
    if (MODE == AIMET_RNN_LSTM)
        load4(c, j.c_prev + at, w);

    if (live)
    {
        const float* ig = j.ig + t * j.ig_step_stride + (int64_t) b * j.ig_row_stride;
        const float* hg = j.hg + (int64_t) b * j.hg_row_stride;
        float gi[4], gh[4];
        if (MODE == AIMET_RNN_LSTM)
        {
            float gate[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
            {
                load_gate(gi, gh, ig, hg, j.b_ih, j.b_hh, g * H + col, w);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    gate[g][k] = gi[k] + gh[k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const float i_ = sigmoid_r(gate[0][k]), f_ = sigmoid_r(gate[1][k]);
                const float g_ = tanh_r(gate[2][k]), o_ = sigmoid_r(gate[3][k]);
                c[k]           = (f_ * c[k]) + (i_ * g_);
                h[k]           = o_ * tanh_r(c[k]);
            }
        }
        else if (MODE == AIMET_RNN_GRU)
        {
            float r[4], z[4];
            load_gate(gi, gh, ig, hg, j.b_ih, j.b_hh, col, w);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                r[k] = sigmoid_r(gh[k] + gi[k]);
            load_gate(gi, gh, ig, hg, j.b_ih, j.b_hh, H + col, w);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                z[k] = sigmoid_r(gh[k] + gi[k]);
            load_gate(gi, gh, ig, hg, j.b_ih, j.b_hh, 2 * H + col, w);
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const float n = tanh_r(gi[k] + (gh[k] * r[k]));
                h[k]          = ((h[k] - n) * z[k]) + n;
            }
        }
        else
        {
            load_gate(gi, gh, ig, hg, j.b_ih, j.b_hh, col, w);
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const float s = gh[k] + gi[k];
                h[k]          = MODE == AIMET_RNN_TANH ? tanh_r(s) : (s > 0.0f ? s : 0.0f);
            }
        }
    }
    // the reference quantizes the whole state after the row replacement, kept rows included
    if (a.h_qdq)
    {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            h[k] = dequantize(quantize_nearest(h[k], a.hp), a.hp);
    }
    store4(j.h_next + at, h, w);
    if (MODE == AIMET_RNN_LSTM)
    {
        if (a.c_qdq)
        {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                c[k] = dequantize(quantize_nearest(c[k], a.cp), a.cp);
        }
        store4(j.c_next + at, c, w);
    }
    if (live)
        store4(j.out + t * j.out_step_stride + (int64_t) b * j.out_row_stride + col, h, w);
}

bool aligned4(const void* p)
{
    return (reinterpret_cast<uintptr_t>(p) & 3) == 0;
}

}   // namespace
}   // namespace aimet_amd

using namespace aimet_amd;

extern "C" {

int aimet_rnn_step(int mode, const aimet_rnn_step_job* jobs, int count, int64_t B, int64_t H, int64_t T, int64_t step,
                   int64_t valid_rows, const aimet_tf_encoding* h_enc, int h_enabled, const aimet_tf_encoding* c_enc,
                   int c_enabled, int op_mode, void* stream)
{
    return guarded([&] {
        AIMET_REQUIRE(mode >= AIMET_RNN_LSTM && mode <= AIMET_RNN_RELU, "recurrent step: mode must be LSTM, GRU, "
                                                                        "RNN_TANH or RNN_RELU");
        AIMET_REQUIRE(jobs != nullptr && count >= 1 && count <= AIMET_RNN_MAX_JOBS,
                      "recurrent step: 1 or 2 jobs per launch");
        AIMET_REQUIRE(B > 0 && H > 0 && T > 0, "recurrent step: B, H and T must be positive");
        AIMET_REQUIRE(H < (int64_t(1) << 28) && B < (int64_t(1) << 31) && T < (int64_t(1) << 31) &&
                          B * ceil_div(H, 4) < (int64_t(1) << 31),
                      "recurrent step: too large (B * ceil(H / 4) must stay below 2^31)");
        AIMET_REQUIRE(step >= 0 && step < T, "recurrent step: step must lie in [0, T)");
        AIMET_REQUIRE(valid_rows >= 0 && valid_rows <= B, "recurrent step: valid_rows must lie in [0, B]");
        AIMET_REQUIRE(op_mode >= AIMET_RNN_OP_PASSTHROUGH && op_mode <= AIMET_RNN_OP_ACTIVE,
                      "recurrent step: the op mode must be PASSTHROUGH, ANALYSIS or ACTIVE");
        const bool lstm = mode == AIMET_RNN_LSTM;
        const int64_t G = lstm ? 4 : (mode == AIMET_RNN_GRU ? 3 : 1);
        StepArgs a {};
        a.B = (int) B, a.H = (int) H, a.units = (int) ceil_div(H, 4), a.T = (int) T, a.step = (int) step;
        a.valid_rows = (int) valid_rows;
        const bool active = op_mode == AIMET_RNN_OP_ACTIVE;
        a.h_qdq = active && h_enabled, a.c_qdq = active && c_enabled && lstm;
        if (a.h_qdq)
        {
            AIMET_REQUIRE(h_enc != nullptr, "recurrent step: the enabled h quantizer has no encoding");
            a.hp = tensor_params(*h_enc);
        }
        if (a.c_qdq)
        {
            AIMET_REQUIRE(c_enc != nullptr, "recurrent step: the enabled c quantizer has no encoding");
            a.cp = tensor_params(*c_enc);
        }
        for (int n = 0; n < count; ++n)
        {
            const aimet_rnn_step_job& j = jobs[n];
            require_device_ptr(j.ig, "recurrent step input product");
            require_device_ptr(j.hg, "recurrent step hidden product");
            require_device_ptr(j.h_prev, "recurrent step h_prev");
            require_device_ptr(j.h_next, "recurrent step h_next");
            require_device_ptr(j.out, "recurrent step output slab");
            if (lstm)
            {
                require_device_ptr(j.c_prev, "recurrent step c_prev");
                require_device_ptr(j.c_next, "recurrent step c_next");
            }
            if (j.b_ih)
                require_device_ptr(j.b_ih, "recurrent step b_ih");
            if (j.b_hh)
                require_device_ptr(j.b_hh, "recurrent step b_hh");
            if (j.lens)
                require_device_ptr(j.lens, "recurrent step sequence lengths");
            AIMET_REQUIRE(aligned4(j.ig) && aligned4(j.hg) && aligned4(j.h_prev) && aligned4(j.h_next) &&
                              aligned4(j.out) && aligned4(j.c_prev) && aligned4(j.c_next) && aligned4(j.b_ih) &&
                              aligned4(j.b_hh) && aligned4(j.lens),
                          "recurrent step: misaligned pointer");
            AIMET_REQUIRE(j.ig_row_stride >= G * H && j.hg_row_stride >= G * H && j.out_row_stride >= H &&
                              j.ig_step_stride >= 0 && j.out_step_stride >= 0,
                          "recurrent step: a row stride is shorter than its row");
            a.job[n] = StepJob {j.ig, j.hg, j.b_ih, j.b_hh, j.h_prev, j.c_prev, j.h_next, j.c_next, j.out, j.lens,
                                j.ig_step_stride, j.ig_row_stride, j.hg_row_stride, j.out_step_stride,
                                j.out_row_stride, j.reverse != 0};
        }
        hipStream_t s = as_stream(stream);
        const dim3 grid((unsigned) ceil_div(B * a.units, kBlk), (unsigned) count);
        switch (mode)
        {
        case AIMET_RNN_LSTM: rnn_step_kernel<AIMET_RNN_LSTM><<<grid, kBlk, 0, s>>>(a); break;
        case AIMET_RNN_GRU: rnn_step_kernel<AIMET_RNN_GRU><<<grid, kBlk, 0, s>>>(a); break;
        case AIMET_RNN_TANH: rnn_step_kernel<AIMET_RNN_TANH><<<grid, kBlk, 0, s>>>(a); break;
        default: rnn_step_kernel<AIMET_RNN_RELU><<<grid, kBlk, 0, s>>>(a); break;
        }
        AIMET_LAUNCH_CHECK();
        g_launches.add(1);
    });
}

int aimet_rnn_launch_count(int64_t* count, int reset)
{
    return guarded([&] { g_launches.read(count, reset); });
}

}   // extern "C"
