// rnn_math_host.cpp -- aimet_amd/csrc/rnn_math.hpp compiled for the host, for rnn_math_sweep.py:
// the kernel's sigmoid and tanh over arrays, as a small shared library.
//   g++ -O2 -ffp-contract=off -shared -fPIC -I aimet_amd/csrc -o rnn_math_host.so tools/studies/rnn_math_host.cpp
#include <cstdint>

#include "rnn_math.hpp"

extern "C" {

void rnn_sigmoid_many(const float* x, float* y, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        y[i] = aimet_amd::rnn_math::sigmoid_r(x[i]);
}

void rnn_tanh_many(const float* x, float* y, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        y[i] = aimet_amd::rnn_math::tanh_r(x[i]);
}

}   // extern "C"
