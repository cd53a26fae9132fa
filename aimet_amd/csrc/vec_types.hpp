// vec_types.hpp -- the 16-B register vector of the kernels: four floats, one global_load_dwordx4 /
// ds_read_b128. Its own header (nothing else in it) so that fast_pow.hpp, which the stand-alone
// studies include without the C ABI on their include path, can take it too; everything else gets
// it through common.hpp.
#pragma once

namespace aimet_amd
{

typedef float f4 __attribute__((ext_vector_type(4)));

}   // namespace aimet_amd
