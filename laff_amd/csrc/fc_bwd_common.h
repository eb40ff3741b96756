// fc_bwd_common.h -- what the two backward kernels of the FC projection share: fc_bwd.hip (dense X) and fc_gather_bwd.hip (sparse X).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace laff {

// dz = da * act'(a) from the forward's output a; at most three roundings, and dact(0, 0) = 0 for every activation
template <int ACT>
__device__ __forceinline__ float dact(float a, float g) {
    if constexpr (ACT == LAFF_ACT_TANH) return g * fmaf(-a, a, 1.0f);
    else if constexpr (ACT == LAFF_ACT_SIGMOID) return g * (a * (1.0f - a));
    else if constexpr (ACT == LAFF_ACT_RELU) return a > 0.0f ? g : 0.0f;
    else return g;
}

}  // namespace laff
