// The matrix-core weight gradient of the grouped 1x1 convolutions: defined in conv1x1_wgrad.hip, asked and launched by the weight
// gradient's one planner and its launchers (conv_bwd.hip).  G groups of M output and K input channels, P pixels per plane.
#pragma once

#include "common.hpp"

namespace mspl {

// 0 = launched (gw accumulated into); 1 = not this form's shape
int conv1x1_wgrad_mfma_try(const float* gy, const float* x, int N, int G, int M, int K, int P, float* gw, hipStream_t s);
// what _try would do, without doing it: 0 and the waves per tile / 64-pixel groups of the reduction range, or 1
int conv1x1_wgrad_mfma_plan(int N, int G, int M, int K, int P, int* nslots, int* ngroups);
// the leading problems of a run that fit the kernel, in one launch; returns how many it took (0: the first one does not fit)
int conv1x1_wgrad_mfma_batch(const float* const* gy, const float* const* x, float* const* gw, const float* const* rowscale, const int* N,
                             const int* G, const int* M, const int* K, const int* P, int nprob, hipStream_t s);

}  // namespace mspl
