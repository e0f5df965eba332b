// Host-side plan of the split-K 1x1 form: decided in conv1x1_splitk.hip, asked by the one decision function of mspl_conv1x1_fwd
// (conv1x1.hip, pw_decide), which the launcher and mspl_conv1x1_fwd_plan both call.  No device call, no state.
#pragma once

#include "common.hpp"

namespace mspl {

struct SkPlan {
    int nsub;        // 32-pixel sub-tiles per workgroup (1, 2)
    int ch;          // MFMA steps (2 k each) per chunk whose loads are issued together: an instantiation (8, 16)
    int ks;          // k per wave = K / 4, a multiple of 2 * ch
    int tiles;       // pixel tiles per image (32 * nsub pixels each)
    int64_t blocks;  // N * groups * tiles workgroups
};

// 0 = the split-K form takes the shape (p filled); 1 = not this form's (the caller continues with the other matrix-core forms).
// lean: the call has no pre_add / residual / reinforcement / gate (the kernel applies scale, shift, alpha and raw_out only).
int conv1x1_splitk_plan(int N, int M, int K, int groups, int HW, bool lean, SkPlan* p);
void conv1x1_splitk_launch(const float* x, const float* w, int N, int M, int K, int groups, int HW, const SkPlan& p, const Epi& e,
                           float* out, hipStream_t s);

}  // namespace mspl
