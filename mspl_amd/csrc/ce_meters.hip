// The loss and meter half of one train_seg_ue iteration (utilities/train_eval_seg.py:202-222) after `outputs + 0.5 * out_aux`:
//     loss  = CrossEntropyLoss(weight, ignore_index)(o, target).mean()     = sum_valid w[t] * (lse(o) - o[t]) / sum_valid w[t]
//     areas = MIOU(num_classes - 1).get_iou(o, target)                     argmax, the reference's uint8 +1 arithmetic, three histograms
//     loss  = (loss - b).abs() + b;  losses.update(loss.item(), inputs.size(0))
// The reference reads the full-size logits for the loss, copies prediction and target to the host for three torch.histc calls and
// synchronises once more for loss.item().  Here ONE pass over the logits gives the cross-entropy sums and the areas, and a
// one-thread launch floods the loss, adds it to the epoch's meter and clears the sums: nothing leaves the device.
#include <algorithm>

#include "common.hpp"
#include "loss_parts.hpp"

namespace mspl {

// One thread per pixel, lanes along the pixels of a class plane: every one of the C loads of a wave is 256 contiguous bytes.
// CT > 0: the class count at compile time -- the C loads are issued together and the logits stay in registers for the maximum, the
// exponentials and o[t]; CT == 0: any C, streamed with a running log-sum-exp (first maximum by the strict '>', like torch.max).
template <int CT>
__global__ __launch_bounds__(256) void ce_meters_kernel(const float* __restrict__ pred, const int64_t* __restrict__ target,
                                                        const float* __restrict__ cw, int ignore, int Crt, int HW, int K,
                                                        int64_t total, double* __restrict__ sums,
                                                        unsigned long long* __restrict__ areas) {
    __shared__ unsigned int hsh[3 * MIOU_MAX_BINS];
    const int C = CT > 0 ? CT : Crt;
    if (areas) {
        miou_clear(hsh, K);
        __syncthreads();
    }
    // grid-stride with a bounded grid: a workgroup ends with two atomics on the same two addresses (losses.hip, wce_fwd_kernel)
    double s_loss = 0.0, s_w = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t n = idx / HW;
        const float* a = pred + (size_t)n * C * HW + (idx - n * HW);
        const int64_t t64 = target[idx];
        const bool valid = t64 >= 0 && t64 < C && t64 != (int64_t)ignore;
        const unsigned t8 = miou_label_code(t64);
        if (!valid && (t8 == 0 || !areas)) continue;           // the pixel counts nowhere: its logits are not read
        float lse, ot = 0.f;
        int best = 0;
        if (CT > 0) {
            float v[CT > 0 ? CT : 1];
#pragma unroll
            for (int c = 0; c < CT; ++c) v[c] = a[(size_t)c * HW];
            float m = v[0];
#pragma unroll
            for (int c = 1; c < CT; ++c) if (v[c] > m) { m = v[c]; best = c; }
            float S = 0.f;
#pragma unroll
            for (int c = 0; c < CT; ++c) { S += expf(v[c] - m); if ((int64_t)c == t64) ot = v[c]; }
            lse = m + logf(S);
        } else {
            float m = -INFINITY, S = 0.f;
            for (int c = 0; c < C; ++c) {
                const float o = a[(size_t)c * HW];
                if (o > m) { S = S * expf(m - o) + 1.f; m = o; best = c; }
                else S += expf(o - m);
                if ((int64_t)c == t64) ot = o;
            }
            lse = m + logf(S);
        }
        if (valid) {
            const float w = cw ? cw[t64] : 1.f;
            s_loss += (double)(w * (lse - ot));
            s_w += (double)w;
        }
        if (areas) miou_count(hsh, K, miou_codes8((unsigned)best, t8));
    }
    ce_sums_reduce(s_loss, s_w, sums);
    if (areas) miou_flush(hsh, K, areas);
}

// `.mean()` of the one-element loss, the flooding of :221 and AverageMeter.update(loss.item(), n) of :222 in fp32 and the reference's
// order; the sign is what torch's abs backward multiplies by (0 at equality).  The batch sums are cleared for the next step.
__global__ void ce_flood_finalize_kernel(double* __restrict__ sums, float b, double nimg, float* __restrict__ out3,
                                         double* __restrict__ meter) {
    const float den = (float)sums[1];
    const float l = (float)sums[0] / den;               // (NaN for a batch without a valid pixel, as CrossEntropyLoss)
    const float d = l - b;
    const float flooded = fabsf(d) + b;
    out3[0] = flooded;
    out3[1] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    out3[2] = den;
    if (meter) meter[0] += (double)flooded * nimg;
    sums[0] = 0.0;
    sums[1] = 0.0;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_ce_meters_fwd(const float* pred, const int64_t* target, const float* class_weights, int32_t ignore_index,
                                  int32_t N, int32_t C, int32_t HW, int32_t miou_classes, double* sums, unsigned long long* areas,
                                  void* stream) {
    MSPL_REQUIRE(pred && target && sums, MSPL_ERR_NULL_POINTER, "ce_meters: null pointer");
    MSPL_REQUIRE(N > 0 && C > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "ce_meters: bad shape N=%d C=%d HW=%d", N, C, HW);
    MSPL_REQUIRE(miou_classes >= 1 && miou_classes <= 64, MSPL_ERR_UNSUPPORTED, "ce_meters: %d MIOU classes (1..64)", miou_classes);
    const int64_t total = (int64_t)N * HW;
    const int64_t blocks = std::min<int64_t>(ceil_div64(total, 256), 2048);
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
#define MSPL_CE_METERS(CT) \
    hipLaunchKernelGGL((ce_meters_kernel<CT>), grid, block, 0, st, pred, target, class_weights, ignore_index, C, HW, miou_classes, total, sums, areas)
    switch (C) {
        case 5: MSPL_CE_METERS(5); break;         // greenhouse
        case 13: MSPL_CE_METERS(13); break;       // camvid
        case 20: MSPL_CE_METERS(20); break;       // cityscapes
        default: MSPL_CE_METERS(0); break;
    }
#undef MSPL_CE_METERS
    MSPL_CHECK_LAUNCH("ce_meters_fwd");
    return MSPL_OK;
}

extern "C" int mspl_ce_flood_finalize(double* sums, float flood_level, int32_t batch_images, float* out3, double* meter, void* stream) {
    MSPL_REQUIRE(sums && out3, MSPL_ERR_NULL_POINTER, "ce_flood_finalize: null pointer");
    MSPL_REQUIRE(batch_images > 0, MSPL_ERR_BAD_SHAPE, "ce_flood_finalize: %d images", batch_images);
    hipLaunchKernelGGL(ce_flood_finalize_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sums, flood_level, (double)batch_images, out3,
                       meter);
    MSPL_CHECK_LAUNCH("ce_flood_finalize");
    return MSPL_OK;
}
