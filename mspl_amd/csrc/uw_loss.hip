// The tail of a uest self-training step (uest_seg_multi_os.py:958-1089): the fused uncertainty-weighted loss (K11) with its
// closed-form gradients for both heads, and the flat Adam update (torch.optim.Adam semantics).
#include <stdlib.h>

#include <algorithm>

#include "common.hpp"

namespace mspl {

// ---- K11: loss = 20 * mean_pix( -w[t] * log_softmax(pred + 0.5 aux)[t] * exp(-kld) ) + mean_pix(kld),
//      kld = KL(softmax(pred) || softmax(aux)) per pixel (NOT detached: gradients flow through it, uest:1020-1023).
//      One thread per pixel: forward terms and the closed-form gradients w.r.t. pred and aux.
__global__ __launch_bounds__(256) void uw_loss_kernel(const float* __restrict__ pred, const float* __restrict__ aux,
                                                      const int64_t* __restrict__ target, const float* __restrict__ cw,
                                                      int N, int C, int HW, float ce_scale, float inv_npix,
                                                      float* __restrict__ loss_acc, float* __restrict__ gpred,
                                                      float* __restrict__ gaux, float* __restrict__ kld_out) {
    // grid-stride over the pixels with a bounded grid: every workgroup ends with ONE atomic on the same address, and a chain of
    // same-address device atomics advances at ~12-25 ns per link (one workgroup per 256 pixels: 7 680 links at 16 x 256x480)
    const int64_t total = (int64_t)N * HW;
    float contrib = 0.f;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int n = (int)(idx / HW), p = (int)(idx - (int64_t)n * HW);
        const float* pp = pred + (size_t)n * C * HW + p;
        const float* ap = aux + (size_t)n * C * HW + p;
        float m1 = -INFINITY, m2 = -INFINITY, mo = -INFINITY;
        for (int c = 0; c < C; ++c) {
            const float a = pp[(size_t)c * HW], b = ap[(size_t)c * HW];
            m1 = fmaxf(m1, a); m2 = fmaxf(m2, b); mo = fmaxf(mo, a + 0.5f * b);
        }
        float s1 = 0.f, s2 = 0.f, so = 0.f;
        for (int c = 0; c < C; ++c) {
            const float a = pp[(size_t)c * HW], b = ap[(size_t)c * HW];
            s1 += expf(a - m1); s2 += expf(b - m2); so += expf(a + 0.5f * b - mo);
        }
        const float l1 = m1 + logf(s1), l2 = m2 + logf(s2), lo = mo + logf(so);
        float kld = 0.f;
        for (int c = 0; c < C; ++c) {
            const float a = pp[(size_t)c * HW], b = ap[(size_t)c * HW];
            const float p1 = expf(a - l1);
            kld += p1 * (a - l1) - p1 * (b - l2);
        }
        const int t = (int)target[idx];
        const float wt = (t >= 0 && t < C) ? cw[t] : 0.f;
        const float ot = (t >= 0 && t < C) ? pp[(size_t)t * HW] + 0.5f * ap[(size_t)t * HW] : 0.f;
        const float nll = -(ot - lo);                      // -log_softmax(o)[t]
        const float u = expf(-kld);
        const float ce = wt * nll * u;                     // per-pixel weighted CE
        contrib += ce_scale * ce * inv_npix + kld * inv_npix;
        if (kld_out) kld_out[idx] = kld;
        if (gpred) {
            // d loss / d kld = (1 - ce_scale * ce) / npix ; d ce / d o_c = wt * u * (softmax(o)_c - [c == t])
            const float gk = (1.f - ce_scale * ce) * inv_npix;
            const float go = ce_scale * wt * u * inv_npix;
            for (int c = 0; c < C; ++c) {
                const float a = pp[(size_t)c * HW], b = ap[(size_t)c * HW];
                const float p1 = expf(a - l1), p2 = expf(b - l2), po = expf(a + 0.5f * b - lo);
                const float d = (a - l1) - (b - l2);       // log p1 - log p2
                const float dk_da = p1 * (d - kld);        // d kld / d pred_c
                const float dk_db = p1 - p2;               // d kld / d aux_c   (= -(p1 - p2) * -1 ... see derivation)
                const float dce = go * (po - (c == t ? 1.f : 0.f));
                gpred[(size_t)n * C * HW + (size_t)c * HW + p] = dce + gk * dk_da;
                gaux[(size_t)n * C * HW + (size_t)c * HW + p] = 0.5f * dce - gk * dk_db;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_down(contrib, o, 64);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = contrib;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss_acc, (part[0] + part[1]) + (part[2] + part[3]));
}

// ---- Adam (torch.optim.Adam semantics: L2 weight decay folded into the gradient, bias correction)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float lr, float b1, float b2, float omb1,
                                                   float omb2, float eps, float wd, float bc1, float bc2_sqrt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i] + wd * p[i];
    const float mi = b1 * m[i] + omb1 * gi;          // omb = 1 - beta rounded from double (torch's `value=1 - beta2`)
    const float vi = b2 * v[i] + omb2 * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] -= (lr / bc1) * (mi / denom);
}

}  // namespace mspl

using namespace mspl;

/* loss_acc (1 float, device) is ACCUMULATED into (caller zeroes).  gpred/gaux/kld_out may be NULL (forward only). */
static int uw_loss_launch(const float* pred, const float* aux, const int64_t* target, const float* class_weights, int32_t N, int32_t C,
                          int32_t HW, float ce_scale, float out_scale, float* loss_acc, float* gpred, float* gaux, float* kld_out,
                          void* stream) {
    MSPL_REQUIRE(pred && aux && target && class_weights && loss_acc, MSPL_ERR_NULL_POINTER, "uw_loss: null pointer");
    MSPL_REQUIRE((gpred == nullptr) == (gaux == nullptr), MSPL_ERR_NULL_POINTER, "uw_loss: gpred and gaux go together");
    MSPL_REQUIRE(N > 0 && C > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "uw_loss: bad shape N=%d C=%d HW=%d", N, C, HW);
    const int64_t total = (int64_t)N * HW;
    // (measured, one atomic per workgroup: 16 x 5 x 256x480 two heads 156 / 105 / 95 / 92 / 112 us at 512 / 1024 / 2048 / 4096 / 7680
    // workgroups; the 4-image micro-batches of the graphed step 32 / 28 / 36 us at 512 / 1024 / 1920)
    static const int max_blocks = MSPL_TUNE_INT("MSPL_LOSS_BLOCKS", 1024);
    const int64_t blocks = std::min<int64_t>(ceil_div64(total, 256), max_blocks);
    hipLaunchKernelGGL(uw_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, aux, target,
                       class_weights, N, C, HW, ce_scale, out_scale / (float)total, loss_acc, gpred, gaux, kld_out);
    MSPL_CHECK_LAUNCH("uw_loss");
    return MSPL_OK;
}

extern "C" int mspl_uw_loss_fwd_bwd(const float* pred, const float* aux, const int64_t* target, const float* class_weights,
                                    int32_t N, int32_t C, int32_t HW, float ce_scale, float* loss_acc, float* gpred,
                                    float* gaux, float* kld_out, void* stream) {
    return uw_loss_launch(pred, aux, target, class_weights, N, C, HW, ce_scale, 1.0f, loss_acc, gpred, gaux, kld_out, stream);
}

extern "C" int mspl_uw_loss_scaled_fwd_bwd(const float* pred, const float* aux, const int64_t* target, const float* class_weights,
                                           int32_t N, int32_t C, int32_t HW, float ce_scale, float out_scale, float* loss_acc,
                                           float* gpred, float* gaux, float* kld_out, void* stream) {
    return uw_loss_launch(pred, aux, target, class_weights, N, C, HW, ce_scale, out_scale, loss_acc, gpred, gaux, kld_out, stream);
}

extern "C" int mspl_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                              float eps, float weight_decay, int32_t step, void* stream) {
    MSPL_REQUIRE(p && g && m && v, MSPL_ERR_NULL_POINTER, "adam_step: null pointer");
    MSPL_REQUIRE(n >= 0 && step >= 1, MSPL_ERR_BAD_SHAPE, "adam_step: n=%lld step=%d", (long long)n, step);
    if (n == 0) return MSPL_OK;
    // in double, as torch.optim.Adam forms them: (float)0.999 is 1.3e-8 too large, which 1.f - beta2 turns into 1.3e-5 of every second
    // moment and powf(beta2, step) into 1.3e-8 * step of the bias correction (tests/optim_shadow.py)
    const float bc1 = (float)(1.0 - pow(beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow(beta2, (double)step));
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr,
                       (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay, bc1, bc2s);
    MSPL_CHECK_LAUNCH("adam_step");
    return MSPL_OK;
}
