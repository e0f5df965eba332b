// NIDLoss (loss_fns/segmentation_loss.py:54-144): normalised information distance between the grey-level histogram of the
// camera image and the (soft-arg-max) label histogram.  This file holds the two heavy steps; the (K x C) entropy arithmetic
// after them is done by the caller on tiny tensors.
//   soft_arg_max (:124-141)        lab = sum_j j * exp((A_j - max A)*500) / (sum exp + 1e-12)
//   get_probabilities (:76-101)    P_c[k,p] = sum_b  sig((g - mu_k + L/2)/bw_c) - sig((g - mu_k - L/2)/bw_c),  g = (r+g+b)/3,
//                                  P_l[c,p] = sum_b  sig((lab - c + 1/2)/bw_l) - sig((lab - c - 1/2)/bw_l)   (rows c < min(C,K):
//                                  the reference fills P_l inside its loop over the K image bins),
//                                  joint = P_c P_l^T / norm, p_c = rowsum(P_c)/norm, p_l = rowsum(P_l)/norm, norm = B*H*W
// Forward: one thread per pixel POSITION p (the batch sum happens before the outer product, as in the reference); per-thread
// columns of P_c / P_l live in LDS, then each wave reduces its share of the K*C products over the workgroup's 256
// positions; per-workgroup partials are summed in double by a second kernel (no float atomics: deterministic).
// Backward (w.r.t. the label logits only; the camera image carries no gradient in the reference's use): same staging,
// G_l[c,p] = sum_k GJ[k,c] P_c[k,p] + Gpl[c], then d lab and the soft-arg-max Jacobian per image.
#include "common.hpp"
#include "nid_parts.hpp"

namespace mspl {

// (the sigmoids, the soft-arg-max and the per-position column arithmetic are in nid_parts.hpp, shared with nid_heads.hip)
__device__ __forceinline__ void stage_columns(const float* __restrict__ cam, const float* __restrict__ lab, const NidG& g, int p,
                                              float* As, float* Ls, bool with_labels) {
    const int t = threadIdx.x;
    for (int k = 0; k < g.K; ++k) As[k * 256 + t] = 0.f;
    if (with_labels)
        for (int c = 0; c < g.Cl; ++c) Ls[c * 256 + t] = 0.f;
    if (p >= g.P) return;
    for (int b = 0; b < g.B; ++b) {
        nid_camera_add(As, t, nid_gray(cam + (size_t)b * 3 * g.P + p, (size_t)g.P), g.K, g.bw_c);
        if (with_labels)
            nid_label_add(Ls, t, soft_arg_max(lab + (size_t)b * g.C * g.P + p, g.C, (size_t)g.P, g.beta, 1e-12f), g.Cl, g.bw_l);
    }
}

// partial: (blocks, K*Cl + K + Cl)
__global__ __launch_bounds__(256) void nid_hist_kernel(const float* __restrict__ cam, const float* __restrict__ lab, NidG g,
                                                       float* __restrict__ partial) {
    extern __shared__ float lds[];
    float* As = lds;
    float* Ls = lds + g.K * 256;
    stage_columns(cam, lab, g, blockIdx.x * 256 + threadIdx.x, As, Ls, true);
    __syncthreads();
    nid_partial_sums(As, Ls, g.K, g.Cl, partial + (size_t)blockIdx.x * (g.K * g.Cl + g.K + g.Cl));
}

// gj: (K, Cl) = dL/d joint, gpl: (Cl) = dL/d p_l, both already divided by norm.  glab: (B, C, P) overwritten.
__global__ __launch_bounds__(256) void nid_bwd_kernel(const float* __restrict__ cam, const float* __restrict__ lab, NidG g,
                                                      const float* __restrict__ gj, const float* __restrict__ gpl,
                                                      float* __restrict__ glab) {
    extern __shared__ float lds[];
    float* As = lds;
    float* Gl = lds + g.K * 256;
    float* Gj = Gl + g.Cl * 256;
    const int t = threadIdx.x, p = blockIdx.x * 256 + t;
    for (int i = t; i < g.K * g.Cl; i += 256) Gj[i] = gj[i];
    stage_columns(cam, lab, g, p, As, Gl, false);
    __syncthreads();
    if (p >= g.P) return;
    nid_label_grad_column(Gl, As, Gj, gpl, t, g.K, g.Cl);
    for (int b = 0; b < g.B; ++b) {
        const float* a = lab + (size_t)b * g.C * g.P + p;
        float* ga = glab + (size_t)b * g.C * g.P + p;
        const NidLab r = nid_dlab(a, g.C, (size_t)g.P, Gl, t, g.Cl, g.beta, g.bw_l);
        for (int j = 0; j < g.C; ++j) ga[(size_t)j * g.P] = nid_dlogit(r, a[(size_t)j * g.P], j, g.beta);
    }
}

static int nid_geom(NidG& g, int B, int C, int H, int W, int K, float bw_c, float bw_l, const char* who) {
    MSPL_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && K > 0, MSPL_ERR_BAD_SHAPE, "%s: bad shape B=%d C=%d %dx%d K=%d", who, B, C, H, W, K);
    MSPL_REQUIRE(K <= NID_MAXB && C <= NID_MAXB, MSPL_ERR_UNSUPPORTED, "%s: at most %d image bins and label bins (got %d, %d)", who,
                 NID_MAXB, K, C);
    MSPL_REQUIRE(bw_c > 0.f && bw_l > 0.f, MSPL_ERR_BAD_SHAPE, "%s: bandwidths must be positive", who);
    MSPL_REQUIRE((size_t)(K + (C < K ? C : K)) * 1024 + (size_t)K * C * 4 <= 65536, MSPL_ERR_UNSUPPORTED,
                 "%s: K=%d image bins x C=%d label bins exceed the 64 KiB staging budget", who, K, C);
    g.B = B; g.C = C; g.K = K; g.Cl = C < K ? C : K; g.P = H * W; g.bw_c = bw_c; g.bw_l = bw_l; g.beta = 500.0f;
    return MSPL_OK;
}

}  // namespace mspl

using namespace mspl;

extern "C" int64_t mspl_nid_workspace_floats(int32_t C, int32_t H, int32_t W, int32_t K) {
    if (C <= 0 || H <= 0 || W <= 0 || K <= 0) return MSPL_ERR_BAD_SHAPE;
    const int Cl = C < K ? C : K;
    return (int64_t)ceil_div(H * W, 256) * (K * Cl + K + Cl);
}

extern "C" int mspl_nid_hist_fwd(const float* camera, const float* label, int32_t B, int32_t C, int32_t H, int32_t W, int32_t K,
                                 float bw_camera, float bw_label, float* ws, float* out, void* stream) {
    MSPL_REQUIRE(camera && label && ws && out, MSPL_ERR_NULL_POINTER, "nid_hist: null pointer");
    NidG g;
    if (int rc = nid_geom(g, B, C, H, W, K, bw_camera, bw_label, "nid_hist")) return rc;
    const int blocks = ceil_div(g.P, 256), E = g.K * g.Cl + g.K + g.Cl;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nid_hist_kernel, dim3((unsigned)blocks), dim3(256), (size_t)(g.K + g.Cl) * 256 * sizeof(float), s, camera, label, g, ws);
    MSPL_CHECK_LAUNCH("nid_hist");
    hipLaunchKernelGGL(nid_reduce_kernel, dim3((unsigned)ceil_div(E, 256)), dim3(256), 0, s, ws, blocks, E, 1.0 / ((double)g.P * B), out);
    MSPL_CHECK_LAUNCH("nid_hist(reduce)");
    return MSPL_OK;
}

extern "C" int mspl_nid_hist_bwd(const float* camera, const float* label, int32_t B, int32_t C, int32_t H, int32_t W, int32_t K,
                                 float bw_camera, float bw_label, const float* gjoint, const float* gpl, float* glabel, void* stream) {
    MSPL_REQUIRE(camera && label && gjoint && gpl && glabel, MSPL_ERR_NULL_POINTER, "nid_hist_bwd: null pointer");
    NidG g;
    if (int rc = nid_geom(g, B, C, H, W, K, bw_camera, bw_label, "nid_hist_bwd")) return rc;
    const size_t lds = ((size_t)(g.K + g.Cl) * 256 + (size_t)g.K * g.Cl) * sizeof(float);
    hipLaunchKernelGGL(nid_bwd_kernel, dim3((unsigned)ceil_div(g.P, 256)), dim3(256), lds, (hipStream_t)stream, camera, label, g, gjoint,
                       gpl, glabel);
    MSPL_CHECK_LAUNCH("nid_hist_bwd");
    return MSPL_OK;
}
