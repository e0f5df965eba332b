// The per-pixel arithmetic of NIDLoss (loss_fns/segmentation_loss.py:54-144) shared by its kernels: nid.hip (label logits at
// label resolution) and nid_heads.hip (a low-resolution head, interpolated inside the kernel).  Both files call these helpers and
// nothing else for the sigmoids, the soft-arg-max and the per-position columns, so a pixel's `lab` value, its column entries and
// its gradient are the same floats in both forms; only the order in which positions are summed differs.
//   soft_arg_max (:124-141)        lab = sum_j j * exp((A_j - max A)*500) / (sum exp + 1e-12)
//   get_probabilities (:76-101)    P_c[k,p] = sum_b  sig((g - mu_k + L/2)/bw_c) - sig((g - mu_k - L/2)/bw_c),  g = (r+g+b)/3,
//                                  P_l[c,p] = sum_b  sig((lab - c + 1/2)/bw_l) - sig((lab - c - 1/2)/bw_l)   (rows c < min(C,K))
// Columns live in LDS as [row][256], one position per thread (thread t owns element row * 256 + t).
#pragma once
#include "common.hpp"

namespace mspl {

constexpr int NID_MAXB = 32;      // image bins and label bins are both limited to 32 (the scripts use 16 / 32 and <= 21)
constexpr int NID_POS = 256;      // positions per workgroup: the row stride of the LDS columns

__device__ __forceinline__ float sigm(float u) { return 1.0f / (1.0f + expf(-u)); }

struct NidG {
    int B, C, K, Cl, P;           // Cl = min(C, K): label bins that are ever filled
    float bw_c, bw_l, beta;
};

__device__ __forceinline__ float soft_arg_max(const float* __restrict__ a, int C, size_t stride, float beta, float eps) {
    float m = a[0];
    for (int j = 1; j < C; ++j) m = fmaxf(m, a[j * stride]);
    float s = 0.f, t = 0.f;
    for (int j = 0; j < C; ++j) {
        const float e = expf((a[j * stride] - m) * beta);
        s += e;
        t += (e * (float)j);
    }
    return t / (s + eps);
}

// grey level of one image at one position (cp: its red value; planes P apart)
__device__ __forceinline__ float nid_gray(const float* __restrict__ cp, size_t P) { return ((cp[0] + cp[P]) + cp[2 * P]) / 3.0f; }

// As[k][t] += one image's camera term, k < K
__device__ __forceinline__ void nid_camera_add(float* As, int t, float gray, int K, float bw_c) {
    const float Lc = 1.0f / (float)K;
    for (int k = 0; k < K; ++k) {
        const float mu = Lc * ((float)k + 0.5f);
        As[k * NID_POS + t] += sigm((gray - mu + Lc / 2) / bw_c) - sigm((gray - mu - Lc / 2) / bw_c);
    }
}

// Ls[c][t] += one image's label term at soft-arg-max value v, c < Cl
__device__ __forceinline__ void nid_label_add(float* Ls, int t, float v, int Cl, float bw_l) {
    for (int c = 0; c < Cl; ++c)
        Ls[c * NID_POS + t] += sigm((v - (float)c + 0.5f) / bw_l) - sigm((v - (float)c - 0.5f) / bw_l);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// One workgroup's share of joint | p_c | p_l from its columns (after a barrier): each wave reduces its share of the E = K*Cl + K + Cl
// sums over the 256 positions.  out: E floats.
__device__ __forceinline__ void nid_partial_sums(const float* As, const float* Ls, int K, int Cl, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int E = K * Cl + K + Cl;
    for (int q = wave; q < E; q += 4) {
        float s = 0.f;
        if (q < K * Cl) {
            const float* a = As + (q / Cl) * NID_POS;
            const float* l = Ls + (q % Cl) * NID_POS;
#pragma unroll
            for (int j = 0; j < 4; ++j) s = fmaf(a[lane + 64 * j], l[lane + 64 * j], s);
        } else {
            const float* a = q < K * Cl + K ? As + (q - K * Cl) * NID_POS : Ls + (q - K * Cl - K) * NID_POS;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += a[lane + 64 * j];
        }
        s = wave_sum(s);
        if (lane == 0) out[q] = s;
    }
}

// partial (blocks, E) -> out[e] = (sum over the blocks in order, in double) * inv_norm: no float atomics, two runs are bit-identical
static __global__ __launch_bounds__(256) void nid_reduce_kernel(const float* __restrict__ partial, int blocks, int E, double inv_norm,
                                                                float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += (double)partial[(size_t)b * E + e];
    out[e] = (float)(s * inv_norm);
}

// Gl[c][t] = dL/dP_l[c,p] = sum_k GJ[k,c] P_c[k,p] + Gpl[c], from the position's camera column As[.][t] (Gj: the (K, Cl) matrix in LDS)
__device__ __forceinline__ void nid_label_grad_column(float* Gl, const float* As, const float* Gj, const float* __restrict__ gpl,
                                                      int t, int K, int Cl) {
    for (int c = 0; c < Cl; ++c) {
        float s = gpl[c];
        for (int k = 0; k < K; ++k) s = fmaf(Gj[k * Cl + c], As[k * NID_POS + t], s);
        Gl[c * NID_POS + t] = s;
    }
}

// One image's soft-arg-max at a position, and dL/d lab there.  a: its C logits, `stride` apart.
struct NidLab { float m, S, v, dv; };

__device__ __forceinline__ NidLab nid_dlab(const float* __restrict__ a, int C, size_t stride, const float* Gl, int t, int Cl,
                                           float beta, float bw_l) {
    NidLab r;
    r.m = a[0];
    for (int j = 1; j < C; ++j) r.m = fmaxf(r.m, a[j * stride]);
    float s = 0.f, tt = 0.f;
    for (int j = 0; j < C; ++j) {
        const float e = expf((a[j * stride] - r.m) * beta);
        s += e;
        tt += e * (float)j;
    }
    r.S = s + 1e-12f;
    r.v = tt / r.S;
    r.dv = 0.f;
    for (int c = 0; c < Cl; ++c) {
        const float s1 = sigm((r.v - (float)c + 0.5f) / bw_l), s2 = sigm((r.v - (float)c - 0.5f) / bw_l);
        r.dv = fmaf(Gl[c * NID_POS + t], (s1 * (1.f - s1) - s2 * (1.f - s2)) / bw_l, r.dv);
    }
    return r;
}

// dL/d logit j of that image at that position (the soft-arg-max Jacobian)
__device__ __forceinline__ float nid_dlogit(const NidLab& r, float aj, int j, float beta) {
    const float e = expf((aj - r.m) * beta);
    return r.dv * beta * (e / r.S) * ((float)j - r.v);
}

}  // namespace mspl
