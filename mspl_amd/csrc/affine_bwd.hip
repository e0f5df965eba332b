// Backward of the pointwise layer tails: the affine (folded or batch-statistics BatchNorm) + PReLU backward with its per-channel
// sums, the EESP block's suffix sums over the four branch gradients (plain, and fused with br_after_cat's BatchNorm + PReLU), and
// the DownSampler tail y = PReLU(cat[a, b] + reinf), forward and backward.
#include <stdlib.h>

#include <algorithm>

#include "common.hpp"

namespace mspl {

// Batch-statistics BatchNorm (the supervised loop): what follows the channel sums of the affine backward -- d gamma, d beta and the
// coefficients of gz = p * z + q (mspl_bn_batch_stats_bwd_coeffs) -- done by the workgroup that adds a channel's last partial ("last
// block done": atomic adds -> their acknowledgement -> counter), which also hands the two sums and the counter back zeroed (persistent workspace).
struct BnTail {
    unsigned* cnt;            // null: no tail (gscale / gshift are the caller's accumulators)
    unsigned per_channel;     // workgroups per channel
    const float* gamma;  const float* mean;  const float* invstd;
    float inv_m;  int accumulate;
    float* ggamma;  float* gbeta;  float* pc;  float* qc;
};

// ---- affine + PReLU backward.  Forward: z = (c + pre) * scale + shift + res ; y = z > 0 ? z : alpha * z.
// Outputs gz (optional) and gc = gz * scale; per-channel sums into gscale / gshift / galpha (atomics; zeroed by caller).
__global__ __launch_bounds__(256) void affine_prelu_bwd_kernel(const float* __restrict__ c, const float* __restrict__ pre,
                                                               const float* __restrict__ res, const float* __restrict__ gy,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const float* __restrict__ alpha, int N, int C, int HW, int parts,
                                                               float* __restrict__ gz_out, float* __restrict__ gc_out,
                                                               float* __restrict__ gscale, float* __restrict__ gshift,
                                                               float* __restrict__ galpha, const float* __restrict__ bn_mean,
                                                               const float* __restrict__ bn_inv, BnTail tl) {
    // A workgroup owns one of `parts` contiguous ranges of a channel's N * HW elements (the N planes taken as one sequence): the
    // number of same-address atomics per channel is `parts`, whatever N is.  (One workgroup per (image, channel, chunk) made it
    // N * chunks: at 16 x 16 x 144x240 the 256 atomic chains per channel cost 55 of the kernel's 81 us.)
    const int ch = blockIdx.x / parts, rng = blockIdx.x - ch * parts;
    const float sc = scale ? scale[ch] : 1.f, sh = shift ? shift[ch] : 0.f;
    const bool act = alpha != nullptr;
    const float al = act ? alpha[ch] : 1.f;
    float s_scale = 0.f, s_shift = 0.f, s_alpha = 0.f;
    auto one = [&](float cv, float pv, float rv, float g, float& gz, float& gcv) {
        const float u = cv + pv;
        const float z = fmaf(u, sc, sh) + rv;             // the forward epilogue's expression (epi_apply: fmaf, then + residual): same PReLU branch
        gz = (!act || z > 0.f) ? g : al * g;
        if (act && z <= 0.f) s_alpha += g * z;
        s_scale += gz * u;
        s_shift += gz;
        gcv = gz * sc;
    };
    const bool vec = (HW & 3) == 0;
    const int L = vec ? (HW >> 2) : HW;                    // units (quads or elements) per plane
    const long long total = (long long)N * L;
    const long long per = (total + parts - 1) / parts;
    const long long u0 = (long long)rng * per, u1 = min(total, u0 + per);
    const int step_n = 256 / L, step_q = 256 - step_n * L;
    long long u = u0 + threadIdx.x;
    int n = (int)(u / L), q = (int)(u - (long long)n * L);
    auto advance = [&]() { u += 256; q += step_q; n += step_n; if (q >= L) { q -= L; ++n; } };
    if (vec) {                                 // 16-byte operands, four independent quads per operand in flight per iteration
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        constexpr int UQ = 4;
        while (u < u1) {
            size_t o[UQ];  bool h[UQ];
#pragma unroll
            for (int i = 0; i < UQ; ++i) {
                h[i] = u < u1;
                o[i] = h[i] ? (((size_t)n * C + ch) * (size_t)HW) + 4 * (size_t)q : o[0];
                advance();
            }
            float4 cv[UQ], gv[UQ], pv[UQ], rv[UQ];
#pragma unroll
            for (int i = 0; i < UQ; ++i) {
                cv[i] = *reinterpret_cast<const float4*>(c + o[i]);
                gv[i] = *reinterpret_cast<const float4*>(gy + o[i]);
                pv[i] = pre ? *reinterpret_cast<const float4*>(pre + o[i]) : zero;
                rv[i] = res ? *reinterpret_cast<const float4*>(res + o[i]) : zero;
            }
#pragma unroll
            for (int i = 0; i < UQ; ++i) {
                if (!h[i]) continue;
                float4 gz, gc;
                one(cv[i].x, pv[i].x, rv[i].x, gv[i].x, gz.x, gc.x); one(cv[i].y, pv[i].y, rv[i].y, gv[i].y, gz.y, gc.y);
                one(cv[i].z, pv[i].z, rv[i].z, gv[i].z, gz.z, gc.z); one(cv[i].w, pv[i].w, rv[i].w, gv[i].w, gz.w, gc.w);
                if (gz_out) *reinterpret_cast<float4*>(gz_out + o[i]) = gz;
                if (gc_out) *reinterpret_cast<float4*>(gc_out + o[i]) = gc;
            }
        }
    } else {
        while (u < u1) {
            const size_t o = (((size_t)n * C + ch) * (size_t)HW) + (size_t)q;
            advance();
            float gz, gc;
            one(c[o], pre ? pre[o] : 0.f, res ? res[o] : 0.f, gy[o], gz, gc);
            if (gz_out) gz_out[o] = gz;
            if (gc_out) gc_out[o] = gc;
        }
    }
    float v[3] = {s_scale, s_shift, s_alpha};
    __shared__ float part[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = wave_sum_dpp(v[k]);                            // total in lane 63
        if ((threadIdx.x & 63) == 63) part[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t_scale = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        const float t_shift = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
        // frozen BatchNorm folded into (scale, shift) = (gamma*inv, beta - mean*gamma*inv): the map from (dscale, dshift) to
        // (dgamma, dbeta) is linear, so every workgroup's partial goes straight to the parameters' gradient buffers
        if (gscale) atomicAdd(&gscale[ch], bn_inv ? (t_scale - bn_mean[ch] * t_shift) * bn_inv[ch] : t_scale);
        if (gshift) atomicAdd(&gshift[ch], t_shift);
        if (galpha && act) atomicAdd(&galpha[ch], (part[2][0] + part[2][1]) + (part[2][2] + part[2][3]));
        if (tl.cnt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // (atomics acknowledged before the counter: see bn_stats_fused_kernel)
            if (atomicAdd(tl.cnt + ch, 1u) == tl.per_channel - 1) {
                const float dsc = __uint_as_float(atomicExch(reinterpret_cast<unsigned*>(gscale + ch), 0u));      // read and clear
                const float dsh = __uint_as_float(atomicExch(reinterpret_cast<unsigned*>(gshift + ch), 0u));
                tl.cnt[ch] = 0u;
                const float is = tl.invstd[ch], mu = tl.mean[ch];
                const float t = dsc + (-mu) * dsh;
                tl.ggamma[ch] = tl.accumulate ? tl.ggamma[ch] + t * is : t * is;
                tl.gbeta[ch] = tl.accumulate ? tl.gbeta[ch] + dsh : dsh;
                const float p = ((tl.gamma[ch] * t) * (is * is * is)) * (-tl.inv_m);
                tl.pc[ch] = p;
                tl.qc[ch] = (dsh * sc) * (-tl.inv_m) - p * mu;
            }
        }
    }
}

// ---- suffix sum over the 4 branch blocks of an (N, 4n, HW) gradient: out_k = sum_{j >= k} g_j  (HFF backward).
//      Output is branch-major (4, N, n, HW) so that every branch is a contiguous (N, n, HW) tensor.
__global__ __launch_bounds__(256) void hff_suffix_kernel(const float* __restrict__ g, int n, int HW, float* __restrict__ out,
                                                         int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;     // over N * n * HW
    if (idx >= total) return;
    const int64_t plane = (int64_t)n * HW;
    const int64_t img = idx / plane, r = idx - img * plane;
    const float* gp = g + img * 4 * plane + r;
    const float g3 = gp[3 * plane], g2 = gp[2 * plane] + g3, g1 = gp[plane] + g2, g0 = gp[0] + g1;
    out[idx] = g0; out[total + idx] = g1; out[2 * total + idx] = g2; out[3 * total + idx] = g3;
}

// ---- br_after_cat's BatchNorm + PReLU backward and the suffix sum in one pass (the EESP block's backward between conv_1x1_exp and
//      the four depthwise branches, nn_layers/eesp.py:76-80): z (N,4n,HW) = the raw concatenation K2 produced, gy = dL/d(PReLU(BN(z))).
//      gc = gy * (u > 0 ? 1 : alpha) * scale; out_k = sum_{m >= k} gc_m, branch-major (4,N,n,HW); per-channel sums -> d gamma / d beta /
//      d alpha (frozen BatchNorm transform as in affine_prelu_bwd_kernel).  One workgroup per (image, j, chunk): the four channels
//      k*n + j of a pixel are needed together.
__global__ __launch_bounds__(256) void hff_bn_prelu_suffix_kernel(const float* __restrict__ z, const float* __restrict__ gy,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const float* __restrict__ alpha, const float* __restrict__ bn_mean,
                                                                  const float* __restrict__ bn_inv, int n, int HW, int chunks,
                                                                  int64_t total, float* __restrict__ out, float* __restrict__ gscale,
                                                                  float* __restrict__ gshift, float* __restrict__ galpha,
                                                                  const float* __restrict__ stat_p, const float* __restrict__ stat_q) {
    // stat_p / stat_q (4n each, or null): br_after_cat in train(): the statistics path p * z + q joins the direct gradient before the
    // suffix sum (mspl_hff_bn_stat_suffix_bwd; the channel sums were taken by mspl_bn_train_prelu_bwd, gscale / gshift / galpha null)
    const int tix = (int)threadIdx.x, tstep = 256;
    int b = (int)blockIdx.x;
    const int chunk = b % chunks;  b /= chunks;
    const int j = b % n;
    const int img = b / n;
    float sc[4], sh[4], al[4], s_sc[4], s_sh[4], s_al[4];
    const bool act = alpha != nullptr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ch = k * n + j;
        sc[k] = scale ? scale[ch] : 1.f;  sh[k] = shift ? shift[ch] : 0.f;  al[k] = act ? alpha[ch] : 1.f;
        s_sc[k] = s_sh[k] = s_al[k] = 0.f;
    }
    const bool stat = stat_p != nullptr;
    float pk[4] = {0.f, 0.f, 0.f, 0.f}, qk[4] = {0.f, 0.f, 0.f, 0.f};
    if (stat) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { pk[k] = stat_p[k * n + j];  qk[k] = stat_q[k * n + j]; }
    }
    const size_t in0 = ((size_t)img * 4 * n + j) * (size_t)HW, kin = (size_t)n * HW;
    const size_t out0 = ((size_t)img * n + j) * (size_t)HW;
    auto one = [&](int k, float zv, float g) {
        const float u = fmaf(zv, sc[k], sh[k]);              // K2's own epilogue expression: same PReLU branch
        const bool pos = !act || u > 0.f;
        const float gz = pos ? g : al[k] * g;
        if (!pos) s_al[k] += g * u;
        s_sc[k] += gz * zv;
        s_sh[k] += gz;
        return stat ? fmaf(zv, pk[k], qk[k]) + gz * sc[k] : gz * sc[k];
    };
    if ((HW & 3) == 0) {
        const int q4 = HW >> 2, per = (q4 + chunks - 1) / chunks;
        const int q0 = chunk * per, q1 = min(q4, q0 + per);
        for (int q = q0 + tix; q < q1; q += tstep) {
            float4 zv[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                zv[k] = reinterpret_cast<const float4*>(z + in0 + k * kin)[q];
                gv[k] = reinterpret_cast<const float4*>(gy + in0 + k * kin)[q];
            }
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                acc.x += one(k, zv[k].x, gv[k].x);  acc.y += one(k, zv[k].y, gv[k].y);
                acc.z += one(k, zv[k].z, gv[k].z);  acc.w += one(k, zv[k].w, gv[k].w);
                reinterpret_cast<float4*>(out + (size_t)k * total + out0)[q] = acc;
            }
        }
    } else {
        const int per = (HW + chunks - 1) / chunks;
        const int p0 = chunk * per, p1 = min(HW, p0 + per);
        for (int p = p0 + tix; p < p1; p += tstep) {
            float acc = 0.f;
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                acc += one(k, z[in0 + k * kin + p], gy[in0 + k * kin + p]);
                out[(size_t)k * total + out0 + p] = acc;
            }
        }
    }
    __shared__ float part[12][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v[3] = {s_sc[k], s_sh[k], s_al[k]};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            v[t] = wave_sum_dpp(v[t]);                        // total in lane 63
            if ((threadIdx.x & 63) == 63) part[k * 3 + t][threadIdx.x >> 6] = v[t];
        }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x, ch = k * n + j;
        auto tot = [&](int i) { return (part[i][0] + part[i][1]) + (part[i][2] + part[i][3]); };
        const float t_sc = tot(k * 3), t_sh = tot(k * 3 + 1);
        if (gscale) atomicAdd(&gscale[ch], bn_inv ? (t_sc - bn_mean[ch] * t_sh) * bn_inv[ch] : t_sc);
        if (gshift) atomicAdd(&gshift[ch], t_sh);
        if (galpha && act) atomicAdd(&galpha[ch], tot(k * 3 + 2));
    }
}

}  // namespace mspl

using namespace mspl;

static int affine_prelu_bwd_launch(const float* c, const float* pre_add, const float* residual, const float* gy,
                                   const float* scale, const float* shift, const float* alpha, int32_t N, int32_t C,
                                   int32_t HW, float* gz, float* gc, float* gscale, float* gshift, float* galpha,
                                   const float* bn_mean, const float* bn_inv, void* stream, BnTail tl = BnTail()) {
    MSPL_REQUIRE(c && gy, MSPL_ERR_NULL_POINTER, "affine_prelu_bwd: null pointer");
    MSPL_REQUIRE(N > 0 && C > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "affine_prelu_bwd: bad shape N=%d C=%d HW=%d", N, C, HW);
    // ~MSPL_AFF_BLOCKS workgroups, at least ~2 units per thread, and as few same-address atomic chains per channel as that allows.
    // 384 (1.5 per CU; four 16-byte loads per operand in flight per thread): inside the training steps, where two micro-batch lanes
    // run side by side, the leaner grid is the faster one (same box, alternating: 768 / 512 / 384 / 256 -> uest step 5.73 / 5.68 /
    // 5.665 / 5.67 ms, supervised 8.73 / 8.68 / 8.65 / 8.68 ms; rounds 2-4 ran 768, tuned on the kernel alone)
    static const int target = MSPL_TUNE_INT("MSPL_AFF_BLOCKS", 384);
    const int64_t units = (int64_t)N * ((HW & 3) == 0 ? HW / 4 : HW);
    int64_t parts = ceil_div64(target, C);
    if (parts > units / 512) parts = units / 512;
    if (parts < 1) parts = 1;
    const int64_t blocks = (int64_t)C * parts;
    MSPL_REQUIRE(blocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "affine_prelu_bwd: grid too large");
    tl.per_channel = (unsigned)parts;
    hipLaunchKernelGGL(affine_prelu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, c, pre_add, residual, gy,
                       scale, shift, alpha, N, C, HW, (int)parts, gz, gc, gscale, gshift, galpha, bn_mean, bn_inv, tl);
    MSPL_CHECK_LAUNCH("affine_prelu_bwd");
    return MSPL_OK;
}

extern "C" int mspl_affine_prelu_bwd(const float* c, const float* pre_add, const float* residual, const float* gy,
                                     const float* scale, const float* shift, const float* alpha, int32_t N, int32_t C,
                                     int32_t HW, float* gz, float* gc, float* gscale, float* gshift, float* galpha,
                                     void* stream) {
    return affine_prelu_bwd_launch(c, pre_add, residual, gy, scale, shift, alpha, N, C, HW, gz, gc, gscale, gshift, galpha, nullptr,
                                   nullptr, stream);
}

extern "C" int mspl_bn_train_prelu_bwd(const float* z, const float* residual, const float* gy, const float* scale, const float* shift,
                                       const float* alpha, const float* gamma, const float* mean, const float* invstd, int32_t N, int32_t C,
                                       int32_t HW, float* gres, float* gc, void* ws_zeroed, int32_t accumulate, float* ggamma, float* gbeta,
                                       float* galpha, float* p, float* q, void* stream) {
    MSPL_REQUIRE(scale && shift && gamma && mean && invstd && ws_zeroed && ggamma && gbeta && p && q, MSPL_ERR_NULL_POINTER,
                 "bn_train_prelu_bwd: null pointer");
    MSPL_REQUIRE(((uintptr_t)ws_zeroed & 7) == 0, MSPL_ERR_BAD_SHAPE, "bn_train_prelu_bwd: workspace must be 8-byte aligned");
    // the backward's part of the BatchNorm's persistent workspace (mspl_bn_fused_workspace_bytes): behind the forward's 2C doubles + C counters
    float* sums = reinterpret_cast<float*>(static_cast<char*>(ws_zeroed) + (size_t)C * 20 + ((8 - ((size_t)C * 20) % 8) % 8));
    BnTail tl = BnTail();
    tl.cnt = reinterpret_cast<unsigned*>(sums + 2 * (size_t)C);
    tl.gamma = gamma; tl.mean = mean; tl.invstd = invstd;
    tl.inv_m = (float)(1.0 / ((double)N * (double)HW)); tl.accumulate = accumulate;
    tl.ggamma = ggamma; tl.gbeta = gbeta; tl.pc = p; tl.qc = q;
    return affine_prelu_bwd_launch(z, nullptr, residual, gy, scale, shift, alpha, N, C, HW, gres, gc, sums, sums + C, galpha, nullptr, nullptr,
                                   stream, tl);
}

extern "C" int mspl_bn_prelu_bwd(const float* c, const float* pre_add, const float* residual, const float* gy, const float* scale,
                                 const float* shift, const float* alpha, const float* bn_mean, const float* bn_inv, int32_t N,
                                 int32_t C, int32_t HW, float* gz, float* gc, float* ggamma, float* gbeta, float* galpha,
                                 void* stream) {
    MSPL_REQUIRE(scale && shift && bn_mean && bn_inv, MSPL_ERR_NULL_POINTER, "bn_prelu_bwd: null pointer");
    return affine_prelu_bwd_launch(c, pre_add, residual, gy, scale, shift, alpha, N, C, HW, gz, gc, ggamma, gbeta, galpha, bn_mean,
                                   bn_inv, stream);
}

extern "C" int mspl_hff_suffix_sum(const float* g, int32_t N, int32_t n, int32_t HW, float* out, void* stream) {
    MSPL_REQUIRE(g && out, MSPL_ERR_NULL_POINTER, "hff_suffix_sum: null pointer");
    MSPL_REQUIRE(N > 0 && n > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "hff_suffix_sum: bad shape");
    const int64_t total = (int64_t)N * n * HW;
    hipLaunchKernelGGL(hff_suffix_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream, g, n, HW, out, total);
    MSPL_CHECK_LAUNCH("hff_suffix_sum");
    return MSPL_OK;
}

extern "C" int mspl_hff_bn_prelu_suffix_bwd(const float* z, const float* gy, const float* scale, const float* shift, const float* alpha,
                                            const float* bn_mean, const float* bn_inv, int32_t N, int32_t n, int32_t HW, float* out,
                                            float* gscale, float* gshift, float* galpha, void* stream) {
    MSPL_REQUIRE(z && gy && out, MSPL_ERR_NULL_POINTER, "hff_bn_prelu_suffix_bwd: null pointer");
    MSPL_REQUIRE((bn_mean == nullptr) == (bn_inv == nullptr), MSPL_ERR_NULL_POINTER, "hff_bn_prelu_suffix_bwd: mean / inv must come together");
    MSPL_REQUIRE(N > 0 && n > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "hff_bn_prelu_suffix_bwd: bad shape");
    const int64_t total = (int64_t)N * n * HW;
    int chunks = 1;
    while ((int64_t)N * n * chunks < 2048 && HW / (chunks * 2) >= 1024) chunks *= 2;
    const int64_t blocks = (int64_t)N * n * chunks;
    MSPL_REQUIRE(blocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "hff_bn_prelu_suffix_bwd: grid too large");
    hipLaunchKernelGGL(hff_bn_prelu_suffix_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, gy, scale, shift, alpha,
                       bn_mean, bn_inv, n, HW, chunks, total, out, gscale, gshift, galpha, (const float*)nullptr, (const float*)nullptr);
    MSPL_CHECK_LAUNCH("hff_bn_prelu_suffix_bwd");
    return MSPL_OK;
}

extern "C" int mspl_hff_bn_stat_suffix_bwd(const float* z, const float* gy, const float* scale, const float* shift, const float* alpha,
                                           const float* stat_p, const float* stat_q, int32_t N, int32_t n, int32_t HW, float* out,
                                           void* stream) {
    MSPL_REQUIRE(z && gy && out && scale && shift && stat_p && stat_q, MSPL_ERR_NULL_POINTER, "hff_bn_stat_suffix_bwd: null pointer");
    MSPL_REQUIRE(N > 0 && n > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "hff_bn_stat_suffix_bwd: bad shape");
    const int64_t total = (int64_t)N * n * HW;
    int chunks = 1;
    while ((int64_t)N * n * chunks < 2048 && HW / (chunks * 2) >= 1024) chunks *= 2;
    const int64_t blocks = (int64_t)N * n * chunks;
    MSPL_REQUIRE(blocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "hff_bn_stat_suffix_bwd: grid too large");
    hipLaunchKernelGGL(hff_bn_prelu_suffix_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, gy, scale, shift, alpha,
                       (const float*)nullptr, (const float*)nullptr, n, HW, chunks, total, out, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr, stat_p, stat_q);
    MSPL_CHECK_LAUNCH("hff_bn_stat_suffix_bwd");
    return MSPL_OK;
}

// ---- DownSampler tail (nn_layers/eesp.py:131-144): y = PReLU(cat[a, b] + reinf) without the concatenation.  a (N,nin,HW): the
// pooled input, b (N,C-nin,HW): the strided EESP branch, reinf (N,C,HW) or null.  Forward: one pass reading the two sources where
// torch.cat + add + PReLU made three; backward: dL/da, dL/db land in two CONTIGUOUS tensors (the slices of one gradient that
// autograd's CatBackward hands out had to be copied before our kernels could take them) and d alpha is reduced on the way.
__global__ __launch_bounds__(256) void down_tail_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ r, const float* __restrict__ alpha, int nin, int C,
                                                            int HW4, float* __restrict__ y) {
    const int plane = blockIdx.z * gridDim.y + blockIdx.y;              // n * C + c
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int n = plane / C, c = plane - n * C;
    if (q >= HW4) return;
    const float4* src = reinterpret_cast<const float4*>(c < nin ? a + ((size_t)n * nin + c) * (size_t)HW4 * 4
                                                                : b + ((size_t)n * (C - nin) + (c - nin)) * (size_t)HW4 * 4);
    float4 v = src[q];
    if (r) {
        const float4 t = reinterpret_cast<const float4*>(r + (size_t)plane * HW4 * 4)[q];
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    const float al = alpha[c];
    v.x = v.x > 0.f ? v.x : al * v.x; v.y = v.y > 0.f ? v.y : al * v.y;
    v.z = v.z > 0.f ? v.z : al * v.z; v.w = v.w > 0.f ? v.w : al * v.w;
    reinterpret_cast<float4*>(y + (size_t)plane * HW4 * 4)[q] = v;
}

__global__ __launch_bounds__(256) void down_tail_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ r, const float* __restrict__ gy,
                                                            const float* __restrict__ alpha, int nin, int C, int HW4, int chunks,
                                                            float* __restrict__ ga, float* __restrict__ gb, float* __restrict__ gr,
                                                            float* __restrict__ galpha) {
    int bid = blockIdx.x;
    const int chunk = bid % chunks;  bid /= chunks;
    const int c = bid % C, n = bid / C;
    const size_t soff = (c < nin ? ((size_t)n * nin + c) : ((size_t)n * (C - nin) + (c - nin))) * (size_t)HW4;
    const float4* src = reinterpret_cast<const float4*>(c < nin ? a : b) + soff;
    float4* gsrc = reinterpret_cast<float4*>(c < nin ? ga : gb) + soff;
    const size_t poff = ((size_t)n * C + c) * (size_t)HW4;
    const float4* r4 = r ? reinterpret_cast<const float4*>(r) + poff : nullptr;
    const float4* g4 = reinterpret_cast<const float4*>(gy) + poff;
    float4* gr4 = gr ? reinterpret_cast<float4*>(gr) + poff : nullptr;
    const float al = alpha[c];
    const int per = (HW4 + chunks - 1) / chunks, q0 = chunk * per, q1 = min(HW4, q0 + per);
    float s_alpha = 0.f;
    auto one = [&](float z, float g) { if (z > 0.f) return g; s_alpha += g * z; return al * g; };
    for (int q = q0 + threadIdx.x; q < q1; q += 256) {
        float4 z = src[q];
        if (r4) { const float4 t = r4[q]; z.x += t.x; z.y += t.y; z.z += t.z; z.w += t.w; }
        const float4 g = g4[q];
        float4 gz;
        gz.x = one(z.x, g.x); gz.y = one(z.y, g.y); gz.z = one(z.z, g.z); gz.w = one(z.w, g.w);
        gsrc[q] = gz;
        if (gr4) gr4[q] = gz;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s_alpha += __shfl_down(s_alpha, o, 64);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s_alpha;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(galpha + c, (part[0] + part[1]) + (part[2] + part[3]));
}

extern "C" int mspl_down_tail_fwd(const float* a, const float* b, const float* reinf, const float* alpha, int32_t N, int32_t nin,
                                  int32_t C, int32_t HW, float* y, void* stream) {
    MSPL_REQUIRE(a && b && alpha && y, MSPL_ERR_NULL_POINTER, "down_tail_fwd: null pointer");
    MSPL_REQUIRE(N > 0 && nin > 0 && nin < C && HW > 0, MSPL_ERR_BAD_SHAPE, "down_tail_fwd: bad shape N=%d nin=%d C=%d HW=%d", N, nin, C, HW);
    MSPL_REQUIRE((HW & 3) == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)reinf | (uintptr_t)y)) & 15) == 0, MSPL_ERR_UNSUPPORTED,
                 "down_tail_fwd: planes must be a multiple of 4 pixels and 16-byte aligned");
    const int64_t planes = (int64_t)N * C;
    MSPL_REQUIRE(planes < 65535ll * 65535ll, MSPL_ERR_BAD_SHAPE, "down_tail_fwd: too many planes");
    MSPL_REQUIRE(planes % 65535 == 0 || planes < 65535, MSPL_ERR_UNSUPPORTED, "down_tail_fwd: plane count %lld", (long long)planes);
    const dim3 grid = plane_grid(ceil_div(HW / 4, 256), planes);
    hipLaunchKernelGGL(down_tail_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, b, reinf, alpha, nin, C, HW / 4, y);
    MSPL_CHECK_LAUNCH("down_tail_fwd");
    return MSPL_OK;
}

extern "C" int mspl_down_tail_bwd(const float* a, const float* b, const float* reinf, const float* gy, const float* alpha, int32_t N,
                                  int32_t nin, int32_t C, int32_t HW, float* ga, float* gb, float* greinf, float* galpha, void* stream) {
    MSPL_REQUIRE(a && b && gy && alpha && ga && gb && galpha, MSPL_ERR_NULL_POINTER, "down_tail_bwd: null pointer");
    MSPL_REQUIRE((reinf == nullptr) == (greinf == nullptr), MSPL_ERR_NULL_POINTER, "down_tail_bwd: reinf and greinf go together");
    MSPL_REQUIRE(N > 0 && nin > 0 && nin < C && HW > 0, MSPL_ERR_BAD_SHAPE, "down_tail_bwd: bad shape N=%d nin=%d C=%d HW=%d", N, nin, C, HW);
    MSPL_REQUIRE((HW & 3) == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)reinf | (uintptr_t)gy | (uintptr_t)ga | (uintptr_t)gb |
                                     (uintptr_t)greinf)) & 15) == 0, MSPL_ERR_UNSUPPORTED,
                 "down_tail_bwd: planes must be a multiple of 4 pixels and 16-byte aligned");
    int chunks = 1;
    while ((int64_t)N * C * chunks < 4096 && HW / 4 / (chunks * 2) >= 512) chunks *= 2;
    const int64_t blocks = (int64_t)N * C * chunks;
    MSPL_REQUIRE(blocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "down_tail_bwd: grid too large");
    hipLaunchKernelGGL(down_tail_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, reinf, gy, alpha, nin, C, HW / 4,
                       chunks, ga, gb, greinf, galpha);
    MSPL_CHECK_LAUNCH("down_tail_bwd");
    return MSPL_OK;
}
