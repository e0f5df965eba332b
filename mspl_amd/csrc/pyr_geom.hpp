// Geometry of the EfficientPyrPool branches, shared by every kernel file of the family (pyrpool.hip, pyrpool_sep.hip,
// pyrpool_stream.hip, pyrpool_train.hip, pyr_prep.hip, pyr_down_bwd.hip): the pooling-window bounds, the separable-stencil view of the
// up-sampled branches, the host-side classification of a branch list, the tap dispatch and the forward launchers' argument bundle.
//
//   t = adaptive_avg_pool2d(dw3x3(bilinear_up(x)))  ==  sum_ky sum_kx w[ky][kx] * A_ky x G_kx^T
// with banded, position-dependent matrices A_k (rows) / G_k (columns): entry (p, q) of A_k multiplies x[p - R + q], R = (T - 1) / 2.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace mspl {

constexpr int PYR_MAXB = 5;

// ATen's adaptive pooling window of output o of O over I inputs: [floor(o * I / O), ceil((o + 1) * I / O)), in 32-bit unsigned
// arithmetic (the launchers bound the sizes).  resample.hip's ada_start / ada_end are the 64-bit form for maps of any size.
__host__ __device__ __forceinline__ int pyr_bin_s(int o, int I, int O) { return (int)(((unsigned)o * (unsigned)I) / (unsigned)O); }
__host__ __device__ __forceinline__ int pyr_bin_e(int o, int I, int O) { return (int)((((unsigned)(o + 1)) * (unsigned)I + O - 1) / (unsigned)O); }

// Stencil coefficients of one output position p (row or column) and one kernel offset k of an up branch with T taps:
// acc[q] multiplies x[p - R + q], R = (T - 1) / 2.  Twin of p2_fill_up_tables' body (pyrpool_sep.hip): the same values, kept apart
// because merging them changes that kernel's register allocation.  A branch of the map's own size (S == I) gives acc[k] = 1: the
// plain 3x3 tap.
template <int T>
__device__ __forceinline__ void p3_coeffs(int p, int k, int I, int S, float sc, float (&acc)[5]) {
    constexpr int R = (T - 1) / 2;
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] = 0.f;
    if (p < 0 || p >= I) return;
    const int us = pyr_bin_s(p, S, I), ue = pyr_bin_e(p, S, I);
    const float inv = 1.0f / (float)(ue - us);
    for (int uu = us; uu < ue; ++uu) {
        const int v = uu + k - 1;
        if (v < 0 || v >= S) continue;          // zero padding of the 3x3 on the up-sampled grid
        int ia, ib;  float w0, w1;
        bilinear_src(sc, v, I, ia, ib, w0, w1);
        const int ta = ia - (p - R), tb = ib - (p - R);
#pragma unroll
        for (int q = 0; q < T; ++q) {
            if (q == ta) acc[q] += w0 * inv;
            if (q == tb) acc[q] += w1 * inv;
        }
    }
}

__device__ __forceinline__ float p3_from_left(float v) {    // value of lane - 1 (0 for lane 0)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float p3_from_right(float v) {   // value of lane + 1 (0 for lane 63)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}

// ---- host side

// Smallest R such that every source of output p lies in [p-R, p+R] (one dimension); large when unsupported.
static inline int stencil_radius(int I, int S) {
    const float sc = bilinear_scale(I, S);
    int R = 0;
    for (int p = 0; p < I; ++p) {
        const int us = (int)(((int64_t)p * S) / I), ue = (int)((((int64_t)p + 1) * S + I - 1) / I);
        for (int v = std::max(us - 1, 0); v <= std::min(ue, S - 1); ++v) {
            int a, b;
            bilinear_src_host(sc, v, I, a, b);
            R = std::max(R, std::max(p - a, b - p));
        }
    }
    return R;
}

// Stencil taps of an up branch of hs x ws on an h x w map: 3 (radius <= 1 in both directions), 5 (radius 2), 0: not a stencil of 5.
static inline int pyr_up_taps(int h, int w, int hs, int ws) {
    const int R = std::max(stencil_radius(h, hs), stencil_radius(w, ws));
    return R > 2 ? 0 : (R <= 1 ? 3 : 5);
}

// What a branch list is, and nothing about which kernel form runs it: every form reads this and applies its own limits.
// The values of the first three kinds are the ones the Pyr*Geom structs carry.
enum { PYR_UP = 0, PYR_SAME = 1, PYR_DOWN = 2, PYR_MIXED = 3 };
struct PyrBranches {
    int nb;                                // as given; nothing below is filled when it is outside 0 .. PYR_MAXB
    int kind[PYR_MAXB];                    // PYR_UP: hs >= h and ws >= w, not both equal; PYR_DOWN: <=; PYR_MIXED: neither, or a size <= 0
    int taps[PYR_MAXB];                    // PYR_UP: pyr_up_taps; else 0
    float sh[PYR_MAXB], sw[PYR_MAXB];      // bilinear scales; up / same: x -> branch grid, down: branch grid -> map; mixed: 0
    int nup, nsame, ndown, nmixed;
    bool standard;                         // strictly [up, up, same, down, down], the up branches larger in BOTH directions
};
static inline PyrBranches pyr_classify(int h, int w, int nb, const int32_t* hs, const int32_t* ws) {
    PyrBranches b;
    memset(&b, 0, sizeof(b));
    b.nb = nb;
    if (nb < 0 || nb > PYR_MAXB) return b;
    bool strict_up[PYR_MAXB] = {false, false, false, false, false};
    for (int i = 0; i < nb; ++i) {
        if (hs[i] <= 0 || ws[i] <= 0) {
            b.kind[i] = PYR_MIXED;  ++b.nmixed;
        } else if (hs[i] == h && ws[i] == w) {
            b.kind[i] = PYR_SAME;  ++b.nsame;
        } else if (hs[i] >= h && ws[i] >= w) {
            b.kind[i] = PYR_UP;  ++b.nup;
            b.taps[i] = pyr_up_taps(h, w, hs[i], ws[i]);
            strict_up[i] = hs[i] > h && ws[i] > w;
        } else if (hs[i] <= h && ws[i] <= w) {
            b.kind[i] = PYR_DOWN;  ++b.ndown;
            b.sh[i] = bilinear_scale(hs[i], h); b.sw[i] = bilinear_scale(ws[i], w);
        } else {
            b.kind[i] = PYR_MIXED;  ++b.nmixed;
        }
        if (b.kind[i] <= PYR_SAME) { b.sh[i] = bilinear_scale(h, hs[i]); b.sw[i] = bilinear_scale(w, ws[i]); }
    }
    b.standard = nb == 5 && strict_up[0] && strict_up[1] && b.kind[2] == PYR_SAME && b.kind[3] == PYR_DOWN && b.kind[4] == PYR_DOWN;
    return b;
}

// LAUNCH(T0, T1, ...) for the run-time tap pair (t0, t1), each 3 or 5: the four instantiations a kernel with two up branches has.
#define MSPL_PYR_TAP_DISPATCH(t0, t1, LAUNCH, ...) do { \
        if ((t0) == 3 && (t1) == 3) LAUNCH(3, 3, ##__VA_ARGS__); \
        else if ((t0) == 3) LAUNCH(3, 5, ##__VA_ARGS__); \
        else if ((t1) == 3) LAUNCH(5, 3, ##__VA_ARGS__); \
        else LAUNCH(5, 5, ##__VA_ARGS__); } while (0)
// One up branch only: the second template argument stays 3 and (3, 5) / (5, 5) are never instantiated.
#define MSPL_PYR_TAP_DISPATCH_1UP(t0, LAUNCH, ...) do { \
        if ((t0) == 3) LAUNCH(3, 3, ##__VA_ARGS__); else LAUNCH(5, 3, ##__VA_ARGS__); } while (0)

// What pyrpool_fused_launch (pyrpool.hip) hands to the forms it tries first.  Each returns MSPL_OK when it launched, 1 when it leaves
// the shape to the next form, < 0 on error.
struct PyrFwdArgs {
    const float* x;
    int N, P, h, w, nb;
    const int32_t* hs; const int32_t* ws;
    const float* const* stage_w;           // per branch (P,1,3,3), up / same branches
    const float* const* down_e;            // per branch (N,P,hs,ws), down branches
    const float* br_scale; const float* br_shift; const float* br_alpha;   // nb*P each (merge_layer.0)
    const float* merge_w;                  // (P, nb, 3, 3)
    Epi e;
    float* out;
    float* zcat;                           // training forward: the branch values before merge_layer.0, or null
    const float* tab;                      // geometry tables of pyrpool_stream_tables_build, or null
    hipStream_t stream;
    PyrBranches br;
};
int pyrpool_stream_try(const PyrFwdArgs& a);        // pyrpool_stream.hip: register-streaming form
int pyrpool_sep_try(const PyrFwdArgs& a);           // pyrpool_sep.hip: LDS-tiled stencil form
int pyrpool_stream_tables_build(int h, int w, int nb, const int32_t* hs, const int32_t* ws, float* tab, int64_t bytes, hipStream_t stream);
int64_t pyrpool_stream_tables_bytes(int h, int w, int nb, const int32_t* hs, const int32_t* ws);
void pyrpool_stream_plan(int N, int P, int h, int w, int nb, const int32_t* hs, const int32_t* ws, int32_t* out);

}  // namespace mspl
