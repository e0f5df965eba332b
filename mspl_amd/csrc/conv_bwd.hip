// Convolution backward for the training steps: the data gradient in gather form (strided convolutions; stride-1 data gradients run
// on the forward kernels with the weights mspl_transpose_weights prepares) and the weight gradient in its forms -- generic, 3x3 with
// few input channels per group (per position, 16-byte strips, four output channels per workgroup, stride-2 strips), 1x1 with 16x16
// LDS tiles or on the matrix cores (conv1x1_wgrad.hip) -- chosen by ONE planner, conv_bwd_weight_plan, which the launcher and
// mspl_conv_bwd_weight_plan both ask.
#include <stdlib.h>

#include <algorithm>

#include "common.hpp"
#include "conv1x1_wgrad.hpp"

namespace mspl {

struct ConvGeom {
    int N, Cin, Cout, G, cin_g, cout_g, H, W, Ho, Wo, K, stride, dil, pad;
};

// ---- data gradient: gx[n,ci,iy,ix] = sum_{co in group, ky, kx} w[co,ci_g,ky,kx] * gy[n,co,oy,ox]
//      with oy*stride = iy + pad - ky*dil (must divide), same for x.
__global__ __launch_bounds__(256) void conv_bwd_data_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                            ConvGeom g, int accumulate, float* __restrict__ gx,
                                                            int64_t total) {
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ix = (int)(idx % g.W);  int64_t t = idx / g.W;
    const int iy = (int)(t % g.H);  t /= g.H;
    const int ci = (int)(t % g.Cin);
    const int n = (int)(t / g.Cin);
    const int grp = ci / g.cin_g, cig = ci - grp * g.cin_g;
    float acc = 0.f;
    for (int ky = 0; ky < g.K; ++ky) {
        const int ty = iy + g.pad - ky * g.dil;
        if (ty < 0 || ty % g.stride) continue;
        const int oy = ty / g.stride;
        if (oy >= g.Ho) continue;
        for (int kx = 0; kx < g.K; ++kx) {
            const int tx = ix + g.pad - kx * g.dil;
            if (tx < 0 || tx % g.stride) continue;
            const int ox = tx / g.stride;
            if (ox >= g.Wo) continue;
            const float* gp = gy + (((size_t)n * g.Cout + (size_t)grp * g.cout_g) * g.Ho + oy) * (size_t)g.Wo + ox;
            const float* wp = w + (((size_t)grp * g.cout_g) * g.cin_g + cig) * (size_t)(g.K * g.K) + ky * g.K + kx;
            for (int co = 0; co < g.cout_g; ++co)
                acc = fmaf(wp[(size_t)co * g.cin_g * g.K * g.K], gp[(size_t)co * g.Ho * g.Wo], acc);
        }
    }
    if (accumulate) gx[idx] += acc; else gx[idx] = acc;
}

// ---- weight gradient, generic: one workgroup per (weight element, pixel chunk); partial sums are combined with
//      float atomics (gw zero-filled by the launcher unless accumulating).
__global__ __launch_bounds__(256) void conv_bwd_weight_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                              ConvGeom g, int chunks, float* __restrict__ gw) {
    int b = blockIdx.x;
    const int chunk = b % chunks;  b /= chunks;
    const int widx = b;
    const int kx = b % g.K;  b /= g.K;
    const int ky = b % g.K;  b /= g.K;
    const int cig = b % g.cin_g;
    const int co = b / g.cin_g;
    const int grp = co / g.cout_g;
    const int ci = grp * g.cin_g + cig;
    const int npix = g.Ho * g.Wo;
    const int64_t total = (int64_t)g.N * npix;
    const int64_t per = (total + chunks - 1) / chunks;
    const int64_t i0 = chunk * per, i1 = min(total, i0 + per);
    float acc = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const int n = (int)(i / npix), p = (int)(i - (int64_t)n * npix);
        const int oy = p / g.Wo, ox = p - oy * g.Wo;
        const int iy = oy * g.stride - g.pad + ky * g.dil, ix = ox * g.stride - g.pad + kx * g.dil;
        if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
        acc = fmaf(gy[((size_t)n * g.Cout + co) * npix + p], x[(((size_t)n * g.Cin + ci) * g.H + iy) * (size_t)g.W + ix], acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&gw[widx], (part[0] + part[1]) + (part[2] + part[3]));
}

// ---- weight gradient of a 3x3 convolution with few input channels per group (CG = cin_g <= 5: depthwise, the
//      stem, the pyramid merge conv; any stride / dilation): one workgroup per (output channel, pixel chunk); a thread
//      walks output pixels (coalesced gy reads, the x taps hit L1/L2) carrying the CG*9 tap sums in registers, so gy
//      is streamed once instead of once per tap.
template <int CG>
__global__ __launch_bounds__(256) void g3x3_bwd_weight_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                              ConvGeom g, int chunks, float* __restrict__ gw) {
    const int chunk = blockIdx.x % chunks, co = blockIdx.x / chunks;
    const int ci0 = (co / g.cout_g) * CG;
    const int npix = g.Ho * g.Wo;
    const int64_t total = (int64_t)g.N * npix;
    const int64_t per = (total + chunks - 1) / chunks;
    const int64_t i0 = chunk * per, i1 = min(total, i0 + per);
    const size_t plane = (size_t)g.H * g.W;
    float acc[CG * 9];
#pragma unroll
    for (int t = 0; t < CG * 9; ++t) acc[t] = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const int n = (int)(i / npix), p = (int)(i - (int64_t)n * npix);
        const int oy = p / g.Wo, ox = p - oy * g.Wo;
        const float gv = gy[((size_t)n * g.Cout + co) * npix + p];
        const float* xp = x + ((size_t)n * g.Cin + ci0) * plane;
        const int by = oy * g.stride - g.pad, bx = ox * g.stride - g.pad;
        int offs[9];
        float msk[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = by + ky * g.dil;
            const bool oky = iy >= 0 && iy < g.H;
            const int iyc = min(max(iy, 0), g.H - 1);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = bx + kx * g.dil;
                offs[ky * 3 + kx] = iyc * g.W + min(max(ix, 0), g.W - 1);
                msk[ky * 3 + kx] = (oky && ix >= 0 && ix < g.W) ? gv : 0.f;
            }
        }
        // request every tap of this position before the first use (hipcc otherwise emits load -> wait -> fma per tap)
        float xv[CG * 9];
#pragma unroll
        for (int ci = 0; ci < CG; ++ci)
#pragma unroll
            for (int t = 0; t < 9; ++t) xv[ci * 9 + t] = xp[ci * plane + offs[t]];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ci = 0; ci < CG; ++ci)
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[ci * 9 + t] = fmaf(msk[t], xv[ci * 9 + t], acc[ci * 9 + t]);
    }
    __shared__ float part[4][CG * 9];
#pragma unroll
    for (int t = 0; t < CG * 9; ++t) {
        const float v = wave_sum_dpp(acc[t]);                  // total in lane 63
        if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < CG * 9)
        atomicAdd(&gw[(size_t)co * CG * 9 + threadIdx.x],
                  (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]));
}

// Strip form of the same for stride 1 / dilation 1 / padding 1 on rows of whole 16-byte strips (the EfficientPWConv expansions, the
// pyramid stages and merge convolutions: every stride-1 3x3 of the training steps): a thread takes FOUR adjacent output positions per
// step -- gy as one 16-byte load, each input row as one 16-byte load + its two neighbours -- so a position's tap costs a quarter of a
// load instruction instead of one: the per-position form is bound by the L1 load path (CG * 9 four-byte loads per position:
// 179 us for the 8-channel-group expansion at 16 x 144x240 whose operands are 141 MB).
template <int CG>
__global__ __launch_bounds__(256) void g3x3_bwd_weight_strip_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                    ConvGeom g, int chunks, float* __restrict__ gw) {
    // The cout_g output channels of a group read the SAME input chunk: their workgroups are issued back to back on ONE XCD (workgroup b
    // goes to XCD b % 8), so the chunk is fetched into that XCD's L2 once instead of cout_g times through the Infinity Cache (137 us for
    // the 8-channel-group expansion: 4.6 TB/s of re-reads).
    const int xcd = blockIdx.x & 7, qq = blockIdx.x >> 3;
    const int cog = qq % g.cout_g, pair = (qq / g.cout_g) * 8 + xcd;          // pair = (group, chunk)
    if (pair >= g.G * chunks) return;
    const int chunk = pair % chunks, co = (pair / chunks) * g.cout_g + cog;
    const int ci0 = (co / g.cout_g) * CG;
    const int XS = g.W >> 2, nstrip = g.H * XS;                     // Ho == H, Wo == W
    const int64_t total = (int64_t)g.N * nstrip;
    const int64_t per = (total + chunks - 1) / chunks;
    const int64_t i0 = chunk * per, i1 = min(total, i0 + per);
    const size_t plane = (size_t)g.H * g.W;
    float acc[CG * 9];
#pragma unroll
    for (int t = 0; t < CG * 9; ++t) acc[t] = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const int n = (int)(i / nstrip), sidx = (int)(i - (int64_t)n * nstrip);
        const int oy = sidx / XS, x0 = (sidx - oy * XS) * 4;
        const float4 g4 = *reinterpret_cast<const float4*>(gy + ((size_t)n * g.Cout + co) * plane + (size_t)oy * g.W + x0);
        const float gvv[4] = {g4.x, g4.y, g4.z, g4.w};
        const float* xp = x + ((size_t)n * g.Cin + ci0) * plane;
        const float ml = x0 > 0 ? 1.f : 0.f, mr = x0 + 4 < g.W ? 1.f : 0.f;
        const int xl = max(x0 - 1, 0), xr = min(x0 + 4, g.W - 1);
        int roff[3];  float rm[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy - 1 + ky;
            rm[ky] = (iy >= 0 && iy < g.H) ? 1.f : 0.f;
            roff[ky] = min(max(iy, 0), g.H - 1) * g.W;
        }
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) {
            // the channel's nine loads first, then the arithmetic
            float4 v[3];  float l[3], r[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float* row = xp + ci * plane + roff[ky];
                v[ky] = *reinterpret_cast<const float4*>(row + x0);
                l[ky] = row[xl];
                r[ky] = row[xr];
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float w6[6] = {l[ky] * (ml * rm[ky]), v[ky].x * rm[ky], v[ky].y * rm[ky], v[ky].z * rm[ky], v[ky].w * rm[ky],
                                     r[ky] * (mr * rm[ky])};
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    float a = acc[ci * 9 + ky * 3 + kx];
#pragma unroll
                    for (int j = 0; j < 4; ++j) a = fmaf(gvv[j], w6[j + kx], a);
                    acc[ci * 9 + ky * 3 + kx] = a;
                }
            }
        }
    }
    __shared__ float part[4][CG * 9];
#pragma unroll
    for (int t = 0; t < CG * 9; ++t) {
        const float v = wave_sum_dpp(acc[t]);                  // total in lane 63
        if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < CG * 9)
        atomicAdd(&gw[(size_t)co * CG * 9 + threadIdx.x],
                  (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]));
}

// The same for COB consecutive output channels of one group per workgroup: a position's CG * 9 taps are loaded once and serve COB
// output channels (the stem's 3 -> 32 stride-2 gradient loaded every tap 32 times: 424 M four-byte loads through L1, 197 us for
// 87 MB of operands).  Per accumulator the positions arrive in the same order as above: same sums.
template <int CG, int COB>
__global__ __launch_bounds__(256, 3) void g3x3_bwd_weight_cob_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                  ConvGeom g, int chunks, float* __restrict__ gw) {
    const int chunk = blockIdx.x % chunks, co0 = (blockIdx.x / chunks) * COB;
    const int ci0 = (co0 / g.cout_g) * CG;
    const int npix = g.Ho * g.Wo;
    const int64_t total = (int64_t)g.N * npix;
    const int64_t per = (total + chunks - 1) / chunks;
    const int64_t i0 = chunk * per, i1 = min(total, i0 + per);
    const size_t plane = (size_t)g.H * g.W;
    float acc[COB][CG * 9];
#pragma unroll
    for (int c = 0; c < COB; ++c)
#pragma unroll
        for (int t = 0; t < CG * 9; ++t) acc[c][t] = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const int n = (int)(i / npix), p = (int)(i - (int64_t)n * npix);
        const int oy = p / g.Wo, ox = p - oy * g.Wo;
        float gv[COB];
#pragma unroll
        for (int c = 0; c < COB; ++c) gv[c] = gy[((size_t)n * g.Cout + co0 + c) * npix + p];
        const float* xp = x + ((size_t)n * g.Cin + ci0) * plane;
        const int by = oy * g.stride - g.pad, bx = ox * g.stride - g.pad;
        int offs[9];
        float msk[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = by + ky * g.dil;
            const bool oky = iy >= 0 && iy < g.H;
            const int iyc = min(max(iy, 0), g.H - 1);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = bx + kx * g.dil;
                offs[ky * 3 + kx] = iyc * g.W + min(max(ix, 0), g.W - 1);
                msk[ky * 3 + kx] = (oky && ix >= 0 && ix < g.W) ? 1.f : 0.f;
            }
        }
        float xv[CG * 9];
#pragma unroll
        for (int ci = 0; ci < CG; ++ci)
#pragma unroll
            for (int t = 0; t < 9; ++t) xv[ci * 9 + t] = xp[ci * plane + offs[t]];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ci = 0; ci < CG; ++ci)
#pragma unroll
            for (int t = 0; t < 9; ++t) xv[ci * 9 + t] *= msk[t];           // zero padding (the address was clamped)
#pragma unroll
        for (int c = 0; c < COB; ++c)
#pragma unroll
            for (int t = 0; t < CG * 9; ++t) acc[c][t] = fmaf(gv[c], xv[t], acc[c][t]);
    }
    __shared__ float part[4][COB * CG * 9];
#pragma unroll
    for (int c = 0; c < COB; ++c)
#pragma unroll
        for (int t = 0; t < CG * 9; ++t) {
            const float v = wave_sum_dpp(acc[c][t]);           // total in lane 63
            if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6][c * CG * 9 + t] = v;
        }
    __syncthreads();
    if (threadIdx.x < COB * CG * 9)
        atomicAdd(&gw[(size_t)co0 * CG * 9 + threadIdx.x],
                  (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]));
}

// Stride 2 / padding 1 on rows of whole 32-byte blocks (the stem, 3 -> 32 at 288x480): four adjacent output positions per thread.
// Their 3x3 windows cover input columns 2*ox0 - 1 .. 2*ox0 + 7 of each input row: two aligned 16-byte loads and the left neighbour
// instead of twelve 4-byte loads at a stride of two floats; COB output channels share them.  (The per-position form ran at two, then
// three waves per SIMD with one exposed load round trip per position: 166 -> 135 us for 96 MB of operands.)
template <int CG, int COB>
__global__ __launch_bounds__(256, 3) void g3x3_bwd_weight_s2_strip_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                          ConvGeom g, int chunks, float* __restrict__ gw) {
    const int cgb = g.cout_g / COB;                               // workgroups per (group, chunk) pair: issued back to back on one XCD
    const int xcd = blockIdx.x & 7, qq = blockIdx.x >> 3;
    const int cog = qq % cgb, pair = (qq / cgb) * 8 + xcd;
    if (pair >= g.G * chunks) return;
    const int chunk = pair % chunks, co0 = (pair / chunks) * g.cout_g + cog * COB;
    const int ci0 = (co0 / g.cout_g) * CG;
    const int XS = g.Wo >> 2, nstrip = g.Ho * XS;
    const int64_t total = (int64_t)g.N * nstrip;
    const int64_t per = (total + chunks - 1) / chunks;
    const int64_t i0 = chunk * per, i1 = min(total, i0 + per);
    const size_t plane = (size_t)g.H * g.W, oplane = (size_t)g.Ho * g.Wo;
    float acc[COB][CG * 9];
#pragma unroll
    for (int c = 0; c < COB; ++c)
#pragma unroll
        for (int t = 0; t < CG * 9; ++t) acc[c][t] = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const int n = (int)(i / nstrip), sidx = (int)(i - (int64_t)n * nstrip);
        const int oy = sidx / XS, ox0 = (sidx - oy * XS) * 4;
        float gv[COB][4];
#pragma unroll
        for (int c = 0; c < COB; ++c) {
            const float4 t4 = *reinterpret_cast<const float4*>(gy + ((size_t)n * g.Cout + co0 + c) * oplane + (size_t)oy * g.Wo + ox0);
            gv[c][0] = t4.x; gv[c][1] = t4.y; gv[c][2] = t4.z; gv[c][3] = t4.w;
        }
        const float* xp = x + ((size_t)n * g.Cin + ci0) * plane + 2 * ox0;
        const float ml = ox0 > 0 ? 1.f : 0.f;
        const int lo = ox0 > 0 ? -1 : 0;
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) {
            float4 a[3], b[3];  float l[3];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = 2 * oy - 1 + ky;                                  // <= H - 1 (H even); -1 at the top
                const float* row = xp + ci * plane + (size_t)max(iy, 0) * g.W;
                a[ky] = *reinterpret_cast<const float4*>(row);
                b[ky] = *reinterpret_cast<const float4*>(row + 4);
                l[ky] = row[lo];
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float rm = (2 * oy - 1 + ky >= 0) ? 1.f : 0.f;
                const float w9[9] = {l[ky] * (ml * rm), a[ky].x * rm, a[ky].y * rm, a[ky].z * rm, a[ky].w * rm,
                                     b[ky].x * rm, b[ky].y * rm, b[ky].z * rm, b[ky].w * rm};
#pragma unroll
                for (int c = 0; c < COB; ++c)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        float v = acc[c][ci * 9 + ky * 3 + kx];
#pragma unroll
                        for (int j = 0; j < 4; ++j) v = fmaf(gv[c][j], w9[2 * j + kx], v);
                        acc[c][ci * 9 + ky * 3 + kx] = v;
                    }
            }
            __builtin_amdgcn_sched_barrier(0);            // one channel's nine loads in flight at a time (all 27 hoisted: 70+ spilled VGPRs)
        }
    }
    __shared__ float part[4][COB * CG * 9];
#pragma unroll
    for (int c = 0; c < COB; ++c)
#pragma unroll
        for (int t = 0; t < CG * 9; ++t) {
            const float v = wave_sum_dpp(acc[c][t]);           // total in lane 63
            if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6][c * CG * 9 + t] = v;
        }
    __syncthreads();
    if (threadIdx.x < COB * CG * 9)
        atomicAdd(&gw[(size_t)co0 * CG * 9 + threadIdx.x],
                  (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]));
}

// ---- weight gradient of a grouped 1x1 convolution: gw[co, ci] = sum_{n,p} gy[n,co,p] * x[n,ci,p].
//      A workgroup owns a 16 x 16 tile of one group's (co, ci) pairs and a chunk of pixels; both operand tiles
//      (16 rows x 256 pixels) are staged in LDS with coalesced loads, each thread reduces one (co, ci) pair over the
//      staged pixels (row reads are LDS broadcasts / conflict-free), partial sums combined with float atomics.
__global__ __launch_bounds__(256) void conv1x1_bwd_weight_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                 ConvGeom g, int chunks, int tiles_m, int tiles_k,
                                                                 float* __restrict__ gw) {
    __shared__ float A[16][260];      // gy rows (co), 256 pixels (+4 pad: rows land on different banks)
    __shared__ float B[16][260];      // x rows (ci)
    int b = blockIdx.x;
    const int chunk = b % chunks;  b /= chunks;
    const int tk = b % tiles_k;  b /= tiles_k;
    const int tm = b % tiles_m;
    const int grp = b / tiles_m;
    const int M = g.cout_g, K = g.cin_g, HW = g.Ho * g.Wo;
    const int m0 = tm * 16, k0 = tk * 16;
    const int tid = threadIdx.x;
    const int tmi = tid >> 4, tki = tid & 15;      // this thread's (co, ci) pair inside the tile
    const int64_t total = (int64_t)g.N * HW;
    const int64_t per = ((total + chunks - 1) / chunks + 255) / 256 * 256;
    const int64_t i0 = chunk * per, i1 = min(total, i0 + per);
    float acc = 0.f;
    for (int64_t base = i0; base < i1; base += 256) {
        // stage: thread t loads pixel base+t of 16 rows of each operand (coalesced along pixels).  Row and pixel
        // indices are clamped so all 32 loads are unconditional and issue back to back; masked to zero afterwards.
        const int64_t i = base + tid;
        const bool ok = i < i1;
        const int64_t ic = ok ? i : i1 - 1;
        const int n = (int)(ic / HW), p = (int)(ic - (int64_t)n * HW);
        const float* ga = gy + ((size_t)n * g.Cout + (size_t)grp * M) * HW + p;
        const float* xb = x + ((size_t)n * g.Cin + (size_t)grp * K) * HW + p;
        float ra[16], rb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ra[r] = ga[(size_t)min(m0 + r, M - 1) * HW];
            rb[r] = xb[(size_t)min(k0 + r, K - 1) * HW];
        }
        __builtin_amdgcn_sched_barrier(0);          // keep the 32 loads in flight together (no per-load wait)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            A[r][tid] = (ok && m0 + r < M) ? ra[r] : 0.f;
            B[r][tid] = (ok && k0 + r < K) ? rb[r] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < 256; q += 4) {
            const float4 a4 = *reinterpret_cast<const float4*>(&A[tmi][q]);
            const float4 b4 = *reinterpret_cast<const float4*>(&B[tki][q]);
            acc = fmaf(a4.x, b4.x, acc); acc = fmaf(a4.y, b4.y, acc); acc = fmaf(a4.z, b4.z, acc); acc = fmaf(a4.w, b4.w, acc);
        }
        __syncthreads();
    }
    if (m0 + tmi < M && k0 + tki < K)
        atomicAdd(&gw[((size_t)grp * M + m0 + tmi) * K + k0 + tki], acc);
}

static int conv_geom(const char* who, int N, int Cin, int Cout, int groups, int H, int W, int K, int stride, int dil, ConvGeom& g) {
    MSPL_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && groups > 0 && H > 0 && W > 0, MSPL_ERR_BAD_SHAPE, "%s: bad shape", who);
    MSPL_REQUIRE(Cin % groups == 0 && Cout % groups == 0, MSPL_ERR_BAD_SHAPE, "%s: channels not divisible by groups", who);
    MSPL_REQUIRE((K == 1 || K == 3) && (stride == 1 || stride == 2) && dil >= 1, MSPL_ERR_UNSUPPORTED,
                 "%s: kernel %d stride %d dilation %d", who, K, stride, dil);
    g.N = N; g.Cin = Cin; g.Cout = Cout; g.G = groups; g.cin_g = Cin / groups; g.cout_g = Cout / groups;
    g.H = H; g.W = W; g.K = K; g.stride = stride; g.dil = dil; g.pad = dil * (K - 1) / 2;
    g.Ho = (H + 2 * g.pad - dil * (K - 1) - 1) / stride + 1;
    g.Wo = (W + 2 * g.pad - dil * (K - 1) - 1) / stride + 1;
    return MSPL_OK;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_conv_bwd_data(const float* gy, const float* w, int32_t N, int32_t Cin, int32_t Cout, int32_t groups,
                                  int32_t H, int32_t W, int32_t K, int32_t stride, int32_t dilation, int32_t accumulate,
                                  float* gx, void* stream) {
    MSPL_REQUIRE(gy && w && gx, MSPL_ERR_NULL_POINTER, "conv_bwd_data: null pointer");
    ConvGeom g;
    if (int rc = conv_geom("conv_bwd_data", N, Cin, Cout, groups, H, W, K, stride, dilation, g)) return rc;
    const int64_t total = (int64_t)N * Cin * H * W;
    MSPL_REQUIRE(ceil_div64(total, 256) < (1ll << 31), MSPL_ERR_BAD_SHAPE, "conv_bwd_data: grid too large");
    hipLaunchKernelGGL(conv_bwd_data_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream, gy, w, g,
                       accumulate, gx, total);
    MSPL_CHECK_LAUNCH("conv_bwd_data");
    return MSPL_OK;
}

// Which kernel form mspl_conv_bwd_weight launches for a shape and into how many parts it splits the reduction: the ONE place where
// that is decided (the launcher below switches on the result; mspl_conv_bwd_weight_plan hands it to callers and tests).
// aligned16: gy and x are both 16-byte aligned (the strip forms read them as float4).
struct WgradPlan {
    int form;            // mspl_wgrad_form_t
    int parts;           // chunks of the N*Ho*Wo range (matrix-core 1x1: waves per tile)
    int ngroups;         // matrix-core 1x1: 64-pixel groups of the reduction range; else 0
};

static WgradPlan conv_bwd_weight_plan(const ConvGeom& g, bool aligned16) {
    WgradPlan p;
    p.ngroups = 0;
    const int K = g.K, Cout = g.Cout;
    const int64_t total = (int64_t)g.N * g.Ho * g.Wo;
    static const int s2_strip = MSPL_TUNE_INT("MSPL_G3X3_WGRAD_S2STRIP", 1);
    static const int strip_form = MSPL_TUNE_INT("MSPL_G3X3_WGRAD_STRIP", 1);
    int chunks = 1;
    if (K == 1) {
        static const bool no_mfma = MSPL_TUNE_INT("MSPL_WGRAD_LDS", 0) != 0;      // A/B aid: force the 16x16 LDS kernel
        if (!no_mfma && conv1x1_wgrad_mfma_plan(g.N, g.G, g.cout_g, g.cin_g, g.Ho * g.Wo, &p.parts, &p.ngroups) == 0) {
            p.form = MSPL_WGRAD_1X1_MFMA;
            return p;
        }
        p.ngroups = 0;
        // (the 16x16 tile is zero padded for groups with fewer channels, e.g. the 3-channel image reinforcement)
        const int tiles_m = ceil_div(g.cout_g, 16), tiles_k = ceil_div(g.cin_g, 16);
        const int64_t base = (int64_t)g.G * tiles_m * tiles_k;
        static const int minpx = MSPL_TUNE_INT("MSPL_WGRAD16_MINPX", 256);
        while (base * chunks < 2048 && total / (chunks * 2) >= minpx) chunks *= 2;
        p.form = MSPL_WGRAD_1X1_LDS;
    } else if (s2_strip && K == 3 && g.cin_g == 3 && g.cout_g % 4 == 0 && Cout >= 16 && g.stride == 2 && g.dil == 1 && g.pad == 1 &&
               (g.W & 7) == 0 && (g.H & 1) == 0 && aligned16) {
        const int64_t strips = total / 4;
        while ((int64_t)(Cout / 2) * chunks < 2048 && strips / (chunks * 2) >= 512) chunks *= 2;
        p.form = MSPL_WGRAD_STEM_S2_STRIP;
    } else if (K == 3 && g.cin_g == 3 && g.cout_g % 4 == 0 && Cout >= 16) {       // the stem: four output channels per workgroup share the taps
        while ((int64_t)(Cout / 4) * chunks < 2048 && total / (chunks * 2) >= 2048) chunks *= 2;
        p.form = MSPL_WGRAD_STEM_COB4;
    } else if (strip_form && K == 3 && (g.cin_g <= 5 || g.cin_g == 8) && g.stride == 1 && g.dil == 1 && g.pad == 1 && (g.W & 3) == 0 &&
               aligned16) {
        const int64_t strips = total / 4;
        while ((int64_t)Cout * chunks < 2048 && strips / (chunks * 2) >= 1024) chunks *= 2;
        p.form = MSPL_WGRAD_STRIP;
    } else if (K == 3 && (g.cin_g <= 5 || g.cin_g == 8)) {
        while ((int64_t)Cout * chunks < 4096 && total / (chunks * 2) >= 2048) chunks *= 2;
        p.form = MSPL_WGRAD_G3X3;
    } else {
        const int64_t nw = (int64_t)Cout * g.cin_g * K * K;
        while (nw * chunks < 2048 && total / (chunks * 2) >= 4096) chunks *= 2;
        p.form = MSPL_WGRAD_GENERIC;
    }
    p.parts = chunks;
    return p;
}

extern "C" int mspl_conv_bwd_weight_plan(int32_t N, int32_t Cin, int32_t Cout, int32_t groups, int32_t H, int32_t W, int32_t K,
                                         int32_t stride, int32_t dilation, int32_t aligned16, int32_t* form, int32_t* parts,
                                         int32_t* ngroups) {
    MSPL_REQUIRE(form && parts, MSPL_ERR_NULL_POINTER, "conv_bwd_weight_plan: null pointer");
    ConvGeom g;
    if (int rc = conv_geom("conv_bwd_weight_plan", N, Cin, Cout, groups, H, W, K, stride, dilation, g)) return rc;
    const WgradPlan p = conv_bwd_weight_plan(g, aligned16 != 0);
    *form = p.form;
    *parts = p.parts;
    if (ngroups) *ngroups = p.ngroups;
    return MSPL_OK;
}

// KERNEL<CG> for the channels per group the planner gives the 3x3 forms: 1..5 or 8.  For mspl_conv_bwd_weight only: the launch
// arguments (s, gy, x, g, chunks, gw) are its locals, and the macro is undefined after it.
#define MSPL_G3X3_CG_DISPATCH(KERNEL, cg, grid) do { \
        switch (cg) { \
            case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, s, gy, x, g, chunks, gw); break; \
            case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, s, gy, x, g, chunks, gw); break; \
            case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, s, gy, x, g, chunks, gw); break; \
            case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, s, gy, x, g, chunks, gw); break; \
            case 5: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(256), 0, s, gy, x, g, chunks, gw); break; \
            default: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(256), 0, s, gy, x, g, chunks, gw); break; \
        } } while (0)

extern "C" int mspl_conv_bwd_weight(const float* gy, const float* x, int32_t N, int32_t Cin, int32_t Cout, int32_t groups,
                                    int32_t H, int32_t W, int32_t K, int32_t stride, int32_t dilation, int32_t accumulate,
                                    float* gw, void* stream) {
    MSPL_REQUIRE(gy && x && gw, MSPL_ERR_NULL_POINTER, "conv_bwd_weight: null pointer");
    ConvGeom g;
    if (int rc = conv_geom("conv_bwd_weight", N, Cin, Cout, groups, H, W, K, stride, dilation, g)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nw = (int64_t)Cout * g.cin_g * K * K;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(gw, 0, (size_t)nw * sizeof(float), s);      // async memset node: graph-capturable
        MSPL_REQUIRE(e == hipSuccess, MSPL_ERR_HIP, "conv_bwd_weight: memset failed: %s", hipGetErrorString(e));
    }
    const WgradPlan plan = conv_bwd_weight_plan(g, ((((uintptr_t)gy) | ((uintptr_t)x)) & 15) == 0);
    const int chunks = plan.parts;
    switch (plan.form) {
    case MSPL_WGRAD_1X1_MFMA: {
        const int rc = conv1x1_wgrad_mfma_try(gy, x, N, groups, g.cout_g, g.cin_g, g.Ho * g.Wo, gw, s);
        MSPL_REQUIRE(rc == 0, MSPL_ERR_UNSUPPORTED, "conv_bwd_weight: the matrix-core 1x1 form refused a shape its plan accepted");
        MSPL_CHECK_LAUNCH("conv_bwd_weight(1x1, mfma)");
        return MSPL_OK;
    }
    case MSPL_WGRAD_1X1_LDS: {
        const int tiles_m = ceil_div(g.cout_g, 16), tiles_k = ceil_div(g.cin_g, 16);
        const int64_t blocks = (int64_t)groups * tiles_m * tiles_k * chunks;
        MSPL_REQUIRE(blocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "conv_bwd_weight: grid too large");
        hipLaunchKernelGGL(conv1x1_bwd_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, s, gy, x, g, chunks, tiles_m, tiles_k, gw);
        MSPL_CHECK_LAUNCH("conv_bwd_weight(1x1)");
        return MSPL_OK;
    }
    case MSPL_WGRAD_STEM_S2_STRIP: {
        const int64_t pairs8 = ((int64_t)g.G * chunks + 7) & ~7ll;
        hipLaunchKernelGGL((g3x3_bwd_weight_s2_strip_kernel<3, 2>), dim3((unsigned)(pairs8 * (g.cout_g / 2))), dim3(256), 0, s, gy, x, g, chunks, gw);
        MSPL_CHECK_LAUNCH("conv_bwd_weight(3x3 stride 2, few input channels, strips)");
        return MSPL_OK;
    }
    case MSPL_WGRAD_STEM_COB4:
        hipLaunchKernelGGL((g3x3_bwd_weight_cob_kernel<3, 4>), dim3((unsigned)(Cout / 4 * chunks)), dim3(256), 0, s, gy, x, g, chunks, gw);
        MSPL_CHECK_LAUNCH("conv_bwd_weight(3x3, few input channels, 4 output channels per workgroup)");
        return MSPL_OK;
    case MSPL_WGRAD_STRIP: {
        const int64_t pairs8 = ((int64_t)g.G * chunks + 7) & ~7ll;                 // (group, chunk) pairs, padded to whole rounds of the 8 XCDs
        const dim3 grid((unsigned)(pairs8 * g.cout_g));
        MSPL_G3X3_CG_DISPATCH(g3x3_bwd_weight_strip_kernel, g.cin_g, grid);
        MSPL_CHECK_LAUNCH("conv_bwd_weight(3x3, few input channels, strips)");
        return MSPL_OK;
    }
    case MSPL_WGRAD_G3X3: {
        const dim3 grid((unsigned)(Cout * chunks));
        MSPL_G3X3_CG_DISPATCH(g3x3_bwd_weight_kernel, g.cin_g, grid);
        MSPL_CHECK_LAUNCH("conv_bwd_weight(3x3, few input channels)");
        return MSPL_OK;
    }
    default: break;
    }
    const int64_t blocks = nw * chunks;
    MSPL_REQUIRE(blocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "conv_bwd_weight: grid too large");
    hipLaunchKernelGGL(conv_bwd_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, s, gy, x, g, chunks, gw);
    MSPL_CHECK_LAUNCH("conv_bwd_weight");
    return MSPL_OK;
}
#undef MSPL_G3X3_CG_DISPATCH

// Weight gradients of several grouped 1x1 convolutions, ACCUMULATED into gw[i] (parameter gradient buffers), in as few launches as
// the problems allow: runs of problems that fit the matrix-core kernel share one launch (csrc/conv1x1_wgrad.hip), the others go
// through mspl_conv_bwd_weight one by one.
extern "C" int mspl_conv1x1_wgrad_batch(const float* const* gy, const float* const* x, float* const* gw, const float* const* rowscale,
                                        const int32_t* N, const int32_t* Cin, const int32_t* Cout, const int32_t* groups, const int32_t* HW,
                                        int32_t nprob, void* stream) {
    MSPL_REQUIRE(gy && x && gw && N && Cin && Cout && groups && HW, MSPL_ERR_NULL_POINTER, "conv1x1_wgrad_batch: null pointer");
    MSPL_REQUIRE(nprob >= 0 && nprob <= 4096, MSPL_ERR_BAD_SHAPE, "conv1x1_wgrad_batch: %d problems", nprob);
    hipStream_t s = (hipStream_t)stream;
    int G[16], M[16], K[16], P[16], NN[16];
    int at = 0;
    while (at < nprob) {
        int cnt = 0;
        for (; cnt < 16 && at + cnt < nprob; ++cnt) {
            const int i = at + cnt;
            MSPL_REQUIRE(gy[i] && x[i] && gw[i], MSPL_ERR_NULL_POINTER, "conv1x1_wgrad_batch: problem %d has a null pointer", i);
            MSPL_REQUIRE(N[i] > 0 && Cin[i] > 0 && Cout[i] > 0 && groups[i] > 0 && HW[i] > 0 && Cin[i] % groups[i] == 0 &&
                         Cout[i] % groups[i] == 0, MSPL_ERR_BAD_SHAPE, "conv1x1_wgrad_batch: problem %d: N=%d Cin=%d Cout=%d groups=%d HW=%d",
                         i, N[i], Cin[i], Cout[i], groups[i], HW[i]);
            NN[cnt] = N[i]; G[cnt] = groups[i]; M[cnt] = Cout[i] / groups[i]; K[cnt] = Cin[i] / groups[i]; P[cnt] = HW[i];
        }
        const int done = conv1x1_wgrad_mfma_batch(gy + at, x + at, gw + at, rowscale ? rowscale + at : nullptr, NN, G, M, K, P, cnt, s);
        if (done > 0) {
            MSPL_CHECK_LAUNCH("conv1x1_wgrad_batch");
            at += done;
        } else {                 // the first problem of the run is not for the matrix-core kernel
            MSPL_REQUIRE(!(rowscale && rowscale[at]), MSPL_ERR_UNSUPPORTED, "conv1x1_wgrad_batch: problem %d: rowscale needs the matrix-core kernel "
                         "(>= 8 channels per group, HW %% 4 == 0)", at);
            if (int rc = mspl_conv_bwd_weight(gy[at], x[at], N[at], Cin[at], Cout[at], groups[at], 1, HW[at], 1, 1, 1, 1, gw[at], stream)) return rc;
            ++at;
        }
    }
    return MSPL_OK;
}

// Transposed (and, for 3x3, spatially flipped) copies of many convolution weights in ONE launch: the weights of the data-gradient
// convolutions of a training step (autograd.ConvFn.backward runs the data gradient of a stride-1 convolution on the forward
// kernels).  Per weight this was a permute copy (+ a flip) of a few KB issued from ATen inside the backward chain: 81 + 33
// launches of the ~1500 of a step.  seg: per weight {src, dst} pointers and {groups, cin_g, cout_g, k}; blk: per block its
// segment and the index of its first element inside it.
namespace mspl {
struct WtSeg { const float* src; float* dst; int32_t G, cin_g, cout_g, k; int32_t numel, pad; };

__global__ __launch_bounds__(256) void transpose_weights_kernel(const WtSeg* __restrict__ seg, const int2* __restrict__ blk) {
    const int2 b = blk[blockIdx.x];
    const WtSeg sg = seg[b.x];
    const int i = b.y + threadIdx.x;                   // destination index: (((g * cin_g + ci) * cout_g + co) * k + ky) * k + kx
    if (i >= sg.numel) return;
    const int kk = sg.k * sg.k;
    const int t = i / kk, r = i - t * kk;
    const int co = t % sg.cout_g, t2 = t / sg.cout_g;
    const int ci = t2 % sg.cin_g, g = t2 / sg.cin_g;
    const int rs = kk - 1 - r;                          // flip both spatial axes (identity for k = 1)
    sg.dst[i] = sg.src[(((size_t)g * sg.cout_g + co) * sg.cin_g + ci) * kk + rs];
}
}  // namespace mspl

extern "C" int mspl_transpose_weights(const void* seg_table, const void* block_table, int32_t nblocks, void* stream) {
    MSPL_REQUIRE(seg_table && block_table, MSPL_ERR_NULL_POINTER, "transpose_weights: null pointer");
    MSPL_REQUIRE(nblocks >= 0, MSPL_ERR_BAD_SHAPE, "transpose_weights: nblocks=%d", nblocks);
    if (nblocks == 0) return MSPL_OK;
    hipLaunchKernelGGL(mspl::transpose_weights_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream,
                       (const mspl::WtSeg*)seg_table, (const int2*)block_table);
    MSPL_CHECK_LAUNCH("transpose_weights");
    return MSPL_OK;
}
