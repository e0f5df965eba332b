// Backward of the resampling ops, all in gather form (no atomics, gx overwritten): the 3x3 / stride-2 average pool (per pixel and
// 16-byte strips), the align_corners bilinear resize (per pixel, separable LDS tiles, a wave per pixel, a workgroup per input row)
// and the adaptive average pool.  The form of the first two is decided by one planner each, which the launcher and the plan query
// (mspl_avgpool3x3s2_bwd_plan, mspl_bilinear_bwd_plan) both ask.
#include <stdlib.h>

#include <algorithm>

#include "common.hpp"

namespace mspl {

// Geometry of one launch: gy is (N, C, Ho, Wo), gx (N, C, Hi, Wi); sh / sw are the bilinear scales (0 for a single output row / column)
struct RsG { int N, C, Hi, Wi, Ho, Wo; float sh, sw; unsigned mHi, mWi, mHo, mWo; };   // m*: ceil(2^32/d) division magics

// n / d for n * d < 2^32 with m = ceil(2^32 / d) (d == 1: m overflows to 0, handled)
__device__ __forceinline__ unsigned udiv_magic(unsigned n, unsigned d, unsigned m) { return d == 1 ? n : __umulhi(n, m); }

// Even planes, rows of whole 16-byte strips: a thread turns a 2 x 5 patch of the output gradient (two float4 + their right neighbours)
// into the 2 x 8 block of the input gradient under it -- even rows / columns are covered by one output, odd ones by two (the gather of
// the kernel below, written out: same order of additions) -- with 16-byte loads and stores instead of one pixel per thread
// (56 -> 15 us at 32 x 128x240).
__global__ __launch_bounds__(256) void avgpool3x3s2_bwd_vec_kernel(const float* __restrict__ gy, RsG g, int XS, float* __restrict__ gx) {
    const int t = blockIdx.z * gridDim.y + blockIdx.y;      // plane n*C + c
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.N * g.C || s >= g.Ho * XS) return;
    const int k = s / XS, m0 = (s - k * XS) * 4;             // output row, first output column
    const float* r0 = gy + (size_t)t * g.Ho * g.Wo + (size_t)k * g.Wo + m0;
    const bool hasr = m0 + 4 < g.Wo, hasd = k + 1 < g.Ho;
    const float4 a4 = *reinterpret_cast<const float4*>(r0);
    const float ar = hasr ? r0[4] : 0.f;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);  float br = 0.f;
    if (hasd) { b4 = *reinterpret_cast<const float4*>(r0 + g.Wo);  br = hasr ? r0[g.Wo + 4] : 0.f; }
    const float a[5] = {a4.x, a4.y, a4.z, a4.w, ar}, b[5] = {b4.x, b4.y, b4.z, b4.w, br};
    float e[8], o[8];                                        // input rows 2k (even) and 2k+1 (odd), columns 2 m0 .. 2 m0 + 7
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // the gather visits (oy, ox) in ascending order starting from 0: 0 + g[k][m] (+ g[k][m+1]) (+ g[k+1][m]) (+ g[k+1][m+1])
        e[2 * j] = (0.f + a[j]) * (1.0f / 9.0f);
        o[2 * j] = hasd ? ((0.f + a[j]) + b[j]) * (1.0f / 9.0f) : (0.f + a[j]) * (1.0f / 9.0f);
        const bool hr = j < 3 || hasr;                       // the last odd column of a row has no right neighbour output
        e[2 * j + 1] = hr ? ((0.f + a[j]) + a[j + 1]) * (1.0f / 9.0f) : (0.f + a[j]) * (1.0f / 9.0f);
        o[2 * j + 1] = hasd ? (hr ? ((((0.f + a[j]) + a[j + 1]) + b[j]) + b[j + 1]) * (1.0f / 9.0f) : ((0.f + a[j]) + b[j]) * (1.0f / 9.0f))
                            : (hr ? ((0.f + a[j]) + a[j + 1]) * (1.0f / 9.0f) : (0.f + a[j]) * (1.0f / 9.0f));
    }
    float* d = gx + (size_t)t * g.Hi * g.Wi + (size_t)(2 * k) * g.Wi + 2 * m0;
    *reinterpret_cast<float4*>(d) = make_float4(e[0], e[1], e[2], e[3]);
    *reinterpret_cast<float4*>(d + 4) = make_float4(e[4], e[5], e[6], e[7]);
    *reinterpret_cast<float4*>(d + g.Wi) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(d + g.Wi + 4) = make_float4(o[4], o[5], o[6], o[7]);
}

__global__ __launch_bounds__(256) void avgpool3x3s2_bwd_kernel(const float* __restrict__ gy, RsG g, float* __restrict__ gx, int64_t total) {
    const int t = blockIdx.z * gridDim.y + blockIdx.y;      // plane n*C + c
    const int pi = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.N * g.C || pi >= g.Hi * g.Wi) return;
    const int iy = (int)udiv_magic(pi, g.Wi, g.mWi), ix = pi - iy * g.Wi;
    const int64_t idx = (int64_t)t * g.Hi * g.Wi + pi;
    const float* gp = gy + (size_t)t * g.Ho * g.Wo;
    float acc = 0.f;                                         // gather: outputs whose 3x3/s2/p1 window covers (iy, ix)
    for (int oy = max(0, iy / 2); oy <= min(g.Ho - 1, (iy + 1) / 2); ++oy) {
        if (2 * oy - 1 > iy || 2 * oy + 1 < iy) continue;
        for (int ox = max(0, ix / 2); ox <= min(g.Wo - 1, (ix + 1) / 2); ++ox) {
            if (2 * ox - 1 > ix || 2 * ox + 1 < ix) continue;
            acc += gp[(size_t)oy * g.Wo + ox];
        }
    }
    gx[idx] = acc * (1.0f / 9.0f);
}

// Gather form (deterministic, no atomics): one thread per INPUT pixel, loops over the output rows/columns whose
// two bilinear sources include it.  Output y uses source rows floor(y*sh) and +1, so the candidates for input row iy
// are y in [ceil((iy-1)/sh), floor((iy+1)/sh)] (clamped); same along x.
template <int MAXC>
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const float* __restrict__ gy, RsG g, float* __restrict__ gx, int64_t total) {
    const int t = blockIdx.z * gridDim.y + blockIdx.y;      // plane n*C + c
    const int pi = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.N * g.C || pi >= g.Hi * g.Wi) return;
    const int iy = pi / g.Wi, ix = pi - iy * g.Wi;
    const int64_t idx = (int64_t)t * g.Hi * g.Wi + pi;
    const float* gp = gy + (size_t)t * g.Ho * g.Wo;
    int ylo = 0, yhi = g.Ho - 1, xlo = 0, xhi = g.Wo - 1;
    // outputs whose source floor(o*s) is i-1 or i lie in [ceil((i-1)/s), ceil((i+1)/s) - 1]; one extra on each side covers the
    // float rounding of o*s in the forward (the weights below are evaluated exactly as the forward does, so extras get 0)
    if (g.sh > 0.f) { ylo = max(0, (int)ceilf((float)(iy - 1) / g.sh) - 1); yhi = min(g.Ho - 1, (int)floorf((float)(iy + 1) / g.sh) + 1); }
    if (g.sw > 0.f) { xlo = max(0, (int)ceilf((float)(ix - 1) / g.sw) - 1); xhi = min(g.Wo - 1, (int)floorf((float)(ix + 1) / g.sw) + 1); }
    float acc = 0.f;
    const int nx = xhi - xlo + 1;
    if (nx <= MAXC) {
        // the column weights do not depend on the row: evaluate them once (x2 / x4 up-sampling: 7 / 11 candidates, at most 4
        // of them non-zero), then each candidate row costs one weight evaluation and the loads of the non-zero columns only
        float wxs[MAXC];
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            wxs[j] = 0.f;
            if (j < nx) {
                int x0, x1;  float wx0, wx1;
                bilinear_src(g.sw, xlo + j, g.Wi, x0, x1, wx0, wx1);
                wxs[j] = (x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f);
            }
        }
        for (int oy = ylo; oy <= yhi; ++oy) {
            int y0, y1;  float wy0, wy1;
            bilinear_src(g.sh, oy, g.Hi, y0, y1, wy0, wy1);
            const float wy = (y0 == iy ? wy0 : 0.f) + (y1 == iy ? wy1 : 0.f);
            if (wy == 0.f) continue;
            const float* row = gp + (size_t)oy * g.Wo + xlo;
            float rv[MAXC];
#pragma unroll
            for (int j = 0; j < MAXC; ++j) rv[j] = row[min(j, nx - 1)];      // clamped and unconditional (wxs is 0 past nx):
            __builtin_amdgcn_sched_barrier(0);                                // the row's reads leave as one batch
            float rowacc = 0.f;
#pragma unroll
            for (int j = 0; j < MAXC; ++j) rowacc = fmaf(wxs[j], rv[j], rowacc);
            acc = fmaf(wy, rowacc, acc);
        }
        gx[idx] = acc;
        return;
    }
    for (int oy = ylo; oy <= yhi; ++oy) {
        int y0, y1;  float wy0, wy1;
        bilinear_src(g.sh, oy, g.Hi, y0, y1, wy0, wy1);
        const float wy = (y0 == iy ? wy0 : 0.f) + (y1 == iy ? wy1 : 0.f);
        if (wy == 0.f) continue;
        float rowacc = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            int x0, x1;  float wx0, wx1;
            bilinear_src(g.sw, ox, g.Wi, x0, x1, wx0, wx1);
            const float wx = (x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f);
            if (wx != 0.f) rowacc = fmaf(wx, gp[(size_t)oy * g.Wo + ox], rowacc);
        }
        acc = fmaf(wy, rowacc, acc);
    }
    gx[idx] = acc;
}

// Tiled separable form of the same gather (x2 / x4 up-sampling: the decoder merges and the two heads, 9-10 launches per training
// step).  bilinear^T = R_y^T . gy . R_x is separable: a workgroup owns TLH x 64 INPUT pixels of one plane, stages the output-gradient
// rows / columns they can receive from in LDS, (A) contracts the columns -- H[r][j] = sum_k wx[j][k] * G[r][clo[j] + k], the column
// weights evaluated ONCE per workgroup into an LDS table instead of once per thread and candidate -- and (B) contracts the rows of H
// with the row-weight table.  Candidates, weights and the order of the additions are exactly bilinear_bwd_kernel's (zero-weight
// candidates contribute fma(0, finite, acc) = acc), so the results are bit-identical; the per-thread form spent ~250-300 vector
// instructions per input pixel on re-evaluating bilinear_src (146 us for the 72x120 -> 288x480 head at 16 x 13 planes: 0.8 TB/s).
__host__ __device__ __forceinline__ int bb_lo(float s, int i) { return s > 0.f ? max(0, (int)ceilf((float)(i - 1) / s) - 1) : 0; }
__host__ __device__ __forceinline__ int bb_hi(float s, int i, int O) { return s > 0.f ? min(O - 1, (int)floorf((float)(i + 1) / s) + 1) : O - 1; }

template <int MAXC, int TLH>
__global__ __launch_bounds__(256) void bilinear_bwd_tile_kernel(const float* __restrict__ gy, RsG g, int FH, int FWS, int tiles_x,
                                                                float* __restrict__ gx) {
    constexpr int TLW = 64;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* G = sm;                                      // [FH][FWS]: output-gradient tile, zero past the staged columns
    float* Hh = G + FH * FWS;                           // [FH + MAXC][TLW]: column-contracted rows, zero past the staged rows
    float* WX = Hh + (FH + MAXC) * TLW;                 // [MAXC][TLW] column weights of candidate k of input column j
    float* WY = WX + MAXC * TLW;                        // [TLH][MAXC] row weights
    int* CL = reinterpret_cast<int*>(WY + TLH * MAXC);  // [TLW] first candidate column of input column j, relative to the tile
    int* RL = CL + TLW;                                 // [TLH] first candidate row of input row i, relative to the tile
    const int t = blockIdx.z * gridDim.y + blockIdx.y;  // plane n*C + c
    if (t >= g.N * g.C) return;
    const int txi = blockIdx.x % tiles_x, tyi = blockIdx.x / tiles_x;
    const int iy0 = tyi * TLH, ix0 = txi * TLW;
    const int iyl = min(iy0 + TLH, g.Hi) - 1, ixl = min(ix0 + TLW, g.Wi) - 1;
    const int RY0 = bb_lo(g.sh, iy0), RY1 = bb_hi(g.sh, iyl, g.Ho), CX0 = bb_lo(g.sw, ix0), CX1 = bb_hi(g.sw, ixl, g.Wo);
    const int nrows = min(RY1 - RY0 + 1, FH), ncols = min(CX1 - CX0 + 1, FWS - MAXC);      // (the host sized FH / FWS from the same formulas)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* gp = gy + (size_t)t * g.Ho * g.Wo;
    // ---- stage the gradient tile: a wave per row, lanes over the columns, two rows' loads in flight
    for (int r = wave; r < nrows; r += 8) {
        const float* ra = gp + (size_t)(RY0 + r) * g.Wo + CX0;
        const bool hb = r + 4 < nrows;
        const float* rb = gp + (size_t)(RY0 + (hb ? r + 4 : r)) * g.Wo + CX0;
        for (int c0 = 0; c0 < FWS; c0 += 128) {
            const int ca = c0 + lane, cb = c0 + 64 + lane;
            const float a0 = ca < ncols ? ra[ca] : 0.f, a1 = cb < ncols ? ra[cb] : 0.f;
            const float b0 = (hb && ca < ncols) ? rb[ca] : 0.f, b1 = (hb && cb < ncols) ? rb[cb] : 0.f;
            if (ca < FWS) { G[r * FWS + ca] = a0;  if (hb) G[(r + 4) * FWS + ca] = b0; }
            if (cb < FWS) { G[r * FWS + cb] = a1;  if (hb) G[(r + 4) * FWS + cb] = b1; }
        }
    }
    // rows of H past the staged ones: read (with zero weights) by phase B
    for (int i = tid; i < MAXC * TLW; i += 256) Hh[nrows * TLW + i] = 0.f;
    // ---- weight tables
    for (int task = tid; task < MAXC * TLW; task += 256) {
        const int k = task / TLW, j = task - k * TLW, ix = ix0 + j;
        float w = 0.f;
        int lo = CX0;
        if (ix <= ixl) {
            lo = bb_lo(g.sw, ix);
            const int ox = lo + k;
            if (ox <= bb_hi(g.sw, ix, g.Wo)) {
                int x0, x1;  float wx0, wx1;
                bilinear_src(g.sw, ox, g.Wi, x0, x1, wx0, wx1);
                w = (x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f);
            }
        }
        WX[task] = w;
        if (k == 0) CL[j] = lo - CX0;
    }
    for (int task = tid; task < TLH * MAXC; task += 256) {
        const int i = task / MAXC, k = task - i * MAXC, iy = iy0 + i;
        float w = 0.f;
        int lo = RY0;
        if (iy <= iyl) {
            lo = bb_lo(g.sh, iy);
            const int oy = lo + k;
            if (oy <= bb_hi(g.sh, iy, g.Ho)) {
                int y0, y1;  float wy0, wy1;
                bilinear_src(g.sh, oy, g.Hi, y0, y1, wy0, wy1);
                w = (y0 == iy ? wy0 : 0.f) + (y1 == iy ? wy1 : 0.f);
            }
        }
        WY[task] = w;
        if (k == 0) RL[i] = lo - RY0;
    }
    __syncthreads();
    // ---- (A) contract the columns: thread = input column j, rows wave, wave + 4, ...
    {
        float wx[MAXC];
#pragma unroll
        for (int k = 0; k < MAXC; ++k) wx[k] = WX[k * TLW + lane];
        const float* gcol = G + CL[lane];
        for (int r = wave; r < nrows; r += 4) {
            const float* row = gcol + r * FWS;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < MAXC; ++k) acc = fmaf(wx[k], row[k], acc);
            Hh[r * TLW + lane] = acc;
        }
    }
    __syncthreads();
    // ---- (B) contract the rows and store
    for (int i = wave; i < TLH; i += 4) {
        const int iy = iy0 + i, ix = ix0 + lane;
        if (iy > iyl || ix > ixl) continue;
        const float* hcol = Hh + RL[i] * TLW + lane;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) acc = fmaf(WY[i * MAXC + k], hcol[k * TLW], acc);
        gx[(size_t)t * g.Hi * g.Wi + (size_t)iy * g.Wi + ix] = acc;
    }
}

// Large up-sampling ratios (the pyramid's 0.1 branch: 7x12 -> 64x120, 24x24 candidate outputs per input pixel, and only a
// few hundred input pixels per plane): one WAVE per input pixel, lanes over the candidate columns, rows walked together.
__global__ __launch_bounds__(256) void bilinear_bwd_wave_kernel(const float* __restrict__ gy, RsG g, float* __restrict__ gx, int64_t total_in) {
    const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= total_in) return;                                  // wave-uniform
    const int hw = g.Hi * g.Wi;
    const int64_t t = w / hw;
    const int pi = (int)(w - t * hw);
    const int iy = pi / g.Wi, ix = pi - iy * g.Wi;
    const float* gp = gy + (size_t)t * g.Ho * g.Wo;
    int ylo = 0, yhi = g.Ho - 1, xlo = 0, xhi = g.Wo - 1;
    if (g.sh > 0.f) { ylo = max(0, (int)floorf((float)(iy - 1) / g.sh) - 1); yhi = min(g.Ho - 1, (int)ceilf((float)(iy + 1) / g.sh) + 1); }
    if (g.sw > 0.f) { xlo = max(0, (int)floorf((float)(ix - 1) / g.sw) - 1); xhi = min(g.Wo - 1, (int)ceilf((float)(ix + 1) / g.sw) + 1); }
    float acc = 0.f;
    for (int xb = xlo; xb <= xhi; xb += 64) {
        const int ox = xb + lane;
        float wx = 0.f;
        if (ox <= xhi) {
            int x0, x1;  float wx0, wx1;
            bilinear_src(g.sw, ox, g.Wi, x0, x1, wx0, wx1);
            wx = (x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f);
        }
        const int oxc = min(ox, xhi);
        float col = 0.f;
        for (int oy = ylo; oy <= yhi; ++oy) {
            int y0, y1;  float wy0, wy1;
            bilinear_src(g.sh, oy, g.Hi, y0, y1, wy0, wy1);
            const float wy = (y0 == iy ? wy0 : 0.f) + (y1 == iy ? wy1 : 0.f);
            if (wy == 0.f) continue;                            // wave-uniform
            col = fmaf(wy, gp[(size_t)oy * g.Wo + oxc], col);
        }
        acc = fmaf(wx, col, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) gx[w] = acc;
}

// Large ratios, second form: a workgroup per (plane, INPUT row).  The candidate output rows of that input row are reduced
// vertically with coalesced reads (thread = output column), the row of column sums goes through LDS, then thread b < Wi finishes
// input pixel (row, b) over its candidate columns.  Every output row is read about twice (once per input row it feeds) instead of
// once per input PIXEL and candidate column block: 96 -> ~15 us for the 13x24 -> 128x240 map of the pyramid's 0.1 branch.
__global__ __launch_bounds__(256) void bilinear_bwd_rows_kernel(const float* __restrict__ gy, RsG g, float* __restrict__ gx) {
    extern __shared__ float colsum[];                       // Wo floats
    const int iy = blockIdx.x % g.Hi;
    const int t = blockIdx.x / g.Hi;                        // plane
    const float* gp = gy + (size_t)t * g.Ho * g.Wo;
    int ylo = 0, yhi = g.Ho - 1;
    if (g.sh > 0.f) { ylo = max(0, (int)floorf((float)(iy - 1) / g.sh) - 1); yhi = min(g.Ho - 1, (int)ceilf((float)(iy + 1) / g.sh) + 1); }
    for (int ox = threadIdx.x; ox < g.Wo; ox += 256) {
        float col = 0.f;
        for (int oy = ylo; oy <= yhi; ++oy) {
            int y0, y1;  float wy0, wy1;
            bilinear_src(g.sh, oy, g.Hi, y0, y1, wy0, wy1);
            const float wy = (y0 == iy ? wy0 : 0.f) + (y1 == iy ? wy1 : 0.f);
            if (wy == 0.f) continue;                            // uniform
            col = fmaf(wy, gp[(size_t)oy * g.Wo + ox], col);
        }
        colsum[ox] = col;
    }
    __syncthreads();
    for (int ix = threadIdx.x; ix < g.Wi; ix += 256) {
        int xlo = 0, xhi = g.Wo - 1;
        if (g.sw > 0.f) { xlo = max(0, (int)floorf((float)(ix - 1) / g.sw) - 1); xhi = min(g.Wo - 1, (int)ceilf((float)(ix + 1) / g.sw) + 1); }
        float acc = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            int x0, x1;  float wx0, wx1;
            bilinear_src(g.sw, ox, g.Wi, x0, x1, wx0, wx1);
            const float wx = (x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f);
            acc = fmaf(wx, colsum[ox], acc);
        }
        gx[((size_t)t * g.Hi + iy) * g.Wi + ix] = acc;
    }
}

// Gather form (deterministic, no atomics, no zero fill): one thread per INPUT pixel; the outputs whose window
// [floor(o*I/O), ceil((o+1)*I/O)) contains it are o in [floor(i*O/I), ceil((i+1)*O/I) - 1] (1-2 per axis when pooling down,
// 2-3 when the "pool" enlarges the map, the 2.0 / 1.5 pyramid scales).
__global__ __launch_bounds__(256) void adaptive_avgpool_bwd_kernel(const float* __restrict__ gy, RsG g, float* __restrict__ gx, int64_t total) {
    const int t = blockIdx.z * gridDim.y + blockIdx.y;      // plane n*C + c
    const int pi = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.N * g.C || pi >= g.Hi * g.Wi) return;
    const float* gp = gy + (size_t)t * g.Ho * g.Wo;
    // divisions by the four (launch-constant) sizes through mul-hi magics: exact while numerator * divisor < 2^32, which the
    // launcher checks; a 32-bit hardware-less division is ~30 instructions, and this kernel does ten of them per pixel
    const unsigned Hi = g.Hi, Wi = g.Wi, Ho = g.Ho, Wo = g.Wo;
    const unsigned uy = udiv_magic(pi, Wi, g.mWi), ux = pi - uy * Wi;
    const int oy0 = (int)udiv_magic(uy * Ho, Hi, g.mHi), oy1 = min(g.Ho - 1, (int)udiv_magic((uy + 1) * Ho + Hi - 1, Hi, g.mHi) - 1);
    const int ox0 = (int)udiv_magic(ux * Wo, Wi, g.mWi), ox1 = min(g.Wo - 1, (int)udiv_magic((ux + 1) * Wo + Wi - 1, Wi, g.mWi) - 1);
    float acc = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy) {
        const int ys = (int)udiv_magic((unsigned)oy * Hi, Ho, g.mHo), ye = (int)udiv_magic(((unsigned)oy + 1) * Hi + Ho - 1, Ho, g.mHo);
        if ((int)uy < ys || (int)uy >= ye) continue;
        for (int ox = ox0; ox <= ox1; ++ox) {
            const int xs = (int)udiv_magic((unsigned)ox * Wi, Wo, g.mWo), xe = (int)udiv_magic(((unsigned)ox + 1) * Wi + Wo - 1, Wo, g.mWo);
            if ((int)ux < xs || (int)ux >= xe) continue;
            acc += gp[(size_t)oy * g.Wo + ox] / (float)((ye - ys) * (xe - xs));
        }
    }
    gx[(size_t)t * g.Hi * g.Wi + pi] = acc;
}

}  // namespace mspl

using namespace mspl;

static void rs_geom_fill(int N, int C, int Hi, int Wi, int Ho, int Wo, RsG& g) {
    g.N = N; g.C = C; g.Hi = Hi; g.Wi = Wi; g.Ho = Ho; g.Wo = Wo;
    g.sh = bilinear_scale(Hi, Ho); g.sw = bilinear_scale(Wi, Wo);
    auto magic = [](int d) { return (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); };
    g.mHi = magic(Hi); g.mWi = magic(Wi); g.mHo = magic(Ho); g.mWo = magic(Wo);
}

static int rs_geom(const char* who, const float* gy, float* gx, int N, int C, int Hi, int Wi, int Ho, int Wo, RsG& g) {
    MSPL_REQUIRE(gy && gx, MSPL_ERR_NULL_POINTER, "%s: null pointer", who);
    MSPL_REQUIRE(N > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, MSPL_ERR_BAD_SHAPE, "%s: bad shape", who);
    rs_geom_fill(N, C, Hi, Wi, Ho, Wo, g);
    return MSPL_OK;
}

// Which kernel form mspl_avgpool3x3s2_bwd launches: decided here and nowhere else (the launcher switches on the result,
// mspl_avgpool3x3s2_bwd_plan hands it to callers and tests).  aligned16: gy and gx are both 16-byte aligned.
static int avgpool3x3s2_bwd_plan(int H, int W, bool aligned16) {
    return ((H & 1) == 0 && (W & 7) == 0 && aligned16) ? MSPL_AVGPOOL_BWD_VEC : MSPL_AVGPOOL_BWD_PLAIN;      // whole 16-byte strips on both sides
}

extern "C" int mspl_avgpool3x3s2_bwd_plan(int32_t N, int32_t C, int32_t H, int32_t W, int32_t aligned16, int32_t* form) {
    MSPL_REQUIRE(form, MSPL_ERR_NULL_POINTER, "avgpool3x3s2_bwd_plan: null pointer");
    MSPL_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, MSPL_ERR_BAD_SHAPE, "avgpool3x3s2_bwd_plan: bad shape");
    MSPL_REQUIRE((int64_t)H * W * W < (1ll << 32), MSPL_ERR_BAD_SHAPE, "avgpool3x3s2_bwd_plan: plane too large for 32-bit index arithmetic");
    *form = avgpool3x3s2_bwd_plan(H, W, aligned16 != 0);
    return MSPL_OK;
}

extern "C" int mspl_avgpool3x3s2_bwd(const float* gy, int32_t N, int32_t C, int32_t H, int32_t W, float* gx, void* stream) {
    RsG g;
    if (int rc = rs_geom("avgpool3x3s2_bwd", gy, gx, N, C, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1, g)) return rc;
    const int64_t total = (int64_t)N * C * H * W;
    MSPL_REQUIRE((int64_t)H * W * W < (1ll << 32), MSPL_ERR_BAD_SHAPE, "avgpool3x3s2_bwd: plane too large for 32-bit index arithmetic");
    if (avgpool3x3s2_bwd_plan(H, W, ((((uintptr_t)gy) | ((uintptr_t)gx)) & 15) == 0) == MSPL_AVGPOOL_BWD_VEC) {
        const int XS = g.Wo / 4;
        hipLaunchKernelGGL(avgpool3x3s2_bwd_vec_kernel, plane_grid(ceil_div(g.Ho * XS, 256), N * C), dim3(256), 0, (hipStream_t)stream, gy, g, XS, gx);
        MSPL_CHECK_LAUNCH("avgpool3x3s2_bwd(16-byte strips)");
        return MSPL_OK;
    }
    hipLaunchKernelGGL(avgpool3x3s2_bwd_kernel, plane_grid(ceil_div(H * W, 256), N * C), dim3(256), 0, (hipStream_t)stream, gy, g, gx, total);
    MSPL_CHECK_LAUNCH("avgpool3x3s2_bwd");
    return MSPL_OK;
}

// Which kernel form mspl_bilinear_bwd launches for a shape, and the tile forms' grid and LDS extents: the ONE place where that is
// decided (the launcher below switches on the result; mspl_bilinear_bwd_plan hands it to callers and tests).  No form depends on
// the operands' alignment.
struct BilinearBwdPlan {
    int form;                // mspl_bilinear_bwd_form_t
    int tiles_x, tiles_y;    // tile forms: workgroups per plane along x / y; else 0
    int FH, FW;              // tile forms: staged output-gradient rows / columns; else 0
    int FWS;                 // tile forms: LDS row stride
    size_t lds;
};

static BilinearBwdPlan bilinear_bwd_plan(const RsG& g) {
    BilinearBwdPlan p;
    memset(&p, 0, sizeof(p));
    const int N = g.N, C = g.C, Hi = g.Hi, Wi = g.Wi, Ho = g.Ho, Wo = g.Wo;
    const int64_t total = (int64_t)N * C * Hi * Wi;
    // candidate window per input pixel is 2/scale + 3 wide: beyond 12 columns a wave per input pixel is the better shape
    const bool wide = g.sw <= 0.f || 2.0f / g.sw + 3.0f > 12.0f;
    static const int rows_form = MSPL_TUNE_INT("MSPL_BILINEAR_BWD_ROWS", 1);
    if (wide && rows_form && Wo <= 8192 && (int64_t)N * C * Hi < (1ll << 31)) { p.form = MSPL_BILINEAR_BWD_ROWS; return p; }
    if (wide && total * 64 < (1ll << 31) * 256ll) { p.form = MSPL_BILINEAR_BWD_WAVE; return p; }
    static const int tile_form = MSPL_TUNE_INT("MSPL_BILINEAR_BWD_TILE", 1);
    if (tile_form && g.sh > 0.f && g.sw > 0.f) {
        // candidate windows (rows and columns) of at most 8 (x2) or 12 (x4): the tiled separable form
        const float cw = 2.0f / g.sw + 3.0f, rw = 2.0f / g.sh + 3.0f;
        const int maxc = (cw <= 8.0f && rw <= 8.0f) ? 8 : ((cw <= 12.0f && rw <= 12.0f) ? 12 : 0);
        if (maxc) {
            const int TLH = maxc == 8 ? 8 : 4, TLW = 64;
            const int tiles_x = ceil_div(Wi, TLW), tiles_y = ceil_div(Hi, TLH);
            int FH = 1, FW = 1;
            for (int ty = 0; ty < tiles_y; ++ty) {
                const int i0 = ty * TLH, il = (i0 + TLH < Hi ? i0 + TLH : Hi) - 1;
                FH = std::max(FH, bb_hi(g.sh, il, Ho) - bb_lo(g.sh, i0) + 1);
            }
            for (int tx = 0; tx < tiles_x; ++tx) {
                const int i0 = tx * TLW, il = (i0 + TLW < Wi ? i0 + TLW : Wi) - 1;
                FW = std::max(FW, bb_hi(g.sw, il, Wo) - bb_lo(g.sw, i0) + 1);
            }
            const int FWS = ((FW + maxc + 3) & ~3) | 4;            // row stride: staged columns + the candidates' over-read, not a multiple of 8 floats
            const size_t lds = ((size_t)FH * FWS + (size_t)(FH + maxc) * TLW + (size_t)maxc * TLW + (size_t)TLH * maxc + TLW + TLH) * sizeof(float);
            if (lds <= 64 * 1024 && (int64_t)tiles_x * tiles_y < (1ll << 31)) {
                p.form = maxc == 8 ? MSPL_BILINEAR_BWD_TILE8 : MSPL_BILINEAR_BWD_TILE12;
                p.tiles_x = tiles_x; p.tiles_y = tiles_y; p.FH = FH; p.FW = FW; p.FWS = FWS; p.lds = lds;
                return p;
            }
        }
    }
    // x2 up-sampling (the decoder, the heads): at most 7 candidate columns
    p.form = (g.sw > 0.f && 2.0f / g.sw + 3.0f <= 8.0f) ? MSPL_BILINEAR_BWD_GENERIC8 : MSPL_BILINEAR_BWD_GENERIC12;
    return p;
}

extern "C" int mspl_bilinear_bwd_plan(int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t aligned,
                                      int32_t* form, int32_t* tiles_x, int32_t* tiles_y, int32_t* FH, int32_t* FW) {
    (void)aligned;
    MSPL_REQUIRE(form, MSPL_ERR_NULL_POINTER, "bilinear_bwd_plan: null pointer");
    MSPL_REQUIRE(N > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, MSPL_ERR_BAD_SHAPE, "bilinear_bwd_plan: bad shape");
    RsG g;
    rs_geom_fill(N, C, Hi, Wi, Ho, Wo, g);
    const BilinearBwdPlan p = bilinear_bwd_plan(g);
    *form = p.form;
    if (tiles_x) *tiles_x = p.tiles_x;
    if (tiles_y) *tiles_y = p.tiles_y;
    if (FH) *FH = p.FH;
    if (FW) *FW = p.FW;
    return MSPL_OK;
}

/* Gather form: gx is overwritten. */
extern "C" int mspl_bilinear_bwd(const float* gy, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                 float* gx, void* stream) {
    RsG g;
    if (int rc = rs_geom("bilinear_bwd", gy, gx, N, C, Hi, Wi, Ho, Wo, g)) return rc;
    const int64_t total = (int64_t)N * C * Hi * Wi;
    const BilinearBwdPlan plan = bilinear_bwd_plan(g);
    const dim3 grid = plane_grid(ceil_div(Hi * Wi, 256), N * C);
    switch (plan.form) {
    case MSPL_BILINEAR_BWD_ROWS:
        hipLaunchKernelGGL(bilinear_bwd_rows_kernel, dim3((unsigned)((int64_t)N * C * Hi)), dim3(256), (size_t)Wo * sizeof(float),
                           (hipStream_t)stream, gy, g, gx);
        MSPL_CHECK_LAUNCH("bilinear_bwd(rows)");
        return MSPL_OK;
    case MSPL_BILINEAR_BWD_WAVE:
        hipLaunchKernelGGL(bilinear_bwd_wave_kernel, dim3((unsigned)ceil_div64(total * 64, 256)), dim3(256), 0, (hipStream_t)stream, gy, g,
                           gx, total);
        MSPL_CHECK_LAUNCH("bilinear_bwd(wave)");
        return MSPL_OK;
    case MSPL_BILINEAR_BWD_TILE8:
    case MSPL_BILINEAR_BWD_TILE12: {
        const dim3 tgrid = plane_grid(plan.tiles_x * plan.tiles_y, N * C);
        if (plan.form == MSPL_BILINEAR_BWD_TILE8)
            hipLaunchKernelGGL((bilinear_bwd_tile_kernel<8, 8>), tgrid, dim3(256), plan.lds, (hipStream_t)stream, gy, g, plan.FH, plan.FWS, plan.tiles_x, gx);
        else
            hipLaunchKernelGGL((bilinear_bwd_tile_kernel<12, 4>), tgrid, dim3(256), plan.lds, (hipStream_t)stream, gy, g, plan.FH, plan.FWS, plan.tiles_x, gx);
        MSPL_CHECK_LAUNCH("bilinear_bwd(tiled)");
        return MSPL_OK;
    }
    case MSPL_BILINEAR_BWD_GENERIC8:
        hipLaunchKernelGGL(bilinear_bwd_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, gy, g, gx, total);
        break;
    default:
        hipLaunchKernelGGL(bilinear_bwd_kernel<12>, grid, dim3(256), 0, (hipStream_t)stream, gy, g, gx, total);
        break;
    }
    MSPL_CHECK_LAUNCH("bilinear_bwd");
    return MSPL_OK;
}

/* Gather form: gx is overwritten. */
extern "C" int mspl_adaptive_avgpool_bwd(const float* gy, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                         float* gx, void* stream) {
    RsG g;
    if (int rc = rs_geom("adaptive_avgpool_bwd", gy, gx, N, C, Hi, Wi, Ho, Wo, g)) return rc;
    // numerators reach (Hi+1)*Ho + Hi resp. Hi*Wi; the magics are exact while numerator * divisor < 2^32
    MSPL_REQUIRE(((int64_t)(Hi + 1) * Ho + Hi) * (Hi > Ho ? Hi : Ho) < (1ll << 32) && ((int64_t)(Wi + 1) * Wo + Wi) * (Wi > Wo ? Wi : Wo) < (1ll << 32) &&
                     (int64_t)Hi * Wi * Wi < (1ll << 32),
                 MSPL_ERR_BAD_SHAPE, "adaptive_avgpool_bwd: map too large for the 32-bit window arithmetic");
    const int64_t total = (int64_t)N * C * Hi * Wi;
    hipLaunchKernelGGL(adaptive_avgpool_bwd_kernel, plane_grid(ceil_div(Hi * Wi, 256), N * C), dim3(256), 0, (hipStream_t)stream, gy, g, gx, total);
    MSPL_CHECK_LAUNCH("adaptive_avgpool_bwd");
    return MSPL_OK;
}
