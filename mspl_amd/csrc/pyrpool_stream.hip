// K6, third form -- the fused EfficientPyrPool body as a register-streaming kernel (no LDS traffic in the inner loop).
//
// Same arithmetic as pyrpool_sep.hip (nn_layers/efficient_pyramid_pool.py:36-61; the up-sampled branches collapsed into
// position-dependent separable stencils on x), same order of floating-point operations, different machine mapping.  The
// stencil form in pyrpool_sep.hip turned out to be LDS-bound: per 1x4 strip it issues ~107 LDS reads (x patch, per-row and
// per-column coefficient tables, low-resolution maps, branch tiles for the merge convolution) for ~430 FMAs, and a CU's four
// SIMDs share one LDS pipe (PMC / MSPL_PYR_STOP timings).  Here nothing in the inner loop goes through LDS:
//   * a WAVE owns one (image, plane), one block of columns and one segment of rows; lane = PXL adjacent columns; the wave
//     walks DOWN the rows.  The 5-row window of x and the 3-row window of the five branch maps live in registers and slide.
//   * row-dependent coefficients (A tables) are wave-uniform: computed once per wave into a small LDS table, read back with
//     broadcast reads (3-6 per row); column-dependent coefficients (C tables, bilinear sources of the low-resolution maps) are
//     per-lane constants computed once per wave and kept in registers; weights / BN constants of the plane are wave-uniform
//     (scalar loads).
//   * the merge convolution needs the branch values of the two neighbouring columns: v_mov_dpp wave_shr / wave_shl from the
//     neighbouring lanes; lanes 0 and 63 are halo lanes (they compute branch values but write no output), so waves never
//     exchange data and there is no barrier in the kernel.
//   * x rows and low-resolution rows are read straight from global memory (coalesced 4/8-byte accesses, L1/L2 hits for the
//     overlaps), the next row's loads are issued one row ahead.
//   * the A and G tables depend on the map geometry alone: the inference launches read them from a block that p3_tables_kernel wrote
//     once (TAB form, row segments up to 72 rows); the training forward and mspl_pyrpool_fused_fwd compute them per workgroup.
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>

#include "common.hpp"
#include "pyr_geom.hpp"

namespace mspl {

constexpr int P3_MAXB = 5;
// Branch rows per trip of the row loop.  One row per trip pays ~60 of its ~312 vector instructions for moving the sliding windows at
// the back edge (hipcc does not unroll the loop by itself: `#pragma unroll 2` is refused); with two steps in the loop body the windows
// are renamed between them: rocprofv3 inside the label pass, alternating libraries, 43.4 -> 41.9 us per launch at 144x240 / 72x120,
// 24.2 -> 22.9 us for the one-pixel form.  Three and five steps (222 / 256 registers, no spill) are SLOWER (47.6 / 49.0 us).
#ifndef P3_STEPS
#define P3_STEPS 2
#endif
constexpr int P3_SEGMAX = 19;       // in-kernel tables: (SEG + 2) * 3 row-table entries are computed by the 64 lanes in one step
// Geometry tables from memory (TAB): a segment's rows ys-1 .. ye of both A tables are copied into LDS, 2 * (SEG + 2) * 96 bytes; 72
// rows take the 14 KB the column tables of the in-kernel form take, so the LDS bound on resident workgroups stays where it was.
constexpr int P3_TAB_SEGMAX = 72;
constexpr int P3_TAB_ACOPY = ((P3_TAB_SEGMAX + 2) * 6 + 127) / 128;       // 16-byte pieces per thread of the copy (128 threads per table)

struct Pyr3Geom {
    int N, P, h, w;
    int hs[P3_MAXB], ws[P3_MAXB];
    float sh[P3_MAXB], sw[P3_MAXB];  // up branches: x -> U grid; down branches: E grid -> output grid
    int SEG, nseg, ncb, CBW;         // output rows per segment, segments per plane, column blocks, output columns per block
    unsigned total;                  // waves
};

// One up branch for the lane's PXL columns at one row.  xw[rr][j]: image row br-2+rr, column px0-2+j.
// Arow: this row's [ky][8] coefficients in LDS (same address for every lane: broadcast read).  Same evaluation order as
// up_branch_strip (pyrpool_sep.hip): per kernel row ky the vertical stencil first, then the horizontal one, accumulated over ky.
template <int T, int PXL>
__device__ __forceinline__ void p3_up_branch(const float (&xw)[5][PXL + 4], const float* __restrict__ Arow,
                                             const float (&C)[3][PXL][5], float (&b)[PXL]) {
    constexpr int R0 = (5 - T) / 2;
    constexpr int NCOL = PXL + T - 1;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        float a[5];
        {
            const float4 t4 = *reinterpret_cast<const float4*>(Arow + ky * 8);
            a[0] = t4.x; a[1] = t4.y; a[2] = t4.z; a[3] = t4.w;
            a[4] = T > 4 ? Arow[ky * 8 + 4] : 0.f;
        }
        float cs[NCOL];
#pragma unroll
        for (int s = 0; s < NCOL; ++s) {
            float v = a[0] * xw[R0][R0 + s];
#pragma unroll
            for (int rr = 1; rr < T; ++rr) v = fmaf(a[rr], xw[R0 + rr][R0 + s], v);
            cs[s] = v;
        }
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
            float v = b[j];
#pragma unroll
            for (int s = 0; s < T; ++s) v = fmaf(C[ky][j][s], cs[j + s], v);
            b[j] = v;
        }
    }
}

template <int PXL> struct P3Vec;
template <> struct P3Vec<1> { typedef float T; };
template <> struct P3Vec<2> { typedef float2 T; };
template <int PXL> __device__ __forceinline__ float p3_vec_get(const typename P3Vec<PXL>::T& v, int j);
template <> __device__ __forceinline__ float p3_vec_get<1>(const float& v, int) { return v; }
template <> __device__ __forceinline__ float p3_vec_get<2>(const float2& v, int j) { return j == 0 ? v.x : v.y; }

// Branch layout handled here (the reference's scales sorted descending: 2.0, 1.5, 1.0, 0.5, 0.1):
//   branch 0: up (T0 taps), 1: up (T1 taps), 2: same, 3: down, 4: down.
// Every read-only operand is a `const float* __restrict__` kernel argument of its own: only then does hipcc turn the
// wave-uniform reads of the plane's weights into scalar loads (pointers inside the geometry struct are not known to be
// unaliased with `out`, and the per-row constants came back as 13 global_load_dwordx4 per lane and row).
// TRAIN: the training forward also keeps the branch values before merge_layer.0 (zcat, torch.cat order) and the bare merge convolution
// (mraw): what the backward kernels of pyrpool_train.hip read.
// TAB: the row and column tables come from memory (p3_tables_kernel below wrote them, once per geometry) instead of being computed
// by every workgroup; tab = [A: ub][row -1 .. h][ky][8] then [G: ub][kx][tap][lane slot][PXL], lane slot = cb * 62 + lane.
template <int T0, int T1, int PXL, bool TRAIN, bool TAB>
__global__ __launch_bounds__(256, 2) void pyrpool_stream_kernel(const float* __restrict__ x, const float* __restrict__ sw0,
                                                                const float* __restrict__ sw1, const float* __restrict__ sw2,
                                                                const float* __restrict__ de3, const float* __restrict__ de4,
                                                                const float* __restrict__ br_scale, const float* __restrict__ br_shift,
                                                                const float* __restrict__ br_alpha, const float* __restrict__ merge_w,
                                                                const float* __restrict__ ep_scale,
                                                                const float* __restrict__ ep_shift,
                                                                const float* __restrict__ ep_alpha, int ep_ctot, int ep_coff,
                                                                Pyr3Geom g, float* __restrict__ out, float* __restrict__ zcat,
                                                                float* __restrict__ mraw, const float* __restrict__ tab) {
    // The four waves of a workgroup take four consecutive planes of the SAME column block and row segment: the row tables (A) and
    // the channel-independent column tables (G) are identical for them, so they are computed once per workgroup (a quarter of
    // the column tasks per wave) into LDS; after the one barrier every wave folds its own plane's 3x3 weights into its
    // per-lane C tables and never touches LDS tables of columns again.
    __shared__ __attribute__((aligned(16))) float At[2][((TAB ? P3_TAB_SEGMAX : P3_SEGMAX) + 2) * 24];        // [up branch][row][ky][8]
    // merge_layer.2's 45 weights of the wave's plane, [branch][12] (9 used): read back with three broadcast 16-byte LDS reads per
    // branch and row.  As 45 scalar registers (rounds 1-2) they did not fit next to the other plane constants: 44 spilled SGPRs,
    // 32 v_readlane per row step (412 -> 382 vector instructions per row; same box, three launches in flight: 16 400 -> 16 700 images/s).
    __shared__ __attribute__((aligned(16))) float Wm[4][5][12];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned bid = blockIdx.x;
    const int sgi = bid % g.nseg;  bid /= g.nseg;
    const int cb = bid % g.ncb;  bid /= g.ncb;
    const int plane = (int)bid * 4 + wave;                                 // (N * P) % 4 == 0 (checked by the launcher)
    const int n = plane / g.P, c = plane - n * g.P;
    const int h = g.h, w = g.w;
    const int ys = sgi * g.SEG, ye = min(ys + g.SEG, h);
    const int px0 = cb * g.CBW + (lane - 1) * PXL;                      // lane 0 / 63: halo columns of the block
    const bool writer = lane >= 1 && lane <= 62 && px0 < w;

    float C0[3][PXL][5], C1[3][PXL][5];
    typedef typename P3Vec<PXL>::T gvec_t;
    gvec_t Gr[2][3][5];                                                  // TAB: this lane's G entries, [up branch][kx][tap] x PXL columns
    float4 Ar[P3_TAB_ACOPY];                                             // TAB: this thread's pieces of the segment's A rows
    if constexpr (!TAB) {
        __shared__ float Gt[2][3][PXL][5][64];                                             // [up branch][kx][column][tap][lane]
        // ---- per-workgroup setup
        // (1) row tables of the two up branches (wave 0: branch 0, wave 1: branch 1): entry = lane -> (row index, ky), rows ys-1 .. ye
        if (wave < 2) {
            const int ri = lane / 3, ky = lane - 3 * ri;
            if (ri < g.SEG + 2) {
                float acc[5];
                if (wave == 0) p3_coeffs<T0>(ys - 1 + ri, ky, h, g.hs[0], g.sh[0], acc);
                else p3_coeffs<T1>(ys - 1 + ri, ky, h, g.hs[1], g.sh[1], acc);
                float* d = &At[wave][ri * 24 + ky * 8];
                d[0] = acc[0]; d[1] = acc[1]; d[2] = acc[2]; d[3] = acc[3]; d[4] = acc[4];
            }
        }
        // (2) column tables G_kx[column][tap]: 6 * PXL tasks (branch, kx, column) per lane, task t goes to wave t % 4
#pragma unroll
        for (int t = 0; t < 6 * PXL; ++t) {
            if ((t & 3) == wave) {                                          // uniform
                const int ub = t / (3 * PXL), r = t - ub * 3 * PXL, kx = r / PXL, j = r - kx * PXL;     // compile-time
                float acc[5];
                if (ub == 0) p3_coeffs<T0>(px0 + j, kx, w, g.ws[0], g.sw[0], acc);
                else p3_coeffs<T1>(px0 + j, kx, w, g.ws[1], g.sw[1], acc);
#pragma unroll
                for (int q = 0; q < 5; ++q) Gt[ub][kx][j][q][lane] = acc[q];
            }
        }
        __syncthreads();
        // (2b) per-lane C_ky[j][s] = sum_kx w[ky][kx] * G_kx[j][s] with this wave's plane's weights
        {
            const float* w0p = sw0 + (size_t)c * 9;
            const float* w1p = sw1 + (size_t)c * 9;
#pragma unroll
            for (int j = 0; j < PXL; ++j)
#pragma unroll
                for (int s2 = 0; s2 < 5; ++s2) {
                    const float a0 = Gt[0][0][j][s2][lane], a1 = Gt[0][1][j][s2][lane], a2 = Gt[0][2][j][s2][lane];
                    const float b0 = Gt[1][0][j][s2][lane], b1 = Gt[1][1][j][s2][lane], b2 = Gt[1][2][j][s2][lane];
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        C0[ky][j][s2] = fmaf(w0p[ky * 3 + 2], a2, fmaf(w0p[ky * 3 + 1], a1, w0p[ky * 3] * a0));
                        C1[ky][j][s2] = fmaf(w1p[ky * 3 + 2], b2, fmaf(w1p[ky * 3 + 1], b1, w1p[ky * 3] * b0));
                    }
                }
        }
    } else {
        // ---- tables from memory.  Requested first, so that they fly together with the x rows and the low-resolution samples below:
        // the lane's column entries (taps a branch does not have are zero and never read) ...
        const gvec_t* Gp = reinterpret_cast<const gvec_t*>(tab + 2 * (h + 2) * 24);
        const int nslots = g.ncb * 62 + 2, slot = cb * 62 + lane;
#pragma unroll
        for (int ub = 0; ub < 2; ++ub)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int q = 0; q < 5; ++q)
                    if (q < (ub == 0 ? T0 : T1)) Gr[ub][kx][q] = Gp[((ub * 3 + kx) * 5 + q) * nslots + slot];
        // ... and the workgroup's copy of the segment's rows ys-1 .. ye of A (waves 0-1: branch 0, waves 2-3: branch 1)
        const int npc = min(g.SEG + 2, h + 2 - ys) * 6, t7 = threadIdx.x & 127;
        const float4* Ap = reinterpret_cast<const float4*>(tab) + ((wave >> 1) * (h + 2) + ys) * 6;
#pragma unroll
        for (int k = 0; k < P3_TAB_ACOPY; ++k) Ar[k] = Ap[min(t7 + 128 * k, npc - 1)];
    }
    // (3) per-lane bilinear column sources of the two low-resolution maps
    unsigned dxa[2][PXL], dxb[2][PXL];  float dw0[2][PXL], dw1[2][PXL];        // byte offsets inside a low-resolution row
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < PXL; ++j) {
            const int px = min(max(px0 + j, 0), w - 1);
            int xa, xb;
            bilinear_src(g.sw[3 + i], px, g.ws[3 + i], xa, xb, dw0[i][j], dw1[i][j]);
            dxa[i][j] = (unsigned)xa * 4u;  dxb[i][j] = (unsigned)xb * 4u;
        }
    // (4) wave-uniform constants of this plane (scalar loads)
    const float* wsame = sw2 + (size_t)c * 9;
    if (lane < 45) Wm[wave][lane / 9][lane % 9] = merge_w[(size_t)c * 45 + lane];      // (a wave's LDS operations execute in order: no barrier)
    const float4* wmq = reinterpret_cast<const float4*>(&Wm[wave][0][0]);
    float bsc[5], bsh[5], bal[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) { bsc[i] = br_scale[i * g.P + c]; bsh[i] = br_shift[i * g.P + c]; bal[i] = br_alpha[i * g.P + c]; }
    const int cabs = ep_coff + c;
    const float esc = ep_scale ? ep_scale[cabs] : 1.f, esh = ep_shift ? ep_shift[cabs] : 0.f, eal = ep_alpha ? ep_alpha[cabs] : 1.f;
    // The plane index is wave-uniform (n, c follow from the wave index); said so explicitly, the plane bases are kernel argument +
    // scalar offset and the row bases of the loop are computed on the scalar unit (412 -> 392 vector instructions per row step).
    const unsigned plane_id = __builtin_amdgcn_readfirstlane((unsigned)(n * g.P + c));
    const float* xpl = x + (size_t)plane_id * (size_t)(h * w);
    const float* e3 = de3 + (size_t)plane_id * (size_t)(g.hs[3] * g.ws[3]);
    const float* e4 = de4 + (size_t)plane_id * (size_t)(g.hs[4] * g.ws[4]);
    float* opl = out + ((size_t)__builtin_amdgcn_readfirstlane((unsigned)(n * ep_ctot + cabs))) * (size_t)(h * w);
    bool colin[PXL];
#pragma unroll
    for (int j = 0; j < PXL; ++j) colin[j] = px0 + j >= 0 && px0 + j < w;

    // x row loader: columns px0-2 .. px0+PXL+1 of row r (zero outside the image).  Buffer loads through a per-ROW descriptor built on
    // the scalar unit (base = the row, records = the row's bytes, or 0 for a row outside the image) + a per-lane byte offset that
    // never changes (columns outside the image: an offset past the records): the range check of the load returns the zeros, so
    // no vector instruction goes into addressing or masking (rounds 2-4: one 64-bit address add per load and one multiply by a
    // 0/1 mask per value -- 12 of the ~500 vector instructions of a row step; 28 with the low-resolution rows below).
    // PXL == 2: px0 is even and so is w (launcher), so the six columns are three 8-byte loads, each inside or outside as a whole.
    constexpr unsigned P3_OOB = 0x7ffffff0u;
    unsigned xoff[PXL + 4];
#pragma unroll
    for (int j = 0; j < PXL + 4; ++j) {
        const int cx = px0 - 2 + j;
        xoff[j] = (cx >= 0 && cx < w) ? (unsigned)cx * 4u : P3_OOB;
    }
    auto load_row = [&](int r, float (&v)[PXL + 4]) {
        const bool rin = r >= 0 && r < h;                                                   // uniform
        const float* row = xpl + (size_t)(rin ? r : 0) * w;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, rin ? w * 4 : 0, 0x00020000);
        if (PXL == 2) {
#pragma unroll
            for (int j = 0; j < PXL + 4; j += 2) {
                typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rs, xoff[j], 0, 0);
                v[j] = __uint_as_float(t.x);  v[j + 1] = __uint_as_float(t.y);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PXL + 4; ++j) v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xoff[j], 0, 0));
        }
    };

    float xw[5][PXL + 4];
    // rows br-2 .. br+2 for the first branch row br = ys - 1: rows ys-3 .. ys+1
#pragma unroll
    for (int rr = 0; rr < 5; ++rr) load_row(ys - 3 + rr, xw[rr]);
    // low-resolution values of the NEXT branch row, requested one row ahead: [map][column][ya/xa, ya/xb, yb/xa, yb/xb]
    float en[2][PXL][4];
    float enwy0[2], enwy1[2];
    auto load_e = [&](int r) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int ya, yb;
            bilinear_src(g.sh[3 + i], min(max(r, 0), h - 1), g.hs[3 + i], ya, yb, enwy0[i], enwy1[i]);       // uniform
            const int rowb = g.ws[3 + i] * 4;
            const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>((i == 0 ? e3 : e4) + ya * g.ws[3 + i]), 0, rowb, 0x00020000);
            const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>((i == 0 ? e3 : e4) + yb * g.ws[3 + i]), 0, rowb, 0x00020000);
#pragma unroll
            for (int j = 0; j < PXL; ++j) {
                en[i][j][0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ra, dxa[i][j], 0, 0));
                en[i][j][1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ra, dxb[i][j], 0, 0));
                en[i][j][2] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, dxa[i][j], 0, 0));
                en[i][j][3] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, dxb[i][j], 0, 0));
            }
        }
    };
    load_e(ys - 1);
    if constexpr (TAB) {
        const int npc = min(g.SEG + 2, h + 2 - ys) * 6, t7 = threadIdx.x & 127;
        float4* Ad = reinterpret_cast<float4*>(&At[wave >> 1][0]);
#pragma unroll
        for (int k = 0; k < P3_TAB_ACOPY; ++k)
            if (t7 + 128 * k < npc) Ad[t7 + 128 * k] = Ar[k];
        __syncthreads();
        // per-lane C_ky[j][s] = sum_kx w[ky][kx] * G_kx[j][s] with this wave's plane's weights: the expression of step (2b) above
        const float* w0p = sw0 + (size_t)c * 9;
        const float* w1p = sw1 + (size_t)c * 9;
#pragma unroll
        for (int j = 0; j < PXL; ++j)
#pragma unroll
            for (int s2 = 0; s2 < 5; ++s2) {
                float ga[3], gb[3];
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    ga[kx] = s2 < T0 ? p3_vec_get<PXL>(Gr[0][kx][s2], j) : 0.f;
                    gb[kx] = s2 < T1 ? p3_vec_get<PXL>(Gr[1][kx][s2], j) : 0.f;
                }
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    C0[ky][j][s2] = fmaf(w0p[ky * 3 + 2], ga[2], fmaf(w0p[ky * 3 + 1], ga[1], w0p[ky * 3] * ga[0]));
                    C1[ky][j][s2] = fmaf(w1p[ky * 3 + 2], gb[2], fmaf(w1p[ky * 3 + 1], gb[1], w1p[ky * 3] * gb[0]));
                }
            }
    }
    // Merge convolution, accumulated as the branch rows arrive: branch row br contributes kernel row 2 of output row br-1, kernel
    // row 1 of output row br and kernel row 0 of output row br+1.  acc[0]: output row br-1 (complete after this row), acc[1]: row
    // br, acc[2]: row br+1.  (Summation order over (branch, kernel row) differs from pyrpool_sep's branch-major order: fp32
    // rounding-level differences, covered by the tests' tolerance against the oracle.)
    float acc[3][PXL];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < PXL; ++j) acc[r][j] = 0.f;

    // Two branch rows per trip of the loop: the sliding windows (x rows, low-resolution samples, merge accumulators) are renamed
    // between the two steps instead of moved, the moves are paid once per trip at the back edge.
    auto row_step = [&](const int br) __attribute__((always_inline)) {
        // ---- branch maps of row br
        float bv[5][PXL];
        const bool rowin = br >= 0 && br < h;
        float ecur[2][PXL][4], wy0c[2], wy1c[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wy0c[i] = enwy0[i]; wy1c[i] = enwy1[i];
#pragma unroll
            for (int j = 0; j < PXL; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) ecur[i][j][q] = en[i][j][q];
        }
        if (br < ye) load_e(br + 1);                       // next row's low-resolution values fly during this row's arithmetic
        float xn[PXL + 4];
        load_row(br + 3, xn);                              // the row that enters the window at the end of this iteration
        __builtin_amdgcn_sched_barrier(0);
        if (rowin) {
            const float* A0 = &At[0][(br - (ys - 1)) * 24];
            const float* A1 = &At[1][(br - (ys - 1)) * 24];
#pragma unroll
            for (int j = 0; j < PXL; ++j) { bv[0][j] = 0.f; bv[1][j] = 0.f; bv[2][j] = 0.f; }
            p3_up_branch<T0, PXL>(xw, A0, C0, bv[0]);
            p3_up_branch<T1, PXL>(xw, A1, C1, bv[1]);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float w0 = wsame[ky * 3], w1 = wsame[ky * 3 + 1], w2 = wsame[ky * 3 + 2];
#pragma unroll
                for (int j = 0; j < PXL; ++j) {
                    bv[2][j] = fmaf(w0, xw[1 + ky][j + 1], bv[2][j]);
                    bv[2][j] = fmaf(w1, xw[1 + ky][j + 2], bv[2][j]);
                    bv[2][j] = fmaf(w2, xw[1 + ky][j + 3], bv[2][j]);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < PXL; ++j) {
                    const float top = dw0[i][j] * ecur[i][j][0] + dw1[i][j] * ecur[i][j][1];
                    const float bot = dw0[i][j] * ecur[i][j][2] + dw1[i][j] * ecur[i][j][3];
                    bv[3 + i][j] = wy0c[i] * top + wy1c[i] * bot;
                }
            if (TRAIN && writer && br >= ys && br < ye) {          // rows ys-1 and ye belong to the neighbouring segments
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    float* zp = zcat + (((size_t)n * 5 + i) * g.P + c) * (size_t)h * w + (size_t)br * w + px0;
                    if (PXL == 2) *reinterpret_cast<float2*>(zp) = make_float2(bv[i][0], bv[i][PXL - 1]);
                    else zp[0] = bv[i][0];
                }
            }
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int j = 0; j < PXL; ++j) {
                    float v = fmaf(bv[i][j], bsc[i], bsh[i]);
                    v = v > 0.f ? v : bal[i] * v;
                    bv[i][j] = colin[j] ? v : 0.f;           // zero outside the image: the merge convolution's padding
                }
        } else {
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int j = 0; j < PXL; ++j) bv[i][j] = 0.f;
        }
        // ---- this row's contributions to the three output rows it touches; neighbouring columns come from the neighbouring lanes
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            float bx[PXL + 2];
            bx[0] = p3_from_left(bv[i][PXL - 1]);
#pragma unroll
            for (int j = 0; j < PXL; ++j) bx[1 + j] = bv[i][j];
            bx[PXL + 1] = p3_from_right(bv[i][0]);
            const float4 q0 = wmq[i * 3], q1 = wmq[i * 3 + 1], q2 = wmq[i * 3 + 2];
            const float wv[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
            for (int r = 0; r < 3; ++r) {                   // acc[r] <-> output row br-1+r <-> kernel row ky = 2 - r
                const int ky = 2 - r;
                const float w0 = wv[ky * 3], w1 = wv[ky * 3 + 1], w2 = wv[ky * 3 + 2];
#pragma unroll
                for (int j = 0; j < PXL; ++j) {
                    acc[r][j] = fmaf(w0, bx[j], acc[r][j]);
                    acc[r][j] = fmaf(w1, bx[j + 1], acc[r][j]);
                    acc[r][j] = fmaf(w2, bx[j + 2], acc[r][j]);
                }
            }
        }
        // ---- slide the x window (row br+3, requested at the top of this iteration, enters it)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int j = 0; j < PXL + 4; ++j) xw[rr][j] = xw[rr + 1][j];
#pragma unroll
        for (int j = 0; j < PXL + 4; ++j) xw[4][j] = xn[j];
        // ---- output row y = br - 1 is complete
        const int y = br - 1;
        if (y >= ys) {
            float v[PXL];
#pragma unroll
            for (int j = 0; j < PXL; ++j) {
                v[j] = fmaf(acc[0][j], esc, esh);
                v[j] = (ep_alpha && v[j] <= 0.f) ? eal * v[j] : v[j];
            }
            if (writer) {
                float* dst = opl + (size_t)y * w + px0;
                if (PXL == 2) store_out2(dst, make_float2(v[0], v[PXL - 1]));
                else dst[0] = v[0];
                if (TRAIN) {
                    float* rp = mraw + ((size_t)n * g.P + c) * (size_t)h * w + (size_t)y * w + px0;
                    if (PXL == 2) *reinterpret_cast<float2*>(rp) = make_float2(acc[0][0], acc[0][PXL - 1]);
                    else rp[0] = acc[0][0];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PXL; ++j) { acc[0][j] = acc[1][j]; acc[1][j] = acc[2][j]; acc[2][j] = 0.f; }
    };
    constexpr int STEPS = TRAIN ? 2 : P3_STEPS;            // (the training forward holds more per row: two steps fit its registers)
#pragma unroll 1
    for (int br = ys - 1; br <= ye; br += STEPS) {
        row_step(br);
#pragma unroll
        for (int u = 1; u < STEPS; ++u)
            if (br + u <= ye) row_step(br + u);
    }
}


// ---- geometry tables
// One thread per table entry: A[ub][row -1 .. h][ky][8] (5 coefficients + 3 zeros) and G[ub][kx][tap][lane slot][PXL], lane slot s
// <-> columns (s - 1) * PXL + j: every column a lane of any column block can own, the halo lanes' and the ones right of the image
// included (p3_coeffs gives zeros outside the image).  The same p3_coeffs<T> calls with the same arguments as steps (1) and (2) of
// the kernel above, in a file compiled with the same flags: the same bits.
template <int T0, int T1, int PXL>
__global__ __launch_bounds__(256) void p3_tables_kernel(Pyr3Geom g, float* __restrict__ tab) {
    const int h = g.h, w = g.w, nslots = g.ncb * 62 + 2;
    const int na = 2 * (h + 2) * 3, ng = 2 * 3 * nslots * PXL;
    const int t = blockIdx.x * 256 + threadIdx.x;
    float acc[5];
    if (t < na) {
        const int ub = t / ((h + 2) * 3), r = t - ub * (h + 2) * 3, row = r / 3, ky = r - row * 3;
        if (ub == 0) p3_coeffs<T0>(row - 1, ky, h, g.hs[0], g.sh[0], acc);
        else p3_coeffs<T1>(row - 1, ky, h, g.hs[1], g.sh[1], acc);
        float* d = tab + (ub * (h + 2) + row) * 24 + ky * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q) d[q] = q < 5 ? acc[q] : 0.f;
    } else if (t < na + ng) {
        const int u = t - na;
        const int ub = u / (3 * nslots * PXL), r = u - ub * 3 * nslots * PXL, kx = r / (nslots * PXL), r2 = r - kx * nslots * PXL;
        const int slot = r2 / PXL, j = r2 - slot * PXL;
        if (ub == 0) p3_coeffs<T0>((slot - 1) * PXL + j, kx, w, g.ws[0], g.sw[0], acc);
        else p3_coeffs<T1>((slot - 1) * PXL + j, kx, w, g.ws[1], g.sw[1], acc);
        float* d = tab + 2 * (h + 2) * 24;
#pragma unroll
        for (int q = 0; q < 5; ++q) d[(((ub * 3 + kx) * 5 + q) * nslots + slot) * PXL + j] = acc[q];
    }
}

// What the streaming form decides from the shapes alone (pyrpool_stream_try switches on this; mspl_pyrpool_stream_plan hands it to
// callers and tests).  The part that does not depend on the batch -- the geometry a table is built for -- comes first.
struct P3Shape {
    bool ok;
    int T0, T1, PXL, ncb, CBW;
};
static P3Shape p3_shape(int h, int w, const PyrBranches& br) {
    P3Shape s;
    memset(&s, 0, sizeof(s));
    static const int off = (MSPL_TUNE_INT("MSPL_PYR_STREAM", 1) == 0);
    // maps narrower than ~half a wave leave most lanes idle: the LDS-tiled form is faster there (18x30: 12 vs 17 us)
    static const int min_w = MSPL_TUNE_INT("MSPL_PYR_STREAM_MINW", 40);
    if (off || br.nb != 5 || w < min_w || h <= 0) return s;
    // branch pattern: up, up, same, down, down (strictly), both up branches stencils of at most 5 taps
    if (!br.standard || br.taps[0] == 0 || br.taps[1] == 0) return s;
    s.T0 = br.taps[0]; s.T1 = br.taps[1];
    s.PXL = w <= 62 ? 1 : 2;
    if (s.PXL == 2 && (w & 1)) return s;                   // 8-byte stores and x row loads
    s.CBW = 62 * s.PXL;
    s.ncb = ceil_div(w, s.CBW);
    s.ok = true;
    return s;
}

struct P3Plan {
    bool taken;
    P3Shape s;
    int seg_tab, nseg_tab, seg_ik, nseg_ik;                // rows per segment and segments per plane: tables from memory / in-kernel tables
    int64_t waves_tab, waves_ik;
};
static P3Plan p3_plan(int N, int P, int h, int w, const PyrBranches& br) {
    P3Plan p;
    memset(&p, 0, sizeof(p));
    if (N <= 0 || P <= 0 || ((int64_t)N * P) % 4 != 0) return p;
    p.s = p3_shape(h, w, br);
    if (!p.s.ok) return p;
    const int64_t cols = (int64_t)N * P * p.s.ncb;         // waves per row segment
    static const int dbg_seg = MSPL_TUNE_INT("MSPL_PYR_SEG", 0);
    // in-kernel tables: enough waves to put >= 2 on every SIMD when the maps allow, halo rows (2 of SEG + 2 branch rows, 6 of
    // SEG + 6 x rows) kept small otherwise
    int seg = std::min(h, P3_SEGMAX);
    while (seg > 6 && cols * ceil_div(h, seg) < 2048) --seg;
    seg = ceil_div(h, ceil_div(h, seg));
    if (dbg_seg > 0 && dbg_seg <= P3_SEGMAX) seg = std::min(dbg_seg, h);
    p.seg_ik = seg; p.nseg_ik = ceil_div(h, seg); p.waves_ik = cols * p.nseg_ik;
    // tables from memory: DESIGN 4i holds the sweep this rule comes from
    static const int min_waves = MSPL_TUNE_INT("MSPL_PYR_TAB_WAVES", 2048);
    static const int seg_cap = std::min(std::max(MSPL_TUNE_INT("MSPL_PYR_TAB_SEGCAP", P3_TAB_SEGMAX), 1), P3_TAB_SEGMAX);
    seg = std::min(h, seg_cap);
    while (seg > 6 && cols * ceil_div(h, seg) < min_waves) --seg;
    seg = ceil_div(h, ceil_div(h, seg));
    if (dbg_seg > 0 && dbg_seg <= P3_TAB_SEGMAX) seg = std::min(dbg_seg, h);
    p.seg_tab = seg; p.nseg_tab = ceil_div(h, seg); p.waves_tab = cols * p.nseg_tab;
    p.taken = p.waves_ik < (1ll << 31) && p.waves_tab < (1ll << 31);
    return p;
}

static size_t p3_table_floats(const P3Shape& s, int h) { return (size_t)2 * (h + 2) * 24 + (size_t)30 * (s.ncb * 62 + 2) * s.PXL; }

static void p3_fill_geom(Pyr3Geom& g, const P3Shape& s, int N, int P, int h, int w, const int32_t* hs, const int32_t* ws,
                         const PyrBranches& br) {
    memset(&g, 0, sizeof(g));
    g.N = N; g.P = P; g.h = h; g.w = w;
    for (int i = 0; i < 5; ++i) {
        g.hs[i] = hs[i]; g.ws[i] = ws[i];
        if (i != 2) { g.sh[i] = br.sh[i]; g.sw[i] = br.sw[i]; }
    }
    g.CBW = s.CBW;
    g.ncb = s.ncb;
}

// Which geometry the table at an address was built for: the builder notes it, the launcher compares.  (The table itself lives in
// device memory, which the launcher cannot read without a synchronisation.)
struct P3TabKey {
    int v[9];                                              // h, w, hs0, ws0, hs1, ws1, T0, T1, PXL
    bool operator==(const P3TabKey& o) const { return memcmp(v, o.v, sizeof(v)) == 0; }
};
static P3TabKey p3_tab_key(const P3Shape& s, int h, int w, const int32_t* hs, const int32_t* ws) {
    P3TabKey k = {{h, w, hs[0], ws[0], hs[1], ws[1], s.T0, s.T1, s.PXL}};
    return k;
}
static std::mutex p3_tab_mutex;
static std::unordered_map<const void*, P3TabKey>& p3_tab_registry() {
    static std::unordered_map<const void*, P3TabKey> m;
    return m;
}

int pyrpool_stream_tables_build(int h, int w, int nb, const int32_t* hs, const int32_t* ws, float* tab, int64_t bytes,
                                hipStream_t stream) {
    const PyrBranches br = pyr_classify(h, w, nb, hs, ws);
    const P3Shape s = p3_shape(h, w, br);
    MSPL_REQUIRE(s.ok, MSPL_ERR_UNSUPPORTED, "pyr_stream_tables: the streaming form does not cover a %dx%d map with these branches", h, w);
    MSPL_REQUIRE(bytes == (int64_t)(p3_table_floats(s, h) * sizeof(float)), MSPL_ERR_BAD_SHAPE,
                 "pyr_stream_tables: %lld bytes given, the geometry takes %zu", (long long)bytes, p3_table_floats(s, h) * sizeof(float));
    MSPL_REQUIRE((((uintptr_t)tab) & 15) == 0, MSPL_ERR_BAD_SHAPE, "pyr_stream_tables: the table must be 16-byte aligned");
    Pyr3Geom g;
    p3_fill_geom(g, s, 0, 0, h, w, hs, ws, br);
    const int entries = 2 * (h + 2) * 3 + 2 * 3 * (s.ncb * 62 + 2) * s.PXL;
    const dim3 grid((unsigned)ceil_div(entries, 256)), blk(256);
#define MSPL_P3_TABLES(A, B, L) hipLaunchKernelGGL((p3_tables_kernel<A, B, L>), grid, blk, 0, stream, g, tab)
    if (s.PXL == 1) MSPL_PYR_TAP_DISPATCH(s.T0, s.T1, MSPL_P3_TABLES, 1);
    else MSPL_PYR_TAP_DISPATCH(s.T0, s.T1, MSPL_P3_TABLES, 2);
#undef MSPL_P3_TABLES
    MSPL_CHECK_LAUNCH("pyr_stream_tables");
    std::lock_guard<std::mutex> lock(p3_tab_mutex);
    p3_tab_registry()[tab] = p3_tab_key(s, h, w, hs, ws);
    return MSPL_OK;
}

int64_t pyrpool_stream_tables_bytes(int h, int w, int nb, const int32_t* hs, const int32_t* ws) {
    const P3Shape s = p3_shape(h, w, pyr_classify(h, w, nb, hs, ws));
    return s.ok ? (int64_t)(p3_table_floats(s, h) * sizeof(float)) : 0;
}

void pyrpool_stream_plan(int N, int P, int h, int w, int nb, const int32_t* hs, const int32_t* ws, int32_t* out) {
    const P3Plan p = p3_plan(N, P, h, w, pyr_classify(h, w, nb, hs, ws));
    for (int i = 0; i < MSPL_PYR_STREAM_PLAN_LEN; ++i) out[i] = 0;
    if (!p.taken) return;
    out[MSPL_PYR_STREAM_PLAN_TAKEN] = 1;
    out[MSPL_PYR_STREAM_PLAN_T0] = p.s.T0; out[MSPL_PYR_STREAM_PLAN_T1] = p.s.T1;
    out[MSPL_PYR_STREAM_PLAN_PXL] = p.s.PXL; out[MSPL_PYR_STREAM_PLAN_NCB] = p.s.ncb; out[MSPL_PYR_STREAM_PLAN_CBW] = p.s.CBW;
    out[MSPL_PYR_STREAM_PLAN_SEG] = p.seg_tab; out[MSPL_PYR_STREAM_PLAN_NSEG] = p.nseg_tab;
    out[MSPL_PYR_STREAM_PLAN_WAVES] = (int32_t)p.waves_tab;
    out[MSPL_PYR_STREAM_PLAN_SEG_INKERNEL] = p.seg_ik; out[MSPL_PYR_STREAM_PLAN_NSEG_INKERNEL] = p.nseg_ik;
    out[MSPL_PYR_STREAM_PLAN_WAVES_INKERNEL] = (int32_t)p.waves_ik;
}

// Returns MSPL_OK when launched, 1 when the shape is left to the LDS-tiled kernels, < 0 on error.  a.tab: geometry tables of
// pyrpool_stream_tables_build, or null for the in-kernel tables; a table of another geometry is an error, nothing is launched.
int pyrpool_stream_try(const PyrFwdArgs& a) {
    const int N = a.N, P = a.P, h = a.h, w = a.w;
    const int32_t* hs = a.hs;  const int32_t* ws = a.ws;
    const float* x = a.x;  const float* const* stage_w = a.stage_w;  const float* const* down_e = a.down_e;
    float* out = a.out;  float* zcat = a.zcat;  const float* tab = a.tab;
    const Epi& e = a.e;
    const P3Plan plan = p3_plan(N, P, h, w, a.br);
    if (!plan.taken) return 1;
    const P3Shape& s = plan.s;
    if (tab) {
        MSPL_REQUIRE(!zcat, MSPL_ERR_UNSUPPORTED, "pyrpool_fused(streaming form): the training forward takes no geometry tables");
        bool known = false;
        P3TabKey have;
        {
            std::lock_guard<std::mutex> lock(p3_tab_mutex);
            auto it = p3_tab_registry().find(tab);
            if (it != p3_tab_registry().end()) { known = true; have = it->second; }
        }
        MSPL_REQUIRE(known, MSPL_ERR_BAD_SHAPE, "pyrpool_fused(streaming form): no geometry tables were built at %p", (const void*)tab);
        MSPL_REQUIRE(have == p3_tab_key(s, h, w, hs, ws), MSPL_ERR_BAD_SHAPE,
                     "pyrpool_fused(streaming form): the tables were built for a %dx%d map (up branches %dx%d, %dx%d), this is %dx%d "
                     "(%dx%d, %dx%d)", have.v[0], have.v[1], have.v[2], have.v[3], have.v[4], have.v[5], h, w, hs[0], ws[0], hs[1], ws[1]);
    }
    if (e.pre_add || e.residual || e.reinf_r || e.gate) return 1;    // only the scale/shift/PReLU epilogue
    if (!stage_w[0] || !stage_w[1] || !stage_w[2] || !down_e[3] || !down_e[4]) return 1;
    const int PXL = s.PXL;
    if (PXL == 2 && ((((uintptr_t)out) & 7) || (((uintptr_t)x) & 7))) return 1;     // 8-byte stores and x row loads
    if (zcat && (!e.raw || e.ctot != P || e.coff != 0)) return 1;      // training forward: un-sliced destination + raw output
    if (zcat && PXL == 2 && ((((uintptr_t)zcat) | ((uintptr_t)e.raw)) & 7)) return 1;
    Pyr3Geom g;
    p3_fill_geom(g, s, N, P, h, w, hs, ws, a.br);
    g.SEG = tab ? plan.seg_tab : plan.seg_ik;
    g.nseg = tab ? plan.nseg_tab : plan.nseg_ik;
    const int64_t waves = tab ? plan.waves_tab : plan.waves_ik;
    g.total = (unsigned)waves;
    const dim3 grid((unsigned)(waves / 4)), blk(256);          // workgroup = 4 consecutive planes of one (column block, segment)
#define MSPL_P3_ARGS x, stage_w[0], stage_w[1], stage_w[2], down_e[3], down_e[4], a.br_scale, a.br_shift, a.br_alpha, a.merge_w, e.scale, e.shift, e.alpha, e.ctot, e.coff, g, out
#define MSPL_P3_LAUNCH(A, B, L) do { \
        if (zcat) hipLaunchKernelGGL((pyrpool_stream_kernel<A, B, L, true, false>), grid, blk, 0, a.stream, MSPL_P3_ARGS, zcat, e.raw, (const float*)nullptr); \
        else if (tab) hipLaunchKernelGGL((pyrpool_stream_kernel<A, B, L, false, true>), grid, blk, 0, a.stream, MSPL_P3_ARGS, (float*)nullptr, (float*)nullptr, tab); \
        else hipLaunchKernelGGL((pyrpool_stream_kernel<A, B, L, false, false>), grid, blk, 0, a.stream, MSPL_P3_ARGS, (float*)nullptr, (float*)nullptr, (const float*)nullptr); } while (0)
    if (PXL == 1) MSPL_PYR_TAP_DISPATCH(s.T0, s.T1, MSPL_P3_LAUNCH, 1);
    else MSPL_PYR_TAP_DISPATCH(s.T0, s.T1, MSPL_P3_LAUNCH, 2);
#undef MSPL_P3_LAUNCH
#undef MSPL_P3_ARGS
    MSPL_CHECK_LAUNCH("pyrpool_fused(streaming form)");
    return MSPL_OK;
}

}  // namespace mspl
