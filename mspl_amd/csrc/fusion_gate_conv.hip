// The trainable RGB-D fusion gate as one node (nn_layers/fusion_gate.py:27-41):
//     z = W[:, :C] . rgb + W[:, C:] . depth,   g = sigmoid(z),   out = rgb * g + depth * (1 - g)
// forward in ONE launch, and the weight gradient of its 1x1 convolution with both column halves from one read of gz.
//
// Forward.  The product is C[M x P] = W[M x 2C] . [rgb; depth][2C x P] with M = C; pixels are contiguous in NCHW.  It runs as in
// conv1x1.hip's LDS-ring form: v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain), a wave owns 128 consecutive pixels of the
// flattened (image, pixel) axis and one 32-row chunk, lane (half, li) loads ONE float4 X[k + half][4 li .. 4 li + 3] per k-step and
// uses its components as the B operand of four MFMAs, so the accumulators of a row are 4 consecutive pixels = one 16-byte store.
// The two sources are two K = C passes over ONE accumulator set: the workgroup stages W[rows, :C] in LDS (odd row stride), walks
// rgb, re-stages W[rows, C:], walks depth.  The weight tile is rows x C -- 64 x 257 or 32 x 513 floats at the most, what the 1x1
// kernel stages at K = 512 -- and K = 2C = 1024 needs no form of its own.  The first B groups of a pass are requested before the
// staging, so their latency hides under it and the barrier.
// The blend needs rgb[m][p] and depth[m][p] for the rows the workgroup owns: rows of the very pixel columns its waves (or the
// sibling workgroups of the same pixel group, which are neighbours in the grid) have just read as B operands.  They are read again
// in the epilogue, after the lines have just been used.  What the L2s actually fetch is in DESIGN 7f (counters): the row blocks of one
// pixel group sit on different XCDs, each with its own L2, so the B rows are fetched several times -- 4.5x the two inputs at C = 512.
// Planes that are no multiple of 4 pixels take a scalar form (one thread per element) up to 4096 pixels per batch; see below.
#include <algorithm>
#include <mutex>

#include "common.hpp"

namespace mspl {

typedef float fgx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float fg_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }      // fusion.hip's

struct FgGeom {
    int N, C, HW;
    int KS;        // LDS row stride of the weight tile (odd)
    int MB;        // output rows per workgroup (32 | 64)
    int WM;        // waves along the rows (MB / 32); 4 / WM waves along the pixels
    int mblocks;   // C / MB
    int ptiles;    // 128-pixel tiles of the flattened batch
    int pgroups;   // ceil(ptiles / (4 / WM))
};

constexpr int FG_RING = 4;      // B groups (8 k-values each) in flight per wave

__global__ __launch_bounds__(256, 2) void fusion_gate_conv_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                                  const float* __restrict__ w, FgGeom g, float* __restrict__ z,
                                                                  float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float At[];            // [MB][KS]
    // sibling row blocks of one pixel group are neighbours in the grid, so they run at about the same time
    const int mb = blockIdx.x % g.mblocks, pg = blockIdx.x / g.mblocks;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int WP = 4 / g.WM;
    const int chunk = wave % g.WM, wp = wave / g.WM;
    const int li = lane & 31, half = lane >> 5;
    const int m0 = mb * g.MB;
    const int ptile = pg * WP + wp;
    const bool active = ptile < g.ptiles;                                 // wave-uniform; inactive waves still stage and meet the barriers
    const int total_px = g.N * g.HW;
    const int gp = (ptile * 32 + li) * 4;                                 // first of this lane's 4 pixels (HW % 4 == 0: one image)
    const bool pok = active && gp < total_px;
    const int gpc = pok ? gp : 0;
    const int img = gpc / g.HW, p = gpc - img * g.HW;
    const size_t plane = (size_t)g.HW;
    const float* arow0 = At + (size_t)(chunk * 32 + li) * g.KS + half;

    fgx16 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
    float4 b[FG_RING][4];

#pragma unroll 1
    for (int src = 0; src < 2; ++src) {
        // X[img][k + half][p .. p + 3]; k advances by whole planes
        const float* xb = (src ? depth : rgb) + ((size_t)img * g.C + half) * plane + p;
        auto load_group = [&](float4 (&bb)[4], int kb) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) bb[kk] = *reinterpret_cast<const float4*>(xb + (size_t)(kb + 2 * kk) * plane);
        };
        if (active) {
#pragma unroll
            for (int i = 0; i < FG_RING; ++i) load_group(b[i], 8 * i);    // C >= 32 = 8 * FG_RING
        }
        if (src) __syncthreads();                                         // every wave has left the first pass: the tile may go
        {
            const int kv = g.C >> 2, total = g.MB * kv;
            const float* wg = w + (size_t)m0 * 2 * g.C + (size_t)src * g.C;
#pragma unroll 4
            for (int i = tid; i < total; i += 256) {
                const int m = i / kv, k = (i - m * kv) << 2;
                const float4 v = *reinterpret_cast<const float4*>(wg + (size_t)m * 2 * g.C + k);
                float* d = At + m * g.KS + k;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll 1
            for (int kb0 = 0; kb0 < g.C; kb0 += 8 * FG_RING) {            // C % 32 == 0: every slot of the ring is a whole group
#pragma unroll
                for (int i = 0; i < FG_RING; ++i) {
                    const int kb = kb0 + 8 * i;
                    const float* arow = arow0 + kb;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const float a = arow[2 * kk];
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[i][kk].x, acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[i][kk].y, acc[1], 0, 0, 0);
                        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[i][kk].z, acc[2], 0, 0, 0);
                        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[i][kk].w, acc[3], 0, 0, 0);
                    }
                    if (kb + 8 * FG_RING < g.C) load_group(b[i], kb + 8 * FG_RING);      // uniform
                }
            }
        }
    }
    if (!pok) return;                                                     // (no barrier follows)

    // ---- epilogue.  Sub-tile s, register r: row = (r & 3) + 8 * (r >> 2) + 4 * half, pixel gp + s.
    const size_t base = ((size_t)img * g.C + m0 + chunk * 32 + 4 * half) * plane + p;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = rg * 4 + q;
            const size_t off = base + (size_t)(q + 8 * rg) * plane;
            const float4 rv = *reinterpret_cast<const float4*>(rgb + off);
            const float4 dv = *reinterpret_cast<const float4*>(depth + off);
            const float zz[4] = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
            if (z) store_out4(z + off, make_float4(zz[0], zz[1], zz[2], zz[3]));
            const float g0 = fg_sigmoid(zz[0]), g1 = fg_sigmoid(zz[1]), g2 = fg_sigmoid(zz[2]), g3 = fg_sigmoid(zz[3]);
            float4 o;
            o.x = rv.x * g0 + dv.x * (1.0f - g0);
            o.y = rv.y * g1 + dv.y * (1.0f - g1);
            o.z = rv.z * g2 + dv.z * (1.0f - g2);
            o.w = rv.w * g3 + dv.w * (1.0f - g3);
            store_out4(out + off, o);
        }
        asm volatile("" ::: "memory");   // one row quad at a time: keeps hipcc from hoisting all 16 rows' work
    }
}

// ------------------------------------------------------------------ scalar form (small planes that are no multiple of 4 pixels)
// Level 4 of a 32x48 input has 6 pixels per plane: nothing to tile.  One thread per output element walks k = 0 .. 2C-1 in order with
// fmaf -- the chain the matrix cores run -- so the two forms agree on z wherever both could run.  Threads of a wave share the weight row
// (a broadcast load) and read consecutive pixels.  Bounded to N * HW <= FG_SCALAR_MAX_PX pixels: beyond that the node declines.
constexpr int FG_SCALAR_MAX_PX = 4096;

__global__ __launch_bounds__(256) void fusion_gate_conv_scalar_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                                      const float* __restrict__ w, int N, int C, int HW,
                                                                      float* __restrict__ z, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;                          // (n, m, p) flattened: the output's own offset
    if (i >= N * C * HW) return;
    const int p = i % HW, m = (i / HW) % C, n = i / (HW * C);
    const float* wr = w + (size_t)m * 2 * C;
    const float* xr = rgb + (size_t)n * C * HW + p;
    const float* xd = depth + (size_t)n * C * HW + p;
    float acc = 0.f;
    for (int k = 0; k < C; ++k) acc = fmaf(wr[k], xr[(size_t)k * HW], acc);
    for (int k = 0; k < C; ++k) acc = fmaf(wr[C + k], xd[(size_t)k * HW], acc);
    if (z) z[i] = acc;
    const float g = fg_sigmoid(acc);
    out[i] = rgb[i] * g + depth[i] * (1.0f - g);
}

// gw[m, s*C + k] (+)= sum_{n,p} gz[n, m, p] * src_s[n, k, p]: one thread per element of gw, the whole range in order (no atomics
// among the threads of this launch; accumulate adds to the shared buffer with one atomic per element).
__global__ __launch_bounds__(256) void fusion_gate_conv_wgrad_scalar_kernel(const float* __restrict__ gz, const float* __restrict__ rgb,
                                                                            const float* __restrict__ depth, int N, int C, int HW,
                                                                            int accumulate, float* __restrict__ gw) {
    const int i = blockIdx.x * 256 + threadIdx.x;                          // (m, s, k) flattened: gw's own offset
    if (i >= 2 * C * C) return;
    const int k = i % C, s = (i / C) & 1, m = i / (2 * C);
    const float* x = s ? depth : rgb;
    // two-level sum: blocks of 64 products, then the blocks -- 64 + 64 roundings at the limit of 4096 pixels instead of 4096 in a row
    // (one chain measured 5.8x the float32 ATen reference's error against float64 on 2048 x 2 pixels)
    float acc = 0.f, part = 0.f;
    int cnt = 0;
    for (int n = 0; n < N; ++n) {
        const float* a = gz + ((size_t)n * C + m) * HW;
        const float* b = x + ((size_t)n * C + k) * HW;
        for (int p = 0; p < HW; ++p) {
            part = fmaf(a[p], b[p], part);
            if (++cnt == 64) { acc += part; part = 0.f; cnt = 0; }
        }
    }
    acc += part;
    if (accumulate) atomicAdd(gw + i, acc);
    else gw[i] = acc;
}

struct FgPlan {
    FgGeom g;
    size_t lds;
    unsigned grid;
    int form;      // an mspl_fusion_gate_conv_form_t
};

// Which form serves a shape, 0 for none: the one predicate behind mspl_fusion_gate_conv_fits, the two launchers and the two plans.
static int fg_form(int N, int C, int HW) {
    if (N <= 0 || C < 32 || C > 512 || (C & 31) != 0 || HW <= 0 || (int64_t)N * C * HW >= (1ll << 30)) return 0;
    if ((HW & 3) == 0) return MSPL_FGC_FORM_MFMA_X4;
    return (int64_t)N * HW <= FG_SCALAR_MAX_PX ? MSPL_FGC_FORM_SCALAR : 0;
}

// The one place the forward launch is decided.  Host only, no device call, no state.
static int fg_decide(int N, int C, int HW, FgPlan& p) {
    MSPL_REQUIRE(N > 0 && C > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "fusion_gate_conv: bad shape N=%d C=%d HW=%d", N, C, HW);
    const int form = fg_form(N, C, HW);
    MSPL_REQUIRE(form != 0, MSPL_ERR_UNSUPPORTED,
                 "fusion_gate_conv: N=%d C=%d HW=%d is not served (C %% 32 == 0, 32 <= C <= 512, HW %% 4 == 0 or N*HW <= %d)", N, C, HW,
                 FG_SCALAR_MAX_PX);
    memset(&p, 0, sizeof(p));
    p.form = form;
    FgGeom& g = p.g;
    g.N = N; g.C = C; g.HW = HW;
    if (form == MSPL_FGC_FORM_SCALAR) {
        p.grid = (unsigned)ceil_div(N * C * HW, 256);    // <= 4096 * 512 / 256
        return MSPL_OK;
    }
    g.KS = C | 1;
    g.MB = ((C & 63) == 0 && C <= 256) ? 64 : 32;        // 64 x 257 and 32 x 513 floats: the 1x1 kernel's tile at K = 512
    g.WM = g.MB / 32;
    g.mblocks = C / g.MB;
    g.ptiles = (int)ceil_div64((int64_t)N * HW, 128);
    g.pgroups = ceil_div(g.ptiles, 4 / g.WM);
    p.lds = (size_t)g.MB * g.KS * sizeof(float);
    p.grid = (unsigned)(g.mblocks * g.pgroups);          // < 2^30 / 128 * 16
    return MSPL_OK;
}

// ------------------------------------------------------------------ weight gradient
// gw[m, k] (+)= sum_{n,p} gz[n, m, p] * rgb[n, k, p],   gw[m, C + k] (+)= sum_{n,p} gz[n, m, p] * depth[n, k, p]
// The fragment-load tile of conv1x1_wgrad.hip with two B operands: lane (r, h) loads the 16 bytes at pixel p0 + 4h of row r of gz,
// rgb and depth; element j of the three float4 feeds one MFMA into the rgb tile and one into the depth tile.  gz is read once.
struct FgWg {
    int N, C, P;
    int tc;          // 32-tiles along C (rows and columns alike)
    int gpi;         // 64-pixel groups per image
    int ngroups;     // N * gpi
    int nslots;      // waves per tile pair (multiple of 4)
};

__global__ __launch_bounds__(256) void fusion_gate_conv_wgrad_kernel(const float* __restrict__ gz, const float* __restrict__ rgb,
                                                                     const float* __restrict__ depth, FgWg g, float* __restrict__ gw) {
    __shared__ float red[4][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int bslots = g.nslots >> 2;
    const int tile = blockIdx.x / bslots;
    const int slot = (blockIdx.x - tile * bslots) * 4 + wave;
    const int m0 = (tile / g.tc) * 32, k0 = (tile % g.tc) * 32;          // C % 32 == 0: every row and column is inside
    const size_t P = (size_t)g.P, img = (size_t)g.C * P;
    const float* ap0 = gz + (size_t)(m0 + r) * P;
    const float* bp0 = rgb + (size_t)(k0 + r) * P;
    const float* dp0 = depth + (size_t)(k0 + r) * P;
    fgx16 accr, accd;
#pragma unroll
    for (int i = 0; i < 16; ++i) { accr[i] = 0.f; accd[i] = 0.f; }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = slot; q < g.ngroups; q += g.nslots) {                   // wave-uniform
        const int n = q / g.gpi, p0 = (q - n * g.gpi) * 64;
        float4 a[8], b[8], d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int pc = min(p0 + 8 * i + 4 * h, g.P - 4);             // clamped: P % 4 == 0, a float4 is inside or outside the plane
            a[i] = *reinterpret_cast<const float4*>(ap0 + n * img + pc);
            b[i] = *reinterpret_cast<const float4*>(bp0 + n * img + pc);
            d[i] = *reinterpret_cast<const float4*>(dp0 + n * img + pc);
        }
        __builtin_amdgcn_sched_barrier(0);                               // all requests leave before the first MFMA
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (p0 + 8 * i + 4 * h >= g.P) { a[i] = zero; b[i] = zero; d[i] = zero; }
            accr = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[i].x, accr, 0, 0, 0);
            accd = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, d[i].x, accd, 0, 0, 0);
            accr = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[i].y, accr, 0, 0, 0);
            accd = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, d[i].y, accd, 0, 0, 0);
            accr = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[i].z, accr, 0, 0, 0);
            accd = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, d[i].z, accd, 0, 0, 0);
            accr = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[i].w, accr, 0, 0, 0);
            accd = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, d[i].w, accd, 0, 0, 0);
        }
    }
    // the four waves hold four slices of the same two tiles: summed through LDS, one atomic per element and workgroup
#pragma unroll 1
    for (int srcw = 0; srcw < 2; ++srcw) {
        if (srcw) __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) red[wave][i][lane] = srcw ? accd[i] : accr[i];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = threadIdx.x + 256 * j;
            const int i = e >> 6, l = e & 63;
            const float v = (red[0][i][l] + red[1][i][l]) + (red[2][i][l] + red[3][i][l]);
            const int row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), col = l & 31;
            atomicAdd(gw + (size_t)(m0 + row) * 2 * g.C + (size_t)srcw * g.C + k0 + col, v);
        }
    }
}

// The one place the weight-gradient launch is decided.
static int fg_wgrad_decide(int N, int C, int HW, FgWg& g, unsigned& grid) {
    MSPL_REQUIRE(N > 0 && C > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "fusion_gate_conv_bwd_weight: bad shape N=%d C=%d HW=%d", N, C, HW);
    const int form = fg_form(N, C, HW);
    MSPL_REQUIRE(form != 0, MSPL_ERR_UNSUPPORTED,
                 "fusion_gate_conv_bwd_weight: N=%d C=%d HW=%d is not served (C %% 32 == 0, 32 <= C <= 512, HW %% 4 == 0 or N*HW <= %d)",
                 N, C, HW, FG_SCALAR_MAX_PX);
    memset(&g, 0, sizeof(g));
    g.N = N; g.C = C; g.P = HW;
    if (form == MSPL_FGC_FORM_SCALAR) {
        g.nslots = 0;                                    // (the scalar form: one thread per element of gw)
        grid = (unsigned)ceil_div(2 * C * C, 256);
        return MSPL_OK;
    }
    g.tc = C / 32;
    const int tiles = g.tc * g.tc;
    g.gpi = ceil_div(HW, 64);
    g.ngroups = N * g.gpi;
    // waves per tile pair: ~3 waves on every SIMD of the chip, at least one workgroup, never more waves than 64-pixel groups
    int ns = ceil_div(3072, tiles);
    if (ns > g.ngroups) ns = g.ngroups;
    if (ns < 4) ns = 4;
    g.nslots = (ns + 3) & ~3;
    grid = (unsigned)(tiles * (g.nslots >> 2));          // <= 256 * 768
    return MSPL_OK;
}

static bool fg_aligned16(const void* a, const void* b, const void* c, const void* d, const void* e) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_fusion_gate_conv_fits(int32_t N, int32_t C, int32_t HW) { return fg_form(N, C, HW) != 0 ? 1 : 0; }

extern "C" int mspl_fusion_gate_conv_fwd(const float* rgb, const float* depth, const float* w, int32_t N, int32_t C, int32_t HW,
                                         float* z, float* out, void* stream) {
    MSPL_REQUIRE(rgb && depth && w && out, MSPL_ERR_NULL_POINTER, "fusion_gate_conv: null pointer");
    FgPlan p;
    if (int rc = fg_decide(N, C, HW, p)) return rc;
    if (p.form == MSPL_FGC_FORM_SCALAR) {
        hipLaunchKernelGGL(fusion_gate_conv_scalar_kernel, dim3(p.grid), dim3(256), 0, (hipStream_t)stream, rgb, depth, w, N, C, HW, z, out);
        MSPL_CHECK_LAUNCH("fusion_gate_conv(scalar)");
        return MSPL_OK;
    }
    MSPL_REQUIRE(fg_aligned16(rgb, depth, w, z, out), MSPL_ERR_UNSUPPORTED, "fusion_gate_conv: operands must be 16-byte aligned");
    static std::once_flag attr_once;  // dynamic LDS above 64 KiB needs the opt-in (once per process, thread-safe)
    std::call_once(attr_once, [] {
        (void)hipFuncSetAttribute((const void*)fusion_gate_conv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
        (void)hipGetLastError();
    });
    hipLaunchKernelGGL(fusion_gate_conv_kernel, dim3(p.grid), dim3(256), p.lds, (hipStream_t)stream, rgb, depth, w, p.g, z, out);
    MSPL_CHECK_LAUNCH("fusion_gate_conv");
    return MSPL_OK;
}

extern "C" int mspl_fusion_gate_conv_plan(int32_t N, int32_t C, int32_t HW, int32_t* out) {
    MSPL_REQUIRE(out, MSPL_ERR_NULL_POINTER, "fusion_gate_conv_plan: null out");
    for (int i = 0; i < MSPL_FGC_PLAN_LEN; ++i) out[i] = 0;
    FgPlan p;
    if (int rc = fg_decide(N, C, HW, p)) return rc;
    out[MSPL_FGC_PLAN_FORM] = p.form;
    out[MSPL_FGC_PLAN_GRID_X] = (int32_t)p.grid;
    if (p.form == MSPL_FGC_FORM_SCALAR) return MSPL_OK;              // (one output element per thread: no tile to report)
    out[MSPL_FGC_PLAN_ROWS] = p.g.MB;
    out[MSPL_FGC_PLAN_PIXELS] = 128 * (4 / p.g.WM);
    out[MSPL_FGC_PLAN_WAVE_PIXELS] = 128;
    out[MSPL_FGC_PLAN_LDS_BYTES] = (int32_t)p.lds;
    out[MSPL_FGC_PLAN_GRID_X] = (int32_t)p.grid;
    return MSPL_OK;
}

extern "C" int mspl_fusion_gate_conv_bwd_weight(const float* gz, const float* rgb, const float* depth, int32_t N, int32_t C,
                                                int32_t HW, int32_t accumulate, float* gw, void* stream) {
    MSPL_REQUIRE(gz && rgb && depth && gw, MSPL_ERR_NULL_POINTER, "fusion_gate_conv_bwd_weight: null pointer");
    FgWg g;
    unsigned grid;
    if (int rc = fg_wgrad_decide(N, C, HW, g, grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (g.nslots == 0) {
        hipLaunchKernelGGL(fusion_gate_conv_wgrad_scalar_kernel, dim3(grid), dim3(256), 0, s, gz, rgb, depth, N, C, HW, accumulate, gw);
        MSPL_CHECK_LAUNCH("fusion_gate_conv_bwd_weight(scalar)");
        return MSPL_OK;
    }
    MSPL_REQUIRE(fg_aligned16(gz, rgb, depth, nullptr, nullptr), MSPL_ERR_UNSUPPORTED,
                 "fusion_gate_conv_bwd_weight: operands must be 16-byte aligned");
    if (!accumulate) {
        const hipError_t e = hipMemsetAsync(gw, 0, (size_t)2 * C * C * sizeof(float), s);      // async memset node: graph-capturable
        MSPL_REQUIRE(e == hipSuccess, MSPL_ERR_HIP, "fusion_gate_conv_bwd_weight: hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(fusion_gate_conv_wgrad_kernel, dim3(grid), dim3(256), 0, s, gz, rgb, depth, g, gw);
    MSPL_CHECK_LAUNCH("fusion_gate_conv_bwd_weight");
    return MSPL_OK;
}

extern "C" int mspl_fusion_gate_conv_bwd_weight_plan(int32_t N, int32_t C, int32_t HW, int32_t* form, int32_t* parts,
                                                     int32_t* ngroups) {
    MSPL_REQUIRE(form && parts, MSPL_ERR_NULL_POINTER, "fusion_gate_conv_bwd_weight_plan: null out");
    *form = 0; *parts = 0;
    if (ngroups) *ngroups = 0;
    FgWg g;
    unsigned grid;
    if (int rc = fg_wgrad_decide(N, C, HW, g, grid)) return rc;
    if (g.nslots == 0) {
        *form = MSPL_FGC_WGRAD_SCALAR;
        *parts = 1;
        return MSPL_OK;
    }
    *form = MSPL_FGC_WGRAD_MFMA_PAIR;
    *parts = g.nslots;
    if (ngroups) *ngroups = g.ngroups;
    return MSPL_OK;
}
