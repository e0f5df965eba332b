// Weight (and bias) gradient of K13's dense 1x1 / dilated 3x3 convolution on the fp32 matrix cores: what Conv2d autograd gives for
// nn_layers/aspp.py:40-51 / :87-98 when the ASPP heads train.
//
//     dWp[tap][co][ci] = sum over (n, y, x) of gy[n][co][y][x] * x[n][ci][y + dy(tap)][x + dx(tap)]      (zero outside the image)
//     db[co]           = sum over (n, y, x) of gy[n][co][y][x]
//
// in the packed (taps, Cout, Cin) layout of ops.pack_dense_weight.  Implicit GEMM per tap: M = Cout, N = Cin, K = N*H*W, on
// v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain).  Workgroup tile: 128 output channels x 64 input channels of one
// tap; a wave owns 32 x 64 = two accumulator tiles; K runs over chunks of 32 consecutive pixels of the flattened (image, y, x)
// axis.  BOTH operands are contiguous along K in memory, the opposite of what the matrix instruction wants (one k per lane
// half, rows along the lanes), so both go through LDS as [row][k] images with a row stride of 33 floats: the loader writes 32
// consecutive pixels of one row from 32 lanes (consecutive banks), the matrix read takes one k of 32 rows (rows 33 floats apart:
// 32 different banks).  The shifted operand has no alignment guarantee, so it is fetched one dword per lane, as in the forward.
// The next chunk is fetched into registers while the current one is multiplied from LDS.
//
// Work that does not exist is skipped: a tap whose shift leaves the image for every pixel (dilation >= H or >= W in that tap's
// direction) gets an exact 0.0f and no K loop, and for the other off-centre rows of taps the loop jumps over the pixel chunks
// whose rows all fall outside (dilation 18 on a 32-row map: 18 of 32 rows).
//
// The pixel axis is split into `split` ranges (the 1x1 convolutions, Cin = 512 and conv_1x1_3 have far fewer tiles than the chip
// has CUs, and even the bottleneck 3x3's 576 tiles quantise badly on 256 CUs); each range writes its partial tile to the caller's
// workspace and a second launch adds the partials in range order.  No floating-point atomics anywhere: the same inputs give the
// same bits.  The bias gradient is taken from the A operand registers of the centre tap's first column of tiles (gy is never
// read a second time for it).
#include "common.hpp"

namespace mspl {

typedef float floatx16w __attribute__((ext_vector_type(16)));

constexpr int DW_BM = 128, DW_BN = 64, DW_KC = 32;
constexpr int DW_LS = DW_KC + 1;            // LDS row stride (floats) of both operand images
constexpr int DW_MAX_SPLIT = 64;

struct DenseWgradGeom {
    int N, Cin, Cout, H, W, taps, dil;
    int mblocks, nblocks, split;
    int nch;                                // chunks of 32 pixels over N*H*W
    unsigned dead;                          // bit t: tap t's shift leaves the image everywhere
};

__global__ __launch_bounds__(256, 2) void dense_conv_wgrad_kernel(const float* __restrict__ gy, const float* __restrict__ x, DenseWgradGeom g,
                                                                  float* __restrict__ dst, float* __restrict__ bdst) {
    __shared__ float As[DW_BM * DW_LS];
    __shared__ float Bs[DW_BN * DW_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const int mb = blockIdx.x % g.mblocks, nb = blockIdx.x / g.mblocks;
    const int tap = blockIdx.y, sp = blockIdx.z;
    const int m0 = mb * DW_BM, n0 = nb * DW_BN;
    const int HW = g.H * g.W;
    const int64_t P = (int64_t)g.N * HW;
    const size_t E = (size_t)g.taps * g.Cout * g.Cin;
    float* tile = dst + (size_t)sp * E + ((size_t)tap * g.Cout + m0) * g.Cin + n0;

    if ((g.dead >> tap) & 1u) {             // exactly zero; with a split the second pass writes it
        if (g.split == 1) {
            for (int i = tid; i < DW_BM * DW_BN; i += 256) {
                const int r = i >> 6, c = i & 63;
                if (m0 + r < g.Cout && n0 + c < g.Cin) tile[(size_t)r * g.Cin + c] = 0.0f;
            }
        }
        return;
    }

    int dy = 0, dx = 0;
    if (g.taps == 9) { dy = (tap / 3 - 1) * g.dil; dx = (tap % 3 - 1) * g.dil; }
    // rows of an image whose shifted row lies inside it, as a range of the flattened plane
    const int lo = (dy < 0 ? -dy : 0) * g.W, hi = (dy > 0 ? g.H - dy : g.H) * g.W;
    const int c0 = (int)((int64_t)sp * g.nch / g.split), c1 = (int)((int64_t)(sp + 1) * g.nch / g.split);
    // first chunk >= c in this range with a pixel whose shifted row exists (c1: none)
    auto next_live = [&](int c) -> int {
        if (c >= c1) return c1;
        const int64_t p0 = (int64_t)c * DW_KC;
        const int64_t n = p0 / HW;
        const int rem = (int)(p0 - n * HW);
        if ((rem < hi && rem + DW_KC - 1 >= lo) || rem + DW_KC - 1 >= HW + lo) return c;
        const int64_t tgt = (rem < lo ? n : n + 1) * HW + lo;
        const int64_t cn = tgt / DW_KC;
        return cn < c1 ? (int)cn : c1;
    };

    // loader role: pixel k of the chunk, rows lr0 + 8*u (A: u = 0..15, B: u = 0..7)
    const int lk = tid & 31, lr0 = tid >> 5;
    const bool do_bias = bdst != nullptr && nb == 0 && tap == (g.taps == 9 ? 4 : 0);

    floatx16w acc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
    float areg[16], breg[8], bsum[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) bsum[u] = 0.f;

    auto fetch = [&](int c) {
        const int64_t p = (int64_t)c * DW_KC + lk;
        const bool pok = p < P;
        const int n = pok ? (int)(p / HW) : 0;
        const int rem = pok ? (int)(p - (int64_t)n * HW) : 0;
        const int y = rem / g.W, xx = rem - y * g.W;
        const float* ga = gy + ((size_t)n * g.Cout + m0 + lr0) * HW + rem;
#pragma unroll
        for (int u = 0; u < 16; ++u) areg[u] = (pok && m0 + lr0 + 8 * u < g.Cout) ? ga[(size_t)(8 * u) * HW] : 0.f;
        const int ys = y + dy, xs = xx + dx;
        const bool ok = pok && ys >= 0 && ys < g.H && xs >= 0 && xs < g.W;
        const float* xa = x + ((size_t)n * g.Cin + n0 + lr0) * HW + (ok ? ys * g.W + xs : 0);
#pragma unroll
        for (int u = 0; u < 8; ++u) breg[u] = (ok && n0 + lr0 + 8 * u < g.Cin) ? xa[(size_t)(8 * u) * HW] : 0.f;
    };
    auto stash = [&]() {
#pragma unroll
        for (int u = 0; u < 16; ++u) As[(lr0 + 8 * u) * DW_LS + lk] = areg[u];
#pragma unroll
        for (int u = 0; u < 8; ++u) Bs[(lr0 + 8 * u) * DW_LS + lk] = breg[u];
        if (do_bias) {
#pragma unroll
            for (int u = 0; u < 16; ++u) bsum[u] += areg[u];
        }
    };

    int c = next_live(c0);
    if (c < c1) {
        fetch(c);
        stash();
    }
    __syncthreads();
    const float* ap = As + (wave * 32 + li) * DW_LS + half;
    const float* bp = Bs + li * DW_LS + half;
    while (c < c1) {
        const int cn = next_live(c + 1);
        if (cn < c1) fetch(cn);             // global -> registers while this chunk is multiplied
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < DW_KC / 2; ++ks) {
            const float a = ap[2 * ks];
            const float b0 = bp[2 * ks], b1 = bp[32 * DW_LS + 2 * ks];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
        }
        __syncthreads();
        if (cn < c1) stash();
        __syncthreads();
        c = cn;
    }

    // lane holds input-channel column li (+32 for the second tile), rows (r & 3) + 8 * (r >> 2) + 4 * half
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ci = n0 + s * 32 + li;
        if (ci >= g.Cin) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m0 + row < g.Cout) tile[(size_t)row * g.Cin + s * 32 + li] = acc[s][r];
        }
    }
    if (do_bias) {                          // the 32 lanes of a loader row group hold that row's pixels k = 0..31
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            float v = bsum[u];
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 32);
            const int co = m0 + lr0 + 8 * u;
            if (lk == 0 && co < g.Cout) bdst[(size_t)sp * g.Cout + co] = v;
        }
    }
}

// second pass of a split: partials added in range order (dead taps: 0.0f), weight elements first, then the bias
__global__ __launch_bounds__(256) void dense_conv_wgrad_sum_kernel(const float* __restrict__ ws, DenseWgradGeom g, float* __restrict__ dw,
                                                                   float* __restrict__ db) {
    const size_t E = (size_t)g.taps * g.Cout * g.Cin;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < E) {
        const int tap = (int)(i / ((size_t)g.Cout * g.Cin));
        float v = 0.0f;
        if (!((g.dead >> tap) & 1u)) {
            v = ws[i];
            for (int s = 1; s < g.split; ++s) v += ws[(size_t)s * E + i];
        }
        dw[i] = v;
    } else if (db != nullptr && i < E + g.Cout) {
        const float* wb = ws + (size_t)g.split * E;
        const size_t co = i - E;
        float v = wb[co];
        for (int s = 1; s < g.split; ++s) v += wb[(size_t)s * g.Cout + co];
        db[co] = v;
    }
}

// shape checks and the launch geometry shared by the size query and the launcher
static int dense_wgrad_geom(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t dilation, int32_t split,
                            DenseWgradGeom& g) {
    MSPL_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, MSPL_ERR_BAD_SHAPE,
                 "dense_conv_wgrad: bad shape N=%d Cin=%d Cout=%d %dx%d", N, Cin, Cout, H, W);
    MSPL_REQUIRE(ksize == 1 || ksize == 3, MSPL_ERR_UNSUPPORTED, "dense_conv_wgrad: kernel size %d (1 or 3)", ksize);
    MSPL_REQUIRE(dilation >= 1, MSPL_ERR_UNSUPPORTED, "dense_conv_wgrad: dilation %d", dilation);
    MSPL_REQUIRE(Cin % 32 == 0, MSPL_ERR_UNSUPPORTED, "dense_conv_wgrad: Cin=%d is not a multiple of 32", Cin);
    MSPL_REQUIRE(split >= 0, MSPL_ERR_BAD_SHAPE, "dense_conv_wgrad: split %d", split);
    const int64_t nch = ceil_div64((int64_t)N * H * W, DW_KC);
    MSPL_REQUIRE(nch < (1ll << 30), MSPL_ERR_BAD_SHAPE, "dense_conv_wgrad: too many pixels");
    g.N = N; g.Cin = Cin; g.Cout = Cout; g.H = H; g.W = W; g.taps = ksize * ksize; g.dil = dilation;
    g.mblocks = ceil_div(Cout, DW_BM);
    g.nblocks = ceil_div(Cin, DW_BN);
    g.nch = (int)nch;
    g.dead = 0;
    int live = 1;
    if (g.taps == 9) {
        live = 0;
        for (int t = 0; t < 9; ++t) {
            const bool dead = (t / 3 != 1 && dilation >= H) || (t % 3 != 1 && dilation >= W);
            if (dead) g.dead |= 1u << t; else ++live;
        }
    }
    MSPL_REQUIRE((int64_t)g.mblocks * g.nblocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "dense_conv_wgrad: grid too large");
    if (split == 0) {
        // about eight workgroups per CU, ranges of at least 16 chunks (512 pixels), at most 32 ranges.  Measured at 16 x 2048 x 32 x 64
        // (tools/aspp_train_probe.py, wgrad_ms_by_split): the 3x3 convolutions' 576 tiles are 2.25 per CU, one range leaves a quarter of
        // the chip idle in the last round and the row-skipping taps finish early -- 3.9 ms as one range, 2.9-3.0 ms as 4, 8 or 16; the
        // 1x1 convolutions (64 / 40 tiles) 2.16 ms as one range, 0.40 / 0.30 ms as 32.
        const int64_t tiles = (int64_t)g.mblocks * g.nblocks * live;
        int64_t s = ceil_div64(2048, tiles);
        if (s > nch / 16) s = nch / 16;
        if (s > 32) s = 32;
        split = s < 1 ? 1 : (int)s;
    }
    MSPL_REQUIRE(split <= DW_MAX_SPLIT, MSPL_ERR_UNSUPPORTED, "dense_conv_wgrad: split %d (at most %d)", split, DW_MAX_SPLIT);
    g.split = split;
    return MSPL_OK;
}

}  // namespace mspl

using namespace mspl;

extern "C" int64_t mspl_dense_conv_wgrad_workspace_bytes(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize,
                                                         int32_t dilation, int32_t split) {
    DenseWgradGeom g;
    if (int rc = dense_wgrad_geom(N, Cin, Cout, H, W, ksize, dilation, split, g)) return rc;
    if (g.split == 1) return 0;
    return (int64_t)g.split * ((int64_t)g.taps * Cout * Cin + Cout) * (int64_t)sizeof(float);
}

extern "C" int mspl_dense_conv_wgrad(const float* gy, const float* x, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W,
                                     int32_t ksize, int32_t dilation, int32_t split, void* workspace, int64_t workspace_bytes,
                                     float* dw_packed, float* dbias, void* stream) {
    MSPL_REQUIRE(gy && x && dw_packed, MSPL_ERR_NULL_POINTER, "dense_conv_wgrad: null pointer");
    DenseWgradGeom g;
    if (int rc = dense_wgrad_geom(N, Cin, Cout, H, W, ksize, dilation, split, g)) return rc;
    const int64_t E = (int64_t)g.taps * Cout * Cin;
    const dim3 grid((unsigned)(g.mblocks * g.nblocks), (unsigned)g.taps, (unsigned)g.split);
    if (g.split == 1) {
        hipLaunchKernelGGL(dense_conv_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, gy, x, g, dw_packed, dbias);
        MSPL_CHECK_LAUNCH("dense_conv_wgrad");
        return MSPL_OK;
    }
    const int64_t need = (int64_t)g.split * (E + Cout) * (int64_t)sizeof(float);
    MSPL_REQUIRE(workspace != nullptr && workspace_bytes >= need, MSPL_ERR_BAD_SHAPE,
                 "dense_conv_wgrad: split %d needs a workspace of %lld bytes (mspl_dense_conv_wgrad_workspace_bytes), got %lld", g.split,
                 (long long)need, (long long)workspace_bytes);
    float* ws = (float*)workspace;
    hipLaunchKernelGGL(dense_conv_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, gy, x, g, ws,
                       dbias ? ws + (size_t)g.split * E : nullptr);
    MSPL_CHECK_LAUNCH("dense_conv_wgrad");
    const int64_t total = E + (dbias ? Cout : 0);
    hipLaunchKernelGGL(dense_conv_wgrad_sum_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)ws, g, dw_packed, dbias);
    MSPL_CHECK_LAUNCH("dense_conv_wgrad");
    return MSPL_OK;
}
