// Head of a DownSampler block in one launch (inference): the EESP branch's proj_1x1 (nn_layers/eesp.py:60-67: grouped 1x1, 4
// groups, BatchNorm, PReLU) and the average-pool branch with the block's epilogue (nn_layers/eesp.py:123-144: AvgPool2d(3, 2, 1)
// into channels [0, nin) of the output, + the image reinforcement, module PReLU) from ONE read of the block's input, + the plane
// sums of the input that the decoder's EfficientPWConv gate needs.
//
// Group g of the projection reads exactly the input channels [g*K, (g+1)*K), K = nin / groups, so a workgroup that owns (image,
// group, 256 strips of a plane) walks those K channels once.  A thread owns what a thread of avgpool3x3s2_down_kernel owns: four
// pooled outputs of a row = the 2 x 8 input block (rows 2y, 2y+1; columns 2*x0 .. 2*x0+7) plus the halo row 2y-1 and the halo column
// 2*x0-1 (both re-read through L1 / L2: they are some other thread's own block).  Per input channel the nine loads of that kernel
// feed its pool arithmetic unchanged, and the sixteen own pixels also go into M x 16 projection accumulators (M = n / groups).
//
// Results: the pooled half and the plane-sum partials repeat avgpool3x3s2_down_kernel<false> operation by operation (same strip
// split, same slot layout: bit-identical); the reduced tensor is PReLU(fma(sum_k fma(w[m][k], x[k], acc), scale, shift)) with k
// ascending from zero: the order of conv1x1_thin_kernel (bit-identical where that kernel serves the projection).
// Nothing here depends on N beyond gridDim.z.
#include "common.hpp"

namespace mspl {

struct DhGeom {
    int nin, K, nr;                   // input channels, input channels per group, reduced channels (groups * M)
    int Hi, Wi, Ho, Wo, XS;           // XS = Wo / 4 strips per pooled row
    unsigned mag_xs;
    int ctot;                         // channels of the block's output
};

struct DhTile {                       // one input channel's share of a thread: rows 2y-1 (clamped), 2y, 2y+1
    float4 a[3], b[3];
    float l[3];
};

__device__ __forceinline__ DhTile dh_load(const float* __restrict__ src, const unsigned (&o)[3], bool left) {
    DhTile t;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        t.a[ky] = *reinterpret_cast<const float4*>(src + o[ky]);
        t.b[ky] = *reinterpret_cast<const float4*>(src + o[ky] + 4);
        t.l[ky] = src[left ? o[ky] - 1 : o[ky]];
    }
    return t;
}

// M: reduced channels per group (6: level 2 of ESPDNet s=2.0, 8: level 3).  REINF: the block has the image reinforcement.
// 16 * M accumulators + two tiles (the next channel's loads are in flight while this one's FMAs issue): two waves per SIMD.
template <int M, bool REINF>
__global__ __launch_bounds__(256, 2) void down_head_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                           const float* __restrict__ pscale, const float* __restrict__ pshift,
                                                           const float* __restrict__ palpha, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ alpha,
                                                           const float* __restrict__ reinf_r, const float* __restrict__ reinf_w,
                                                           DhGeom g, float* __restrict__ r, float* __restrict__ out,
                                                           float* __restrict__ psum) {
    constexpr int MP = (M + 3) & ~3;                                 // weight rows in LDS, padded to whole 16-byte reads
    extern __shared__ __attribute__((aligned(16))) float smem[];     // wl[K][MP], then part[K][4]
    float* wl = smem;
    float* part = smem + g.K * MP;
    const int grp = blockIdx.y, n = blockIdx.z;
    for (int i = threadIdx.x; i < g.K * MP; i += 256) {
        const int m = i % MP, k = i / MP;
        wl[i] = m < M ? wp[((size_t)grp * M + m) * g.K + k] : 0.f;
    }
    __syncthreads();
    const unsigned strips = (unsigned)(g.Ho * g.XS);
    const unsigned s0 = blockIdx.x * 256u + threadIdx.x;
    const bool live = s0 < strips;
    const unsigned s = live ? s0 : strips - 1;                       // idle lanes of the last workgroup repeat its last strip, store nothing
    const int y = g.XS == 1 ? (int)s : (int)__umulhi(s, g.mag_xs);
    const int x0 = ((int)s - y * g.XS) * 4;
    const unsigned plane = (unsigned)(g.Hi * g.Wi);
    const float* src = x + ((size_t)n * g.nin + (size_t)grp * g.K) * (size_t)plane;          // uniform
    unsigned o[3];
    float mk[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * y - 1 + ky;
        mk[ky] = (iy >= 0 && iy < g.Hi) ? 1.f : 0.f;
        o[ky] = (unsigned)(min(max(iy, 0), g.Hi - 1) * g.Wi + 2 * x0);
    }
    const bool left = x0 > 0;
    const float lm = left ? 1.f : 0.f;
    const unsigned pix = (unsigned)(y * g.Wo + x0), hw = (unsigned)(g.Ho * g.Wo);
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    if (REINF) {
        const float* rr = reinf_r + (size_t)n * 3 * hw;                                      // uniform
        r0 = *reinterpret_cast<const float4*>(rr + pix);
        r1 = *reinterpret_cast<const float4*>(rr + hw + pix);
        r2 = *reinterpret_cast<const float4*>(rr + 2 * hw + pix);
    }
    float acc[M][16];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[m][j] = 0.f;
    float* pooled = out + ((size_t)n * g.ctot + (size_t)grp * g.K) * (size_t)hw + pix;

    DhTile cur = dh_load(src, o, left);
#pragma unroll 1
    for (int k = 0; k < g.K; ++k) {
        const int kn = min(k + 1, g.K - 1);                          // (the last round requests its own channel again: no branch)
        const DhTile nxt = dh_load(src + (size_t)kn * plane, o, left);
        // ---- pool branch of input channel c = grp*K + k: avgpool3x3s2_down_kernel's arithmetic
        const float4* a = cur.a;
        const float4* b = cur.b;
        float own = ((a[1].x + a[1].y) + (a[1].z + a[1].w)) + ((b[1].x + b[1].y) + (b[1].z + b[1].w));
        own += mk[2] * (((a[2].x + a[2].y) + (a[2].z + a[2].w)) + ((b[2].x + b[2].y) + (b[2].z + b[2].w)));
        float pa[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const float w = mk[ky];
            pa[0] += w * ((lm * cur.l[ky] + a[ky].x) + a[ky].y);
            pa[1] += w * ((a[ky].y + a[ky].z) + a[ky].w);
            pa[2] += w * ((a[ky].w + b[ky].x) + b[ky].y);
            pa[3] += w * ((b[ky].y + b[ky].z) + b[ky].w);
        }
        const int c = grp * g.K + k;                                                          // uniform
        const float sc = scale[c], sh = shift[c], al = alpha[c];
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaf(pa[j] * (1.0f / 9.0f), sc, sh);
        if (REINF) {
            const float rw0 = reinf_w[c * 3], rw1 = reinf_w[c * 3 + 1], rw2 = reinf_w[c * 3 + 2];
            v[0] += rw0 * r0.x + rw1 * r1.x + rw2 * r2.x;
            v[1] += rw0 * r0.y + rw1 * r1.y + rw2 * r2.y;
            v[2] += rw0 * r0.z + rw1 * r1.z + rw2 * r2.z;
            v[3] += rw0 * r0.w + rw1 * r1.w + rw2 * r2.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.0f ? v[j] : al * v[j];
        if (live) store_out4(pooled + (size_t)k * hw, make_float4(v[0], v[1], v[2], v[3]));
        own = wave_sum_dpp(live ? own : 0.f);
        if ((threadIdx.x & 63) == 63) part[k * 4 + (threadIdx.x >> 6)] = own;
        // ---- projection: the sixteen own pixels of this input channel into every reduced channel of the group
        const float xv[16] = {a[1].x, a[1].y, a[1].z, a[1].w, b[1].x, b[1].y, b[1].z, b[1].w,
                              a[2].x, a[2].y, a[2].z, a[2].w, b[2].x, b[2].y, b[2].z, b[2].w};
#pragma unroll
        for (int m4 = 0; m4 < MP; m4 += 4) {
            const float4 wv = *reinterpret_cast<const float4*>(wl + k * MP + m4);
            const float ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) {
                if (m4 + mm < M) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[m4 + mm][j] = fmaf(ww[mm], xv[j], acc[m4 + mm][j]);
                }
            }
        }
        cur = nxt;
    }
    // ---- reduced tensor: proj_1x1's BatchNorm + PReLU, rows 2y and 2y+1
    if (live) {
        float* rd = r + ((size_t)n * g.nr + (size_t)grp * M) * (size_t)plane;                 // uniform
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int cr = grp * M + m;
            const float ps = pscale[cr], pb = pshift[cr], pl = palpha[cr];
            float t[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float u = fmaf(acc[m][j], ps, pb);
                t[j] = u > 0.0f ? u : pl * u;
            }
            float* d = rd + (size_t)m * plane;
            store_out4(d + o[1], make_float4(t[0], t[1], t[2], t[3]));
            store_out4(d + o[1] + 4, make_float4(t[4], t[5], t[6], t[7]));
            store_out4(d + o[2], make_float4(t[8], t[9], t[10], t[11]));
            store_out4(d + o[2] + 4, make_float4(t[12], t[13], t[14], t[15]));
        }
    }
    __syncthreads();
    // one slot per (plane, workgroup), planes in (n, c) order, the four wave partials added in a fixed tree: the gate sums the slots in order
    if ((int)threadIdx.x < g.K) {
        const float* p = part + threadIdx.x * 4;
        psum[((size_t)n * g.nin + (size_t)grp * g.K + threadIdx.x) * gridDim.x + blockIdx.x] = (p[0] + p[1]) + (p[2] + p[3]);
    }
}

// Shapes served: 4 groups, n / 4 in {6, 8}, nin / 4 <= 64, H even, W a multiple of 8 (whole 16-byte strips of pooled outputs).
static bool down_head_shape_ok(int N, int nin, int n, int groups, int H, int W) {
    if (N <= 0 || nin <= 0 || n <= 0 || H < 2 || W < 8 || groups != 4 || nin % 4 || n % 4) return false;
    const int M = n / 4, K = nin / 4;
    if ((M != 6 && M != 8) || K < 1 || K > 64) return false;
    if ((H & 1) || (W & 7) || N > 65535) return false;
    if ((int64_t)nin * H * W >= (1ll << 30) || (int64_t)(H / 2) * (W / 8) * (W / 8) >= (1ll << 32)) return false;
    return true;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_down_head_fits(int32_t N, int32_t nin, int32_t n, int32_t groups, int32_t H, int32_t W, uint32_t launch_flags) {
    (void)launch_flags;
    return down_head_shape_ok(N, nin, n, groups, H, W) ? 1 : 0;
}

// Partial plane sums per plane written by mspl_down_head_fwd for an (H, W) input (the psum buffer holds N * nin times this).
extern "C" int mspl_down_head_psum_blocks(int32_t H, int32_t W) {
    if (H < 2 || W < 8 || (H & 1) || (W & 7)) return MSPL_ERR_BAD_SHAPE;
    return ceil_div((H / 2) * (W / 8), 256);
}

extern "C" int mspl_down_head_fwd(const float* x, const float* wp, const float* pscale, const float* pshift, const float* palpha,
                                  int32_t N, int32_t nin, int32_t n, int32_t groups, int32_t H, int32_t W,
                                  const mspl_epilogue_t* ep, float* r, float* out, float* psum, void* stream) {
    MSPL_REQUIRE(x && wp && pscale && pshift && palpha && ep && r && out && psum, MSPL_ERR_NULL_POINTER, "down_head: null pointer");
    MSPL_REQUIRE(down_head_shape_ok(N, nin, n, groups, H, W), MSPL_ERR_UNSUPPORTED,
                 "down_head: shape N=%d nin=%d n=%d groups=%d %dx%d is not a fused one (mspl_down_head_fits)", N, nin, n, groups, H, W);
    if (int rc = check_epi(ep, nin, "down_head")) return rc;
    MSPL_REQUIRE(ep->scale && ep->shift && ep->alpha && !ep->pre_add && !ep->residual && !ep->gate && !ep->raw_out &&
                 ep->out_coff == 0 && ep->out_ctot >= nin, MSPL_ERR_UNSUPPORTED,
                 "down_head: the epilogue is scale, shift, alpha (+ reinforcement) on channels [0, nin) of the destination");
    MSPL_REQUIRE(((((uintptr_t)x) | ((uintptr_t)r) | ((uintptr_t)out) | ((uintptr_t)ep->reinf_r)) & 15) == 0, MSPL_ERR_UNSUPPORTED,
                 "down_head: tensors must be 16-byte aligned");
    DhGeom g;
    g.nin = nin; g.K = nin / groups; g.nr = n;
    g.Hi = H; g.Wi = W; g.Ho = H / 2; g.Wo = W / 2; g.XS = g.Wo / 4;
    g.mag_xs = (unsigned)((0x100000000ull + g.XS - 1) / g.XS);
    g.ctot = ep->out_ctot;
    const int M = n / groups, MP = (M + 3) & ~3;
    const size_t lds = (size_t)g.K * (MP + 4) * sizeof(float);
    const dim3 grid((unsigned)ceil_div(g.Ho * g.XS, 256), (unsigned)groups, (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
#define MSPL_DH_LAUNCH(MM, RF)                                                                                                  \
    hipLaunchKernelGGL((down_head_kernel<MM, RF>), grid, dim3(256), lds, s, x, wp, pscale, pshift, palpha, ep->scale, ep->shift, \
                       ep->alpha, ep->reinf_r, ep->reinf_w, g, r, out, psum)
    if (M == 6) { if (ep->reinf_r) MSPL_DH_LAUNCH(6, true); else MSPL_DH_LAUNCH(6, false); }
    else        { if (ep->reinf_r) MSPL_DH_LAUNCH(8, true); else MSPL_DH_LAUNCH(8, false); }
#undef MSPL_DH_LAUNCH
    MSPL_CHECK_LAUNCH("down_head");
    return MSPL_OK;
}
