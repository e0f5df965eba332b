// K11 at head resolution: the uest loss of uest_seg_multi_os.py:1020-1023 taken from the two decoder outputs BEFORE their bilinear
// up-sampling (model/segmentation/espdnet_ue.py:301-302: main at H/2 x W/2, auxiliary at H/4 x W/4, both interpolated to H x W with
// align_corners=True).
//
// The three-step form (two bilinear launches, then mspl_uw_loss_scaled_fwd_bwd) writes the two full-size logit tensors and reads them
// back: 75 + 47 us of a 6.7 ms step at 16 x 5 x 288x480.  Here a workgroup owns a band of TH rows x 256 columns of the label map: it
// stages the patches of both low-resolution maps that band interpolates from in LDS and evaluates the up-sampled logits per pixel
// with the reference's own expression (wy0 * (wx0 * a + wx1 * b) + wy1 * (...): the forward is the one mspl_resize_bilinear
// computes), the loss terms and the closed-form gradients of uw_loss_kernel (uw_loss.hip).  The gradients leave at label resolution
// (N,C,H,W), for mspl_bilinear_bwd: the full-size logits never exist.
//
// (Measured and not kept, round 5: the transposed interpolation inside this kernel as ds_add_f32 into LDS accumulators of the patches'
// shape -- 40 LDS float atomics per pixel, conflict-free by construction: 463 us against 69 us without them at 16 x 5 x 256x480.  LDS
// float atomics retire at ~0.3 lanes per clock and CU; the global atomic flush of the patches was free.)
#include <algorithm>
#include <mutex>

#include "common.hpp"
#include "loss_parts.hpp"

namespace mspl {

struct UhGeom {
    int N, C, H, W;
    int Hm, Wm, Ha, Wa;             // main / auxiliary maps
    float shm, swm, sha, swa;       // bilinear scales (align_corners=True)
    int TH, tiles_x, tiles_y;       // band height; 256-column tiles per row; bands per image
    int MR, MC, AR, AC;             // LDS patch capacities (rows, columns)
    unsigned total;                 // tiles
    float ce_scale, inv_npix;
};

constexpr int UH_TW = 256;

// exp / log of the softmax terms on the transcendental unit (v_exp_f32 / v_log_f32 with one multiply: ~1 ulp on arguments <= 0 resp. sums in
// [1, C]; expf / logf expand to ~10 instructions each and the pixel loop holds 3 C + 1 of them: ~1030 -> ~820 vector instructions in the kernel, 69 -> 43 us at 16 x 5 x 256x480)
__device__ __forceinline__ float uh_exp(float x) { return __expf(x); }
__device__ __forceinline__ float uh_log(float x) { return __logf(x); }

// CM: class capacity of the register arrays; EXACT: C == CM (no per-class predicates).  Up to 8 classes the three exponentials of a
// class are kept from the sums to the gradients; beyond, they are recomputed (5 x CM registers spill at CM = 20).
//
// METERS: the training loop's per-step meters (uest_seg_multi_os.py:1032-1037) taken where the up-sampled main logits already sit in
// registers.  MIOU(K).get_iou(pred, labels) is the first maximum of a[0..C) (torch.max(output, 1) on the MAIN head alone, not on
// a + 0.5 bv) and uint8 arithmetic on it (segmentation_miou.py:28-41, the rule of miou_areas_kernel in labels.hip); the pixel's
// two codes p and g ride through the four pixels of a row packed in two registers, and the three K-bin histograms are taken per
// row after the pixel loop: a compare per bin, the population count of its lane mask on the scalar unit, one LDS add by lane 0
// (label_epilogue's histogram, labels.hip).  Per workgroup: one 64-bit atomic per non-empty bin, and one double atomic that adds
// meter_weight x (its share of the loss) for losses.update(loss.item(), images.size(0)).  The non-METERS instantiations compile to
// what they were before the meters existed (every addition sits under `if constexpr`-like constant conditions).
struct UhMeters {
    unsigned long long* areas;      // [3 K]: inter | pred | mask
    double* meter;                  // meter[0] += meter_weight * loss
    int K;
    float weight;
};

template <int CM, bool EXACT, bool METERS = false>
__global__ __launch_bounds__(256) void uw_loss_heads_kernel(const float* __restrict__ mainp, const float* __restrict__ auxp,
                                                            const int64_t* __restrict__ target, const float* __restrict__ cw,
                                                            UhGeom g, float* __restrict__ loss_acc, float* __restrict__ gpred,
                                                            float* __restrict__ gaux, UhMeters mt) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ unsigned int mhist[METERS ? 3 * MIOU_MAX_BINS : 1];
    if (METERS) miou_clear(mhist, mt.K);       // (ordered before its first use by the tile loop's barrier)
    const int C = EXACT ? CM : g.C;
    constexpr bool KEEP = CM <= 8;
    constexpr int CK = KEEP ? CM : 1;
    const int msz = g.MR * g.MC, asz = g.AR * g.AC;
    float* LM = sm;                      // [C][MR][MC] main logits
    float* LA = LM + C * msz;            // [C][AR][AC] auxiliary logits
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float contrib = 0.f;
    for (unsigned tile = blockIdx.x; tile < g.total; tile += gridDim.x) {
        const BandTile bt = band_tile(tile, g.tiles_x, g.tiles_y, g.TH, UH_TW, g.H, g.W);
        const int img = bt.img, y0 = bt.y0, x0 = bt.x0, rows = bt.rows;
        const BandPatch pm = band_patch(g.shm, g.swm, g.Hm, g.Wm, bt, g.MR, g.MC);
        const BandPatch pa = band_patch(g.sha, g.swa, g.Ha, g.Wa, bt, g.AR, g.AC);
        const int my0 = pm.y0, mx0 = pm.x0, ay0 = pa.y0, ax0 = pa.x0;
        band_stage(LM, mainp, img, C, g.Hm, g.Wm, pm, g.MC, msz, wave, lane);
        band_stage(LA, auxp, img, C, g.Ha, g.Wa, pa, g.AC, asz, wave, lane);
        __syncthreads();
        for (int r = wave; r < rows; r += 4) {
            const int y = y0 + r;
            int ya, yb;  float wy0m, wy1m, wy0a, wy1a;
            bilinear_src(g.shm, y, g.Hm, ya, yb, wy0m, wy1m);
            const int rm0 = (ya - my0) * g.MC - mx0, rm1 = (yb - my0) * g.MC - mx0;
            bilinear_src(g.sha, y, g.Ha, ya, yb, wy0a, wy1a);
            const int ra0 = (ya - ay0) * g.AC - ax0, ra1 = (yb - ay0) * g.AC - ax0;
            const size_t rowoff = ((size_t)img * g.H + y) * (size_t)g.W;
            const size_t goff = ((size_t)img * C * g.H + y) * (size_t)g.W;
            // a wave takes the row's 256 columns as four runs of 64 (coalesced label loads and gradient stores), one pixel per lane
            // at a time: unrolled, the four pixels' softmax terms are all live at once (205 VGPRs at C = 5, spills beyond)
            unsigned pk_p = 0, pk_g = 0;     // METERS: the row's four (p, g) codes, a byte each; 0 counts nowhere
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int xs = x0 + j * 64 + lane;
                if (xs >= g.W) continue;
                const int t = (int)target[rowoff + xs];
                int xa, xb;  float wx0m, wx1m, wx0a, wx1a;
                bilinear_src(g.swm, xs, g.Wm, xa, xb, wx0m, wx1m);
                const int m00 = rm0 + xa, m01 = rm0 + xb, m10 = rm1 + xa, m11 = rm1 + xb;
                bilinear_src(g.swa, xs, g.Wa, xa, xb, wx0a, wx1a);
                const int a00 = ra0 + xa, a01 = ra0 + xb, a10 = ra1 + xa, a11 = ra1 + xb;
                float a[CM], bv[CM];
                float m1 = -INFINITY, m2 = -INFINITY, mo = -INFINITY;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (EXACT || c < C) {
                        const float* pm = LM + c * msz;
                        const float* pa = LA + c * asz;
                        const float topm = wx0m * pm[m00] + wx1m * pm[m01], botm = wx0m * pm[m10] + wx1m * pm[m11];
                        const float topa = wx0a * pa[a00] + wx1a * pa[a01], bota = wx0a * pa[a10] + wx1a * pa[a11];
                        a[c] = wy0m * topm + wy1m * botm;
                        bv[c] = wy0a * topa + wy1a * bota;
                        m1 = fmaxf(m1, a[c]);  m2 = fmaxf(m2, bv[c]);  mo = fmaxf(mo, a[c] + 0.5f * bv[c]);
                    }
                }
                if (METERS) {
                    float best = a[0];  unsigned bi = 0;
#pragma unroll
                    for (int c = 1; c < CM; ++c)
                        if ((EXACT || c < C) && a[c] > best) { best = a[c];  bi = (unsigned)c; }
                    miou_pack(pk_p, pk_g, j, miou_codes(bi, t));
                }
                float e1[CK], e2[CK], eo[CK];
                float s1 = 0.f, s2 = 0.f, so = 0.f;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (EXACT || c < C) {
                        const float x1 = uh_exp(a[c] - m1), x2 = uh_exp(bv[c] - m2), xo = uh_exp(a[c] + 0.5f * bv[c] - mo);
                        if (KEEP) { e1[KEEP ? c : 0] = x1;  e2[KEEP ? c : 0] = x2;  eo[KEEP ? c : 0] = xo; }
                        s1 += x1;  s2 += x2;  so += xo;
                    }
                }
                const float l1 = m1 + uh_log(s1), l2 = m2 + uh_log(s2), lo = mo + uh_log(so);
                const float r1 = __builtin_amdgcn_rcpf(s1), r2 = __builtin_amdgcn_rcpf(s2), ro = __builtin_amdgcn_rcpf(so);
                const bool tin = t >= 0 && t < C;
                float kld = 0.f, ot = 0.f;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (EXACT || c < C) {
                        const float p1 = KEEP ? e1[KEEP ? c : 0] * r1 : uh_exp(a[c] - m1) * r1;
                        kld += p1 * (a[c] - l1) - p1 * (bv[c] - l2);
                        if (c == t) ot = a[c] + 0.5f * bv[c];
                    }
                }
                const float wt = tin ? cw[t] : 0.f;
                const float nll = -(ot - lo);
                const float u = uh_exp(-kld);
                const float ce = wt * nll * u;
                contrib += g.ce_scale * ce * g.inv_npix + kld * g.inv_npix;
                const float gk = (1.f - g.ce_scale * ce) * g.inv_npix;
                const float go = g.ce_scale * wt * u * g.inv_npix;
                float* dp = gpred + goff + xs;
                float* da = gaux + goff + xs;
                const size_t hw = (size_t)g.H * g.W;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (EXACT || c < C) {
                        const float p1 = (KEEP ? e1[KEEP ? c : 0] : uh_exp(a[c] - m1)) * r1, p2 = (KEEP ? e2[KEEP ? c : 0] : uh_exp(bv[c] - m2)) * r2;
                        const float po = (KEEP ? eo[KEEP ? c : 0] : uh_exp(a[c] + 0.5f * bv[c] - mo)) * ro;
                        const float d = (a[c] - l1) - (bv[c] - l2);
                        const float dce = go * (po - (c == t ? 1.f : 0.f));
                        dp[c * hw] = dce + gk * (p1 * (d - kld));
                        da[c * hw] = 0.5f * dce - gk * (p1 - p2);
                    }
                }
            }
            if (METERS) miou_tally_row(mhist, mt.K, pk_p, pk_g, lane);
        }
        __syncthreads();                 // the next tile's staging overwrites the patches
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_down(contrib, o, 64);
    __shared__ float part[4];
    if (lane == 0) part[wave] = contrib;
    __syncthreads();
    if (!METERS) {
        if (tid == 0) atomicAdd(loss_acc, (part[0] + part[1]) + (part[2] + part[3]));
    } else {
        if (tid == 0) {
            const float share = (part[0] + part[1]) + (part[2] + part[3]);
            atomicAdd(loss_acc, share);
            atomicAdd(mt.meter, (double)mt.weight * (double)share);
        }
        // (the tile loop's last barrier ordered every wave's LDS adds; a workgroup with no tile has only zeros)
        miou_flush(mhist, mt.K, mt.areas);
    }
}

}  // namespace mspl

using namespace mspl;

// (a predicated 20-class form for the counts in between spills 6 600 registers: those take the three-step form)
extern "C" int mspl_uw_loss_heads_supported(int32_t C) { return (C >= 1 && C <= 8) || C == 13 || C == 20; }

// mt == nullptr: the plain kernel.  With meters the workgroup's 3 x 64 LDS counters come on top of the patches, so the band is sized
// against 1 KB less (the gradients of a pixel do not depend on the band it falls in).
static int uh_launch(const float* main_lo, const float* aux_lo, const int64_t* target, const float* class_weights,
                     int32_t N, int32_t C, int32_t Hm, int32_t Wm, int32_t Ha, int32_t Wa, int32_t H, int32_t W,
                     float ce_scale, float out_scale, float* loss_acc, float* gpred, float* gaux, const UhMeters* mt, void* stream) {
    const size_t extra = mt ? 1024 : 0;
    MSPL_REQUIRE(main_lo && aux_lo && target && class_weights && loss_acc && gpred && gaux, MSPL_ERR_NULL_POINTER, "uw_loss_heads: null pointer");
    MSPL_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && Hm > 0 && Wm > 0 && Ha > 0 && Wa > 0, MSPL_ERR_BAD_SHAPE,
                 "uw_loss_heads: bad shape N=%d C=%d main %dx%d aux %dx%d labels %dx%d", N, C, Hm, Wm, Ha, Wa, H, W);
    MSPL_REQUIRE(mspl_uw_loss_heads_supported(C), MSPL_ERR_UNSUPPORTED, "uw_loss_heads: C=%d classes (built for 1..8, 13, 20: use the up-sampled form)", C);
    MSPL_REQUIRE(Hm <= H && Wm <= W && Ha <= H && Wa <= W, MSPL_ERR_UNSUPPORTED, "uw_loss_heads: heads larger than the label map");
    MSPL_REQUIRE((int64_t)N * C * H * W < (1ll << 40), MSPL_ERR_BAD_SHAPE, "uw_loss_heads: too large");
    UhGeom g;
    g.N = N; g.C = C; g.H = H; g.W = W; g.Hm = Hm; g.Wm = Wm; g.Ha = Ha; g.Wa = Wa;
    g.shm = bilinear_scale(Hm, H); g.swm = bilinear_scale(Wm, W); g.sha = bilinear_scale(Ha, H); g.swa = bilinear_scale(Wa, W);
    g.tiles_x = ceil_div(W, UH_TW);
    // band height: 8 rows (two per wave) when that still gives ~3 workgroups per CU, else 4; halved while the patches outgrow 64 KB
    // of LDS (four workgroups per CU at C = 5), 128 KB at most (C = 20)
    size_t lds = 0;
    g.TH = band_height(N, H, g.tiles_x, 64 * 1024 - extra, [&](int th) {
        g.MR = bilinear_span(Hm, H, th);  g.MC = bilinear_span(Wm, W, UH_TW) | 1;
        g.AR = bilinear_span(Ha, H, th);  g.AC = bilinear_span(Wa, W, UH_TW) | 1;
        return lds = (size_t)C * ((size_t)g.MR * g.MC + (size_t)g.AR * g.AC) * sizeof(float);
    });
    MSPL_REQUIRE(lds <= 128 * 1024, MSPL_ERR_UNSUPPORTED, "uw_loss_heads: patches of %zu bytes do not fit", lds);
    g.tiles_y = ceil_div(H, g.TH);
    const int64_t tiles = (int64_t)N * g.tiles_y * g.tiles_x;
    MSPL_REQUIRE(tiles < (1ll << 31), MSPL_ERR_BAD_SHAPE, "uw_loss_heads: too many tiles");
    g.total = (unsigned)tiles;
    g.ce_scale = ce_scale;
    g.inv_npix = out_scale / (float)((int64_t)N * H * W);
    // one same-address atomic per workgroup on the loss: a bounded grid walks the tiles (uw_loss.hip, uw_loss_launch)
    const unsigned blocks = (unsigned)std::min<int64_t>(tiles, 1536);
    hipStream_t s = (hipStream_t)stream;
    static std::once_flag once;
    static bool attr_ok = false;
    std::call_once(once, [] {
        attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&uw_loss_heads_kernel<13, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) == hipSuccess &&
                  hipFuncSetAttribute(reinterpret_cast<const void*>(&uw_loss_heads_kernel<20, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) == hipSuccess &&
                  hipFuncSetAttribute(reinterpret_cast<const void*>(&uw_loss_heads_kernel<13, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) == hipSuccess &&
                  hipFuncSetAttribute(reinterpret_cast<const void*>(&uw_loss_heads_kernel<20, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) == hipSuccess;
    });
    MSPL_REQUIRE(lds + extra <= 64 * 1024 || (attr_ok && C > 8), MSPL_ERR_UNSUPPORTED, "uw_loss_heads: patches of %zu bytes do not fit", lds);
    const UhMeters m = mt ? *mt : UhMeters{nullptr, nullptr, 0, 0.f};
#define MSPL_UH(CMv, EX)                                                                                                                       \
    do {                                                                                                                                       \
        if (mt) hipLaunchKernelGGL((uw_loss_heads_kernel<CMv, EX, true>), dim3(blocks), dim3(256), lds, s, main_lo, aux_lo, target, class_weights, g, loss_acc, gpred, gaux, m); \
        else hipLaunchKernelGGL((uw_loss_heads_kernel<CMv, EX, false>), dim3(blocks), dim3(256), lds, s, main_lo, aux_lo, target, class_weights, g, loss_acc, gpred, gaux, m); \
    } while (0)
    if (C == 5) MSPL_UH(5, true);
    else if (C <= 8) MSPL_UH(8, false);
    else if (C == 13) MSPL_UH(13, true);
    else MSPL_UH(20, true);
#undef MSPL_UH
    MSPL_CHECK_LAUNCH("uw_loss_heads");
    return MSPL_OK;
}

extern "C" int mspl_uw_loss_heads_fwd_bwd(const float* main_lo, const float* aux_lo, const int64_t* target, const float* class_weights,
                                          int32_t N, int32_t C, int32_t Hm, int32_t Wm, int32_t Ha, int32_t Wa, int32_t H, int32_t W,
                                          float ce_scale, float out_scale, float* loss_acc, float* gpred, float* gaux, void* stream) {
    return uh_launch(main_lo, aux_lo, target, class_weights, N, C, Hm, Wm, Ha, Wa, H, W, ce_scale, out_scale, loss_acc, gpred, gaux, nullptr, stream);
}

// The same step with the training loop's meters (uest_seg_multi_os.py:1032-1037) taken inside the kernel: areas[3 K] += the
// [inter | pred | mask] histograms of MIOU(miou_classes).get_iou(up-sampled main head, target), meter[0] += meter_weight * loss.
// Both are accumulated into: the caller zeroes them.
extern "C" int mspl_uw_loss_heads_meters_fwd_bwd(const float* main_lo, const float* aux_lo, const int64_t* target, const float* class_weights,
                                                 int32_t N, int32_t C, int32_t Hm, int32_t Wm, int32_t Ha, int32_t Wa, int32_t H, int32_t W,
                                                 float ce_scale, float out_scale, float* loss_acc, float* gpred, float* gaux,
                                                 int32_t miou_classes, float meter_weight, unsigned long long* areas, double* meter, void* stream) {
    MSPL_REQUIRE(areas && meter, MSPL_ERR_NULL_POINTER, "uw_loss_heads_meters: null pointer");
    MSPL_REQUIRE(miou_classes >= 1 && miou_classes <= 64, MSPL_ERR_UNSUPPORTED, "uw_loss_heads_meters: %d classes (1..64)", miou_classes);
    const UhMeters mt{areas, meter, miou_classes, meter_weight};
    return uh_launch(main_lo, aux_lo, target, class_weights, N, C, Hm, Wm, Ha, Wa, H, W, ce_scale, out_scale, loss_acc, gpred, gaux, &mt, stream);
}
