// The loss, the meters and the logit gradient of one train_seg iteration (utilities/train_eval_seg.py:44-47, :57) taken from the
// decoder's single low-resolution head BEFORE its bilinear up-sampling (model/segmentation/espnetv2.py / espdnet.py: the last line of
// forward(), F.interpolate(..., mode='bilinear', align_corners=True) to the input size):
//     loss  = CrossEntropyLoss(weight, ignore_index)(up(head), target)       = sum_valid w[t] * (lse(o) - o[t]) / sum_valid w[t]
//     areas = MIOU(num_classes - 1).get_iou(up(head), target)                first maximum, the reference's uint8 +1 arithmetic
//     d loss / d up(head), unnormalised                                       w[t] * (softmax(o) - onehot(t)), zero where invalid
// The form built from the existing kernels writes the full-size logits (mspl_resize_bilinear), reads them for the sums and areas
// (mspl_ce_meters_fwd), reads them again and writes a full-size gradient (mspl_weighted_ce_bwd) and reads that (mspl_bilinear_bwd):
// five passes over N*C*H*W floats.  Here, as in uw_loss_heads.hip with one head, a workgroup owns a band of TH rows x 256 columns of
// the label map, stages the patch of the head that band interpolates from in LDS and evaluates the up-sampled logits per pixel with
// mspl_resize_bilinear's own expression (wy0 * (wx0 * a + wx1 * b) + wy1 * (...)): the full-size logits never exist, and the
// gradient leaves at label resolution for mspl_bilinear_bwd.  CrossEntropyLoss divides by the sum of the valid weights, known only
// after the whole pass, so the gradient is written WITHOUT that factor: the caller multiplies the small (N,C,Hm,Wm) result of the
// transposed interpolation (which is linear) by upstream / sums[1].
//
// The cross-entropy term is the centred one, w * (log S - (o_t - m)) with S = sum exp(o_c - m): both parts are small wherever the
// pixel is classified right, whatever the size of the logits (DESIGN section 2 on `x - (max + log sum)`).
//
// Build log (-Rpass-analysis=kernel-resource-usage, gfx950), <CM, EXACT, GRAD>: VGPRs / scratch bytes
//     <5,true,false> 54 / 0     <5,true,true> 57 / 0     <8,false,false> 64 / 0     <8,false,true> 75 / 0
//     <13,true,false> 75 / 0    <13,true,true> 88 / 0    <20,true,false> 96 / 0     <20,true,true> 117 / 0
// (832 bytes of static LDS each: the 3 x 64 area counters and the partial sums)
#include <algorithm>

#include "common.hpp"
#include "loss_parts.hpp"

namespace mspl {

struct ChGeom {
    int N, C, H, W;
    int Hm, Wm;                     // the head
    float sh, sw;                   // bilinear scales (align_corners=True)
    int TH, tiles_x, tiles_y;       // band height; 256-column tiles per row; bands per image
    int MR, MC;                     // LDS patch capacity (rows, columns)
    unsigned total;                 // tiles
    int ignore, K;
};

constexpr int CH_TW = 256;
constexpr size_t CH_LDS_BUDGET = 62 * 1024;        // dynamic LDS: the static counters and partial sums (under 1 KB) come on top

// CM: class capacity of the register array; EXACT: C == CM (no per-class predicates).  Up to 8 classes the exponentials are kept from
// the sum to the gradient; beyond, they are recomputed (uw_loss_heads.hip).  GRAD: write gfull.  areas == nullptr: no histograms.
template <int CM, bool EXACT, bool GRAD>
__global__ __launch_bounds__(256) void ce_head_kernel(const float* __restrict__ head, const int64_t* __restrict__ target,
                                                      const float* __restrict__ cw, ChGeom g, double* __restrict__ sums,
                                                      unsigned long long* __restrict__ areas, float* __restrict__ gfull) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    // (The area counters, the row tally and the sums reduction stay written out here: through loss_parts.hpp's miou_* helpers and
    // ce_sums_reduce the forward-only <20,true,false> measured 133.8 against 133.1 us at 16 x 20 x 256x480, with the band helpers
    // alone 133.0.  A change of the rule there is a change here.)
    __shared__ unsigned int mhist[3 * MIOU_MAX_BINS];
    __shared__ double red[2][4];
    const bool meters = areas != nullptr;
    if (meters) {
        for (int i = threadIdx.x; i < 3 * g.K; i += 256) mhist[i] = 0;       // (ordered before its first use by the tile loop's barrier)
    }
    const int C = EXACT ? CM : g.C;
    constexpr bool KEEP = GRAD && CM <= 8;
    constexpr int CK = KEEP ? CM : 1;
    const int msz = g.MR * g.MC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s_loss = 0.0, s_w = 0.0;
    for (unsigned tile = blockIdx.x; tile < g.total; tile += gridDim.x) {
        const BandTile bt = band_tile(tile, g.tiles_x, g.tiles_y, g.TH, CH_TW, g.H, g.W);
        const int img = bt.img, y0 = bt.y0, x0 = bt.x0, rows = bt.rows;
        const BandPatch pt = band_patch(g.sh, g.sw, g.Hm, g.Wm, bt, g.MR, g.MC);
        const int my0 = pt.y0, mx0 = pt.x0, nmr = pt.nr, nmc = pt.nc;
        band_stage(sm, head, img, C, g.Hm, g.Wm, pt, g.MC, msz, wave, lane);
        __syncthreads();
        for (int r = wave; r < rows; r += 4) {
            const int y = y0 + r;
            int ya, yb;  float wy0, wy1;
            bilinear_src(g.sh, y, g.Hm, ya, yb, wy0, wy1);
            // (clamped like the staging: an index can never leave the patch, whatever the two evaluations of the rule give)
            const int rm0 = min(ya - my0, nmr - 1) * g.MC, rm1 = min(yb - my0, nmr - 1) * g.MC;
            const size_t rowoff = ((size_t)img * g.H + y) * (size_t)g.W;
            const size_t goff = ((size_t)img * C * g.H + y) * (size_t)g.W;
            const size_t hw = (size_t)g.H * g.W;
            // a wave takes the row's 256 columns as four runs of 64 (coalesced label loads and gradient stores), one pixel per lane at a time
            unsigned pk_p = 0, pk_g = 0;     // the row's four (p, g) codes, a byte each; 0 counts nowhere
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int xs = x0 + j * 64 + lane;
                if (xs >= g.W) continue;
                const int64_t t64 = target[rowoff + xs];
                const bool valid = t64 >= 0 && t64 < (int64_t)C && t64 != (int64_t)g.ignore;
                const int t = valid ? (int)t64 : -1;
                int xa, xb;  float wx0, wx1;
                bilinear_src(g.sw, xs, g.Wm, xa, xb, wx0, wx1);
                const int ca = min(xa - mx0, nmc - 1), cb = min(xb - mx0, nmc - 1);
                const int m00 = rm0 + ca, m01 = rm0 + cb, m10 = rm1 + ca, m11 = rm1 + cb;
                float a[CM];
                float m = -INFINITY;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (EXACT || c < C) {
                        const float* pm = sm + c * msz;
                        const float top = wx0 * pm[m00] + wx1 * pm[m01], bot = wx0 * pm[m10] + wx1 * pm[m11];
                        a[c] = wy0 * top + wy1 * bot;
                        m = fmaxf(m, a[c]);
                    }
                }
                if (meters) {
                    float best = a[0];  unsigned bi = 0;
#pragma unroll
                    for (int c = 1; c < CM; ++c)
                        if ((EXACT || c < C) && a[c] > best) { best = a[c];  bi = (unsigned)c; }
                    const unsigned g8 = ((unsigned)(t64 & 255) + 1u) & 255u;
                    const unsigned p8 = g8 ? ((bi + 1u) & 255u) : 0u;
                    pk_p |= p8 << (8 * j);
                    pk_g |= g8 << (8 * j);
                }
                float e[CK];
                float S = 0.f, dt = 0.f;                 // dt = o_t - m
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (EXACT || c < C) {
                        const float d = a[c] - m;
                        const float x = expf(d);
                        if (KEEP) e[KEEP ? c : 0] = x;
                        S += x;
                        if (c == t) dt = d;
                    }
                }
                const float w = valid ? (cw ? cw[t] : 1.f) : 0.f;
                if (valid) {
                    s_loss += (double)(w * (logf(S) - dt));
                    s_w += (double)w;
                }
                if (GRAD) {
                    const float rw = w / S;             // (0 for an invalid pixel: its gradient is zeros)
                    float* dp = gfull + goff + xs;
#pragma unroll
                    for (int c = 0; c < CM; ++c) {
                        if (EXACT || c < C) {
                            const float x = KEEP ? e[KEEP ? c : 0] : expf(a[c] - m);
                            dp[c * hw] = valid ? (rw * x - (c == t ? w : 0.f)) : 0.f;
                        }
                    }
                }
            }
            if (meters) {
                const unsigned eq = pk_p ^ pk_g;                        // a zero byte: p == g, the intersection carries p
                for (unsigned k = 1; k <= (unsigned)g.K; ++k) {
                    unsigned ci = 0, cp = 0, cg = 0;                     // wave-uniform
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool isp = ((pk_p >> (8 * j)) & 0xffu) == k, isg = ((pk_g >> (8 * j)) & 0xffu) == k;
                        cp += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(isp));
                        cg += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(isg));
                        ci += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(isp && ((eq >> (8 * j)) & 0xffu) == 0u));
                    }
                    if (lane == 0) {
                        if (ci) atomicAdd(&mhist[k - 1], ci);
                        if (cp) atomicAdd(&mhist[g.K + k - 1], cp);
                        if (cg) atomicAdd(&mhist[2 * g.K + k - 1], cg);
                    }
                }
            }
        }
        __syncthreads();                 // the next tile's staging overwrites the patch
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s_loss += __shfl_down(s_loss, o, 64);  s_w += __shfl_down(s_w, o, 64); }
    if (lane == 0) { red[0][wave] = s_loss;  red[1][wave] = s_w; }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&sums[0], (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
        atomicAdd(&sums[1], (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    }
    // (the barrier above ordered every wave's LDS adds; a workgroup with no tile has only zeros)
    if (meters)
        for (int i = tid; i < 3 * g.K; i += 256)
            if (mhist[i]) atomicAdd(&areas[i], (unsigned long long)mhist[i]);
}

static bool ch_classes(int C) { return (C >= 1 && C <= 8) || C == 13 || C == 20; }

// The launcher's plan: everything that can refuse a geometry, decided before anything is launched.  Returns MSPL_OK and fills g / lds,
// or the error code with `why` pointing at a static reason.
static int ch_plan(int N, int C, int Hm, int Wm, int H, int W, ChGeom& g, size_t& lds, const char*& why) {
    why = "";
    if (!(N > 0 && C > 0 && H > 0 && W > 0 && Hm > 0 && Wm > 0)) { why = "bad shape";  return MSPL_ERR_BAD_SHAPE; }
    if (!ch_classes(C)) { why = "class count (built for 1..8, 13, 20)";  return MSPL_ERR_UNSUPPORTED; }
    if (Hm > H || Wm > W) { why = "head larger than the label map";  return MSPL_ERR_UNSUPPORTED; }
    if ((int64_t)N * C * H * W >= (1ll << 40)) { why = "too large";  return MSPL_ERR_BAD_SHAPE; }
    g.N = N; g.C = C; g.H = H; g.W = W; g.Hm = Hm; g.Wm = Wm;
    g.sh = bilinear_scale(Hm, H);  g.sw = bilinear_scale(Wm, W);
    g.tiles_x = ceil_div(W, CH_TW);
    g.TH = band_height(N, H, g.tiles_x, CH_LDS_BUDGET, [&](int th) {
        g.MR = bilinear_span(Hm, H, th);  g.MC = bilinear_span(Wm, W, CH_TW) | 1;
        return lds = (size_t)C * (size_t)g.MR * g.MC * sizeof(float);
    });
    if (lds > CH_LDS_BUDGET) { why = "the head's patch does not fit LDS";  return MSPL_ERR_UNSUPPORTED; }
    g.tiles_y = ceil_div(H, g.TH);
    const int64_t tiles = (int64_t)N * g.tiles_y * g.tiles_x;
    if (tiles >= (1ll << 31)) { why = "too many tiles";  return MSPL_ERR_BAD_SHAPE; }
    g.total = (unsigned)tiles;
    return MSPL_OK;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_ce_head_supported(int32_t C) { return ch_classes(C) ? 1 : 0; }

extern "C" int mspl_ce_head_fits(int32_t N, int32_t C, int32_t Hm, int32_t Wm, int32_t H, int32_t W) {
    ChGeom g;  size_t lds = 0;  const char* why;
    return ch_plan(N, C, Hm, Wm, H, W, g, lds, why) == MSPL_OK ? 1 : 0;
}

extern "C" int mspl_ce_head_meters_fwd_bwd(const float* head, const int64_t* target, const float* class_weights, int32_t ignore_index,
                                           int32_t N, int32_t C, int32_t Hm, int32_t Wm, int32_t H, int32_t W, int32_t miou_classes,
                                           double* sums, unsigned long long* areas, float* ghead_full, void* stream) {
    MSPL_REQUIRE(head && target && sums, MSPL_ERR_NULL_POINTER, "ce_head: null pointer");
    MSPL_REQUIRE(!areas || (miou_classes >= 1 && miou_classes <= 64), MSPL_ERR_UNSUPPORTED, "ce_head: %d MIOU classes (1..64)", miou_classes);
    ChGeom g;  size_t lds = 0;  const char* why;
    const int rc = ch_plan(N, C, Hm, Wm, H, W, g, lds, why);
    MSPL_REQUIRE(rc == MSPL_OK, rc, "ce_head: %s (N=%d C=%d head %dx%d labels %dx%d: use the up-sampled form)", why, N, C, Hm, Wm, H, W);
    g.ignore = ignore_index;
    g.K = areas ? miou_classes : 0;
    // two same-address double atomics per workgroup: a bounded grid walks the tiles (uw_loss_heads.hip)
    const unsigned blocks = (unsigned)std::min<int64_t>((int64_t)g.total, 1536);
    hipStream_t s = (hipStream_t)stream;
#define MSPL_CH(CMv, EX)                                                                                                                        \
    do {                                                                                                                                        \
        if (ghead_full) hipLaunchKernelGGL((ce_head_kernel<CMv, EX, true>), dim3(blocks), dim3(256), lds, s, head, target, class_weights, g, sums, areas, ghead_full); \
        else hipLaunchKernelGGL((ce_head_kernel<CMv, EX, false>), dim3(blocks), dim3(256), lds, s, head, target, class_weights, g, sums, areas, ghead_full); \
    } while (0)
    if (C == 5) MSPL_CH(5, true);
    else if (C <= 8) MSPL_CH(8, false);
    else if (C == 13) MSPL_CH(13, true);
    else MSPL_CH(20, true);
#undef MSPL_CH
    MSPL_CHECK_LAUNCH("ce_head_meters_fwd_bwd");
    return MSPL_OK;
}
