// NIDLoss at head resolution: NIDLoss(camera, F.interpolate(main_lo, (H, W), mode='bilinear', align_corners=True))
// (loss_fns/segmentation_loss.py:54-144 composed with model/segmentation/espdnet_ue.py:301) from the decoder's low-resolution main
// head, without a (B,C,H,W) tensor in either direction.  The three-step form (mspl_bilinear_fwd, mspl_nid_hist_fwd / _bwd,
// mspl_bilinear_bwd) writes the full-size logits, reads them twice and writes and folds a full-size gradient.
//
// Forward: a workgroup owns a band of NH_TH rows x NH_TW columns of label-map POSITIONS (256, one per thread) and loops over the B
// images inside it -- the reference sums P_c and P_l over the batch per position before the outer product (:86-96), so the batch
// cannot be split across workgroups.  Per image it stages the head patch the band interpolates from (loss_parts.hpp), evaluates
// the up-sampled logits with the expression of mspl_bilinear_fwd (wy0 * (wx0 * a + wx1 * b) + wy1 * (...)) into a per-thread LDS
// column and hands that column to the helpers of nid_parts.hpp -- the code nid.hip runs on a full-size tensor.  Per-workgroup
// partials, then the fixed-order sum in double of nid_reduce_kernel: no float atomics, two runs are bit-identical.  The camera
// columns P_c[k,p] depend on the batch alone; they are left in the workspace for the backward (K*H*W floats: 15.7 MB at K = 32,
// 256x480, written and read once, against B * 2 K sigmoids per position to recompute them).
//
// mspl_nid_finalize: the K x Cl entropy arithmetic (:98-118) and its closed-form derivative in one workgroup, in double.
//
// Backward: same bands.  dL/d lab per image as in nid_bwd_kernel (the shared helpers again), and where it is not exactly zero -- with
// beta = 500 and bw_label = 1e-3 that is near ties of adjacent classes only -- the soft-arg-max Jacobian times the four
// interpolation weights is added to an LDS accumulator of the patch's shape (LDS float atomics; few pixels take this branch), and the
// patch's non-zero entries are added to gmain_lo with global float atomics (patches of neighbouring bands overlap by a row / column).
// The backward is therefore not bit-reproducible from run to run, like the project's other gradient sinks.
#include <algorithm>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "loss_parts.hpp"
#include "nid_parts.hpp"

namespace mspl {

constexpr int NH_TH = 4, NH_TW = 64;              // the band: a wave per row, a lane per column
static_assert(NH_TH * NH_TW == NID_POS, "one position per thread");
constexpr size_t NH_LDS_BUDGET = 128 * 1024;

struct NhGeom {
    int B, C, K, Cl, H, W, Hm, Wm;
    float sh, sw;                   // bilinear scales (align_corners=True)
    int tiles_x, tiles_y;           // bands per row of bands / per column
    int MR, MC;                     // LDS patch capacity (rows, columns)
    float bw_c, bw_l, beta;
};

// where a thread's position interpolates from, as offsets into a [MR][MC] patch plane
struct NhTaps { int m00, m01, m10, m11; float wy0, wy1, wx0, wx1; };

__device__ __forceinline__ NhTaps nh_taps(const NhGeom& g, const BandPatch& pm, int y, int x) {
    NhTaps q;
    int ya, yb, xa, xb;
    bilinear_src(g.sh, y, g.Hm, ya, yb, q.wy0, q.wy1);
    bilinear_src(g.sw, x, g.Wm, xa, xb, q.wx0, q.wx1);
    const int r0 = (ya - pm.y0) * g.MC - pm.x0, r1 = (yb - pm.y0) * g.MC - pm.x0;
    q.m00 = r0 + xa;  q.m01 = r0 + xb;  q.m10 = r1 + xa;  q.m11 = r1 + xb;
    return q;
}

// the position's C up-sampled logits of the staged image into its column A[.][t]: operations and order of mspl_bilinear_fwd
__device__ __forceinline__ void nh_interpolate(float* A, const float* LM, int msz, int C, const NhTaps& q, int t) {
    for (int c = 0; c < C; ++c) {
        const float* p = LM + c * msz;
        const float top = q.wx0 * p[q.m00] + q.wx1 * p[q.m01], bot = q.wx0 * p[q.m10] + q.wx1 * p[q.m11];
        A[c * NID_POS + t] = q.wy0 * top + q.wy1 * bot;
    }
}

// partial: (bands, K*Cl + K + Cl); pc_cols: (K, H*W), the camera columns for the backward
__global__ __launch_bounds__(256) void nid_heads_fwd_kernel(const float* __restrict__ cam, const float* __restrict__ mainp, NhGeom g,
                                                            float* __restrict__ partial, float* __restrict__ pc_cols) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int msz = g.MR * g.MC;
    float* As = sm;                              // [K][256]  camera columns
    float* Ls = As + g.K * NID_POS;              // [Cl][256] label columns
    float* A = Ls + g.Cl * NID_POS;              // [C][256]  up-sampled logits of the current image
    float* LM = A + g.C * NID_POS;               // [C][MR][MC] head patch of the current image
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const BandTile bt = band_tile(blockIdx.x, g.tiles_x, g.tiles_y, NH_TH, NH_TW, g.H, g.W);       // (its image index is 0)
    const BandPatch pm = band_patch(g.sh, g.sw, g.Hm, g.Wm, bt, g.MR, g.MC);
    const bool live = wave < bt.rows && lane < bt.cols;
    const int y = bt.y0 + wave, x = bt.x0 + lane;
    const size_t P = (size_t)g.H * g.W, p = (size_t)y * g.W + x;
    for (int k = 0; k < g.K; ++k) As[k * NID_POS + t] = 0.f;
    for (int c = 0; c < g.Cl; ++c) Ls[c * NID_POS + t] = 0.f;
    NhTaps q = {};
    if (live) q = nh_taps(g, pm, y, x);
    for (int b = 0; b < g.B; ++b) {
        band_stage(LM, mainp, b, g.C, g.Hm, g.Wm, pm, g.MC, msz, wave, lane);
        __syncthreads();
        if (live) {
            nh_interpolate(A, LM, msz, g.C, q, t);
            nid_camera_add(As, t, nid_gray(cam + (size_t)b * 3 * P + p, P), g.K, g.bw_c);
            nid_label_add(Ls, t, soft_arg_max(A + t, g.C, (size_t)NID_POS, g.beta, 1e-12f), g.Cl, g.bw_l);
        }
        __syncthreads();                         // the next image's staging overwrites the patch; orders the columns for the sums
    }
    if (live)
        for (int k = 0; k < g.K; ++k) pc_cols[(size_t)k * P + p] = As[k * NID_POS + t];
    nid_partial_sums(As, Ls, g.K, g.Cl, partial + (size_t)blockIdx.x * (g.K * g.Cl + g.K + g.Cl));
}

// gj (K, Cl), gpl (Cl): dL/d joint, dL/d p_l already divided by B*H*W.  gmain (B, C, Hm, Wm): accumulated into.
__global__ __launch_bounds__(256) void nid_heads_bwd_kernel(const float* __restrict__ mainp, NhGeom g, const float* __restrict__ pc_cols,
                                                            const float* __restrict__ gj, const float* __restrict__ gpl,
                                                            const float* __restrict__ gscale, float* __restrict__ gmain) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int msz = g.MR * g.MC;
    float* R = sm;                               // [max(K, C)][256] the camera column, then the current image's up-sampled logits
    float* Gl = R + max(g.K, g.C) * NID_POS;     // [Cl][256] dL/dP_l
    float* LM = Gl + g.Cl * NID_POS;             // [C][MR][MC] head patch
    float* PG = LM + g.C * msz;                  // [C][MR][MC] its gradient
    float* Gj = PG + g.C * msz;                  // [K][Cl]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const BandTile bt = band_tile(blockIdx.x, g.tiles_x, g.tiles_y, NH_TH, NH_TW, g.H, g.W);
    const BandPatch pm = band_patch(g.sh, g.sw, g.Hm, g.Wm, bt, g.MR, g.MC);
    const bool live = wave < bt.rows && lane < bt.cols;
    const int y = bt.y0 + wave, x = bt.x0 + lane;
    const size_t P = (size_t)g.H * g.W, p = (size_t)y * g.W + x;
    for (int i = t; i < g.K * g.Cl; i += 256) Gj[i] = gj[i];
    if (live)
        for (int k = 0; k < g.K; ++k) R[k * NID_POS + t] = pc_cols[(size_t)k * P + p];
    __syncthreads();
    NhTaps q = {};
    if (live) {
        nid_label_grad_column(Gl, R, Gj, gpl, t, g.K, g.Cl);      // (R and Gl columns are the thread's own: no barrier before R is reused)
        q = nh_taps(g, pm, y, x);
    }
    const float gs = gscale ? gscale[0] : 1.0f;
    const int pn = pm.nr * pm.nc;
    for (int b = 0; b < g.B; ++b) {
        band_stage(LM, mainp, b, g.C, g.Hm, g.Wm, pm, g.MC, msz, wave, lane);
        for (int i = t; i < g.C * msz; i += 256) PG[i] = 0.f;
        __syncthreads();
        if (live) {
            nh_interpolate(R, LM, msz, g.C, q, t);
            const NidLab r = nid_dlab(R + t, g.C, (size_t)NID_POS, Gl, t, g.Cl, g.beta, g.bw_l);
            if (r.dv != 0.f) {                   // exactly zero away from near-ties of adjacent classes
                for (int j = 0; j < g.C; ++j) {
                    const float gv = nid_dlogit(r, R[j * NID_POS + t], j, g.beta) * gs;
                    if (gv == 0.f) continue;
                    float* pg = PG + j * msz;
                    atomicAdd(&pg[q.m00], (q.wy0 * q.wx0) * gv);
                    atomicAdd(&pg[q.m01], (q.wy0 * q.wx1) * gv);
                    atomicAdd(&pg[q.m10], (q.wy1 * q.wx0) * gv);
                    atomicAdd(&pg[q.m11], (q.wy1 * q.wx1) * gv);
                }
            }
        }
        __syncthreads();
        for (int i = t; i < g.C * pn; i += 256) {
            const int c = i / pn, rem = i - c * pn, rr = rem / pm.nc, xx = rem - rr * pm.nc;
            const float v = PG[c * msz + rr * g.MC + xx];
            if (v != 0.f) atomicAdd(&gmain[(((size_t)b * g.C + c) * g.Hm + pm.y0 + rr) * (size_t)g.Wm + pm.x0 + xx], v);
        }
        __syncthreads();                         // the next image's staging and zero fill overwrite both patches
    }
}

// out: joint (K, Cl) | p_c (K) | p_l (Cl) as mspl_nid_hist_fwd leaves them; n = min(label_bin, Cl) label bins enter the loss (the
// reference's bins beyond Cl are never filled: they add nothing to any sum).  One workgroup.
__device__ __forceinline__ double nf_block_sum(double v, double* red) {
    __syncthreads();                             // (red may still be read from the sum before)
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void nid_finalize_kernel(const float* __restrict__ out, int K, int Cl, int n, double inv_norm,
                                                           float* __restrict__ loss2, float* __restrict__ gjoint, float* __restrict__ gpl) {
    __shared__ double red[256];
    __shared__ double gl[NID_MAXB];
    const int t = threadIdx.x;
    const double eps = 1e-7;
    const float* J = out;
    const float* pc = out + K * Cl;
    const float* pl = pc + K;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = t; i < K * n; i += 256) a += (double)J[(i / n) * Cl + i % n];
    for (int i = t; i < K; i += 256) b += (double)pc[i];
    for (int i = t; i < n; i += 256) c += (double)pl[i];
    const double sJ = nf_block_sum(a, red), sc = nf_block_sum(b, red), sl = nf_block_sum(c, red);
    double vi = 0.0, vh = 0.0;
    for (int i = t; i < K * n; i += 256) {
        const int k = i / n, l = i % n;
        const double j = (double)J[k * Cl + l] / sJ, m = ((double)pc[k] / sc) * ((double)pl[l] / sl);
        vi += j * (log(j + eps) - log(m + eps));
        vh -= j * log(j + eps);
    }
    const double I = nf_block_sum(vi, red), Hh = nf_block_sum(vh, red);
    // loss2 = ((1 - I / Hh) - 0.95) * 20
    const double dI = -20.0 / Hh, dH = 20.0 * I / (Hh * Hh);
    if (t == 0) loss2[0] = (float)(((1.0 - I / Hh) - 0.95) * 20.0);
    // d loss2 / d (normalised) p_l[l] = dI * -sum_k j[k,l] c[k] / (c[k] l[l] + eps)
    if (t < n) {
        double s = 0.0;
        const double ln = (double)pl[t] / sl;
        for (int k = 0; k < K; ++k) {
            const double cn = (double)pc[k] / sc;
            s -= ((double)J[k * Cl + t] / sJ) * cn / (cn * ln + eps);
        }
        gl[t] = dI * s;
    }
    double dj = 0.0, dl = 0.0;                  // sum g * normalised value: the normalisations' own derivative
    for (int i = t; i < K * n; i += 256) {
        const int k = i / n, l = i % n;
        const double j = (double)J[k * Cl + l] / sJ, m = ((double)pc[k] / sc) * ((double)pl[l] / sl);
        const double lg = log(j + eps), q = j / (j + eps);
        dj += (dI * (lg - log(m + eps) + q) - dH * (lg + q)) * j;
    }
    __syncthreads();                             // gl
    if (t < n) dl = gl[t] * ((double)pl[t] / sl);
    const double sdj = nf_block_sum(dj, red), sdl = nf_block_sum(dl, red);
    for (int i = t; i < K * Cl; i += 256) {
        const int k = i / Cl, l = i % Cl;
        double gv = 0.0;
        if (l < n) {
            const double j = (double)J[i] / sJ, m = ((double)pc[k] / sc) * ((double)pl[l] / sl);
            const double lg = log(j + eps), q = j / (j + eps);
            gv = ((dI * (lg - log(m + eps) + q) - dH * (lg + q)) - sdj) / sJ;
        }
        gjoint[i] = (float)(gv * inv_norm);
    }
    if (t < Cl) gpl[t] = t < n ? (float)((gl[t] - sdl) / sl * inv_norm) : 0.f;
}

// The one place the shape is judged and the band sized: the launchers and mspl_nid_heads_plan call it.
struct NhPlan { NhGeom g; size_t lds_fwd, lds_bwd; int fan; };

// most label positions along one axis whose two sources include one given head position
static int nh_fan(int in_size, int out_size) {
    const float sc = bilinear_scale(in_size, out_size);
    int most = 0;
    std::vector<int> cnt((size_t)in_size, 0);
    for (int o = 0; o < out_size; ++o) {
        int i0, i1;
        bilinear_src_host(sc, o, in_size, i0, i1);
        ++cnt[i0];
        if (i1 != i0) ++cnt[i1];
    }
    for (int i = 0; i < in_size; ++i) most = std::max(most, cnt[i]);
    return most;
}

static int nh_plan(NhPlan& pl, int B, int C, int Hm, int Wm, int H, int W, int K, float bw_c, float bw_l, const char* who) {
    MSPL_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && Hm > 0 && Wm > 0 && K > 0, MSPL_ERR_BAD_SHAPE,
                 "%s: bad shape B=%d C=%d head %dx%d labels %dx%d K=%d", who, B, C, Hm, Wm, H, W, K);
    MSPL_REQUIRE(bw_c > 0.f && bw_l > 0.f, MSPL_ERR_BAD_SHAPE, "%s: bandwidths must be positive", who);
    MSPL_REQUIRE((int64_t)H * W < (1ll << 31) && (int64_t)B * C * H * W < (1ll << 40), MSPL_ERR_BAD_SHAPE, "%s: too large", who);
    MSPL_REQUIRE(K <= NID_MAXB && C <= NID_MAXB, MSPL_ERR_UNSUPPORTED, "%s: at most %d image bins and classes (got %d, %d)", who, NID_MAXB, K, C);
    MSPL_REQUIRE(Hm <= H && Wm <= W, MSPL_ERR_UNSUPPORTED, "%s: head %dx%d larger than the label map %dx%d", who, Hm, Wm, H, W);
    NhGeom& g = pl.g;
    g.B = B; g.C = C; g.K = K; g.Cl = C < K ? C : K; g.H = H; g.W = W; g.Hm = Hm; g.Wm = Wm;
    g.sh = bilinear_scale(Hm, H); g.sw = bilinear_scale(Wm, W);
    g.tiles_x = ceil_div(W, NH_TW); g.tiles_y = ceil_div(H, NH_TH);
    g.MR = bilinear_span(Hm, H, NH_TH); g.MC = bilinear_span(Wm, W, NH_TW) | 1;
    g.bw_c = bw_c; g.bw_l = bw_l; g.beta = 500.0f;
    const size_t msz = (size_t)g.MR * g.MC;
    pl.lds_fwd = ((size_t)(g.K + g.Cl + g.C) * NID_POS + (size_t)g.C * msz) * sizeof(float);
    pl.lds_bwd = ((size_t)(std::max(g.K, g.C) + g.Cl) * NID_POS + 2 * (size_t)g.C * msz + (size_t)g.K * g.Cl) * sizeof(float);
    MSPL_REQUIRE(std::max(pl.lds_fwd, pl.lds_bwd) <= NH_LDS_BUDGET, MSPL_ERR_UNSUPPORTED, "%s: columns and patches of %zu bytes exceed the LDS budget",
                 who, std::max(pl.lds_fwd, pl.lds_bwd));
    MSPL_REQUIRE((int64_t)g.tiles_x * g.tiles_y < (1ll << 31), MSPL_ERR_BAD_SHAPE, "%s: too many bands", who);
    pl.fan = nh_fan(Hm, H) * nh_fan(Wm, W);
    return MSPL_OK;
}

static bool nh_large_lds() {
    static std::once_flag once;
    static bool ok = false;
    std::call_once(once, [] {
        ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&nid_heads_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NH_LDS_BUDGET) == hipSuccess &&
             hipFuncSetAttribute(reinterpret_cast<const void*>(&nid_heads_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NH_LDS_BUDGET) == hipSuccess;
    });
    return ok;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_nid_heads_plan(int32_t B, int32_t C, int32_t Hm, int32_t Wm, int32_t H, int32_t W, int32_t K, int32_t* out) {
    MSPL_REQUIRE(out, MSPL_ERR_NULL_POINTER, "nid_heads_plan: null pointer");
    for (int i = 0; i < MSPL_NH_PLAN_LEN; ++i) out[i] = 0;
    NhPlan pl;
    if (int rc = nh_plan(pl, B, C, Hm, Wm, H, W, K, 1.f, 1.f, "nid_heads_plan")) return rc;
    out[MSPL_NH_PLAN_BAND_ROWS] = NH_TH;
    out[MSPL_NH_PLAN_BAND_COLS] = NH_TW;
    out[MSPL_NH_PLAN_PATCH_ROWS] = pl.g.MR;
    out[MSPL_NH_PLAN_PATCH_COLS] = pl.g.MC;
    out[MSPL_NH_PLAN_LDS_FWD] = (int32_t)pl.lds_fwd;
    out[MSPL_NH_PLAN_LDS_BWD] = (int32_t)pl.lds_bwd;
    out[MSPL_NH_PLAN_BANDS] = pl.g.tiles_x * pl.g.tiles_y;
    out[MSPL_NH_PLAN_FAN] = pl.fan;
    return MSPL_OK;
}

extern "C" int64_t mspl_nid_heads_workspace_floats(int32_t C, int32_t H, int32_t W, int32_t K) {
    if (C <= 0 || H <= 0 || W <= 0 || K <= 0) return MSPL_ERR_BAD_SHAPE;
    const int Cl = C < K ? C : K;
    return (int64_t)ceil_div(W, NH_TW) * ceil_div(H, NH_TH) * (K * Cl + K + Cl) + (int64_t)K * H * W;
}

extern "C" int mspl_nid_heads_fwd(const float* camera, const float* main_lo, int32_t B, int32_t C, int32_t Hm, int32_t Wm, int32_t H,
                                  int32_t W, int32_t K, float bw_camera, float bw_label, float* ws, float* out, void* stream) {
    NhPlan pl;
    if (int rc = nh_plan(pl, B, C, Hm, Wm, H, W, K, bw_camera, bw_label, "nid_heads_fwd")) return rc;
    MSPL_REQUIRE(camera && main_lo && ws && out, MSPL_ERR_NULL_POINTER, "nid_heads_fwd: null pointer");
    MSPL_REQUIRE(pl.lds_fwd <= 64 * 1024 || nh_large_lds(), MSPL_ERR_HIP, "nid_heads_fwd: %zu bytes of LDS refused by the runtime", pl.lds_fwd);
    const NhGeom& g = pl.g;
    const int bands = g.tiles_x * g.tiles_y, E = g.K * g.Cl + g.K + g.Cl;
    float* pc_cols = ws + (size_t)bands * E;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nid_heads_fwd_kernel, dim3((unsigned)bands), dim3(256), pl.lds_fwd, s, camera, main_lo, g, ws, pc_cols);
    MSPL_CHECK_LAUNCH("nid_heads_fwd");
    hipLaunchKernelGGL(nid_reduce_kernel, dim3((unsigned)ceil_div(E, 256)), dim3(256), 0, s, ws, bands, E, 1.0 / ((double)g.H * g.W * B), out);
    MSPL_CHECK_LAUNCH("nid_heads_fwd(reduce)");
    return MSPL_OK;
}

extern "C" int mspl_nid_finalize(const float* out, int32_t K, int32_t C, int32_t label_bin, double norm, float* loss2, float* gjoint,
                                 float* gpl, void* stream) {
    MSPL_REQUIRE(out && loss2 && gjoint && gpl, MSPL_ERR_NULL_POINTER, "nid_finalize: null pointer");
    MSPL_REQUIRE(K > 0 && C > 0 && label_bin > 0 && norm > 0.0, MSPL_ERR_BAD_SHAPE, "nid_finalize: bad shape K=%d C=%d label_bin=%d", K, C, label_bin);
    MSPL_REQUIRE(K <= NID_MAXB && C <= NID_MAXB, MSPL_ERR_UNSUPPORTED, "nid_finalize: at most %d image bins and classes (got %d, %d)", NID_MAXB, K, C);
    MSPL_REQUIRE(label_bin <= C, MSPL_ERR_BAD_SHAPE, "nid_finalize: label_bin=%d above the %d classes of the logits", label_bin, C);
    const int Cl = C < K ? C : K, n = label_bin < Cl ? label_bin : Cl;
    hipLaunchKernelGGL(nid_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out, K, Cl, n, 1.0 / norm, loss2, gjoint, gpl);
    MSPL_CHECK_LAUNCH("nid_finalize");
    return MSPL_OK;
}

extern "C" int mspl_nid_heads_bwd(const float* main_lo, int32_t B, int32_t C, int32_t Hm, int32_t Wm, int32_t H, int32_t W, int32_t K,
                                  float bw_label, const float* ws, const float* gjoint, const float* gpl, const float* gscale,
                                  float* gmain_lo, void* stream) {
    NhPlan pl;
    if (int rc = nh_plan(pl, B, C, Hm, Wm, H, W, K, 1.f, bw_label, "nid_heads_bwd")) return rc;
    MSPL_REQUIRE(main_lo && ws && gjoint && gpl && gmain_lo, MSPL_ERR_NULL_POINTER, "nid_heads_bwd: null pointer");
    MSPL_REQUIRE(pl.lds_bwd <= 64 * 1024 || nh_large_lds(), MSPL_ERR_HIP, "nid_heads_bwd: %zu bytes of LDS refused by the runtime", pl.lds_bwd);
    const NhGeom& g = pl.g;
    const int bands = g.tiles_x * g.tiles_y, E = g.K * g.Cl + g.K + g.Cl;
    hipLaunchKernelGGL(nid_heads_bwd_kernel, dim3((unsigned)bands), dim3(256), pl.lds_bwd, (hipStream_t)stream, main_lo, g,
                       ws + (size_t)bands * E, gjoint, gpl, gscale, gmain_lo);
    MSPL_CHECK_LAUNCH("nid_heads_bwd");
    return MSPL_OK;
}
