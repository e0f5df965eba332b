// The parts every loss / meter kernel is built from (ce_head.hip, uw_loss_heads.hip, ce_meters.hip, eval.hip, miou_areas_kernel in
// labels.hip, wce_fwd_kernel in losses.hip): the MIOU area rule, the workgroup reduction of the cross-entropy sums, the band / patch
// code of the kernels that evaluate a low-resolution head at label resolution, and the host's patch sizing.  A new loss kernel
// starts from these; a rule that changes changes here (and in ce_head_kernel, which keeps its row tally and reduction written out:
// the comment there says why).
#pragma once
#include <algorithm>

#include "common.hpp"

namespace mspl {

// ---------------------------------------------------------------------------------------------------------------- MIOU areas
// MIOU.get_iou in the reference's uint8 arithmetic (utilities/metrics/segmentation_miou.py:28-41):
//   p = uint8(prediction) + 1,  g = uint8(target) + 1      (255 wraps to 0 = ignored)
//   p = g ? p : 0;  inter = (p == g) ? p : 0;  three K-bin histograms over the values 1..K (torch.histc(min=1, max=K)),
// kept per workgroup as 3 K LDS counters [inter | pred | mask] (K <= 64) and flushed with one 64-bit atomic per non-empty bin.
constexpr int MIOU_MAX_BINS = 64;

struct MiouCodes { unsigned p8, g8; };       // 0 counts nowhere

__device__ __forceinline__ unsigned miou_u8_plus1(unsigned v) { return (v + 1u) & 255u; }
// (L: int64_t, or the int a kernel narrowed its label to -- widening that one back costs uw_loss_heads_kernel<8,false,true> registers)
template <typename L>
__device__ __forceinline__ unsigned miou_label_code(L label) { return miou_u8_plus1((unsigned)(label & 255)); }
// pred: the first-maximum class (or a uint8 label); g8: the label's code
__device__ __forceinline__ MiouCodes miou_codes8(unsigned pred, unsigned g8) { return MiouCodes{g8 ? miou_u8_plus1(pred) : 0u, g8}; }
template <typename L>
__device__ __forceinline__ MiouCodes miou_codes(unsigned pred, L label) { return miou_codes8(pred, miou_label_code(label)); }

__device__ __forceinline__ void miou_clear(unsigned int* h, int K) {
    for (int i = threadIdx.x; i < 3 * K; i += 256) h[i] = 0;
}

// per-pixel form: up to three LDS atomics by the pixel's thread.  (The three tests stay written out: through a one-bin helper the
// compiler rewrites them as (v - 1) < K and eval_epilogue_kernel / miou_areas_kernel take two more registers.)
__device__ __forceinline__ void miou_count(unsigned int* h, int K, MiouCodes c) {
    const unsigned p8 = c.p8, g8 = c.g8;
    const unsigned in8 = (p8 == g8) ? p8 : 0u;
    if (in8 >= 1 && in8 <= (unsigned)K) atomicAdd(&h[in8 - 1], 1u);
    if (p8 >= 1 && p8 <= (unsigned)K) atomicAdd(&h[K + p8 - 1], 1u);
    if (g8 >= 1 && g8 <= (unsigned)K) atomicAdd(&h[2 * K + g8 - 1], 1u);
}

// per-row form: a lane packs the codes of its four pixels of a row, a byte each, ...
__device__ __forceinline__ void miou_pack(unsigned& pk_p, unsigned& pk_g, int j, MiouCodes c) {
    pk_p |= c.p8 << (8 * j);
    pk_g |= c.g8 << (8 * j);
}
// ... and the wave tallies them per bin: a compare, the population count of its lane mask on the scalar unit, one LDS add by lane 0
__device__ __forceinline__ void miou_tally_row(unsigned int* h, int K, unsigned pk_p, unsigned pk_g, int lane) {
    const unsigned eq = pk_p ^ pk_g;                        // a zero byte: p == g, the intersection carries p
    for (unsigned k = 1; k <= (unsigned)K; ++k) {
        unsigned ci = 0, cp = 0, cg = 0;                     // wave-uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool isp = ((pk_p >> (8 * j)) & 0xffu) == k, isg = ((pk_g >> (8 * j)) & 0xffu) == k;
            cp += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(isp));
            cg += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(isg));
            ci += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(isp && ((eq >> (8 * j)) & 0xffu) == 0u));
        }
        if (lane == 0) {
            if (ci) atomicAdd(&h[k - 1], ci);
            if (cp) atomicAdd(&h[K + k - 1], cp);
            if (cg) atomicAdd(&h[2 * K + k - 1], cg);
        }
    }
}

// (after a barrier that orders the workgroup's LDS adds)
__device__ __forceinline__ void miou_flush(const unsigned int* h, int K, unsigned long long* __restrict__ areas) {
    for (int i = threadIdx.x; i < 3 * K; i += 256)
        if (h[i]) atomicAdd(&areas[i], (unsigned long long)h[i]);
}

// ------------------------------------------------------------------------------------------------------------------- CE sums
// sums[0] += a, sums[1] += b over a workgroup of four waves: shuffle ladder, one LDS slot per wave, two atomics by thread 0 that
// pair the waves as (0 + 1) + (2 + 3).  Contains one workgroup barrier (miou_flush may follow it directly).
template <typename T>
__device__ __forceinline__ void ce_sums_reduce(T a, T b, T* __restrict__ sums) {
    __shared__ T red[2][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&sums[0], (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
        atomicAdd(&sums[1], (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    }
}

// ----------------------------------------------------------------------------------------------------------------- head band
// A workgroup owns a band of TH rows x TW columns of the label map and stages, per head, the patch that band interpolates from.
struct BandTile { int img, y0, x0, rows, cols; };

__device__ __forceinline__ BandTile band_tile(unsigned tile, int tiles_x, int tiles_y, int TH, int TW, int H, int W) {
    unsigned b = tile;
    const int txi = b % tiles_x;  b /= tiles_x;
    const int tyi = b % tiles_y;
    const int img = b / tiles_y;
    const int y0 = tyi * TH, x0 = txi * TW;
    return BandTile{img, y0, x0, min(TH, H - y0), min(TW, W - x0)};
}

// the patch: first source row / column of the band's first pixel .. second source of its last, at most MR x MC (the host sized MR,
// MC from the same rule: bilinear_span)
struct BandPatch { int y0, x0, nr, nc; };

__device__ __forceinline__ BandPatch band_patch(float sh, float sw, int Hs, int Ws, const BandTile& t, int MR, int MC) {
    int y0, y1, x0, x1, t0, t1;  float f0, f1;
    bilinear_src(sh, t.y0, Hs, y0, t1, f0, f1);              bilinear_src(sh, t.y0 + t.rows - 1, Hs, t0, y1, f0, f1);
    bilinear_src(sw, t.x0, Ws, x0, t1, f0, f1);              bilinear_src(sw, t.x0 + t.cols - 1, Ws, t0, x1, f0, f1);
    return BandPatch{y0, x0, min(y1 - y0 + 1, MR), min(x1 - x0 + 1, MC)};
}

// stage a (N, C, Hs, Ws) head's patch as [C][MR][MC] (msz = MR * MC): a wave per (channel, row), lanes over the columns
__device__ __forceinline__ void band_stage(float* dst, const float* __restrict__ head, int img, int C, int Hs, int Ws,
                                           const BandPatch& p, int MC, int msz, int wave, int lane) {
    for (int cr = wave; cr < C * p.nr; cr += 4) {
        const int c = cr / p.nr, r = cr - c * p.nr;
        const float* src = head + (((size_t)img * C + c) * Hs + p.y0 + r) * (size_t)Ws + p.x0;
        for (int x = lane; x < p.nc; x += 64) dst[c * msz + r * MC + x] = src[x];
    }
}

// ---------------------------------------------------------------------------------------------------------------------- host
// Most source positions any run of `tile` consecutive outputs starting at a multiple of `tile` touches (bilinear, align_corners);
// with align4 the first position is rounded down to a multiple of 4 and the count up to a multiple of 4 (16-byte staging chunks).
static inline int bilinear_span(int in_size, int out_size, int tile, bool align4 = false) {
    const float sc = bilinear_scale(in_size, out_size);
    int most = 1;
    for (int o0 = 0; o0 < out_size; o0 += tile) {
        int a0, a1, b0, b1;
        bilinear_src_host(sc, o0, in_size, a0, a1);
        bilinear_src_host(sc, std::min(o0 + tile, out_size) - 1, in_size, b0, b1);
        if (align4) a0 &= ~3;
        int cnt = b1 - a0 + 1;
        if (align4) cnt = (cnt + 3) & ~3;
        most = std::max(most, cnt);
    }
    return most;
}

// Band height: 8 rows (two per wave) when that still gives ~3 workgroups per CU, else 4; halved while the patches outgrow the
// budget.  lds_bytes(th) sizes the patches for a height (and may record them: its last call is for the height returned).
template <class F>
static inline int band_height(int N, int H, int tiles_x, size_t budget, F&& lds_bytes) {
    int th = ((int64_t)N * ceil_div(H, 8) * tiles_x >= 768) ? 8 : 4;
    while (lds_bytes(th) > budget && th > 1) th >>= 1;
    return th;
}

}  // namespace mspl
