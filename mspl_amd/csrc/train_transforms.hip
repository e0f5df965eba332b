// Train-time loader transforms on the device (include/mspl_hip.h "train-time loader transforms").
//   transforms/segmentation/data_transforms.py:67-91    RandomScale: Image.ANTIALIAS (LANCZOS) rgb, NEAREST label, BILINEAR depth
//   transforms/segmentation/data_transforms.py:94-136   RandomCrop: Pad(fill 0 | ignore_idx) + crop
//   transforms/segmentation/data_transforms.py:191-212  Resize: BILINEAR rgb / depth, NEAREST label
//   transforms/segmentation/data_transforms.py:15-66    RandomFlip, Tensorize / Normalize
// The reference runs these with Pillow on the host, one image at a time (greenhouse.py:211-219, camvid.py:95-104,
// cityscapes.py:109-117, greenhouse.py:118-125).  Here the random draws stay on the host and a batch of one source size is
// transformed by at most three launches:
//   scale (rgb), scale (depth): Pillow's two resampling passes FUSED per output tile -- the horizontal pass for the source rows
//       the tile's output rows need goes to LDS (uint8-rounded, as Pillow stores it), the vertical pass reads LDS.  A row's
//       horizontal result depends on that row alone, so the halo rows recomputed by neighbouring tiles are the same bytes.
//       Writes the scaled uint8 image to the caller's workspace; images whose size does not change are skipped (read in place).
//   output: Resize (the same fused tile, BILINEAR) or pad + crop, mirror, /255, normalise for rgb and depth, and the label as ONE
//       gather through the composed NEAREST index tables -- one launch for all three outputs.
// The inputs are STORES of M frames read by slot (mspl_train_transform_store_fwd; a contiguous batch is the store of N slots read in
// order), the label maps have their own size (Hl, Wl), and a 256-byte table may remap the source label values inside the gather.
// Every size, slot and table entry is clamped where it is used: a bad record gives wrong pixels, never an access outside the buffers.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace mspl {

namespace {

constexpr int TT_PRECISION_BITS = 32 - 8 - 2;
constexpr int TT_W = 64;           // output columns per tile: one wave per tile row, stores coalesced along W
constexpr int TT_H = 32;           // output rows per tile
constexpr int TT_THREADS = 256;
constexpr int TT_MAX_ROWS = 256;   // LDS rows of horizontal results: 64 KiB at 4 bytes per (row, column)

__device__ __forceinline__ int tt_clip8(int v) {
    v >>= TT_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// clip8 of each channel's accumulator, packed (channel c in byte c).  The empty asm keeps hipcc from fusing the shift + clamp + pack
// of two channels into v_ashr_pk_u8_i32: that instruction writes only the low half of its destination, and the packed value then
// carried the register's old upper half into channel 2 (+1 on a few pixels per image, seen on gfx950 against Pillow).
template <int C>
__device__ __forceinline__ uint32_t pack_clip8(const int (&acc)[C]) {
    uint32_t px = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int v = tt_clip8(acc[c]);
        asm volatile("" : "+v"(v));
        px |= (uint32_t)v << (8 * c);
    }
    return px;
}

// Packed pixel: channel c in byte c.
template <int C>
__device__ __forceinline__ uint32_t load_px(const uint8_t* p) {
    if (C == 1) return p[0];
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// One output tile (TT_H x TT_W at oy0, ox0) of Pillow's resample of img (Hin x Win x C uint8) to Hout x Wout.  xt / yt: device
// tables (layout in mspl_hip.h) or NULL to skip that pass (Resample.c ImagingResampleInner: need_horizontal / need_vertical).
// emit(yo, xo, packed) receives every output pixel of the tile that lies inside Hout x Wout.
template <int C, typename Emit>
__device__ __forceinline__ void resample_tile(const uint8_t* __restrict__ img, int Hin, int Win, int Hout, int Wout,
                                              const int32_t* __restrict__ xt, const int32_t* __restrict__ yt, int oy0, int ox0,
                                              int rows_cap, uint32_t* __restrict__ hbuf, Emit emit) {
    const int tid = threadIdx.x;
    const int oyl = min(oy0 + TT_H, Hout) - 1;
    const int ys = yt ? yt[0] : 0;
    int ry0 = oy0, nrows = oyl - oy0 + 1;
    if (yt) {
        const int32_t* f = yt + 1 + (size_t)oy0 * ys;
        const int32_t* l = yt + 1 + (size_t)oyl * ys;
        ry0 = clampi(f[0], 0, Hin - 1);
        nrows = clampi(l[0] + l[1] - ry0, 1, rows_cap);
    }
    nrows = min(min(nrows, rows_cap), Hin - ry0);
    const int xs = xt ? xt[0] : 0;
    // horizontal pass (or a plain copy of the rows when the width does not change) into LDS
    for (int i = tid; i < nrows * TT_W; i += TT_THREADS) {
        const int r = i / TT_W, xl = i - r * TT_W;
        const int xo = ox0 + xl;
        if (xo >= Wout) continue;
        const uint8_t* row = img + (size_t)(ry0 + r) * Win * C;
        uint32_t px;
        if (xt) {
            const int32_t* t = xt + 1 + (size_t)xo * xs;
            const int x0 = clampi(t[0], 0, Win - 1);
            const int cnt = clampi(t[1], 0, min(xs - 2, Win - x0));
            int acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 1 << (TT_PRECISION_BITS - 1);
            const uint8_t* s = row + (size_t)x0 * C;
            for (int j = 0; j < cnt; ++j) {
                const int kv = t[2 + j];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += (int)s[j * C + c] * kv;
            }
            px = pack_clip8<C>(acc);
        } else {
            px = load_px<C>(row + (size_t)min(xo, Win - 1) * C);
        }
        hbuf[r * TT_W + xl] = px;
    }
    __syncthreads();
    // vertical pass from LDS (or the LDS rows as they are when the height does not change)
    for (int i = tid; i < TT_H * TT_W; i += TT_THREADS) {
        const int yl = i / TT_W, xl = i - yl * TT_W;
        const int yo = oy0 + yl, xo = ox0 + xl;
        if (yo >= Hout || xo >= Wout) continue;
        uint32_t px;
        if (yt) {
            const int32_t* t = yt + 1 + (size_t)yo * ys;
            const int r0 = clampi(t[0] - ry0, 0, nrows - 1);
            const int cnt = clampi(t[1], 0, min(ys - 2, nrows - r0));
            int acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 1 << (TT_PRECISION_BITS - 1);
            for (int j = 0; j < cnt; ++j) {
                const int kv = t[2 + j];
                const uint32_t h = hbuf[(r0 + j) * TT_W + xl];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += (int)((h >> (8 * c)) & 255u) * kv;
            }
            px = pack_clip8<C>(acc);
        } else {
            px = hbuf[min(yl, nrows - 1) * TT_W + xl];
        }
        emit(yo, xo, px);
    }
}

__device__ __forceinline__ bool rec_scaled(const mspl_train_rec_t& r, int Hs, int Ws) { return r.sh != Hs || r.sw != Ws; }

// Image n of the batch is slot slots[n] of the store (n itself without a slot list), clamped into the store.
__device__ __forceinline__ size_t slot_of(const int32_t* __restrict__ slots, int n, int M) {
    return (size_t)clampi(slots ? slots[n] : n, 0, M - 1);
}

struct ScaleArgs {
    const uint8_t* src;            // store (M,Hs,Ws,C)
    const int32_t* slots;          // N slot numbers or null
    int M;
    const mspl_train_rec_t* recs;
    uint8_t* ws;                   // (N, max_sh * max_sw * C)
    int Hs, Ws, max_sh, max_sw, rows_cap, depth;
};

// RandomScale for rgb (LANCZOS, C = 3) or depth (BILINEAR, C = 1): one workgroup per (output tile, image).
template <int C>
__global__ __launch_bounds__(TT_THREADS) void train_scale_kernel(ScaleArgs a) {
    extern __shared__ uint32_t hbuf[];
    const int n = blockIdx.z;
    const mspl_train_rec_t& r = a.recs[n];
    const int sh = clampi(r.sh, 1, a.max_sh), sw = clampi(r.sw, 1, a.max_sw);
    const int oy0 = blockIdx.y * TT_H, ox0 = blockIdx.x * TT_W;
    if (!rec_scaled(r, a.Hs, a.Ws) || oy0 >= sh || ox0 >= sw) return;        // whole workgroup: before any barrier
    const int32_t* xt = sw != a.Ws ? (a.depth ? r.dscale_x : r.scale_x) : nullptr;
    const int32_t* yt = sh != a.Hs ? (a.depth ? r.dscale_y : r.scale_y) : nullptr;
    const uint8_t* img = a.src + slot_of(a.slots, n, a.M) * a.Hs * a.Ws * C;
    uint8_t* dst = a.ws + (size_t)n * a.max_sh * a.max_sw * C;
    resample_tile<C>(img, a.Hs, a.Ws, sh, sw, xt, yt, oy0, ox0, a.rows_cap, hbuf, [&](int yo, int xo, uint32_t px) {
        uint8_t* d = dst + ((size_t)yo * sw + xo) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = (uint8_t)(px >> (8 * c));
    });
}

struct OutArgs {
    const uint8_t* rgb;            // store (M,Hs,Ws,3)
    const uint8_t* label;          // store (M,Hl,Wl) or null
    const uint8_t* depth;          // store (M,Hs,Ws) or null
    const int32_t* slots;          // N slot numbers or null
    const uint8_t* lut;            // 256 bytes: remap of the source label values, or null
    const mspl_train_rec_t* recs;
    const uint8_t* ws_rgb;         // scaled rgb, (N, max_sh * max_sw * 3)
    const uint8_t* ws_depth;       // scaled depth, (N, max_sh * max_sw)
    const float* mean;
    const float* stdv;
    float* out_rgb;                // (N,3,H,W)
    int64_t* out_label;            // (N,H,W)
    float* out_depth;              // (N,1,H,W)
    int M, Hs, Ws, Hl, Wl, H, W, max_sh, max_sw, crop, scale_stage, ignore_idx, rows_cap;
};

// Pad + crop: output (yo, xo) is pixel (yo + dy, xo + dx) of the sh x sw image, 0 (the Pad fill) outside it.
template <int C, typename Emit>
__device__ __forceinline__ void crop_pixels(const uint8_t* __restrict__ img, int sh, int sw, int H, int W, int dy, int dx, int oy0,
                                            int ox0, Emit emit) {
    for (int i = threadIdx.x; i < TT_H * TT_W; i += TT_THREADS) {
        const int yl = i / TT_W, xl = i - yl * TT_W;
        const int yo = oy0 + yl, xo = ox0 + xl;
        if (yo >= H || xo >= W) continue;
        const int yy = yo + dy, xx = xo + dx;
        const uint32_t px = (yy >= 0 && yy < sh && xx >= 0 && xx < sw) ? load_px<C>(img + ((size_t)yy * sw + xx) * C) : 0u;
        emit(yo, xo, px);
    }
}

__global__ __launch_bounds__(TT_THREADS) void train_output_kernel(OutArgs a) {
    extern __shared__ uint32_t hbuf[];
    const int n = blockIdx.z;
    const mspl_train_rec_t& r = a.recs[n];
    const int sh = clampi(r.sh, 1, a.max_sh), sw = clampi(r.sw, 1, a.max_sw);
    const bool scaled = rec_scaled(r, a.Hs, a.Ws);
    const int oy0 = blockIdx.y * TT_H, ox0 = blockIdx.x * TT_W;
    const int H = a.H, W = a.W;
    const bool flip = r.flip != 0;
    // crop: output (yo, xo) is pixel (yo + crop_i - pad_h, xo + crop_j - pad_w) of the scaled image
    const int dy = a.crop ? clampi(r.crop_i, 0, 2 * max(r.pad_h, 0) + sh - H) - max(r.pad_h, 0) : 0;
    const int dx = a.crop ? clampi(r.crop_j, 0, 2 * max(r.pad_w, 0) + sw - W) - max(r.pad_w, 0) : 0;
    const int32_t* xt = (!a.crop && sw != W) ? r.out_x : nullptr;
    const int32_t* yt = (!a.crop && sh != H) ? r.out_y : nullptr;
    const size_t plane = (size_t)H * W;
    const size_t slot = slot_of(a.slots, n, a.M);

    {   // rgb
        const uint8_t* img = scaled ? a.ws_rgb + (size_t)n * a.max_sh * a.max_sw * 3 : a.rgb + slot * a.Hs * a.Ws * 3;
        float* o = a.out_rgb + (size_t)n * 3 * plane;
        float m[3] = {0.f, 0.f, 0.f}, s[3] = {1.f, 1.f, 1.f};
        const bool norm = a.mean != nullptr;
        if (norm) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { m[c] = a.mean[c]; s[c] = a.stdv[c]; }
        }
        auto emit = [&](int yo, int xo, uint32_t px) {
            const int xd = flip ? W - 1 - xo : xo;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = (float)((px >> (8 * c)) & 255u) / 255.0f;       // to_tensor: true division, as ATen's div(255)
                if (norm) v = (v - m[c]) / s[c];                          // normalize: sub_ then div_
                o[c * plane + (size_t)yo * W + xd] = v;
            }
        };
        if (a.crop) crop_pixels<3>(img, sh, sw, H, W, dy, dx, oy0, ox0, emit);
        else resample_tile<3>(img, sh, sw, H, W, xt, yt, oy0, ox0, a.rows_cap, hbuf, emit);
    }
    if (a.out_depth) {
        __syncthreads();                                                  // hbuf is reused
        const uint8_t* img = scaled ? a.ws_depth + (size_t)n * a.max_sh * a.max_sw : a.depth + slot * a.Hs * a.Ws;
        float* o = a.out_depth + (size_t)n * plane;
        auto emit = [&](int yo, int xo, uint32_t px) {
            const int xd = flip ? W - 1 - xo : xo;
            o[(size_t)yo * W + xd] = (float)(px & 255u) / 255.0f;
        };
        if (a.crop) crop_pixels<1>(img, sh, sw, H, W, dy, dx, oy0, ox0, emit);
        else resample_tile<1>(img, sh, sw, H, W, xt, yt, oy0, ox0, a.rows_cap, hbuf, emit);
    }
    if (a.out_label) {   // NEAREST (scale) then NEAREST (Resize) or pad + crop, composed into one gather from the source map
        // The map has its own size (Hl, Wl).  RandomScale resizes it from that size to the frame's scaled size (lsh, lsw) = (sh, sw);
        // without that stage it reaches Resize as it is: (lsh, lsw) = (Hl, Wl).
        const int lsh = a.scale_stage ? sh : a.Hl, lsw = a.scale_stage ? sw : a.Wl;
        const uint8_t* lab = a.label + slot * a.Hl * a.Wl;
        int64_t* o = a.out_label + (size_t)n * plane;
        const int32_t* nx = lsw != a.Wl ? r.near_x : nullptr;
        const int32_t* ny = lsh != a.Hl ? r.near_y : nullptr;
        const int32_t* nox = (!a.crop && lsw != W) ? r.near_out_x : nullptr;
        const int32_t* noy = (!a.crop && lsh != H) ? r.near_out_y : nullptr;
        for (int i = threadIdx.x; i < TT_H * TT_W; i += TT_THREADS) {
            const int yl = i / TT_W, xl = i - yl * TT_W;
            const int yo = oy0 + yl, xo = ox0 + xl;
            if (yo >= H || xo >= W) continue;
            int yy, xx;                                                   // pixel of the scaled map
            if (a.crop) {
                yy = yo + dy;
                xx = xo + dx;
            } else {
                yy = noy ? noy[yo] : yo;
                xx = nox ? nox[xo] : xo;
            }
            int64_t v = a.ignore_idx;
            if (yy >= 0 && yy < lsh && xx >= 0 && xx < lsw) {
                const int ry = clampi(ny ? ny[yy] : yy, 0, a.Hl - 1);
                const int rx = clampi(nx ? nx[xx] : xx, 0, a.Wl - 1);
                const uint8_t sv = lab[(size_t)ry * a.Wl + rx];
                v = a.lut ? a.lut[sv] : sv;                               // the pad fill above does not pass through the remap
            }
            o[(size_t)yo * W + (flip ? W - 1 - xo : xo)] = v;
        }
    }
}

// Rows of horizontal results a tile's vertical pass can span: (TT_H - 1) * scale + 2 * support, +2 for the roundings of
// Resample.c's (int)(center -+ support + 0.5) bounds.
int tile_rows(int in, int out, double support) {
    if (in == out) return TT_H;
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil((TT_H - 1) * scale + 2.0 * support * fs) + 2;
}

}  // namespace

}  // namespace mspl

using namespace mspl;

extern "C" int64_t mspl_train_transform_workspace_bytes(int32_t N, int32_t max_sh, int32_t max_sw, int32_t with_depth) {
    if (N <= 0 || max_sh <= 0 || max_sw <= 0) return MSPL_ERR_BAD_SHAPE;
    return (int64_t)N * max_sh * max_sw * (with_depth ? 4 : 3);
}

extern "C" int mspl_train_transform_store_fwd(const uint8_t* rgb, const uint8_t* label, const uint8_t* depth, int32_t M, int32_t N,
                                              int32_t Hs, int32_t Ws, int32_t Hl, int32_t Wl, int32_t H, int32_t W, int32_t crop,
                                              int32_t scale_stage, int32_t ignore_idx, const mspl_train_rec_t* recs_host,
                                              const mspl_train_rec_t* recs_dev, const int32_t* slots_host, const int32_t* slots_dev,
                                              const uint8_t* label_lut, const float* mean, const float* stdv, uint8_t* ws,
                                              int32_t max_sh, int32_t max_sw, float* out_rgb, int64_t* out_label, float* out_depth,
                                              void* stream) {
    MSPL_REQUIRE(rgb && recs_host && recs_dev && out_rgb, MSPL_ERR_NULL_POINTER, "train_transform: null pointer");
    MSPL_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && max_sh > 0 && max_sw > 0, MSPL_ERR_BAD_SHAPE,
                 "train_transform: bad shape N=%d %dx%d -> %dx%d (scaled at most %dx%d)", N, Hs, Ws, H, W, max_sh, max_sw);
    MSPL_REQUIRE(N <= 65535 && (int64_t)max_sh * max_sw * 4 <= 0x7fffffff && (int64_t)Hs * Ws * 3 <= 0x7fffffff &&
                     (int64_t)H * W * 3 <= 0x7fffffff, MSPL_ERR_BAD_SHAPE, "train_transform: sizes too large");
    MSPL_REQUIRE((label == nullptr) == (out_label == nullptr) && (depth == nullptr) == (out_depth == nullptr), MSPL_ERR_NULL_POINTER,
                 "train_transform: label / depth and their outputs go together");
    MSPL_REQUIRE((mean == nullptr) == (stdv == nullptr), MSPL_ERR_NULL_POINTER, "train_transform: mean and std go together");
    MSPL_REQUIRE(ignore_idx >= -0x7fffffff, MSPL_ERR_BAD_SHAPE, "train_transform: ignore_idx");
    MSPL_REQUIRE(M > 0 && (slots_host == nullptr) == (slots_dev == nullptr), MSPL_ERR_BAD_SHAPE,
                 "train_transform: a store of %d slots, or one slot list without its copy", M);
    MSPL_REQUIRE(slots_host || N <= M, MSPL_ERR_BAD_SHAPE, "train_transform: %d images from a store of %d slots", N, M);
    for (int n = 0; slots_host && n < N; ++n)
        MSPL_REQUIRE(slots_host[n] >= 0 && slots_host[n] < M, MSPL_ERR_BAD_SHAPE, "train_transform: image %d reads slot %d of a store of %d",
                     n, slots_host[n], M);
    if (label) {
        MSPL_REQUIRE(Hl > 0 && Wl > 0 && (int64_t)Hl * Wl <= 0x7fffffff, MSPL_ERR_BAD_SHAPE, "train_transform: label maps of %dx%d", Hl, Wl);
        MSPL_REQUIRE(scale_stage || !crop || (Hl == Hs && Wl == Ws), MSPL_ERR_UNSUPPORTED,
                     "train_transform: RandomCrop without RandomScale of %dx%d label maps on %dx%d frames (the reference crops them "
                     "misaligned)", Hl, Wl, Hs, Ws);
    }
    int scale_rows = 1, dscale_rows = 1, out_rows = 1, sh_max = 0, sw_max = 0;
    bool any_scaled = false;
    for (int n = 0; n < N; ++n) {
        const mspl_train_rec_t& r = recs_host[n];
        MSPL_REQUIRE(r.sh > 0 && r.sw > 0 && r.sh <= max_sh && r.sw <= max_sw, MSPL_ERR_BAD_SHAPE,
                     "train_transform: image %d scaled to %dx%d, outside 1..%dx%d", n, r.sh, r.sw, max_sh, max_sw);
        MSPL_REQUIRE(r.flip == 0 || r.flip == 1, MSPL_ERR_BAD_SHAPE, "train_transform: image %d flip %d", n, r.flip);
        const bool sx = r.sw != Ws, sy = r.sh != Hs;
        MSPL_REQUIRE(scale_stage || !(sx || sy), MSPL_ERR_BAD_SHAPE, "train_transform: image %d scaled to %dx%d without a RandomScale stage",
                     n, r.sh, r.sw);
        MSPL_REQUIRE((!sx || r.scale_x) && (!sy || r.scale_y), MSPL_ERR_NULL_POINTER, "train_transform: image %d scale tables", n);
        MSPL_REQUIRE(!depth || ((!sx || r.dscale_x) && (!sy || r.dscale_y)), MSPL_ERR_NULL_POINTER,
                     "train_transform: image %d depth scale tables", n);
        // the label map goes from its own size to (lsh, lsw): the frame's scaled size, or its own size without a RandomScale stage
        const int lsh = scale_stage ? r.sh : Hl, lsw = scale_stage ? r.sw : Wl;
        MSPL_REQUIRE(!label || ((lsw == Wl || r.near_x) && (lsh == Hl || r.near_y)), MSPL_ERR_NULL_POINTER,
                     "train_transform: image %d label scale tables", n);
        if (crop) {
            MSPL_REQUIRE(r.pad_h >= 0 && r.pad_w >= 0 && r.sh + 2 * r.pad_h >= H && r.sw + 2 * r.pad_w >= W, MSPL_ERR_BAD_SHAPE,
                         "train_transform: image %d padded to %dx%d, smaller than the crop %dx%d", n, r.sh + 2 * r.pad_h,
                         r.sw + 2 * r.pad_w, H, W);
            MSPL_REQUIRE(r.crop_i >= 0 && r.crop_j >= 0 && r.crop_i <= r.sh + 2 * r.pad_h - H && r.crop_j <= r.sw + 2 * r.pad_w - W,
                         MSPL_ERR_BAD_SHAPE, "train_transform: image %d crop origin (%d, %d) outside the padded image", n, r.crop_i,
                         r.crop_j);
        } else {
            MSPL_REQUIRE((r.sw == W || r.out_x) && (r.sh == H || r.out_y), MSPL_ERR_NULL_POINTER,
                         "train_transform: image %d Resize tables", n);
            MSPL_REQUIRE(!label || ((lsw == W || r.near_out_x) && (lsh == H || r.near_out_y)), MSPL_ERR_NULL_POINTER,
                         "train_transform: image %d label Resize tables", n);
            out_rows = std::max(out_rows, tile_rows(r.sh, H, 1.0));
        }
        if (sx || sy) {
            any_scaled = true;
            sh_max = std::max(sh_max, (int)r.sh);
            sw_max = std::max(sw_max, (int)r.sw);
            scale_rows = std::max(scale_rows, tile_rows(Hs, r.sh, 3.0));
            dscale_rows = std::max(dscale_rows, tile_rows(Hs, r.sh, 1.0));
        }
    }
    MSPL_REQUIRE(!any_scaled || ws, MSPL_ERR_NULL_POINTER, "train_transform: a scaled image needs the workspace");
    MSPL_REQUIRE(scale_rows <= TT_MAX_ROWS && out_rows <= TT_MAX_ROWS, MSPL_ERR_UNSUPPORTED,
                 "train_transform: a tile spans %d source rows (at most %d): scale factor too small", std::max(scale_rows, out_rows),
                 TT_MAX_ROWS);
    hipStream_t s = (hipStream_t)stream;
    if (any_scaled) {
        ScaleArgs sa{rgb, slots_dev, M, recs_dev, ws, Hs, Ws, max_sh, max_sw, scale_rows, 0};
        dim3 grid((unsigned)ceil_div(sw_max, TT_W), (unsigned)ceil_div(sh_max, TT_H), (unsigned)N);
        hipLaunchKernelGGL(train_scale_kernel<3>, grid, dim3(TT_THREADS), (size_t)scale_rows * TT_W * 4, s, sa);
        MSPL_CHECK_LAUNCH("train_transform(scale rgb)");
        if (depth) {
            ScaleArgs da{depth, slots_dev, M, recs_dev, ws + (size_t)N * max_sh * max_sw * 3, Hs, Ws, max_sh, max_sw, dscale_rows, 1};
            hipLaunchKernelGGL(train_scale_kernel<1>, grid, dim3(TT_THREADS), (size_t)dscale_rows * TT_W * 4, s, da);
            MSPL_CHECK_LAUNCH("train_transform(scale depth)");
        }
    }
    OutArgs oa{rgb, label, depth, slots_dev, label ? label_lut : nullptr, recs_dev, ws, ws ? ws + (size_t)N * max_sh * max_sw * 3 : nullptr,
               mean, stdv, out_rgb, out_label, out_depth, M, Hs, Ws, label ? Hl : Hs, label ? Wl : Ws, H, W, max_sh, max_sw,
               crop ? 1 : 0, scale_stage ? 1 : 0, ignore_idx, out_rows};
    dim3 grid((unsigned)ceil_div(W, TT_W), (unsigned)ceil_div(H, TT_H), (unsigned)N);
    hipLaunchKernelGGL(train_output_kernel, grid, dim3(TT_THREADS), crop ? 0 : (size_t)out_rows * TT_W * 4, s, oa);
    MSPL_CHECK_LAUNCH("train_transform(output)");
    return MSPL_OK;
}

// A contiguous batch is a store of N slots read in order, its label maps at the frame's size; the records alone say what is scaled.
extern "C" int mspl_train_transform_fwd(const uint8_t* rgb, const uint8_t* label, const uint8_t* depth, int32_t N, int32_t Hs,
                                        int32_t Ws, int32_t H, int32_t W, int32_t crop, int32_t ignore_idx,
                                        const mspl_train_rec_t* recs_host, const mspl_train_rec_t* recs_dev, const float* mean,
                                        const float* stdv, uint8_t* ws, int32_t max_sh, int32_t max_sw, float* out_rgb,
                                        int64_t* out_label, float* out_depth, void* stream) {
    return mspl_train_transform_store_fwd(rgb, label, depth, N, N, Hs, Ws, Hs, Ws, H, W, crop, 1, ignore_idx, recs_host, recs_dev, nullptr,
                                          nullptr, nullptr, mean, stdv, ws, max_sh, max_sw, out_rgb, out_label, out_depth, stream);
}
