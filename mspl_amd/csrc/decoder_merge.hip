// Head of a decoder stage in ONE launch (inference): the skip connection's grouped 3x3 + BN + PReLU + gate
// (EfficientPWConv.forward, nn_layers/efficient_pt.py:25-29), the x2 bilinear up-merge with the bottom-up tensor + BN + PReLU
// (model/segmentation/espdnet_ue.py:276-299) and the following pyramid block's projection_layer, 1x1 + BN + PReLU down to P
// planes (nn_layers/efficient_pyramid_pool.py:20,38):
//     proj[n,p,y,x] = prelu_p(bn_p(sum_c Wp[p,c] * m[n,c,y,x]))
//     m[n,c,y,x]    = prelu_br(bn_br(pw[n,c,y,x] + bilinear2x(bu)[n,c,y,x]))
//     pw[n,c,y,x]   = gate[n,c] * prelu_e(bn_e(grouped3x3(enc)[n,c,y,x]))
// Neither pw nor m is written: as three launches (conv3x3, bilinear with pre_add, conv1x1) each of them crossed memory twice only
// to cross a launch boundary.
//
// Mapping (register tile, no LDS traffic on the pixel path): a lane owns 2 rows x 2 adjacent columns of one image and carries the
// P x 2 x 2 projection accumulators; LPR = W / 2 lanes (at most 64, wider rows are cut into equal column blocks) cover a row pair
// and 64 / LPR row pairs of the SAME image share a wave, so every per-channel constant is wave-uniform: the three BN/PReLU triples
// and the gate travel in scalar registers, the 3x3 weights are LDS broadcasts (as scalar loads inside the channel loop they were a
// dependent round trip per channel: 128 -> 48 at 16 x 72x120 52.2 -> 49.5 us, 256 -> 64 at 36x60 33.5 -> 28.7).  The wave walks the groups outermost.  Per input channel it reads four
// rows (two output rows + one halo row either side) as 8-byte loads; halo columns come from the neighbouring lanes (DPP), and where
// the neighbour column belongs to another wave's column block the two edge lanes fetch it themselves.  Per `dec` channel it gathers
// the 3 x 3 low-resolution samples its four pixels blend.  The next input channel's rows are requested before the current ones are
// used, into the other of two named register buffers (nothing is copied at a loop's back edge); the low-resolution samples likewise
// where a group is one fetch, and at the group's start where it is eight.  All loads go through one buffer descriptor per tensor
// with loop-invariant lane offsets and the channel / plane offset as the scalar operand (no vector address arithmetic per load).
// The projection runs on the vector unit, the weight column Wp[0..P-1][c]
// broadcast from LDS (staged once per workgroup), channels ascending: the order of conv1x1_thin_kernel.
//
// Operation order per `dec` channel is that of the kernels this launch replaces (common.hpp epi_apply; bilinear_src; the 3x3 tap
// order of the kernel that serves the group shape in mspl_conv3x3_fwd), so m is bit-identical to the three-launch chain's.
#include "common.hpp"

namespace mspl {

struct DmGeom {
    int N, Cin, Cout, H, W, Hi, Wi;
    int LPR, SUB, ncb, rpw;      // lanes per row pair, row pairs per wave, column blocks per row, waves per (image, column block)
    unsigned total;              // waves
    float sh, sw;
};

struct DmParams {
    const float* enc;  const float* bu;  const float* w3;
    const float* e_scale;  const float* e_shift;  const float* e_alpha;  const float* gate;
    const float* b_scale;  const float* b_shift;  const float* b_alpha;
    const float* wp;  const float* p_scale;  const float* p_shift;  const float* p_alpha;
};

__device__ __forceinline__ float dm_from_left(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dm_from_right(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}

typedef unsigned dm_u32x2 __attribute__((ext_vector_type(2)));

constexpr int DM_PS = 16;        // LDS stride of one channel's projection weight column (floats)

// CG / COB: input / output channels per group.  KYOUT: the 3x3 sums run kernel row, input channel, kernel column (the order of
// gconv3x3_stream_kernel); otherwise input channel, kernel row, kernel column (conv3x3_kernel, dwconv3x3_stream_kernel).
// SPLIT: waves that share one pixel tile, each walking 1 / SPLIT of the groups; their partial projections are summed through LDS in
// wave order (small maps: one wave per tile leaves most SIMDs without a wave and the rest with nothing to hide a load behind).
// EDGE: rows are cut into column blocks (g.ncb > 1), so the halo column of a block's first / last lane is loaded, not shuffled.  A
// compile-time choice keeps every step of the walk below one straight-line block: with a branch around the edge loads the compiler
// copied the double buffers at the back edges again and needed 40 more registers.
template <int CG, int COB, int P, bool KYOUT, int SPLIT, bool EDGE>
__global__ __launch_bounds__(256) void decoder_merge_kernel(DmParams a, DmGeom g, float* __restrict__ out) {
    constexpr int CH = KYOUT ? CG : 1;          // input channels fetched (and prefetched) together
    constexpr int NCH = CG / CH;
    extern __shared__ __attribute__((aligned(16))) float wl[];      // [Cout][DM_PS]: Wp transposed, rows past P zero; SPLIT > 1: + partial sums
    for (int i = threadIdx.x; i < g.Cout * DM_PS; i += 256) {
        const int c = i / DM_PS, p = i - c * DM_PS;
        wl[i] = p < P ? a.wp[(size_t)p * g.Cout + c] : 0.f;
    }
    float* w3s = wl + g.Cout * DM_PS;                               // the 3x3 weights (read by uniform address: LDS broadcasts)
    for (int i = threadIdx.x; i < g.Cout * CG * 9; i += 256) w3s[i] = a.w3[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int ws = SPLIT == 1 ? 0 : (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // slice of the groups
    unsigned wid = SPLIT == 1 ? __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)) : blockIdx.x;
    if (wid >= g.total) return;                                     // wave-uniform (SPLIT > 1: workgroup-uniform)
    const int chunk = wid % g.rpw;  wid /= g.rpw;
    const int cb = wid % g.ncb;
    const int n = wid / g.ncb;                                      // uniform
    const int H = g.H, W = g.W, Hi = g.Hi, Wi = g.Wi;
    const int sub = lane / g.LPR, cl = lane - sub * g.LPR;
    const int rp_raw = chunk * g.SUB + sub;
    const int col_raw = (cb * g.LPR + cl) * 2;
    const bool live = sub < g.SUB && rp_raw < (H >> 1) && col_raw < W;
    const int y0 = min(rp_raw, (H >> 1) - 1) * 2;                   // dead lanes work on clamped, in-bounds coordinates
    const int col = min(col_raw, W - 2);
    const bool lok = cl > 0, rok = cl < g.LPR - 1 && col_raw + 2 < W;        // neighbour lane holds the neighbour column
    const bool ledge = EDGE && live && cl == 0 && col > 0;                    // neighbour column lies in another column block
    const bool redge = EDGE && live && cl == g.LPR - 1 && col + 2 < W;
    const bool top_in = y0 > 0, bot_in = y0 + 2 < H;
    // lane byte offsets into the wave's image, fixed for the whole walk; the channel / plane offset is wave-uniform and travels as
    // the scalar offset of every load (no per-load vector address arithmetic).  EDGE: every lane issues the edge load; a lane that
    // has no edge column asks for the wave's first row element again (in range, a line the row load already brings) and drops it.
    int roff[4], eoff[EDGE ? 4 : 1];
    const int ecol = ledge ? -1 : 2;                                // edge column relative to col
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        roff[r] = (min(max(y0 - 1 + r, 0), H - 1) * W + col) * 4;
        if (EDGE) eoff[r] = (ledge || redge) ? roff[r] + ecol * 4 : __builtin_amdgcn_readfirstlane(roff[r]);
    }

    // bilinear sources of the 2 x 2 pixels (align_corners=True).  The launcher has checked that the first source of an odd row /
    // column is one of the two sources of the even one before it (the second, except in the first pair where both start at 0), so
    // 3 rows x 3 columns of bu serve the four pixels.
    int xa[2], xb[2], ya[2], yb[2];
    float wx0[2], wx1[2], wy0[2], wy1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        bilinear_src(g.sw, col + j, Wi, xa[j], xb[j], wx0[j], wx1[j]);
        bilinear_src(g.sh, y0 + j, Hi, ya[j], yb[j], wy0[j], wy1[j]);
    }
    const bool xfirst = xa[1] == xa[0], yfirst = ya[1] == ya[0];    // the odd column / row starts at the even one's FIRST source
    int boff[9];
    {
        const int rr[3] = {ya[0] * Wi, yb[0] * Wi, yb[1] * Wi}, cc[3] = {xa[0], xb[0], xb[1]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) boff[r * 3 + c] = (rr[r] + cc[c]) * 4;
    }
    const int G = g.Cout / COB;
    const size_t hw = (size_t)H * W, hwi = (size_t)Hi * Wi;
    const int hwb = H * W * 4, hwib = Hi * Wi * 4;                  // bytes of a plane (the launcher bounds an image's bytes)
    // one descriptor per tensor, over this wave's image: every address below is clamped in range, the range check is a safety net
    const __amdgpu_buffer_rsrc_t ers =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.enc + (size_t)n * g.Cin * hw), 0, g.Cin * hwb, 0x00020000);
    const __amdgpu_buffer_rsrc_t brs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bu + (size_t)n * g.Cout * hwi), 0, g.Cout * hwib, 0x00020000);
    const float* gaten = a.gate + (size_t)n * g.Cout;

    struct RawC { float2 row[CH][4]; float edge[EDGE ? CH : 1][4]; };
    struct RawB { float s[COB][9]; };
    auto load_c = [&](int q, RawC& rc) {                            // q: chunk of CH input channels
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int so = (q * CH + i) * hwb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const dm_u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(ers, roff[r], so, 0);
                rc.row[i][r] = make_float2(__uint_as_float(t.x), __uint_as_float(t.y));
            }
            if constexpr (EDGE) {                                   // read under ledge / redge only
#pragma unroll
                for (int r = 0; r < 4; ++r) rc.edge[i][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ers, eoff[r], so, 0));
            }
        }
    };
    auto load_b = [&](int grp, RawB& rb) {
#pragma unroll
        for (int c = 0; c < COB; ++c) {
            const int so = (grp * COB + c) * hwib;
#pragma unroll
            for (int k = 0; k < 9; ++k) rb.s[c][k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brs, boff[k], so, 0));
        }
    };

    float pacc[P][2][2];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int t = 0; t < 2; ++t) pacc[p][t][0] = pacc[p][t][1] = 0.f;

    // the 3x3 taps of one chunk of CH input channels (chunk cc of its group) into acc
    auto conv_chunk = [&](const RawC& rc, const float* wg, int cc, float (&acc)[COB][2][2]) {
        // input row r of channel i feeds output row 0 through kernel row r and output row 1 through kernel row r - 1
        auto feed = [&](int i, int r) {
            float2 v = rc.row[i][r];
            float ev = EDGE ? rc.edge[i][r] : 0.f;
            const bool rin = r == 0 ? top_in : (r == 3 ? bot_in : true);
            if (!rin) { v.x = 0.f; v.y = 0.f; ev = 0.f; }
            float win[4];
            win[1] = v.x;  win[2] = v.y;
            const float fl = dm_from_left(v.y), fr = dm_from_right(v.x);
            win[0] = lok ? fl : (ledge ? ev : 0.f);
            win[3] = rok ? fr : (redge ? ev : 0.f);
            const int ci = cc * CH + i;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ky = r - t;
                if (ky < 0 || ky > 2) continue;
#pragma unroll
                for (int c = 0; c < COB; ++c) {
                    const float* wk = wg + (c * CG + ci) * 9 + ky * 3;
                    const float w0 = wk[0], w1 = wk[1], w2 = wk[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[c][t][j] = fmaf(w0, win[j], acc[c][t][j]);
                        acc[c][t][j] = fmaf(w1, win[j + 1], acc[c][t][j]);
                        acc[c][t][j] = fmaf(w2, win[j + 2], acc[c][t][j]);
                    }
                }
            }
        };
        if (KYOUT) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < CH; ++i) feed(i, r);
        } else {
#pragma unroll
            for (int i = 0; i < CH; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) feed(i, r);
        }
    };
    // both epilogues, the blend and the projection of one group's COB output channels
    auto finish = [&](int grp, const RawB& rb, const float (&acc)[COB][2][2]) {
#pragma unroll
        for (int c = 0; c < COB; ++c) {
            const int co = grp * COB + c;
            const float es = a.e_scale[co], eb = a.e_shift[co], ea = a.e_alpha[co], gt = gaten[co];
            const float bs = a.b_scale[co], bb = a.b_shift[co], ba = a.b_alpha[co];
            const float* s = rb.s[c];
            float h[3][2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                h[r][0] = wx0[0] * s[r * 3 + 0] + wx1[0] * s[r * 3 + 1];
                h[r][1] = wx0[1] * (xfirst ? s[r * 3 + 0] : s[r * 3 + 1]) + wx1[1] * s[r * 3 + 2];
            }
            const float hodd[2] = {yfirst ? h[0][0] : h[1][0], yfirst ? h[0][1] : h[1][1]};       // row ya[1], horizontally blended
            float m[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float pw = fmaf(acc[c][t][j], es, eb);
                    pw = pw > 0.0f ? pw : ea * pw;
                    pw *= gt;
                    float v = wy0[t] * (t == 0 ? h[0][j] : hodd[j]) + wy1[t] * h[t + 1][j];
                    v += pw;
                    v = fmaf(v, bs, bb);
                    m[t][j] = v > 0.0f ? v : ba * v;
                }
            const float* wc = wl + co * DM_PS;
#pragma unroll
            for (int p4 = 0; p4 < P; p4 += 4) {
                const float4 wv = *reinterpret_cast<const float4*>(wc + p4);
                const float ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                for (int pp = 0; pp < 4; ++pp) {
                    if (p4 + pp >= P) continue;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        pacc[p4 + pp][t][0] = fmaf(ww[pp], m[t][0], pacc[p4 + pp][t][0]);
                        pacc[p4 + pp][t][1] = fmaf(ww[pp], m[t][1], pacc[p4 + pp][t][1]);
                    }
                }
            }
        }
    };

    // Two named buffers for the fetched input rows: a step computes from one while the other loads and the next step swaps the
    // names, so nothing is copied at a back edge.  The prefetch past the last chunk / group is clamped to the last one (in bounds,
    // unused).
    const int g0 = ws * (G / SPLIT), g1 = g0 + G / SPLIT;           // G % SPLIT == 0 (launcher)
    const int Q = g.Cin / CH;
    static_assert(NCH == 1 || NCH % 2 == 0, "the channel loop runs in pairs of chunks");
    RawC c0, c1;
    load_c(g0 * NCH, c0);
    if constexpr (NCH == 1) {
        // one chunk per group: the group loop itself is the two-step body, the low-resolution samples are double-buffered with
        // the rows (a group is too short to hide their latency behind itself)
        auto group = [&](int grp, const RawC& ccur, RawC& cnxt, const RawB& bcur, RawB& bnxt) {
            load_b(min(grp + 1, G - 1), bnxt);
            load_c(min(grp + 1, Q - 1), cnxt);
            float acc[COB][2][2];
#pragma unroll
            for (int c = 0; c < COB; ++c)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[c][t][0] = acc[c][t][1] = 0.f;
            conv_chunk(ccur, w3s + grp * COB * CG * 9, 0, acc);
            finish(grp, bcur, acc);
        };
        RawB b0, b1;
        load_b(g0, b0);
#pragma unroll 1
        for (int grp = g0;;) {                                      // an odd trip count leaves after the first step (uniform)
            group(grp, c0, c1, b0, b1);
            if (++grp == g1) break;
            group(grp, c1, c0, b1, b0);
            if (++grp == g1) break;
        }
    } else {
        // NCH chunks per group, walked in pairs: c0 holds the group's first chunk on entry and the next group's on exit.  The
        // group's low-resolution samples are requested when the group starts and used after its 3x3 loop, which hides them: one
        // buffer, nothing to copy.
#pragma unroll 1
        for (int grp = g0; grp < g1; ++grp) {
            RawB b;
            load_b(grp, b);
            const float* wg = w3s + grp * COB * CG * 9;
            float acc[COB][2][2];
#pragma unroll
            for (int c = 0; c < COB; ++c)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[c][t][0] = acc[c][t][1] = 0.f;
#pragma unroll 1
            for (int cc = 0; cc < NCH; cc += 2) {                   // (unrolled 8 x 27 weights overflow the scalar registers)
                load_c(grp * NCH + cc + 1, c1);
                conv_chunk(c0, wg, cc, acc);
                load_c(min(grp * NCH + cc + 2, Q - 1), c0);
                conv_chunk(c1, wg, cc + 1, acc);
            }
            finish(grp, b, acc);
        }
    }
    if (SPLIT > 1) {                                                // partial sums of waves 1 .. SPLIT-1 -> LDS, added by wave 0 in wave order
        float* red = w3s + g.Cout * CG * 9;                         // [SPLIT - 1][P * 4][64]
        if (ws > 0) {
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int k = 0; k < 4; ++k) red[((ws - 1) * P * 4 + p * 4 + k) * 64 + lane] = pacc[p][k >> 1][k & 1];
        }
        __syncthreads();
        if (ws > 0) return;
#pragma unroll 1
        for (int w = 0; w < SPLIT - 1; ++w)
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int k = 0; k < 4; ++k) pacc[p][k >> 1][k & 1] += red[(w * P * 4 + p * 4 + k) * 64 + lane];
    }
    if (!live) return;
    float* on = out + (size_t)n * P * hw + (size_t)y0 * W + col;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const float ps = a.p_scale[p], pb = a.p_shift[p], pa = a.p_alpha[p];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v0 = fmaf(pacc[p][t][0], ps, pb), v1 = fmaf(pacc[p][t][1], ps, pb);
            v0 = v0 > 0.0f ? v0 : pa * v0;
            v1 = v1 > 0.0f ? v1 : pa * v1;
            store_out2(on + (size_t)p * hw + (size_t)t * W, make_float2(v0, v1));
        }
    }
}

// The kernel reads 3 x 3 samples of bu per 2 x 2 output pixels: the first bilinear source of every odd output row / column must be
// one of the two sources of the even one before it (true for the x2 align_corners=True map at every even size up to 4096; checked
// here with the device's own float expressions, so that a size where rounding breaks the rule falls back instead of reading the
// wrong sample).
static bool dm_sources_pair_up(float scale, int in_size, int out_size) {
    for (int d = 0; d + 1 < out_size; d += 2) {
        int idx[2];
        for (int j = 0; j < 2; ++j) {
            const float real = scale * (float)(d + j);
            int i = (int)floorf(real);
            if (i > in_size - 1) i = in_size - 1;
            idx[j] = i;
        }
        const int nxt0 = idx[0] + ((idx[0] < in_size - 1) ? 1 : 0);
        if (idx[1] != idx[0] && idx[1] != nxt0) return false;
    }
    return true;
}

template <int CG, int COB, bool KYOUT, int SPLIT, bool EDGE>
static int dm_launch_edge(const DmParams& a, const DmGeom& g, int P, float* out, hipStream_t s) {
    const dim3 grid(SPLIT == 1 ? (unsigned)ceil_div64((int64_t)g.total, 4) : g.total), blk(256);
    const size_t lds = ((size_t)g.Cout * (DM_PS + CG * 9) + (size_t)(SPLIT - 1) * P * 4 * 64) * sizeof(float);
    switch (P) {
        case 16: hipLaunchKernelGGL((decoder_merge_kernel<CG, COB, 16, KYOUT, SPLIT, EDGE>), grid, blk, lds, s, a, g, out); break;
        case 10: hipLaunchKernelGGL((decoder_merge_kernel<CG, COB, 10, KYOUT, SPLIT, EDGE>), grid, blk, lds, s, a, g, out); break;
        case 6: hipLaunchKernelGGL((decoder_merge_kernel<CG, COB, 6, KYOUT, SPLIT, EDGE>), grid, blk, lds, s, a, g, out); break;
        case 2: hipLaunchKernelGGL((decoder_merge_kernel<CG, COB, 2, KYOUT, SPLIT, EDGE>), grid, blk, lds, s, a, g, out); break;
        default: return 1;
    }
    return 0;
}

// rows wider than 128 columns are cut into column blocks (a geometry of the map alone): the form that loads the blocks' halo columns
template <int CG, int COB, bool KYOUT, int SPLIT>
static int dm_launch_split(const DmParams& a, const DmGeom& g, int P, float* out, hipStream_t s) {
    return g.ncb > 1 ? dm_launch_edge<CG, COB, KYOUT, SPLIT, true>(a, g, P, out, s) : dm_launch_edge<CG, COB, KYOUT, SPLIT, false>(a, g, P, out, s);
}

// Four waves per tile for the grouped shapes (8 -> 3, 4 -> 1: a wave's walk over all groups is long and their maps are small:
// measured at batch 16, one launch alone, 128 -> 48 at 72x120 97.7 us with one wave per tile against 49.5 us, 256 -> 64 at 36x60
// 119.5 against 28.7) and for depthwise maps of fewer than 64 tiles per image.  Depthwise otherwise: one wave per tile, and the
// projection sums the channels in ascending order like conv1x1_thin_kernel.  The choice must not look at N: an image's result may
// not depend on the batch it travels in (tests/test_gpu_fullsize.py: batch independence, lanes of grouped batches).
template <int CG, int COB, bool KYOUT>
static int dm_launch(const DmParams& a, const DmGeom& g, int P, float* out, hipStream_t s) {
    static const int split_below = MSPL_TUNE_INT("MSPL_DM_SPLIT_BELOW", 64);
    if ((CG > 1 || g.ncb * g.rpw < split_below) && (g.Cout / COB) % 4 == 0) return dm_launch_split<CG, COB, KYOUT, 4>(a, g, P, out, s);
    return dm_launch_split<CG, COB, KYOUT, 1>(a, g, P, out, s);
}

// 0 = launched, 1 = shape left to the three-launch chain, < 0 = error.
static int decoder_merge_try(const DmParams& a, int N, int Cin, int Cout, int P, int H, int W, float* out, hipStream_t s) {
    auto al16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    if ((H & 1) || (W & 1) || H < 2 || W < 2 || !(P == 2 || P == 6 || P == 10 || P == 16)) return 1;
    if (!al16(a.enc) || !al16(a.bu) || !al16(out) || !al16(a.w3)) return 1;
    if ((int64_t)N * Cin * H * W >= (1ll << 31) || (int64_t)N * Cout * H * W >= (1ll << 31) || Cout > 1024) return 1;
    // the kernel addresses an image of enc / bu through a buffer descriptor: 32-bit byte offsets and a 32-bit byte count per image
    if ((int64_t)Cin * H * W * 4 >= (1ll << 31) || (int64_t)Cout * (H / 2) * (W / 2) * 4 >= (1ll << 31)) return 1;
    int G = Cin, r = Cout;                                         // groups = gcd(Cin, Cout), nn_layers/efficient_pt.py:19
    while (r) { const int t = G % r; G = r; r = t; }
    const int cg = Cin / G, cob = Cout / G;
    DmGeom g;
    g.N = N; g.Cin = Cin; g.Cout = Cout; g.H = H; g.W = W; g.Hi = H / 2; g.Wi = W / 2;
    g.sh = bilinear_scale(g.Hi, H);
    g.sw = bilinear_scale(g.Wi, W);
    if (!dm_sources_pair_up(g.sh, g.Hi, H) || !dm_sources_pair_up(g.sw, g.Wi, W)) return 1;
    const int lprt = W / 2;
    g.ncb = ceil_div(lprt, 64);
    g.LPR = ceil_div(lprt, g.ncb);
    g.SUB = 64 / g.LPR;
    g.rpw = ceil_div(H / 2, g.SUB);
    const int64_t waves = (int64_t)N * g.ncb * g.rpw;
    if (waves >= (1ll << 31)) return 1;
    g.total = (unsigned)waves;
    int rc = 1;
    if (cg == 1 && cob == 1) rc = dm_launch<1, 1, false>(a, g, P, out, s);            // depthwise: one order in every 3x3 kernel
    else if (cg == 8 && cob == 3) rc = dm_launch<8, 3, false>(a, g, P, out, s);       // always the LDS-tiled conv3x3_kernel
    else if (cg == 4 && cob == 1 && G >= 16 && (W & 3) == 0 && W >= 16 && W <= 256 && H >= 4)   // what gconv3x3_stream_kernel<4,1> takes
        rc = dm_launch<4, 1, true>(a, g, P, out, s);
    if (rc) return rc;
    MSPL_CHECK_LAUNCH("decoder_merge");
    return 0;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_decoder_merge_fwd(const float* enc, const float* bu, const float* w3, const float* e_scale, const float* e_shift,
                                      const float* e_alpha, const float* gate, const float* b_scale, const float* b_shift,
                                      const float* b_alpha, const float* wp, const float* p_scale, const float* p_shift,
                                      const float* p_alpha, int32_t N, int32_t Cin, int32_t Cout, int32_t P, int32_t H, int32_t W,
                                      float* out, void* stream) {
    MSPL_REQUIRE(enc && bu && w3 && e_scale && e_shift && e_alpha && gate && b_scale && b_shift && b_alpha && wp && p_scale &&
                 p_shift && p_alpha && out, MSPL_ERR_NULL_POINTER, "decoder_merge: null pointer");
    MSPL_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && P > 0 && H > 0 && W > 0, MSPL_ERR_BAD_SHAPE,
                 "decoder_merge: bad shape N=%d Cin=%d Cout=%d P=%d H=%d W=%d", N, Cin, Cout, P, H, W);
    const DmParams a = {enc, bu, w3, e_scale, e_shift, e_alpha, gate, b_scale, b_shift, b_alpha, wp, p_scale, p_shift, p_alpha};
    const int rc = decoder_merge_try(a, N, Cin, Cout, P, H, W, out, (hipStream_t)stream);
    if (rc < 0) return rc;
    MSPL_REQUIRE(rc == 0, MSPL_ERR_UNSUPPORTED, "decoder_merge: Cin=%d Cout=%d P=%d H=%d W=%d is not a fused shape", Cin, Cout, P, H, W);
    return MSPL_OK;
}
