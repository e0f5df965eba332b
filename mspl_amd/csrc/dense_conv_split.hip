// K13 in split-bf16 arithmetic -- the opt-in matrix mode of the ASPP heads' inference path (nn_layers/aspp.py:40-43 / :87-90 and
// conv_1x1_3 of :49 / :96).  The same implicit GEMM as dense_conv.hip,
//     out[co][p] = sum_tap sum_ci W[tap][co][ci] * x[ci][p shifted by tap]     (zero outside the image, padding = dilation),
// with every fp32 operand split into PLANES bf16 planes:  r_0 = v,  plane_i = bf16_rne(r_i),  r_{i+1} = r_i - float(plane_i)  (the
// subtraction is exact in fp32).  The products plane_i(w) * plane_j(x) with i + j < PLANES -- 3 for PLANES = 2 ("bf16x3"), 6 for
// PLANES = 3 ("bf16x6") -- run on v_mfma_f32_32x32x16_bf16 (16x the issue rate of the exact-fp32 MFMA of K13) and all add into the
// same fp32 accumulators, in a fixed order: the same inputs give the same bits.
//
// Weights arrive split (ops.pack_dense_weight_split): (planes, taps, Cout, Cin) bf16, Cin contiguous, so a lane's A fragment (8
// consecutive k of one row) is 16 bytes.  Activations stay fp32 in memory and are split while they are staged: a thread takes 8
// channels of one pixel (each of the 8 loads coalesced over the wave's pixels), converts with v_cvt_pk_bf16_f32 and writes one
// 16-byte chunk per plane to a [pixel][k] LDS image, so a B fragment is one ds_read_b128 as well.
// Both LDS images have rows of 32 k = 64 bytes padded to 80: a ds_read_b128 is served in groups of 16 lanes that hold the rows
// {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of one k chunk; row r starts at 16-byte slot 5r mod 16 of the 256-byte bank row, and
// both row sets cover every residue mod 16 once: conflict free.  The 16-byte stores of 8 consecutive pixels land on 8 distinct
// slots of the 128-byte store bank row.
// Workgroup tile, K chunk (32 channels = two 32x32x16 k-steps), register prefetch of the next chunk, wide form, accumulator layout
// and epilogue are K13's (the C/D layout of the bf16 32x32 MFMA equals that of 32x32x2_f32); the K loop runs channel chunks outer,
// taps inner (K13: taps outer).
#include "common.hpp"

namespace mspl {

typedef float floatx16s __attribute__((ext_vector_type(16)));
typedef float floatx2s __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8s __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2s __attribute__((ext_vector_type(2)));
typedef unsigned uintx4s __attribute__((ext_vector_type(4)));

struct DenseSplitGeom {
    int N, Cin, Cout, H, W, taps, dil;      // taps = 1 or 9
    int mblocks;
};

constexpr int DS_BM = 128, DS_KC = 32;
constexpr int DS_ROW = 5;                   // LDS row stride in 16-byte chunks: 4 chunks of 8 k + 1 pad (see the header)

// 8 fp32 values -> PLANES x 8 bf16 (one 16-byte chunk per plane, element j in bits 16*(j&1) of word j>>1: k order in memory)
template <int PLANES>
__device__ __forceinline__ void split8(const float (&v)[8], uintx4s (&pl)[PLANES]) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = v[j];
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const floatx2s f = {r[2 * q], r[2 * q + 1]};
            const unsigned bits = __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2s));      // v_cvt_pk_bf16_f32: RNE
            pl[p][q] = bits;
            if (p + 1 < PLANES) {
                r[2 * q] -= __uint_as_float(bits << 16);
                r[2 * q + 1] -= __uint_as_float(bits & 0xffff0000u);
            }
        }
    }
}

// WIDE = false: 128 output channels x 64 pixels, waves 4 x 1, a wave owns 32 rows x 64 pixels (two accumulator tiles).
// WIDE = true:  128 x 128 pixels, waves 2 x 2, a wave owns 64 rows x 64 pixels (four tiles) -- for grids that fill the chip.
template <int PLANES, bool WIDE>
__global__ __launch_bounds__(256, 2) void dense_conv_split_kernel(const float* __restrict__ x, const uintx4s* __restrict__ wsp,
                                                                  DenseSplitGeom g, Epi e, float* __restrict__ out) {
    constexpr int BN = WIDE ? 128 : 64;
    constexpr int TM = WIDE ? 2 : 1;                          // 32-row tiles per wave
    constexpr int NB = BN / 64;                               // 8-channel groups a thread stages per chunk
    constexpr int GSTEP = 4 / NB;
    __shared__ uintx4s As[PLANES * DS_BM * DS_ROW];
    __shared__ uintx4s Bs[PLANES * BN * DS_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const int wm = WIDE ? wave >> 1 : wave, wn = WIDE ? wave & 1 : 0;
    const int mb = blockIdx.x % g.mblocks, pt = blockIdx.x / g.mblocks;
    const int m0 = mb * DS_BM;
    const int HW = g.H * g.W;
    const int64_t P = (int64_t)g.N * HW;

    // B loader role: pixel column bj, channel groups bg0 + GSTEP * u (8 channels each)
    const int bj = tid & (BN - 1), bg0 = tid / BN;
    const int64_t bp = (int64_t)pt * BN + bj;
    const bool bpok = bp < P;
    const int bn = bpok ? (int)(bp / HW) : 0;
    const int brem = bpok ? (int)(bp - (int64_t)bn * HW) : 0;
    const int by = brem / g.W, bx = brem - by * g.W;
    const float* xn = x + (size_t)bn * g.Cin * HW;
    // A loader role: rows ar0 + 64 * u (u = 0, 1), 16-byte column acol of the 32-channel chunk, every plane
    const int acol = tid & 3, ar0 = tid >> 2;
    const int row16 = g.Cin / 8;                              // a weight row in 16-byte units
    const size_t plane16 = (size_t)g.taps * g.Cout * row16;

    floatx16s acc[TM][2];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nchunk = g.Cin / DS_KC;                         // Cin % 32 == 0 (launcher)
    const int nstage = g.taps * nchunk;
    uintx4s areg[PLANES][2];
    float breg[NB][8];
    auto fetch = [&](int stage) {
        // channel chunk outer, tap inner: the nine shifted reads of one 32-channel slab follow each other, so the taps that differ in
        // their x shift only hit the lines the previous stage just fetched instead of streaming the whole input once per tap
        const int chunk = g.taps == 9 ? stage / 9 : stage, tap = stage - chunk * g.taps, ci0 = chunk * DS_KC;
        const uintx4s* wt = wsp + ((size_t)tap * g.Cout + m0) * row16 + ci0 / 8 + acol;
#pragma unroll
        for (int p = 0; p < PLANES; ++p)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = ar0 + 64 * u;
                const uintx4s z = {0u, 0u, 0u, 0u};
                areg[p][u] = (m0 + r < g.Cout) ? wt[p * plane16 + (size_t)r * row16] : z;
            }
        int dy = 0, dx = 0;
        if (g.taps == 9) { dy = (tap / 3 - 1) * g.dil; dx = (tap % 3 - 1) * g.dil; }
        const int yy = by + dy, xx = bx + dx;
        const bool ok = bpok && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W;
        const float* src = xn + (size_t)ci0 * HW + (ok ? yy * g.W + xx : 0);
#pragma unroll
        for (int u = 0; u < NB; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) breg[u][j] = ok ? src[(size_t)(8 * (bg0 + GSTEP * u) + j) * HW] : 0.f;
    };
    auto stash = [&]() {
#pragma unroll
        for (int p = 0; p < PLANES; ++p)
#pragma unroll
            for (int u = 0; u < 2; ++u) As[(p * DS_BM + ar0 + 64 * u) * DS_ROW + acol] = areg[p][u];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            uintx4s pl[PLANES];
            split8<PLANES>(breg[u], pl);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) Bs[(p * BN + bj) * DS_ROW + bg0 + GSTEP * u] = pl[p];
        }
    };

    fetch(0);
    stash();
    __syncthreads();
    const uintx4s* ap = As + (wm * 32 * TM + li) * DS_ROW + half;
    const uintx4s* bpp = Bs + (wn * 64 + li) * DS_ROW + half;
    for (int stage = 0; stage < nstage; ++stage) {
        if (stage + 1 < nstage) fetch(stage + 1);            // global -> registers while this chunk is multiplied
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 2; ++s) {                         // k-step s: lane half h holds k = 16 s + 8 h + j = chunk 2 s + h
            bf16x8s a[PLANES][TM], b[PLANES][2];
#pragma unroll
            for (int p = 0; p < PLANES; ++p) {
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) a[p][tm] = __builtin_bit_cast(bf16x8s, ap[(p * DS_BM + tm * 32) * DS_ROW + 2 * s]);
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) b[p][tn] = __builtin_bit_cast(bf16x8s, bpp[(p * BN + tn * 32) * DS_ROW + 2 * s]);
            }
#pragma unroll
            for (int i = 0; i < PLANES; ++i)
#pragma unroll
                for (int j = 0; j < PLANES - i; ++j)          // the kept products: i + j < PLANES
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                        for (int tn = 0; tn < 2; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][tm], b[j][tn], acc[tm][tn], 0, 0, 0);
        }
        __syncthreads();
        if (stage + 1 < nstage) stash();
        __syncthreads();
    }

    // epilogue: lane holds pixel column li of tile tn, rows (r & 3) + 8 * (r >> 2) + 4 * half of tile tm
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int64_t p = (int64_t)pt * BN + wn * 64 + tn * 32 + li;
        if (p >= P) continue;
        const int n = (int)(p / HW);
        const int rem = (int)(p - (int64_t)n * HW);
        float* ob = out + ((size_t)n * e.ctot + e.coff) * (size_t)HW + rem;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + wm * 32 * TM + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < g.Cout) {
                    const int cabs = e.coff + co;
                    float v = acc[tm][tn][r];
                    v = fmaf(v, e.scale ? e.scale[cabs] : 1.f, e.shift ? e.shift[cabs] : 0.f);
                    if (e.alpha) v = v > 0.f ? v : e.alpha[cabs] * v;
                    ob[(size_t)co * HW] = v;
                }
            }
    }
}

template <int PLANES>
static void launch_split(bool wide, unsigned grid, hipStream_t stream, const float* x, const uintx4s* w, const DenseSplitGeom& g, const Epi& e,
                         float* out) {
    if (wide)
        hipLaunchKernelGGL((dense_conv_split_kernel<PLANES, true>), dim3(grid), dim3(256), 0, stream, x, w, g, e, out);
    else
        hipLaunchKernelGGL((dense_conv_split_kernel<PLANES, false>), dim3(grid), dim3(256), 0, stream, x, w, g, e, out);
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_dense_conv_split_fits(int32_t Cin, int32_t Cout, int32_t ksize, int32_t planes) {
    return (planes == 2 || planes == 3) && (ksize == 1 || ksize == 3) && Cin > 0 && Cin % DS_KC == 0 && Cout > 0 ? 1 : 0;
}

extern "C" int mspl_dense_conv_split_fwd(const float* x, const uint16_t* w_split, int32_t N, int32_t Cin, int32_t Cout, int32_t H,
                                         int32_t W, int32_t ksize, int32_t dilation, int32_t planes, const mspl_epilogue_t* ep,
                                         float* out, void* stream) {
    MSPL_REQUIRE(x && w_split && out, MSPL_ERR_NULL_POINTER, "dense_conv_split: null pointer");
    MSPL_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, MSPL_ERR_BAD_SHAPE,
                 "dense_conv_split: bad shape N=%d Cin=%d Cout=%d %dx%d", N, Cin, Cout, H, W);
    MSPL_REQUIRE(planes == 2 || planes == 3, MSPL_ERR_UNSUPPORTED, "dense_conv_split: %d planes (2 or 3)", planes);
    MSPL_REQUIRE(ksize == 1 || ksize == 3, MSPL_ERR_UNSUPPORTED, "dense_conv_split: kernel size %d (1 or 3)", ksize);
    MSPL_REQUIRE(dilation >= 1, MSPL_ERR_BAD_SHAPE, "dense_conv_split: dilation %d", dilation);
    MSPL_REQUIRE(Cin % DS_KC == 0, MSPL_ERR_UNSUPPORTED, "dense_conv_split: Cin=%d is not a multiple of %d", Cin, DS_KC);
    MSPL_REQUIRE((((uintptr_t)w_split) & 15) == 0, MSPL_ERR_UNSUPPORTED, "dense_conv_split: split weights must be 16-byte aligned");
    if (int rc = check_epi(ep, Cout, "dense_conv_split")) return rc;
    MSPL_REQUIRE(!ep || (!ep->pre_add && !ep->residual && !ep->reinf_r && !ep->gate), MSPL_ERR_UNSUPPORTED,
                 "dense_conv_split: only scale/shift/alpha epilogue terms are supported");
    MSPL_REQUIRE((int64_t)H * W < (1ll << 31) && (int64_t)ksize * ksize * Cout * (Cin / 8) < (1ll << 40), MSPL_ERR_BAD_SHAPE,
                 "dense_conv_split: image or weight too large");
    const Epi e = make_epi(ep, Cout, H * W);
    DenseSplitGeom g;
    g.N = N; g.Cin = Cin; g.Cout = Cout; g.H = H; g.W = W; g.taps = ksize * ksize; g.dil = dilation;
    g.mblocks = ceil_div(Cout, DS_BM);
    const int64_t P = (int64_t)N * H * W;
    const bool wide = ceil_div64(P, 128) * g.mblocks >= 512;                  // enough 128-pixel tiles to fill the chip (K13's rule)
    const int64_t ptiles = ceil_div64(P, wide ? 128 : 64);
    MSPL_REQUIRE(ptiles * g.mblocks < (1ll << 31), MSPL_ERR_BAD_SHAPE, "dense_conv_split: grid too large");
    const unsigned grid = (unsigned)(ptiles * g.mblocks);
    const uintx4s* w = reinterpret_cast<const uintx4s*>(w_split);
    if (planes == 2)
        launch_split<2>(wide, grid, (hipStream_t)stream, x, w, g, e, out);
    else
        launch_split<3>(wide, grid, (hipStream_t)stream, x, w, g, e, out);
    MSPL_CHECK_LAUNCH("dense_conv_split");
    return MSPL_OK;
}
