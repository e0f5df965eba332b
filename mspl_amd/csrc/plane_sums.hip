// Small sums of the training steps: per-plane dot products and broadcasts (global average pool and gate gradients), the
// EfficientPWConv gate backward, and the sum of up to eight equally shaped gradients in one launch (with or without a per-plane
// constant).
#include <stdlib.h>

#include <algorithm>

#include "common.hpp"

namespace mspl {

// ---- per-plane dot product: out[n*C + c] = sum_p a[n,c,p] * b[n,c,p]   (gate gradient; b == nullptr: plain sum)
__global__ __launch_bounds__(256) void plane_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, int HW,
                                                        float* __restrict__ out) {
    const size_t base = (size_t)blockIdx.x * HW;
    float s = 0.f;
    if ((HW & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) {          // 16-byte operands, four quads per operand in flight
        const float4* a4 = reinterpret_cast<const float4*>(a + base);
        const float4* b4 = b ? reinterpret_cast<const float4*>(b + base) : nullptr;
        const int L = HW >> 2;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll 4
        for (int i = threadIdx.x; i < L; i += 256) {
            const float4 x = a4[i], y = b4 ? b4[i] : one;
            s0 = fmaf(x.x, y.x, s0); s1 = fmaf(x.y, y.y, s1); s2 = fmaf(x.z, y.z, s2); s3 = fmaf(x.w, y.w, s3);
        }
        s = (s0 + s1) + (s2 + s3);
    } else
    for (int i = threadIdx.x; i < HW; i += 256) s = fmaf(a[base + i], b ? b[base + i] : 1.f, s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// ---- EfficientPWConv gate backward: gate = sigmoid(W . mean); given ggate (N,Cout):
//      gs = ggate * gate * (1 - gate); gW[co,ci] = sum_n gs[n,co] * mean[n,ci]; gmean[n,ci] = sum_co gs[n,co] * W[co,ci]
template <bool ACC>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ ggate, const float* __restrict__ gate,
                                                       const float* __restrict__ mean, const float* __restrict__ w, int N,
                                                       int Cin, int Cout, float* __restrict__ gw, float* __restrict__ gmean) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < Cout * Cin) {
        const int co = idx / Cin, ci = idx - co * Cin;
        float s = 0.f;
        // (unrolled: the loads of eight iterations leave together; one iteration at a time the two loops were 16 + Cout dependent L2
        // round trips: 20-31 us per launch for ~1 MB)
#pragma unroll 8
        for (int n = 0; n < N; ++n) {
            const float gt = gate[n * Cout + co];
            s = fmaf(ggate[n * Cout + co] * gt * (1.f - gt), mean[n * Cin + ci], s);
        }
        if (ACC) atomicAdd(&gw[idx], s); else gw[idx] = s;      // ACC: gw is the parameter's gradient buffer (other launches add to it too)
    }
    if (idx < N * Cin) {
        const int n = idx / Cin, ci = idx - n * Cin;
        float s = 0.f;
#pragma unroll 8
        for (int co = 0; co < Cout; ++co) {
            const float gt = gate[n * Cout + co];
            s = fmaf(ggate[n * Cout + co] * gt * (1.f - gt), w[co * Cin + ci], s);
        }
        gmean[idx] = s;
    }
}

// ---- broadcast a per-plane value over the plane (gx = v[n*C+c] * mul), optionally accumulating
__global__ __launch_bounds__(256) void plane_broadcast_kernel(const float* __restrict__ v, int HW, float mul, int accumulate,
                                                              float* __restrict__ gx, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const float val = v[idx / HW] * mul;
    if (accumulate) gx[idx] += val; else gx[idx] = val;
}

}  // namespace mspl

using namespace mspl;

extern "C" int mspl_plane_dot(const float* a, const float* b, int32_t planes, int32_t HW, float* out, void* stream) {
    MSPL_REQUIRE(a && out, MSPL_ERR_NULL_POINTER, "plane_dot: null pointer");
    MSPL_REQUIRE(planes > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "plane_dot: bad shape");
    hipLaunchKernelGGL(plane_dot_kernel, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, a, b, HW, out);
    MSPL_CHECK_LAUNCH("plane_dot");
    return MSPL_OK;
}

extern "C" int mspl_plane_broadcast(const float* v, int32_t planes, int32_t HW, float mul, int32_t accumulate, float* gx,
                                    void* stream) {
    MSPL_REQUIRE(v && gx, MSPL_ERR_NULL_POINTER, "plane_broadcast: null pointer");
    MSPL_REQUIRE(planes > 0 && HW > 0, MSPL_ERR_BAD_SHAPE, "plane_broadcast: bad shape");
    const int64_t total = (int64_t)planes * HW;
    hipLaunchKernelGGL(plane_broadcast_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream, v, HW, mul,
                       accumulate, gx, total);
    MSPL_CHECK_LAUNCH("plane_broadcast");
    return MSPL_OK;
}

extern "C" int mspl_gap_gate_bwd(const float* ggate, const float* gate, const float* mean, const float* w, int32_t N,
                                 int32_t Cin, int32_t Cout, float* gw, float* gmean, void* stream) {
    MSPL_REQUIRE(ggate && gate && mean && w && gw && gmean, MSPL_ERR_NULL_POINTER, "gap_gate_bwd: null pointer");
    MSPL_REQUIRE(N > 0 && Cin > 0 && Cout > 0, MSPL_ERR_BAD_SHAPE, "gap_gate_bwd: bad shape");
    const int n = max(Cout * Cin, N * Cin);
    hipLaunchKernelGGL(gate_bwd_kernel<false>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, ggate, gate, mean, w, N,
                       Cin, Cout, gw, gmean);
    MSPL_CHECK_LAUNCH("gap_gate_bwd");
    return MSPL_OK;
}

extern "C" int mspl_gap_gate_bwd_accum(const float* ggate, const float* gate, const float* mean, const float* w, int32_t N,
                                       int32_t Cin, int32_t Cout, float* gw, float* gmean, void* stream) {
    MSPL_REQUIRE(ggate && gate && mean && w && gw && gmean, MSPL_ERR_NULL_POINTER, "gap_gate_bwd_accum: null pointer");
    MSPL_REQUIRE(N > 0 && Cin > 0 && Cout > 0, MSPL_ERR_BAD_SHAPE, "gap_gate_bwd_accum: bad shape");
    const int n = max(Cout * Cin, N * Cin);
    hipLaunchKernelGGL(gate_bwd_kernel<true>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, ggate, gate, mean, w, N,
                       Cin, Cout, gw, gmean);
    MSPL_CHECK_LAUNCH("gap_gate_bwd_accum");
    return MSPL_OK;
}

// out = sum of up to 8 equally shaped tensors in one launch (the gradient of a tensor with several consumers: autograd would add
// them pairwise, n - 1 launches that read 2 and write 1 tensor each).  Summation order: ((s0 + s1) + s2) + ... like the pairwise adds.
namespace mspl {
struct SumSrcs { const float* p[8]; };

__global__ __launch_bounds__(256) void sum_n_kernel(SumSrcs srcs, int n, int64_t count4, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count4) return;
    float4 a = reinterpret_cast<const float4*>(srcs.p[0])[i];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        if (k >= n) break;
        const float4 b = reinterpret_cast<const float4*>(srcs.p[k])[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    reinterpret_cast<float4*>(out)[i] = a;
}
}  // namespace mspl

extern "C" int mspl_sum_n(const float* const* srcs, int32_t n, int64_t count, float* out, void* stream) {
    MSPL_REQUIRE(srcs && out, MSPL_ERR_NULL_POINTER, "sum_n: null pointer");
    MSPL_REQUIRE(n >= 1 && n <= 8 && count >= 0 && (count & 3) == 0, MSPL_ERR_BAD_SHAPE, "sum_n: n=%d count=%lld (1..8 tensors, count %% 4 == 0)",
                 n, (long long)count);
    mspl::SumSrcs s;
    for (int k = 0; k < 8; ++k) {
        s.p[k] = k < n ? srcs[k] : srcs[0];
        MSPL_REQUIRE(s.p[k] && (((uintptr_t)s.p[k]) & 15) == 0, MSPL_ERR_NULL_POINTER, "sum_n: source %d is NULL or not 16-byte aligned", k);
    }
    MSPL_REQUIRE((((uintptr_t)out) & 15) == 0, MSPL_ERR_UNSUPPORTED, "sum_n: unaligned destination");
    if (count == 0) return MSPL_OK;
    hipLaunchKernelGGL(mspl::sum_n_kernel, dim3((unsigned)ceil_div64(count / 4, 256)), dim3(256), 0, (hipStream_t)stream, s, n, count / 4, out);
    MSPL_CHECK_LAUNCH("sum_n");
    return MSPL_OK;
}

namespace mspl {
// sum of n tensors + a per-plane constant (mul * pc[plane]): the gradient of a global average pool is constant over its plane, so the
// sum of an encoder output's gradients takes it as N * C values instead of a full-size tensor somebody wrote only to have it added
__global__ __launch_bounds__(256) void sum_n_planes_kernel(SumSrcs srcs, int n, const float* __restrict__ pc, float mul, int planes,
                                                           int HW4, float* __restrict__ out) {
    const int plane = blockIdx.z * gridDim.y + blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (plane >= planes || q >= HW4) return;           // the (y, z) plane split rounds up past planes > 65535
    const int64_t i = (int64_t)plane * HW4 + q;
    const float c = mul * pc[plane];
    float4 a = reinterpret_cast<const float4*>(srcs.p[0])[i];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        if (k >= n) break;
        const float4 b = reinterpret_cast<const float4*>(srcs.p[k])[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    a.x += c; a.y += c; a.z += c; a.w += c;
    reinterpret_cast<float4*>(out)[i] = a;
}
}  // namespace mspl

extern "C" int mspl_sum_n_planes(const float* const* srcs, int32_t n, const float* plane_const, float mul, int32_t planes, int32_t HW,
                                 float* out, void* stream) {
    MSPL_REQUIRE(srcs && out && plane_const, MSPL_ERR_NULL_POINTER, "sum_n_planes: null pointer");
    MSPL_REQUIRE(n >= 1 && n <= 8 && planes > 0 && HW > 0 && (HW & 3) == 0, MSPL_ERR_BAD_SHAPE,
                 "sum_n_planes: n=%d planes=%d HW=%d (1..8 tensors, HW %% 4 == 0)", n, planes, HW);
    mspl::SumSrcs s;
    for (int k = 0; k < 8; ++k) {
        s.p[k] = k < n ? srcs[k] : srcs[0];
        MSPL_REQUIRE(s.p[k] && (((uintptr_t)s.p[k]) & 15) == 0, MSPL_ERR_NULL_POINTER, "sum_n_planes: source %d is NULL or not 16-byte aligned", k);
    }
    MSPL_REQUIRE((((uintptr_t)out) & 15) == 0, MSPL_ERR_UNSUPPORTED, "sum_n_planes: unaligned destination");
    hipLaunchKernelGGL(mspl::sum_n_planes_kernel, plane_grid(ceil_div(HW / 4, 256), planes), dim3(256), 0, (hipStream_t)stream, s, n, plane_const,
                       mul, planes, HW / 4, out);
    MSPL_CHECK_LAUNCH("sum_n_planes");
    return MSPL_OK;
}
