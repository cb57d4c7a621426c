// qtts_xgemm_dev.h - device pieces the codec's contraction kernels share
// (k_codec.hip: k_xgemm, k_conv, k_convb, k_xlin, k_xgemv and the reduce
// kernels; k_convh.hip: the one-plane bf16 conv): SnakeBeta with its sin^2,
// the stream axis' segment offsets, the epilogues, the conv tile constants and
// the bf16 pack.  Every function is file-local to the including unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qtts_codec.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

namespace {

// sin^2(r): the sign of sin drops out, so one Cody-Waite step by pi
// (pi = PI_HI + PI_LO; both products exact inside the fmas, k exact below
// 2^24) and the odd Taylor series through y^13 on [-pi/2, pi/2] (truncation
// < 1e-9) give sinf(r)^2 to 2.2e-7 absolute (checked over |r| <= 8192) in
// ~15 instructions instead of the general sinf's ~90 plus its inlined
// large-argument path.
__device__ __forceinline__ float sin2(float r) {
    const float k = rintf(r * 0.318309886183790672f);
    float y = fmaf(-k, 3.14159274101257324f, r);
    y = fmaf(-k, -8.74227765734758577e-08f, y);
    const float y2 = y * y;
    float p = 1.6059043836821613e-10f;                 // 1/13!
    p = fmaf(p, y2, -2.5052108385441720e-08f);         // -1/11!
    p = fmaf(p, y2, 2.7557319223985893e-06f);          // 1/9!
    p = fmaf(p, y2, -1.9841269841269841e-04f);         // -1/7!
    p = fmaf(p, y2, 8.3333333333333333e-03f);          // 1/5!
    p = fmaf(p, y2, -1.6666666666666667e-01f);         // -1/3!
    const float sn = fmaf(y * y2, p, y);
    return sn * sn;
}

__device__ __forceinline__ float snake1(float x, float a, float ib) { return x + ib * sin2(x * a); }

// stream axis (XGemm::nseg / seg_m).  Conv forms: workgroup column bx of the
// grid is tile bx % tiles of segment bx / tiles; xg_seg moves the operands to
// that segment (nz: the main kernel's grid z, whose partials a segment owns).
__device__ __forceinline__ void xg_seg(XGemm &g, int sg, int nz) {
    g.B += (size_t)sg * g.seg_ldb;
    g.C += (size_t)sg * g.seg_ldc;
    if (g.res) g.res += (size_t)sg * g.seg_ldres;
    if (g.part) g.part += (size_t)sg * nz * g.M * g.N;
}
__device__ __forceinline__ int xg_seg_tile(XGemm &g) {
    int bx = blockIdx.x;
    if (g.nseg > 1) {
        const int tps = gridDim.x / g.nseg, sg = bx / tps;
        bx -= sg * tps;
        xg_seg(g, sg, gridDim.z);
    }
    return bx;
}
// stacked rows: where row m of a per-segment operand lies (ld: its segment stride)
__device__ __forceinline__ size_t xg_srow(const XGemm &g, int m, int ld) {
    if (!g.seg_m) return (size_t)m;
    const int sg = m / g.seg_m;
    return (size_t)sg * ld + (m - sg * g.seg_m);
}

__device__ __forceinline__ float gelu_tanh(float v) {
    return 0.5f * v * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
}

__device__ __forceinline__ void xg_epi(const XGemm &g, int m, int n, float v) {
    switch (g.emode) {
        case XE_STORE: g.C[(size_t)m * g.ldc + n] = v; break;
        case XE_BIAS_N: g.C[(size_t)m * g.ldc + n] = v + g.bias[n]; break;
        case XE_BIAS_N_GELU: g.C[(size_t)m * g.ldc + n] = gelu_tanh(v + g.bias[n]); break;
        case XE_SILU_MUL: {
            const float gt = g.aux[(size_t)m * g.ldaux + n];
            g.C[(size_t)m * g.ldc + n] = (gt / (1.0f + expf(-gt))) * v;
            break;
        }
        case XE_SCALE_RESID_N: g.C[(size_t)m * g.ldc + n] += v * g.vec[n]; break;
        case XE_BIAS_T: g.C[(size_t)n * g.ldc + xg_srow(g, m, g.seg_ldc)] = v + g.bias[n]; break;
        case XE_BIAS_GAMMA_RES_T:
            g.C[(size_t)n * g.ldc + xg_srow(g, m, g.seg_ldc)] =
                (v + g.bias[n]) * g.vec[n] + g.res[(size_t)n * g.ldres + xg_srow(g, m, g.seg_ldres)];
            break;
        case XE_BIAS_M: {
            float y = v + (g.bias ? g.bias[m] : 0.f);
            if (g.stride > 1 || g.phase > 0) g.C[(size_t)m * g.ldc + (size_t)n * g.stride + g.phase] = y;
            else g.C[(size_t)m * g.ldc + n] = y;
            break;
        }
        case XE_BIAS_M_RES: g.C[(size_t)m * g.ldc + n] = v + g.bias[m] + g.res[(size_t)m * g.ldres + n]; break;
        case XE_BIAS_M_SNAKE: g.C[(size_t)m * g.ldc + n] = snake1(v + g.bias[m], g.ea[m], g.eb[m]); break;
    }
}

// the conv kernels' tile: 64 output channels, stages of whole 16-channel
// groups, and the staged window's halo >= (Kw-1)*dil (host-checked)
constexpr int CV_BM = 64, CV_BN = 128, CV_BC = 16, CV_HALO = 64;
constexpr int CB_SNAKE_MAX = 1536;   // input channels per split the bf16 conv kernels take with SnakeBeta (larger: k_conv)

// two floats -> two bf16 (round to nearest even), low half first
__device__ __forceinline__ uint32_t cb_pk(float lo, float hi) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    const bf2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

}  // namespace
