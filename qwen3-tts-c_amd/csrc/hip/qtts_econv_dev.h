// qtts_econv_dev.h - what the voice-clone encoders' two contraction kernels
// share (k_enc.hip: k_econv, k_econv_reduce and launch_econv; k_econvh.hip: the
// one-plane bf16 k_econvh): the launch descriptor, the epilogue and the bf16
// pack.  The device functions are file-local to the including unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qtts_enc.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

enum { PAD_ZERO = 0, PAD_REFLECT = 1, PAD_REPLICATE = 2 };
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_RELU_TANH = 2, ACT_GELU = 3, ACT_SIGMOID = 4 };

struct EConv {
    const unsigned short *w = nullptr;  // [3][M][Kp] bf16 planes
    size_t wplane = 0;                  // M * Kp
    int M = 0, K = 0, Kp = 0, kw = 1, stride = 1, dil = 1, padl = 0, pmode = PAD_ZERO, act_in = ACT_NONE;
    const float *x = nullptr, *x2 = nullptr;   // x'(ci, t) = x[b*xb + ci*xc + t*xt] (+ x2, same strides)
    size_t xb = 0;
    int xc = 0, xt = 1;
    int lin[ENC_MAXB], lout[ENC_MAXB];
    float *y = nullptr;                 // y[b*yb + m*yc + n*yt]
    size_t yb = 0;
    int yc = 0, yt = 1;
    const float *bias = nullptr;        // [M]
    const float *bias2 = nullptr;       // [b][bias2_b] per-utterance bias
    int bias2_b = 0;
    int act_out = ACT_NONE;
    const float *vec = nullptr;         // LayerScale [M] (after the activation)
    const float *res = nullptr;         // residual, res[b*rb + m*rc + n*rt]
    size_t rb = 0;
    int rc = 0, rt = 1;
    // split-K (set by launch_econv): blockIdx.z = b * kz + split; raw partial
    // tiles to part[split][b][M][pn], k_econv_reduce sums them in split order
    float *part = nullptr;
    int kz = 1, pn = 0, nb = 1;
};

// k_econvh.hip: k_econvh<rows> on launch_econv's grid for the same plan (g.kz,
// g.nb, g.pn and g.part set as for k_econv; k_econv_reduce follows for kz > 1)
void qtts_econvh_launch(const EConv &g, bool rows, dim3 grid, hipStream_t st);
long long qtts_econvh_launches();   // launches since the library loaded

namespace {

__device__ __forceinline__ void econv_store(const EConv &g, int b, int m, int n, float v) {
    const float *bias2 = g.bias2 ? g.bias2 + (size_t)b * g.bias2_b : nullptr;
    if (g.bias) v += g.bias[m];
    if (bias2) v += bias2[m];
    switch (g.act_out) {
        case 1: v = fmaxf(v, 0.f); break;
        case 2: v = tanhf(fmaxf(v, 0.f)); break;
        case 3: v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); break;
        case 4: v = 1.0f / (1.0f + expf(-v)); break;
        default: break;
    }
    if (g.vec) v *= g.vec[m];
    if (g.res) v += g.res[(size_t)b * g.rb + (size_t)m * g.rc + (size_t)n * g.rt];
    g.y[(size_t)b * g.yb + (size_t)m * g.yc + (size_t)n * g.yt] = v;
}

// two floats -> two bf16 (nearest even), lo in the low half
__device__ __forceinline__ uint32_t e_pk(float lo, float hi) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    const bf2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

}  // namespace
