// qtts_bgemv_dev.h - the device layer of the three lock-step batch GEMVs
// (k_gemvm.hip: 2..16 rows, x planes staged per workgroup; k_gemvb.hip: 2..16
// rows, x slices per wave; k_gemvx.hip: 17..64 rows, a moving K step per
// wave): the source kinds, the table-row lookup, bf16 packing, the exact
// 3-plane split, buffer-descriptor loads, the epilogue and the self-reducing
// split-K tail.
// The staging of an x unit, the weight-fragment offsets, the partial sum, the
// 3-plane MFMA step and the D-tile output stay written out in each kernel,
// although k_gemvb and k_gemvx share the text: as __forceinline__ helpers they
// change every instruction stream (the callee is canonicalised on its own
// before it is inlined), the sum of squares beside them can be contracted as
// fma(y, y, x x) for fma(x, x, y y) (k_gemvb<1, 1, 8, 0, 0>, <1, 1, 8, 0, 3>:
// other bits), and the variant that kept every bit measured 0.2 % (8 rows) and
// 0.6 % (32, 64 rows) slower end to end: profiles/bgemv_refactor_bench.txt.
#pragma once
#include "qtts_common.h"
#include "qtts_kernels.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// Source kinds: a kernel specialised on one has no branch between its loads,
// so the compiler's vmcnt bookkeeping stays exact (a uniform branch between
// source kinds that issue different loads into different registers makes it
// wait for every outstanding load -- the weights included -- at the join);
// BG_SRC_ANY decides at run time (k_gemvm's generic path).
enum { BG_SRC_X = 0, BG_SRC_XADD = 1, BG_SRC_TAB = 2, BG_SRC_TABF = 3, BG_SRC_ANY = 4 };

// k_gemvx's workgroup: waves, and the staged row stride in floats (32 columns
// + 4: fragment reads spread over banks); the planner sizes its LDS by them
constexpr int QTTS_GX_W = 8, QTTS_GX_LDX = 36;

namespace qtts_gm {

// the leading (preloaded) kernel arguments of k_gemvb / k_gemvx: the source's
// base by kind, and the ids of a table source
inline const void *src_base(const GemvArgs &a, int src) {
    return src == BG_SRC_TAB ? (const void *)a.table : src == BG_SRC_TABF ? (const void *)a.table_f32 : (const void *)a.x;
}
inline const int *src_ids(const GemvArgs &a, int src) {
    return src == BG_SRC_TAB || src == BG_SRC_TABF ? a.ids + a.ids_off : nullptr;
}

// id of the table row that batch row b reads (ids: a.ids + a.ids_off)
__device__ __forceinline__ unsigned row_id(const GemvArgs &a, const int *ids, int b) {
    const int *p = ids + (size_t)b * a.ids_bstride;
    if (a.row_sel) p += (size_t)a.row_sel[b] * a.ids_rstride;
    return (unsigned)*p;
}

// two f32 -> packed bf16 (round to nearest even: v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    const bf2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float lo_f(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float hi_f(uint32_t p) { return __uint_as_float(p & 0xFFFF0000u); }

// x = x1 + x2 + x3 (each bf16, exact: 24 mantissa bits in three 8-bit pieces)
// for 4 values; p1 / p2 / p3 receive 4 packed bf16 each (8 B)
__device__ __forceinline__ void split4(float4 v, uint2 &p1, uint2 &p2, uint2 &p3) {
    const uint32_t a1 = pk_bf16(v.x, v.y), b1 = pk_bf16(v.z, v.w);
    const float ex = v.x - lo_f(a1), ey = v.y - hi_f(a1), ez = v.z - lo_f(b1), ew = v.w - hi_f(b1);
    const uint32_t a2 = pk_bf16(ex, ey), b2 = pk_bf16(ez, ew);
    const uint32_t a3 = pk_bf16(ex - lo_f(a2), ey - hi_f(a2)), b3 = pk_bf16(ez - lo_f(b2), ew - hi_f(b2));
    p1 = make_uint2(a1, b1);
    p2 = make_uint2(a2, b2);
    p3 = make_uint2(a3, b3);
}

// buffer descriptor over a wave-uniform base (kernel arguments): loads take a
// 32-bit byte offset instead of a 64-bit address per lane (cdna_hip_programming.md T8)
// (readfirstlane makes the uniformity provable: no waterfall loop per load, T20)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *p) {
    const uint64_t u = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    void *q = (void *)(uintptr_t)(((uint64_t)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(q, (short)0, 0x7FFFFFF0, 0x00020000);
}
// float4 at element offset eoff
__device__ __forceinline__ float4 ld4(__amdgpu_buffer_rsrc_t r, unsigned eoff) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, eoff * 4u, 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// Self-reducing split-K (GemvArgs::tick), hand-off form R1 of
// cdna_hip_programming.md Guideline 16 (as k_attn_dec's split merge): the
// partials went out write-through (sc1), every wave drains them, one relaxed
// ticket add per workgroup; the last column to arrive adds the kz partials of
// its row block (nr rows) in column order to the residual (the order the
// consumer's xadd prologue used) and resets the ticket.
__device__ __forceinline__ void reduce_last(const GemvArgs &a, int nr, int *flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int old = __hip_atomic_fetch_add(a.tick + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        flag[0] = old == (int)gridDim.y - 1;
    }
    __syncthreads();
    if (!flag[0]) return;
    const int rb = blockIdx.x * nr, kz = gridDim.y;
    for (int i = threadIdx.x; i < a.nb * nr; i += blockDim.x) {
        const int b = i / nr, r = rb + (i - b * nr);
        if (r >= a.R) continue;
        // every partial (kz <= 4, host) and the residual issued before the sum
        const float *p = a.ypart + (size_t)b * a.R + r;
        float *y = a.y + (size_t)b * a.ldy + r;
        float t[4];
#pragma unroll
        for (int z = 0; z < 4; ++z) t[z] = ld_sc1(p + (size_t)(z < kz ? z : 0) * a.ld_ypart);
        const float y0 = *y;
        float s = t[0];
#pragma unroll
        for (int z = 1; z < 4; ++z)
            if (z < kz) s += t[z];
        *y = y0 + s;
    }
    if (threadIdx.x == 0) __hip_atomic_store(a.tick + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the GEMV epilogue of one output element val = (W x)[b][r]; `up` is the value
// 4 weight rows further (the SwiGLU partner of a gate row, row_shl:4)
__device__ __forceinline__ void epilogue(const GemvArgs &a, int bb, int r, float val, float up) {
    float *yr = a.y + (size_t)bb * a.ldy;
    switch (a.epi) {
        case EPI_STORE: yr[r] = val; break;
        case EPI_BIAS: yr[r] = val + a.bias[r]; break;
        case EPI_BIAS_SILU: {
            const float z = val + a.bias[r];
            yr[r] = z / (1.0f + expf(-z));
            break;
        }
        case EPI_RESID: yr[r] += val; break;
        case EPI_SWIGLU:
            if ((r & 7) < 4) yr[(r >> 3) * 4 + (r & 3)] = (val / (1.0f + expf(-val))) * up;
            break;
    }
}

}  // namespace qtts_gm
