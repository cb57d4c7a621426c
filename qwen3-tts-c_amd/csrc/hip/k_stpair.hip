// k_stpair.hip - the sub-talker's positions 0 and 1 as one two-row pass at
// batch 1 (gfx950): pair forms of k_gemvw (k_gemvw.hip) and k_attn_o
// (k_attn.hip).
//
// Pass 0's input (the talker hidden) and pass 1's (the table row of the
// talker's draw) are both known when the sub-talker starts, so the two
// positions run as a causal two-token prefill: every sub-talker matrix is
// read once for both rows and the launch boundary and the dependent x fetch
// are paid once.  Per row the arithmetic and its order are those of the
// single-row kernels, so each output row is bit-identical to a single-row
// launch (tests/test_gpu_st_pair.py compares them bit for bit).
//
// A file of its own (built with the same kernarg preload as k_gemvw.hip and
// k_attn.hip) so that the single-row kernels' code objects stay exactly as
// they were.
#include "qtts_common.h"
#include "qtts_kernels.h"
#include "qtts_l2pf.h"

namespace {

__device__ __forceinline__ float dot8w(const v4u &w, const float *x) {
    const float4 x0 = *reinterpret_cast<const float4 *>(x);
    const float4 x1 = *reinterpret_cast<const float4 *>(x + 4);
    float s = 0.f;
    s = fmaf(__uint_as_float(w.x << 16), x0.x, s); s = fmaf(__uint_as_float(w.x & 0xFFFF0000u), x0.y, s);
    s = fmaf(__uint_as_float(w.y << 16), x0.z, s); s = fmaf(__uint_as_float(w.y & 0xFFFF0000u), x0.w, s);
    s = fmaf(__uint_as_float(w.z << 16), x1.x, s); s = fmaf(__uint_as_float(w.z & 0xFFFF0000u), x1.y, s);
    s = fmaf(__uint_as_float(w.w << 16), x1.z, s); s = fmaf(__uint_as_float(w.w & 0xFFFF0000u), x1.w, s);
    return s;
}

// The single-row kernels' code objects round these expressions in one fixed
// way (read off their gfx950 ISA); the pair kernels spell the same roundings
// out so that contraction cannot choose another:
//   sum of squares and the RoPE products: every product and sum rounded
//   score chunk q4 . k4: y's product, then x, z, w as fused multiply-adds --
//   except the last of a lane's four chunks at HD >= 32, whose products and
//   sums are all rounded (k_attn_o<32 / 64 / 128>; k_attn_o<16> fuses all four)
//   P.V: fused multiply-adds in key order
__device__ __forceinline__ float sumsq4(const float4 &v) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y)), __fmul_rn(v.z, v.z)),
                     __fmul_rn(v.w, v.w));
}
__device__ __forceinline__ float dot4_fused(const float4 &q, const float4 &k) {
    return fmaf(q.w, k.w, fmaf(q.z, k.z, fmaf(q.x, k.x, __fmul_rn(q.y, k.y))));
}
__device__ __forceinline__ float dot4_rounded(const float4 &q, const float4 &k) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q.x, k.x), __fmul_rn(q.y, k.y)), __fmul_rn(q.z, k.z)),
                     __fmul_rn(q.w, k.w));
}
// a c - b s / a c + b s with rounded products
__device__ __forceinline__ float rot_sub(float a, float c, float b, float s) {
    return __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, s));
}
__device__ __forceinline__ float rot_add(float a, float c, float b, float s) {
    return __fadd_rn(__fmul_rn(a, c), __fmul_rn(b, s));
}

// diagnostic phase stamps as in k_gemvw / k_attn_o (compiled in only with
// `make EXTRA=-DQTTS_STAMPS`): 100 MHz wall clock, one lane per workgroup
__device__ __forceinline__ void gw2_stamp(const GemvArgs &a, int k) {
#ifdef QTTS_STAMPS
    if (a.dbg && threadIdx.x == 0) a.dbg[blockIdx.x * 8 + k] = __builtin_amdgcn_s_memrealtime();
#endif
}
__device__ __forceinline__ void ao2_stamp(const AttnArgs &t, int k) {
#ifdef QTTS_STAMPS
    if (t.dbg && threadIdx.x == 0)
        t.dbg[(blockIdx.x + (size_t)gridDim.x * blockIdx.y) * 8 + k] = __builtin_amdgcn_s_memrealtime();
#endif
}

// ---------------------------------------------------------------------------
// Two-row k_gemvw<RW, NV, false>: y[b][r] = epilogue(sum_c W[r, c] xin[b][c]),
// b < 2.  Same mapping and load order as the single-row kernel: both x rows,
// their per-head partials (GemvArgs::xadd, row b of partial p at xadd +
// p ld_xadd + b ldb_xadd) and the norm weights first, then the residual rows
// of an EPI_RESID epilogue, then the lane's whole weight slice, then the
// next launch's prefetch.  One weight slice in registers; every dot8w chunk
// is applied to row 0's and row 1's staged x.
// x rows at stride ldx, y rows at stride ldy, xcopy rows (the new residual,
// written by workgroup 0) at stride ldxc.
// Dynamic LDS: [xs: 2 C floats][red: 2 x 4 floats].
template <int RW, int NV>
__global__ __launch_bounds__(256) void k_gemvw2(const float *x, const bf16_t *W, GemvArgs a) {
    gw2_stamp(a, 0);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int C = 512 * NV, XQ = C / 1024 > 0 ? (C + 1023) / 1024 : 1;   // float4 of x per thread and row
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row0 = blockIdx.x * 4 * RW;
    float *xs = smem, *red = smem + 2 * C;

    // 1. x, partials, norm weights
    constexpr int PMAX = XQ == 1 ? 8 : 0;
    float4 xv[2][XQ], pv[2][XQ][PMAX > 0 ? PMAX : 1], nwv[XQ];
    const int np = a.xadd ? a.n_xadd : 0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float *xrow = x + (size_t)b * a.ldx;
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int c = 4 * (tid + 256 * q);
            const int cc = c < C ? c : 0;
            xv[b][q] = *reinterpret_cast<const float4 *>(xrow + cc);
#pragma unroll
            for (int p = 0; p < PMAX; ++p)
                if (p < np)
                    pv[b][q][p] = *reinterpret_cast<const float4 *>(a.xadd + (size_t)p * a.ld_xadd +
                                                                    (size_t)b * a.ldb_xadd + cc);
        }
    }
#pragma unroll
    for (int q = 0; q < XQ; ++q) {
        const int c = 4 * (tid + 256 * q);
        if (a.norm_w) nwv[q] = *reinterpret_cast<const float4 *>(a.norm_w + (c < C ? c : 0));
    }

    // 1b. the residual rows of an EPI_RESID epilogue (rows owned by this
    //     workgroup; unconditional loads from a clamped address)
    const bool resid = a.epi == EPI_RESID;
    float yres[2][RW];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < RW; ++i) yres[b][i] = a.y[(size_t)b * a.ldy + (resid ? row0 + w + 4 * i : 0)];

    // 2. the weight slice of this lane in flight
    v4u wv[RW][NV];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        const v4u *p = reinterpret_cast<const v4u *>(W + (size_t)(row0 + w + 4 * i) * C) + lane;
#pragma unroll
        for (int k = 0; k < NV; ++k) wv[i][k] = p[64 * k];
    }
    // 2b. the next launch's weight slice into this XCD's L2 (GemvArgs::pf)
    L2PfRegs pfr;
    qtts_l2pf_issue<256, false>(a.pf, blockIdx.x, pfr, W);

    // 3. residual + partials summed in partial order, RMS statistic, per row
    float ss[2] = {0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int c = 4 * (tid + 256 * q);
            float4 v = xv[b][q];
            if (np > 0) {
                float4 s = pv[b][q][0];
#pragma unroll
                for (int p = 1; p < PMAX; ++p)
                    if (p < np) { s.x += pv[b][q][p].x; s.y += pv[b][q][p].y; s.z += pv[b][q][p].z; s.w += pv[b][q][p].w; }
                for (int p = PMAX; p < np; ++p) {
                    const float4 t = *reinterpret_cast<const float4 *>(a.xadd + (size_t)p * a.ld_xadd +
                                                                       (size_t)b * a.ldb_xadd + c);
                    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
                }
                v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w;
            }
            if (c >= C) v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.norm_w) ss[b] = __fadd_rn(ss[b], sumsq4(v));
            xv[b][q] = v;
        }
    }
    float inv[2] = {1.f, 1.f};
    if (a.norm_w) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            ss[b] = wave_sum(ss[b]);
            if (lane == 0) red[4 * b + w] = ss[b];
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 2; ++b)
            inv[b] = rms_inv(red[4 * b] + red[4 * b + 1] + red[4 * b + 2] + red[4 * b + 3], C, a.eps);
    }
    gw2_stamp(a, 1);
    const bool cp = a.xcopy && blockIdx.x == 0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int c = 4 * (tid + 256 * q);
            if (c < C) {
                float4 v = xv[b][q];
                if (cp) *reinterpret_cast<float4 *>(a.xcopy + (size_t)b * a.ldxc + c) = v;
                if (a.norm_w) {
                    const float4 nw = nwv[q];
                    v.x = v.x * inv[b] * nw.x; v.y = v.y * inv[b] * nw.y; v.z = v.z * inv[b] * nw.z; v.w = v.w * inv[b] * nw.w;
                }
                *reinterpret_cast<float4 *>(xs + b * C + c) = v;
            }
        }
    }
    __syncthreads();

    // 4. one wave per row: the lane's chunks in order against each x row, then the wave sums
    float acc[2][RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < NV; ++k) s += dot8w(wv[i][k], xs + b * C + 8 * (lane + 64 * k));
            acc[b][i] = wave_sum(s);
        }
    }
    gw2_stamp(a, 2);
    // Epilogue, one output per lane: every lane holds every sum (wave_sum), so
    // lane e takes the wave's output e -- row b = e / RW, i = e % RW (SwiGLU:
    // the gate / up pair e of the 2 x RW / 2) -- and the SiLUs and stores of
    // the two rows run side by side.  (Lane 0 doing all of them in turn, as
    // the single-row kernel does for its RW outputs, took 1.5 us of the pair
    // gate|up's 5.6 us in the in-graph stamps.)
    if (a.epi == EPI_SWIGLU) {
        if constexpr (RW >= 2) {
            float g = 0.f, u = 0.f;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int jj = 0; jj < RW / 2; ++jj)
                    if (lane == b * (RW / 2) + jj) { g = acc[b][2 * jj]; u = acc[b][2 * jj + 1]; }
            if (lane < RW) {
                const int b = lane / (RW / 2), i = 2 * (lane - b * (RW / 2));
                const int r = row0 + w + 4 * i;
                a.y[(size_t)b * a.ldy + (r >> 3) * 4 + (r & 3)] = (g / (1.0f + expf(-g))) * u;
            }
        }
    } else {
        float v = 0.f, yr = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < RW; ++i)
                if (lane == b * RW + i) { v = acc[b][i]; yr = yres[b][i]; }
        if (lane < 2 * RW) {
            const int b = lane / RW, r = row0 + w + 4 * (lane - b * RW);
            a.y[(size_t)b * a.ldy + r] = resid ? yr + v : v;
        }
    }
    gw2_stamp(a, 3);
    qtts_l2pf_sink(a.pf, pfr);
    gw2_stamp(a, 4);
}

// ---------------------------------------------------------------------------
// Two-row k_attn_o<HD>: row 0 at position 0, row 1 at position 1 of slot 0.
// Same grid (row blocks x kv heads).  Each workgroup stages both rows'
// q0|q1|k|v -- 8 segments of HD/4 lanes: per-head RMSNorm, RoPE at the row's
// position -- with the expressions of attn_short_wg (qtts_attn_dev.h) in its
// order.  Row 0 attends to its own key; row 1 to keys {0, 1}, key 0's k and v
// being the values staged here from row 0 (another workgroup of this launch
// stores them): no K/V cache row is read.  One W_o fragment per lane
// multiplies both rows' attention: part[(kvh 2 + j) R + row].
// rb == 0 stores both rows' k / v at cache rows 0 and 1 (unless skip[0]).
// AttnArgs::xc_dst (layer 0): the last workgroup also copies row 1's input
// table row (xc_tab fp32 / xc_tab16 bf16, xc_n wide) to xc_dst.
// row1: row 1's q|k|v row, or the q|k|v table with ids != nullptr (row *ids).
template <int HD>
__global__ __launch_bounds__(256) void k_attn_o2(const float *row0, const float *row1, const int *ids, AttnArgs t,
                                                 const bf16_t *Wo, int R, float *part) {
    constexpr int W2 = 2 * HD, LPS = W2 / 8 < 8 ? W2 / 8 : 8, NJ = W2 / (8 * LPS), RPW = 256 / LPS;
    constexpr int D4 = HD / 4, LPK = HD / 16, NK = 16;
    __shared__ __attribute__((aligned(16))) float lq[2 * 4 * HD];   // per row: rotated q0 | q1 | k, raw v
    __shared__ __attribute__((aligned(16))) float att[2 * W2];
    __shared__ float sc[2 * 2 * NK];
    const int tid = threadIdx.x, kvh = blockIdx.y, rb = blockIdx.x;
    ao2_stamp(t, 0);
    const int slot = tid / LPS, sub = tid - slot * LPS;
    const int row = rb * RPW + slot, rowc = row < R ? row : R - 1;
    const int AD = t.NH * HD, KVD = t.KV * HD;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- every load first: both rows' q0|q1|k|v, the norm weights and RoPE rows
    const int seg = tid / D4, l = tid - seg * D4;   // seg = 4 j + kind; kind 0, 1: query heads, 2: k, 3: v
    const int j = seg >> 2, kind = seg & 3;
    size_t xid = 0;
    if (ids) xid = (size_t)(*ids);
    // the slot's stop flag with the first loads (read where the cache rows are
    // stored it was one more dependent round trip in the rb == 0 workgroups)
    int skipv = *(t.skip ? t.skip : reinterpret_cast<const int *>(row0));
    if (!t.skip) skipv = 0;
    float4 x = zero4;
    if (seg < 8) {
        const float *rw = j ? row1 + xid * t.ld_qkv : row0;
        const float *src = kind < 2 ? rw + (2 * kvh + kind) * HD
                                    : rw + (kind == 2 ? t.NH * HD : (t.NH + t.KV) * HD) + kvh * HD;
        x = reinterpret_cast<const float4 *>(src)[l];
    }
    float4 nwq = zero4, c4 = zero4, s4 = zero4;
    if (seg < 8 && kind < 3) {
        nwq = reinterpret_cast<const float4 *>(kind < 2 ? t.qn_w : t.kn_w)[l];
        c4 = reinterpret_cast<const float4 *>(t.rope_cos + (size_t)j * HD)[l];
        s4 = reinterpret_cast<const float4 *>(t.rope_sin + (size_t)j * HD)[l];
    }
    // the residual copy's source (unconditional loads from clamped addresses)
    const bool xc = t.xc_dst != nullptr;
    const int xcc = xc && 4 * tid < t.xc_n ? 4 * tid : 0;
    const float4 xcf = *reinterpret_cast<const float4 *>(xc && t.xc_tab ? t.xc_tab + xid * t.xc_n + xcc : row0);
    const uint2 xch = *reinterpret_cast<const uint2 *>(
        xc && t.xc_tab16 ? reinterpret_cast<const void *>(t.xc_tab16 + xid * t.xc_n + xcc)
                         : reinterpret_cast<const void *>(row0));
    __builtin_amdgcn_sched_barrier(0);   // keep the W_o loads behind these
    // the weight fragment (row `row`, columns W2 kvh + 8 (sub + LPS jj)) and the next launch's slice
    v4u wv[NJ];
    const bf16_t *wr = Wo + (size_t)rowc * AD + W2 * kvh + 8 * sub;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) wv[jj] = *reinterpret_cast<const v4u *>(wr + 8 * LPS * jj);
    L2PfRegs pfr;
    qtts_l2pf_issue<256>(t.pf, blockIdx.x + gridDim.x * blockIdx.y, pfr, Wo);

    // ---- per-head RMSNorm + RoPE -> LDS; k, v -> cache rows 0 and 1
    float ss = sumsq4(x);
    ss = group_sum<D4>(ss);
    if (kind < 3) {
        const float iv = rms_inv(ss, HD, t.eps);
        const float4 wq = nwq;
        x.x = x.x * iv * wq.x; x.y = x.y * iv * wq.y; x.z = x.z * iv * wq.z; x.w = x.w * iv * wq.w;
    }
    float4 o4;
    if constexpr (D4 / 2 == 16) {   // the rotate-half partner one row away
        o4.x = xor16_get(x.x); o4.y = xor16_get(x.y); o4.z = xor16_get(x.z); o4.w = xor16_get(x.w);
    } else {
        o4.x = __shfl_xor(x.x, D4 / 2, 64); o4.y = __shfl_xor(x.y, D4 / 2, 64);
        o4.z = __shfl_xor(x.z, D4 / 2, 64); o4.w = __shfl_xor(x.w, D4 / 2, 64);
    }
    if (seg < 8) {
        float4 y = x;
        if (kind < 3) {
            if (l < D4 / 2) {   // x[i] c[i] - x[i+half] s[i]
                y.x = rot_sub(x.x, c4.x, o4.x, s4.x); y.y = rot_sub(x.y, c4.y, o4.y, s4.y);
                y.z = rot_sub(x.z, c4.z, o4.z, s4.z); y.w = rot_sub(x.w, c4.w, o4.w, s4.w);
            } else {            // x[i+half] c[i] + x[i] s[i]
                y.x = rot_add(x.x, c4.x, o4.x, s4.x); y.y = rot_add(x.y, c4.y, o4.y, s4.y);
                y.z = rot_add(x.z, c4.z, o4.z, s4.z); y.w = rot_add(x.w, c4.w, o4.w, s4.w);
            }
        }
        reinterpret_cast<float4 *>(lq)[tid] = y;   // lq[j][kind][4 l]
        if (kind >= 2 && rb == 0 && !skipv) {
            float *dst = (kind == 2 ? t.kc : t.vc) + (size_t)j * KVD + kvh * HD;
            reinterpret_cast<float4 *>(dst)[l] = y;
        }
    }
    if (xc && rb == (int)gridDim.x - 1 && kvh == (int)gridDim.y - 1) {   // row 1's input row as its residual
        for (int c = 4 * tid; c < t.xc_n; c += 4 * 256) {
            float4 v = xcf;
            uint2 u = xch;
            if (c != 4 * tid) {
                if (t.xc_tab) v = *reinterpret_cast<const float4 *>(t.xc_tab + xid * t.xc_n + c);
                else u = *reinterpret_cast<const uint2 *>(t.xc_tab16 + xid * t.xc_n + c);
            }
            if (!t.xc_tab)
                v = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u),
                                __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xFFFF0000u));
            *reinterpret_cast<float4 *>(t.xc_dst + c) = v;
        }
    }
    __syncthreads();

    // ---- scores q_j . k_ts / sqrt(HD), ts <= j: HD/16 lanes per (row, query head, key)
    {
        const int dI = tid / LPK, su = tid - dI * LPK;
        const int sj = dI >> 2, gs = (dI >> 1) & 1, ts = dI & 1;
        const bool live = dI < 8 && ts <= sj;
        float d = 0.f;
        if (live) {
            const float4 *q4 = reinterpret_cast<const float4 *>(lq + sj * 4 * HD + gs * HD + 16 * su);
            const float4 *k4 = reinterpret_cast<const float4 *>(lq + ts * 4 * HD + 2 * HD + 16 * su);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 k = k4[c], q = q4[c];
                d = __fadd_rn(d, c == 3 && HD >= 32 ? dot4_rounded(q, k) : dot4_fused(q, k));
            }
        }
        d = group_sum<LPK>(d);
        if (su == 0 && live) sc[(sj * 2 + gs) * NK + ts] = d * div_rn(1.0f, sqrt_rn((float)HD));
    }
    __syncthreads();

    // ---- softmax per (row, head) over its j + 1 keys (16-lane groups, as the single-row kernel)
    if (tid < 4 * NK) {
        const int sj = tid / (2 * NK), tt = tid & (NK - 1), n = sj + 1;
        const float s = tt < n ? sc[tid] : -INFINITY;
        float m = s;
        m = group_max<NK>(m);
        const float e = tt < n ? expf(s - m) : 0.f;
        float sum = e;
        sum = group_sum<NK>(sum);
        sc[tid] = e * div_rn(1.0f, sum);
    }
    __syncthreads();

    // ---- P.V, keys in order: row 0 over key 0, row 1 over keys 0, 1
    if (tid < W2) {
        const int go = tid / HD, dd = tid - go * HD;
        const float v0 = lq[3 * HD + dd], v1 = lq[4 * HD + 3 * HD + dd];
        float a0 = 0.f;   // (row 0: 0 + 1 v, the single-row kernel's expression)
        a0 = fmaf(sc[go * NK], v0, a0);
        float a1 = 0.f;
        a1 = fmaf(sc[(2 + go) * NK], v0, a1);
        a1 = fmaf(sc[(2 + go) * NK + 1], v1, a1);
        att[go * HD + dd] = a0;
        att[W2 + go * HD + dd] = a1;
    }
    __syncthreads();

    ao2_stamp(t, 4);
    // ---- the O projection's columns of this head pair, both rows against one fragment
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        float f[8];
        unpack8(wv[jj], f);
        const float *xp = att + 8 * (sub + LPS * jj);
        const float4 x0 = *reinterpret_cast<const float4 *>(xp);
        const float4 x1 = *reinterpret_cast<const float4 *>(xp + 4);
        acc0 = fmaf(f[0], x0.x, acc0); acc0 = fmaf(f[1], x0.y, acc0);
        acc0 = fmaf(f[2], x0.z, acc0); acc0 = fmaf(f[3], x0.w, acc0);
        acc0 = fmaf(f[4], x1.x, acc0); acc0 = fmaf(f[5], x1.y, acc0);
        acc0 = fmaf(f[6], x1.z, acc0); acc0 = fmaf(f[7], x1.w, acc0);
        const float4 z0 = *reinterpret_cast<const float4 *>(xp + W2);
        const float4 z1 = *reinterpret_cast<const float4 *>(xp + W2 + 4);
        acc1 = fmaf(f[0], z0.x, acc1); acc1 = fmaf(f[1], z0.y, acc1);
        acc1 = fmaf(f[2], z0.z, acc1); acc1 = fmaf(f[3], z0.w, acc1);
        acc1 = fmaf(f[4], z1.x, acc1); acc1 = fmaf(f[5], z1.y, acc1);
        acc1 = fmaf(f[6], z1.z, acc1); acc1 = fmaf(f[7], z1.w, acc1);
    }
    acc0 = group_sum<LPS>(acc0);
    acc1 = group_sum<LPS>(acc1);
    ao2_stamp(t, 2);
    if (sub == 0 && row < R) {
        part[((size_t)kvh * 2 + 0) * R + row] = acc0;
        part[((size_t)kvh * 2 + 1) * R + row] = acc1;
    }
    qtts_l2pf_sink(t.pf, pfr);
    ao2_stamp(t, 3);
}

}  // namespace

// shapes the pair GEMV serves: C = 512 NV, R = 1024 RW, one workgroup per CU
bool qtts_gemvw_pair_covers(int R, int C, int epi) {
    if (R < 1024 || C < 512 || R % 1024 || C % 512) return false;
    if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU) return false;
    const int RW = R / 1024, NV = C / 512;
    if (epi == EPI_SWIGLU && (RW & 1)) return false;
    return (RW == 4 && NV == 2) || (RW == 6 && NV == 2) || (RW == 1 && NV == 6) || (RW == 1 && NV == 2) ||
           (RW == 2 && NV == 2);
}

// Two x rows (a.x, stride a.ldx) against one weight stream: 1 = not covered.
int qtts_gemvw_pair(const GemvArgs &a, hipStream_t st) {
#ifdef QTTS_ARGDUMP
    qtts_argdump::gemv("qtts_gemvw_pair", a);
#endif
    if (a.nb != 2 || !qtts_gemvw_pair_covers(a.R, a.C, a.epi)) return 1;
    if (a.table || a.table_f32 || a.amerge || a.ypart || a.reps != 1 || a.nt || a.xcopy_normed || !a.x || !a.y) return 1;
    if (a.ldx % 4 || a.ldx < a.C || ((uintptr_t)a.x & 15)) return 1;
    // (partials only at C <= 1024, where the first 8 are held in registers, as in k_gemvw)
    if (a.xadd && (((uintptr_t)a.xadd & 15) || a.ld_xadd % 4 || a.ldb_xadd % 4 || a.n_xadd < 1 || a.C > 1024)) return 1;
    if (a.norm_w && ((uintptr_t)a.norm_w & 15)) return 1;
    if (a.xcopy && (((uintptr_t)a.xcopy & 15) || a.ldxc % 4 || a.ldxc < a.C)) return 1;
    if (a.ldy < (a.epi == EPI_SWIGLU ? a.R / 2 : a.R)) return 1;
    const int NV = a.C / 512, RW = a.R / 1024;
    const dim3 grid(a.R / (4 * RW));
    const size_t smem = (size_t)(2 * a.C + 8) * sizeof(float);
#define QTTS_GW2(RW_, NV_)                                                                          \
    if (RW == RW_ && NV == NV_) {                                                                   \
        hipLaunchKernelGGL((k_gemvw2<RW_, NV_>), grid, dim3(256), smem, st, a.x, a.W, a);           \
        qtts_last_kernel = "k_gemvw2<" #RW_ ", " #NV_ ">";                                          \
        return hipGetLastError() == hipSuccess ? 0 : -1;                                            \
    }
    // sub-talker (Hs 1024): q|k|v 4096x1024, gate|up 6144x1024, down 1024x3072;
    // the small test models' 1024x1024 and 2048x1024
    QTTS_GW2(4, 2) QTTS_GW2(6, 2) QTTS_GW2(1, 6) QTTS_GW2(1, 2) QTTS_GW2(2, 2)
#undef QTTS_GW2
    return 1;
}

// Rows 0 and 1 of slot 0 at positions 0 and 1: a.qkv holds row 0 (and row 1 at
// a.qkv + a.ld_qkv unless a.qkv_tab is set: row 1 is then the table's row
// a.tab_ids[a.tab_off]); a.kc / a.vc the slot's cache [S][KV HD]; part
// [KV][2][R].  1 = not covered.
bool qtts_attn_o_pair_covers(const AttnArgs &a, const bf16_t *Wo) {
    return qtts_attn_o_covers(a, Wo) && a.S >= 2 && !a.pos && !a.tab_row_sel && a.qkv && a.ld_qkv % 4 == 0 &&
           ((uintptr_t)a.qkv & 15) == 0 && (!a.qkv_tab || (a.tab_ids && ((uintptr_t)a.qkv_tab & 15) == 0)) &&
           (!a.xc_dst || ((a.xc_tab || a.xc_tab16) && a.qkv_tab && a.xc_n >= 4 && a.xc_n % 4 == 0 &&
                          ((uintptr_t)a.xc_dst & 15) == 0));
}

int qtts_attn_o_pair(const AttnArgs &a, const bf16_t *Wo, int R, float *part, hipStream_t st) {
#ifdef QTTS_ARGDUMP
    qtts_argdump::attn("qtts_attn_o_pair", a, R, Wo, part);
#endif
    if (!qtts_attn_o_pair_covers(a, Wo)) return 1;
    const int W2 = 2 * a.HD, LPS = W2 / 8 < 8 ? W2 / 8 : 8, RPW = 256 / LPS;
    const dim3 grid((R + RPW - 1) / RPW, a.KV);
    const float *row1 = a.qkv_tab ? a.qkv_tab : a.qkv + a.ld_qkv;
    const int *ids = a.qkv_tab ? a.tab_ids + a.tab_off : nullptr;
    switch (a.HD) {
        case 128: hipLaunchKernelGGL((k_attn_o2<128>), grid, dim3(256), 0, st, a.qkv, row1, ids, a, Wo, R, part); qtts_last_kernel = "k_attn_o2<128>"; break;
        case 64: hipLaunchKernelGGL((k_attn_o2<64>), grid, dim3(256), 0, st, a.qkv, row1, ids, a, Wo, R, part); qtts_last_kernel = "k_attn_o2<64>"; break;
        case 32: hipLaunchKernelGGL((k_attn_o2<32>), grid, dim3(256), 0, st, a.qkv, row1, ids, a, Wo, R, part); qtts_last_kernel = "k_attn_o2<32>"; break;
        default: hipLaunchKernelGGL((k_attn_o2<16>), grid, dim3(256), 0, st, a.qkv, row1, ids, a, Wo, R, part); qtts_last_kernel = "k_attn_o2<16>"; break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
