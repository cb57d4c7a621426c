// k_gemvx.hip - wide lock-step batch decode GEMV (17..64 utterances) on the
// bf16 matrix cores.
//
// y[b, r] = epilogue( inv[b] * sum_c W[r, c] * (x[b, c] * nw[c]) ),  17 <= nb <= 64
//
// Role: k_gemvb's (the per-utterance kernel_matvec_bf16 /
// kernel_swiglu_matvec_bf16 calls and the rms_norm / residual passes around
// them, K.c:27-39, 95-149, 213-233, T.c:142-247, batched so that one weight
// read per launch serves every utterance), for more rows than one 16-row MFMA
// M tile.  k_gemvb keeps a wave's K slice of ALL rows in LDS for the whole
// launch; at 64 rows x 2048 columns that is 512 KB against 160 KB per
// workgroup, so here the slice MOVES: a wave owns one 32-column K step at a
// time.
//
// Mapping: a workgroup = TPW tiles of 16 weight rows x 8 waves.  The K steps
// of the workgroup's column (C / kz columns, gridDim.y = kz) are dealt
// round-robin: wave w takes steps w, w + 8, w + 16, ...  Per step the wave
//   1. has the step's x (nb rows x 32 columns, coalesced float4 units: 8
//      lanes per row) or table rows by id, the norm weights and then the TPW
//      weight fragments in registers, loaded one step AHEAD (the split-K
//      partials-in form adds its partials per 16-row group at the step, not
//      ahead: 5 loads per unit would not fit the registers);
//   2. writes x (+ partials, in order) * nw to its own LDS rows as fp32 (no
//      barrier: one wave writes and reads them) and adds the slice's squares
//      to its per-row statistic;
//   3. per 16-row M tile reads the MFMA A fragment (row lane & 15, columns
//      8 (lane >> 4) .. +7), splits it into three exact bf16 planes in
//      registers and runs v_mfma_f32_16x16x32_bf16 against each weight
//      fragment (B: weight row lane & 15).
// Then, per M tile, the 8 partial tiles of every weight tile are summed in
// wave order through LDS by wave t (tile t), scaled by inv[b] and handed to
// the epilogue.  Every row sees the same K partition and the same order of
// sums whatever its index and whatever the other rows hold, so at fixed nb a
// permutation of the input rows permutes the output rows bit for bit.
// RMSNorm is applied after the dot product, as k_gemvb does; the products are
// exact (3 x bf16 planes), so the result differs from an fp32 GEMV in
// summation order only (the GEMV bar of tests/test_gpu_kernels.py).
//
// x comes from L2 once per workgroup: nb / (8 TPW) bytes per weight byte.
#include <atomic>
#include <string>

#include "qtts_bgemv_dev.h"

namespace {

using namespace qtts_gm;

constexpr int GX_W = QTTS_GX_W, GX_LDX = QTTS_GX_LDX;   // waves per workgroup, staged row stride (qtts_bgemv_dev.h)

// (src -- a.x, a.table or a.table_f32 by SRC --, ids, W and xadd lead the
// arguments: preloaded into SGPRs, Makefile)
template <int MT, int TPW, int SRC>
__global__ __launch_bounds__(64 * GX_W) void k_gemvx(const void *src, const int *ids, const bf16_t *Wt,
                                                      const float *xadd, GemvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int W = GX_W, LDX = GX_LDX, PM = 4;
    constexpr bool AHEAD = SRC != BG_SRC_XADD;   // x of the next step loaded with its weights
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nb = a.nb;
    const int kz = gridDim.y, Ck = a.C / kz, woff = blockIdx.y * Ck;
    const int S = Ck / 32, nit = (S + W - 1) / W;
    const int r0 = blockIdx.x * (16 * TPW);
    const int wreg = max(nb * LDX, TPW * 256);   // floats per wave region (x rows, then the partial tiles)
    float *xs = smem + w * wreg;
    float *ssq = smem + W * wreg;                // [W][64] per-wave row sums of squares
    float *invs = ssq + W * 64;                  // [64]
    int *flag = reinterpret_cast<int *>(invs + 64);
    const bool norm = a.norm_w != nullptr;

    // ---- unit coordinates: unit (m, q) of this lane = row 16 m + 8 q + lane / 8, float4 column lane % 8
    const int ucol = 4 * (lane & 7);
    int urow[MT][2];
    bool uok[MT][2];
    unsigned uid[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int b = 16 * m + 8 * q + (lane >> 3);
            uok[m][q] = b < nb;
            urow[m][q] = b < nb ? b : 0;             // clamped: every load is unconditional
            uid[m][q] = 0;
        }
    if constexpr (SRC == BG_SRC_TAB || SRC == BG_SRC_TABF) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < 2; ++q) uid[m][q] = row_id(a, ids, urow[m][q]);
    }
    const auto rx = rsrc(src);
    const auto rp = rsrc(SRC == BG_SRC_XADD ? (const void *)xadd : src);
    const auto rn = rsrc(norm ? (const void *)a.norm_w : src);
    const auto rw = rsrc(Wt);
    unsigned wo[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        int row = r0 + 16 * t + (lane & 15);
        row = row < a.R ? row : a.R - 1;
        wo[t] = ((unsigned)row * (unsigned)a.C + (unsigned)(woff + 8 * (lane >> 4))) * 2u;
    }

    // ---- the loads of one step (clamped to the column's last: unconditional), in retire order
    float4 xn[MT][2];
    uint2 tn[MT][2];
    float4 nwn = make_float4(1.f, 1.f, 1.f, 1.f);
    v4u wn[TPW];
    auto fetch = [&](int it) {
        int u = it * W + w;
        u = u < S ? u : S - 1;
        const unsigned c0 = (unsigned)(woff + 32 * u + ucol);
        if constexpr (AHEAD) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if constexpr (SRC == BG_SRC_TAB) {
                        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rx, (uid[m][q] * (unsigned)a.C + c0) * 2u, 0, 0);
                        tn[m][q] = make_uint2(v[0], v[1]);
                    } else if constexpr (SRC == BG_SRC_TABF) {
                        xn[m][q] = ld4(rx, uid[m][q] * (unsigned)a.C + c0);
                    } else {
                        xn[m][q] = ld4(rx, (unsigned)urow[m][q] * (unsigned)a.ldx + c0);
                    }
                }
        }
        if (norm) nwn = ld4(rn, c0);
#pragma unroll
        for (int t = 0; t < TPW; ++t)
            wn[t] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rw, wo[t] + 64u * (unsigned)u, 0, 0));
    };

    const bool copier = a.xcopy && blockIdx.x == 0 && blockIdx.y == 0;
    float ss[MT][2];
    floatx4 acc[MT][TPW];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        ss[m][0] = 0.f; ss[m][1] = 0.f;
#pragma unroll
        for (int t = 0; t < TPW; ++t) acc[m][t] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    const int tb = lane & 15, kq = 8 * (lane >> 4);

    fetch(0);
    for (int it = 0; it < nit; ++it) {
        const int u = it * W + w;
        const bool live = u < S;                 // wave-uniform
        const int c0 = woff + 32 * (live ? u : S - 1) + ucol;
        // this step's registers; the next step's loads go out behind them
        float4 xc_[MT][2];
        uint2 tc_[MT][2];
        v4u wc[TPW];
        const float4 nwc = nwn;
#pragma unroll
        for (int t = 0; t < TPW; ++t) wc[t] = wn[t];
        // x (+ partials) -> raw copy, x * nw -> the wave's LDS rows; sums of squares
        auto put = [&](int m, int q, float4 v) {
            const bool ok = uok[m][q];
            float4 *xc = reinterpret_cast<float4 *>(a.xcopy + (size_t)urow[m][q] * a.ldxc + c0);
            if (copier && ok && !a.xcopy_normed) *xc = v;
            ss[m][q] += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
            v.x *= nwc.x; v.y *= nwc.y; v.z *= nwc.z; v.w *= nwc.w;
            if (copier && ok && a.xcopy_normed) *xc = v;   // x * nw; scaled by inv after the barrier
            if (ok) *reinterpret_cast<float4 *>(xs + urow[m][q] * LDX + ucol) = v;
        };
        if constexpr (AHEAD) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) { xc_[m][q] = xn[m][q]; tc_[m][q] = tn[m][q]; }
            if (it + 1 < nit) fetch(it + 1);
            if (!live) continue;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if constexpr (SRC == BG_SRC_TAB) put(m, q, make_float4(lo_f(tc_[m][q].x), hi_f(tc_[m][q].x), lo_f(tc_[m][q].y), hi_f(tc_[m][q].y)));
                    else put(m, q, xc_[m][q]);
                }
        } else {
            // partials-in: x and its PM partials per 16-row group, summed in
            // order (p0 + p1 + ...), added to x as GemvArgs::xadd prescribes and
            // staged group by group; then the next step's weights, which land
            // under this step's MFMAs (x behind them would wait for them)
            if (!live) continue;
            const int np = a.n_xadd;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float4 pv[2][PM];
#pragma unroll
                for (int q = 0; q < 2; ++q) xc_[m][q] = ld4(rx, (unsigned)urow[m][q] * (unsigned)a.ldx + (unsigned)c0);
#pragma unroll
                for (int p = 0; p < PM; ++p) {
                    // (the partial's base is wave-uniform: the load's scalar offset, no register per partial)
                    const int po = (p < np ? p : np - 1) * a.ld_xadd * 4;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const auto t = __builtin_amdgcn_raw_buffer_load_b128(
                            rp, ((unsigned)urow[m][q] * (unsigned)a.ldb_xadd + (unsigned)c0) * 4u, po, 0);
                        pv[q][p] = make_float4(__uint_as_float(t[0]), __uint_as_float(t[1]), __uint_as_float(t[2]), __uint_as_float(t[3]));
                    }
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float4 s = pv[q][0];
#pragma unroll
                    for (int p = 1; p < PM; ++p)
                        if (p < np) { s.x += pv[q][p].x; s.y += pv[q][p].y; s.z += pv[q][p].z; s.w += pv[q][p].w; }
                    float4 v = xc_[m][q];
                    v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w;
                    put(m, q, v);
                }
            }
            if (it + 1 < nit) fetch(it + 1);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // one wave writes and reads its rows: LDS is in order

        // ---- per M tile: A fragment (three exact planes) x each tile's weight fragment
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int ar = 16 * m + tb;
            const float *xf = xs + (ar < nb ? ar : 0) * LDX + kq;   // rows >= nb: row 0 (D rows >= nb are not stored)
            const float4 f0 = *reinterpret_cast<const float4 *>(xf);
            const float4 f1 = *reinterpret_cast<const float4 *>(xf + 4);
            uint2 a1, a2, a3, b1, b2, b3;
            split4(f0, a1, a2, a3);
            split4(f1, b1, b2, b3);
            const bf16x8 h1 = __builtin_bit_cast(bf16x8, v4u{a1.x, a1.y, b1.x, b1.y});
            const bf16x8 h2 = __builtin_bit_cast(bf16x8, v4u{a2.x, a2.y, b2.x, b2.y});
            const bf16x8 h3 = __builtin_bit_cast(bf16x8, v4u{a3.x, a3.y, b3.x, b3.y});
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h1, __builtin_bit_cast(bf16x8, wc[t]), acc[m][t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2, __builtin_bit_cast(bf16x8, wc[t]), acc[m][t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h3, __builtin_bit_cast(bf16x8, wc[t]), acc[m][t], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the fragments are read before the next step's rows land
    }

    // ---- per-row statistic of this wave's steps (the 8 lanes of a row)
    if (norm) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float s = group_sum<8>(ss[m][q]);
                if ((lane & 7) == 0 && uok[m][q]) ssq[w * 64 + urow[m][q]] = s;
            }
    }
    floatx4 *red = reinterpret_cast<floatx4 *>(xs);   // the wave's partial tiles over its own (dead) x rows
#pragma unroll
    for (int t = 0; t < TPW; ++t) red[t * 64 + lane] = acc[0][t];
    __syncthreads();
    if (norm) {
        if (threadIdx.x < 64) {   // row tid: the W slice sums in wave order
            const int lr = (int)threadIdx.x < nb ? (int)threadIdx.x : 0;
            float s2 = 0.f;
#pragma unroll
            for (int k = 0; k < W; ++k) s2 += ssq[k * 64 + lr];
            invs[threadIdx.x] = rms_inv(s2, a.C, a.eps);
        }
        __syncthreads();
        if (copier && a.xcopy_normed) {   // the normalised copy: (x * nw) * inv[b], over this wave's own steps
            for (int it = 0; it < nit; ++it) {
                const int u = it * W + w;
                if (u >= S) break;
                const int c0 = woff + 32 * u + ucol;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        if (!uok[m][q]) continue;
                        const float iv = invs[urow[m][q]];
                        float4 *xc = reinterpret_cast<float4 *>(a.xcopy + (size_t)urow[m][q] * a.ldxc + c0);
                        float4 v = *xc;
                        v.x *= iv; v.y *= iv; v.z *= iv; v.w *= iv;
                        *xc = v;
                    }
            }
        }
    }

    // ---- per M tile: tile t's W partial tiles in wave order (wave t), inv, epilogue
    const bool tile_wave = w < TPW && r0 + 16 * w < a.R;
    const int r = r0 + 16 * w + (lane & 15);   // D: column = lane & 15 (weight row), row = 4 (lane >> 4) + i (batch row)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (m > 0) {
            __syncthreads();   // the previous M tile's partials are summed
#pragma unroll
            for (int t = 0; t < TPW; ++t) red[t * 64 + lane] = acc[m][t];
            __syncthreads();
        }
        if (!tile_wave) continue;
        floatx4 pt[W];
#pragma unroll
        for (int k = 0; k < W; ++k) pt[k] = reinterpret_cast<const floatx4 *>(smem + k * wreg)[w * 64 + lane];
        floatx4 v = pt[0];
#pragma unroll
        for (int k = 1; k < W; ++k) v += pt[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int bb = 16 * m + 4 * (lane >> 4) + i;
            float val = v[i];
            if (norm) val *= invs[bb < nb ? bb : 0];
            // lane + 4 within the 16-lane row (row_shl:4; lanes 12-15 keep their own, unused)
            const float up = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(val), __float_as_int(val), 0x104, 0xF, 0xF, false));
            if (bb >= nb || r >= a.R) continue;
            if (a.tick) st_sc1(a.ypart + blockIdx.y * a.ld_ypart + (size_t)bb * a.R + r, val);
            else if (a.ypart) a.ypart[blockIdx.y * a.ld_ypart + (size_t)bb * a.R + r] = val;
            else epilogue(a, bb, r, val, up);
        }
    }
    // self-reducing split-K producer (every thread reaches the ticket barrier)
    if (a.tick) reduce_last(a, 16 * TPW, flag);
}

std::atomic<long long> g_wide_launches{0};

// (rocprofv3's spelling of the instantiation, built once per instantiation: the
// bench looks its profile rows up by it)
template <int MT, int TP, int SS>
void launch_gx(const BgPlan &p, hipStream_t st, const void *srcp, const int *idsp, const GemvArgs &a) {
    hipLaunchKernelGGL((k_gemvx<MT, TP, SS>), p.grid, p.block, p.smem, st, srcp, idsp, a.W, a.xadd, a);
    static const std::string nm = "k_gemvx<" + std::to_string(MT) + ", " + std::to_string(TP) + ", " + std::to_string(SS) + ">";
    qtts_last_kernel = nm.c_str();
}

}  // namespace

// wide-kernel launches enqueued (or captured) since the library loaded: a
// test's proof that one launch, not one per 16 rows, served a wide batch
extern "C" long long qtts_hip_gemv_wide_launches(void) { return g_wide_launches.load(); }

// the launch of a k_gemvx plan (qtts_bgemv_plan): 0 ok, -1 launch error
int qtts_gemvx_launch(const GemvArgs &a, const BgPlan &p, hipStream_t st) {
    const int MT = p.t[0], TPW = p.t[1], src = p.src;
    const void *srcp = qtts_gm::src_base(a, src);
    const int *idsp = qtts_gm::src_ids(a, src);
#define QTTS_GX(MM, TP, SS) launch_gx<MM, TP, SS>(p, st, srcp, idsp, a);
#define QTTS_GX_SRC(MM, TP)                                        \
    if (src == BG_SRC_X) QTTS_GX(MM, TP, BG_SRC_X)                 \
    else if (src == BG_SRC_XADD) QTTS_GX(MM, TP, BG_SRC_XADD)      \
    else if (src == BG_SRC_TAB) QTTS_GX(MM, TP, BG_SRC_TAB)        \
    else QTTS_GX(MM, TP, BG_SRC_TABF)
#define QTTS_GX_T(MM)                                              \
    if (TPW == 1) { QTTS_GX_SRC(MM, 1) }                           \
    else if (TPW == 2) { QTTS_GX_SRC(MM, 2) }                      \
    else { QTTS_GX_SRC(MM, 3) }
    switch (MT) {
        case 2: QTTS_GX_T(2) break;
        case 3: QTTS_GX_T(3) break;
        default: QTTS_GX_T(4) break;
    }
#undef QTTS_GX_T
#undef QTTS_GX_SRC
#undef QTTS_GX
    if (hipGetLastError() != hipSuccess) return -1;
    g_wide_launches.fetch_add(1);
    return 0;
}
