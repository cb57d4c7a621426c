// k_xlinh.hip - the codec's linears on ONE bf16 plane per operand (the opt-in
// bf16 linear precision; k_codec.hip's k_xlin / k_xgemv / k_xgemm keep the
// fp32-equivalent products).
//
//   C(m, n) = epi( sum_k A(m, k) * W[n][k] ),  bmode XB_WT, amode XA_ROWS / XA_TRANS
//
//   operands  A: loaded fp32 (rows: two 16-B loads per 8 k; trans: 8 strided
//             scalars, lanes along m; stacked rows through xg_srow), rounded to
//             bf16 nearest even (cb_pk).  W: the weight's bf16 twin (XGemm::Bh,
//             compact [N][K], the weight rounded to nearest even = plane 1 of
//             k_wt_split), 16-B loads.  Sums fp32, epilogue xg_epi.
//   order     K is cut into stages of 64 k = four 16-deep steps of
//             v_mfma_f32_32x32x16_bf16 (a last stage of 32 k: two steps;
//             K % 32 == 0).  Stage s belongs to phase s % 8.  A phase's sum S_j
//             is one accumulator chain over its stages, steps in increasing k.
//             The element is ((((0 + S_0) + S_1) + ...) + S_7), fp32 adds in
//             that order (an empty phase adds its 0).  This is a function of K
//             alone.  An element reads row m of A and row n of W only, and an
//             MFMA's output element is the dot product of its own row and
//             column, so its bits are a function of (those rows, K): the same
//             whatever M, the grid, and which of the two kernels below ran.
//   k_xlinh   the tile kernel: 64 x 64 of C per workgroup of 2 x 2 waves, a
//             wave one 32 x 32 block on eight phase accumulators (128 registers),
//             summed in registers.  Stages through LDS: rows of 64 k (128 B) =
//             eight 16-B chunks, chunk q of row r at chunk q ^ ((r >> 1) & 7),
//             so the 16 lanes of a ds_read_b128 pass (16 consecutive rows, one
//             chunk) and of a ds_write_b128 pass (two rows x eight chunks, or
//             16 rows x one chunk) hit 16 distinct 16-B slots of a 256-B bank
//             line; 8 KB + 8 KB.  The next stage's loads stay in registers
//             across the MFMAs (fp32 A items of 8 k, converted only when
//             stored, and 16-B twin items).
//   k_xlinh_p the phase kernel, for grids the tile kernel would leave under
//             256 workgroups (small M: the weight stream of a 1-frame push):
//             one wave per (32 x 32 block, phase), grid (N / 32, M / 32, 8) --
//             256 workgroups at N 1024 and 1 to 32 rows, each streaming its
//             eighth of the block's twin rows.  No LDS and no barrier: a lane
//             loads its own MFMA fragments (row lane & 31, 8 k at 8 * (lane >>
//             5) of each step) straight into registers, the next stage of its
//             phase in flight across the MFMAs.  S_j goes to the split
//             workspace; k_xg_reduce adds the eight in order from 0 and runs
//             the epilogue.
#include "qtts_xgemm_dev.h"

namespace {

constexpr int XH_KS = 64;   // k per stage
constexpr int XH_P = 8;     // phases

// 16-B chunk q (8 k) of row `row` in a [rows][64] bf16 tile, in elements
__device__ __forceinline__ int xh_swz(int row, int q) { return row * XH_KS + 8 * (q ^ ((row >> 1) & 7)); }

__global__ __launch_bounds__(256, 2) void k_xlinh(XGemm g) {
    constexpr int NT = 256, BM = 64, BN = 64;
    constexpr int NAT = BM * 8 / NT, NBT = BN * 8 / NT;      // (row, chunk) items per thread and stage
    __shared__ __attribute__((aligned(16))) unsigned short As[BM * XH_KS];
    __shared__ __attribute__((aligned(16))) unsigned short Ws[BN * XH_KS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int K = g.K;
    const bool tr = g.amode == XA_TRANS;
    // an item's row and chunk do not change with the stage: its first element and where it goes in LDS.
    // rows: chunk fastest (a row's 256 B contiguous); trans: row fastest (the lanes along m are contiguous)
    const float *pa[NAT];
    const unsigned short *pw[NBT];
    int sa[NAT], sw[NBT], qa[NAT], qw[NBT];
    const size_t kst = tr ? (size_t)g.lda : 1;               // elements between consecutive k of A
#pragma unroll
    for (int j = 0; j < NAT; ++j) {
        const int e = tid + NT * j, row = tr ? e % BM : e >> 3, q = tr ? e / BM : e & 7, m = m0 + row;
        qa[j] = q;
        sa[j] = xh_swz(row, q);
        pa[j] = m < g.M ? (tr ? g.A + xg_srow(g, m, g.seg_lda) : g.A + (size_t)m * g.lda) + 8 * q * kst : nullptr;
    }
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
        const int e = tid + NT * j, row = e >> 3, q = e & 7, n = n0 + row;
        qw[j] = q;
        sw[j] = xh_swz(row, q);
        pw[j] = n < g.N ? g.Bh + (size_t)n * K + 8 * q : nullptr;
    }
    float ra[NAT][8];
    uint4 rb[NBT];
    // items of rows past M / N and chunks at or past K (the 32-deep last stage) load zeros
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NAT; ++j) {
            const bool ok = pa[j] && k0 + 8 * qa[j] < K;
            if (!ok) {
#pragma unroll
                for (int i = 0; i < 8; ++i) ra[j][i] = 0.f;
            } else if (tr) {
                const float *p = pa[j] + (size_t)k0 * kst;
#pragma unroll
                for (int i = 0; i < 8; ++i) ra[j][i] = p[i * kst];
            } else {
                const float4 *p = reinterpret_cast<const float4 *>(pa[j] + k0);
                const float4 u = p[0], v = p[1];
                ra[j][0] = u.x; ra[j][1] = u.y; ra[j][2] = u.z; ra[j][3] = u.w;
                ra[j][4] = v.x; ra[j][5] = v.y; ra[j][6] = v.z; ra[j][7] = v.w;
            }
        }
#pragma unroll
        for (int j = 0; j < NBT; ++j) {
            const bool ok = pw[j] && k0 + 8 * qw[j] < K;
            rb[j] = ok ? *reinterpret_cast<const uint4 *>(pw[j] + k0) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    floatx16 acc[XH_P];
#pragma unroll
    for (int p = 0; p < XH_P; ++p)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[p][i] = 0.f;
    load(0);
    const int r = lane & 31, hh = lane >> 5;
    for (int kb = 0; kb < K; kb += XH_P * XH_KS) {
#pragma unroll
        for (int p = 0; p < XH_P; ++p) {                     // stage kb / 64 + p: phase p
            const int k0 = kb + p * XH_KS;
            if (k0 < K) {                                    // (uniform)
#pragma unroll
                for (int j = 0; j < NAT; ++j)
                    *reinterpret_cast<uint4 *>(&As[sa[j]]) =
                        make_uint4(cb_pk(ra[j][0], ra[j][1]), cb_pk(ra[j][2], ra[j][3]), cb_pk(ra[j][4], ra[j][5]),
                                   cb_pk(ra[j][6], ra[j][7]));
#pragma unroll
                for (int j = 0; j < NBT; ++j) *reinterpret_cast<uint4 *>(&Ws[sw[j]]) = rb[j];
                __syncthreads();
                const bool whole = K - k0 >= XH_KS;          // else 32 k: steps 0 and 1
                if (k0 + XH_KS < K) load(k0 + XH_KS);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    if (ks < 2 || whole) {
                        const int q = 2 * ks + hh;
                        const bf16x8 a = *reinterpret_cast<const bf16x8 *>(&As[xh_swz(wm + r, q)]);
                        const bf16x8 w = *reinterpret_cast<const bf16x8 *>(&Ws[xh_swz(wn + r, q)]);
                        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, w, acc[p], 0, 0, 0);
                    }
                }
                __syncthreads();
            }
        }
    }
    const int n = n0 + wn + (lane & 31);
    if (n >= g.N) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        float v = 0.f;                                       // k_xg_reduce's sum, term for term
#pragma unroll
        for (int p = 0; p < XH_P; ++p) v += acc[p][i];
        if (m < g.M) xg_epi(g, m, n, v);
    }
}

// one wave: block (blockIdx.x, blockIdx.y), phase blockIdx.z; S_phase -> g.part[phase][M][N]
__global__ __launch_bounds__(64) void k_xlinh_p(XGemm g) {
    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const int m = blockIdx.y * 32 + r, n = blockIdx.x * 32 + r, ph = blockIdx.z;
    const int K = g.K;
    const bool tr = g.amode == XA_TRANS, am = m < g.M, wn = n < g.N;
    const size_t kst = tr ? (size_t)g.lda : 1;
    // the lane's fragment of step ks of the stage at k0: 8 k from k0 + 16 ks + 8 hh
    const float *pa = am ? (tr ? g.A + xg_srow(g, m, g.seg_lda) : g.A + (size_t)m * g.lda) + 8 * hh * kst : nullptr;
    const unsigned short *pw = wn ? g.Bh + (size_t)n * K + 8 * hh : nullptr;
    float ra[4][8];
    uint4 rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = k0 + 16 * ks;                      // (8 hh inside pa / pw; K % 32 == 0: a step is whole or absent)
            const bool in = k < K;
            if (!(am && in)) {
#pragma unroll
                for (int i = 0; i < 8; ++i) ra[ks][i] = 0.f;
            } else if (tr) {
                const float *p = pa + (size_t)k * kst;
#pragma unroll
                for (int i = 0; i < 8; ++i) ra[ks][i] = p[i * kst];
            } else {
                const float4 *p = reinterpret_cast<const float4 *>(pa + k);
                const float4 u = p[0], v = p[1];
                ra[ks][0] = u.x; ra[ks][1] = u.y; ra[ks][2] = u.z; ra[ks][3] = u.w;
                ra[ks][4] = v.x; ra[ks][5] = v.y; ra[ks][6] = v.z; ra[ks][7] = v.w;
            }
            rb[ks] = wn && in ? *reinterpret_cast<const uint4 *>(pw + k) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    constexpr int STEP = XH_P * XH_KS;
    if (ph * XH_KS < K) load(ph * XH_KS);
    for (int k0 = ph * XH_KS; k0 < K; k0 += STEP) {
        bf16x8 a[4], w[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const uint4 v = make_uint4(cb_pk(ra[ks][0], ra[ks][1]), cb_pk(ra[ks][2], ra[ks][3]),
                                       cb_pk(ra[ks][4], ra[ks][5]), cb_pk(ra[ks][6], ra[ks][7]));
            a[ks] = __builtin_bit_cast(bf16x8, v);
            w[ks] = __builtin_bit_cast(bf16x8, rb[ks]);
        }
        const bool whole = K - k0 >= XH_KS;
        if (k0 + STEP < K) load(k0 + STEP);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            if (ks < 2 || whole) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks], w[ks], acc, 0, 0, 0);
    }
    float *pz = g.part + (size_t)ph * g.M * g.N;
    const int nn = blockIdx.x * 32 + (lane & 31);
    if (nn >= g.N) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int mm = blockIdx.y * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        if (mm < g.M) pz[(size_t)mm * g.N + nn] = acc[i];
    }
}

// w [N] rows of ldb floats -> compact bf16 [N][K], nearest even (K even)
__global__ void k_wt_half(const float *w, int ldb, int N, int K, uint32_t *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)(K / 2);
    if (i >= per * N) return;
    const size_t n = i / per, k = 2 * (i - n * per);
    out[i] = cb_pk(w[n * ldb + k], w[n * ldb + k + 1]);
}

}  // namespace

void qtts_xlinh_twin(const float *w, int ldb, int N, int K, unsigned short *out, hipStream_t st) {
    const size_t n = (size_t)N * (K / 2);
    hipLaunchKernelGGL(k_wt_half, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, ldb, N, K,
                       reinterpret_cast<uint32_t *>(out));
}

// the partials the caller's k_xg_reduce has to sum: XH_P after the phase kernel, 1 (nothing to sum) after the tile kernel
int qtts_xlinh_launch(const XGemm &g, hipStream_t st) {
    // the tile kernel where its grid gives every CU a workgroup, or the workspace
    // cannot hold the phases' partials; else one wave per (32 x 32 block, phase)
    const int wide = ((g.N + 63) / 64) * ((g.M + 63) / 64);
    if (wide >= 256 || !g.part || (size_t)XH_P * g.M * g.N > g.part_elems) {
        hipLaunchKernelGGL(k_xlinh, dim3((g.N + 63) / 64, (g.M + 63) / 64), dim3(256), 0, st, g);
        return 1;
    }
    hipLaunchKernelGGL(k_xlinh_p, dim3((g.N + 31) / 32, (g.M + 31) / 32, XH_P), dim3(64), 0, st, g);
    return XH_P;
}
