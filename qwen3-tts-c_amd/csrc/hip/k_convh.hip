// k_convh.hip - the codec's causal convs on ONE bf16 plane per operand (the
// opt-in bf16 codec precision; k_codec.hip's k_convb keeps fp32-equivalent
// products with three planes and six MFMAs per product block).
//
// Same contraction, tiles, grid, splits and epilogues as k_convb<KW, WN>:
//   out[co][t] = epi( sum_tap sum_ci Wt[tap][co][ci] * x'[ci][t + tap*dil - pad] ),
// x' = SnakeBeta(x) where g.sa is set, a 64 (co) x 64*WN (t) tile per
// workgroup of 2 x WN waves, each wave 32 x 64 on two fp32 accumulators of
// v_mfma_f32_32x32x16_bf16.  What differs:
//
//   operands  weights: plane 1 of the relayout's three planes (wt_planes) is
//             the weight rounded to nearest even -- read where k_convb reads
//             it, no new weight memory.  Inputs: loaded fp32, SnakeBeta in
//             fp32, rounded to bf16 (nearest even, cb_pk) as the stage is
//             written to LDS.  Accumulation, partials and epilogues fp32.
//   stage     CH_BC = 32 input channels (two 16-deep MFMA steps) per barrier
//             pair: one MFMA per product block leaves 14 per wave in a
//             16-channel stage at KW 7, too few to cover two barriers; 32
//             channels make 28 and halve the barriers per channel.  The last
//             stage of a split may hold 16 channels (a split's channels are a
//             multiple of 16, not of 32): its upper half is neither loaded
//             nor multiplied.
//   LDS       rows of 32 channels (64 B) = four 16-B chunks; chunk q of row r
//             lives at chunk q ^ ((r >> 2) & 3), so the 16 lanes of a
//             ds_read_b128 pass (16 consecutive rows, one chunk) hit 16
//             distinct 16-B slots of a 256-B bank line, for the weights'
//             fixed rows and for the window's rows at any tap shift alike.
//             KW 7 / WN 4: 28,672 B weights + 20,480 B window = 49,152 B.
//   registers the next stage's loads stay in registers across the MFMAs (the
//             double buffer of k_convb): 16-B bf16 weight items and fp32
//             window items of 8 channels, converted only when stored.
#include "qtts_xgemm_dev.h"

namespace {

constexpr int CH_BC = 32;   // input channels per stage

// 16-B chunk q (8 channels) of row `row` in a [rows][32] bf16 tile, in elements
__device__ __forceinline__ int ch_swz(int row, int q) { return row * CH_BC + 8 * (q ^ ((row >> 2) & 3)); }

// waves per SIMD the register budget is held to: 4 (128 registers; two 8-wave
// or four 4-wave workgroups per CU), except KW 7 / WN 2, whose 28 weight and
// 24 window registers of the next stage beside 32 accumulators spilled 23
// VGPRs at 128: 3 there (168 registers, three workgroups per CU)
constexpr int ch_minw(int kw, int wn) { return kw == 7 && wn == 2 ? 3 : 4; }

// blockIdx.z = phase * kz + split, as k_conv / k_convb
template <int KW, int WN>
__global__ __launch_bounds__(128 * WN, ch_minw(KW, WN)) void k_convh(XGemm g) {
    constexpr int NT = 128 * WN, BNT = 64 * WN;
    const int nzk = g.kz > 1 ? g.kz : 1, ph = blockIdx.z / nzk, kzi = blockIdx.z - ph * nzk;
    const int nph = gridDim.z / nzk, ci = g.K / KW;
    // plane 1 follows the fp32 relayout of all phases; this phase's [KW][M][ci]
    const unsigned short *wb = reinterpret_cast<const unsigned short *>(g.wt + (size_t)nph * g.M * g.K) +
                               (size_t)ph * KW * g.M * ci;
    g.phase += ph;
    constexpr int NBW = BNT + CV_HALO;                       // staged window columns
    constexpr int NA = KW * CV_BM * 4;                       // 16-B weight items per stage
    constexpr int NAT = (NA + NT - 1) / NT;
    constexpr int NB = 4 * NBW;                              // (chunk, column) window items per stage
    constexpr int NBT = (NB + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) unsigned short As[KW * CV_BM * CH_BC];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[NBW * CH_BC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.y * CV_BM, n0 = xg_seg_tile(g) * BNT;
    const int wm = (wave / WN) * 32, wn = (wave % WN) * 64;
    const int dil = g.dil, t0 = n0 - g.pad;
    const int cpz = ci / nzk, cbeg = kzi * cpz, cend = cbeg + cpz;   // this split's input channels
    const int win = BNT + (KW - 1) * dil;                    // columns actually needed
    floatx16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    uint4 ra[NAT];
    float rb[NBT][8];
    // chunks of 8 channels at or past cend (the 16-channel last stage) load zeros
    auto load = [&](int c0) {
#pragma unroll
        for (int j = 0; j < NAT; ++j) {
            const int e = tid + NT * j;                      // item in [KW][BM][4]
            const int q = e & 3, m = (e >> 2) % CV_BM, tap = e / (4 * CV_BM);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (e < NA && m0 + m < g.M && c0 + 8 * q < cend)
                v = *reinterpret_cast<const uint4 *>(wb + ((size_t)tap * g.M + m0 + m) * ci + c0 + 8 * q);
            ra[j] = v;
        }
#pragma unroll
        for (int j = 0; j < NBT; ++j) {
            const int e = tid + NT * j, q = e / NBW, x = e - q * NBW, t = t0 + x;
            const bool ok = q < 4 && c0 + 8 * q < cend && x < win && t >= g.tmin && t < g.L;
#pragma unroll
            for (int i = 0; i < 8; ++i) rb[j][i] = ok ? g.B[(size_t)(c0 + 8 * q + i) * g.ldb + t] : 0.f;
        }
    };
    load(cbeg);
    // SnakeBeta's parameters come through the scalar cache: an item's 8
    // channels are wave-uniform (NBW is a multiple of 64)
    static_assert(NBW % 64 == 0, "k_convh: staged window columns must be whole waves");
    const bool snake = g.sa != nullptr;
    const int r = lane & 31, hh = lane >> 5;
    for (int c0 = cbeg; c0 < cend; c0 += CH_BC) {
#pragma unroll
        for (int j = 0; j < NAT; ++j) {
            const int e = tid + NT * j;
            if (e < NA) *reinterpret_cast<uint4 *>(&As[ch_swz(e >> 2, e & 3)]) = ra[j];   // row = tap * 64 + m
        }
#pragma unroll
        for (int j = 0; j < NBT; ++j) {
            const int e = tid + NT * j, q = e / NBW, x = e - q * NBW;
            if (q < 4) {
                const int cu = __builtin_amdgcn_readfirstlane(c0 + 8 * q);
                if (snake && cu < cend) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) rb[j][i] = snake1(rb[j][i], g.sa[cu + i], g.sb[cu + i]);
                }
                *reinterpret_cast<uint4 *>(&Bs[ch_swz(x, q)]) =
                    make_uint4(cb_pk(rb[j][0], rb[j][1]), cb_pk(rb[j][2], rb[j][3]), cb_pk(rb[j][4], rb[j][5]),
                               cb_pk(rb[j][6], rb[j][7]));
            }
        }
        __syncthreads();
        const int nks = cend - c0 > CV_BC ? 2 : 1;           // 16-deep steps this stage holds
        if (c0 + CH_BC < cend) load(c0 + CH_BC);
#pragma unroll
        for (int tap = 0; tap < KW; ++tap) {
            const int sh = tap * dil, arow = tap * CV_BM + wm + r;
            const int b0 = wn + r + sh, b1 = b0 + 32;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks < nks) {
                    const int q = 2 * ks + hh;
                    const bf16x8 a = *reinterpret_cast<const bf16x8 *>(&As[ch_swz(arow, q)]);
                    const bf16x8 x0 = *reinterpret_cast<const bf16x8 *>(&Bs[ch_swz(b0, q)]);
                    const bf16x8 x1 = *reinterpret_cast<const bf16x8 *>(&Bs[ch_swz(b1, q)]);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, x0, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, x1, acc1, 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    float *pz = nzk > 1 ? g.part + (size_t)blockIdx.z * g.M * g.N : nullptr;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        const int n = n0 + wn + (lane & 31);
        if (m >= g.M) continue;
        if (pz) {
            if (n < g.N) pz[(size_t)m * g.N + n] = acc0[i];
            if (n + 32 < g.N) pz[(size_t)m * g.N + n + 32] = acc1[i];
            continue;
        }
        if (n < g.N) xg_epi(g, m, n, acc0[i]);
        if (n + 32 < g.N) xg_epi(g, m, n + 32, acc1[i]);
    }
}

template <int WN>
void convh_launch_wn(const XGemm &g, dim3 grid, hipStream_t st) {
    switch (g.Kw) {
        case 7: hipLaunchKernelGGL((k_convh<7, WN>), grid, dim3(128 * WN), 0, st, g); break;
        case 3: hipLaunchKernelGGL((k_convh<3, WN>), grid, dim3(128 * WN), 0, st, g); break;
        case 2: hipLaunchKernelGGL((k_convh<2, WN>), grid, dim3(128 * WN), 0, st, g); break;
        default: hipLaunchKernelGGL((k_convh<1, WN>), grid, dim3(128 * WN), 0, st, g); break;
    }
}

}  // namespace

void qtts_convh_launch(const XGemm &g, int wn, dim3 grid, hipStream_t st) {
    if (wn == 4) convh_launch_wn<4>(g, grid, st);
    else convh_launch_wn<2>(g, grid, st);
}
