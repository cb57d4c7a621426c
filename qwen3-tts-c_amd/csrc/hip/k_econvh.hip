// k_econvh.hip - the voice-clone encoders' contraction on ONE bf16 plane per
// operand (the opt-in bf16 encoder precision; k_enc.hip's k_econv keeps the
// fp32-equivalent products with three planes and six MFMAs per product block).
//
// Same contraction, descriptor, tile, grid, split-K ranges and epilogue as
// k_econv<ROWS>:  out[b][m][n] = epi( sum_k W[m][k] * x'[b][k][n] ), a 64 (out
// channels) x 64 (time) tile per workgroup of 2 x 2 waves, blockIdx.z = b * kz
// + split, split z owns the 32-wide K-steps [nk z / kz, nk (z + 1) / kz) of
// launch_econv's plan, raw partials to g.part for k_econv_reduce when kz > 1,
// else econv_store.  What differs:
//
//   operands  weights: plane 0 of the [3][M][Kp] split.  k_ewsplit makes it
//             with e_pk, a float -> __bf16 conversion: round to nearest even,
//             not truncation, so plane 0 is the weight rounded to bf16 and each
//             operand carries at most 2^-9 relative error.  Read where k_econv
//             reads it: no new weight memory.  Inputs: loaded fp32, the padding
//             remap, the Res2Net sum and the ELU prologue in fp32, rounded to
//             bf16 (nearest even, e_pk) as the stage is written to LDS.
//             Accumulators, partials and the epilogue fp32.
//   products  one v_mfma_f32_32x32x16_bf16 per 16-deep product block.
//   stage     64 k (four MFMA steps) per barrier.  A split's range is a
//             multiple of 32, not of 64: the last stage of a range may hold 32
//             k, and its upper half is neither loaded (the weight row ends at
//             Kp) nor multiplied.
//   LDS       one plane leaves room for rows of 64 k (128 B = eight 16-B
//             chunks) and for two stages: the next stage is written into the
//             other buffer while this one is multiplied, so a stage costs one
//             barrier (k_econv: two per 32 k).  2 x (8 KB + 8 KB) = 32 KB.
//             Chunk q of row r lives at chunk q ^ ((r >> 1) & 7): two rows
//             share a 256-B bank line, so the 16 lanes of a ds_read_b128 pass
//             (16 consecutive rows, one chunk), of the weights' ds_write_b128
//             pass (two rows x eight chunks) and of the inputs' (16 rows x one
//             chunk) hit 16 distinct 16-B slots of the line.
//   registers the stage after next's loads stay in registers across the MFMAs:
//             two 16-B weight items and two fp32 input items of 8 k per
//             thread, converted only when stored.
//   order     an output's sum is one accumulator chain over its split's k in
//             increasing order, then k_econv_reduce's sum over the splits in
//             split order.  It reads row m of W and column (b, n) of x' only,
//             and the split depends on the shape and the padded length, never
//             on the batch: an utterance's result is bit-identical alone and
//             in a batch of equal padding.
#include <atomic>

#include "qtts_econv_dev.h"

namespace {

constexpr int EH_KS = 64;   // k per stage

// 16-B chunk q (8 k) of row `row` in a [64][64] bf16 tile, in elements
__device__ __forceinline__ int eh_swz(int row, int q) { return row * EH_KS + 8 * (q ^ ((row >> 1) & 7)); }

// ROWS: the input is time-major rows with k contiguous (kw = 1, xc = 1,
// stride 1, no padding, no prologue): an item's 8 k values are two float4 loads.
template <bool ROWS>
__global__ __launch_bounds__(256) void k_econvh(EConv g) {
    __shared__ __attribute__((aligned(16))) unsigned short As[2][64 * EH_KS];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[2][64 * EH_KS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kz = g.kz, b = blockIdx.z / kz, kzi = blockIdx.z - b * kz;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int lout = g.lout[b], lin = g.lin[b];
    if (n0 >= lout) return;   // uniform per workgroup, before any barrier
    const float *x = g.x + (size_t)b * g.xb;
    const float *x2 = g.x2 ? g.x2 + (size_t)b * g.xb : nullptr;
    // this split's k range, in k_econv's 32-wide steps
    const int nk = g.Kp / 32, kb = nk * kzi / kz * 32, ke = nk * (kzi + 1) / kz * 32;
    // weight items: rows ar and ar + 32, 16-B chunk ac of the 128-B stage row
    const int ar = tid >> 3, ac = tid & 7;
    const unsigned short *wa[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
        wa[j] = m0 + ar + 32 * j < g.M ? g.w + (size_t)(m0 + ar + 32 * j) * g.Kp + 8 * ac : nullptr;
    // input items: column bn, chunks bq and bq + 4
    const int bn = tid & 63, bq = tid >> 6;
    const bool bcol = n0 + bn < lout;
    const int tcol = (n0 + bn) * g.stride - g.padl;
    uint4 ra[2];
    float rb[2][8];
    // rows past M, columns past lout and chunks at or past ke (or K) load zeros
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            ra[j] = wa[j] && k0 + 8 * ac < ke ? *reinterpret_cast<const uint4 *>(wa[j] + k0) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + 8 * (bq + 4 * j);
            const bool in = bcol && k < ke && k < g.K;
            if (ROWS) {
                if (in) {
                    const float4 *src = reinterpret_cast<const float4 *>(x + (size_t)(n0 + bn) * g.xt + k);
                    const float4 u = src[0], v = src[1];
                    rb[j][0] = u.x; rb[j][1] = u.y; rb[j][2] = u.z; rb[j][3] = u.w;
                    rb[j][4] = v.x; rb[j][5] = v.y; rb[j][6] = v.z; rb[j][7] = v.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) rb[j][i] = 0.f;
                }
                continue;
            }
            int ci = k / g.kw, tap = k - ci * g.kw;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float v = 0.f;
                if (in && k + i < g.K) {
                    int t = tcol + tap * g.dil;
                    bool ok = true;
                    if (t < 0 || t >= lin) {
                        if (g.pmode == PAD_REFLECT) t = t < 0 ? -t : 2 * (lin - 1) - t;
                        else if (g.pmode == PAD_REPLICATE) t = t < 0 ? 0 : lin - 1;
                        else ok = false;
                    }
                    if (ok) {
                        const size_t o = (size_t)ci * g.xc + (size_t)t * g.xt;
                        v = x[o];
                        if (x2) v += x2[o];
                        if (g.act_in == 1) v = v > 0.f ? v : expm1f(v);   // ELU (alpha 1), before the padding
                    }
                }
                rb[j][i] = v;
                if (++tap == g.kw) { tap = 0; ++ci; }
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<uint4 *>(&As[buf][eh_swz(ar + 32 * j, ac)]) = ra[j];
            *reinterpret_cast<uint4 *>(&Bs[buf][eh_swz(bn, bq + 4 * j)]) =
                make_uint4(e_pk(rb[j][0], rb[j][1]), e_pk(rb[j][2], rb[j][3]), e_pk(rb[j][4], rb[j][5]),
                           e_pk(rb[j][6], rb[j][7]));
        }
    };
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, r = lane & 31, hh = lane >> 5;
    load(kb);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += EH_KS, buf ^= 1) {
        const bool more = k0 + EH_KS < ke, whole = ke - k0 >= EH_KS;   // (uniform)
        if (more) load(k0 + EH_KS);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks < 2 || whole) {
                const int q = 2 * ks + hh;
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(&As[buf][eh_swz(wm + r, q)]);
                const bf16x8 w = *reinterpret_cast<const bf16x8 *>(&Bs[buf][eh_swz(wn + r, q)]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, w, acc, 0, 0, 0);
            }
        }
        if (more) store(buf ^ 1);   // (the buffer every wave left at the last barrier)
        __syncthreads();
    }
    const int n = n0 + wn + r;
    if (n >= lout) return;
    if (kz > 1) {
        float *pz = g.part + ((size_t)kzi * g.nb + b) * g.M * g.pn;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * hh;
            if (m < g.M) pz[(size_t)m * g.pn + n] = acc[i];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * hh;
        if (m < g.M) econv_store(g, b, m, n, acc[i]);
    }
}

std::atomic<long long> g_econvh_launches{0};

}  // namespace

void qtts_econvh_launch(const EConv &g, bool rows, dim3 grid, hipStream_t st) {
    if (rows) hipLaunchKernelGGL((k_econvh<true>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((k_econvh<false>), grid, dim3(256), 0, st, g);
    ++g_econvh_launches;
}

long long qtts_econvh_launches() { return g_econvh_launches.load(); }
