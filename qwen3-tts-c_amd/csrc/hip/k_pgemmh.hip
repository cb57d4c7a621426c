// k_pgemmh.hip - the talker prefill's projections over many prompt rows on ONE
// bf16 plane per operand (the opt-in bf16 prefill precision; k_pgemm.hip keeps
// the fp32-equivalent products on three planes).
//
//   y[m][n] = epi( sum_k bf16(xn[m][k]) W[n][k] ),  xn = x, or x * inv * norm_w
//
//   operands  k_round1: one pass over x (+ RMSNorm, the row's statistic formed
//             in the same launch by k_split3's / k_row_rms's expression),
//             x * inv * w in fp32, rounded to bf16 nearest even -> ONE plane
//             [Mp][K] (Mp: rows rounded up to the 128-row tile, pad rows zero):
//             2 bytes per activation element where k_split3 writes 6, in the
//             first third of the same scratch.  W: the talker's bf16 rows as
//             they are (no twin).  bf16 x bf16 products are exact in fp32;
//             sums fp32.
//   k_pgemmh  a 128 x 64 WN tile per workgroup of 2 x WN waves (WN 2: 128 x 128,
//             256 threads; WN 4: 128 x 256, 512 threads), a wave 64 x 64 = 2 x 2
//             v_mfma_f32_32x32x16_bf16 tiles.  K in stages of 64 = four 16-deep
//             steps: 16 MFMAs per wave between barriers (a 32-deep stage of one
//             plane would hold 8).  Both operands through LDS in rows of 128 B =
//             eight 16-B chunks, chunk q of row r at q ^ ((r >> 1) & 7): the 16
//             lanes of a ds_read_b128 pass (16 consecutive rows, one chunk) and
//             of a ds_write_b128 pass (two rows x eight chunks) hit 16 distinct
//             16-B slots of a 256-B bank line.  Two buffers: A 16 KB + W 16 / 32
//             KB each.  A thread owns the same (row, chunk) items in every
//             stage; the loads of stage s + 2 are issued before stage s's MFMAs
//             into the register set stage s came in (two sets), stage s + 1 goes
//             from the other set to the idle buffer behind the MFMAs, one
//             barrier per stage.  No branch around a load or an LDS store: the
//             stage index is clamped instead, the tail re-loads the last stage.
//   order     an element is one accumulator chain over its column's stages,
//             steps in increasing k; split-K columns over grid.z are summed in
//             column order with the epilogue by k_mgemm_reduce: a function of
//             (K, kz) alone.
// Epilogues: store / residual add / SwiGLU over the interleaved gate|up row
// quads (the up row n + 4 is lane + 4 of the same 32-wide tile).
#include <atomic>
#include <type_traits>

#include "qtts_common.h"
#include "qtts_kernels.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {

__device__ __forceinline__ uint32_t ph_pk(float lo, float hi) {   // two floats -> bf16 pair, nearest even
    uint32_t a = __float_as_uint(lo), b = __float_as_uint(hi);
    a = (a + 0x7FFFu + ((a >> 16) & 1u)) >> 16;
    b = (b + 0x7FFFu + ((b >> 16) & 1u)) & 0xFFFF0000u;
    return a | b;
}

// x rows (+ RMSNorm, K.c:27-39) -> one bf16 plane; one 256-thread workgroup per
// row (grid Mp), 8 consecutive k per thread and pass.  Rows >= M are zeros.
__global__ __launch_bounds__(256) void k_round1(const float *x, int ldx, int M, int K, const float *norm_w, float eps,
                                                unsigned short *plane) {
    __shared__ float red[4];
    const int t = blockIdx.x, tid = threadIdx.x;
    v4u *out = reinterpret_cast<v4u *>(plane + (size_t)t * K);
    if (t >= M) {   // (uniform)
        v4u z;
        z.x = z.y = z.z = z.w = 0u;
        for (int k = tid; k < K / 8; k += 256) out[k] = z;
        return;
    }
    const float *xr = x + (size_t)t * ldx;
    float iv = 1.f;
    if (norm_w) {
        float ss = 0.f;
        for (int c = tid; c < K; c += 256) ss += xr[c] * xr[c];
        iv = rms_inv(block_sum256(ss, red), K, eps);
    }
    for (int k = tid * 8; k < K; k += 256 * 8) {
        const float4 a = *reinterpret_cast<const float4 *>(xr + k);
        const float4 b = *reinterpret_cast<const float4 *>(xr + k + 4);
        float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (norm_w) {
            const float4 n0 = *reinterpret_cast<const float4 *>(norm_w + k);
            const float4 n1 = *reinterpret_cast<const float4 *>(norm_w + k + 4);
            const float nw[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] * iv * nw[j];
        }
        v4u q;
        q.x = ph_pk(v[0], v[1]);
        q.y = ph_pk(v[2], v[3]);
        q.z = ph_pk(v[4], v[5]);
        q.w = ph_pk(v[6], v[7]);
        out[k / 8] = q;
    }
}

constexpr int HM = 128, HK = 64, HQ = HK / 8;   // row tile, k per stage, 16-B chunks per LDS row

// 16-B chunk index of (row, chunk q) in a [rows][8 chunks] tile
__device__ __forceinline__ int hswz(int row, int q) { return row * HQ + (q ^ ((row >> 1) & 7)); }

template <int WN>
__global__ __launch_bounds__(128 * WN) void k_pgemmh(GemvArgs a, const unsigned short *plane, float *part) {
    constexpr int NT = 128 * WN, BN = 64 * WN;
    constexpr int A_PT = HM * HQ / NT, W_PT = BN * HQ / NT;   // (row, chunk) items per thread and stage
    static_assert(HM * HQ % NT == 0 && BN * HQ % NT == 0, "k_pgemmh: stage chunks per thread");
    __shared__ __attribute__((aligned(16))) v4u As[2][HM * HQ];
    __shared__ __attribute__((aligned(16))) v4u Ws[2][BN * HQ];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w & 1, wn = w >> 1;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * HM;
    const int K = a.C, N = a.R, M = a.nb;
    const int nst = K / HK / gridDim.z;
    const size_t k0 = (size_t)blockIdx.z * nst * HK;

    // a thread's items: 8 consecutive lanes take the 128 contiguous bytes of a row's stage
    const v4u *ga[A_PT], *gw[W_PT];
    int la[A_PT], lw[W_PT];
#pragma unroll
    for (int j = 0; j < A_PT; ++j) {
        const int e = tid + NT * j, r = e / HQ, q = e % HQ;
        ga[j] = reinterpret_cast<const v4u *>(plane + (size_t)(m0 + r) * K + k0 + 8 * q);   // (m0 + r < Mp: pad rows exist)
        la[j] = hswz(r, q);
    }
#pragma unroll
    for (int j = 0; j < W_PT; ++j) {
        const int e = tid + NT * j, r = e / HQ, q = e % HQ;
        const int row = n0 + r < N ? n0 + r : N - 1;   // (the last tile's rows past R: row R - 1 again, never stored)
        gw[j] = reinterpret_cast<const v4u *>(a.W + (size_t)row * K + k0 + 8 * q);
        lw[j] = hswz(r, q);
    }
    v4u ra[2][A_PT], rw[2][W_PT];
    const int s1 = nst > 1 ? 1 : 0;
#pragma unroll
    for (int j = 0; j < A_PT; ++j) ra[0][j] = ga[j][0];
#pragma unroll
    for (int j = 0; j < W_PT; ++j) rw[0][j] = gw[j][0];
#pragma unroll
    for (int j = 0; j < A_PT; ++j) ra[1][j] = ga[j][s1 * HQ];
#pragma unroll
    for (int j = 0; j < W_PT; ++j) rw[1][j] = gw[j][s1 * HQ];
#pragma unroll
    for (int j = 0; j < A_PT; ++j) As[0][la[j]] = ra[0][j];
#pragma unroll
    for (int j = 0; j < W_PT; ++j) Ws[0][lw[j]] = rw[0][j];
    __syncthreads();

    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    // (stage s's register set is s & 1: the body is unrolled by 2 so the set is
    // a constant; nst is even, qtts_pgemmh_plan)
    auto stage = [&](int s, auto setc) {
        constexpr int set = decltype(setc)::value;
        const int cur = s & 1;
        const int sn = s + 2 < nst ? s + 2 : nst - 1;
#pragma unroll
        for (int j = 0; j < A_PT; ++j) ra[set][j] = ga[j][sn * HQ];
#pragma unroll
        for (int j = 0; j < W_PT; ++j) rw[set][j] = gw[j][sn * HQ];
        // (keeps the loads in front of the MFMAs: two stages of cover, not one)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < HK / 16; ++ks) {
            const int q = 2 * ks + fh;   // the lane's 8 k of this step
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                af[t] = __builtin_bit_cast(bf16x8, As[cur][hswz(64 * wm + 32 * t + fr, q)]);
                bf[t] = __builtin_bit_cast(bf16x8, Ws[cur][hswz(64 * wn + 32 * t + fr, q)]);
            }
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tm], bf[tn], acc[tm][tn], 0, 0, 0);
        }
        // stage s + 1 (the other set) into the other buffer
#pragma unroll
        for (int j = 0; j < A_PT; ++j) As[cur ^ 1][la[j]] = ra[set ^ 1][j];
#pragma unroll
        for (int j = 0; j < W_PT; ++j) Ws[cur ^ 1][lw[j]] = rw[set ^ 1][j];
        __syncthreads();
    };
    for (int s = 0; s < nst; s += 2) {
        stage(s, std::integral_constant<int, 0>{});
        stage(s + 1, std::integral_constant<int, 1>{});
    }

    // acc[tm][tn][e] is (row m, weight row n) with
    // m = m0 + 64 wm + 32 tm + (e & 3) + 8 (e >> 2) + 4 fh, n = n0 + 64 wn + 32 tn + fr
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int n = n0 + 64 * wn + 32 * tn + fr;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + 64 * wm + 32 * tm + (e & 3) + 8 * (e >> 2) + 4 * fh;
                const float v = acc[tm][tn][e];
                const float up = __shfl(v, lane + 4 < 64 ? lane + 4 : lane, 64);
                if (m >= M || n >= N) continue;
                if (part) {
                    part[((size_t)blockIdx.z * M + m) * N + n] = v;
                    continue;
                }
                float *yr = a.y + (size_t)m * a.ldy;
                switch (a.epi) {
                    case EPI_STORE: yr[n] = v; break;
                    case EPI_RESID: yr[n] += v; break;
                    case EPI_SWIGLU:
                        if ((n & 7) < 4) yr[(n >> 3) * 4 + (n & 3)] = (v / (1.0f + expf(-v))) * up;
                        break;
                }
            }
        }
    }
}

std::atomic<long long> g_pgemmh_launches{0};

}  // namespace

extern "C" long long qtts_hip_pgemmh_launches(void) { return g_pgemmh_launches.load(); }

// qtts_pgemmh's launch decisions, host only (nothing launched, no pointer
// dereferenced).  The cover test is qtts_pgemm_plan's; the plane scratch needed
// is Mp K bf16.  bn: 256 asks for the 128 x 256 tile, anything else gives 128 x 128.
// 0 = planned, 1 = not covered.
int qtts_pgemmh_plan(const GemvArgs &a, bool has_planes, size_t plane_elems, bool has_part, size_t part_elems, int bn,
                     PgPlan &p) {
    p = PgPlan();
    if (a.nb < 17 || a.C % 256 || a.R % 32 || !a.x || a.table || a.table_f32 || a.xadd || a.xcopy || a.bias ||
        a.ldx % 4 || ((uintptr_t)a.x & 15) ||
        (a.epi != EPI_STORE && a.epi != EPI_RESID && a.epi != EPI_SWIGLU) || !has_planes)
        return 1;
    const int Mp = (a.nb + HM - 1) / HM * HM;
    if ((size_t)Mp * a.C > plane_elems) return 1;
    // The tile width: 128 unless 256 is asked for.  Two 64 KB workgroups share a
    // CU and cover each other's barriers; measured through the whole prefill call
    // 128 is ahead of 256 at every row count (1024 rows 9.58 vs 10.07 ms, 64 rows
    // 3.03 vs 3.41, 4000 rows 48.8 vs 49.5; profiles/prefill_bf16_bench.txt).
    const int BN = bn == 256 ? 256 : 128;
    // split-K while the tiles would not fill the chip, each column an even
    // number of stages (the kernel's loop) and at least 4 of them (256 k):
    // C % 256 == 0 makes one column even
    const int tiles = (a.R + BN - 1) / BN * (Mp / HM), nst = a.C / HK;
    int kz = 1;
    while (has_part && tiles * kz < 256 && kz < 8 && nst % (4 * kz) == 0 && nst / (2 * kz) >= 4 &&
           (size_t)2 * kz * a.nb * a.R <= part_elems)
        kz *= 2;
    p.BN = BN;
    p.Mp = Mp;
    p.kz = kz;
    p.grid = dim3((a.R + BN - 1) / BN, Mp / HM, kz);
    p.kernel = BN == 256 ? RG_PGEMMH_4 : RG_PGEMMH_2;
    return 0;
}

// Returns 1 when the shape is not covered (the caller goes on to the exact
// kernels), 0 ok, -1 error.  plane: >= Mp C bf16 (the first third of
// qtts_pgemm_plane_elems).  bn: as qtts_pgemmh_plan takes it; 0 = QTTS_HIP_PGEMM_BN.
int qtts_pgemmh(const GemvArgs &a, unsigned short *plane, size_t plane_elems, hipStream_t st, float *part,
                size_t part_elems, int bn) {
    PgPlan p;
    if (!bn) bn = qtts_pgemm_bn_env();
    if (qtts_pgemmh_plan(a, plane != nullptr, plane_elems, part != nullptr, part_elems, bn, p)) return 1;
    const int kz = p.kz;
    hipLaunchKernelGGL(k_round1, dim3(p.Mp), dim3(256), 0, st, a.x, a.ldx, a.nb, a.C, a.norm_w, a.eps, plane);
    if (p.BN == 256) {
        hipLaunchKernelGGL(k_pgemmh<4>, p.grid, dim3(512), 0, st, a, plane, kz > 1 ? part : nullptr);
        qtts_last_kernel = "k_pgemmh<4>";
    } else {
        hipLaunchKernelGGL(k_pgemmh<2>, p.grid, dim3(256), 0, st, a, plane, kz > 1 ? part : nullptr);
        qtts_last_kernel = "k_pgemmh<2>";
    }
    ++g_pgemmh_launches;
    if (kz > 1 && qtts_mgemm_reduce(a, part, kz, st) != 0) return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
