// k_attn_tile.hip - tiled causal attention over segments on the fp32 matrix
// cores (gfx950): the multi-row attention of long prefills.
//
// k_attn mode 1 launches one workgroup per (query head, row) and each reads
// every key and value row of its slot on its own.  Here a key block is loaded
// once for a whole tile of query rows and for every query head of its kv head.
//
// A segment (AttnSeg) is a run of `count` consecutive rows of one slot at
// consecutive positions pos0, pos0 + 1, ...; its rows are rows row0, row0 + 1,
// ... of qkv / out.  All keys [0, pos0 + count) are in the cache when the
// kernel runs (qtts_qk_prep wrote the call's own rows), and the kernel reads
// nothing else.  Key t counts for the row at position p iff t <= p.
//
// Workgroup: one (tile of BM = 32 query positions, kv head, segment); grid
// (tiles of the longest segment, KV, segments), tiles past a segment's end
// exit at once, the last (longest) tiles are scheduled first.  GPH = NH / KV
// query heads are stacked: 2 GPH waves, wave w owns the 16 rows of head
// w / 2 at tile positions 16 (w & 1) .. + 15, so a K / V block serves 32 GPH
// query rows.
//
// LDS: one key block of BN = 32 keys, K and V each [BN][HD + 4] fp32 (a bf16
// cache is widened on the way in; keys above the tile's last position are
// stored as zeros, they are masked and never read from the cache), and one
// [16][BN + 4] strip per wave.  HD 128, GPH 2: 33.8 + 9.2 KB.  The next
// block's cache rows are loaded into registers while the current one is
// multiplied (one LDS buffer, two barriers per block).
//
// Registers: q in A-operand layout for the life of the tile (HD / 4 VGPRs),
// the running max / sum of the lane's 4 rows, the output accumulators (HD / 4
// VGPRs), two 16 x 16 score tiles.
//
// Matrix instruction: v_mfma_f32_16x16x4_f32 (A: lane 16 k + i holds A[i][k],
// B: lane 16 k + j holds B[k][j], D: lane 16 (i / 4) + j holds D[i][j] in VGPR
// i % 4), fp32 operands, products and sums.  The contraction index and the
// output column are free to permute, so every LDS operand read is 16 bytes:
//   S = q K^T   step (c4, i): lane group k = lane / 16 contracts d = 16 c4 + 4 k + i;
//               one ds_read_b128 of K[key][16 c4 + 4 k ..] feeds 4 steps
//   O += P V    step (s4, i): key 16 s4 + 4 k + i; output tile 4 ng + i' holds
//               columns d = 64 ng + 4 j + i', so one ds_read_b128 of
//               V[key][64 ng + 4 j ..] feeds 4 tiles and a lane's 4 outputs of a
//               row are 16 contiguous bytes
// P goes through the wave's strip only to turn from D layout into A layout.
//
// Online softmax (expf, scale 1 / sqrt(HD) as k_attn): per block the row
// maxima and sums over 16-lane groups, accumulators rescaled by exp(m_old -
// m_new).  Block 0 always holds key 0 <= p, so a row's maximum is finite from
// the first block on.  Only blocks that reach above the wave's first position
// take the per-element mask; a wave skips blocks wholly above its last
// position; blocks wholly above the tile's last position are never loaded.
#include "qtts_common.h"
#include "qtts_kernels.h"
#include <atomic>

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

constexpr int BM = 32, BN = 32, PLD = BN + 4;

// 4 consecutive cache elements as fp32 (bf16: a 16-bit shift, exact)
template <typename CT>
__device__ __forceinline__ v4f ld4(const CT *p) {
    if constexpr (sizeof(CT) == 4) return *reinterpret_cast<const v4f *>(p);
    else {
        const v2u u = *reinterpret_cast<const v2u *>(p);
        v4f r;
        r.x = __uint_as_float(u.x << 16); r.y = __uint_as_float(u.x & 0xFFFF0000u);
        r.z = __uint_as_float(u.y << 16); r.w = __uint_as_float(u.y & 0xFFFF0000u);
        return r;
    }
}

template <int HD, int GPH, typename CT>
__global__ __launch_bounds__(128 * GPH) void k_attn_tile(AttnArgs a, const AttnSeg *segs) {
    constexpr int NT = 128 * GPH;          // threads
    constexpr int LD = HD + 4;             // K / V row stride in LDS
    constexpr int C4 = HD / 4;             // 16-byte chunks per row
    constexpr int NLD = BN * C4 / NT;      // chunks per thread per block (K and V each)
    constexpr int NQ = HD / 16, NG = HD / 64;
    static_assert(BN * C4 % NT == 0, "whole chunks per thread");
    __shared__ __attribute__((aligned(16))) float Ks[BN * LD];
    __shared__ __attribute__((aligned(16))) float Vs[BN * LD];
    __shared__ __attribute__((aligned(16))) float Ps[2 * GPH][16 * PLD];

    const AttnSeg sg = segs[blockIdx.z];
    const int ntile = (sg.count + BM - 1) / BM;
    if ((int)blockIdx.x >= ntile) return;
    const int m0 = (ntile - 1 - (int)blockIdx.x) * BM;               // the longest tiles first
    const int kvh = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int KVD = a.KV * HD;
    const int nrow = min(BM, sg.count - m0);                         // live rows of the tile
    const int plast = sg.pos0 + m0 + nrow - 1;                       // the tile's last position
    const int nkb = plast / BN + 1;
    const CT *Kc = reinterpret_cast<const CT *>(a.kc) + (size_t)sg.slot * a.S * KVD + kvh * HD;
    const CT *Vc = reinterpret_cast<const CT *>(a.vc) + (size_t)sg.slot * a.S * KVD + kvh * HD;

    // ---- this wave's 16 rows: head, positions ----
    const int h = kvh * GPH + (w >> 1);
    const int wm = 16 * (w & 1);                                     // first tile row of the wave
    const int wp0 = sg.pos0 + m0 + wm;                               // its position
    const int wplast = min(wp0 + 15, plast);
    // rows past the segment repeat its last row (computed, never stored)
    const int qrow = sg.row0 + m0 + min(wm + li, nrow - 1);
    v4f q[NQ];
    {
        const float *qp = a.qkv + (size_t)qrow * a.ld_qkv + h * HD + 4 * lg;
#pragma unroll
        for (int c = 0; c < NQ; ++c) q[c] = *reinterpret_cast<const v4f *>(qp + 16 * c);
    }
    int rp[4];                                                       // positions of the lane's 4 score rows
#pragma unroll
    for (int v = 0; v < 4; ++v) rp[v] = min(wp0 + 4 * lg + v, plast);

    // ---- cache rows of a block, in registers ----
    v4f kreg[NLD], vreg[NLD];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int c = tid + NT * j, kr = c / C4, kc4 = c - kr * C4;
            const int t = min(kb * BN + kr, plast);                  // (rows above plast: a valid row, zeroed below)
            kreg[j] = ld4(Kc + (size_t)t * KVD + 4 * kc4);
            vreg[j] = ld4(Vc + (size_t)t * KVD + 4 * kc4);
        }
    };
    auto stage = [&](int kb) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int c = tid + NT * j, kr = c / C4, kc4 = c - kr * C4;
            const bool live = kb * BN + kr <= plast;
            const v4f z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<v4f *>(Ks + kr * LD + 4 * kc4) = live ? kreg[j] : z;
            *reinterpret_cast<v4f *>(Vs + kr * LD + 4 * kc4) = live ? vreg[j] : z;
        }
    };

    const float scale = div_rn(1.0f, sqrt_rn((float)HD));
    float mrow[4], lrow[4];
    v4f o[NQ];
#pragma unroll
    for (int v = 0; v < 4; ++v) { mrow[v] = -INFINITY; lrow[v] = 0.f; }
#pragma unroll
    for (int n = 0; n < NQ; ++n) o[n] = v4f{0.f, 0.f, 0.f, 0.f};
    float *ps = Ps[w];

    fetch(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();                                             // the previous block's reads are done
        stage(kb);
        __syncthreads();
        if (kb + 1 < nkb) fetch(kb + 1);
        if (kb * BN > wplast) continue;                              // wholly above this wave's rows
        // ---- S = q K^T for the block's two 16-key halves ----
        v4f s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
            const v4f k0 = *reinterpret_cast<const v4f *>(Ks + li * LD + 16 * c + 4 * lg);
            const v4f k1 = *reinterpret_cast<const v4f *>(Ks + (16 + li) * LD + 16 * c + 4 * lg);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(q[c][i], k0[i], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q[c][i], k1[i], s1, 0, 0, 0);
            }
        }
        // ---- scale, mask, online softmax: rows 4 lg + v, keys kb BN + li and + 16 ----
        const bool diag = kb * BN + BN - 1 > min(wp0, plast);
        const int t0 = kb * BN + li, t1 = t0 + 16;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float x0 = s0[v] * scale, x1 = s1[v] * scale;
            if (diag) {
                x0 = t0 <= rp[v] ? x0 : -INFINITY;
                x1 = t1 <= rp[v] ? x1 : -INFINITY;
            }
            const float mn = fmaxf(mrow[v], group_max<16>(fmaxf(x0, x1)));
            const float al = expf(mrow[v] - mn);
            const float e0 = expf(x0 - mn), e1 = expf(x1 - mn);
            lrow[v] = lrow[v] * al + group_sum<16>(e0 + e1);
            mrow[v] = mn;
#pragma unroll
            for (int n = 0; n < NQ; ++n) o[n][v] *= al;
            ps[(4 * lg + v) * PLD + li] = e0;
            ps[(4 * lg + v) * PLD + 16 + li] = e1;
        }
        // the strip is this wave's alone: its LDS operations complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- O += P V ----
#pragma unroll
        for (int s4 = 0; s4 < BN / 16; ++s4) {
            const v4f p = *reinterpret_cast<const v4f *>(ps + li * PLD + 16 * s4 + 4 * lg);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float *vr = Vs + (16 * s4 + 4 * lg + i) * LD + 4 * li;
#pragma unroll
                for (int ng = 0; ng < NG; ++ng) {
                    const v4f vv = *reinterpret_cast<const v4f *>(vr + 64 * ng);
#pragma unroll
                    for (int i2 = 0; i2 < 4; ++i2)
                        o[4 * ng + i2] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[i], vv[i2], o[4 * ng + i2], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                             // the strip's reads before the next block's writes
    }

    // ---- out = O / l: row 4 lg + v, columns 64 ng + 4 li .. + 3 ----
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int m = wm + 4 * lg + v;
        if (m >= nrow) continue;
        const float inv = div_rn(1.0f, lrow[v]);
        float *op = a.out + (size_t)(sg.row0 + m0 + m) * a.ld_out + h * HD + 4 * li;
#pragma unroll
        for (int ng = 0; ng < NG; ++ng) {
            v4f r;
#pragma unroll
            for (int i2 = 0; i2 < 4; ++i2) r[i2] = o[4 * ng + i2][v] * inv;
            *reinterpret_cast<v4f *>(op + 64 * ng) = r;
        }
    }
}

}  // namespace

bool qtts_attn_tile_covers(const AttnArgs &a) {
    if (a.KV < 1 || a.NH % a.KV) return false;
    const int gph = a.NH / a.KV;
    return a.win == 0 && (a.HD == 64 || a.HD == 128) && (gph == 1 || gph == 2) &&
           (a.kv_dtype == 0 || a.kv_dtype == 1) && a.S >= 1 && a.nrows >= 1 && a.qkv && a.out && a.kc && a.vc &&
           a.ld_qkv % 4 == 0 && a.ld_out % 4 == 0 && ((uintptr_t)a.qkv & 15) == 0 && ((uintptr_t)a.out & 15) == 0 &&
           ((uintptr_t)a.kc & 15) == 0 && ((uintptr_t)a.vc & 15) == 0;
}

static std::atomic<long long> g_tile_launches{0};
long long qtts_attn_tile_launches() { return g_tile_launches.load(); }

int qtts_attn_tile(const AttnArgs &a, const AttnSeg *segs, int nseg, hipStream_t st) {
    if (!qtts_attn_tile_covers(a) || !segs || nseg < 1 || nseg > 65535) return 1;
    const int longest = a.seg_max > 0 ? a.seg_max : a.nrows;
    const int gph = a.NH / a.KV;
    const dim3 grid((longest + BM - 1) / BM, a.KV, nseg), block(128 * gph);
#define QTTS_AT(H, G)                                                                                  \
    if (a.HD == H && gph == G) {                                                                       \
        if (a.kv_dtype == 1) {                                                                         \
            hipLaunchKernelGGL((k_attn_tile<H, G, bf16_t>), grid, block, 0, st, a, segs);              \
            qtts_last_kernel = "k_attn_tile<" #H ", " #G ", bf16>";                                    \
        } else {                                                                                       \
            hipLaunchKernelGGL((k_attn_tile<H, G, float>), grid, block, 0, st, a, segs);               \
            qtts_last_kernel = "k_attn_tile<" #H ", " #G ">";                                          \
        }                                                                                              \
    }
    QTTS_AT(128, 2) QTTS_AT(128, 1) QTTS_AT(64, 2) QTTS_AT(64, 1)
#undef QTTS_AT
    ++g_tile_launches;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
