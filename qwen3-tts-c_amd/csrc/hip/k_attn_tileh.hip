// k_attn_tileh.hip - tiled causal attention over segments on the bf16 matrix
// cores (gfx950): k_attn_tile's contract (k_attn_tile.hip: segments, q ready,
// every key [0, pos0 + count) in the cache, key t counts for position p iff
// t <= p, both cache element types, HD 64 | 128, 1 | 2 query heads per kv
// head, no window) in the opt-in bf16 prefill attention precision.
//
// Precision: q rounded once to bf16 (nearest even) as it is loaded; K and V
// rounded to bf16 on the way into LDS from an fp32 cache, bits as they are from
// a bf16 cache; P rounded to bf16 before the P V product.  Scores (fp32 sums of
// exact bf16 x bf16 products), the scale (an fp32 multiply after the matrix
// instruction), mask, max, exp, row sums, rescale, accumulators and the final
// division are fp32.  The row sum adds the ROUNDED P values, widened: out is a
// convex combination of the V rows the kernel multiplied.
//
// Matrix instruction: v_mfma_f32_16x16x32_bf16.  With i = lane & 15 and g =
// lane >> 4, A: lane (i, g) holds A[i][8 g .. + 7], B: lane (j, g) holds
// B[8 g .. + 7][j], D: lane (j, g) holds D[4 g .. + 3][j].  Both products are
// computed TRANSPOSED, so that P never leaves registers:
//   S^T = K q^T     A: a 16-key x 32-d slab of K, lane (i, g) reads K[key i][32 c
//                   + 8 g .. + 7], one 16-byte LDS read of row-major K.  B: q^T,
//                   in registers for the life of the tile (HD / 32 operands per
//                   16 query rows).  D: lane (j, g) holds the scores of query
//                   row j against keys 4 g .. 4 g + 3 of the key tile.
//   O^T += V^T P^T  the contraction index is free to permute: index 8 g + e of a
//                   32-key step is key 4 g + e of the step's first key tile (e <
//                   4) and key 4 g + e - 4 of its second.  B (P^T) is then the 8
//                   scores the lane already holds, exponentiated, rounded and
//                   packed in place.  A (V^T): V is staged transposed in LDS,
//                   [HD][BN] bf16 with the keys of a step in that order, so lane
//                   (d, g) reads its 8 keys as one 16-byte chunk.  D: lane (j, g)
//                   holds O[row j][16 dt + 4 g .. + 3], 16 contiguous bytes.
// A lane's scores all belong to one query row: max, sum and rescale factor are
// one scalar per lane and 16-row tile.  The row max is two cross-lane steps
// (v_permlane16 / 32_swap) over the four lane groups; the row sum stays a
// per-lane partial (the rescale factor is the row's, the same in its four
// lanes) and is summed across the groups once, at the end; the accumulator
// rescale needs no cross-lane traffic and is skipped while no row of the wave
// moves its maximum.
//
// Workgroup: one (tile of BM = 64 query positions, kv head, segment), grid and
// tile order as k_attn_tile (the longest tiles first), 4 waves.  GPH 2: wave w
// owns 32 rows (two 16-row tiles that share every K and V operand read) of
// head w / 2 at tile rows 32 (w & 1); GPH 1: 16 rows at 16 w.  A K / V block
// serves 64 GPH query rows.
//
// LDS: one block of BN = 64 keys.  K [BN][HD] bf16 in 16-byte chunks, chunk q
// of row r at q ^ (r & 15) (HD 128: rows of 256 B) or q ^ ((r >> 1) & 7) (HD
// 64: rows of 128 B): the 16 lanes of a ds_read_b128 pass (16 consecutive keys,
// one chunk) and of a stage write (one row, or two, all chunks) hit 16 distinct
// 16-byte slots of a 256-byte bank line.  V^T [HD][BN] bf16, rows of 128 B, the
// same swizzle; a stage thread owns 4 consecutive keys x 8 d and writes 8 x 8
// bytes (4 d-chunks x 8 key groups per 32 lanes: two lanes per 8-byte slot
// pair of a bank line, a 2-way conflict on 8 writes per block).  HD 128: 16 +
// 16 KB.  The next block's cache rows are loaded into registers (raw: fp32 rows
// are rounded as they are staged) while the current one is multiplied; one LDS
// buffer, two barriers per block.  Keys above the tile's last position are
// loaded from a clamped valid row and stored as zeros, K and V alike (a masked
// probability is 0, and 0 x NaN is NaN in the matrix instruction).
//
// Causality as k_attn_tile: blocks wholly above the tile's last position are
// never loaded, a wave skips blocks wholly above its last position (and, in
// its last block, the 16-key tiles wholly above it), only blocks that reach
// above the wave's first position take the per-element mask, rows past the
// segment's end are computed from a clamped row and never stored.
#include "qtts_common.h"
#include "qtts_kernels.h"
#include <atomic>

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 64, BN = 64, NT = 256;
constexpr float LOG2E = 1.44269504088896340736f;

__device__ __forceinline__ uint32_t th_pk(float lo, float hi) {   // two floats -> bf16 pair, nearest even
    uint32_t a = __float_as_uint(lo), b = __float_as_uint(hi);
    a = (a + 0x7FFFu + ((a >> 16) & 1u)) >> 16;
    b = (b + 0x7FFFu + ((b >> 16) & 1u)) & 0xFFFF0000u;
    return a | b;
}
__device__ __forceinline__ v4u th_pk8(const v4f &a, const v4f &b) {
    v4u r;
    r.x = th_pk(a.x, a.y); r.y = th_pk(a.z, a.w); r.z = th_pk(b.x, b.y); r.w = th_pk(b.z, b.w);
    return r;
}

// 8 consecutive cache elements, raw: one 16-byte load (bf16) or two (fp32)
template <typename CT> struct Raw8;
template <> struct Raw8<bf16_t> {
    v4u u;
    __device__ __forceinline__ void load(const bf16_t *p) { u = *reinterpret_cast<const v4u *>(p); }
    __device__ __forceinline__ v4u bits() const { return u; }
};
template <> struct Raw8<float> {
    v4f a, b;
    __device__ __forceinline__ void load(const float *p) {
        a = *reinterpret_cast<const v4f *>(p);
        b = *reinterpret_cast<const v4f *>(p + 4);
    }
    __device__ __forceinline__ v4u bits() const { return th_pk8(a, b); }
};

// 16-byte chunk index of (row, chunk q) in a tile of rows of CPR chunks
template <int CPR>
__device__ __forceinline__ int tswz(int row, int q) {
    if constexpr (CPR == 16) return row * 16 + (q ^ (row & 15));
    else return row * 8 + (q ^ ((row >> 1) & 7));
}

template <int HD, int GPH, typename CT>
__global__ __launch_bounds__(NT, 2) void k_attn_tileh(AttnArgs a, const AttnSeg *segs) {
    constexpr int CPR = HD / 8;                 // 16-byte chunks per K row
    constexpr int NK = BN * CPR / NT;           // K chunks per thread and block
    constexpr int VI = (BN / 4) * CPR;          // V items (4 keys x 8 d) per block: one per thread, HD 64: threads < 128
    constexpr int RT = GPH;                     // 16-row tiles per wave
    constexpr int WPH = 4 / GPH;                // waves per head
    constexpr int NC = HD / 32, ND = HD / 16;
    static_assert((HD == 64 || HD == 128) && (GPH == 1 || GPH == 2) && VI <= NT, "k_attn_tileh: shapes");
    __shared__ __attribute__((aligned(16))) v4u Ks[BN * CPR];
    __shared__ __attribute__((aligned(16))) v4u Vt[HD * 8];

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

    // ---- this wave's 16 RT rows: head, positions; q^T as B operands ----
    const int h = kvh * GPH + w / WPH;
    const int wm = 16 * RT * (w % WPH);                              // first tile row of the wave
    const int wp0 = sg.pos0 + m0 + wm;                               // its position
    const int wplast = min(wp0 + 16 * RT - 1, plast);
    bf16x8 qf[RT][NC];
    int rp[RT];                                                      // position of the lane's query row of tile rt
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        // rows past the segment repeat its last row (computed, never stored)
        const int qrow = sg.row0 + m0 + min(wm + 16 * rt + li, nrow - 1);
        const float *qp = a.qkv + (size_t)qrow * a.ld_qkv + h * HD + 8 * lg;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            qf[rt][c] = __builtin_bit_cast(bf16x8, th_pk8(*reinterpret_cast<const v4f *>(qp + 32 * c),
                                                          *reinterpret_cast<const v4f *>(qp + 32 * c + 4)));
        rp[rt] = min(wp0 + 16 * rt + li, plast);
    }

    // ---- cache rows of a block, in registers ----
    // K item j: chunk kq[j] of key row kr[j]; the V item: d-chunk vdc of keys 4 vkg .. + 3
    // (4 d-chunks of a key group in neighbouring lanes: 64 contiguous bytes per row)
    const bool vown = VI == NT || tid < VI;
    const int vdc = (tid & 3) + 4 * ((tid >> 6) % (CPR / 4)), vkg = (tid >> 2) & 15;
    Raw8<CT> kreg[NK], vreg[4];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const int c = tid + NT * j, kr = c / CPR, kq = c % CPR;
            const int t = min(kb * BN + kr, plast);                  // (rows above plast: a valid row, zeroed below)
            kreg[j].load(Kc + (size_t)t * KVD + 8 * kq);
        }
        if (vown) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = min(kb * BN + 4 * vkg + i, plast);
                vreg[i].load(Vc + (size_t)t * KVD + 8 * vdc);
            }
        }
    };
    auto stage = [&](int kb) {
        const v4u z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const int c = tid + NT * j, kr = c / CPR, kq = c % CPR;
            Ks[tswz<CPR>(kr, kq)] = kb * BN + kr <= plast ? kreg[j].bits() : z;
        }
        if (vown) {
            v4u r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = kb * BN + 4 * vkg + i <= plast ? vreg[i].bits() : z;
            // keys 4 vkg .. + 3 of the block: step vkg / 8, key tile (vkg / 4) & 1, lane group vkg & 3 of the
            // V^T operand: the 8-byte half (vkg / 4) & 1 of chunk 4 (vkg / 8) + (vkg & 3)
            const int vq = 4 * (vkg >> 3) + (vkg & 3), vh = (vkg >> 2) & 1;
            v2u *vt2 = reinterpret_cast<v2u *>(Vt);
#pragma unroll
            for (int e = 0; e < 4; ++e) {                            // d = 8 vdc + 2 e (low halves) and + 1 (high)
                const uint32_t x0 = r[0][e], x1 = r[1][e], x2 = r[2][e], x3 = r[3][e];
                v2u lo, hi;
                lo.x = (x0 & 0xFFFFu) | (x1 << 16); lo.y = (x2 & 0xFFFFu) | (x3 << 16);
                hi.x = (x0 >> 16) | (x1 & 0xFFFF0000u); hi.y = (x2 >> 16) | (x3 & 0xFFFF0000u);
                vt2[2 * tswz<8>(8 * vdc + 2 * e, vq) + vh] = lo;
                vt2[2 * tswz<8>(8 * vdc + 2 * e + 1, vq) + vh] = hi;
            }
        }
    };

    const float scale = div_rn(1.0f, sqrt_rn((float)HD));
    float mrow[RT], lrow[RT];                                        // the row's maximum; the LANE's part of its sum
    v4f o[RT][ND];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        mrow[rt] = -INFINITY; lrow[rt] = 0.f;
#pragma unroll
        for (int n = 0; n < ND; ++n) o[rt][n] = v4f{0.f, 0.f, 0.f, 0.f};
    }

    fetch(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();                                             // the previous block's reads are done
        stage(kb);
        __syncthreads();
        if (kb + 1 < nkb) fetch(kb + 1);
        if (kb * BN > wplast) continue;                              // wholly above this wave's rows
        const int nkt = min(BN / 16, (wplast - kb * BN) / 16 + 1);   // key tiles that reach the wave's rows
        // ---- S^T = K q^T: s[rt][kt][v] = row (rt, li) against key kb BN + 16 kt + 4 lg + v ----
        v4f s[RT][BN / 16];
#pragma unroll
        for (int kt = 0; kt < BN / 16; ++kt) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) s[rt][kt] = v4f{0.f, 0.f, 0.f, 0.f};
            if (kt < nkt) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const bf16x8 kf = __builtin_bit_cast(bf16x8, Ks[tswz<CPR>(16 * kt + li, 4 * c + lg)]);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        s[rt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[rt][c], s[rt][kt], 0, 0, 0);
                }
            }
        }
        // ---- scale, mask, online softmax; P^T rounded and packed in place ----
        const bool diag = kb * BN + BN - 1 > min(wp0, plast);
        bf16x8 pf[RT][BN / 32];
        bool moved = false;
        float al[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < BN / 16; ++kt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float x = s[rt][kt][v] * scale;
                    if (diag) x = kb * BN + 16 * kt + 4 * lg + v <= rp[rt] ? x : -INFINITY;
                    s[rt][kt][v] = x;
                    mx = fmaxf(mx, x);
                }
            float mine, other = swap16_other(mx, mine);              // the row's four lanes: lane groups 0 .. 3
            mx = fmaxf(mine, other);
            other = swap32_other(mx, mine);
            const float mn = fmaxf(mrow[rt], fmaxf(mine, other));    // (finite: block 0 holds key 0 <= p)
            al[rt] = __builtin_amdgcn_exp2f((mrow[rt] - mn) * LOG2E);
            moved = moved || mn != mrow[rt];
            mrow[rt] = mn;
            float ls = 0.f;
#pragma unroll
            for (int st = 0; st < BN / 32; ++st) {
                v4u pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) {                        // index 8 lg + 2 e, + 1 of the step
                    const float p0 = __builtin_amdgcn_exp2f((s[rt][2 * st + e / 2][2 * (e & 1)] - mn) * LOG2E);
                    const float p1 = __builtin_amdgcn_exp2f((s[rt][2 * st + e / 2][2 * (e & 1) + 1] - mn) * LOG2E);
                    const uint32_t u = th_pk(p0, p1);
                    pk[e] = u;
                    ls += __uint_as_float(u << 16) + __uint_as_float(u & 0xFFFF0000u);
                }
                pf[rt][st] = __builtin_bit_cast(bf16x8, pk);
            }
            lrow[rt] = lrow[rt] * al[rt] + ls;
        }
        if (__any(moved)) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < ND; ++n) o[rt][n] *= al[rt];
        }
        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int st = 0; st < BN / 32; ++st) {
            if (2 * st < nkt) {
#pragma unroll
                for (int n = 0; n < ND; ++n) {
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, Vt[tswz<8>(16 * n + li, 4 * st + lg)]);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        o[rt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[rt][st], o[rt][n], 0, 0, 0);
                }
            }
        }
    }

    // ---- out = O / l: row (rt, li), columns 16 n + 4 lg .. + 3 ----
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float mine, other = swap16_other(lrow[rt], mine);
        float l = mine + other;
        other = swap32_other(l, mine);
        l = mine + other;
        const int m = wm + 16 * rt + li;
        if (m >= nrow) continue;
        const float inv = div_rn(1.0f, l);
        float *op = a.out + (size_t)(sg.row0 + m0 + m) * a.ld_out + h * HD + 4 * lg;
#pragma unroll
        for (int n = 0; n < ND; ++n) *reinterpret_cast<v4f *>(op + 16 * n) = o[rt][n] * inv;
    }
}

}  // namespace

bool qtts_attn_tileh_covers(const AttnArgs &a) { return qtts_attn_tile_covers(a); }   // the same contract

static std::atomic<long long> g_tileh_launches{0};
long long qtts_attn_tileh_launches() { return g_tileh_launches.load(); }

int qtts_attn_tileh(const AttnArgs &a, const AttnSeg *segs, int nseg, hipStream_t st) {
    if (!qtts_attn_tileh_covers(a) || !segs || nseg < 1 || nseg > 65535) return 1;
    const int longest = a.seg_max > 0 ? a.seg_max : a.nrows;
    const int gph = a.NH / a.KV;
    const dim3 grid((longest + BM - 1) / BM, a.KV, nseg), block(NT);
#define QTTS_ATH(H, G)                                                                                 \
    if (a.HD == H && gph == G) {                                                                       \
        if (a.kv_dtype == 1) {                                                                         \
            hipLaunchKernelGGL((k_attn_tileh<H, G, bf16_t>), grid, block, 0, st, a, segs);             \
            qtts_last_kernel = "k_attn_tileh<" #H ", " #G ", bf16>";                                   \
        } else {                                                                                       \
            hipLaunchKernelGGL((k_attn_tileh<H, G, float>), grid, block, 0, st, a, segs);              \
            qtts_last_kernel = "k_attn_tileh<" #H ", " #G ">";                                         \
        }                                                                                              \
    }
    QTTS_ATH(128, 2) QTTS_ATH(128, 1) QTTS_ATH(64, 2) QTTS_ATH(64, 1)
#undef QTTS_ATH
    ++g_tileh_launches;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
