// qtts_bgemv.hip - the planner and router of the lock-step batch GEMV (2..64
// rows): which of k_gemvb / k_gemvm / k_gemvx takes a GemvArgs, with which
// template integers, grid, block and LDS bytes (qtts_bgemv_plan: host code, no
// launch; tests/test_bgemv_plan.py pins it without a GPU), and the launch of
// that plan (qtts_bgemv).  The kernels, and the launch switch over their
// instantiations, are in k_gemvb.hip, k_gemvm.hip and k_gemvx.hip.
#include <algorithm>

#include "qtts_bgemv_dev.h"

namespace {

// What all three kernels ask of their arguments; fills the K columns and the
// source kind.  false = not covered.
bool args_ok(const GemvArgs &a, int &kz, int &src) {
    if (a.nb < 2 || a.nb > 64 || a.R % 16 || a.C % 32 || (size_t)a.R * a.C * 2 >= ((size_t)1 << 31)) return false;
    const bool tab = a.table != nullptr, tabf = !tab && a.table_f32 != nullptr;
    if (tab || tabf) {
        if (!a.ids || (tabf && ((uintptr_t)a.table_f32 & 15))) return false;
    } else if (!a.x || a.ldx % 4 || ((uintptr_t)a.x & 15)) {
        return false;
    }
    if (a.norm_w && ((uintptr_t)a.norm_w & 15)) return false;
    if (a.xcopy && (a.ldxc % 4 || ((uintptr_t)a.xcopy & 15))) return false;
    // (at most 4 partials: k_gemvb / k_gemvx hold them in registers, and the runtime's split-K has at most 4 columns)
    if (a.xadd && (tab || tabf || ((uintptr_t)a.xadd & 15) || a.ld_xadd % 4 || a.ldb_xadd % 4 || a.n_xadd < 1 ||
                   a.n_xadd > 4))
        return false;
    if (a.amerge) return false;   // the attention merge is the batch-1 prologue's (k_gemvw)
    kz = a.ypart ? a.kz : 1;
    if (a.ypart && (kz < 2 || (a.tick && kz > 4) || a.norm_w || tab || tabf || a.xcopy || a.C % (32 * kz) ||
                    ((uintptr_t)a.ypart & 3)))
        return false;
    src = tab ? BG_SRC_TAB : tabf ? BG_SRC_TABF : a.xadd ? BG_SRC_XADD : BG_SRC_X;
    return true;
}
// a self-reducing split-K request (GemvArgs::tick) is complete
bool tick_ok(const GemvArgs &a) { return a.ypart && a.y && a.epi == EPI_RESID; }

// ---- k_gemvb
int geom_gemvb(const GemvArgs &a, int kz, int src, BgPlan &p) {
    // (read per call: launches happen at graph capture, and tests switch it
    // per model instance).  QTTS_HIP_GEMVB=0 keeps k_gemvm for every shape (A/B).
    const char *ge = getenv("QTTS_HIP_GEMVB");
    if (ge && !atoi(ge)) return 1;
    if (a.tick && !tick_ok(a)) return 1;   // (not covered: k_gemvm, asked next, reports the error)
    const bool xadd = src == BG_SRC_XADD;
    // K slice per wave: the fewest steps that keep <= wmax waves (16; the
    // QTTS_HIP_GB_W=8 A/B switch: 512-thread workgroups, two per CU, one tile each)
    const char *gbw = getenv("QTTS_HIP_GB_W");
    const int wmax = gbw && atoi(gbw) == 8 ? 8 : 16;
    const int S = a.C / kz / 32;
    int SPW = 1;
    while (SPW < 8 && (S / SPW > wmax || S % SPW)) SPW *= 2;
    if (S % SPW || S / SPW > 16) return 1;
    const int W = S / SPW;
    const int NBC = a.nb <= 8 ? 8 : 16;
    const int PM = xadd ? (a.n_xadd <= 2 ? 2 : 4) : 0;
    // tiles per workgroup: about one round of workgroups over the 256 CUs,
    // within the register file (estimate below) and W >= TPW epilogue waves
    const int T = a.R / 16;
    int TPW = wmax == 8 && W <= 8 ? 1 : (T * kz + 128) / 256;
    TPW = std::max(1, std::min(TPW, 3));
    if (SPW == 8 && TPW > 2) TPW = 2;
    if (SPW <= 2 && TPW > 2) TPW = 2;
    if (SPW == 1) TPW = 1;
    // instantiations whose partials would not fit the 128 registers of a
    // 1024-thread workgroup (hipcc -Rpass-analysis=kernel-resource-usage
    // reports scratch for exactly these): k_gemvm takes those shapes
    auto spills = [&](int tpw) {
        if (PM == 0) return false;
        if (NBC == 16) return SPW >= 4;
        if (SPW == 8) return !(tpw == 1 && PM == 2);
        return SPW == 4 && tpw == 3 && PM == 4;
    };
    while (TPW > 1 && (spills(TPW) || W < TPW)) --TPW;
    if (spills(TPW) || W < TPW) return 1;
    const int wreg = std::max(a.nb * (32 * SPW + 4), TPW * 256);
    const size_t smem = ((size_t)W * wreg + (size_t)W * 16) * sizeof(float);
    if (smem > 160 * 1024) return 1;
    const dim3 grid((T + TPW - 1) / TPW, kz);
    if (a.tick && (int)grid.x > QTTS_GM_TICKS) return 1;
    p.kernel = BG_GEMVB; p.nt = 5;
    p.t[0] = SPW; p.t[1] = TPW; p.t[2] = NBC; p.t[3] = PM; p.t[4] = src;
    p.grid = grid; p.block = dim3(64 * W); p.smem = smem;
    return 0;
}

// ---- k_gemvm
// LDS budget for the three bf16 planes of the staged x rows (bytes): one
// workgroup per CU at the largest.
constexpr int GM_PLANES_MAX = 150 * 1024;
int gm_planes(int nb, int cch) { return 3 * nb * (cch + 8) * 2; }

int geom_gemvm(const GemvArgs &in, int kz, int src, BgPlan &p) {
    GemvArgs a = in;
    a.C /= kz;   // the K extent one workgroup column takes (host-side configuration only)
    // 16 waves per workgroup where the shape allows (one workgroup per CU):
    // KS waves per tile keep >= 2 K steps each; TPW tiles per workgroup bring
    // the grid to about one round over the 256 CUs (the x prologue is paid
    // once per workgroup)
    const int nsteps = a.C / 32, T = a.R / 16;
    int tpw = (T + 255) / 256;
    if (tpw > 4) tpw = 4;
    int KS = 16 / (tpw == 3 ? 4 : tpw);
    while (KS > 4 && nsteps < 2 * KS) KS /= 2;
    if (tpw * KS > 16) tpw = 16 / KS;
    // three tiles x 4 waves leave 768 threads, so > 4 x units per thread at
    // batch >= 8 (whose registers, with the partials and the weight group in
    // flight, spill): four tiles per 1024-thread workgroup instead
    if (tpw == 3 && (a.nb * a.C / 4 + 767) / 768 > 4) { tpw = 4; KS = 4; }
    // column chunk: the whole row when it fits, else the fewest equal chunks
    // of whole 32 x KS-column step rounds with an even step count per wave
    int cch = a.C;
    if (gm_planes(a.nb, a.C) > GM_PLANES_MAX) {
        const int unit = 32 * KS;
        if (a.C % unit) return 1;
        int n = 2;
        for (; n <= a.C / unit; ++n)
            if ((a.C / unit) % n == 0 && gm_planes(a.nb, a.C / n) <= GM_PLANES_MAX && (a.C / unit / n) % 2 == 0)
                break;
        if (n > a.C / unit) return 1;
        cch = a.C / n;
    }
    int U;
    if (cch < a.C) {
        const int spc = cch / 32 / KS;
        U = spc % 8 == 0 ? 8 : spc % 4 == 0 ? 4 : 2;
    } else {
        const int J = (nsteps + KS - 1) / KS;
        U = J <= 2 ? 2 : J <= 4 ? 4 : 8;
    }
    const int nthr = 64 * KS * tpw, nu = a.nb * a.C / 4;
    const int xu = (cch == a.C && a.C % 256 == 0) ? (nu + nthr - 1) / nthr : 0;
    const int XU = xu == 0 || xu > 8 ? 0 : xu <= 1 ? 1 : xu <= 2 ? 2 : xu <= 4 ? 4 : xu <= 6 ? 6 : 8;
    const int region = std::max(gm_planes(a.nb, cch), nthr / 64 * 64 * 16);
    const size_t smem = (size_t)region + (16 + (a.nb * a.C / 256 > 64 ? a.nb * a.C / 256 : 64)) * 4;
    const dim3 grid((T + tpw - 1) / tpw, kz);
    // (the last kernel asked at 2..16 rows: a bad ticket request is an error here, not "not covered")
    if (a.tick && (!tick_ok(a) || (int)grid.x > QTTS_GM_TICKS)) {
        fprintf(stderr, "qtts_gemvm: self-reducing split-K needs ypart, y, EPI_RESID and <= %d row blocks\n",
                QTTS_GM_TICKS);
        return -1;
    }
    p.kernel = BG_GEMVM; p.nt = 4;
    p.t[0] = U; p.t[1] = XU; p.t[2] = KS; p.t[3] = XU ? src : BG_SRC_ANY;
    p.grid = grid; p.block = dim3(nthr); p.smem = smem; p.tpw = tpw; p.cch = cch;
    return 0;
}

// ---- k_gemvx
int geom_gemvx(const GemvArgs &a, int kz, int src, BgPlan &p) {
    if (!qtts_gemvx_shape_ok(a.R, a.C)) return 1;
    // (the 2..16-row kernels take more consumer-add columns; this one was written for the runtime's 2..4)
    if (kz > 4) return 1;
    if (a.tick && !tick_ok(a)) return 1;
    if (!a.ypart && !a.y) return 1;   // (only this kernel ever looked; no caller leaves both out)
    // tiles per workgroup: about one round of workgroups over the 256 CUs
    const int T = a.R / 16;
    const int TPW = std::max(1, std::min((T * kz + 128) / 256, 3));
    const int wreg = std::max(a.nb * QTTS_GX_LDX, TPW * 256);
    const size_t smem = ((size_t)QTTS_GX_W * wreg + (size_t)QTTS_GX_W * 64 + 64 + 4) * sizeof(float);
    if (smem > 160 * 1024) return 1;
    const dim3 grid((T + TPW - 1) / TPW, kz);
    if (a.tick && (int)grid.x > QTTS_GM_TICKS) return 1;
    p.kernel = BG_GEMVX; p.nt = 3;
    p.t[0] = (a.nb + 15) / 16; p.t[1] = TPW; p.t[2] = src;
    p.grid = grid; p.block = dim3(64 * QTTS_GX_W); p.smem = smem;
    return 0;
}

}  // namespace

bool qtts_gemvx_shape_ok(int R, int C) {
    return R >= 16 && R % 16 == 0 && C >= 32 && C % 32 == 0 && (size_t)R * C * 2 < ((size_t)1 << 31);
}

int qtts_bgemv_plan(const GemvArgs &a, BgPlan &p, unsigned allowed) {
    p = BgPlan();
    int kz = 1;
    if (!args_ok(a, kz, p.src)) return 1;
    // 17..64 rows: k_gemvx or nothing; 2..16: k_gemvb, else k_gemvm
    if (a.nb > 16) return (allowed & BG_GEMVX) ? geom_gemvx(a, kz, p.src, p) : 1;
    int rc = 1;
    if (allowed & BG_GEMVB) rc = geom_gemvb(a, kz, p.src, p);
    if (rc == 1 && (allowed & BG_GEMVM)) rc = geom_gemvm(a, kz, p.src, p);
    return rc;
}

int qtts_bgemv(const GemvArgs &a, hipStream_t st, unsigned allowed) {
#ifdef QTTS_ARGDUMP
    qtts_argdump::gemv("qtts_bgemv", a, allowed);
#endif
    BgPlan p;
    const int rc = qtts_bgemv_plan(a, p, allowed);
    if (rc) return rc;
    return p.kernel == BG_GEMVX ? qtts_gemvx_launch(a, p, st)
         : p.kernel == BG_GEMVB ? qtts_gemvb_launch(a, p, st) : qtts_gemvm_launch(a, p, st);
}
