// qtts_rt_frame.hip - which launches make up a talker step, a sub-talker pass,
// the two-row pair pass and a prefill layer; the frame graphs built from them.
// Each rule is written once -- LayerView: a layer's four projections;
// talker_attn / st_attn: the attention sites; ResidStream (qtts_dev.h): the
// residual and its pending partials; st_edge_pf: the sub-talker chain's
// next-launch prefetch -- and the callers only say which launches run.
#include "qtts_dev.h"

// ----------------------------------------------------------------- kernels of one frame
enum { PK_GEMV_TALKER = 0, PK_GEMV_SUB = 1, PK_ATTN = 2, PK_SAMPLE = 3, PK_EMBED = 4 };
struct ProfScope {  // brackets one launch with events when profiling is on
    qtts_dev *dv;
    size_t idx;
    ProfScope(qtts_dev *d, int kind, double bytes) : dv(d), idx((size_t)-1) {
        if (!dv->profiling) return;
        qtts_dev::Prof p{kind, bytes, nullptr, nullptr, ""};
        // no system-scope fence per event: a default event's cache write-back /
        // invalidate would be timed as part of every short kernel
        hipEventCreateWithFlags(&p.a, hipEventDisableSystemFence);
        hipEventCreateWithFlags(&p.b, hipEventDisableSystemFence);
        hipEventRecord(p.a, dv->st);
        dv->prof.push_back(p);
        idx = dv->prof.size() - 1;
    }
    void cancel() {
        if (idx == (size_t)-1) return;
        hipEventDestroy(dv->prof[idx].a);
        hipEventDestroy(dv->prof[idx].b);
        dv->prof.pop_back();
        idx = (size_t)-1;
    }
    ~ProfScope() {
        if (idx == (size_t)-1) return;
        hipEventRecord(dv->prof[idx].b, dv->st);
        dv->prof[idx].name = qtts_last_kernel;
    }
};
static double gemv_bytes(const GemvArgs &a) {
    return (double)a.R * a.C * 2 + (double)a.nb * a.C * 4 + (double)a.nb * a.R * 4 + (a.norm_w ? a.C * 4.0 : 0.0);
}
static int pgemv(qtts_dev *dv, const GemvArgs &a, int kind) {
    ProfScope ps(dv, kind, gemv_bytes(a));
    return qtts_gemv(a, dv->st);
}
// Multi-row projection over `rows` activation rows (prefill, text
// projection): > 64 rows in one matrix-core launch (64-row chunks on its
// grid.y), else the matrix-core kernel / batch GEMV / GEMV in chunks of 64 /
// 16.  Row r of x / y / ids is at r*ldx / r*ldy / r*ids_bstride.
int rows_proj(qtts_dev *dv, GemvArgs a, int rows, bool prefill) {
    const int xs = a.ldx, ys = a.ldy;
    // the talker prefill over > 16 rows (voice-clone prompts, long prefills):
    // activations split once, LDS-tiled MFMA GEMM (k_pgemm.hip;
    // QTTS_HIP_PGEMM=0: k_mgemm as before)
    if (prefill && dv->pgemm && rows > 16 && (!a.norm_w || rows <= dv->pinv_cap)) {
        GemvArgs c = a;
        c.nb = rows;
        const int rc = qtts_pgemm(c, dv->pinv, dv->pplanes, dv->pplanes_elems, dv->st, dv->mpart, dv->mpart_elems);
        if (rc <= 0) return rc;
    }
    if (rows > 64 && (!a.norm_w || rows <= dv->pinv_cap)) {
        GemvArgs c = a;
        c.nb = rows;
        const int rc = qtts_mgemm(c, dv->pinv, dv->st, dv->mpart, dv->mpart_elems);
        if (rc <= 0) return rc;
    }
    for (int r0 = 0; r0 < rows;) {
        GemvArgs c = a;
        int nr = rows - r0 < 64 ? rows - r0 : 64;
        if (c.x) c.x = a.x + (size_t)r0 * xs;
        if (c.ids) c.ids = a.ids + (size_t)r0 * a.ids_bstride;
        c.y = a.y + (size_t)r0 * ys;
        c.nb = nr;
        int rc = 1;
        // <= 16 rows (a custom-voice prompt): the batch decode kernels (k_gemvb,
        // x sliced per wave, else k_gemvm, x split once per workgroup; ~1
        // round over the CUs) stream the weights faster than the 64-row
        // prefill GEMM.  (QTTS_HIP_PREFILL_GEMVB=0: k_gemvm only, the round-4
        // path: 72 us of prefill per talker layer at the P128 prompt's rows,
        // profiles/r05af_first_packet.txt)
        static const bool pgb = [] { const char *e = getenv("QTTS_HIP_PREFILL_GEMVB"); return !(e && !atoi(e)); }();
        // the residual projections (O, down: R / 16 row tiles, too few for
        // the chip) split over K in two columns that reduce their own
        // partials, as the talker's decode does (QTTS_HIP_PREFILL_SPLIT=kz,
        // 2 or 4; 0: none)
        static const int psk = [] { const char *e = getenv("QTTS_HIP_PREFILL_SPLIT");
                                    int v = e ? atoi(e) : 2; return v == 4 ? 4 : v ? 2 : 0; }();
        if (nr >= 2 && nr <= 16 && pgb && psk && c.epi == EPI_RESID && !c.norm_w && c.R / 16 < 256 &&
            c.C % (32 * psk) == 0 && c.R <= (dv->d.H > dv->d.Hs ? dv->d.H : dv->d.Hs)) {
            GemvArgs k = c;
            k.ypart = dv->ppart; k.kz = psk; k.ld_ypart = (size_t)nr * k.R; k.tick = dv->btick;
            rc = qtts_bgemv(k, dv->st, BG_GEMVB);
        }
        // (never k_gemvx: above 16 rows the prefill GEMM below; the planner answers 1 outside 2..16 rows)
        if (rc == 1) rc = qtts_bgemv(c, dv->st, pgb ? BG_GEMVB | BG_GEMVM : BG_GEMVM);
        if (rc == 1 && nr >= 2) rc = qtts_mgemm(c, dv->pinv, dv->st, dv->mpart, dv->mpart_elems);
        if (rc < 0) return -1;
        if (rc == 1) {
            nr = nr < 16 ? nr : 16;
            c.nb = nr;
            CKI(qtts_gemv(c, dv->st));
        }
        r0 += nr;
    }
    return 0;
}

GemvArgs gv(const bf16_t *W, int R, int C, const float *x, int ldx, float *y, int ldy, int nb, int epi) {
    GemvArgs a;
    a.W = W; a.R = R; a.C = C; a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.nb = nb; a.epi = epi;
    return a;
}

// A layer's weights with the dims of its stack and the stack's non-temporal
// weight-load policy (the talker's decode: nt 1; its prefill and the
// sub-talker: 0).  Every q|k|v, O, gate|up and down GEMV is one of these four.
struct LayerView {
    const Layer &ly;
    int H, I, QKV, AD, nt;
    float eps;
    GemvArgs qkv(const float *x, float *y, int rows) const {   // input norm, q|k|v rows
        GemvArgs a = gv(ly.wqkv, QKV, H, x, H, y, QKV, rows, EPI_STORE);
        a.norm_w = ly.in; a.eps = eps; a.nt = nt;
        return a;
    }
    GemvArgs o(const float *att, float *x, int rows) const {   // O projection onto the residual
        GemvArgs a = gv(ly.wo, H, AD, att, AD, x, H, rows, EPI_RESID);
        return a.nt = nt, a;
    }
    GemvArgs gate_up(const float *x, float *h, int rows) const {   // post norm, gate|up, SwiGLU
        GemvArgs a = gv(ly.wgu, 2 * I, H, x, H, h, I, rows, EPI_SWIGLU);
        a.norm_w = ly.post; a.eps = eps; a.nt = nt;
        return a;
    }
    GemvArgs down(const float *h, float *x, int rows) const {   // down projection onto the residual
        GemvArgs a = gv(ly.wdown, H, I, h, I, x, H, rows, EPI_RESID);
        return a.nt = nt, a;
    }
};
static LayerView talker_view(const qtts_dev *dv, int l, int nt) {
    return LayerView{dv->tl[l], dv->d.H, dv->d.I, dv->QKV(), dv->d.NH * dv->d.HD, nt, dv->d.eps};
}
static LayerView sub_view(const qtts_dev *dv, int l) {
    return LayerView{dv->sl[l], dv->d.Hs, dv->d.Is, dv->QKVs(), dv->d.NHs * dv->d.HDs, 0, dv->d.eps};
}

// ST_PROJECT_INPUT (T.c:693-702) of every embedding row a pass g >= 1 can
// read, once at load: the per-frame input projection GEMV of those passes
// becomes a row gather (the row a pass needs is fixed by the code id alone).
int build_proj_tables(qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    const int nid = d.V > d.Vs ? d.V : d.Vs;
    std::vector<int> io(nid);
    for (int i = 0; i < nid; ++i) io[i] = i;
    int *ids = (int *)dalloc(dv, (size_t)nid * 4, false);
    dv->codec_ptab = (float *)dalloc(dv, (size_t)d.V * d.Hs * 4, true);
    dv->st_ptab = (float *)dalloc(dv, (size_t)(d.G - 1) * d.Vs * d.Hs * 4, true);
    if (!ids || !dv->codec_ptab || !dv->st_ptab) return -1;
    CK(hipMemcpy(ids, io.data(), (size_t)nid * 4, hipMemcpyHostToDevice));
    GemvArgs a;
    a.W = dv->st_proj; a.R = d.Hs; a.C = d.H; a.y = dv->codec_ptab; a.ldy = d.Hs;
    a.epi = dv->st_projb ? EPI_BIAS : EPI_STORE; a.bias = dv->st_projb; a.nt = 0;
    a.table = dv->codec_emb; a.ids = ids; a.ids_bstride = 1;
    CKI(rows_proj(dv, a, d.V));
    for (int g = 0; g < d.G - 1; ++g) {
        a.table = dv->st_emb + (size_t)g * d.Vs * d.H;
        a.y = dv->st_ptab + (size_t)g * d.Vs * d.Hs;
        CKI(rows_proj(dv, a, d.Vs));
    }
    CK(hipStreamSynchronize(dv->st));
    return 0;
}

// The layer-0 q|k|v table (qtts_dev::qkv0_tab): row r of group g's block is
// exactly what the per-frame GEMV computes for input id r (same lean kernel,
// same arguments but the output row), so reading it is bit-identical.  One
// launch per group, the ids on grid.y (GemvArgs::reps); a per-row launch for
// each of ~32k ids took ~0.2 s and crashed rocprofv3's counter collection.
int build_qkv0_table(qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    if (d.G < 2 || d.Ls < 1) return 0;
    if (d.NHs != 2 * d.KVs) return 0;   // read only by the fused attention + O kernel (qtts_attn_o_covers)
    const int QKV = dv->QKVs();
    const size_t rows = (size_t)d.V + (size_t)(d.G - 2) * d.Vs;
    const int nid = d.V > d.Vs ? d.V : d.Vs;
    std::vector<int> io(nid);
    for (int i = 0; i < nid; ++i) io[i] = i;
    int *ids = (int *)dalloc(dv, (size_t)nid * 4, true);
    dv->qkv0_tab = (float *)dalloc(dv, rows * QKV * 4, true);
    if (!ids || !dv->qkv0_tab) return -1;
    CK(hipMemcpy(ids, io.data(), (size_t)nid * 4, hipMemcpyHostToDevice));
    const bool proj = dv->st_proj != nullptr;
    for (int g = 1; g < d.G; ++g) {
        GemvArgs a = sub_view(dv, 0).qkv(nullptr, nullptr, 1);
        if (proj) a.table_f32 = g == 1 ? dv->codec_ptab : dv->st_ptab + (size_t)(g - 2) * d.Vs * d.Hs;
        else a.table = g == 1 ? dv->codec_emb : dv->st_emb + (size_t)(g - 2) * d.Vs * d.H;
        a.ids = ids; a.ids_bstride = 1;
        a.reps = g == 1 ? d.V : d.Vs;
        a.ldy_rep = QKV;
        a.y = dv->qkv0_tab + (g == 1 ? 0 : (size_t)d.V + (size_t)(g - 2) * d.Vs) * QKV;
        const int rc = qtts_gemvw(a, dv->st);
        if (rc < 0) return -1;
        if (rc == 0) continue;
        // shapes the lean kernel does not cover (small test models): the
        // per-frame path runs k_gemv1, so the table does too, one row a launch
        const int n = a.reps;
        float *base = a.y;
        a.reps = 1;
        for (int r = 0; r < n; ++r) {
            a.ids_off = r;
            a.y = base + (size_t)r * QKV;
            CKI(qtts_gemv(a, dv->st));
        }
    }
    CK(hipStreamSynchronize(dv->st));
    return 0;
}

// Batch split-K (nb >= 2, k_gemvm): the O and down projections of R rows take
// kz workgroup columns when R / 16 tiles would not fill the chip; they store
// partials, and the next GEMV that reads the residual adds them (ResidStream).
// 0 = no split.
static int bsplit_kz(const qtts_dev *dv, int R, int C) {
    if (!dv->bsplit || dv->nrun < 2) return 0;
    int kz = R / 16 >= 256 ? 1 : 256 / (R / 16);
    // (up to 8 rows the consumers add the partials: 2 columns measured +0.8 %
    // at batch 8 over 4, profiles/r03b_batch_kz_ab.txt)
    const int cap = dv->bkz_max > 0 ? dv->bkz_max : dv->nrun <= 8 ? 2 : 4;
    if (kz > cap) kz = cap;
    // above 8 rows, a column slice wider than 2048 (the 1.7B talker's down
    // projection: 6144 / 2) gives k_gemvb's waves 8 steps of 16 staged rows,
    // over the 160 KB of LDS, and the launch fell back to k_gemvm (17.5 us at
    // batch 16 against 10.1 us for batch 8's k_gemvb); more columns keep the
    // slices at <= 4 steps a wave
    if ((dv->nrun > 8 && dv->bkz_wide) || dv->bkz_wide == 2) {
        const int wcap = dv->bkz_wide == 2 ? 4 : cap;
        while (2 * kz <= wcap && C / kz > 2048 && C % (64 * kz) == 0) kz *= 2;
    }
    while (kz > 1 && C % (32 * kz)) kz /= 2;
    return kz > 1 ? kz : 0;
}

// Next-launch weight slices (L2Prefetch): what workgroup b of the NEXT launch
// reads, for the two launch shapes of the batch-1 sub-talker chain, taken from
// that launch's own GemvArgs (`next`)
//   k_gemvw (grid 256): rows [b R / 256, (b + 1) R / 256), contiguous
//   (a next launch of `grid` workgroups, 256 or 512: this launch's workgroup b
//   < 256 takes the first cap bytes of the next one's workgroup b -- b and
//   b + 256 share an XCD, so a 512 grid is half covered)
static L2Prefetch pf_gemvw(const qtts_dev *dv, const GemvArgs &next, int grid = 256) {
    L2Prefetch p;
    const int R = next.R, C = next.C;
    if (R % grid) return p;
    long long bytes = (long long)(R / grid) * C * 2;
    if (bytes > 64LL * 256 * QTTS_PF_LOADS) bytes = 64LL * 256 * QTTS_PF_LOADS;
    if (bytes % 64) return p;
    p.base = reinterpret_cast<const unsigned char *>(next.W);
    p.pa = (long long)(R / grid) * C * 2; p.pb = 0; p.chunks = (int)(bytes / 64); p.lg = 30; p.ld = 0;
    p.nwg = grid; p.sink = dv->pf_sink;
    return p;
}
#ifdef QTTS_STAMPS
#define DBG_XFIRST(a) do { const char *e_ = getenv("QTTS_HIP_DBG_XFIRST"); (a).dbg_xfirst = e_ ? atoi(e_) : 0; } while (0)
#else
#define DBG_XFIRST(a) do { } while (0)
#endif
//   k_attn_o (grid (R / RPW, KV), linear b = rb + (R / RPW) kvh): rows
//   [RPW rb, +RPW) x columns [2 HD kvh, +2 HD) of W_o [R][NH HD], `o` the O
//   projection that launch fuses
static L2Prefetch pf_attn_o(const qtts_dev *dv, const GemvArgs &o, int NH, int HD) {
    L2Prefetch p;
    const int R = o.R, W2 = 2 * HD, LPS = W2 / 8 < 8 ? W2 / 8 : 8, RPW = 256 / LPS;
    const int cpr = W2 * 2 / 64;   // 64-B chunks per row slice
    if (R % RPW || (cpr & (cpr - 1)) || cpr < 1 || RPW * cpr > 256 * QTTS_PF_LOADS) return p;
    p.base = reinterpret_cast<const unsigned char *>(o.W);
    p.pm = R / RPW; p.pa = (long long)RPW * NH * HD * 2; p.pb = W2 * 2;
    p.chunks = RPW * cpr; p.lg = __builtin_ctz(cpr); p.ld = NH * HD * 2; p.sink = dv->pf_sink;
    p.nwg = (R / RPW) * (NH / 2);   // (R / RPW) row blocks x the kv heads of a GQA-2 W_o
    return p;
}

// the flag a frame's stop readers take: a fed run's gate (k_textfeed.hip), else `stopped`
static const int *stop_rd(const qtts_dev *dv) { return dv->fed ? dv->tf_gate : dv->stopped; }

// The talker's attention of layer l over `rows` rows.  Decode: row b at
// kv_len[b], split over the keys, stopped rows skipped; at batch 1 the split
// merge moves into the O projection's prologue (defer: one dependent hand-off
// fewer per layer).  Cached (the prefill): row r of slot prow_b[r] at ppos[r].
static AttnArgs talker_attn(const qtts_dev *dv, int l, int rows, bool cached) {
    const qtts_dims_t &d = dv->d;
    const Layer &ly = dv->tl[l];
    AttnArgs t;
    t.mode = cached ? 1 : 0; t.qkv = cached ? dv->pqkv : dv->qkv; t.ld_qkv = dv->QKV();
    t.qn_w = ly.qn; t.kn_w = ly.kn; t.eps = d.eps;
    t.rope_cos = dv->rope_cos; t.rope_sin = dv->rope_sin;
    t.kc = dv->kv_layer(dv->kc, l); t.vc = dv->kv_layer(dv->vc, l); t.S = dv->S; t.kv_dtype = dv->kv_dtype;
    t.NH = d.NH; t.KV = d.KV; t.HD = d.HD; t.out = cached ? dv->patt : dv->att; t.ld_out = d.NH * d.HD; t.nrows = rows;
    if (cached) { t.pos = dv->ppos; t.row_b = dv->prow_b; return t; }
    t.pos = dv->kv_len; t.skip = stop_rd(dv);
    t.part = dv->att_part; t.cnt = dv->att_cnt; t.nsplit = dv->att_nsplit; t.lpk = dv->attn_lpk;
    t.defer = dv->attn_defer && rows == 1 && qtts_attn_defer_ok(t) && qtts_gemvw_amerge_ok(d.H, d.NH * d.HD);
    return t;
}

// one talker step over the nrun rows in x_tk; the residual it leaves: dv->tk_res
int talker_layers(qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    const int nb = dv->nrun, AD = d.NH * d.HD;
    // (the talker's O without split-K at batch 8: 142.0 / 142.6 vs 140.7 / 142.1
    // audio-s/s, within noise; its down without: 135.9 / 135.6)
    const int kzo = bsplit_kz(dv, d.H, AD), kzd = bsplit_kz(dv, d.H, d.I);
    // the talker's O / down reduce their own partials at every batch size:
    // its q|k|v and gate|up prologues (2048-wide x rows) then read x alone
    // (batch 8: 141.1 / 143.1 vs 138.9 / 141.2 audio-s/s adding the partials
    // there, same box; the sub-talker keeps the consumer add up to 8 rows,
    // where self-reduction measured slower)
    const int tk_self = 2;
    ResidStream &rs = dv->tk_res;
    rs.reset(dv->x_tk, dv->x_tk2, d.H, nb);
    for (int l = 0; l < d.L; ++l) {
        const LayerView lv = talker_view(dv, l, 1);
        const bool dbg = dv->gm_dbg && l == dv->gm_dbg_layer;
        GemvArgs a = lv.qkv(rs.xa, dv->qkv, nb);
        rs.read(a);
        const AttnArgs t = talker_attn(dv, l, nb, false);
        dv->att_own = !t.defer;
        GemvArgs o = lv.o(dv->att, rs.xa, nb);
        GemvArgs gu = lv.gate_up(rs.xa, dv->hbuf, nb);
        if (dbg) a.dbg = dv->gm_dbg;
        // (batch 1: the O projection's slices two launches ahead, the attention in between)
        if (nb == 1 && (dv->l2pf_tk & 1)) a.pf = pf_gemvw(dv, o);
        CKI(pgemv(dv, a, PK_GEMV_TALKER));
        { ProfScope ps(dv, PK_ATTN, 0); CKI(qtts_attention(t, dv->st)); }
        if (dbg) o.dbg = dv->gm_dbg + 2048 * 8;
        if (t.defer) {
            o.amerge = dv->att_part; o.am_pos = dv->kv_len; o.am_nsplit = dv->att_nsplit;
            o.am_ch = qtts_attn_keys_per_split(d.HD, true, dv->attn_lpk); o.am_hd = d.HD; o.am_gph = d.NH / d.KV;
        }
        rs.write_split(o, dv->bpo, kzo, dv->btick, tk_self);
        if (nb == 1 && (dv->l2pf_tk & 2)) o.pf = pf_gemvw(dv, gu, 512);
        CKI(pgemv(dv, o, PK_GEMV_TALKER));
        if (dbg) gu.dbg = dv->gm_dbg + 2 * 2048 * 8;
        rs.read(gu);
        CKI(pgemv(dv, gu, PK_GEMV_TALKER));
        GemvArgs dn = lv.down(dv->hbuf, rs.xa, nb);
        if (dbg) dn.dbg = dv->gm_dbg + 3 * 2048 * 8;
        rs.write_split(dn, dv->bpd, kzd, dv->btick, tk_self);
        CKI(pgemv(dv, dn, PK_GEMV_TALKER));
    }
    return 0;
}

// logit head, then the sampler
static int head_sample(qtts_dev *dv, const GemvArgs &a, const SampArgs &s, int kind) {
    CKI(pgemv(dv, a, kind));
    ProfScope ps(dv, PK_SAMPLE, 0);
    if (dv->f_armed) {   // forcing or taps armed: the forced sampler (its own frame graphs, graph_key 2)
        SampForce f;
        f.forced = dv->f_forced; f.drawn = dv->f_drawn; f.taps = dv->f_taps;
        f.tap_logits = dv->f_tap_logits; f.tap_meta = dv->f_tap_meta; f.tap_ld = dv->f_tap_ld;
        return qtts_sample_forced(s, f, dv->st);
    }
    // per-slot parameters: the per-slot sampler (its own frame graphs, graph_key 3 / 4)
    // (a fed run: the rows read the gate; nullptr otherwise -- the launches of before)
    const int *rd = dv->fed ? dv->tf_gate : nullptr;
    if (dv->sp_armed) return qtts_sample_slots(s, dv->sp_tab, !dv->sp_general, dv->st, rd);
    return qtts_sample(s, dv->st, rd);
}

// final norm + codec head on the talker's residual (dv->tk_res: what the last
// talker_layers left, or the prefill's hidden in x_tk); normed hidden ->
// tk_hid (T.c:526-530, Q.c:1295)
GemvArgs talker_head_args(qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    ResidStream &rs = dv->tk_res;
    GemvArgs a = gv(dv->head, d.V, d.H, rs.xa ? rs.xa : dv->x_tk, d.H, dv->logits, d.V, dv->nrun, EPI_STORE);
    a.norm_w = dv->tk_norm; a.eps = d.eps; a.xcopy = dv->tk_hid; a.ldxc = d.H; a.xcopy_normed = 1;
    rs.read(a, false);
    return a;
}
int talker_tail(qtts_dev *dv) { return pgemv(dv, talker_head_args(dv), PK_GEMV_TALKER); }

// codec head, then the group-0 draw with suppression / repetition penalty / EOS rules
static int talker_head_sample(qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    const GemvArgs a = talker_head_args(dv);
    SampArgs s;
    s.logits = dv->logits; s.ld = d.V; s.n = d.V; s.nb = dv->nrun;
    s.top_k = dv->par.top_k; s.top_p = dv->par.top_p; s.temp = dv->par.temperature;
    s.rng = dv->rng; s.mode = 1; s.suppress_lo = d.V - 1024; s.eos = d.eos_id;
    s.rep = dv->par.repetition_penalty; s.counts = dv->counts; s.fixed = dv->par.fixed_codec_tokens;
    s.n_gen = dv->n_gen; s.stopped = dv->stopped; s.cur_row = dv->cur_row; s.stop_step = dv->stop_step;
    s.host_stopped = dv->hstop;
    s.st_rng = dv->st_rng; s.seed_bits = seed_bits(dv->par.seed);
    s.codes = dv->codes; s.codes_bstride = (dv->max_frames + 1) * d.G; s.G = d.G; s.out_tok = dv->last_tok;
    return head_sample(dv, a, s, PK_GEMV_TALKER);
}

// What the layers of a sub-talker pass share.  The generic chain runs pass g at
// position g over the nrun rows; the pair pass (batch 1) runs positions 0 and
// 1 as two rows and stands for pass 1, whose head follows it.
struct StPass {
    int g = 0, rows = 1;   // the pass (its head and prefetch edges; generic chain: its position), residual rows
    bool pair = false;     // the two-row pair pass (k_stpair.hip)
    bool direct = false;   // layer 0 reads `src` itself: no input projection, or the projected row is a table row
    GemvArgs src;          // the input rows of the pass (x / table description only)
    ResidStream rs;
};
static StPass st_pass(const qtts_dev *dv, int g, bool pair = false) {
    const qtts_dims_t &d = dv->d;
    const bool proj = dv->st_proj != nullptr;
    // passes >= 1 of a projecting model gather their already-projected row
    const bool ptab = proj && g >= 1 && dv->st_ptab;
    StPass P;
    P.g = g; P.pair = pair; P.rows = pair ? 2 : dv->nrun; P.direct = !proj || ptab;
    if (g == 0) { P.src.x = dv->tk_hid; P.src.ldx = d.H; }
    else {
        if (ptab) P.src.table_f32 = g == 1 ? dv->codec_ptab : dv->st_ptab + (size_t)(g - 2) * d.Vs * d.Hs;
        else P.src.table = g == 1 ? dv->codec_emb : dv->st_emb + (size_t)(g - 2) * d.Vs * d.H;
        // the previous draw's id (group g - 1: the talker's for g = 1)
        P.src.ids = dv->last_tok; P.src.ids_bstride = 1; P.src.row_sel = nullptr; P.src.ids_rstride = 0; P.src.ids_off = 0;
    }
    P.rs.reset(dv->x_st, dv->x_st2, d.Hs, P.rows);
    return P;
}
static void set_src(GemvArgs &a, const GemvArgs &src) {
    a.x = src.x; a.ldx = src.ldx; a.table = src.table; a.table_f32 = src.table_f32; a.ids = src.ids;
    a.ids_bstride = src.ids_bstride; a.row_sel = src.row_sel; a.ids_rstride = src.ids_rstride; a.ids_off = src.ids_off;
}
// pass 0 produces no logits: its last layer only has to store its k / v
// (ST_FORWARD of pass 1 restarts from its own input, T.c:704-714)
static bool st_kv_only(const qtts_dev *dv, const StPass &P, int l) { return P.g == 0 && l == dv->d.Ls - 1; }
// QTTS_HIP_GM_DBG=99: stamps of pass 5, layer 2's q|k|v / (batch: O) / gate|up / down;
// =98: of the pair pass, layer 2's q|k|v / attention + O / gate|up / down
static bool st_dbg(const qtts_dev *dv, const StPass &P, int l) {
    return dv->gm_dbg && l == 2 && (P.pair ? dv->gm_dbg_layer == 98 : dv->gm_dbg_layer == 99 && P.g == 5);
}
static int pgemv_pair(qtts_dev *dv, const GemvArgs &a) {
    ProfScope ps(dv, PK_GEMV_SUB, gemv_bytes(a));
    if (qtts_gemvw_pair(a, dv->st) != 0) {
        fprintf(stderr, "qtts: pair GEMV launch failed (R=%d C=%d)\n", a.R, a.C);
        return -1;
    }
    return 0;
}
static int st_gemv(qtts_dev *dv, const StPass &P, const GemvArgs &a) {
    return P.pair ? pgemv_pair(dv, a) : pgemv(dv, a, PK_GEMV_SUB);
}
static void st_stamp(const qtts_dev *dv, const StPass &P, GemvArgs &a, int slot) {   // the debug stamps' slot 0..3
    a.dbg = dv->gm_dbg + slot * 2048 * 8;
    if (!P.pair) DBG_XFIRST(a);
}
// pass g's lm head on residual rows x (no residual: the prefetch target only)
static GemvArgs st_head_args(const qtts_dev *dv, int g, const float *x) {
    const qtts_dims_t &d = dv->d;
    GemvArgs a = gv(dv->lm + (size_t)(g - 1) * d.Vs * d.Hs, d.Vs, d.Hs, x, d.Hs, dv->logits_s, d.Vs, dv->nrun, EPI_STORE);
    a.norm_w = dv->st_norm; a.eps = d.eps; a.nt = 0;
    return a;
}

// Batch 1, fused attention + O: each launch of the sub-talker chain also pulls
// the next launch's weight slice into its XCD's L2 (GemvArgs::pf /
// AttnArgs::pf).  The edge `bit` (QTTS_HIP_L2PF) leaving a launch of layer l,
// pass g: 1 q|k|v -> attention + O, 2 attention + O -> gate|up (pass 0's last
// layer stops there: -> the next pass's first launch), 4 gate|up -> down,
// 8 down -> the next layer's q|k|v or the pass's head, 16 head -> the next
// pass's first launch (two launches ahead: the sampler runs in between).
static L2Prefetch st_edge_pf(const qtts_dev *dv, int bit, int l, int g) {
    const qtts_dims_t &d = dv->d;
    const int pfm = dv->nrun == 1 && dv->attn_o ? dv->l2pf : 0;
    if (!(pfm & bit)) return L2Prefetch();
    const LayerView lv = sub_view(dv, l);
    auto first_of = [&](int gn) {   // pass gn's first launch (layer 0: the table attention or q|k|v)
        const bool tab0_ok = dv->qkv0_tab && (!dv->st_proj || dv->st_ptab);
        if (gn >= d.G) return L2Prefetch();
        if (gn >= 1 && tab0_ok) return pf_attn_o(dv, sub_view(dv, 0).o(nullptr, nullptr, 1), d.NHs, d.HDs);
        return pf_gemvw(dv, sub_view(dv, 0).qkv(nullptr, nullptr, 1));
    };
    switch (bit) {
    case 1: return pf_attn_o(dv, lv.o(nullptr, nullptr, 1), d.NHs, d.HDs);
    case 2: return g == 0 && l == d.Ls - 1 ? first_of(1) : pf_gemvw(dv, lv.gate_up(nullptr, nullptr, 1));
    case 4: return pf_gemvw(dv, lv.down(nullptr, nullptr, 1));
    case 8:
        if (l + 1 < d.Ls) return pf_gemvw(dv, sub_view(dv, l + 1).qkv(nullptr, nullptr, 1));
        return g >= 1 ? pf_gemvw(dv, st_head_args(dv, g, nullptr)) : L2Prefetch();
    case 16: return first_of(g + 1);
    }
    return L2Prefetch();
}
// layer 0 of a pass g >= 1: q|k|v come from the load-time table by the pass's
// input id (no GEMV); xc_dst: the kernel also copies the input row there (the
// residual the skipped GEMV would have copied)
static void st_tab_rows(const qtts_dev *dv, AttnArgs &t, const StPass &P, float *xc_dst) {
    const qtts_dims_t &d = dv->d;
    t.qkv_tab = dv->qkv0_tab + (P.g == 1 ? 0 : (size_t)d.V + (size_t)(P.g - 2) * d.Vs) * dv->QKVs();
    t.tab_ids = P.src.ids; t.tab_bstride = P.src.ids_bstride; t.tab_row_sel = P.src.row_sel;
    t.tab_rstride = P.src.ids_rstride; t.tab_off = P.src.ids_off;
    if (xc_dst) { t.xc_tab = P.src.table_f32; t.xc_tab16 = P.src.table; t.xc_dst = xc_dst; t.xc_n = d.Hs; }
}
// The sub-talker's attention of layer l of pass P over its rows of qkv_s, with
// its prefetch edge and stamps (the pair kernel has no attention output of its own and no
// tickets; its row 1 takes layer 0's q|k|v from the table, its input row goes to the residual's row 1)
static AttnArgs st_attn(const qtts_dev *dv, const StPass &P, int l) {
    const qtts_dims_t &d = dv->d;
    const Layer &ly = dv->sl[l];
    const size_t slice = (size_t)l * dv->nb * d.G * d.KVs * d.HDs;
    AttnArgs t;
    t.mode = 0; t.qkv = dv->qkv_s; t.ld_qkv = dv->QKVs(); t.qn_w = ly.qn; t.kn_w = ly.kn; t.eps = d.eps;
    t.rope_cos = dv->rope_cos_s; t.rope_sin = dv->rope_sin_s;
    t.kc = dv->kcs + slice; t.vc = dv->vcs + slice; t.S = d.G;
    t.pos = nullptr; t.pos_const = P.pair ? 0 : P.g; t.NH = d.NHs; t.KV = d.KVs; t.HD = d.HDs; t.ld_out = d.NHs * d.HDs;
    t.nrows = P.rows; t.skip = stop_rd(dv);
    if (!P.pair) { t.out = dv->att_s; t.cnt = dv->att_cnt; }
    else if (l == 0) st_tab_rows(dv, t, P, dv->x_st + d.Hs);
    t.pf = st_edge_pf(dv, 2, l, P.g);
#ifdef QTTS_STAMPS
    if (st_dbg(dv, P, l)) t.dbg = dv->gm_dbg + 2048 * 8;   // (batch 1: the attention + O launch in the "O / -" slot)
#endif
    return t;
}
// ST_PROJECT_INPUT (T.c:693-702) of the pass's input rows into x_st
static int st_project(qtts_dev *dv, const StPass &P) {
    const qtts_dims_t &d = dv->d;
    GemvArgs a = gv(dv->st_proj, d.Hs, d.H, nullptr, 0, dv->x_st, d.Hs, dv->nrun, dv->st_projb ? EPI_BIAS : EPI_STORE);
    set_src(a, P.src);
    a.bias = dv->st_projb; a.nt = 0;
    return pgemv(dv, a, PK_GEMV_SUB);
}
// layer l's q|k|v GEMV over the pass's rows (launched or not, it is what reads the residual here)
static GemvArgs st_qkv_args(qtts_dev *dv, StPass &P, int l) {
    GemvArgs a = sub_view(dv, l).qkv(P.rs.xa, dv->qkv_s, P.rows);
    if (st_dbg(dv, P, l)) st_stamp(dv, P, a, 0);
    if (l == 0 && P.direct && !P.pair) { set_src(a, P.src); a.xcopy = dv->x_st; a.ldxc = dv->d.Hs; a.xcopy_normed = 0; }
    else P.rs.read(a);
    a.pf = st_edge_pf(dv, 1, l, P.g);
    return a;
}
// gate|up (it adds what is pending on the residual), then down; x_is_src: the
// residual is the pass's input table row itself (x_st was not written)
static int st_mlp(qtts_dev *dv, StPass &P, int l, bool x_is_src) {
    const qtts_dims_t &d = dv->d;
    const bool sdbg = st_dbg(dv, P, l);
    const LayerView lv = sub_view(dv, l);
    GemvArgs a = lv.gate_up(P.rs.xa, dv->h_s, P.rows);
    a.pf = st_edge_pf(dv, 4, l, P.g);
    if (sdbg) st_stamp(dv, P, a, 2);
    if (x_is_src) set_src(a, P.src);
    P.rs.read(a);
    CKI(st_gemv(dv, P, a));
    // (the pair pass: row 0 in the last layer needs only its k / v store; its MLP rides along)
    a = lv.down(dv->h_s, P.rs.xa, P.rows);
    a.pf = st_edge_pf(dv, 8, l, P.g);
    if (sdbg) st_stamp(dv, P, a, 3);
    P.rs.write_split(a, dv->bpd, bsplit_kz(dv, d.Hs, d.Is), dv->btick, dv->bself_min);
    return st_gemv(dv, P, a);
}
// the attention kernel, then the O projection onto the residual (batch: split
// over K, the partials added by the next residual reader or by its own last column)
static int st_attn_then_o(qtts_dev *dv, StPass &P, int l, const AttnArgs &t, unsigned long long *odbg) {
    const qtts_dims_t &d = dv->d;
    { ProfScope pa(dv, PK_ATTN, 0); CKI(qtts_attention(t, dv->st)); }
    if (st_kv_only(dv, P, l)) return 0;
    GemvArgs o = sub_view(dv, l).o(dv->att_s, P.rs.xa, P.rows);
    P.rs.write_split(o, dv->bpo, bsplit_kz(dv, d.Hs, d.NHs * d.HDs), dv->btick, dv->bself_min);
    if (odbg) o.dbg = odbg;
    return pgemv(dv, o, PK_GEMV_SUB);
}

// A layer of the lock-step form (batch >= 2, or QTTS_HIP_ATTN_O=0): q|k|v GEMV
// (pass g >= 1, layer 0 at batch >= 2: the load-time table through the short
// attention kernel, which also copies the input row to the residual),
// attention, O with optional split-K, MLP.  (At batch 8 / 16 the fused form
// measured slower, 98 vs 107 / 132 vs 155 audio-s/s, profiles/r01av_bench_batch_attn_o.txt)
static int st_layer_lockstep(qtts_dev *dv, StPass &P, int l) {
    const qtts_dims_t &d = dv->d;
    const GemvArgs a = st_qkv_args(dv, P, l);
    AttnArgs t = st_attn(dv, P, l);
    const bool hd_ok = d.HDs == 128 || d.HDs == 64 || d.HDs == 32 || d.HDs == 16;
    const bool tab0b = l == 0 && P.g >= 1 && P.rows >= 2 && dv->tab0b && dv->qkv0_tab && P.direct &&
                       d.NHs == 2 * d.KVs && d.G <= 16 && hd_ok;
    if (tab0b) st_tab_rows(dv, t, P, P.rs.xa);
    if (!tab0b) CKI(pgemv(dv, a, PK_GEMV_SUB));
    CKI(st_attn_then_o(dv, P, l, t, st_dbg(dv, P, l) ? dv->gm_dbg + 2048 * 8 : nullptr));
    return st_kv_only(dv, P, l) ? 0 : st_mlp(dv, P, l, false);
}

// A layer of the batch-1 fused form: q|k|v GEMV (pass g >= 1, layer 0: the
// load-time table instead, and gate|up reads the residual from the input table
// row itself), then attention + O by kv head into per-head partials
// (qtts_attn_o), which gate|up sums with the residual in its prologue.  The
// table only where the fused kernel runs: it alone reads it, and the skipped
// GEMV is also what copies the residual.  A shape the fused kernel does not
// cover goes on through the lock-step form's attention + O.
static int st_layer_fused(qtts_dev *dv, StPass &P, int l) {
    const qtts_dims_t &d = dv->d;
    const GemvArgs a = st_qkv_args(dv, P, l);
    const GemvArgs o = sub_view(dv, l).o(dv->att_s, P.rs.xa, P.rows);
    AttnArgs t = st_attn(dv, P, l);
    const bool tab0 = l == 0 && P.g >= 1 && dv->qkv0_tab && P.direct && qtts_attn_o_covers(t, o.W);
    if (tab0) st_tab_rows(dv, t, P, nullptr);
    if (!tab0) CKI(pgemv(dv, a, PK_GEMV_SUB));
    int rc;
    {
        ProfScope ps(dv, PK_ATTN, (double)o.R * o.C * 2);
        rc = qtts_attn_o(t, o.W, o.R, dv->opart, dv->st);
        if (rc) ps.cancel();
    }
    if (rc < 0) return -1;
    if (rc == 0) P.rs.hold(dv->opart, d.KVs);
    else CKI(st_attn_then_o(dv, P, l, t, nullptr));   // not covered
    return st_kv_only(dv, P, l) ? 0 : st_mlp(dv, P, l, tab0);
}
// pass g's lm head on the residual (row x of it), then its sampler
static int st_head_sample(qtts_dev *dv, StPass &P, const float *x) {
    const qtts_dims_t &d = dv->d;
    GemvArgs a = st_head_args(dv, P.g, x);
    P.rs.read(a, false);
    a.pf = st_edge_pf(dv, 16, 0, P.g);
    SampArgs s;
    s.logits = dv->logits_s; s.ld = d.Vs; s.n = d.Vs; s.nb = dv->nrun;
    s.top_k = dv->par.st_top_k; s.top_p = dv->par.st_top_p; s.temp = dv->par.st_temperature;
    s.mode = 0; s.st_rng = dv->st_rng; s.stopped = dv->stopped; s.cur_row = dv->cur_row;
    s.codes = dv->codes; s.codes_bstride = (dv->max_frames + 1) * d.G; s.G = d.G; s.g = P.g; s.out_tok = dv->last_tok;
    return head_sample(dv, a, s, PK_GEMV_SUB);
}

// Batch 1: passes 0 and 1 as one two-row pass (k_stpair.hip).  Pass 0's input
// is the talker hidden and pass 1's the table row of the talker's draw
// (last_tok, written by the talker's sampler before the sub-talker's first
// launch), so both rows are known up front: positions 0 and 1 are a causal
// two-token prefill, every matrix is read once for both, and per row the
// arithmetic is the single-row kernels' (bit-identical codes).
// pair passes enqueued (or captured) since the library loaded: a test's proof
// that the pair path, not the 16-pass chain, ran
static std::atomic<long long> g_st_pair_passes{0};
extern "C" long long qtts_hip_st_pair_passes(void) { return g_st_pair_passes.load(); }
// where today's fast path runs (fused attention + O, the layer-0 q|k|v table)
// and the pair kernels cover every shape; everything else keeps the 16 passes
static bool st_pair_ok(const qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    if (!dv->st_pair || dv->nrun != 1 || !dv->attn_o || !dv->qkv0_tab || d.G < 2 || d.Ls < 1) return false;
    if (dv->st_proj && !(dv->st_ptab && dv->codec_ptab)) return false;
    if (!dv->st_proj && d.H != d.Hs) return false;
    const LayerView lv = sub_view(dv, 0);
    for (const GemvArgs &a : {lv.qkv(nullptr, nullptr, 2), lv.gate_up(nullptr, nullptr, 2), lv.down(nullptr, nullptr, 2)})
        if (!qtts_gemvw_pair_covers(a.R, a.C, a.epi)) return false;
    const StPass P = st_pass(dv, 1, true);
    for (int l = 0; l < d.Ls; ++l)
        if (!qtts_attn_o_pair_covers(st_attn(dv, P, l), sub_view(dv, l).o(nullptr, nullptr, 2).W)) return false;
    return true;
}
// passes 0 and 1: row 0's input projection and layer-0 q|k|v are pass 0's own single-row
// launches (row 1's come from the tables), then the layers on both rows, then pass 1's head on row 1
static int subtalker_pair(qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    StPass P0 = st_pass(dv, 0), P = st_pass(dv, 1, true);
    if (!P0.direct) CKI(st_project(dv, P0));
    CKI(pgemv(dv, st_qkv_args(dv, P0, 0), PK_GEMV_SUB));
    for (int l = 0; l < d.Ls; ++l) {
        if (l > 0) CKI(pgemv_pair(dv, st_qkv_args(dv, P, l)));
        const GemvArgs o = sub_view(dv, l).o(nullptr, nullptr, 2);
        const AttnArgs t = st_attn(dv, P, l);
        {
            ProfScope ps(dv, PK_ATTN, (double)o.R * o.C * 2);
            if (qtts_attn_o_pair(t, o.W, o.R, dv->opart, dv->st) != 0) {
                fprintf(stderr, "qtts: pair attention + O launch failed (layer %d)\n", l);
                return -1;
            }
        }
        // gate|up: residual + the per-head O partials of both rows, the new residual to the other buffer
        P.rs.hold(dv->opart, d.KVs);
        CKI(st_mlp(dv, P, l, false));
    }
    g_st_pair_passes.fetch_add(1);
    return st_head_sample(dv, P, P.rs.xa + d.Hs);
}

// 16 sub-talker passes (T.c:539-736): the pair pass where it is covered, then
// per pass its input source, the input projection unless the projected row is a
// table row, the layers in the batch-1 fused or the lock-step form, and the head
int subtalker(qtts_dev *dv) {
    const qtts_dims_t &d = dv->d;
    const bool fused = dv->attn_o && dv->nrun == 1;
    const bool pair = st_pair_ok(dv);
    if (pair) CKI(subtalker_pair(dv));
    for (int g = pair ? 2 : 0; g < d.G; ++g) {
        StPass P = st_pass(dv, g);
        if (!P.direct) CKI(st_project(dv, P));
        for (int l = 0; l < d.Ls; ++l) CKI(fused ? st_layer_fused(dv, P, l) : st_layer_lockstep(dv, P, l));
        if (g == 0) continue;  // pass 0 produces no logits
        CKI(st_head_sample(dv, P, P.rs.xa));
    }
    return 0;
}

static int embed_sum(qtts_dev *dv, int advance) {
    const qtts_dims_t &d = dv->d;
    EmbedSumArgs e;
    e.codes = dv->codes; e.codes_bstride = (dv->max_frames + 1) * d.G; e.G = d.G;
    e.cur_row = dv->cur_row; e.stopped = stop_rd(dv); e.codec_emb = dv->codec_emb; e.st_emb = dv->st_emb;
    e.Vs = d.Vs; e.H = d.H; e.nb = dv->nrun; e.trailing = dv->trailing; e.tr_cap = dv->tr_cap;
    e.n_trailing = dv->n_trailing; e.pad = dv->pad_emb; e.out = dv->x_tk; e.kv_len = dv->kv_len; e.advance = advance;
    ProfScope ps(dv, PK_EMBED, 0);
    return qtts_embed_sum(e, dv->st);
}

int record_frame(qtts_dev *dv, bool with_talker) {
    // step 0 starts from the prefill's hidden in x_tk (no pending partials)
    dv->tk_res.reset(dv->x_tk, dv->x_tk2, dv->d.H, dv->nrun);
    TextGateArgs tg;
    if (dv->fed) {   // the gate first; a talker step updates x_tk in place, so a held slot's row is saved
        tg.stopped = dv->stopped; tg.text_open = dv->tf_open; tg.n_gen = dv->n_gen; tg.n_trailing = dv->n_trailing;
        tg.gate = dv->tf_gate; tg.held = dv->tf_held; tg.x = dv->x_tk; tg.x_save = with_talker ? dv->tf_xsave : nullptr;
        tg.H = dv->d.H; tg.nb = dv->nrun;
        ProfScope ps(dv, PK_EMBED, 0);
        CKI(qtts_text_gate(tg, dv->st));
    }
    if (with_talker) CKI(talker_layers(dv));
    CKI(talker_head_sample(dv));
    CKI(subtalker(dv));
    CKI(embed_sum(dv, with_talker ? 1 : 0));
    if (dv->fed && with_talker) {
        ProfScope ps(dv, PK_EMBED, 0);
        CKI(qtts_text_restore(tg, dv->st));
    }
    return 0;
}

int capture(qtts_dev *dv, bool with_talker, hipGraphExec_t *out) {
    hipGraph_t g = nullptr;
    CK(hipStreamBeginCapture(dv->st, hipStreamCaptureModeThreadLocal));
    int rc = record_frame(dv, with_talker);
    hipError_t e = hipStreamEndCapture(dv->st, &g);
    if (rc || e != hipSuccess) {
        fprintf(stderr, "qtts: frame graph capture failed\n");
        if (g) hipGraphDestroy(g);
        return -1;
    }
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    CK(e);
    return 0;
}

// One graph for step 0 (no talker) and one for every later frame, its talker
// attention grid sized from the KV capacity (splits past the live length exit
// at once).  Graphs per power-of-two bucket of the live key count measured no
// faster, also in EOS mode (4096-frame capacity, 65 splits): 31.0 / 31.3 vs
// 31.1 / 30.5 audio-s/s (profiles/r03c_eos_ab.txt).
int ensure_graphs(qtts_dev *dv) {
    // (the forced sampler's frame is another graph, and so is each per-slot family's)
    // (a fed run's frames, with the gate node, are graphs of their own: + 8)
    const int want = (dv->f_armed ? 2 : dv->sp_armed ? (dv->sp_general ? 4 : 3) : 1) + (dv->fed ? 8 : 0);
    if (dv->g0 && dv->gN && dv->graph_key == want) return 0;
    // (mid-run: a refill admitted the run's first row that needs the full path)
    if (dv->f_phase == 2 && (dv->g0 || dv->gN)) CK(hipStreamSynchronize(dv->st));
    if (dv->g0) { hipGraphExecDestroy(dv->g0); dv->g0 = nullptr; }
    if (dv->gN) { hipGraphExecDestroy(dv->gN); dv->gN = nullptr; }
    drop_row_graphs(dv);
    if (getenv("QTTS_HIP_NO_GRAPH")) { dv->graph_key = 0; return 0; }
    // (the two main graphs always cover every slot)
    const int nrun = dv->nrun;
    dv->nrun = dv->nb;
    int rc = capture(dv, false, &dv->g0);
    if (!rc) rc = capture(dv, true, &dv->gN);
    dv->nrun = nrun;
    CKI(rc);
    dv->graph_key = want;
    return 0;
}

static std::atomic<long long> g_prefill_rows{0};
extern "C" long long qtts_hip_prefill_rows(void) { return g_prefill_rows.load(); }

// talker prefill (T.c:254-472) of prompt rows [first[i], nrows[i]) of slots[i]
// at their own positions (first NULL: from row 0); the rows before them are in
// the cache already: mode-1 attention reads every key back from it.
// last[i] = the row index (in px) of slot i's last row
int prefill_rows(qtts_dev *dv, const std::vector<int> &slots, const std::vector<int> &nrows, std::vector<int> &last,
                 const std::vector<int> *first) {
    const qtts_dims_t &d = dv->d;
    hipStream_t st = dv->st;
    std::vector<int> rb, pp, src;
    last.assign(slots.size(), 0);
    for (size_t i = 0; i < slots.size(); ++i) {
        const int b = slots[i];
        for (int t = first ? (*first)[i] : 0; t < nrows[i]; ++t) {
            rb.push_back(b);
            pp.push_back(t);
            src.push_back(b * dv->p_cap + t);
        }
        last[i] = (int)rb.size() - 1;
    }
    const int R = (int)rb.size();
    if (R < 1 || R > dv->rows_cap) return -1;
    g_prefill_rows += R;
    CK(hipMemcpyAsync(dv->prow_b, rb.data(), R * 4, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(dv->ppos, pp.data(), R * 4, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(dv->psrc, src.data(), R * 4, hipMemcpyHostToDevice, st));
    CKI(qtts_copy_rows(dv->px, d.H, dv->prefill, d.H, dv->psrc, R, d.H, st));
    for (int l = 0; l < d.L; ++l) {
        const LayerView lv = talker_view(dv, l, 0);
        CKI(rows_proj(dv, lv.qkv(dv->px, dv->pqkv, 1), R, true));
        const AttnArgs t = talker_attn(dv, l, R, true);
        CKI(qtts_qk_prep(t, st));
        CKI(qtts_attention(t, st));
        CKI(rows_proj(dv, lv.o(dv->patt, dv->px, 1), R, true));
        CKI(rows_proj(dv, lv.gate_up(dv->px, dv->ph, 1), R, true));
        CKI(rows_proj(dv, lv.down(dv->ph, dv->px, 1), R, true));
    }
    return 0;
}

// One frame run eagerly with an event pair around every kernel launch on the
// context stream; returns the number of kernels, fills kind/bytes/ms.
extern "C" int qtts_dev_profile_frame(qtts_dev_t *dv, int step, int max, int *kind, double *bytes, float *ms,
                                      char *names) {
    if (!dv || dv->nb < 1) return -1;
    hipSetDevice(dv->device);
    CK(hipStreamSynchronize(dv->st));
    dv->prof.clear();
    dv->profiling = true;
    int rc = record_frame(dv, step > 0);
    dv->profiling = false;
    CK(hipStreamSynchronize(dv->st));
    int n = 0;
    for (auto &p : dv->prof) {
        float t = 0.f;
        hipEventElapsedTime(&t, p.a, p.b);
        if (n < max) {
            kind[n] = p.kind; bytes[n] = p.bytes; ms[n] = t;
            if (names) snprintf(names + (size_t)n * 64, 64, "%s", p.name ? p.name : "");
        }
        ++n;
        hipEventDestroy(p.a);
        hipEventDestroy(p.b);
    }
    dv->prof.clear();
    return rc ? -1 : n;
}
