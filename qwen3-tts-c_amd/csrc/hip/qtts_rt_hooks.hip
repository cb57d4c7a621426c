// qtts_rt_hooks.hip - the kernel-level C-ABI of include/qtts_hip.h
// (qtts_hip_*): single kernels and dispatchers on caller-given device
// pointers, for tests and measurements.  None takes a qtts_dev.
#include "qtts_dev.h"

// ----------------------------------------------------------------- kernel-level C-ABI
extern "C" int qtts_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int qtts_hip_sync(void) { return hipDeviceSynchronize() == hipSuccess ? 0 : -1; }

// batch >= 2 goes to the matrix-core kernel (as prefill does), else the GEMV
static int matvec_any(const GemvArgs &a, hipStream_t st) {
    static float *inv = nullptr;   // per-row 1/rms scratch of this test-level entry
    if (a.nb >= 2) {
        if (!inv && hipMalloc(&inv, 64 * sizeof(float)) != hipSuccess) return -1;
        const int rc = qtts_mgemm(a, inv, st);
        if (rc != 1) return rc;
    }
    return qtts_gemv(a, st);
}

extern "C" int qtts_hip_matvec_bf16(float *out, const uint16_t *A, const float *x, int rows, int cols, int batch,
                                    void *stream) {
    GemvArgs a = gv(A, rows, cols, x, cols, out, rows, batch, EPI_STORE);
    return matvec_any(a, (hipStream_t)stream);
}

extern "C" int qtts_hip_rmsnorm_matvec_bf16(float *out, const uint16_t *A, const float *x, const float *w, float eps,
                                            int rows, int cols, int batch, void *stream) {
    GemvArgs a = gv(A, rows, cols, x, cols, out, rows, batch, EPI_STORE);
    a.norm_w = w; a.eps = eps;
    return matvec_any(a, (hipStream_t)stream);
}

// the decode dispatcher itself (qtts_gemv): batch 1 -> k_gemvw / k_gemv1;
// 2..16 -> the batch GEMV's plan (qtts_bgemv: k_gemvb, else k_gemvm, on the
// matrix cores) where it covers the shape, else k_gemv; 17..64 -> k_gemvx or -1
extern "C" int qtts_hip_decode_matvec_bf16(float *out, const uint16_t *A, const float *x, const float *w, float eps,
                                           int rows, int cols, int batch, void *stream) {
    GemvArgs a = gv(A, rows, cols, x, cols, out, rows, batch, EPI_STORE);
    a.norm_w = w; a.eps = eps;
    return qtts_gemv(a, (hipStream_t)stream);
}

extern "C" int qtts_hip_resident_matvec_bf16(float *out, const uint16_t *A, const float *x, const float *w, float eps,
                                             int rows, int cols, int epi, void *stream) {
    if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU) return -1;
    GemvArgs a = gv(A, rows, cols, x, cols, out, epi == EPI_SWIGLU ? rows / 2 : rows, 1, epi);
    a.norm_w = w; a.eps = eps; a.nt = 0;
    return qtts_gemv(a, (hipStream_t)stream);
}

extern "C" int qtts_hip_sample_top_k(int *out, const float *logits, int vocab, int top_k, float top_p, float temp,
                                     uint32_t *rng_bits, int batch, void *stream) {
    SampArgs s;
    s.logits = logits; s.ld = vocab; s.n = vocab; s.nb = batch; s.top_k = top_k; s.top_p = top_p; s.temp = temp;
    s.mode = 0; s.st_rng = rng_bits; s.out_tok = out;
    return qtts_sample(s, (hipStream_t)stream);
}

// qtts_hip_sample_top_k with one parameter set per row: the table is built
// here, the launch family is the one a run with these rows would capture
extern "C" int qtts_hip_sample_top_k_rows(int *out, const float *logits, int vocab, const int *top_k,
                                          const float *top_p, const float *temp, uint32_t *rng_bits, int batch,
                                          void *stream) {
    if (!out || !logits || !top_k || !top_p || !temp || !rng_bits || batch < 1 || batch > 65535) return -1;
    std::vector<SampSlotRow> h((size_t)batch);
    bool all_fast = true;
    for (int b = 0; b < batch; ++b) {
        if (!std::isfinite(top_p[b]) || !std::isfinite(temp[b]) || top_p[b] <= 0.0f) {
            fprintf(stderr, "qtts_hip_sample_top_k_rows: row %d: top_p %g, temperature %g\n", b, top_p[b], temp[b]);
            return -1;
        }
        SampSlotRow &r = h[b];
        r.temp = r.st_temp = temp[b]; r.top_p = r.st_top_p = top_p[b]; r.top_k = r.st_top_k = top_k[b];
        r.rep = 1.0f; r.seed_bits = 0;
        all_fast = all_fast && qtts_sample_row_fast(r, 0, vocab);
    }
    hipStream_t st = (hipStream_t)stream;
    SampSlotRow *t = nullptr;
    CK(hipMalloc((void **)&t, h.size() * sizeof(SampSlotRow)));
    int rc = hipMemcpyAsync(t, h.data(), h.size() * sizeof(SampSlotRow), hipMemcpyHostToDevice, st) == hipSuccess ? 0 : -1;
    if (!rc) {
        SampArgs s;
        s.logits = logits; s.ld = vocab; s.n = vocab; s.nb = batch;
        s.mode = 0; s.st_rng = rng_bits; s.out_tok = out;
        rc = qtts_sample_slots(s, t, all_fast, st);
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;   // (h and t live until the launch finished)
    hipFree(t);
    return rc;
}

// the nucleus short-list kernels (k_sample_n.hip) with the path each row took
static bool nucleus_params_ok(const char *who, int b, float top_p, float temp) {
    if (std::isfinite(top_p) && std::isfinite(temp) && top_p > 0.0f) return true;
    fprintf(stderr, "%s: row %d: top_p %g, temperature %g\n", who, b, top_p, temp);
    return false;
}

extern "C" int qtts_hip_sample_nucleus(int *out, const float *logits, int vocab, int top_k, float top_p, float temp,
                                       uint32_t *rng_bits, int batch, void *stream, int *path) {
    if (!out || !logits || !rng_bits || batch < 1 || batch > 65535 || vocab < 1 || vocab > 4096) return -1;
    if (!nucleus_params_ok("qtts_hip_sample_nucleus", 0, top_p, temp)) return -1;
    SampArgs s;
    s.logits = logits; s.ld = vocab; s.n = vocab; s.nb = batch; s.top_k = top_k; s.top_p = top_p; s.temp = temp;
    s.mode = 0; s.st_rng = rng_bits; s.out_tok = out;
    hipStream_t st = (hipStream_t)stream;
    int rc = qtts_sample_n(s, st, nullptr, path, qtts_sample_nucleus_on());
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    return rc;
}

extern "C" int qtts_hip_sample_nucleus_rows(int *out, int *path, const float *logits, int vocab, const int *top_k,
                                            const float *top_p, const float *temp, uint32_t *rng_bits, int batch,
                                            int eos, int redraw, void *stream) {
    if (!out || !logits || !top_k || !top_p || !temp || !rng_bits || batch < 1 || batch > 65535 || vocab < 1 ||
        vocab > 4096)
        return -1;
    std::vector<SampSlotRow> h((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        if (!nucleus_params_ok("qtts_hip_sample_nucleus_rows", b, top_p[b], temp[b])) return -1;
        SampSlotRow &r = h[b];
        r.temp = r.st_temp = temp[b]; r.top_p = r.st_top_p = top_p[b]; r.top_k = r.st_top_k = top_k[b];
        r.rep = 1.0f; r.seed_bits = 0;
    }
    const bool talker = eos >= 0 && redraw;
    if (talker && eos >= vocab) return -1;
    hipStream_t st = (hipStream_t)stream;
    // the table, then (talker mode) n_gen | stopped | cur_row | codes | st_rng, `batch` words each
    const size_t tab_b = h.size() * sizeof(SampSlotRow), scr_b = talker ? (size_t)batch * 5 * 4 : 0;
    char *mem = nullptr;
    CK(hipMalloc((void **)&mem, tab_b + scr_b));
    SampSlotRow *t = (SampSlotRow *)mem;
    int rc = hipMemcpyAsync(t, h.data(), tab_b, hipMemcpyHostToDevice, st) == hipSuccess ? 0 : -1;
    if (!rc && talker) rc = hipMemsetAsync(mem + tab_b, 0, scr_b, st) == hipSuccess ? 0 : -1;
    if (!rc) {
        SampArgs s;
        s.logits = logits; s.ld = vocab; s.n = vocab; s.nb = batch; s.out_tok = out;
        if (talker) {
            int *w = (int *)(mem + tab_b);
            s.mode = 1; s.rng = rng_bits; s.suppress_lo = vocab; s.eos = eos; s.rep = 1.0f; s.fixed = 1;
            s.n_gen = w; s.stopped = w + batch; s.cur_row = w + 2 * batch; s.codes = w + 3 * batch;
            s.codes_bstride = 1; s.G = 1; s.st_rng = (uint32_t *)(w + 4 * batch);
        } else {
            s.mode = 0; s.st_rng = rng_bits;
        }
        rc = qtts_sample_slots_n(s, t, st, nullptr, path, qtts_sample_nucleus_on());
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;   // (h and the scratch live until the launch finished)
    hipFree(mem);
    return rc;
}

// every rows-long device index vector inside [0, lim) (the kernels index by
// them unchecked)
static int attn_ints_ok(const char *who, const char *what, const int *dev, int rows, int lim, hipStream_t st) {
    std::vector<int> h(rows);
    CK(hipMemcpyAsync(h.data(), dev, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    for (int v : h)
        if (v < 0 || v >= lim) { fprintf(stderr, "%s: %s %d outside [0, %d)\n", who, what, v, lim); return -1; }
    return 0;
}

static bool attn_dims_ok(int NH, int KV, int HD, int S, int rows, int kv_dtype) {
    return NH >= 1 && KV >= 1 && HD >= 1 && S >= 1 && rows >= 1 && rows <= 65535 && (kv_dtype == 0 || kv_dtype == 1);
}

// The talker's decode attention on its own, launched as a talker layer
// launches it (mode 0, the kernel's own split merge); waits for the result.
// skip: AttnArgs::skip, per row (may be NULL).
extern "C" int qtts_hip_attn_decode_ex(float *out, const float *qkv, void *kc, void *vc, const float *qn_w,
                                       const float *kn_w, const float *rope_cos, const float *rope_sin,
                                       const int *pos, int NH, int KV, int HD, int S, int rows, float eps,
                                       int kv_dtype, const int *skip, void *stream) {
    if (!out || !qkv || !kc || !vc || !qn_w || !kn_w || !rope_cos || !rope_sin || !pos) return -1;
    if (!attn_dims_ok(NH, KV, HD, S, rows, kv_dtype)) return -1;
    hipStream_t st = (hipStream_t)stream;
    CKI(attn_ints_ok("qtts_hip_attn_decode", "position", pos, rows, S, st));
    AttnArgs t;
    t.mode = 0; t.qkv = qkv; t.ld_qkv = (NH + 2 * KV) * HD; t.qn_w = qn_w; t.kn_w = kn_w; t.eps = eps;
    t.rope_cos = rope_cos; t.rope_sin = rope_sin;
    t.kc = (float *)kc; t.vc = (float *)vc; t.S = S; t.kv_dtype = kv_dtype;
    t.pos = pos; t.NH = NH; t.KV = KV; t.HD = HD; t.out = out; t.ld_out = NH * HD; t.nrows = rows;
    t.skip = skip;
    const int gph = NH % KV ? 1 : NH / KV, ch = qtts_attn_keys_per_split(HD, false, 0);
    t.nsplit = (S + ch - 1) / ch;
    const size_t part_n = (size_t)rows * KV * t.nsplit * (gph * HD + 2 * gph), cnt_n = (size_t)rows * KV;
    void *scratch = nullptr;
    CK(hipMalloc(&scratch, part_n * 4 + cnt_n * 4));
    t.part = (float *)scratch;
    t.cnt = (int *)(t.part + part_n);
    int rc = hipMemsetAsync(scratch, 0, part_n * 4 + cnt_n * 4, st) == hipSuccess ? 0 : -1;
    if (!rc) rc = qtts_attention(t, st);
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    hipFree(scratch);
    return rc;
}

extern "C" int qtts_hip_attn_decode(float *out, const float *qkv, void *kc, void *vc, const float *qn_w,
                                    const float *kn_w, const float *rope_cos, const float *rope_sin, const int *pos,
                                    int NH, int KV, int HD, int S, int rows, float eps, int kv_dtype, void *stream) {
    return qtts_hip_attn_decode_ex(out, qkv, kc, vc, qn_w, kn_w, rope_cos, rope_sin, pos, NH, KV, HD, S, rows, eps,
                                   kv_dtype, nullptr, stream);
}

// The cached attention (mode 1) on its own: prep 1 as prefill_rows issues it
// (qtts_qk_prep, then qtts_attention, on fused q|k|v rows), prep 0 as the
// codec transformer and the encoder do (q ready, caches filled, a window).
extern "C" int qtts_hip_attn_cached(float *out, float *q, int ld_q, void *kc, void *vc, const float *qn_w,
                                    const float *kn_w, const float *rope_cos, const float *rope_sin,
                                    const int *row_b, const int *pos, int NH, int KV, int HD, int S, int slots,
                                    int rows, float eps, int win, int kv_dtype, int prep, void *stream) {
    if (!out || !q || !kc || !vc || !row_b || !pos) return -1;
    if (prep != 0 && prep != 1) return -1;
    if (prep && (!qn_w || !kn_w || !rope_cos || !rope_sin)) return -1;
    if (!attn_dims_ok(NH, KV, HD, S, rows, kv_dtype) || slots < 1 || win < 0) return -1;
    if (HD < 8 || HD > 128 || (HD & 7) || NH % KV || !qtts_attn_head_ok(HD)) return -1;   // (qtts_attention's own rule, before the cache writes)
    if (ld_q < (prep ? NH + 2 * KV : NH) * HD) return -1;
    if (kv_dtype == 1 && win != 0) return -1;   // (as qtts_attention: no bf16 window path)
    hipStream_t st = (hipStream_t)stream;
    CKI(attn_ints_ok("qtts_hip_attn_cached", "position", pos, rows, S, st));
    CKI(attn_ints_ok("qtts_hip_attn_cached", "slot", row_b, rows, slots, st));
    AttnArgs t;
    t.mode = 1; t.qkv = q; t.ld_qkv = ld_q; t.qn_w = qn_w; t.kn_w = kn_w; t.eps = eps;
    t.rope_cos = rope_cos; t.rope_sin = rope_sin;
    t.kc = (float *)kc; t.vc = (float *)vc; t.S = S; t.kv_dtype = kv_dtype;
    t.pos = pos; t.row_b = row_b; t.NH = NH; t.KV = KV; t.HD = HD; t.out = out; t.ld_out = NH * HD; t.nrows = rows;
    t.win = win;
    int rc = prep ? qtts_qk_prep(t, st) : 0;
    if (!rc) rc = qtts_attention(t, st);
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    return rc;
}

// The sub-talker's attention + O projection by kv head (k_attn_o) on its own:
// fp32 caches [rows][S][KV*HD], no id table; part [KV][rows][R].  1 = a shape
// qtts_attn_o_covers refuses.
extern "C" int qtts_hip_attn_o(float *part, const float *qkv, float *kc, float *vc, const float *qn_w,
                               const float *kn_w, const float *rope_cos, const float *rope_sin, const int *pos,
                               const uint16_t *Wo, int R, int NH, int KV, int HD, int S, int rows, float eps,
                               void *stream) {
    if (!part || !qkv || !kc || !vc || !qn_w || !kn_w || !rope_cos || !rope_sin || !pos || !Wo) return -1;
    if (!attn_dims_ok(NH, KV, HD, S, rows, 0) || R < 1) return -1;
    AttnArgs t;
    t.mode = 0; t.qkv = qkv; t.ld_qkv = (NH + 2 * KV) * HD; t.qn_w = qn_w; t.kn_w = kn_w; t.eps = eps;
    t.rope_cos = rope_cos; t.rope_sin = rope_sin; t.kc = kc; t.vc = vc; t.S = S;
    t.pos = pos; t.NH = NH; t.KV = KV; t.HD = HD; t.ld_out = NH * HD; t.nrows = rows;
    if (!qtts_attn_o_covers(t, Wo)) return 1;
    hipStream_t st = (hipStream_t)stream;
    CKI(attn_ints_ok("qtts_hip_attn_o", "position", pos, rows, S, st));
    int rc = qtts_attn_o(t, Wo, R, part, st);
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    return rc;
}

// The pair form of k_attn_o on its own: rows 0 and 1 of one slot at positions
// 0 and 1, both from qkv [2][(NH + 2 KV) HD] (no id table); caches [S][KV*HD];
// part [KV][2][R].  1 = a shape qtts_attn_o_pair_covers refuses.
extern "C" int qtts_hip_attn_o_pair(float *part, const float *qkv, float *kc, float *vc, const float *qn_w,
                                    const float *kn_w, const float *rope_cos, const float *rope_sin, const int *skip,
                                    const uint16_t *Wo, int R, int NH, int KV, int HD, int S, float eps,
                                    void *stream) {
    if (!part || !qkv || !kc || !vc || !qn_w || !kn_w || !rope_cos || !rope_sin || !Wo) return -1;
    if (!attn_dims_ok(NH, KV, HD, S, 2, 0) || R < 1) return -1;
    AttnArgs t;
    t.mode = 0; t.qkv = qkv; t.ld_qkv = (NH + 2 * KV) * HD; t.qn_w = qn_w; t.kn_w = kn_w; t.eps = eps;
    t.rope_cos = rope_cos; t.rope_sin = rope_sin; t.kc = kc; t.vc = vc; t.S = S;
    t.pos = nullptr; t.NH = NH; t.KV = KV; t.HD = HD; t.ld_out = NH * HD; t.nrows = 2; t.skip = skip;
    if (!qtts_attn_o_pair_covers(t, Wo)) return 1;
    hipStream_t st = (hipStream_t)stream;
    int rc = qtts_attn_o_pair(t, Wo, R, part, st);
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    return rc;
}

// k_gemvw (nrows 1) or its pair form (nrows 2) for the default-cache-policy
// shapes, with the sub-talker chain's prologue: x [nrows][cols] + the partials
// part [n_part][nrows][cols] summed in order (part NULL: none), the sum stored
// to x_new [nrows][cols] (NULL: not stored), RMSNorm by w (NULL: none).
// 1 = a shape the kernel does not cover.
extern "C" int qtts_hip_resident_matvec_rows_bf16(float *out, const uint16_t *A, const float *x, const float *w,
                                                  float eps, int rows, int cols, int epi, const float *part,
                                                  int n_part, float *x_new, int nrows, void *stream) {
    if (!out || !A || !x || rows < 1 || cols < 1 || (nrows != 1 && nrows != 2)) return -1;
    if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU) return -1;
    if (part && n_part < 1) return -1;
    if (part && cols > 1024) return 1;   // (the kernels hold the partials in registers up to 1024 columns)
    GemvArgs a = gv(A, rows, cols, x, cols, out, epi == EPI_SWIGLU ? rows / 2 : rows, nrows, epi);
    a.norm_w = w; a.eps = eps; a.nt = 0;
    if (part) { a.xadd = part; a.n_xadd = n_part; a.ld_xadd = nrows * cols; a.ldb_xadd = cols; }
    if (x_new) { a.xcopy = x_new; a.ldxc = cols; a.xcopy_normed = 0; }
    return nrows == 2 ? qtts_gemvw_pair(a, (hipStream_t)stream) : qtts_gemvw(a, (hipStream_t)stream);
}

// qtts_bgemv_desc_t checked and translated to the batch kernels' arguments
// (the split-K scratch and tickets are the caller's: ypart / tick stay unset).
// No pointer is dereferenced.  -1 = a bad descriptor.
static int bgemv_desc_args(const qtts_bgemv_desc_t *d, GemvArgs &a) {
    if (!d || !d->A || d->rows < 1 || d->cols < 1 || d->batch < 2 || d->batch > QTTS_HIP_MAX_BATCH) return -1;
    if (d->epi < EPI_STORE || d->epi > EPI_SWIGLU || d->src < 0 || d->src > 2) return -1;
    if ((d->epi == EPI_BIAS || d->epi == EPI_BIAS_SILU) && !d->bias) return -1;
    if (d->src == 0 ? !d->x : (!d->table || !d->ids)) return -1;
    if (d->part_in && (d->src != 0 || d->n_part_in < 1 || d->n_part_in > 4)) return -1;
    if (d->kz < 0 || d->kz == 1 || d->kz > 4) return -1;
    if (d->kz >= 2 && (d->self_reduce ? !d->y : !d->part_out)) return -1;
    if (d->kz < 2 && !d->y) return -1;
    a = gv(d->A, d->rows, d->cols, d->src == 0 ? d->x : nullptr, d->ldx, d->y, d->ldy, d->batch, d->epi);
    if (d->src == 1) a.table = (const bf16_t *)d->table;
    if (d->src == 2) a.table_f32 = (const float *)d->table;
    a.ids = d->ids; a.ids_bstride = d->ids_bstride; a.ids_rstride = d->ids_rstride; a.ids_off = d->ids_off;
    a.row_sel = d->row_sel;
    if (d->part_in) {
        a.xadd = d->part_in; a.n_xadd = d->n_part_in; a.ld_xadd = d->batch * d->cols; a.ldb_xadd = d->cols;
    }
    a.norm_w = d->norm_w; a.eps = d->eps;
    if (d->xcopy) { a.xcopy = d->xcopy; a.ldxc = d->cols; a.xcopy_normed = d->xcopy_normed; }
    a.bias = d->bias;
    if (d->kz >= 2) {
        a.kz = d->kz; a.ld_ypart = (size_t)d->batch * d->rows;
        if (!d->self_reduce) { a.ypart = d->part_out; a.y = nullptr; }
    }
    return 0;
}

// One lock-step batch GEMV (qtts_bgemv: 2..16 rows k_gemvb, else k_gemvm;
// 17..64 k_gemvx) with everything the decode frame can ask of it, on its own.  The
// split-K scratch is allocated here; the tickets of the self-reducing form
// live as long as the library (zeroed once: every launch leaves them zero, as
// the frame graph relies on).  1 = no batch kernel covers the case.
extern "C" int qtts_hip_batch_matvec_case(const qtts_bgemv_desc_t *d, void *stream) {
    GemvArgs a;
    if (bgemv_desc_args(d, a)) return -1;
    hipStream_t st = (hipStream_t)stream;
    float *scratch = nullptr;
    static int *ticks = nullptr;   // (one device: the parity entry of a test process)
    if (d->kz >= 2 && d->self_reduce) {
        if (!ticks) {
            CK(hipMalloc((void **)&ticks, QTTS_GM_TICKS * sizeof(int)));
            CK(hipMemset(ticks, 0, QTTS_GM_TICKS * sizeof(int)));
        }
        CK(hipMalloc((void **)&scratch, (size_t)d->kz * a.ld_ypart * 4));
        a.ypart = scratch; a.tick = ticks;
    }
    int rc = qtts_bgemv(a, st);
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    if (scratch) hipFree(scratch);
    return rc;
}

// The plan qtts_hip_batch_matvec_case would launch (qtts_bgemv_plan), host
// only: the self-reducing form's scratch and tickets are stand-in addresses.
extern "C" int qtts_hip_batch_matvec_plan(const qtts_bgemv_desc_t *d, qtts_bgemv_plan_t *out) {
    GemvArgs a;
    if (!out || bgemv_desc_args(d, a)) return -1;
    if (d->kz >= 2 && d->self_reduce) { a.ypart = (float *)(uintptr_t)256; a.tick = (int *)(uintptr_t)256; }
    BgPlan p;
    const int rc = qtts_bgemv_plan(a, p);
    *out = qtts_bgemv_plan_t();
    if (rc) return rc;
    out->kernel = p.kernel; out->n_tmpl = p.nt;
    for (int i = 0; i < p.nt; ++i) out->tmpl[i] = p.t[i];
    out->src = p.src; out->grid_x = (int)p.grid.x; out->grid_y = (int)p.grid.y; out->block = (int)p.block.x;
    out->lds_bytes = p.smem; out->tpw = p.tpw; out->cch = p.cch;
    return 0;
}

// qtts_rows_gemm_desc_t checked and translated to the multi-row GEMMs'
// arguments.  No pointer is dereferenced.  -1 = a bad descriptor.
static int rows_gemm_args(const qtts_rows_gemm_desc_t *d, int force, GemvArgs &a) {
    if (!d || !d->A || !d->y || d->rows < 1 || d->R < 1 || d->C < 1 || force < -1 || force > 2) return -1;
    if (d->epi < EPI_STORE || d->epi > EPI_SWIGLU || d->src < 0 || d->src > 1) return -1;
    if ((d->epi == EPI_BIAS || d->epi == EPI_BIAS_SILU) && !d->bias) return -1;
    if (d->src == 0 ? !d->x : (!d->table || !d->ids)) return -1;
    if (d->ldy < (d->epi == EPI_SWIGLU ? d->R / 2 : d->R) || (d->src == 0 && d->ldx < d->C)) return -1;
    a = gv(d->A, d->R, d->C, d->src == 0 ? d->x : nullptr, d->ldx, d->y, d->ldy, d->rows, d->epi);
    if (d->src == 1) { a.table = d->table; a.ids = d->ids; a.ids_bstride = d->ids_bstride; }
    a.norm_w = d->norm_w; a.eps = d->eps; a.bias = d->bias; a.nt = 0;
    return 0;
}

// The plan of one multi-row projection under `force` (qtts_hip.h): pgemm's
// where it is asked for (or dispatched to) and covers, else mgemm's.
// 0 planned, 1 not covered.
static int rows_gemm_plan(const GemvArgs &a, bool has_inv, bool has_part, size_t part_elems, bool has_planes,
                          size_t plane_elems, int force, bool &use_pgemm, PgPlan &pp, MgPlan &mp) {
    use_pgemm = false;
    if (force >= 1 || (force < 0 && a.nb > 16)) {
        const int bn = force == 1 ? 128 : force == 2 ? 256 : qtts_pgemm_bn_env();
        const int rc = qtts_pgemm_plan(a, has_planes, plane_elems, has_part, part_elems, bn, pp);
        if (rc == 0) { use_pgemm = true; return 0; }
        if (force >= 1) return rc;
    }
    return qtts_mgemm_plan(a, has_inv, has_part, part_elems, mp);
}

static void rows_gemm_report(bool use_pgemm, const PgPlan &pp, const MgPlan &mp, qtts_rows_gemm_plan_t *out) {
    if (!out) return;
    const dim3 g = use_pgemm ? pp.grid : mp.grid;
    out->kernel = use_pgemm ? pp.kernel : mp.kernel;
    out->kz = use_pgemm ? pp.kz : mp.kz;
    out->grid_x = (int)g.x; out->grid_y = (int)g.y; out->grid_z = (int)g.z;
    out->block = use_pgemm && pp.kernel == RG_PGEMM_4 ? 512 : 256;
}

extern "C" int qtts_hip_rows_gemm_plan(const qtts_rows_gemm_desc_t *d, size_t part_elems, size_t plane_elems,
                                       int force, qtts_rows_gemm_plan_t *plan_out) {
    GemvArgs a;
    if (!plan_out || rows_gemm_args(d, force, a)) return -1;
    *plan_out = qtts_rows_gemm_plan_t();
    bool use_pgemm;
    PgPlan pp;
    MgPlan mp;
    const int rc = rows_gemm_plan(a, true, part_elems > 0, part_elems, plane_elems > 0, plane_elems, force, use_pgemm,
                                  pp, mp);
    if (rc) return rc;
    rows_gemm_report(use_pgemm, pp, mp, plan_out);
    return 0;
}

// One multi-row projection on its own, through the launchers themselves
// (which plan again from the same arguments: the report is their plan).
extern "C" int qtts_hip_rows_gemm_case(const qtts_rows_gemm_desc_t *d, int force, qtts_rows_gemm_plan_t *plan_out,
                                       void *stream) {
    GemvArgs a;
    if (rows_gemm_args(d, force, a)) return -1;
    if (plan_out) *plan_out = qtts_rows_gemm_plan_t();
    if (d->norm_w && !d->inv) return -1;
    if ((d->part_elems > 0 && !d->part) || (d->plane_elems > 0 && !d->planes)) return -1;
    float *part = d->part_elems > 0 ? d->part : nullptr;
    unsigned short *planes = d->plane_elems > 0 ? d->planes : nullptr;
    bool use_pgemm;
    PgPlan pp;
    MgPlan mp;
    int rc = rows_gemm_plan(a, d->inv != nullptr, part != nullptr, d->part_elems, planes != nullptr, d->plane_elems,
                            force, use_pgemm, pp, mp);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (use_pgemm)
        rc = qtts_pgemm(a, d->inv, planes, d->plane_elems, st, part, d->part_elems, pp.BN);
    else
        rc = qtts_mgemm(a, d->inv, st, part, d->part_elems);
    if (rc == 1) return -1;   // (the launcher's own plan disagreed with the one reported)
    if (hipStreamSynchronize(st) != hipSuccess) rc = -1;
    if (!rc) rows_gemm_report(use_pgemm, pp, mp, plan_out);
    return rc;
}
