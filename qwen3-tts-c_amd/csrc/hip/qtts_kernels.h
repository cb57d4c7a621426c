// qtts_kernels.h - internal launch interface of the gfx950 kernels (C++ only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t bf16_t;

constexpr int QTTS_GM_TICKS = 1024;   // self-reducing split-K tickets (row blocks per launch)

enum { EPI_STORE = 0, EPI_BIAS = 1, EPI_BIAS_SILU = 2, EPI_RESID = 3, EPI_SWIGLU = 4 };

// The next launch's weight slice, loaded by the SAME workgroup index of this
// launch right after its own weights (qtts_l2pf below): workgroup b of every
// decode launch runs on XCD b % 8, so the slice lands in the L2 that the next
// launch's workgroup b reads from.  For linear workgroup id b:
//   start = base + (b % pm) * pa + (b / pm) * pb,
//   `chunks` 64-B chunks: chunk c at start + (c >> lg) * ld + (c & (2^lg - 1)) * 64
// (rows of 2^lg chunks at stride ld; chunks <= threads x QTTS_PF_LOADS).  One
// 4-B load per chunk brings its line in.
constexpr int QTTS_PF_LOADS = 4;
struct L2Prefetch {
    const unsigned char *base = nullptr;   // nullptr: none
    int pm = 1 << 30;
    long long pa = 0, pb = 0;
    int chunks = 0, lg = 30, ld = 0;
    int cs = 6;                            // log2 bytes per chunk (64 B; the micro-benchmark also runs 128)
    // slices of the target: a workgroup b >= nwg of a launch wider than the
    // next one's grid has no slice of its own and re-reads its fallback line
    // (the start formula would otherwise run past the target's end)
    int nwg = 0;
    unsigned *sink = nullptr;              // never written (the loads' values are folded into a test)
};

struct GemvArgs {
    const bf16_t *W = nullptr;  // [R, C] bf16 row-major
    int R = 0, C = 0;
    int ksplit = 0;             // 0 = auto
    int cch = 0;                // set by the launcher (k_gemv, k_gemvm: BgPlan::cch)
    int nt = 1;                 // non-temporal weight loads
    int nb = 1;                 // batch rows
    // x source: fp32 rows, or bf16 / fp32 table rows gathered by id
    const float *x = nullptr;
    int ldx = 0;
    const bf16_t *table = nullptr;      // [*, C]
    const float *table_f32 = nullptr;   // [*, C] (precomputed projected embeddings)
    const int *ids = nullptr;       // id(b) = ids[b*ids_bstride + row_sel[b]*ids_rstride + ids_off]
    int ids_bstride = 1, ids_rstride = 0, ids_off = 0;
    const int *row_sel = nullptr;
    // lean kernel (qtts_gemvw) only: reps consecutive ids in one launch
    // (grid.y), rep j reads id ids[ids_off + j] and writes y + j * ldy_rep
    int reps = 1;
    size_t ldy_rep = 0;
    // prologue
    // batch-1 prologue only: x += sum_p xadd[p*ld_xadd + c] (p < n_xadd, summed
    // in order first) -- the O projection's per-head partials (qtts_attn_o)
    const float *xadd = nullptr;
    int n_xadd = 0, ld_xadd = 0;
    // batch GEMV (k_gemvb / k_gemvm / k_gemvx): the same prologue per row, at
    // most 4 partials, row b of partial p at xadd + p*ld_xadd + b*ldb_xadd
    int ldb_xadd = 0;
    // batch-1 prologue only (the batch GEMV's planner refuses it): x = the
    // decode attention's output, merged here from its split partials (AttnArgs::defer): amerge [KV][am_nsplit][GPH*HD
    // + 2*GPH], am_ch keys per split, the live key count am_pos[0] + 1
    const float *amerge = nullptr;
    const int *am_pos = nullptr;
    int am_nsplit = 0, am_ch = 0, am_hd = 0, am_gph = 0;
    // batch GEMV split-K producer (all three kernels): kz > 1 workgroup columns each take
    // C / kz of K and store raw partials ypart[z*ld_ypart + b*R + r] (the
    // consumer adds them with the residual through xadd); y / epi unused
    float *ypart = nullptr;
    size_t ld_ypart = 0;
    int kz = 1;
    // self-reducing split-K (batch GEMV, EPI_RESID only, kz <= 4): one zeroed ticket per grid.x
    // workgroup; the last of the kz columns to finish a row block adds the
    // partials in order to the residual, y = y + (p0 + p1 + ...), and resets
    // its ticket, so the next GEMV reads y alone (no xadd)
    int *tick = nullptr;            // [QTTS_GM_TICKS]
    const float *norm_w = nullptr;  // RMSNorm weights [C] (nullptr: no norm)
    float eps = 1e-6f;
    float *xcopy = nullptr;         // workgroup 0 writes x rows here
    int ldxc = 0;
    int xcopy_normed = 0;
    // epilogue
    float *y = nullptr;
    int ldy = 0;
    const float *bias = nullptr;
    int epi = EPI_STORE;
    unsigned long long *dbg = nullptr;   // diagnostics (k_gemvb): [workgroup][8] phase stamps, 100 MHz clock
#ifdef QTTS_STAMPS
    int dbg_xfirst = 0;                  // (stamp builds) k_gemvw waits for x before issuing its weights
#endif
    L2Prefetch pf;                      // batch-1 lean kernel (k_gemvw): the next launch's weights
    // the batch-1 fast path needs 16-B aligned fp32 rows (or a bf16 table)
    bool ldx_ok1() const {
        if (xadd && (((uintptr_t)xadd & 15) || ld_xadd % 4 || n_xadd < 1)) return false;
        if (table) return C % 4 == 0;
        const bool nw_ok = !norm_w || ((uintptr_t)norm_w & 15) == 0;
        if (table_f32) return C % 4 == 0 && ((uintptr_t)table_f32 & 15) == 0 && nw_ok;
        return ((uintptr_t)x & 15) == 0 && nw_ok;
    }
};

int qtts_gemv(const GemvArgs &a, hipStream_t st);
// batch-1 wave-per-row GEMV for Infinity-Cache-resident weights (k_gemvw.hip); 1 = not covered
int qtts_gemvw(const GemvArgs &a, hipStream_t st);
// shapes whose batch-1 GEMV takes the decode attention's merge in its prologue (GemvArgs::amerge)
bool qtts_gemvw_amerge_ok(int R, int C);
// The lock-step batch GEMV (2..64 rows) on the bf16 matrix cores: three kernels,
//   k_gemvb (2..16 rows, x sliced per wave; tried first),
//   k_gemvm (2..16 rows, x staged as bf16 planes per workgroup),
//   k_gemvx (17..64 rows, one moving 32-column K step per wave),
// one planner and one router (qtts_bgemv.hip).  BG_* name a kernel and, or-ed,
// the kernels a caller allows.
enum { BG_NONE = 0, BG_GEMVM = 1, BG_GEMVB = 2, BG_GEMVX = 4, BG_ALL = 7 };
struct BgPlan {
    int kernel = BG_NONE;
    int nt = 0, t[5] = {0, 0, 0, 0, 0};   // the template integers, in the kernel's order (the last: the source kind)
    int src = 0;                          // BG_SRC_* (qtts_bgemv_dev.h)
    dim3 grid, block;
    size_t smem = 0;                      // dynamic LDS bytes
    int tpw = 0, cch = 0;                 // k_gemvm's run-time arguments: tiles per workgroup, staged column chunk
};
// The plan for `a` among the `allowed` kernels: pure host code, nothing is
// launched and no pointer dereferenced; depends on its arguments and on
// QTTS_HIP_GEMVB / QTTS_HIP_GB_W (read per call) only.  0 = planned, 1 = not
// covered, -1 = an argument error.
int qtts_bgemv_plan(const GemvArgs &a, BgPlan &p, unsigned allowed = BG_ALL);
// the planner, then the launch of its plan: the planner's results, -1 on a launch error too
int qtts_bgemv(const GemvArgs &a, hipStream_t st, unsigned allowed = BG_ALL);
// the launch switch over each file's own instantiations (0 ok, -1 launch error)
int qtts_gemvm_launch(const GemvArgs &a, const BgPlan &p, hipStream_t st);
int qtts_gemvb_launch(const GemvArgs &a, const BgPlan &p, hipStream_t st);
int qtts_gemvx_launch(const GemvArgs &a, const BgPlan &p, hipStream_t st);
// the weight shapes k_gemvx takes (qtts_dev_begin refuses a model with another above 16 slots)
bool qtts_gemvx_shape_ok(int R, int C);
// The seven kernels of the multi-row GEMMs (k_mgemm<MT,NW>, k_pgemm<WN>), as
// the plans below name them (QTTS_RG_* of qtts_hip.h).
enum { RG_MGEMM_1_1 = 0, RG_MGEMM_2_1 = 1, RG_MGEMM_4_1 = 2, RG_MGEMM_4_2 = 3, RG_MGEMM_4_4 = 4, RG_PGEMM_2 = 5,
       RG_PGEMM_4 = 6 };
// qtts_mgemm's plan: the kernel (RG_*), its template (mt row tiles x nw weight
// tiles per workgroup), the 64-row chunks, the split-K columns and the grid
struct MgPlan {
    int kernel = -1, mt = 0, nw = 0, nch = 0, kz = 1;
    dim3 grid;
};
// host only: 0 = planned, 1 = not covered (what qtts_mgemm launches for the
// same arguments; has_inv / has_part: its inv_scratch / part are non-null)
int qtts_mgemm_plan(const GemvArgs &a, bool has_inv, bool has_part, size_t part_elems, MgPlan &p);
// multi-row (2..64) projection on the bf16 matrix cores (k_mgemm.hip); 1 = not covered
int qtts_mgemm(const GemvArgs &a, float *inv_scratch, hipStream_t st, float *part = nullptr, size_t part_elems = 0);
// split-K partial floats qtts_mgemm may use for `rows` activation rows and outputs <= widest
size_t qtts_mgemm_part_elems(size_t rows, size_t widest);
int qtts_row_rms(const float *x, int ldx, int rows, int C, float eps, float *inv, hipStream_t st);
// split-K tail of qtts_mgemm / qtts_pgemm: y = epilogue(sum_z part[z][row][R], z in order)
int qtts_mgemm_reduce(const GemvArgs &a, const float *part, int kz, hipStream_t st);
// the talker prefill's projections over > 16 rows (k_pgemm.hip): activations
// split once into 3 bf16 planes (scratch: qtts_pgemm_plane_elems), then an
// LDS-tiled 128 x 128 MFMA GEMM; 1 = shape not covered.  bn: the tile width
// (128 | 256), 0 = QTTS_HIP_PGEMM_BN, else by the row tiles
int qtts_pgemm(const GemvArgs &a, float *inv_scratch, unsigned short *planes, size_t plane_elems, hipStream_t st,
               float *part, size_t part_elems, int bn = 0);
// qtts_pgemm's plan: the kernel (RG_*), the tile width, the padded rows, the
// split-K columns and the grid
struct PgPlan {
    int kernel = -1, BN = 0, Mp = 0, kz = 1;
    dim3 grid;
};
// host only: 0 = planned, 1 = not covered (what qtts_pgemm launches for the
// same arguments; bn 128 | 256 forces the tile width, else by the row tiles)
int qtts_pgemm_plan(const GemvArgs &a, bool has_planes, size_t plane_elems, bool has_part, size_t part_elems, int bn,
                    PgPlan &p);
int qtts_pgemm_bn_env();   // QTTS_HIP_PGEMM_BN as a tile width (128 | 256), else 0
size_t qtts_pgemm_plane_elems(size_t rows, size_t K);

struct AttnArgs {
    int mode = 0;                  // 0 decode (fused q/k norm + rope + cache write), 1 cached
    const float *qkv = nullptr;    // row r: [q NH*HD | k KV*HD | v KV*HD]
    int ld_qkv = 0;
    const float *qn_w = nullptr, *kn_w = nullptr;
    float eps = 1e-6f;
    const float *rope_cos = nullptr, *rope_sin = nullptr;  // [pos][HD]
    float *kc = nullptr, *vc = nullptr;                    // layer slice [B][S][KV*HD]
    int S = 0;
    const int *pos = nullptr;      // decode: pos[b]; cached: pos[row]
    int pos_const = 0;             // used when pos == nullptr
    const int *row_b = nullptr;    // cached: batch index of each row
    int NH = 0, KV = 0, HD = 0;
    float *out = nullptr;          // [rows][NH*HD]
    int ld_out = 0;
    int nrows = 0;
    const int *skip = nullptr;     // decode: per-b stop flags (skip the cache write)
    int win = 0;                   // >0: sliding window (keys t > pos - win), c/qwen_tts_codec.c:363-367
    // decode: the q|k|v row of row r read from a table by id instead of qkv
    // (the sub-talker's layer-0 projections of every input id, precomputed):
    // id = tab_ids[r*tab_bstride + tab_row_sel[r]*tab_rstride + tab_off]
    const float *qkv_tab = nullptr;
    const int *tab_ids = nullptr, *tab_row_sel = nullptr;
    int tab_bstride = 0, tab_rstride = 0, tab_off = 0;
    // decode split-K scratch: [rows][KV][nsplit][GPH*HD + 2*GPH] partials, [rows][KV] tickets (zeroed)
    float *part = nullptr;
    int *cnt = nullptr;
    int nsplit = 0;
    // decode: every split (one or more) leaves its (acc, max, sum) in `part`
    // and the merge is the consumer's (GemvArgs::amerge, the O projection's
    // prologue) instead of the last split's
    int defer = 0;
    L2Prefetch pf;                 // k_attn_o: the next launch's weights
#ifdef QTTS_STAMPS
    unsigned long long *dbg = nullptr;   // (stamp builds) k_attn_o: [workgroup][8] start / end, 100 MHz clock
#endif
    // k_attn_short with a q|k|v table (the batch sub-talker's layer 0): kv
    // head 0's workgroup of row r also copies the input row of id(r) (the
    // table ids above) from xc_tab (fp32) or xc_tab16 (bf16) to xc_dst + r
    // xc_n -- the residual the skipped q|k|v GEMV would have copied
    const float *xc_tab = nullptr;
    const bf16_t *xc_tab16 = nullptr;
    float *xc_dst = nullptr;
    int xc_n = 0;
    // lanes per key of the split kernel at HD 128 (4 / 8 / 16), latched by the
    // model at creation (QTTS_HIP_ATTN_LPK); 0 = the default for HD / defer
    int lpk = 0;
    // element type of the caches behind kc / vc: 0 fp32, 1 bf16 (the pointers
    // then address uint16 rows of the same [B][S][KV*HD] layout).  Only the
    // talker's cache may be bf16: the split decode kernel, the generic k_attn
    // and the prefill writers have a bf16 form, the short / table / k_attn_o
    // paths refuse it.  K and V rows are rounded to nearest even as they are
    // stored, and the token's own k, v enter its attention as the rounded values
    int kv_dtype = 0;
};
// keys per split of the talker decode attention (deferred merge or not; lpk
// as AttnArgs::lpk)
int qtts_attn_keys_per_split(int HD, bool defer, int lpk);
// true when the decode attention takes these arguments on its split kernel,
// whose merge AttnArgs::defer hands to the consumer
bool qtts_attn_defer_ok(const AttnArgs &a);
// sub-talker attention + O projection split by kv head: part [KV][nrows][R]
// (GQA 2, <= 16 keys); 1 = not covered
int qtts_attn_o(const AttnArgs &a, const bf16_t *Wo, int R, float *part, hipStream_t st);
// true when qtts_attn_o takes these arguments (it returns 1 otherwise)
bool qtts_attn_o_covers(const AttnArgs &a, const bf16_t *Wo);

// The sub-talker's positions 0 and 1 as one two-row pass at batch 1
// (k_stpair.hip), each row bit-identical to the single-row launch:
// the pair form of qtts_gemvw for the default-cache-policy shapes -- a.nb == 2,
// x rows at a.x + b a.ldx, y rows at a.y + b a.ldy, partials row b of partial p
// at a.xadd + p a.ld_xadd + b a.ldb_xadd, the new residual rows at a.xcopy +
// b a.ldxc; epilogues STORE / RESID / SWIGLU; 1 = not covered
bool qtts_gemvw_pair_covers(int R, int C, int epi);
int qtts_gemvw_pair(const GemvArgs &a, hipStream_t st);
// and of qtts_attn_o: rows 0 and 1 of slot 0 at positions 0 and 1 (a.pos
// unset); row 0 is a.qkv, row 1 a.qkv + a.ld_qkv or, with a.qkv_tab, the
// table's row a.tab_ids[a.tab_off]; a.kc / a.vc the slot's [S][KV HD] cache
// (rows 0 and 1 written, none read); a.skip[0] keeps the cache write back;
// a.xc_dst: row 1's input table row (xc_tab / xc_tab16, xc_n wide) copied
// there; part [KV][2][R]; 1 = not covered
bool qtts_attn_o_pair_covers(const AttnArgs &a, const bf16_t *Wo);
int qtts_attn_o_pair(const AttnArgs &a, const bf16_t *Wo, int R, float *part, hipStream_t st);

// Name of the kernel instantiation the last launcher on this thread chose
// (diagnostics: per-kernel profile rows match rocprofv3's kernel names).
extern thread_local const char *qtts_last_kernel;
// head sizes the attention kernels serve: k_attn's lane groups (HD/8 lanes per
// key, HD/4 per V row) need a power of two, as every specialised kernel does
inline bool qtts_attn_head_ok(int HD) { return HD == 8 || HD == 16 || HD == 32 || HD == 64 || HD == 128; }
int qtts_attention(const AttnArgs &a, hipStream_t st);
// prefill helper: q/k RMSNorm + RoPE in place on qkv rows, k/v -> cache at (row_b, pos)
int qtts_qk_prep(const AttnArgs &a, hipStream_t st);

struct SampArgs {
    const float *logits = nullptr;
    int ld = 0, n = 0, nb = 1;
    int top_k = 50;
    float top_p = 1.0f, temp = 0.9f;
    uint32_t *rng = nullptr;       // [B] float-bit xorshift state
    int mode = 0;                  // 0 sub-talker, 1 talker
    // talker mode
    int suppress_lo = 0, eos = -1;
    float rep = 1.0f;
    int *counts = nullptr;         // [B][n] occurrences of each generated id
    int fixed = 0;
    int *n_gen = nullptr, *stopped = nullptr, *cur_row = nullptr, *stop_step = nullptr;
    int *host_stopped = nullptr;   // pinned host mirror of `stopped` (set when a slot stops)
    uint32_t *st_rng = nullptr;    // sub-talker state reset per frame
    uint32_t seed_bits = 0;
    // outputs: codes[b*codes_bstride + cur_row[b]*G + g]
    int *codes = nullptr;
    int codes_bstride = 0, G = 16, g = 0;
    int *out_tok = nullptr;        // optional plain output [b]
};
// stop_rd (a fed run, k_textfeed.hip): the flag row b reads in place of
// a.stopped -- the gate; an EOS still goes to a.stopped and a.host_stopped.
// NULL: the launches of before, argument for argument.
int qtts_sample(const SampArgs &a, hipStream_t st, const int *stop_rd = nullptr);

// Teacher forcing and logit taps: the extra pointers of the sampler's forced
// form (qtts_sample_dev.h sample_row_forced).  `forced` and `drawn` have the
// layout of SampArgs::codes ([b * codes_bstride + frame * G + g]); a forced
// entry < 0 leaves the draw free, a drawn entry stays -1 where no draw
// happened.  taps: {slot, frame, group} each, slot -1 unused; tap t's values
// go to tap_logits + t * tap_ld (the n real entries), its {n, RNG state before
// the draw, drawn id, 1} to tap_meta + 4 t.
constexpr int QTTS_MAX_TAPS = 8;
struct SampForce {
    const int *forced = nullptr;
    int *drawn = nullptr;
    const int *taps = nullptr;
    float *tap_logits = nullptr;
    int *tap_meta = nullptr;
    int tap_ld = 0;
};
// qtts_sample with the forced form of the same three launch families
int qtts_sample_forced(const SampArgs &a, const SampForce &f, hipStream_t st);

// Per-slot sampling parameters (qtts_dev_slot_params): one 32-byte row per
// slot, which the per-slot sampler's workgroup b loads as two dwordx4 with its
// first loads (k_sample_p.hip).  Talker draws take temp / top_p / rep / top_k
// and reset st_rng[b] to seed_bits, sub-talker draws take the st_ values; the
// same fields of SampArgs are then unused.
struct alignas(16) SampSlotRow {
    float temp, top_p, rep;
    int top_k;
    float st_temp, st_top_p;
    int st_top_k;
    uint32_t seed_bits;
};
static_assert(sizeof(SampSlotRow) == 32, "two dwordx4 loads cover a row");
// the row's draw of mode `mode` (1 talker, 0 sub-talker) over n logits is
// fast-path eligible (qtts_sample_dev.h fast_path)
bool qtts_sample_row_fast(const SampSlotRow &r, int mode, int n);
// The per-slot sampler: the fast-only 1024-thread family k_sample_pw when
// every row of the run is fast-path eligible in both modes (all_fast; never
// otherwise) and QTTS_HIP_SAMPLE_W is not 0, else the general 256-thread
// kernel k_sample_p, which picks fast or full per row.
int qtts_sample_slots(const SampArgs &a, const SampSlotRow *tab, bool all_fast, hipStream_t st,
                      const int *stop_rd = nullptr);
// its launches enqueued (or captured) since the library loaded (qtts_hip_sample_slot_launches)
long long qtts_sample_slot_launches();
// The nucleus short list (k_sample_n.hip; qtts_sample_dev.h sample_nucleus):
// a draw with top_p < 1 and top_k <= 64 or top-k off (qtts_sample_nucleus_row)
// from at most 64 ids, the full path behind it in the same launch.  qtts_sample
// sends such SampArgs to qtts_sample_n and qtts_sample_slots' general branch
// launches qtts_sample_slots_n unless QTTS_HIP_SAMPLE_NUCLEUS=0 (read per
// call: qtts_sample_nucleus_on), which restores the kernels of before.
// path (may be NULL): per row 1 fast top-k, 2 nucleus short list, 3 full, 0
// stopped.  nucleus false: no row tries the short list.  Neither counts as a
// per-slot launch by itself (qtts_sample_slots counts its own).
bool qtts_sample_nucleus_on();
bool qtts_sample_nucleus_row(float top_p, int top_k, int n);
int qtts_sample_n(const SampArgs &a, hipStream_t st, const int *stop_rd, int *path, bool nucleus);
int qtts_sample_slots_n(const SampArgs &a, const SampSlotRow *tab, hipStream_t st, const int *stop_rd, int *path,
                        bool nucleus);
// writes row b of the table, stream-ordered; rng / st_rng non-null: the slot's
// RNG states start from the row's seed as well
int qtts_slot_row_set(SampSlotRow *tab, int b, const SampSlotRow &r, uint32_t *rng, uint32_t *st_rng, hipStream_t st);

struct EmbedSumArgs {
    const int *codes = nullptr;
    int codes_bstride = 0, G = 16;
    const int *cur_row = nullptr, *stopped = nullptr;
    const bf16_t *codec_emb = nullptr;   // [V][H]
    const bf16_t *st_emb = nullptr;      // [G-1][Vs][H]
    int Vs = 0, H = 0, nb = 1;
    const float *trailing = nullptr;     // [B][tr_cap][H]
    int tr_cap = 0;
    const int *n_trailing = nullptr;
    const float *pad = nullptr;          // [H]
    float *out = nullptr;                // [B][H]
    int *kv_len = nullptr;
    int advance = 0;
};
int qtts_embed_sum(const EmbedSumArgs &a, hipStream_t st);

// prompt assembly: prefill rows [B][p_cap][H] and trailing rows [B][tr_cap][H]
struct PromptArgs {
    const float *proj = nullptr;   // projected text rows [nrows][H]
    const int *plan = nullptr;     // per output row: {proj_row, codec_id, dest_kind(0 prefill/1 trailing), b, slot}
                                   // codec_id >= 0 codec_emb row, -1 none, -2 spk vector,
                                   // <= -3 reference frame (-3 - id): sum of its G group embeddings
    int nplan = 0, H = 0;
    const bf16_t *codec_emb = nullptr;
    const bf16_t *st_emb = nullptr;   // [G-1][Vs][H] sub-talker input embeddings (reference frames)
    const float *spk = nullptr;       // [H] speaker x-vector (voice clone)
    const int *ref_codes = nullptr;   // [n_ref][G] reference codes (voice clone ICL)
    int n_ref = 0, G = 0, V = 0, Vs = 0;
    float *prefill = nullptr;
    int p_cap = 0;
    float *trailing = nullptr;
    int tr_cap = 0;
};
int qtts_prompt_assemble(const PromptArgs &a, hipStream_t st);

int qtts_copy_rows(float *dst, int ldd, const float *src, int lds, const int *src_rows, int nrows, int ncols,
                   hipStream_t st);

// incremental text input (k_textfeed.hip).  The append: n <= QTTS_TF_MAX
// content ids of slot b (kernel arguments) projected into trailing rows
// n_trailing[b] .. + n - 1, close: the slot's tts_eos row behind them and
// text_open[b] = 0; the last launch stores the new count.
constexpr int QTTS_TF_MAX = 16;
struct TextFeedArgs {
    int ids[QTTS_TF_MAX] = {};
    int n = 0, b = 0, close = 0;
    const bf16_t *text_emb = nullptr, *fc1w = nullptr, *fc2w = nullptr;   // [TV][TH], [TH][TH], [H][TH]
    const float *fc1b = nullptr, *fc2b = nullptr;
    int TH = 0, H = 0;
    float *t1 = nullptr;                 // [QTTS_TF_MAX][TH] fc1's output
    float *trailing = nullptr;           // [B][tr_cap][H]
    int tr_cap = 0;
    int *n_trailing = nullptr, *text_open = nullptr;
    const float *eos = nullptr;          // [H] slot b's tts_eos row
};
int qtts_text_append(const TextFeedArgs &a, hipStream_t st);
// the first and the last node of a fed run's frame: gate[b] = stopped[b] |
// (text_open[b] && n_gen[b] >= n_trailing[b]), held[b] counts the frames a live
// slot was held, and the talker input rows x [nb][H] are saved (x_save; NULL:
// the frame runs no talker step) and, for gated slots, put back
struct TextGateArgs {
    const int *stopped = nullptr, *text_open = nullptr, *n_gen = nullptr, *n_trailing = nullptr;
    int *gate = nullptr, *held = nullptr;
    float *x = nullptr, *x_save = nullptr;
    int H = 0, nb = 1;
};
int qtts_text_gate(const TextGateArgs &a, hipStream_t st);
int qtts_text_restore(const TextGateArgs &a, hipStream_t st);
int qtts_text_open(float *eos, const float *trailing_row, int H, int *n_trailing, int *text_open, int *held, int b,
                   hipStream_t st);

// the instruct prefix cache (k_kvprefix.hip): talker K and V rows [0, n) of one
// slot, all L layers, between the caches [L][B][S][KV*HD] and a packed entry
// [2][L][n][KV*HD] of the same element type, in one launch; a plain copy
struct KvPrefixArgs {
    void *kc = nullptr, *vc = nullptr;   // the slot's row 0 of layer 0 in each cache
    void *entry = nullptr;
    size_t layer_stride = 0;             // bytes between two layers of a cache (B * S * row bytes)
    size_t chunk = 0;                    // bytes of one layer's rows [0, n): n * row bytes
    int L = 0;
    int esz = 4;                         // element bytes: 4 fp32, 2 bf16
    int save = 0;                        // 1: cache -> entry, 0: entry -> cache
};
int qtts_kv_prefix_copy(const KvPrefixArgs &a, hipStream_t st);

// work-queue refill of one slot inside a live batch: the
// slot's talker input row <- its last prompt row, kv_len <- pos, and a fresh
// utterance's counters (Q.c:1250-1270: n_gen, rows, stop, repetition counts,
// both RNG states at the seed)
struct SlotResetArgs {
    int b = 0, pos = 0, H = 0, V = 0;
    const float *row = nullptr;          // [H] the prompt row the slot's next talker step consumes
    float *x = nullptr;                  // [B][H] talker input
    int *kv_len = nullptr, *n_gen = nullptr, *cur_row = nullptr, *stopped = nullptr, *stop_step = nullptr;
    int *last_tok = nullptr, *counts = nullptr;   // counts [B][V]
    uint32_t *rng = nullptr, *st_rng = nullptr;
    uint32_t seed_bits = 0;
};
int qtts_slot_reset(const SlotResetArgs &a, hipStream_t st);

#ifdef QTTS_ARGDUMP
#include "qtts_argdump.h"   // the launcher entries' argument dump (tools/frame_args_ab.py)
#endif
