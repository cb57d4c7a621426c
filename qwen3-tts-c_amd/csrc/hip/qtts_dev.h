// qtts_dev.h - the device context behind the C-ABI of include/qtts_hip.h, as
// the four runtime translation units share it (internal, not installed):
//   qtts_runtime.hip   the model, its state, prompts, slots, the stage entries
//   qtts_rt_frame.hip  the launches of a decode frame and of a prefill layer
//   qtts_rt_codec.hip  the codec entries (they forward to k_codec.hip)
//   qtts_rt_hooks.hip  the kernel-level test hooks qtts_hip_* (no qtts_dev)
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <atomic>
#include <vector>

#include "qtts_common.h"
#include "qtts_kernels.h"
#include "qtts_codec.h"
#include "qtts_enc.h"
#include "../../../include/qtts_hip.h"

#define CK(x)                                                                                              \
    do {                                                                                                   \
        hipError_t e_ = (x);                                                                               \
        if (e_ != hipSuccess) {                                                                            \
            fprintf(stderr, "HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, __LINE__, #x);   \
            return -1;                                                                                     \
        }                                                                                                  \
    } while (0)
#define CKI(x)                                                                                             \
    do {                                                                                                   \
        if ((x) != 0) return -1;                                                                           \
    } while (0)

struct Layer {
    bf16_t *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wdown = nullptr;
    float *qn = nullptr, *kn = nullptr, *in = nullptr, *post = nullptr;
};

// The residual stream of a chain of layers: `rows` rows of R floats in xa, plus
// npend partials at pend that are still to be added to them (row b of partial
// p at pend + (p rows + b) R): the split-K columns of an O / down projection
// that does not reduce them itself, or the per-head partials of the fused
// attention + O.  The next GEMV that reads the residual adds them in its
// prologue and writes the sum to the other buffer, xb, which is the residual
// from then on.
struct ResidStream {
    float *xa = nullptr, *xb = nullptr;
    const float *pend = nullptr;
    int npend = 0, R = 0, rows = 0;
    void reset(float *a, float *b, int R_, int rows_) { xa = a; xb = b; pend = nullptr; npend = 0; R = R_; rows = rows_; }
    // this launch left n partials of the residual at `part`
    void hold(const float *part, int n) { pend = part; npend = n; }
    // g reads the residual: it takes what is pending and, with `copy`, writes
    // the summed rows to xb (the buffers flip); a head, which reads the
    // residual last, passes copy = false
    void read(GemvArgs &g, bool copy = true) {
        if (!pend) return;
        add_in(g, copy ? xb : nullptr);
        if (copy) { std::swap(xa, xb); pend = nullptr; npend = 0; }
    }
    // g writes the residual (EPI_RESID) split over kz columns of K (0: no
    // split): from self_min rows up its last column adds the partials itself
    // (GemvArgs::tick) and nothing is pending; below, the next reader adds them
    // (measured: profiles/r02r_bsplit_self_ab.txt; batch 16 174.3 vs 169.5
    // audio-s/s self-reducing, batch 8 109.9 vs 113.9; again after the loads of
    // both sides were unserialised, same box: self-reducing at every batch
    // size gave batch 2 38.7 vs 42.6, 4 70.5 vs 76.0, 8 123.6 vs 126.3, 16
    // 193.3 vs 189.0)
    void write_split(GemvArgs &g, float *part, int kz, int *tick, int self_min) {
        if (!kz) return;
        g.ypart = part; g.kz = kz; g.ld_ypart = (size_t)rows * g.R;
        if (rows >= self_min) { g.tick = tick; return; }
        g.y = nullptr;
        hold(part, kz);
    }

private:
    void add_in(GemvArgs &g, float *xnew) const {
        g.xadd = pend; g.n_xadd = npend; g.ld_xadd = rows * R; g.ldb_xadd = R;
        if (xnew) { g.xcopy = xnew; g.ldxc = R; g.xcopy_normed = 0; }
    }
};

static constexpr int QTTS_MAX_SLOTS = 64;   // row counts with their own tail graph (qtts_dev_set_rows)

struct qtts_dev {
    qtts_dims_t d{};
    int device = 0;
    hipStream_t st = nullptr;
    size_t wbytes = 0, sbytes = 0;
    std::vector<void *> wallocs, sallocs;
    // QTTS_HIP_ARENA=1: small buffers (<= QTTS_ARENA_SMALL) carved from
    // 32 MB blocks (dalloc): one 2 MB-fragment mapping for every activation
    // vector, norm weight and bias instead of one allocation each
    unsigned char *war = nullptr, *sar = nullptr;
    size_t war_off = 0, war_cap = 0, sar_off = 0, sar_cap = 0;
    // talker
    std::vector<Layer> tl, sl;
    bf16_t *codec_emb = nullptr, *text_emb = nullptr, *fc1w = nullptr, *fc2w = nullptr, *head = nullptr;
    float *fc1b = nullptr, *fc2b = nullptr, *tk_norm = nullptr;
    // sub-talker
    bf16_t *st_emb = nullptr, *lm = nullptr, *st_proj = nullptr;
    float *st_projb = nullptr, *st_norm = nullptr;
    // small_to_mtp_projection applied once at load to every embedding row a
    // sub-talker pass g >= 1 can consume (fp32): [V][Hs] of the talker codec
    // embedding (pass 1) and [G-1][Vs][Hs] of the sub-talker ones (passes 2..)
    float *codec_ptab = nullptr, *st_ptab = nullptr;
    // the sub-talker's layer-0 q|k|v of every row a pass g >= 1 can consume
    // (its input is a table row chosen by the previous code alone): fp32
    // [V + (G-2) Vs][QKVs], pass 1 rows first, then pass g at V + (g-2) Vs;
    // computed once at load by the per-frame GEMV itself (bit-identical)
    float *qkv0_tab = nullptr;
    // codec
    CodecModel codec;
    // voice-clone encoders (speaker x-vector, 12 Hz reference codes)
    EncModel enc;
    // rope
    float *rope_cos = nullptr, *rope_sin = nullptr, *rope_cos_s = nullptr, *rope_sin_s = nullptr;
    int rope_max = 0;
    std::set<std::string> got;
    // state
    int nb = 0, nrun = 0, max_frames = 0, S = 0, p_cap = 0, tr_cap = 0, rows_cap = 0;  // nb: allocated slots (strides), nrun: rows launched
    float *x_tk = nullptr, *qkv = nullptr, *att = nullptr, *hbuf = nullptr, *logits = nullptr, *tk_hid = nullptr;
    float *x_st2 = nullptr, *opart = nullptr;   // attn_o: second residual buffer, per-head O partials
    // batch split-K (nb >= 2): second talker residual, O / down partials; the
    // talker's residual after its last layer (what the codec head reads): tk_res
    float *x_tk2 = nullptr, *bpo = nullptr, *bpd = nullptr;
    float *ppart = nullptr;      // prefill split-K partials (<= 16 rows, kz <= 4)
    ResidStream tk_res;
    bool bsplit = true;      // QTTS_HIP_BSPLIT=0: batch O / down projections without split-K
    int bself_min = 9;       // batch split-K producers reduce their own partials from this many rows up
    int bkz_max = 0;         // QTTS_HIP_BKZ_MAX: cap on the batch split-K columns (0: 2 up to 8 rows, else 4)
    int bkz_wide = 1;        // QTTS_HIP_BKZ_WIDE=0: above 8 rows, no extra split-K columns for > 2048-wide slices (bsplit_kz); 2: from 2 rows, up to 4 columns
    float *x_st = nullptr, *qkv_s = nullptr, *att_s = nullptr, *h_s = nullptr, *logits_s = nullptr;
    float *kc = nullptr, *vc = nullptr, *kcs = nullptr, *vcs = nullptr;
    // element type of the talker cache kc / vc, [L][B][S][KV*HD]: 0 fp32, 1 bf16
    // (uint16 rows behind the same pointers; kv_layer() takes the slices).
    // kv_dtype is what the allocated state holds, kv_want what the next
    // qtts_dev_begin allocates (qtts_dev_set_kv_dtype, QTTS_HIP_KV at creation);
    // the sub-talker cache kcs / vcs is always fp32
    int kv_dtype = 0, kv_want = 0;
    // the last talker pass left its last layer's attention output in `att`
    // (false: batch 1 with the merge deferred to the O projection)
    bool att_own = false;
    int *codes = nullptr, *counts = nullptr, *n_gen = nullptr, *stopped = nullptr, *cur_row = nullptr;
    // [B] the id each slot's last draw produced (every sampler's out_tok): the
    // next sub-talker pass reads its input row by it -- one dependent load
    // where codes[b][cur_row[b]][g-1] took two (cur_row, then the code)
    int *last_tok = nullptr;
    int *stop_step = nullptr, *kv_len = nullptr, *n_trailing = nullptr;
    float *att_part = nullptr;   // split-K decode attention partials (talker)
    int *att_cnt = nullptr, att_nsplit = 0;
    int *btick = nullptr;        // self-reducing batch split-K tickets [QTTS_GM_TICKS] (zeroed)
    uint32_t *rng = nullptr, *st_rng = nullptr;
    float *trailing = nullptr, *prefill = nullptr, *pad_emb = nullptr;
    // prefill / prompt scratch
    float *px = nullptr, *pqkv = nullptr, *patt = nullptr, *ph = nullptr, *pt1 = nullptr, *pproj = nullptr;
    int *prow_b = nullptr, *ppos = nullptr, *psrc = nullptr, *pids = nullptr, *pplan = nullptr, *plast = nullptr;
    int ids_cap = 0;
    // voice-clone prompt inputs of the next qtts_dev_prompt (qtts_dev_prompt_ref)
    int *pref = nullptr;
    float *pspk = nullptr;
    int pref_cap = 0, n_pref = 0, has_spk = 0;
    std::vector<int> p_len_h, n_tr_h;
    // The instruct prefix cache (DESIGN.md "Instruct and the prefix cache"):
    // pfx_ids[b] = the text ids of slot b's kind-2 plan rows (its prompt rows
    // [0, n), qtts_dev_prompt); an entry = those rows' K and V of all layers,
    // [2][L][n][KV*HD] in the element type it was saved from, keyed by the ids
    // and that type.  Outside the decode state (sallocs): entries survive
    // qtts_dev_begin and a re-allocation; a change of the KV element type drops
    // them (alloc_state), qtts_dev_destroy drops all.
    struct PrefixEntry {
        std::vector<int> ids;
        int dtype = 0;
        void *buf = nullptr;
        size_t bytes = 0;
        unsigned long long used = 0;   // LRU stamp
    };
    std::vector<std::vector<int>> pfx_ids;
    std::vector<PrefixEntry> pfx;
    int pfx_cap = 16;                  // QTTS_HIP_PREFIX_CACHE entries (0: off), qtts_dev_prefix_cache
    unsigned long long pfx_clock = 0;
    qtts_gen_params_t par{};
    bool have_par = false;
    hipGraphExec_t g0 = nullptr, gN = nullptr;
    // work queue, tail of a run: the talker-first frame graph over the first
    // nrun < nb slots (qtts_dev_set_rows), captured on first use
    hipGraphExec_t gNr[QTTS_MAX_SLOTS + 1] = {};
    // what g0 / gN hold: -1 nothing valid, 0 no graphs (QTTS_HIP_NO_GRAPH),
    // 1 the plain frame, 2 the frame with the forced sampler (f_armed), 3 / 4
    // the frame with the per-slot sampler, fast-only / general (sp_armed);
    // every arming and every qtts_dev_begin that drops one resets it to -1, so
    // a graph of one kind is never replayed for another
    int graph_key = -1;
    // teacher forcing, the free-draw record and logit taps (qtts_dev_force /
    // qtts_dev_tap): allocated by the first arming after a qtts_dev_begin,
    // freed by the next begin -- a plain run holds none of it.  forced / drawn
    // are laid out like `codes`; f_phase: 0 no run begun, 1 begun and no frame
    // launched yet (arming is valid), 2 frames launched
    int *f_forced = nullptr, *f_drawn = nullptr, *f_taps = nullptr, *f_tap_meta = nullptr;
    float *f_tap_logits = nullptr;
    int f_tap_ld = 0, f_ntaps = 0, f_phase = 0;
    int f_run_frames = 0;   // max_frames of the last qtts_dev_begin (the state may hold more)
    bool f_armed = false;
    size_t f_bytes = 0;
    // per-slot sampling parameters (qtts_dev_slot_params): one SampSlotRow per
    // slot on the device with its host mirror, allocated by the first call
    // after a qtts_dev_begin and freed by the next begin -- a plain run holds
    // none of it.  While armed the frames hold the per-slot samplers (graph_key
    // 3: the fast-only family; 4: the general kernel, from the first row of the
    // run that is not fast-path eligible in both modes on -- sp_general never
    // goes back within a run)
    SampSlotRow *sp_tab = nullptr;
    std::vector<SampSlotRow> sp_host;
    bool sp_armed = false, sp_general = false;
    // incremental text input (qtts_dev_text_open / _append, k_textfeed.hip): a
    // run is fed from its first qtts_dev_text_open until the next
    // qtts_dev_begin; its frames are graphs of their own (graph_key + 8) whose
    // first node computes `gate` and whose stop readers take it (stop_rd).  The
    // buffers live with the state, allocated by the first fed run on it:
    // tf_open / tf_gate / tf_held [B], tf_eos [B][H] each slot's tts_eos row,
    // tf_xsave [B][H] the talker input rows of a frame, tf_t1 [16][TH] fc1's
    // output of an append.  tf_rows / tf_open_h: the host's mirror of
    // n_trailing / text_open; tf_held_h: held counters as of the last poll
    bool fed = false;
    int *tf_open = nullptr, *tf_gate = nullptr, *tf_held = nullptr;
    float *tf_eos = nullptr, *tf_xsave = nullptr, *tf_t1 = nullptr;
    std::vector<int> tf_rows, tf_open_h, tf_held_h;
    // EOS-mode lagged poll: the sampler mirrors each slot's stop into pinned
    // host memory; an event after every frame lets the host wait for frame
    // s - 1 while frame s is already queued (qtts_dev_frame_done)
    int *hstop = nullptr;
    int hstop_cap = 0;
    hipEvent_t fev[2] = {nullptr, nullptr};
    // codec overlapped with the decode (qtts_dev_codec_async_*): its own stream,
    // ordered after the frames it decodes by an event; output stays on device
    hipStream_t cst = nullptr;
    hipEvent_t cev = nullptr;
    float *cwav = nullptr;
    size_t cwav_cap = 0;
    // host codes staged for qtts_dev_codec_stream_push_host / _prime (grown on demand)
    int *push_codes = nullptr;
    size_t push_cap = 0;
    bool prime_pending = false;   // a qtts_dev_codec_stream_prime push runs on cst (cev marks its end)
    float *pwav = nullptr;        // the prime's discarded audio (never the codec_async output cwav)
    size_t pwav_cap = 0;
    // the live codec snapshots saved on this context (qtts_dev_codec_mstream_save):
    // destroy releases their device memory
    std::vector<qtts_codec_snapshot_t *> snaps;
    // a batch's codec passes side by side (qtts_dev_codec_multi): lanes 1.. with
    // their own scratch and stream (lane 0 is `codec`), the waveforms and the
    // host-given codes staged on the device
    std::vector<CodecModel *> clanes;
    std::vector<hipStream_t> clane_st;
    float *mwav = nullptr;
    size_t mwav_cap = 0;
    int *mcodes = nullptr;
    size_t mcodes_cap = 0;
    // per-kernel profiling of one eager frame (qtts_dev_profile_frame)
    struct Prof { int kind; double bytes; hipEvent_t a, b; const char *name; };
    std::vector<Prof> prof;
    bool profiling = false;
    bool attn_o = true;      // QTTS_HIP_ATTN_O=0: sub-talker attention and O projection as two kernels
    bool tab0b = true;       // QTTS_HIP_TAB0B=0: batch layer-0 q|k|v by GEMV instead of the table
    bool st_pair = true;     // QTTS_HIP_ST_PAIR=0: batch-1 sub-talker passes 0 and 1 as two single-row chains
    // QTTS_HIP_L2PF=<mask>: which edges of the batch-1 sub-talker chain carry
    // the next-launch weight prefetch (0 none): 1 q|k|v -> attention + O,
    // 2 attention + O -> gate|up, 4 gate|up -> down, 8 down -> next q|k|v or
    // head, 16 head -> the next pass's first launch (two launches ahead);
    // (the same for the batch chain on k_gemvb measured 2 % slower at batch 8
    // and 16, profiles/r04g_ab_l2pf_batch.txt, and was removed)
    int l2pf = 31;
    int l2pf_tk = 0;         // QTTS_HIP_L2PF_TK bits (batch-1 talker, non-temporal): 1 q|k|v -> O's W_o, 2 O -> gate|up
    unsigned *pf_sink = nullptr;
    bool attn_defer = true;  // QTTS_HIP_ATTN_DEFER=0: batch-1 talker attention merges its own splits
    int attn_lpk = 0;        // QTTS_HIP_ATTN_LPK=4|8|16 (HD 128 split size), latched here: sizes att_part
    // QTTS_HIP_GM_DBG=<layer>: phase stamps of that talker layer's batch GEMVs
    // (q|k|v, O, gate|up, down), printed by qtts_dev_get_codes
    int gm_dbg_layer = -1;
    unsigned long long *gm_dbg = nullptr;
    float *pinv = nullptr;   // per-row 1/rms scratch of the matrix-core projections
    int pinv_cap = 0;
    float *mpart = nullptr;   // split-K partials of the matrix-core projections (k_mgemm_reduce)
    size_t mpart_elems = 0;
    // the prefill GEMM's activation planes [3][rows][K] bf16 (k_pgemm.hip)
    unsigned short *pplanes = nullptr;
    size_t pplanes_elems = 0;
    bool pgemm = true;       // QTTS_HIP_PGEMM=0: the prefill on k_mgemm (rounds 1-5)

    int QKV() const { return (d.NH + 2 * d.KV) * d.HD; }
    int QKVs() const { return (d.NHs + 2 * d.KVs) * d.HDs; }
    size_t kv_esz() const { return kv_dtype == 1 ? 2 : 4; }
    // layer l's slice [B][S][KV*HD] of a talker cache (kc or vc)
    float *kv_layer(float *c, int l) const {
        return reinterpret_cast<float *>(reinterpret_cast<char *>(c) + (size_t)l * nb * S * d.KV * d.HD * kv_esz());
    }
};

// A codec snapshot as the C-ABI hands it out: the codec's snapshot and the
// context that saved it.  Every live one is in g_snaps, so a pointer that was
// freed (or never was a snapshot) is refused by look-up, never dereferenced.
// A snapshot outlives its context as a dead one (owner NULL, no device
// memory) until it is freed.
struct qtts_codec_snapshot {
    CodecSnapshot s;
    qtts_dev *owner = nullptr;
};

// ----------------------------------------------------------------- helpers called across the files
inline uint32_t seed_bits(int seed) {   // a seed as the float-bit RNG state the samplers start from
    float f = (float)seed;
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
// qtts_runtime.hip
void *dalloc(qtts_dev *dv, size_t n, bool weight);
void drop_row_graphs(qtts_dev *dv);
// qtts_rt_frame.hip
GemvArgs gv(const bf16_t *W, int R, int C, const float *x, int ldx, float *y, int ldy, int nb, int epi);
int rows_proj(qtts_dev *dv, GemvArgs a, int rows, bool prefill = false);
int build_proj_tables(qtts_dev *dv);
int build_qkv0_table(qtts_dev *dv);
int talker_layers(qtts_dev *dv);
GemvArgs talker_head_args(qtts_dev *dv);
int talker_tail(qtts_dev *dv);
int subtalker(qtts_dev *dv);
int record_frame(qtts_dev *dv, bool with_talker);
int capture(qtts_dev *dv, bool with_talker, hipGraphExec_t *out);
int ensure_graphs(qtts_dev *dv);
int prefill_rows(qtts_dev *dv, const std::vector<int> &slots, const std::vector<int> &nrows, std::vector<int> &last,
                 const std::vector<int> *first = nullptr);
// qtts_rt_codec.hip
int join_prime(qtts_dev *dv);
void snapshots_orphan(qtts_dev *dv);
