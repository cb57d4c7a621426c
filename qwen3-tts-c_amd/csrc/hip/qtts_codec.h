// qtts_codec.h - internal interface of the device codec decoder (C++ only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../../include/qtts_hip.h"

// Exact streaming decode state (codec_stream_*): every codec op is causal, so
// decoding frames chunk by chunk with (a) the last (K-1)*dil input columns of
// every convolution, (b) the last input frame of every transposed conv with
// K = 2s and (c) the last window-1 K/V rows of every transformer layer
// carried across chunks equals the full decode (Cd.c:581-749) up to fp order.
struct CodecStream {
    bool active = false;
    int pos0 = 0;              // frames decoded so far (absolute transformer position)
    int tc = 0;                // max frames per internal chunk
    int hm = 64;               // left margin (columns) of every channel-major buffer
    std::vector<float *> hist; // history slots [C][H]
    std::vector<int> hist_c, hist_h;
    std::vector<float *> kc, vc;  // transformer layer caches [(win-1) + tc][kvd]
    float *kvtmp = nullptr;
    int hl = 0;                // valid history rows in the K/V caches
    float *bufA = nullptr, *bufB = nullptr, *bufC = nullptr, *bufD = nullptr;
    size_t buf_elems = 0;
    float *tx = nullptr, *txn = nullptr, *tq = nullptr, *tatt = nullptr, *tg = nullptr, *tu = nullptr;
    float *rvq_s = nullptr, *rvq_a = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    int rope_cap = 0;
    int *iota = nullptr;       // [0 .. win + tc)
    int *zeros = nullptr;
    std::vector<void *> allocs;
};

// n independent exact streaming states decoded in one launch sequence per
// push (codec_mstream_*).  Carried per stream: the 21 history slots, the
// per-layer K/V rows, pos0 and hl.  Shared by the streams of a push: the
// activation scratch (one [C][hm + L] plane per stream, planes one after
// another), the RoPE table and the index rows.
struct CodecMStream {
    bool active = false;
    int ns = 0;                    // streams
    int tc = 0;                    // frames per internal pass (<= 16, fewer where ns planes would pass the scratch budget)
    int hm = 64;                   // left margin (columns) of every plane's rows
    int max_frames = 0;
    std::vector<int> pos0, hl;     // per stream: frames decoded, valid K/V history rows
    std::vector<float *> hist;     // slot -> [ns][C][H]
    std::vector<int> hist_c, hist_h;
    float *kv = nullptr;           // [layers][2][ns][S][kvd]
    int S = 0;                     // K/V rows per stream and layer: (win - 1) + tc
    float *bufA = nullptr, *bufB = nullptr, *bufC = nullptr, *bufD = nullptr;
    size_t buf_elems = 0;          // per stream
    float *tx = nullptr, *txn = nullptr, *tq = nullptr, *tk = nullptr, *tv = nullptr, *tatt = nullptr, *tg = nullptr,
          *tu = nullptr;           // [ns * tc] stacked rows
    float *rvq_s = nullptr, *rvq_a = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    int rope_cap = 0;
    int *sid = nullptr, *row_b = nullptr, *pos = nullptr;   // [ns], [ns * tc], [ns * tc]
    long long *coff = nullptr;     // [ns] offset (ints) of each stream's codes from the push's base
    // positions of a push's streams, pass after pass: pass p's pos0 at
    // pp + 3 p n, its hl at pp + (3 p + 1) n, its valid frame counts tv at
    // pp + (3 p + 2) n (n streams in the push, longest count first, so the
    // streams of a pass are the first ones of the push), uploaded once before
    // the first pass.  pp_passes: passes the buffer holds
    int *pp = nullptr;
    int pp_passes = 0;
    std::vector<int> hpp;          // its host copy
    std::vector<int> hsid, hord, hend;   // a push's stream ids in pass order, their places in the caller's order, end state
    std::vector<long long> hcoff;
    // device table of the carried parts of one stream: the history slots'
    // base pointers and per-stream sizes (C * H), for the reset of one stream,
    // then the 2 * layers K/V planes (base of stream 0's rows, per-stream
    // stride S * kvd), for the save / restore of one stream; snap_off: where
    // each history part starts in a snapshot (floats), the total last
    float **hist_base = nullptr;
    int *hist_elems = nullptr;
    int *snap_off = nullptr;
    int snap_hist_elems = 0;       // floats of a snapshot's history parts (each padded to 4)
    float *wav = nullptr;          // [ns][tc * samples per frame], compact
    std::vector<float> hwav;       // its host copy
    size_t state_bytes = 0, scratch_bytes = 0;
    std::vector<void *> allocs;
};

// One stream's carried state outside the multi-stream state (codec_mstream_save
// / _restore; DESIGN.md 7, "Snapshots"): a compact device buffer of the 21
// history parts, then layers x 2 K/V parts of hl * kvd floats, every part
// padded to a multiple of 4 floats, and the host header that says what it is.
// It holds nothing that depends on the stream count or the pass size.
struct CodecSnapshot {
    float *dev = nullptr;
    size_t elems = 0;              // floats allocated
    int pos0 = 0, hl = 0;
    int layers = 0, kvd = 0, win = 0;
    std::vector<int> slot_elems;   // the history parts' sizes (C * H)
    int device = -1;               // the HIP device that owns dev
};

struct CodecModel {
    qtts_dims_t d{};
    hipStream_t st = nullptr;
    std::map<std::string, float *> w;                 // f32 device tensors by checkpoint name
    std::map<std::string, std::vector<int64_t>> shape;
    std::map<std::string, std::vector<float>> host_keep;  // usage / esum pending codebook build
    float *cb = nullptr;                              // [Q][CB][vq] codebooks
    size_t wbytes = 0;
    // scratch (grown on demand)
    std::vector<void *> scratch;
    float *bufA = nullptr, *bufB = nullptr, *bufC = nullptr, *bufD = nullptr;
    size_t buf_elems = 0;
    float *tq = nullptr, *tx = nullptr, *txn = nullptr, *tatt = nullptr, *tg = nullptr, *tu = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    int t_cap = 0, rope_cap = 0;
    int *codes_tmp = nullptr;
    float *wav = nullptr;
    std::map<std::string, float *> wt;         // conv weights re-laid [Kw][co][ci] for k_conv, by name
    float *xg_part = nullptr;                  // split-K workspace of the codec GEMMs
    size_t xg_part_elems = 0;
    CodecStream cs;
    CodecMStream ms;
    // per-stage timing of codec_decode (the reference's -v -v "Codec stages
    // (ms)" line, c/qwen_tts_codec.c:743-746): events around rvq / preconv /
    // transformer / upsample / vocoder when `timing` is on
    bool timing = false, timed = false;
    hipEvent_t tev[6] = {};
    float stage_ms[5] = {};
};

void codec_init(CodecModel *m, const qtts_dims_t *d, hipStream_t st);
void codec_destroy(CodecModel *m);
void codec_free_state(CodecModel *m);
size_t codec_weight_bytes(const CodecModel *m);
int codec_put_tensor(CodecModel *m, const std::string &name, const void *host, int dtype, const int64_t *shape,
                     int ndim, size_t n);
int codec_finalize(CodecModel *m);
// codes: device int32 [T][cq] (time-major).  Returns malloc'd host audio.
float *codec_decode(CodecModel *m, const int *codes_dev, int T, int *out_samples);
// independent decodes side by side: job i (device codes[i], T[i] frames) on
// lane i % nl (lane 0 = m, lanes[k] from codec_lane_new for k >= 1), its
// waveform copied to dwav + dwav_off[i] (device), out_samples[i] samples;
// returns after every lane's stream has drained
size_t codec_state_bytes(const CodecModel *m, int T);   // one lane's scratch for T frames
CodecModel *codec_lane_new(CodecModel *m, hipStream_t st);
void codec_lane_delete(CodecModel *lane);
int codec_decode_many(CodecModel *m, CodecModel *const *lanes, int nl, int n, const int *const *codes, const int *T,
                      float *dwav, const size_t *dwav_off, int *out_samples);
// streaming decode: begin resets the state (max_frames bounds the absolute
// position; chunk > 16 sizes the internal chunk for long pushes); push decodes T more frames (device codes, rows of stride ldc
// ints) and writes T * 1920 samples to host_out.  Returns samples or -1.
int codec_stream_begin(CodecModel *m, int max_frames, int chunk = 0);
int codec_stream_push(CodecModel *m, const int *codes_dev, int ldc, int T, float *host_out);
// the same into `out` (host memory, synchronous; or device memory: enqueued on
// m->st only, nothing waited for)
int codec_stream_push_to(CodecModel *m, const int *codes_dev, int ldc, int T, float *out, bool host);
void codec_stream_free(CodecModel *m);
// n independent streams, one launch sequence per push whatever n.  begin
// (n_streams 1..64) resets every stream; a begin the active state already
// covers re-uses its buffers.  push decodes T more frames of the n distinct
// streams `streams` from the device codes codes_base + code_off[i] (rows of
// ldc ints), T * samples-per-frame floats each into host_out[i].  The streams
// of a push may be at different positions (each row rotates, lands in its
// cache and attends by its own stream's position); any = false keeps the
// older contract and refuses that.  push_ragged: stream i advances by its own
// counts[i] >= 1 frames (its codes hold at least counts[i] rows), counts[i] *
// samples-per-frame floats into host_out[i]; still one launch sequence per
// pass whatever the counts ("Ragged pushes"); returns the largest count times
// samples-per-frame.  host_out nullptr: the audio is dropped and nothing is
// waited for (everything enqueued on m->st; the priming of reference
// frames).  check_ragged: its refusals (push_any's, and counts NULL, a count
// < 1 or > ld_frames, a stream passing its capacity, named).  Every refusal
// is -1 with a message before anything is launched or changed.  pos: frames decoded of a stream, -1 for a
// bad one.  reset: one stream back to position 0 (zero histories, no K/V
// rows), stream-ordered on m->st, the other streams untouched; -1 with a
// message for a bad stream or no begin.
int codec_mstream_begin(CodecModel *m, int n_streams, int max_frames, int chunk = 0);
int codec_mstream_check(CodecModel *m, int n, const int *streams, int T, bool any = false);
int codec_mstream_push(CodecModel *m, int n, const int *streams, const int *codes_base, const long long *code_off,
                       int ldc, int T, float *const *host_out, bool any = false);
int codec_mstream_check_ragged(CodecModel *m, int n, const int *streams, const int *counts, int ld_frames);
int codec_mstream_push_ragged(CodecModel *m, int n, const int *streams, const int *codes_base,
                              const long long *code_off, int ldc, const int *counts, float *const *host_out);
int codec_mstream_reset(CodecModel *m, int stream);
// save: one stream's carried state into the empty snapshot `snap` (its device
// buffer is allocated here; codec_snapshot_release frees it), one launch, the
// stream untouched.  restore: the inverse into any stream of any begin of the
// same codec (history planes and K/V rows 0..hl-1 written, then pos0 / hl
// taken over; rows >= hl stay: none is inside a new row's window).  Both are
// stream-ordered on m->st and wait for nothing on the host.  -1 with a
// message, nothing launched and neither side changed for: no begin (or a
// state re-allocated since), a bad stream, a NULL / empty (save: non-empty)
// snapshot, a snapshot of other codec dims or another device, a restore
// whose position exceeds max_frames.
int codec_mstream_save(CodecModel *m, int stream, CodecSnapshot *snap);
int codec_mstream_restore(CodecModel *m, int stream, const CodecSnapshot *snap);
void codec_snapshot_release(CodecSnapshot *snap);
int codec_mstream_pos(const CodecModel *m, int stream);
void codec_mstream_free(CodecModel *m);

// ---- generic fp32 implicit GEMM (exported for the kernel-level C-ABI) ----
// C(m, n) = sum_k A(m, k) * B(k, n), fp32 products on v_mfma_f32_32x32x2_f32.
enum { XA_ROWS = 0, XA_TRANS = 1, XA_TCONV_W = 2 };
enum { XB_WT = 0, XB_CONV = 1, XB_TCONV = 2 };
enum {
    XE_STORE = 0,        // C[m][n]
    XE_BIAS_N,           // + bias[n]
    XE_BIAS_N_GELU,      // gelu_tanh(acc + bias[n])
    XE_SILU_MUL,         // silu(aux[m][n]) * acc
    XE_SCALE_RESID_N,    // C[m][n] += acc * vec[n]
    XE_BIAS_T,           // out[n][m] = acc + bias[n]
    XE_BIAS_GAMMA_RES_T, // out[n][m] = (acc + bias[n]) * vec[n] + res[n][m]
    XE_BIAS_M,           // conv: out[m][n] = acc + bias[m]
    XE_BIAS_M_RES,       // conv: out[m][n] = acc + bias[m] + res[m][n]
    XE_BIAS_M_SNAKE,     // conv: out[m][n] = snake(acc + bias[m]) with (alpha, inv_beta)[m]
};
struct XGemm {
    int M = 0, N = 0, K = 0;
    int amode = XA_ROWS, bmode = XB_WT, emode = XE_STORE;
    const float *A = nullptr;  int lda = 0;   // rows: A[m*lda+k]; trans: A[k*lda+m]; tconv w: [ci][co][Kw]
    const float *B = nullptr;  int ldb = 0;   // wt: B[n*ldb+k]; conv/tconv: x[ic*ldb + t]
    // conv geometry (XB_CONV: k = ic*Kw + tap; XB_TCONV: k = ic*2 + j)
    int Kw = 1, dil = 1, pad = 0, L = 0, stride = 1, phase = 0, co = 0;
    const float *sa = nullptr, *sb = nullptr;  // optional SnakeBeta on B's input channels
    float *C = nullptr; int ldc = 0;          // output (XE_*_T: out[n*ldc + m]); tconv: out[m*ldc + n*stride + phase]
    const float *bias = nullptr, *vec = nullptr, *aux = nullptr, *res = nullptr;
    int ldaux = 0, ldres = 0;
    const float *ea = nullptr, *eb = nullptr;  // epilogue snake params (XE_BIAS_M_SNAKE)
    float *part = nullptr;                     // split-K workspace (nullptr: no split)
    size_t part_elems = 0;
    int tmin = 0;                              // conv/tconv input columns t >= tmin are read (t < 0: the
                                               // streaming history kept in the buffer's left margin)
    const float *wt = nullptr;                 // XB_CONV: the weights as [Kw][M][K/Kw] (k_conv's layout)
    int kz = 0;                                // k_conv split over input channels (set by the launcher)
    // stream axis (the multi-stream codec; the defaults are the single-segment case).
    // Conv forms (XB_CONV / XB_TCONV): nseg independent column segments of N
    // columns each on grid x; segment s reads B + s*seg_ldb, writes C + s*seg_ldc
    // (res + s*seg_ldres), so a tile never holds two segments and the taps left
    // of column 0 read that segment's own margin.
    // Linear forms over stacked rows (M = segments x seg_m): the operands that
    // are laid out per segment, XA_TRANS's A and the XE_*_T outputs / res, take
    // row m at segment m / seg_m, column m % seg_m (seg_lda / seg_ldc / seg_ldres).
    int nseg = 1, seg_m = 0;
    int seg_lda = 0, seg_ldb = 0, seg_ldc = 0, seg_ldres = 0;
};
int qtts_xgemm(const XGemm &g, hipStream_t st);
