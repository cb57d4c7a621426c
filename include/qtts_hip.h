/*
 * qtts_hip.h - thin C-ABI between the C host (qwen_tts.c, main.c) and the
 * MI355X (gfx950) HIP implementation of the Qwen3-TTS hot path.
 *
 * Plain C: opaque handles, plain pointers and sizes, int error codes
 * (0 = ok, <0 = error with a message on stderr).  No HIP or torch types.
 * "dev" pointers below are device (HBM) addresses; "host" pointers are
 * ordinary process memory.  `stream` arguments are hipStream_t passed as
 * void* (NULL = the default stream).
 *
 * Two layers:
 *   1. Model-level entry points used by the C host's decode loop
 *      (qwen_tts.c) - they replace the compute of
 *        qwen_tts_talker_prefill / qwen_tts_talker_forward   (c/qwen_tts.h:483-486,
 *                                                            c/qwen_tts_talker.c:254-533)
 *        qwen_tts_subtalker_generate                         (c/qwen_tts.h:489-494,
 *                                                            c/qwen_tts_talker.c:539-736)
 *        the per-frame loop body of qwen_tts_generate       (c/qwen_tts.c:1282-1373)
 *        qwen_tts_codec_decode                               (c/qwen_tts.h:497-502,
 *                                                            c/qwen_tts_codec.c:581-749)
 *   2. Kernel-level entry points on device buffers, one per kernel_* of
 *      c/qwen_tts_kernels.h the hot path uses, so each HIP kernel is parity
 *      tested against the CPU oracle in isolation.
 */
#ifndef QTTS_HIP_H
#define QTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qtts_dev qtts_dev_t;

/* Model dimensions (same meaning as qwen_tts_config_t, c/qwen_tts.h:84-144). */
typedef struct {
    int H, I, L, NH, KV, HD, TH, TV, V, G;   /* talker */
    int Hs, Is, Ls, NHs, KVs, HDs, Vs;       /* sub-talker (code predictor) */
    float eps, theta;                        /* talker_rms_norm_eps / talker_rope_theta */
    int cq, ccb, ccbdim, chid, clat, clayers, cheads, ckv, cinter, cwin, cdec;  /* codec */
    int rates[4], ratios[2];
    float ceps;
    int pad_id, bos_id, eos_id;
} qtts_dims_t;

/* Voice-clone encoder dimensions: config.json
 * `speaker_encoder_config` (Qwen3TTSSpeakerEncoderConfig,
 * configuration_qwen3_tts.py:47-67) and speech_tokenizer/config.json
 * `encoder_config` (transformers MimiConfig) + `encoder_valid_num_quantizers`. */
typedef struct {
    /* speaker encoder (ECAPA-TDNN) */
    int mel_dim, enc_dim, n_ch;              /* n_ch = len(enc_channels), 3..8 */
    int ch[8], ks[8], dil[8];
    int att_ch, res2net_scale, se_ch;
    /* 12 Hz tokenizer encoder (Mimi) */
    int hidden, n_filters, ratios[4], kernel, last_kernel, res_kernel, dil_growth, n_res, compress;
    int layers, heads, kv_heads, head_dim, inter, window;
    int n_q, n_sem, cb_size, vq_dim, n_valid;
    float norm_eps, rope_theta;
} qtts_enc_dims_t;

/* Generation parameters (qwen_tts_ctx_t fields, c/qwen_tts.h:420-430). */
typedef struct {
    float temperature, top_p, repetition_penalty;
    int top_k;
    float st_temperature, st_top_p;
    int st_top_k;
    int fixed_codec_tokens;
    int seed;
} qtts_gen_params_t;

/* ---- device + model ---- */
int qtts_hip_device_count(void);
/* Creates the device model on HIP device `device` (selects it for the
 * calling thread).  Returns NULL on error. */
qtts_dev_t *qtts_dev_create(const qtts_dims_t *dims, int device);
void qtts_dev_destroy(qtts_dev_t *dev);
/* Hands one checkpoint tensor (by its safetensors name) to the device.
 * dtype: 0 = F32, 1 = BF16, 2 = F16.  Tensors the hot path does not use are
 * ignored.  Packing (fused [q;k;v], gate|up row quads), bf16 -> f32 of
 * norms/biases, codebook = embedding_sum / max(usage, 1e-5) and SnakeBeta
 * pre-exponentiation (c/qwen_tts.c:481-489, 577-602) happen here. */
int qtts_dev_put_tensor(qtts_dev_t *dev, const char *name, const void *host, int dtype,
                        const int64_t *shape, int ndim);
/* Validates that every required tensor arrived (reports the first missing
 * one like c/qwen_tts.c:381-427) and builds RoPE tables. */
int qtts_dev_finalize(qtts_dev_t *dev);
/* Device bytes currently allocated for weights / state. */
size_t qtts_dev_bytes(const qtts_dev_t *dev, int which /*0 weights, 1 state*/);

/* Element type of the talker KV cache: 0 fp32 (default, or $QTTS_HIP_KV at
 * creation), 1 bf16 -- K (after k-norm and RoPE) and V rows rounded to nearest
 * even as they are stored, a token's own k / v entering its attention as the
 * rounded values, scores / softmax / P.V in fp32 as before.  The sub-talker,
 * codec and encoder caches stay fp32.  set takes effect at the next
 * qtts_dev_begin (new state, new frame graphs) and returns -1 on a bad value;
 * the getter returns the value the next begin will use. */
int qtts_dev_set_kv_dtype(qtts_dev_t *dev, int dtype);
int qtts_dev_kv_dtype(const qtts_dev_t *dev);
/* Diagnostics: talker cache rows [pos0, pos0 + n) of layer `layer`, slot b,
 * to the host as fp32 [n][KV*HD] each (bf16 widened exactly; k_host or v_host
 * may be NULL).  Waits for the context stream.  -1 out of range. */
int qtts_dev_get_kv(qtts_dev_t *dev, int layer, int b, int pos0, int n, float *k_host, float *v_host);
/* Diagnostics: slot b's talker input row [hidden] -- after qtts_dev_prefill the
 * last prompt row's raw hidden state, which frame 0's codec head reads.  Waits
 * for the context stream. */
int qtts_dev_get_hidden(qtts_dev_t *dev, int b, float *host);
/* Diagnostics: what the last talker layer's decode attention of the most
 * recent talker pass read and wrote, for every allocated slot: its q|k|v rows
 * [slots][(NH + 2 KV) HD] and its output [slots][NH HD] (either may be NULL).
 * Waits for the context stream.  The output exists only where the attention
 * merges its own splits (a batch of >= 2 rows, or QTTS_HIP_ATTN_DEFER=0);
 * -1 when asked for it after a pass that deferred the merge. */
int qtts_dev_get_attn(qtts_dev_t *dev, float *qkv_host, float *att_host);

/* ---- generation (batch of nb utterances in lock-step frames) ---- */
/* Lock-step slots per context: 1 plain decode, 2..16 the 16-row matrix-core
 * batch kernels, 17..64 the wide batch kernel (one weight read per GEMV for
 * every slot). */
#define QTTS_HIP_MAX_BATCH 64
/* Allocates state for nb slots (1..QTTS_HIP_MAX_BATCH), max_frames frames (KV
 * capacity = max_prefill + max_frames), resets counters / RNG, (re)captures
 * the frame graphs.  -1 with one line on stderr, before anything is
 * allocated, for more slots than that, and above 16 slots for a model with a
 * decode weight shape the wide batch kernel does not take (named). */
int qtts_dev_begin(qtts_dev_t *dev, int nb, int max_frames, int max_prefill, const qtts_gen_params_t *p);
/* Prompt for slot b (layout built by the host, c/qwen_tts.c:1147-1243):
 *   text_ids[n_text]  text tokens to embed+project (text_embedding -> fc1 ->
 *                     SiLU -> fc2, c/qwen_tts.c:823-847)
 *   plan[5*nplan]     per output row {text row, codec id or -1,
 *                     0 = prefill / 1 = trailing / 2 = prefill row of the
 *                     cacheable prefix (below), b, slot}
 *   p_len, n_trailing prefill / trailing lengths; pad_row = text row of tts_pad */
int qtts_dev_prompt(qtts_dev_t *dev, int b, const int *text_ids, int n_text, const int *plan, int nplan,
                    int p_len, int n_trailing, int pad_row);
/* The instruct prefix cache.  Plan rows of kind 2 are prefill rows (assembled
 * like kind 0) that form the slot's cacheable prefix: they must be the plan's
 * leading rows, prompt rows 0 .. n-1 of slot b in order, text alone (codec id
 * -1), with n < p_len; any other kind-2 plan returns -1 with nothing
 * launched.  Their K / V depend on nothing after them, so qtts_dev_prefill and
 * qtts_dev_refill run a slot with a prefix in two passes, whatever the cache
 * holds: the prefix rows alone (computed once per distinct prefix and saved,
 * afterwards copied back: one launch), then the remaining rows at their own
 * positions.  One cache per device model, keyed by the exact id sequence and
 * the KV element type, LRU, QTTS_HIP_PREFIX_CACHE entries (read at creation,
 * default 16, 0: off -- the prefix rows are then ordinary rows of the one
 * pass).  An entry holds rows [0, n) of all layers, [2][L][n][KV*HD]; entries
 * survive qtts_dev_begin and state re-allocation, a change of the KV element
 * type drops them, qtts_dev_destroy drops all.
 * qtts_dev_prefix_cache: sets the capacity (evicting down to it; 0 clears and
 *   switches the cache off).  qtts_dev_prefix_cache_bytes: device bytes held.
 * qtts_hip_prefix_hits / _misses: restores / computed prefixes, and
 * qtts_hip_prefill_rows: rows sent through the talker prefill passes, since the
 * library loaded (process-wide, like qtts_hip_gemv_wide_launches). */
int qtts_dev_prefix_cache(qtts_dev_t *dev, int max_entries);
size_t qtts_dev_prefix_cache_bytes(const qtts_dev_t *dev);
long long qtts_hip_prefix_hits(void);
long long qtts_hip_prefix_misses(void);
long long qtts_hip_prefill_rows(void);
/* Voice-clone inputs consumed by the next qtts_dev_prompt (no c/ counterpart;
 * modeling_qwen3_tts.py:1967-2019, 2150-2190): reference codes
 * [n_ref][num_code_groups] that plan codec ids <= -3 address (-3 - frame: the
 * frame's 16 group embeddings summed), and the speaker x-vector [hidden] that
 * codec id -2 adds (NULL: none). */
int qtts_dev_prompt_ref(qtts_dev_t *dev, const int *ref_codes, int n_ref, const float *spk);
/* Talker prefill of all nb slots (leaves each slot's last raw hidden). */
int qtts_dev_prefill(qtts_dev_t *dev);
/* Enqueues frame `step` (step 0: codec_head on the prefill hidden; step > 0:
 * talker forward first): sample group 0 -> sub-talker 15 groups -> next
 * input embedding.  Asynchronous (one HIP graph launch). */
int qtts_dev_frame(qtts_dev_t *dev, int step);
/* Waits for the queued work; stopped[b] = 1 once slot b drew EOS
 * (non-fixed mode); n_gen[b] frames stored; stop_step[b] as in the
 * reference's "Stop: eos at step N". */
int qtts_dev_poll(qtts_dev_t *dev, int *stopped, int *n_gen, int *stop_step);
/* EOS mode, lagged: waits only until frame `step` has finished (launch frame
 * step + 1 first) and sets *all_stopped when every slot had drawn EOS by then
 * (the sampler mirrors the stops into pinned host memory). */
int qtts_dev_frame_done(qtts_dev_t *dev, int step, int *all_stopped);
/* ---- work queue (utterances of EOS-variable length on a
 * live lock-step batch; no c/ counterpart -- the reference decodes one
 * utterance per call, Q.c:1059-1443) ---- */
/* Sizes the per-slot trailing text rows for the longest utterance of the run
 * (call after qtts_dev_begin, before the first qtts_dev_prompt). */
int qtts_dev_reserve(qtts_dev_t *dev, int max_trailing);
/* Slot b takes the utterance the last qtts_dev_prompt(dev, b, ...) assembled,
 * inside the live batch: its prompt rows but the last are prefilled into slot
 * b's KV cache, the last row becomes the slot's talker input at position
 * p_len - 1 (the next frame's talker step runs it, then samples the
 * utterance's frame 0), and the slot's counters, repetition counts and RNG
 * states start afresh.  Stream-ordered after the frames already queued. */
int qtts_dev_refill(qtts_dev_t *dev, int b);
/* Stops slot b from the next queued frame on (max_new_tokens / fixed length
 * reached without EOS); stream-ordered. */
int qtts_dev_retire(qtts_dev_t *dev, int b);
/* Lagged like qtts_dev_frame_done: waits for frame `step`, then stopped[b] = 1
 * for every slot that had drawn EOS by then. */
int qtts_dev_frame_stops(qtts_dev_t *dev, int step, int *stopped);
/* Tail of a queue run (nothing left to admit): slot `from`'s whole decode
 * state (KV cache rows, input row, counters, codes, trailing rows, RNG)
 * moves to the freed slot `to`, so the running slots are the first ones;
 * set_rows then launches the first `rows` slots only (a graph per row count,
 * captured on first use).  Both need the stream idle (after frame_stops /
 * get_codes). */
int qtts_dev_move_slot(qtts_dev_t *dev, int from, int to);
int qtts_dev_set_rows(qtts_dev_t *dev, int rows);
/* Copies slot b's codes [n_gen][G] to host. */
int qtts_dev_get_codes(qtts_dev_t *dev, int b, int *host_codes, int max_frames);
/* ---- teacher forcing, the free-draw record and logit taps (no c/
 * counterpart: the reference only samples and continues) ----
 * All of it lasts for one run: armed after qtts_dev_begin and before frame 0,
 * cleared (with its buffers: a plain run allocates none) by the next
 * qtts_dev_begin; the results stay readable until then.  An armed run's frames
 * are graphs of their own with the forced sampler; the next unarmed run
 * captures the plain ones again.  While armed, qtts_dev_refill, _move_slot and
 * _set_rows return -1 (forcing is not defined for the work queue).  Every
 * failure below returns -1 with a message and launches nothing. */
/* Forced codes of slot b: codes[n_frames][G], an entry < 0 leaves that draw
 * free, frames >= n_frames are free.  At draw (f, g) the sampler runs as it
 * always does -- suppression, repetition penalty, the fixed-mode EOS redraw,
 * every RNG advance -- and a forced entry then replaces its result: the stored
 * code, the repetition counts, n_gen, the sub-talker's next input, the next
 * talker embedding and the stop all follow the replaced id (a forced EOS
 * stops the slot; a forced non-EOS continues where the free draw was EOS).
 * n_frames in [0, max_frames]; group-0 ids in [0, V - 1024) or EOS, the other
 * groups' in [0, Vs). */
int qtts_dev_force(qtts_dev_t *dev, int b, const int *codes, int n_frames);
/* Arms one logit tap at draw (frame, group) of slot b; at most 8 per run.
 * Returns the tap's index (arming order). */
int qtts_dev_tap(qtts_dev_t *dev, int b, int frame, int group);
/* Slot b's free-draw record of an armed run: the id the sampler itself
 * produced at every draw, [frames][G], -1 where no draw happened (after a
 * stop, the groups after a forced EOS).  Copies up to max_frames rows (the run
 * holds max_frames + 1 of them) and returns the rows copied; waits for the
 * context stream.  -1 when the last run was not armed. */
int qtts_dev_get_drawn(qtts_dev_t *dev, int b, int *host, int max_frames);
/* Tap i: the values its draw saw -- group 0 after suppression and repetition
 * penalty, before the temperature division and untouched by the EOS redraw;
 * groups >= 1 the raw head output; the n real entries, up to max_n copied --
 * the RNG state before the draw and the free-drawn id (any of the three may be
 * NULL).  Returns n, or -1 if the draw never happened. */
int qtts_dev_get_tap(qtts_dev_t *dev, int i, float *logits_host, int max_n, unsigned *rng_bits, int *drawn);
/* ---- per-slot sampling parameters and seeds (no c/ counterpart: the reference
 * decodes one utterance per call with the ctx's parameters) ----
 * A run samples every slot with qtts_dev_begin's parameters until the first
 * qtts_dev_slot_params after that begin.  That call arms a device table of one
 * 32-byte row per slot, every row first filled from begin's parameters, and
 * from then on the frames hold the per-slot samplers (k_sample_p.hip), whose
 * workgroup b draws with row b: the talker draw with temperature / top_p /
 * repetition_penalty / top_k, resetting the slot's sub-talker RNG to the row's
 * seed each frame, the sub-talker draws with the st_ values.  temperature <= 0
 * becomes 1e-5, top_k <= 0 or >= the vocabulary means no top-k, as in the
 * reference.  fixed_codec_tokens and the frame limit stay run-wide.
 * Which kernel family the frames hold is decided for the run: the fast-only
 * 1024-thread family while every row set so far takes the fast path for both
 * draws (top_p >= 1 and 0 < top_k <= 1024 below the vocabulary), the general
 * 256-thread kernel (fast or full per row) from the first row that does not;
 * a refill that admits such a row mid-run makes the next frame capture the
 * general graphs, and the run never goes back.
 * Before frame 0 the call also sets slot b's two RNG states to the row's
 * seed; later in a run it is ordered on the context stream and the next
 * qtts_dev_refill(dev, b) starts the slot from the row's seed;
 * qtts_dev_move_slot carries the row with the slot.  The next qtts_dev_begin
 * disarms and frees the table (a run that never arms allocates nothing).
 * -1 with a message, and nothing launched, for a call before any
 * qtts_dev_begin, a bad slot, a non-finite value, top_p / st_top_p <= 0 or
 * repetition_penalty <= 0, and when forced codes / taps are armed for the run
 * (qtts_dev_force / qtts_dev_tap likewise return -1 once this is armed: the
 * combination is left out). */
typedef struct {
    float temperature, top_p, repetition_penalty;
    int top_k;
    float st_temperature, st_top_p;
    int st_top_k;
    int seed;
} qtts_slot_params_t;
int qtts_dev_slot_params(qtts_dev_t *dev, int b, const qtts_slot_params_t *p);
/* ---- incremental text input (no c/ counterpart: the reference takes the whole
 * utterance's ids before the prefill; DESIGN.md "Incremental text input") ----
 * With content ids c[0..m) trailing row r is proj(c[r + 1]) for r < m - 1 and
 * row m - 1 is tts_eos; the frame that draws frame r adds row r to the next
 * talker input.  A fed run's frames therefore start with a gate,
 *   gate[b] = stopped[b] | (text_open[b] && n_gen[b] >= n_trailing[b]),
 * and every reader of the stop flag takes it: a slot whose next frame lacks its
 * row is HELD for that frame exactly as a stopped slot is (no draw, no RNG
 * advance, no code row, no counter, no KV position, no new input row; its
 * talker input row is put back at the frame's end), and is looked at again by
 * the next launch.  No kernel waits on a flag.  The whole frame is held:
 * deferring only the embedding sum (drawing a frame before its row is there)
 * is out of scope.  Frame 0 (step 0: the lock-step head on the prefill's
 * hidden states, no talker step) must not be launched while a slot would be
 * held: the caller launches it once every slot has row 0 or is closed.
 * qtts_dev_text_open: after slot b's qtts_dev_prompt -- whose layout is that of
 *   a template with ONE content id, so its only trailing row is tts_eos -- and
 *   before frame 0: the row becomes the slot's eos row, the count goes back to
 *   0, the text is open and the run a fed one, with frame graphs of its own
 *   (an unfed run captures exactly the graphs it always did; the next
 *   qtts_dev_begin ends the fed run).  -1 with a message: outside that window,
 *   forcing / taps armed, a prompt with other trailing rows.  In a fed run
 *   qtts_dev_refill, _move_slot and _set_rows return -1.
 * qtts_dev_text_append: n >= 0 content ids behind the slot's rows, through
 *   text_embedding -> fc1 + bias + SiLU -> fc2 + bias by ONE kernel path whose
 *   per-row summation order does not depend on how many ids share a launch
 *   (k_textfeed.hip: up to 16 ids per launch, passed as kernel arguments);
 *   close: the tts_eos row behind them, text_open[b] = 0.  The row offset is
 *   read on the device and the last store publishes the new count.
 *   Stream-ordered on the context stream, no host wait and no copy -- except
 *   growth past the allocated rows, which waits and makes the next frame
 *   capture its graphs again.  -1 with a message: a slot whose text is not
 *   open (never opened, or closed), an id outside [0, text vocab), n == 0
 *   without close.
 * qtts_dev_get_trailing: rows [row0, row0 + n) of slot b, [n][hidden] floats;
 * qtts_dev_text_state: the device's row count, open flag and held-frame
 *   counter of slot b (any may be NULL).  Both wait for the context stream.
 * qtts_hip_text_held_frames: frames a live slot was held, as the
 *   qtts_dev_poll calls of fed runs saw them, since the library loaded. */
int qtts_dev_text_open(qtts_dev_t *dev, int b);
int qtts_dev_text_append(qtts_dev_t *dev, int b, const int *ids, int n, int close);
int qtts_dev_get_trailing(qtts_dev_t *dev, int b, int row0, int n, float *host);
/* measurement: qtts_dev_text_append between two events on the context stream; waits, *ms = the device time */
int qtts_dev_text_append_ms(qtts_dev_t *dev, int b, const int *ids, int n, int close, float *ms);
int qtts_dev_text_state(qtts_dev_t *dev, int b, int *rows, int *open, int *held);
long long qtts_hip_text_held_frames(void);
/* Codec decode of slot b's generated codes (device-resident) into a malloc'd
 * host buffer of T*1920 samples (caller frees). */
float *qtts_dev_codec_slot(qtts_dev_t *dev, int b, int T, int *out_samples);
/* Per-stage timing of the full codec decodes (the reference's -v -v line
 * "Codec stages (ms): rvq= preconv= transformer= upsample= vocoder=",
 * c/qwen_tts_codec.c:743-746): on != 0 records HIP events between the stages
 * of every later qtts_dev_codec_slot / _decode_host; stage_ms fills ms[5] in
 * that order for the last one (-1 when it was not timed). */
int qtts_dev_codec_timing(qtts_dev_t *dev, int on);
int qtts_dev_codec_stage_ms(const qtts_dev_t *dev, float *ms);

/* Several utterances' full codec decodes (a batch's slots; the reference
 * decodes its one utterance after the loop, Q.c:1376-1383, Cd.c:581-749):
 * job i decodes host_codes[i] ([T[i]][16] host ints) when host_codes and
 * host_codes[i] are non-NULL, else slot slot[i]'s first T[i] generated frames.
 * Up to QTTS_HIP_CODEC_LANES (default 8; fewer when their scratch would pass
 * 16 GB) decodes run side by side on their own
 * streams and scratch, each the same kernels as a lone decode (bit-identical
 * audio).  audio[i] (malloc'd host floats, T[i] * 1920 samples) and samples[i]
 * are filled; returns 0, or -1 with every audio[i] NULL. */
int qtts_dev_codec_multi(qtts_dev_t *dev, int n, const int *const *host_codes, const int *slot, const int *T,
                         float **audio, int *samples);

/* Streaming codec decode, exact and incremental (every codec op is causal:
 * conv histories, transposed-conv tails and the window-72 transformer K/V are
 * carried between pushes).  begin resets the stream (max_frames bounds the
 * total frames); a push decodes T more frames into T * 1920 host samples and
 * returns the sample count (< 0 on error).  push_slot reads slot b's generated
 * codes [frame0, frame0 + T) on the device (no host round trip). */
int qtts_dev_codec_stream_begin(qtts_dev_t *dev, int max_frames);
/* the same with the internal chunk sized for pushes of up to chunk_frames
 * frames at once (<= 16: the default 16) */
int qtts_dev_codec_stream_begin_ex(qtts_dev_t *dev, int max_frames, int chunk_frames);
/* push T host frames [T][16] through the stream on a second HIP stream without
 * waiting, audio dropped; every later stream call is ordered after it (the
 * voice-clone reference frames, overlapped with the prefill) */
int qtts_dev_codec_stream_prime(qtts_dev_t *dev, const int *codes, int T);
int qtts_dev_codec_stream_push_slot(qtts_dev_t *dev, int b, int frame0, int T, float *host_out);
int qtts_dev_codec_stream_push_host(qtts_dev_t *dev, const int *codes, int T, float *host_out);

/* n independent exact streams beside the single one (which these calls leave
 * alone), decoded together: a push runs the codec ONCE over the stacked
 * streams, so its kernel launches do not grow with n and every codec weight is
 * read once.  begin (n_streams 1..QWEN_TTS_MAX_BATCH) resets
 * every stream to position 0; on an active state of the same size it only
 * clears the carried state.  chunk_frames as qtts_dev_codec_stream_begin_ex
 * (internal passes of 16 frames by default, fewer where n_streams planes of
 * scratch would pass 2 GiB).  A push decodes T more frames of the n distinct
 * streams streams[0..n), which must all be at the same position, into T * 1920
 * host samples each (host_out[i] for streams[i]); the codes are slot slots[i]'s
 * generated frames [frame0, frame0 + T) on the device, or host codes
 * [n][T][16].  Returns the samples per stream, or -1 with a message, nothing
 * launched and the state untouched, for: n outside 1..n_streams, a stream
 * index out of range, a stream listed twice, streams at different positions,
 * T < 1, a push past max_frames, a push without begin (a re-allocation of the
 * context's state, e.g. another batch size, ends the streams: begin again).
 * pos: frames decoded so far of a stream, -1 for a bad index or no begin. */
int qtts_dev_codec_mstream_begin(qtts_dev_t *dev, int n_streams, int max_frames, int chunk_frames);
int qtts_dev_codec_mstream_push_slots(qtts_dev_t *dev, int n, const int *streams, const int *slots, int frame0, int T,
                                      float *const *host_out);
int qtts_dev_codec_mstream_push_host(qtts_dev_t *dev, int n, const int *streams, const int *codes, int T,
                                     float *const *host_out);
int qtts_dev_codec_mstream_pos(qtts_dev_t *dev, int stream);
/* The streams of one push at independent positions (the work queue: a
 * refilled slot's stream restarts at 0 while its neighbours continue).  Still
 * one launch sequence and one T for every stream of the push; each stacked
 * row takes its RoPE row, its K/V cache row and its attention window from its
 * own stream's position.  _push_host_any and _push_slots_at are _push_host and
 * _push_slots without the same-position refusal: the capacity is checked per
 * stream (a push in which any listed stream would pass max_frames is refused
 * and names that stream), and _push_slots_at takes slot slots[i]'s frames
 * [frame0[i], frame0[i] + T).  With every stream at one position they decode
 * bit for bit what _push_host / _push_slots decode.
 * reset: one stream back to position 0 (zero conv histories, no K/V rows),
 * stream-ordered, its neighbours untouched; 0, or -1 with a message and
 * nothing changed for a bad stream index or no begin (also after a
 * re-allocation of the context's state). */
int qtts_dev_codec_mstream_push_slots_at(qtts_dev_t *dev, int n, const int *streams, const int *slots,
                                         const int *frame0, int T, float *const *host_out);
int qtts_dev_codec_mstream_push_host_any(qtts_dev_t *dev, int n, const int *streams, const int *codes, int T,
                                         float *const *host_out);
int qtts_dev_codec_mstream_reset(qtts_dev_t *dev, int stream);
/* Ragged pushes: stream i of the push advances by its own counts[i] >= 1
 * frames, still in ONE launch sequence per internal pass whatever n and
 * however the counts differ ("Ragged pushes": a pass runs at the largest count
 * left, shorter streams are padded on the right of their plane, and the
 * codec's causality keeps the padding out of every valid column and out of
 * the carried state; a stream that has run out is no part of later passes).
 * _push_host_ragged: host codes [n][ld_frames][16], stream i's first
 * counts[i] rows; _push_slots_ragged: slot slots[i]'s frames [frame0[i],
 * frame0[i] + count[i]).  host_out[i] receives counts[i] * 1920 samples and
 * nothing beyond them.  Returns the LARGEST count times 1920.  With all counts
 * equal this is _push_host_any / _push_slots_at, the same code path, bit for
 * bit.  Refusals (-1, a message, nothing launched, no state changed) are
 * _push_host_any's, and: counts NULL, a count < 1, a count > ld_frames (slots:
 * frames outside the slot), a stream that would pass max_frames with its own
 * count (named).
 * _prime: the _push_host_ragged push with the audio dropped, enqueued on the
 * second HIP stream and not waited for: the reference frames of a
 * voice-clone batch, overlapped with the prefill as qtts_dev_codec_stream_prime
 * overlaps one utterance's.  Every later multi-stream (and codec) call on the
 * context joins it by event first; qtts_dev_codec_mstream_pos counts the primed
 * frames at once.  0 or -1 (the same refusals). */
int qtts_dev_codec_mstream_push_host_ragged(qtts_dev_t *dev, int n, const int *streams, const int *codes,
                                            const int *counts, int ld_frames, float *const *host_out);
int qtts_dev_codec_mstream_push_slots_ragged(qtts_dev_t *dev, int n, const int *streams, const int *slots,
                                             const int *frame0, const int *count, float *const *host_out);
int qtts_dev_codec_mstream_prime(qtts_dev_t *dev, int n, const int *streams, const int *codes, const int *counts,
                                 int ld_frames);
/* One stream's carried state saved and restored ("Snapshots"): a
 * stream primed once with a voice's reference frames is put into any stream
 * of any later begin in one launch instead of being primed again.  A snapshot
 * is a compact device buffer (the stream's planes of the 21 history slots,
 * then K / V rows 0..hl-1 of every layer, each part padded to 4 floats: 0.54 MB
 * + at most 4.65 MB at the 1.7B codec dims) and a host header (position, hl,
 * the codec dims, the device).  It holds nothing that depends on the stream
 * count or the pass size, so it survives a begin with other ones.
 * _save: a new snapshot of `stream`, the stream untouched; NULL on refusal.
 * _restore: writes the history planes and K/V rows 0..hl-1 of `stream` and
 *   takes over the snapshot's position and hl; rows at hl and above stay (as
 *   after a reset, none is inside a new row's window).
 * Both are ONE launch on the context stream, after a pending prime is joined
 * by event, and wait for nothing on the host.  Refusals (NULL / -1, a message,
 * nothing launched, stream and snapshot as they were): no begin or a state
 * re-allocated since; a bad stream index; a NULL or freed snapshot; a snapshot
 * saved on another context (or whose codec dims or device differ); a restore
 * whose position exceeds the begin's max_frames.
 * _snapshot_free: releases one (NULL, a freed pointer: nothing happens).
 * qtts_dev_destroy releases the device memory of the context's live snapshots;
 * they stay refusable and freeable.  _snapshot_pos / _snapshot_bytes: the
 * frames it stands at / its device bytes; -1 for a NULL, freed or orphaned one. */
typedef struct qtts_codec_snapshot qtts_codec_snapshot_t;
qtts_codec_snapshot_t *qtts_dev_codec_mstream_save(qtts_dev_t *dev, int stream);
int qtts_dev_codec_mstream_restore(qtts_dev_t *dev, int stream, const qtts_codec_snapshot_t *snap);
void qtts_dev_codec_snapshot_free(qtts_codec_snapshot_t *snap);
int qtts_dev_codec_snapshot_pos(const qtts_codec_snapshot_t *snap);
long long qtts_dev_codec_snapshot_bytes(const qtts_codec_snapshot_t *snap);

/* The same exact streaming decode overlapped with the decode loop: it runs on
 * a second (low-priority) HIP stream; push orders itself after the frames
 * already enqueued on the context stream (an event), decodes slot b's frames
 * [frame0, frame0 + T) into a device waveform and returns at once; end copies
 * `frames` * 1920 samples to host_out and waits.  Replaces the codec call
 * after the loop in qwen_tts_generate (Q.c:1376-1383) for one utterance. */
int qtts_dev_codec_async_begin(qtts_dev_t *dev, int max_frames);
int qtts_dev_codec_async_push(qtts_dev_t *dev, int b, int frame0, int T);
int qtts_dev_codec_async_end(qtts_dev_t *dev, float *host_out, int frames);

/* ---- voice-clone audio encoders (no c/ counterpart) ---- */
/* Encoder dimensions; call before the encoder tensors are put (speaker_encoder.*
 * of the model dir, encoder.* of speech_tokenizer/). */
int qtts_dev_enc_config(qtts_dev_t *dev, const qtts_enc_dims_t *dims);
/* bit 0: the speaker encoder is loaded, bit 1: the 12 Hz encoder is loaded */
int qtts_dev_enc_available(qtts_dev_t *dev);
/* Speaker x-vectors (extract_speaker_embedding, modeling_qwen3_tts.py:1941-1954)
 * of nb <= 16 host waveforms at 24 kHz (n[b] samples, > 384 each):
 * out[nb][enc_dim] host floats.  mel_out (optional) receives each utterance's
 * [128][T_b] log-mel back to back, T_b = (n[b] - 256) / 256 + 1. */
int qtts_dev_speaker_embed(qtts_dev_t *dev, int nb, const float *const *wav, const int *n, float *out,
                           float *mel_out);
/* 12 Hz reference codes (Qwen3TTSTokenizer.encode, qwen3_tts_tokenizer.py:208-257,
 * modeling_qwen3_tts_tokenizer_v2.py:961-991) of nb <= 16 host waveforms at
 * 24 kHz, zero-padded to the longest as the tokenizer's batch encode does:
 * codes[nb][max_frames][16] (host ints), frames[b] = ceil(n[b] / 1920).
 * latent (optional): [nb][hidden][max_frames] pre-quantizer embeddings. */
int qtts_dev_encode_audio(qtts_dev_t *dev, int nb, const float *const *wav, const int *n, int *codes,
                          int max_frames, int *frames, float *latent);

/* ---- host-pointer stage wrappers (oracle-level tests, c/qwen_tts.h:483-502) ---- */
int qtts_dev_talker_prefill_host(qtts_dev_t *dev, const float *embeds, int n, float *hidden_out);
int qtts_dev_talker_forward_host(qtts_dev_t *dev, const float *embed, float *logits, float *hidden_out);
int qtts_dev_subtalker_host(qtts_dev_t *dev, const float *hidden, int first_code, int *out_codes);
float *qtts_dev_codec_decode_host(qtts_dev_t *dev, const int *codes, int T, int *out_samples);

/* ---- kernel-level entry points (device buffers) ---- */
/* kernel_matvec_bf16 (c/qwen_tts_kernels.c:95): out[b*rows + r] = sum_c A[r,c] x[b*cols + c] */
int qtts_hip_matvec_bf16(float *out_dev, const uint16_t *A_dev, const float *x_dev, int rows, int cols,
                         int batch, void *stream);
/* kernel_rms_norm fused as a GEMV prologue; exported standalone for tests:
 * out = rmsnorm(x) @ A^T  (c/qwen_tts_kernels.c:27 + :95) */
int qtts_hip_rmsnorm_matvec_bf16(float *out_dev, const uint16_t *A_dev, const float *x_dev, const float *w_dev,
                                 float eps, int rows, int cols, int batch, void *stream);
/* the decode-loop GEMV dispatcher on `batch` lock-step rows (w_dev NULL: no norm):
 * batch 1 -> the batch-1 weight stream, 2..16 -> the batch GEMV planner's
 * choice of k_gemvb, else k_gemvm, on the matrix cores (else the generic
 * k_gemv), 17..64 -> the wide matrix-core batch kernel k_gemvx (one launch,
 * one weight read for all rows; -1 where it does not cover the shape: rows %
 * 16, cols % 32); qtts_hip_batch_matvec_plan reports the batch kernels' plan
 * (c/qwen_tts_kernels.c:27 + :95 per row) */
int qtts_hip_decode_matvec_bf16(float *out_dev, const uint16_t *A_dev, const float *x_dev, const float *w_dev,
                                float eps, int rows, int cols, int batch, void *stream);
/* the batch-1 GEMV of the sub-talker chain (weights resident in the Infinity
 * Cache, default cache policy): w_dev NULL: no norm; epi 0 store, 3 residual
 * (out += A x), 4 SwiGLU over interleaved gate|up row quads (rows/2 outputs)
 * (c/qwen_tts_kernels.c:27 + :95 + :213) */
int qtts_hip_resident_matvec_bf16(float *out_dev, const uint16_t *A_dev, const float *x_dev, const float *w_dev,
                                  float eps, int rows, int cols, int epi, void *stream);
/* kernel_sample_top_k (c/qwen_tts_kernels.c:407) on `batch` logit rows; rng_bits
 * holds the float-bit xorshift state per row (updated in place). */
int qtts_hip_sample_top_k(int *out_dev, const float *logits_dev, int vocab, int top_k, float top_p,
                          float temperature, uint32_t *rng_bits_dev, int batch, void *stream);
/* The same with one parameter set per row: top_k / top_p / temperature are
 * HOST arrays of `batch` entries.  Builds the per-slot parameter table and
 * launches the per-slot sampler family a run with these rows would hold
 * (fast-only when every row is fast-path eligible, else the general kernel;
 * QTTS_HIP_SAMPLE_W=0: always the general one); waits for the launch. */
int qtts_hip_sample_top_k_rows(int *out_dev, const float *logits_dev, int vocab, const int *top_k,
                               const float *top_p, const float *temperature, uint32_t *rng_bits_dev, int batch,
                               void *stream);
/* The sampler with the nucleus short list (k_sample_n.hip): a row with
 * top_p < 1 and top_k <= 64 or top-k off draws from at most 64 ids and one
 * sequential sum over the vocabulary, and runs the full path in the same
 * launch when the short list cannot decide; every other row draws as above.
 * Same ids and RNG states as qtts_hip_sample_top_k / _rows.  path_dev (may be
 * NULL) takes, per row, the path it ran: 1 fast top-k, 2 nucleus short list,
 * 3 full, 0 stopped.  QTTS_HIP_SAMPLE_NUCLEUS=0: no row tries the short list
 * (path 3 where it would have).  -1 without touching a device for a NULL
 * out / logits / rng (or host array), batch < 1, vocab outside 1..4096,
 * top_p <= 0 or a non-finite top_p / temperature.
 * qtts_hip_sample_nucleus: the parameters as launch arguments (the kernel a
 * run with a ctx-wide top_p < 1 launches).
 * qtts_hip_sample_nucleus_rows: one parameter set per row (HOST arrays), the
 * per-slot kernel; eos >= 0 && redraw: talker mode with a fixed length not
 * yet reached, so a row that draws `eos` is redrawn with that logit at -1e9
 * (c/qwen_tts.c:1315-1321), no suppression, no penalty; the entry owns the
 * scratch words of that mode.  Waits for the launch; not counted by
 * qtts_hip_sample_slot_launches. */
int qtts_hip_sample_nucleus(int *out_dev, const float *logits_dev, int vocab, int top_k, float top_p,
                            float temperature, uint32_t *rng_bits_dev, int batch, void *stream, int *path_dev);
int qtts_hip_sample_nucleus_rows(int *out_dev, int *path_dev, const float *logits_dev, int vocab, const int *top_k,
                                 const float *top_p, const float *temperature, uint32_t *rng_bits_dev, int batch,
                                 int eos, int redraw, void *stream);
/* kernel_causal_conv1d (c/qwen_tts_kernels.c:659): [ci, L] -> [co, L] */
int qtts_hip_causal_conv1d(float *out_dev, const float *in_dev, const float *w_dev, const float *b_dev, int ci,
                           int co, int k, int L, int dilation, int groups, void *stream);
/* kernel_transposed_conv1d (c/qwen_tts_kernels.c:873): [ci, L] -> [co, L*stride] */
int qtts_hip_transposed_conv1d(float *out_dev, const float *in_dev, const float *w_dev, const float *b_dev,
                               int ci, int co, int k, int stride, int L, void *stream);
/* kernel_snake_beta (c/qwen_tts_kernels.c:251), alpha/inv_beta pre-processed */
int qtts_hip_snake_beta(float *out_dev, const float *x_dev, const float *alpha_dev, const float *inv_beta_dev,
                        int channels, int length, void *stream);
/* The talker's decode attention (c/qwen_tts_talker.c:150-196 + kernel_causal_attention)
 * as a talker layer launches it: per row r, q / k RMSNorm + RoPE at pos[r], k / v
 * stored at row pos[r] of the caches [rows][S][KV*HD] (kv_dtype 0: fp32
 * elements, 1: bf16 bit patterns, uint16), attention over keys [0, pos[r]],
 * the kernel's own split merge.  qkv_dev [rows][(NH + 2 KV) HD], out_dev
 * [rows][NH HD], rope tables [>= max pos + 1][HD], pos_dev[r] in [0, S).  The
 * split scratch is allocated inside; returns after the launch has finished.
 * A parity entry, not a timing one: every call allocates and frees its
 * scratch and synchronises the stream twice, and it always uses the default
 * keys per split (QTTS_HIP_ATTN_LPK is a model-level switch). */
int qtts_hip_attn_decode(float *out_dev, const float *qkv_dev, void *kc_dev, void *vc_dev,
                         const float *qn_w_dev, const float *kn_w_dev,
                         const float *rope_cos_dev, const float *rope_sin_dev,
                         const int *pos_dev, int NH, int KV, int HD, int S, int rows,
                         float eps, int kv_dtype, void *stream);
/* The same with AttnArgs::skip: skip_dev [rows] (may be NULL), a nonzero flag
 * keeps row r from storing its k / v (a stopped slot); its output is still
 * computed, the token's own k / v included.  qtts_hip_attn_decode forwards
 * here with NULL.  NH == 2 KV with HD 16 / 32 / 64 / 128 runs the short kernel
 * (k_attn_short) at S <= 16 and the split kernel above it, everything else
 * the generic k_attn. */
int qtts_hip_attn_decode_ex(float *out_dev, const float *qkv_dev, void *kc_dev, void *vc_dev,
                            const float *qn_w_dev, const float *kn_w_dev,
                            const float *rope_cos_dev, const float *rope_sin_dev,
                            const int *pos_dev, int NH, int KV, int HD, int S, int rows,
                            float eps, int kv_dtype, const int *skip_dev, void *stream);
/* The cached attention (k_attn mode 1) behind the talker prefill, the codec
 * transformer and the voice-clone encoder: row r attends keys
 * [max(0, pos[r] + 1 - win), pos[r]] (win 0: [0, pos[r]]) of slot row_b[r] of
 * the caches [slots][S][KV*HD].  out_dev [rows][NH HD]; q_dev rows of stride
 * ld_q floats.
 * prep 1: the rows are fused q|k|v rows (ld_q >= (NH + 2 KV) HD);
 *   qtts_qk_prep runs first as the prefill issues it: q heads normalised and
 *   rotated in place, k (normalised, rotated) and v stored at (row_b[r],
 *   pos[r]); then the attention.  Needs the norm weights and RoPE tables.
 * prep 0: q is ready and the caches are filled (the norm weights and tables
 *   are not read and may be NULL).
 * pos_dev[r] in [0, S), row_b_dev[r] in [0, slots), HD in {8, 16, 32, 64, 128}.
 * -1 for kv_dtype 1 with a window (no bf16 window path).  A parity entry as
 * qtts_hip_attn_decode is. */
int qtts_hip_attn_cached(float *out_dev, float *q_dev, int ld_q, void *kc_dev, void *vc_dev,
                         const float *qn_w_dev, const float *kn_w_dev,
                         const float *rope_cos_dev, const float *rope_sin_dev,
                         const int *row_b_dev, const int *pos_dev, int NH, int KV, int HD, int S, int slots,
                         int rows, float eps, int win, int kv_dtype, int prep, void *stream);
/* The sub-talker's attention + O projection by kv head (k_attn_o), fp32 caches
 * [rows][S][KV*HD], no id table: part_dev[(g * rows + r) * R + i] =
 * Wo[i, 2 HD g .. 2 HD (g + 1)) . attention of kv head g's two query heads;
 * Wo_dev bf16 [R][NH*HD], 16-byte aligned.  Row r's k / v are stored at
 * pos_dev[r].  Returns 1 (nothing launched) for a shape the kernel does not
 * cover: NH != 2 KV, S > 16, HD outside 16 / 32 / 64 / 128. */
int qtts_hip_attn_o(float *part_dev, const float *qkv_dev, float *kc_dev, float *vc_dev,
                    const float *qn_w_dev, const float *kn_w_dev,
                    const float *rope_cos_dev, const float *rope_sin_dev, const int *pos_dev,
                    const uint16_t *Wo_dev, int R, int NH, int KV, int HD, int S, int rows, float eps,
                    void *stream);
/* The pair form of k_attn_o: rows 0 and 1 of one slot at positions 0 and 1 in
 * one launch.  qkv_dev [2][(NH + 2 KV) HD]; caches [S][KV*HD] (S >= 2), rows 0
 * and 1 are written and no row is read: row 1 takes key 0's k / v from row 0
 * as staged in the launch.  skip_dev (may be NULL): a nonzero skip_dev[0]
 * keeps both rows from being stored.  part_dev[(g * 2 + r) * R + i] as
 * qtts_hip_attn_o with rows = 2.  Returns 1 (nothing launched) for a shape the
 * kernel does not cover (those of qtts_hip_attn_o, and S < 2). */
int qtts_hip_attn_o_pair(float *part_dev, const float *qkv_dev, float *kc_dev, float *vc_dev,
                         const float *qn_w_dev, const float *kn_w_dev,
                         const float *rope_cos_dev, const float *rope_sin_dev, const int *skip_dev,
                         const uint16_t *Wo_dev, int R, int NH, int KV, int HD, int S, float eps,
                         void *stream);
/* The wave-per-row GEMV of the sub-talker chain with the chain's prologue, on
 * nrows = 1 (k_gemvw) or nrows = 2 (its pair form: one weight read for both x
 * rows) rows: x_dev [nrows][cols]; part_dev [n_part][nrows][cols] (NULL: none)
 * is summed in order and added to x; the sum goes to x_new_dev [nrows][cols]
 * (NULL: not stored); w_dev NULL: no norm; epi as
 * qtts_hip_resident_matvec_bf16; out_dev [nrows][rows] (epi 4: rows / 2).
 * Returns 1 (nothing launched) where the kernel does not cover the shape:
 * nrows 1 needs cols % 512 == 0 and rows % 1024 == 0; nrows 2 one of
 * (rows, cols) = (4096 | 6144 | 1024 | 2048, 1024), (1024, 3072); partials
 * need cols <= 1024. */
int qtts_hip_resident_matvec_rows_bf16(float *out_dev, const uint16_t *A_dev, const float *x_dev, const float *w_dev,
                                       float eps, int rows, int cols, int epi, const float *part_dev, int n_part,
                                       float *x_new_dev, int nrows, void *stream);
/* One lock-step batch decode GEMV with everything the decode frame hands the
 * batch kernels, on its own (a parity entry as qtts_hip_attn_decode is: it
 * allocates its split-K scratch, launches, synchronises, frees):
 *   y[b][r] = epi( inv[b] * sum_c A[r][c] * (xin[b][c] * norm_w[c]) ),  b < batch
 * batch 2..16 runs k_gemvb (else k_gemvm), 17..64 the wide kernel k_gemvx.
 *   src 0: xin = x_dev rows (stride ldx) + part_in_dev [n_part_in][batch][cols]
 *          summed in order first (NULL: none; 1..4);
 *   src 1 / 2: xin = row id(b) of a bf16 / fp32 table [*][cols], id(b) =
 *          ids_dev[ids_off + b * ids_bstride + row_sel_dev[b] * ids_rstride]
 *          (row_sel_dev NULL: no selector term).
 *   norm_w_dev NULL: no RMSNorm (inv = 1, norm_w = 1).  xcopy_dev [batch][cols]
 *   (NULL: none): xin as read (xcopy_normed 0) or normalised (1).
 *   epi 0 store, 1 +bias, 2 SiLU(+bias), 3 residual (y += ...), 4 SwiGLU over
 *   interleaved gate|up row quads (rows / 2 outputs); y rows at stride ldy.
 *   kz 0: no split-K; 2..4 workgroup columns over cols (epi 3 and src 0 without
 *   norm / xcopy only): self_reduce 1 -- the last column to finish a row block
 *   adds the partials in order into y (tickets kept by the library between
 *   calls, left zero by every launch); 0 -- consumer-add: the raw partials go
 *   to part_out_dev [kz][batch][rows] and y is not touched.
 * Returns 1 (nothing launched) where no batch kernel covers the case, -1 on an
 * argument or launch error. */
typedef struct {
    int rows, cols, batch;
    const uint16_t *A;                /* bf16 [rows][cols] */
    int src;
    const float *x; int ldx;
    const void *table;
    const int *ids; int ids_bstride, ids_rstride, ids_off;
    const int *row_sel;
    const float *part_in; int n_part_in;
    const float *norm_w; float eps;
    float *xcopy; int xcopy_normed;
    int epi;
    const float *bias;
    float *y; int ldy;
    int kz, self_reduce;
    float *part_out;
} qtts_bgemv_desc_t;
int qtts_hip_batch_matvec_case(const qtts_bgemv_desc_t *d, void *stream);
/* The planner's answer for that case: which batch kernel (kernel: 0 none, 1
 * k_gemvm, 2 k_gemvb, 4 k_gemvx), its n_tmpl template integers in the kernel's
 * order (the last is the source kind: 0 x rows, 1 x + partials, 2 bf16 table,
 * 3 fp32 table, 4 decided at run time), the launch geometry and the dynamic LDS
 * bytes; tpw / cch are k_gemvm's run-time arguments (tiles per workgroup,
 * staged column chunk; 0 for the others).  The same descriptor and the same
 * results as qtts_hip_batch_matvec_case (0 planned, 1 not covered, -1 error).
 * Host only: no pointer is dereferenced (their alignment is looked at) and no
 * device is needed. */
typedef struct {
    int kernel;
    int n_tmpl, tmpl[5];
    int src;
    int grid_x, grid_y, block;
    size_t lds_bytes;
    int tpw, cch;
} qtts_bgemv_plan_t;
int qtts_hip_batch_matvec_plan(const qtts_bgemv_desc_t *d, qtts_bgemv_plan_t *out);
/* One contraction of the codec's GEMM family (k_codec.hip: qtts_xgemm), as the
 * codec describes it to its dispatcher.  Modes (qtts_codec.h):
 *   amode 0 rows A[m*lda+k], 1 trans A[k*lda+m], 2 transposed-conv weights [ci][co][Kw];
 *   bmode 0 weights B[n*ldb+k], 1 causal conv over x[ic*ldb+t], 2 transposed conv;
 *   emode 0 store, 1 +bias[n], 2 gelu(+bias[n]), 3 silu(aux)*acc, 4 C += acc*vec[n],
 *         5 out[n][m] = acc+bias[n], 6 out[n][m] = (acc+bias[n])*vec[n]+res[n][m],
 *         7 conv +bias[m] (bias may be NULL), 8 +bias[m]+res[m][n], 9 snake(acc+bias[m]; ea, eb).
 * Convs: M = co, N = L, K = ci*Kw (causal) or ci*(Kw/stride) (transposed);
 * input columns t in [tmin, L) are read (tmin <= 0: history left of B).  All
 * pointers are device pointers. */
typedef struct {
    int M, N, K;
    int amode, bmode, emode;
    const float *A; int lda;
    const float *B; int ldb;
    int Kw, dil, pad, L, stride, tmin, co;
    const float *sa, *sb;             /* SnakeBeta (alpha, inv_beta) on the input channels, or NULL */
    float *C; int ldc;
    const float *bias, *vec, *aux, *res;
    int ldaux, ldres;
    const float *ea, *eb;             /* emode 9 */
} qtts_xgemm_desc_t;
/* kernels of the family, as path / path_out below */
enum {
    QTTS_XP_CONVB2 = 0,   /* k_convb<Kw,2>: bf16 3-plane conv, 64 x 128 tile */
    QTTS_XP_CONVB4 = 1,   /* k_convb<Kw,4>: 64 x 256 tile */
    QTTS_XP_CONV = 2,     /* k_conv<Kw>: fp32 MFMA conv */
    QTTS_XP_XLIN = 3,     /* k_xlin: bf16 3-plane linear */
    QTTS_XP_XGEMV = 4,    /* k_xgemv: linear at <= 4 rows */
    QTTS_XP_XGEMM = 5,    /* k_xgemm: generic */
};
/* The dispatcher's plan for the contraction with a split workspace of
 * part_elems floats (0: none): which kernel (path_out) and how many splits
 * (splits_out: input-channel splits of the conv kernels, K splits of k_xlin /
 * k_xgemm, summed by k_conv_reduce / k_xg_reduce; k_xgemv's in-block K slots).
 * force_path -1: the dispatcher's own choice; else that kernel if its
 * predicate covers the shape, 1 if not.  Transposed convs (bmode 2) are
 * planned as the model runs them: all phases in one conv launch, or one
 * k_xgemm per phase.  Host only: no pointer is dereferenced (their alignment
 * is looked at) and no device is needed. */
int qtts_hip_xgemm_plan(const qtts_xgemm_desc_t *d, size_t part_elems, int force_path, int *path_out,
                        int *splits_out);
/* Runs the contraction through that plan: allocates the workspace exactly
 * part_elems large, makes the re-laid conv weights and their bf16 planes as
 * qtts_hip_causal_conv1d does, launches, synchronises, frees.  Returns 1 and
 * launches nothing where force_path does not cover the shape, -1 on an error
 * (among them an epilogue operand the mode needs that is NULL).  A parity
 * entry, not a timing one. */
int qtts_hip_xgemm_case(const qtts_xgemm_desc_t *d, size_t part_elems, int force_path, int *path_out,
                        int *splits_out, void *stream);
/* The same over the conv forms' stream axis (the multi-stream codec): nseg
 * independent column segments of d->N columns each in one launch; segment s
 * reads its input at B + s*seg_ldb and writes C + s*seg_ldc (floats; an
 * in-place res moves with C).  A tile never holds two segments and taps left
 * of a segment read that segment's own margin.  The segments count as tiles
 * for the plan, so path_out / splits_out may differ from the single-segment
 * plan; nseg 1 is qtts_hip_xgemm_case.  Linear forms (bmode 0) take nseg 1
 * only.  Returns as qtts_hip_xgemm_case (1: force_path does not cover). */
int qtts_hip_xgemm_seg_case(const qtts_xgemm_desc_t *d, int nseg, int seg_ldb, int seg_ldc, size_t part_elems,
                            int force_path, int *path_out, int *splits_out, void *stream);
/* One multi-row projection of the prefill and prompt paths, as the runtime's
 * rows_proj hands it to the multi-row GEMMs (k_mgemm.hip, k_pgemm.hip):
 *   y[m][r] = epi( sum_c A[r][c] * xin[m][c] ),  m < rows, r < R
 *   src 0: xin = x rows (stride ldx floats); src 1: xin = row ids[m *
 *          ids_bstride] of a bf16 table [*][C];
 *   norm_w NULL: no RMSNorm, else xin[m][c] * inv[m] * norm_w[c] with
 *          inv[m] = 1 / sqrt(mean_c xin^2 + eps) (src 0 only);
 *   epi 0 store, 1 +bias, 2 SiLU(+bias), 3 residual (y += ...), 4 SwiGLU over
 *   interleaved gate|up row quads (R / 2 outputs); y rows at stride ldy.
 * The device scratch is the caller's: part (part_elems floats; NULL: no
 * split-K), planes (plane_elems bf16; NULL: no k_pgemm) and inv (>= rows
 * floats; needed with norm_w).  All pointers are device pointers. */
typedef struct {
    int rows, R, C;
    const uint16_t *A;                /* bf16 [R][C] */
    int src;
    const float *x; int ldx;
    const uint16_t *table;
    const int *ids; int ids_bstride;
    const float *norm_w; float eps;
    int epi;
    const float *bias;
    float *y; int ldy;
    float *part; size_t part_elems;
    uint16_t *planes; size_t plane_elems;
    float *inv;
} qtts_rows_gemm_desc_t;
/* the seven kernels, as qtts_rows_gemm_plan_t.kernel */
enum {
    QTTS_RG_MGEMM_1_1 = 0,   /* k_mgemm<1,1>: 2..16 rows */
    QTTS_RG_MGEMM_2_1 = 1,   /* k_mgemm<2,1>: 17..32 rows */
    QTTS_RG_MGEMM_4_1 = 2,   /* k_mgemm<4,1>: 33 rows and more, 64-row chunks on grid.y */
    QTTS_RG_MGEMM_4_2 = 3,   /* k_mgemm<4,2>: > 64 rows, 2 weight tiles per workgroup */
    QTTS_RG_MGEMM_4_4 = 4,   /* k_mgemm<4,4>: > 64 rows, 4 weight tiles per workgroup */
    QTTS_RG_PGEMM_2 = 5,     /* k_pgemm<2>: 128 x 128 tile */
    QTTS_RG_PGEMM_4 = 6,     /* k_pgemm<4>: 128 x 256 tile */
};
/* which kernel, its split-K columns (kz > 1: summed by k_mgemm_reduce), grid and block */
typedef struct {
    int kernel, kz;
    int grid_x, grid_y, grid_z, block;
} qtts_rows_gemm_plan_t;
/* The launch plan for the projection with a split workspace of part_elems
 * floats and plane scratch of plane_elems bf16 (0: none; d->part / d->planes
 * and their sizes are not looked at).  force -1: as the runtime's prefill
 * dispatches -- qtts_pgemm above 16 rows where it covers the shape, else
 * qtts_mgemm; 0: qtts_mgemm; 1 / 2: qtts_pgemm at tile width 128 / 256.
 * Returns 0 planned, 1 where the (forced) launcher does not cover the shape,
 * -1 on an argument error.  Host only: no pointer is dereferenced (their
 * alignment is looked at) and no device is needed. */
int qtts_hip_rows_gemm_plan(const qtts_rows_gemm_desc_t *d, size_t part_elems, size_t plane_elems, int force,
                            qtts_rows_gemm_plan_t *plan_out);
/* Runs the projection through that plan with the descriptor's own scratch,
 * synchronises and returns; plan_out (may be NULL) receives what ran.  Returns
 * 1 and launches nothing where the (forced) launcher does not cover the
 * shape, -1 on an argument or launch error.  A parity entry, not a timing one. */
int qtts_hip_rows_gemm_case(const qtts_rows_gemm_desc_t *d, int force, qtts_rows_gemm_plan_t *plan_out, void *stream);
/* snake(x) = x + inv_beta[c] * sin^2(x * alpha[c]) with the codec GEMMs' own
 * sin^2 (sin2 in k_codec.hip; qtts_hip_snake_beta runs sinf), and the fp32
 * expf / tanhf the GELU and SiLU epilogues call: fn 0 snake (needs alpha /
 * inv_beta per channel, x [channels][length]), 1 expf, 2 tanhf (channels = 1).
 * For measuring those functions against float64. */
int qtts_hip_xgemm_func(float *out_dev, const float *x_dev, const float *alpha_dev, const float *inv_beta_dev,
                        int channels, int length, int fn, void *stream);
/* One launch of the voice-clone encoders' contraction kernel (k_enc.hip:
 * k_econv through launch_econv), as the encoders describe it:
 *   y[b*yb + m*yc + n*yt] = epi( sum_k w[m][k] * x'(b, k, n) ),  k = c * kw + tap, m < M, n < lout[b]
 *   x'(b, k, n) = act_in( x[b*xb + c*xc + t*xt] (+ x2, same strides) ),  t = n*stride + tap*dil - padl,
 *                 t outside [0, lin[b]) remapped by pmode: 0 zero, 1 reflect, 2 replicate;
 *   act_in 0 none, 1 ELU;  epi: +bias[m], +bias2[b*bias2_b + m], act_out (0 none, 1 ReLU,
 *   2 tanh(ReLU), 3 exact GELU, 4 sigmoid), *vec[m], +res[b*rb + m*rc + n*rt]; NULL: absent.
 * w is fp32 [M][ci*kw]; part (optional) is the caller's split-K workspace of
 * part_elems floats, NULL: the entry allocates what the plan needs.  All
 * pointers are device pointers. */
typedef struct {
    int M, ci, kw, stride, dil, padl, pmode, act_in;
    const float *w;
    const float *x, *x2; size_t xb; int xc, xt;
    int lin[16], lout[16], nb, nmax;
    float *y; size_t yb; int yc, yt;
    const float *bias, *bias2; int bias2_b, act_out;
    const float *vec;
    const float *res; size_t rb; int rc, rt;
    float *part; size_t part_elems;
} qtts_econv_desc_t;
/* rows 1: the time-major fast path k_econv<true>, 0: the generic kernel; kz:
 * split-K factor (kz > 1: k_econv_reduce sums part_elems floats of partials) */
typedef struct {
    int rows, kz;
    int grid_x, grid_y, grid_z;
    size_t part_elems;
} qtts_econv_plan_t;
/* The launcher's plan for the descriptor.  Returns 0 planned, -1 for what the
 * launcher refuses: nb outside 1..16, M / ci / kw / nmax < 1, lout[b] outside
 * 0..nmax, reflect padding with padl >= lin[b] or lin[b] < 2.  Host only: no
 * pointer is dereferenced (x's alignment is looked at) and no device is needed. */
int qtts_hip_econv_plan(const qtts_econv_desc_t *d, qtts_econv_plan_t *plan_out);
/* Runs the launch: splits w into the three bf16 planes as the model load does
 * (k_ewsplit), launches through launch_econv, synchronises and frees what it
 * allocated.  plan_out (may be NULL) receives what ran.  -1 on a refusal (as
 * above, before any device call; also a part smaller than the plan needs or a
 * NULL w / x / y) or a device error.  A parity entry, not a timing one. */
int qtts_hip_econv_case(const qtts_econv_desc_t *d, qtts_econv_plan_t *plan_out, void *stream);
/* One launch of one of the encoders' small kernels through the launch helper
 * the encoders use.  in / out / n / s per op (device pointers; nb utterances,
 * len = int[nb] valid columns, ldt = row length of a [b][C][ldt] buffer):
 *   0 k_mel       in spec [b][2nf][ldt], len, fb [nm][nf], flo [nm], fhi [nm]; out mel [b][nm][ldt]; n nf, ldt, nb, nm (nf <= 1040)
 *   1 k_row_mean  in x, len; out [b][C]; n ldt, C, nb; s xb
 *   2 k_egemv     in W [R][Cc], x [b][ldx], bias or NULL; out y [b][ldy]; n R, Cc, ldx, act, ldy, nb
 *   3 k_se_apply  in h, s [b][C], res, len; out; n C, ldt, nb; s hb, rb, ob
 *   4 k_asp_stats in x, len; out [b][2C]; n ldt, C, nb; s xb
 *   5 k_asp_pool  in x, logits, len; out [b][2C]; n ldt, C, nb; s xb, lb
 *   6 k_ln_rows   in x [R][D], w, b; out y; n R, D; eps
 *   7 k_rope_bt   in cos [T][hd], sin; out x [R][ld] in place; n R, ld, nh, hd, T
 *   8 k_rows_bt   out row_b [R], pos [R] (int); n R, T
 *   9 k_rvq_enc   in lat [b][hid][T12], psemT [hid][vq], pacT, cbkT [q][vq][CB]; out codes [b][ldc_t][16] (int);
 *                 n T12, hid, rows, CB, vq, nvalid, nsem, ldc_t (hid, vq multiples of 16; nvalid <= 16) */
enum {
    QTTS_EO_MEL = 0, QTTS_EO_ROW_MEAN, QTTS_EO_EGEMV, QTTS_EO_SE_APPLY, QTTS_EO_ASP_STATS, QTTS_EO_ASP_POOL,
    QTTS_EO_LN_ROWS, QTTS_EO_ROPE_BT, QTTS_EO_ROWS_BT, QTTS_EO_RVQ_ENC, QTTS_EO_COUNT
};
typedef struct {
    int op;
    const void *in[6];
    void *out[2];
    int n[8];
    size_t s[3];
    float eps;
} qtts_enc_op_t;
/* Returns 0 launched (not synchronised), -1 refused before any device call
 * (unknown op, a NULL operand the op needs, a size below 1 or outside the
 * limits above) or on a launch error. */
int qtts_hip_enc_op(const qtts_enc_op_t *d, void *stream);
/* The fp32 erff (fn 0) / expm1f (fn 1) k_econv's GELU epilogue and ELU
 * prologue call, elementwise over n values, for measuring them against float64. */
int qtts_hip_enc_func(float *out_dev, const float *x_dev, size_t n, int fn, void *stream);
/* glibc-exact expf replica used by the sampler (for the libm cross-check test) */
int qtts_hip_expf_glibc(float *out_dev, const float *in_dev, int n, void *stream);
int qtts_hip_sync(void);
/* Sub-talker pair passes enqueued (or captured into a frame graph) since the
 * library loaded: positions 0 and 1 run as one two-row pass at batch 1
 * (QTTS_HIP_ST_PAIR=0 at creation: the 16 single-row passes). */
long long qtts_hip_st_pair_passes(void);
/* Launches of the wide batch GEMV (k_gemvx, 17..64 rows) enqueued (or captured
 * into a frame graph) since the library loaded: one per decode GEMV whatever
 * the slot count, none at 16 slots or fewer. */
long long qtts_hip_gemv_wide_launches(void);
/* Launches of the per-slot sampler (qtts_dev_slot_params) enqueued (or captured
 * into a frame graph) since the library loaded: one per code group and frame
 * with launch-per-op frames (QTTS_HIP_NO_GRAPH), none in a run that never
 * armed the table. */
long long qtts_hip_sample_slot_launches(void);

/* Diagnostics: run ONE frame eagerly on the current generation state with an
 * event pair around every kernel launch on the context stream.  kind[i]:
 * 0 talker GEMV, 1 sub-talker GEMV, 2 attention, 3 sampler, 4 embed-sum;
 * bytes[i]: algorithmic bytes of GEMV launches; ms[i]: measured duration;
 * names (optional, max*64 chars): kernel instantiation of launch i as
 * rocprofv3 names it (e.g. "k_gemv1<8, 2, true>").
 * Returns the number of kernels (<0 on error).  Advances the state by one
 * frame, so call it after a generation, not in the middle of one. */
int qtts_dev_profile_frame(qtts_dev_t *dev, int step, int max, int *kind, double *bytes, float *ms, char *names);
/* Measurement: the current device's HBM stream bandwidth over two `bytes`-sized
 * buffers (>> the 256 MB Infinity Cache): a non-temporal float4 read stream and
 * a float4 copy (read + write bytes), `iters` timed launches each with HIP
 * events on their own stream, GB/s (the roofline against a
 * bandwidth measured on the box beside the 8 TB/s nominal). */
int qtts_hip_hbm_bw(size_t bytes, int iters, double *read_gbs, double *copy_gbs);

#ifdef __cplusplus
}
#endif
#endif /* QTTS_HIP_H */
