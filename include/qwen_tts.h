/*
 * qwen_tts.h - public C API of the MI355X (gfx950) Qwen3-TTS hot path.
 *
 * Drop-in for the reference header c/qwen_tts.h: the same constants, the
 * same qwen_tts_config_t, the same public functions with the same
 * signatures, ownership and error behaviour (c/qwen_tts.h:448-502), and a
 * qwen_tts_ctx_t keeping every field name the reference CLI reads or writes
 * (config, generation parameters, progress callback, perf counters,
 * talker_kv_len; c/main.c:214-223,268-270,306-312).  Weights and all
 * generation state live on the GPU behind `hip` (include/qtts_hip.h); the
 * CPU-side weight/scratch fields of the reference struct are not present.
 *
 *   qwen_tts_load        NULL on failure, message on stderr
 *   qwen_tts_generate    malloc'd float32 PCM at 24 kHz, caller frees;
 *                        NULL and *out_samples = 0 on error
 *   qwen_tts_write_wav   0 / -1
 *
 * MI355X additions (not in the c/ reference): qwen_tts_load_on (device
 * choice per ctx; qwen_tts_load takes $QWEN_TTS_HIP_DEVICE or 0),
 * qwen_tts_generate_batch, qwen_tts_last_codes, streaming, text input, and
 * the Python reference's voice clone (codes / x-vector or reference audio).
 */
#ifndef QWEN_TTS_H
#define QWEN_TTS_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#define QWEN_TTS_SAMPLE_RATE      24000
#define QWEN_TTS_DECODE_UPSAMPLE  1920

/* defaults used when config.json omits a key (c/qwen_tts.h:25-78) */
#define QWEN_TTS_TALKER_VOCAB        3072
#define QWEN_TTS_TALKER_HIDDEN       1024
#define QWEN_TTS_TALKER_INTERMEDIATE 2048
#define QWEN_TTS_TALKER_LAYERS       20
#define QWEN_TTS_TALKER_HEADS        16
#define QWEN_TTS_TALKER_KV_HEADS     2
#define QWEN_TTS_TALKER_HEAD_DIM     64
#define QWEN_TTS_TALKER_TEXT_HIDDEN  2048
#define QWEN_TTS_TALKER_TEXT_VOCAB   151936
#define QWEN_TTS_NUM_CODE_GROUPS     32

#define QWEN_TTS_SUBTALKER_VOCAB        2048
#define QWEN_TTS_SUBTALKER_HIDDEN       1024
#define QWEN_TTS_SUBTALKER_INTERMEDIATE 3072
#define QWEN_TTS_SUBTALKER_LAYERS       5
#define QWEN_TTS_SUBTALKER_HEADS        16
#define QWEN_TTS_SUBTALKER_KV_HEADS     8
#define QWEN_TTS_SUBTALKER_HEAD_DIM     128

#define QWEN_TTS_CODEC_NUM_QUANTIZERS 16
#define QWEN_TTS_CODEC_CODEBOOK_SIZE  2048
#define QWEN_TTS_CODEC_HIDDEN         1024
#define QWEN_TTS_CODEC_LATENT         1024
#define QWEN_TTS_CODEC_LAYERS         8
#define QWEN_TTS_CODEC_HEADS          16
#define QWEN_TTS_CODEC_KV_HEADS       16
#define QWEN_TTS_CODEC_INTERMEDIATE   3072
#define QWEN_TTS_CODEC_SLIDING_WINDOW 72
#define QWEN_TTS_CODEC_DECODER_DIM    1536

#define QWEN_TTS_MAX_TALKER_LAYERS    32
#define QWEN_TTS_MAX_SUBTALKER_LAYERS 8
#define QWEN_TTS_MAX_CODEC_LAYERS     12

#define QWEN_TTS_TOKEN_IM_START  151644
#define QWEN_TTS_TOKEN_IM_END    151645
#define QWEN_TTS_TOKEN_ENDOFTEXT 151643
#define QWEN_TTS_TOKEN_TTS_PAD   151671
#define QWEN_TTS_TOKEN_TTS_BOS   151672
#define QWEN_TTS_TOKEN_TTS_EOS   151673

#define QWEN_TTS_CODEC_PAD       2148
#define QWEN_TTS_CODEC_BOS       2149
#define QWEN_TTS_CODEC_EOS       2150
#define QWEN_TTS_CODEC_THINK     2154
#define QWEN_TTS_CODEC_NOTHINK   2155
#define QWEN_TTS_CODEC_THINK_BOS 2156
#define QWEN_TTS_CODEC_THINK_EOS 2157

typedef struct {
    int talker_vocab_size;
    int talker_hidden;
    int talker_intermediate;
    int talker_layers;
    int talker_heads;
    int talker_kv_heads;
    int talker_head_dim;
    int talker_text_hidden;
    int talker_text_vocab;
    int num_code_groups;
    float talker_rms_norm_eps;
    float talker_rope_theta;
    int mrope_section[3];

    int subtalker_vocab_size;
    int subtalker_hidden;
    int subtalker_intermediate;
    int subtalker_layers;
    int subtalker_heads;
    int subtalker_kv_heads;
    int subtalker_head_dim;

    int codec_num_quantizers;
    int codec_codebook_size;
    int codec_codebook_dim;
    int codec_hidden;
    int codec_latent;
    int codec_layers;
    int codec_heads;
    int codec_kv_heads;
    int codec_intermediate;
    int codec_sliding_window;
    int codec_decoder_dim;
    float codec_rms_norm_eps;
    float codec_layer_scale;
    int codec_upsample_rates[4];
    int codec_upsampling_ratios[2];

    int n_speakers;
    char **speaker_names;
    int *speaker_ids;
    int n_languages;
    char **language_names;
    int *language_ids;

    int codec_pad_id;
    int codec_bos_id;
    int codec_eos_id;
    int codec_nothink_id;
    int codec_think_id;
    int codec_think_bos_id;
    int codec_think_eos_id;
} qwen_tts_config_t;

typedef void (*qwen_tts_progress_cb)(int step, int total, void *userdata);

typedef struct {
    qwen_tts_config_t config;
    char model_dir[512];

    /* device-resident model + generation state (include/qtts_hip.h) */
    void *hip;
    int hip_device;

    int talker_kv_len;          /* positions in the talker KV cache of slot 0 */
    float *tk_x;                /* host copy of the post-norm last talker hidden (stage API) */

    /* generation parameters (same names and defaults as the reference) */
    float temperature;
    float subtalker_temperature;
    int top_k;
    int subtalker_top_k;
    float top_p;
    float subtalker_top_p;
    float repetition_penalty;
    int max_new_tokens;
    int fixed_codec_tokens;
    int sample_seed;

    qwen_tts_progress_cb progress_cb;
    void *progress_cb_userdata;

    /* performance stats */
    double perf_total_ms;
    double perf_talker_ms;
    double perf_codec_ms;
    int perf_codec_tokens;

    /* MI355X additions */
    double perf_prefill_ms;
    double perf_first_frame_ms;  /* generate() entry -> first frame's codes on device */
    int *last_codes;             /* [last_frames][num_code_groups] of the last call (slot 0) */
    int last_frames;
    int last_stop_reason;        /* 1 eos, 2 max_tokens */
    int last_stop_step;
    double perf_first_packet_ms; /* qwen_tts_generate_stream(): entry -> first audio chunk delivered */
    void *tokenizer;             /* Qwen2 BPE of the model dir, loaded on first text input */
    /* the last qwen_tts_generate_queue, per utterance in input order */
    int queue_n;
    int **queue_codes;           /* [queue_n] [frames][num_code_groups] (NULL: not taken by this ctx) */
    int *queue_frames;           /* frames generated (-1: not taken) */
    int *queue_stop_reason;      /* 1 eos, 2 max_tokens */
    int *queue_slot;             /* the slot it decoded on */
    int queue_slots;             /* lock-step slots the run used */
    int queue_frames_launched;   /* lock-step frames launched */
    int queue_refills;           /* utterances admitted into a slot freed mid-run */
    long long queue_slot_frames_used; /* sum of frames generated */
    long long queue_rows_launched;    /* sum over launched frames of the slot rows they ran (the tail launches
                                         only the running slots): occupancy = frames_used / rows_launched */
    void *instruct;              /* per-utterance instruct ids armed for the next generation call (one-shot;
                                    qwen_tts_set_utterance_instruct).  It sits in front of `sampling` */
    void *sampling;              /* per-utterance sampling armed for the next generation call (one-shot;
                                    qwen_tts_set_utterance_sampling).  It sits in front of `force`, which
                                    stays the struct's last field */
    void *force;                 /* forced codes / taps armed for the next generation call (one-shot) */
} qwen_tts_ctx_t;

qwen_tts_ctx_t *qwen_tts_load(const char *model_dir);
void qwen_tts_free(qwen_tts_ctx_t *ctx);
void qwen_tts_set_progress_callback(qwen_tts_ctx_t *ctx, qwen_tts_progress_cb cb, void *userdata);
float *qwen_tts_generate(qwen_tts_ctx_t *ctx, const char *text, const char *speaker, const char *language,
                         int *out_samples);
int qwen_tts_write_wav(const char *path, const float *samples, int n_samples, int sample_rate);

static inline float bf16_to_f32(uint16_t bf16) {
    uint32_t f32_bits = ((uint32_t)bf16) << 16;
    float result;
    __builtin_memcpy(&result, &f32_bits, sizeof(float));
    return result;
}

/* stage functions (host pointers; c/qwen_tts.h:483-502) */
void qwen_tts_talker_prefill(qwen_tts_ctx_t *ctx, const float *input_embeds, int seq_len);
void qwen_tts_talker_forward(qwen_tts_ctx_t *ctx, const float *input_embed, float *logits);
void qwen_tts_subtalker_generate(qwen_tts_ctx_t *ctx, const float *talker_hidden, int first_code, int *out_codes);
float *qwen_tts_codec_decode(qwen_tts_ctx_t *ctx, const int *codes, int time_steps, int *out_samples);

/* post-final-norm hidden of the last talker token (the reference's ctx->tk_x) */
int qwen_tts_talker_hidden(qwen_tts_ctx_t *ctx, float *out);

/* ---- MI355X additions ---- */
/* qwen_tts_load on HIP device `device` (< 0: $QWEN_TTS_HIP_DEVICE or 0, which
 * is what qwen_tts_load uses).  No process-global state: one ctx per device
 * and host thread, each owning its device model, streams and graphs. */
qwen_tts_ctx_t *qwen_tts_load_on(const char *model_dir, int device);
/* Element type of the talker KV cache.  QWEN_TTS_KV_F32 (the default) keeps
 * the codes bit-exact against the reference.  QWEN_TTS_KV_BF16 stores every K
 * and V row of the talker rounded to bf16 (nearest even): half the cache bytes
 * (114,688 instead of 229,376 B per position and slot on the 1.7B model), the
 * attention arithmetic itself stays fp32, and the codes are no longer
 * bit-exact against the reference (the Python reference runs its cache in
 * bf16 too).  Takes effect with the next generation call; -1 on a bad value.
 * $QTTS_HIP_KV=bf16|fp32 sets the default of every ctx loaded after it. */
#define QWEN_TTS_KV_F32  0
#define QWEN_TTS_KV_BF16 1
int qwen_tts_set_kv_cache_dtype(qwen_tts_ctx_t *ctx, int dtype);
int qwen_tts_kv_cache_dtype(qwen_tts_ctx_t *ctx);
/* Most lock-step slots of one ctx (qwen_tts_generate_batch, the slots of
 * qwen_tts_generate_queue, qwen_tts_generate_voice_clone_batch): up to 16 run
 * on the 16-row matrix-core batch kernels, 17..64 on the wide batch kernel. */
#define QWEN_TTS_MAX_BATCH 64
/* nb (1..QWEN_TTS_MAX_BATCH) utterances in lock-step frames on this ctx's GPU
 * (weights read once per frame for all of them).  out_audio[i] malloc'd
 * (caller frees), out_samples[i] set; returns 0 when every utterance produced
 * audio, -1 with a message for nb above the limit, before the device is
 * touched. */
int qwen_tts_generate_batch(qwen_tts_ctx_t *ctx, int nb, const char *const *texts, const char *const *speakers,
                            const char *const *languages, float **out_audio, int *out_samples);
/* Work queue (no c/ counterpart): nq utterances on at most nb
 * (1..QWEN_TTS_MAX_BATCH; -1 with a message above it, before the device is
 * touched) lock-step slots.  When a slot's utterance stops (EOS, or max_new_tokens /
 * fixed_codec_tokens frames), the next queued utterance is prefilled into that
 * slot inside the live batch, so a batch of EOS-variable lengths keeps its
 * slots busy instead of riding stopped rows to the longest one.  Each
 * utterance decodes as it would alone (own KV positions, counters, repetition
 * counts, RNG states from sample_seed).  `next` (optional) picks the utterance
 * to admit: it returns an index in [0, nq) not yet taken, or -1 when there is
 * none (e.g. a counter shared by the processes of several GPUs); NULL takes
 * them in order.  out_audio[i] / out_samples[i] (input order) are filled for
 * the utterances this ctx took (NULL / 0 for the others); codes and stop
 * reasons stay in ctx->queue_* until the next call.  Returns 0 when every
 * utterance taken produced audio. */
typedef int (*qwen_tts_queue_next_cb)(void *userdata);
int qwen_tts_generate_queue(qwen_tts_ctx_t *ctx, int nq, const char *const *texts, const char *const *speakers,
                            const char *const *languages, int nb, qwen_tts_queue_next_cb next, void *userdata,
                            float **out_audio, int *out_samples);
/* codes of utterance i of the last qwen_tts_generate_queue: copies up to
 * max_frames rows (codes may be NULL to query), returns the frame count, -1 if
 * this ctx did not decode it */
int qwen_tts_queue_codes(qwen_tts_ctx_t *ctx, int i, int *codes, int max_frames);
/* Voice clone (no c/ counterpart: the Python reference's generate_voice_clone,
 * qwen3_tts_model.py:506-630, modeling_qwen3_tts.py:1967-2232) from the 12 Hz
 * codes of the reference audio (ref_codes [n_ref_frames][16]) and/or the
 * speaker encoder's x-vector (spk_embed [talker hidden]); to start from the
 * reference AUDIO, use qwen_tts_generate_voice_clone_audio[_batch] below, which
 * run the encoders on the device first.
 *   ICL mode  : ref_codes + ref_text (ids CSV of
 *               "<|im_start|>assistant\n{ref}<|im_end|>\n"), spk_embed optional;
 *               the audio is decoded from reference ++ generated codes and the
 *               reference part cut off, as the Python reference does.
 *   x-vector  : ref_codes NULL / n_ref_frames 0, spk_embed set.
 * non_streaming selects the non-streaming text layout.  Returns malloc'd PCM
 * (caller frees); NULL on error. */
float *qwen_tts_generate_voice_clone(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                     const int *ref_codes, int n_ref_frames, const float *spk_embed,
                                     const char *language, int non_streaming, int *out_samples);
/* Streaming voice clone (as qwen_tts_generate_stream, after the type below):
 * the reference frames are pushed through the exact streaming codec first, so
 * chunks start at the reference boundary (sample n_ref_frames * 1920 of the
 * reference ++ generated decode).  The non-streamed call cuts at the Python
 * reference's float position int(ref / total * samples), which for ~5 % of
 * (ref, total) pairs is one sample earlier. */
/* nb (1..QWEN_TTS_MAX_BATCH; -1 with a message above it) voice-clone
 * utterances in lock-step frames (BASELINE C5: batch 8 on one GPU); per-slot
 * arrays as above (ref_codes[b] / spk_embeds[b] may be NULL).
 * Returns 0 when every utterance produced audio. */
int qwen_tts_generate_voice_clone_batch(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                        const char *const *ref_texts, const int *const *ref_codes,
                                        const int *n_ref_frames, const float *const *spk_embeds,
                                        const char *const *languages, int non_streaming, float **out_audio,
                                        int *out_samples);
/* Voice clone from reference AUDIO (the Python reference's
 * create_voice_clone_prompt, qwen3_tts_model.py:356-458, on the device).
 * Waveforms are mono float PCM at 24 kHz (the reference resamples other rates
 * with librosa first; here the caller resamples with qwen_tts_resample below,
 * as the CLI's --ref-audio does for other rates).  The model directory
 * must hold the speaker encoder (speaker_encoder.* + speaker_encoder_config)
 * and the 12 Hz tokenizer encoder (speech_tokenizer/ encoder.* +
 * encoder_config).
 * qwen_tts_speaker_embedding: the x-vector of extract_speaker_embedding
 *   (modeling_qwen3_tts.py:1941-1954: 128-bin log-mel, ECAPA-TDNN), malloc'd
 *   [talker hidden] floats, *out_dim set; NULL on error (> 384 samples needed).
 * qwen_tts_encode_audio: the 12 Hz codes of Qwen3TTSTokenizer.encode
 *   (modeling_qwen3_tts_tokenizer_v2.py:961-991: Mimi encoder, first 16
 *   codebooks), malloc'd [ceil(n / 1920)][16] ints, *out_frames set.
 * qwen_tts_generate_voice_clone_audio[_batch]: encode (all references in one
 *   zero-padded batch, as the tokenizer does) + qwen_tts_generate_voice_clone
 *   [_batch]; ICL mode needs ref_text, x_vector_only drops the codes.  The
 *   batch form stays at 1..16 utterances, the encoders' batch (not
 *   QWEN_TTS_MAX_BATCH): encode larger sets in groups and decode them with
 *   qwen_tts_generate_voice_clone_batch.
 * All return NULL / -1 on error with a message on stderr; buffers are the
 * caller's to free(). */
float *qwen_tts_speaker_embedding(qwen_tts_ctx_t *ctx, const float *wav, int n_samples, int *out_dim);
int *qwen_tts_encode_audio(qwen_tts_ctx_t *ctx, const float *wav, int n_samples, int *out_frames);
float *qwen_tts_generate_voice_clone_audio(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                           const float *ref_wav, int n_ref_samples, const char *language,
                                           int x_vector_only, int non_streaming, int *out_samples);
int qwen_tts_generate_voice_clone_audio_batch(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                              const char *const *ref_texts, const float *const *ref_wavs,
                                              const int *n_ref_samples, const char *const *languages,
                                              const int *x_vector_only, int non_streaming, float **out_audio,
                                              int *out_samples);
/* audio chunk callback of the streaming calls (qwen_tts_generate_stream below) */
typedef void (*qwen_tts_audio_cb)(const float *pcm, int n_samples, void *userdata);
/* streaming form: encode, then qwen_tts_generate_voice_clone_stream; the
 * first-packet time counts from this call's entry (encode included) */
float *qwen_tts_generate_voice_clone_audio_stream(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                                  const float *ref_wav, int n_ref_samples, const char *language,
                                                  int x_vector_only, int non_streaming, int chunk_frames,
                                                  qwen_tts_audio_cb cb, void *userdata, int *out_samples);
/* Resample mono PCM from sr_in to sr_out Hz (reference audio at another rate;
 * the Python reference resamples to 24 kHz with librosa, qwen3_tts_model.py:
 * 441-444): librosa's "polyphase" method = scipy.signal.resample_poly (Kaiser
 * windowed-sinc FIR, ceil(n * sr_out / sr_in) samples).  malloc'd, *n_out set;
 * NULL on error. */
float *qwen_tts_resample(const float *in, int n_in, int sr_in, int sr_out, int *n_out);
/* codes of the last generate() (slot 0): copies up to max_frames rows of
 * num_code_groups ints, returns the frame count */
int qwen_tts_last_codes(qwen_tts_ctx_t *ctx, int *codes, int max_frames);
/* the same for slot `slot` of the last qwen_tts_generate_batch (slot 0 ==
 * qwen_tts_last_codes); -1 on a bad slot */
int qwen_tts_last_codes_slot(qwen_tts_ctx_t *ctx, int slot, int *codes, int max_frames);
/* Teacher-forced decode (no c/ counterpart: the reference only samples and
 * continues).  Resume or extend an utterance from codes already at hand, pin
 * its first frames, replay a recorded run, or ask what the model would have
 * drawn under a given history.  Served by every generation call but
 * qwen_tts_generate_queue (single, batch, stream, voice clone).
 * qwen_tts_force_codes: slot `slot` of the next call continues on
 *   codes[n_frames][num_code_groups]; an entry < 0 leaves that draw free, and
 *   so are the frames >= n_frames.  Every draw still runs exactly as it would
 *   (suppression, repetition penalty, the fixed-length EOS redraw, every RNG
 *   advance); a forced entry then replaces its result, and the stored code,
 *   the repetition counts, the sub-talker's and the talker's next inputs and
 *   the stop follow the replaced id (a forced EOS stops the slot, a forced
 *   non-EOS continues where the free draw was EOS).  Group-0 ids must lie in
 *   [0, vocab - 1024) or be EOS, the other groups' in [0, sub-talker vocab).
 * qwen_tts_tap_draw: records the sampler's inputs at draw (frame, group) of
 *   `slot`; at most 8 per run; returns the tap's index.
 * Arming is ONE-SHOT: the next generate* call consumes it whether it succeeds
 * or not (qwen_tts_generate_queue refuses with -1 and disarms), so a ctx shared
 * between callers cannot inherit it.  That call fails before launching when a
 * slot is >= its batch size, more frames are forced than it generates
 * (max_new_tokens / fixed_codec_tokens), or a tap lies past them.
 * qwen_tts_last_drawn: the free-draw record of the last armed call -- the id
 *   the sampler itself produced at every draw, [frames][num_code_groups], -1
 *   where no draw happened (after a stop; the groups after a forced EOS).
 *   With a reference run's codes forced this is a per-draw parity check under
 *   the reference's own history.  Copies up to max_frames rows, returns the
 *   rows copied; -1 when the last call was not armed.
 * qwen_tts_tap_result: tap i's values -- group 0 after suppression and
 *   repetition penalty, before the temperature division and untouched by the
 *   EOS redraw; groups >= 1 the raw head output; up to max_n of the n real
 *   entries -- the RNG state before the draw and the free-drawn id (each may be
 *   NULL).  Returns n, or -1 if the draw never happened.
 * Both stay readable until the next generation call.  Errors return -1 with a
 * message on stderr. */
int qwen_tts_force_codes(qwen_tts_ctx_t *ctx, int slot, const int *codes, int n_frames);
int qwen_tts_tap_draw(qwen_tts_ctx_t *ctx, int slot, int frame, int group);
int qwen_tts_last_drawn(qwen_tts_ctx_t *ctx, int slot, int *codes, int max_frames);
int qwen_tts_tap_result(qwen_tts_ctx_t *ctx, int i, float *logits, int max_n, unsigned *rng_bits, int *drawn);
/* Per-utterance sampling parameters and seeds (no c/ counterpart: the
 * reference decodes one utterance per call with the ctx's parameters).  N
 * takes of one prompt with N seeds, or requests with different temperature /
 * top-k / top-p / repetition penalty, share one lock-step batch or one work
 * queue; every utterance decodes bit for bit as it would alone with its own
 * parameters and seed, whatever slot it lands in and whatever the other slots
 * draw.  max_new_tokens and fixed_codec_tokens stay the ctx's for all.
 * qwen_tts_sampling_defaults: fills *s from the ctx's current fields (the
 *   values an unarmed call uses).
 * qwen_tts_set_utterance_sampling: per[i] is for utterance i of the NEXT
 *   generation call -- slot i of a batch / voice-clone batch, utterance i
 *   (input order, whatever slot and admission order) of
 *   qwen_tts_generate_queue, per[0] of the single-utterance and stream calls.
 *   The values are checked here: -1 with a message for n < 1, a non-finite
 *   value, top_p / subtalker_top_p <= 0 or repetition_penalty <= 0 (an earlier
 *   arming stays as it was).  temperature <= 0 samples at 1e-5, top_k <= 0 or
 *   >= the vocabulary means no top-k, as in the reference.
 * Arming is ONE-SHOT, as for qwen_tts_force_codes: the next generate* call
 * consumes it whether it succeeds or not.  That call fails with -1 before the
 * device is touched when n differs from its utterance count (nb, nq, or 1), or
 * when forced codes / taps are armed as well (both are disarmed: the
 * combination is not supported). */
typedef struct {
    float temperature, top_p, repetition_penalty;
    int top_k;
    float subtalker_temperature, subtalker_top_p;
    int subtalker_top_k;
    int sample_seed;
} qwen_tts_sampling_t;
int qwen_tts_sampling_defaults(const qwen_tts_ctx_t *ctx, qwen_tts_sampling_t *s);
int qwen_tts_set_utterance_sampling(qwen_tts_ctx_t *ctx, int n, const qwen_tts_sampling_t *per);
/* Instruct (style control) and voice design: the Python reference's
 * generate_custom_voice(..., instruct=...) and generate_voice_design.  The ids
 * of "<|im_start|>user\n{instruct}<|im_end|>\n" (qwen_tts_instruct_prompt) go
 * through the text projection and stand in front of the ordinary prompt rows
 * (modeling_qwen3_tts.py:2075-2080, 2236-2237); nothing else changes.  Voice
 * design is the same call with `speaker` NULL or "" on a *-VoiceDesign
 * checkpoint.
 * qwen_tts_set_utterance_instruct: instruct_ids[i] is the comma-separated id
 *   list for utterance i of the NEXT generation call (slot i of a batch,
 *   utterance i in input order of the queue, entry 0 of the single and stream
 *   calls); a NULL or empty entry: no instruct for that utterance.  One-shot
 *   like per-utterance sampling, and free to combine with it and with forced
 *   codes / taps.  Refused (-1, an earlier arming stays) for n < 1, a NULL
 *   list, an entry that does not parse or an id outside [0, text vocab).
 *   Served by qwen_tts_generate, _stream, _batch, _batch_stream, _queue and
 *   _queue_stream; a call of another utterance count fails with -1 before the
 *   device is touched, and every voice-clone entry and the voice queue refuse
 *   an armed instruct (-1); both disarm.
 * The library applies what it is given: it does not read tts_model_size (the
 * Python wrapper drops the instruct on the 0.6B CustomVoice checkpoint). */
int qwen_tts_set_utterance_instruct(qwen_tts_ctx_t *ctx, int n, const char *const *instruct_ids);
/* Streaming generation (the reference has only a per-step
 * progress callback, c/qwen_tts.h:356): audio is decoded incrementally and
 * exactly (qtts_hip.h codec stream) and handed to `cb` as it is produced --
 * the first chunk after frame 0 (1920 samples, 80 ms), then every
 * `chunk_frames` frames, then the tail.  Returns the whole utterance like
 * qwen_tts_generate (malloc'd, caller frees); NULL on error. */
float *qwen_tts_generate_stream(qwen_tts_ctx_t *ctx, const char *text, const char *speaker, const char *language,
                                int chunk_frames, qwen_tts_audio_cb cb, void *userdata, int *out_samples);
float *qwen_tts_generate_voice_clone_stream(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                            const int *ref_codes, int n_ref_frames, const float *spk_embed,
                                            const char *language, int non_streaming, int chunk_frames,
                                            qwen_tts_audio_cb cb, void *userdata, int *out_samples);
/* Incremental codec decode of host codes [time_steps][16]: begin, then push
 * any number of frames at a time; each push writes time_steps * 1920 samples
 * to `out` and returns that count (-1 on error).  The concatenation equals
 * qwen_tts_codec_decode of all frames at once. */
int qwen_tts_codec_stream_begin(qwen_tts_ctx_t *ctx, int max_frames);
int qwen_tts_codec_stream_push(qwen_tts_ctx_t *ctx, const int *codes, int time_steps, float *out);

/* Streaming for every utterance of a lock-step batch.  Semantics are
 * qwen_tts_generate_batch's (the same prompts, decode loop and codes bit for
 * bit, the same nb limit and refusals, forced codes / taps and per-utterance
 * sampling consumed the same way); the audio comes as qwen_tts_generate_stream
 * delivers it, per utterance: cb(i, pcm, n, userdata) after frame 0, then every
 * chunk_frames frames, then the tail.  All utterances' chunks of one poll are
 * decoded together by the multi-stream exact codec (qtts_hip.h), so the codec
 * work per chunk does not multiply its kernel launches by nb.  In EOS mode an
 * utterance that stops gets its remaining frames at the next poll and no
 * callback after that; the call returns when every utterance has stopped.
 * out_audio[i] (malloc'd, caller frees) is the concatenation of utterance i's
 * chunks.  perf_first_packet_ms: entry -> the last callback of the first
 * chunks; perf_codec_ms: time in the codec pushes (perf_talker_ms excludes it).
 * The work queue streams through qwen_tts_generate_queue_stream below, the
 * voice-clone batch through qwen_tts_generate_voice_clone_batch_stream. */
typedef void (*qwen_tts_batch_audio_cb)(int utterance, const float *pcm, int n_samples, void *userdata);
int qwen_tts_generate_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                   const char *const *speakers, const char *const *languages, int chunk_frames,
                                   qwen_tts_batch_audio_cb cb, void *userdata, float **out_audio, int *out_samples);
/* Incremental text input: a streaming decode that takes its content ids while
 * it runs (an LLM producing the text).  The model is a dual-track streamer:
 * the prefill holds the role ids, the codec prefix and the FIRST content id;
 * every later content id is one "trailing" row, added to the talker input of
 * one frame (DESIGN.md "Incremental text input": the frame that draws frame r
 * adds the row of content id r + 1, or tts_eos behind the last id).  Fed ids
 * are the content ids alone; the library supplies the chat template's role ids
 * and the tts_eos row.
 *
 * The feed callback is called with wait = 0 before every frame launch (push
 * what is at hand, possibly nothing; it adds no device wait) and with
 * wait = 1 when no live utterance can advance (block until you have pushed or
 * closed something).  Return 0 to go on, < 0 to abort the call.
 * qwen_tts_feed_ids / _close are valid only inside the callback and return -1
 * with a message for a bad utterance index, an id outside [0, text vocab) and
 * a push after the utterance was closed; after the utterance has stopped (EOS
 * or the frame limit) they return 0 and do nothing.  qwen_tts_feed_state: the
 * ids taken, the frames launched for the utterance, and whether its next frame
 * lacks its row (any output may be NULL).
 *
 * Start: before the prefill the callback is called with wait = 1 until every
 * utterance has an id; one closed with none fails the call before the device
 * is touched.  Frame 0 is the lock-step head on the prefill's hidden states,
 * so it is launched once every utterance has its second id or is closed (the
 * first packet needs two ids, or one id and a close); until then the callback
 * is called with wait = 1.
 * Holds: a frame runs whole or not at all for a slot.  A slot whose next frame
 * lacks its row, the text still open, is held for that frame exactly as a
 * stopped slot is -- no draw, no RNG advance, no code row, no KV position --
 * and tried again at the next launch.  (Deferring only the embedding sum, so
 * that a frame's draw runs before its row arrives, is out of scope.)
 * When every live utterance is starved, everything decoded and not yet
 * delivered goes out as audio chunks first, then the callback is called with
 * wait = 1; one that returns 0 without a push or close for a starved live
 * utterance fails the call ("feed made no progress").  Otherwise the delivery
 * is qwen_tts_generate_batch_stream's: frame 0, then every chunk_frames, then
 * the tail; starvation flushes add short chunks, every chunk a multiple of
 * 1920 samples; out_audio[i] is the concatenation of utterance i's chunks.
 * Fixed and EOS mode both work; an utterance ends at its EOS or frame limit.
 * For the same ids every feed schedule gives the same codes bit for bit, in
 * any slot, whatever the other slots are fed.  Against the unfed call on the
 * whole template there is no bit guarantee (the unfed text projection changes
 * kernel with the row count); the layout is the same.
 * Per-utterance sampling and instructs are consumed as
 * qwen_tts_generate_batch_stream consumes them; armed forced codes / taps are
 * refused (-1, disarmed).  Voice clone and the two queues have no fed form.
 * -1 (NULL) and no audio on any failure, a callback's abort included; the next
 * call on the context is not affected. */
typedef struct qwen_tts_feed qwen_tts_feed_t;
typedef int (*qwen_tts_text_feed_cb)(qwen_tts_feed_t *feed, int wait, void *userdata);
int qwen_tts_feed_ids(qwen_tts_feed_t *feed, int utterance, const int *ids, int n);
int qwen_tts_feed_close(qwen_tts_feed_t *feed, int utterance);
int qwen_tts_feed_state(const qwen_tts_feed_t *feed, int utterance, int *ids_taken, int *frames_done, int *starved);
float *qwen_tts_generate_fed_stream(qwen_tts_ctx_t *ctx, const char *speaker, const char *language, int chunk_frames,
                                    qwen_tts_text_feed_cb feed_cb, void *feed_userdata, qwen_tts_audio_cb audio_cb,
                                    void *audio_userdata, int *out_samples);
int qwen_tts_generate_fed_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *speakers,
                                       const char *const *languages, int chunk_frames, qwen_tts_text_feed_cb feed_cb,
                                       void *feed_userdata, qwen_tts_batch_audio_cb audio_cb, void *audio_userdata,
                                       float **out_audio, int *out_samples);
/* qwen_tts_generate_voice_clone_batch with every utterance streamed.  Prompts,
 * decode loop, the nb limit, refusals and the one-shot armings are that
 * call's and the codes are its codes bit for bit; the delivery per utterance
 * is qwen_tts_generate_batch_stream's (frame 0, then every chunk_frames
 * frames, then the tail; the perf_* fields defined the same way).  Each slot
 * has a multi-stream codec stream of its own; the reference frames of all ICL
 * slots are run through them first, their audio dropped, in ONE ragged push
 * (every slot by its own reference length) that overlaps the prefill, so each
 * stream carries the state of decoding reference ++ generated; an
 * x-vector-only slot has no reference frames and starts at position 0.
 * out_audio[b] is the concatenation of b's chunks and starts at sample
 * n_ref_frames[b] * 1920 of the reference ++ generated decode: the
 * frame-boundary cut of qwen_tts_generate_voice_clone_stream, not the float
 * cut of the non-streamed call (they differ by at most one sample).
 * The _audio_ form encodes the reference audio first (1..16 utterances, as
 * qwen_tts_generate_voice_clone_audio_batch) and then does the same;
 * perf_first_packet_ms counts from its entry, the encoders included. */
int qwen_tts_generate_voice_clone_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                               const char *const *ref_texts, const int *const *ref_codes,
                                               const int *n_ref_frames, const float *const *spk_embeds,
                                               const char *const *languages, int non_streaming, int chunk_frames,
                                               qwen_tts_batch_audio_cb cb, void *userdata, float **out_audio,
                                               int *out_samples);
int qwen_tts_generate_voice_clone_audio_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                                     const char *const *ref_texts, const float *const *ref_wavs,
                                                     const int *n_ref_samples, const char *const *languages,
                                                     const int *x_vector_only, int non_streaming, int chunk_frames,
                                                     qwen_tts_batch_audio_cb cb, void *userdata, float **out_audio,
                                                     int *out_samples);
/* Incremental codec decode of n_streams (1..QWEN_TTS_MAX_BATCH) independent
 * code sequences at once: begin, then pushes of time_steps frames for the n
 * distinct streams streams[0..n) (all at the same position), codes
 * [n][time_steps][16]; out[i] receives time_steps * 1920 samples of streams[i].
 * Returns that count, or -1 (message; nothing decoded, the streams unchanged).
 * Each stream's concatenation equals qwen_tts_codec_decode of its frames. */
int qwen_tts_codec_mstream_begin(qwen_tts_ctx_t *ctx, int n_streams, int max_frames);
int qwen_tts_codec_mstream_push(qwen_tts_ctx_t *ctx, int n, const int *streams, const int *codes, int time_steps,
                                float *const *out);
/* The same push for streams at different positions: arguments, return value
 * and refusals are qwen_tts_codec_mstream_push's without the same-position
 * one, and the capacity is each stream's own (a push in which any listed
 * stream would pass max_frames is refused, naming it; no stream changes).
 * qwen_tts_codec_mstream_reset puts one stream back to position 0 and leaves
 * the others alone: 0, or -1 with a message and nothing changed for a bad
 * stream, a reset without begin or after a re-allocation of the state. */
int qwen_tts_codec_mstream_push_any(qwen_tts_ctx_t *ctx, int n, const int *streams, const int *codes, int time_steps,
                                    float *const *out);
int qwen_tts_codec_mstream_reset(qwen_tts_ctx_t *ctx, int stream);
/* The ragged push: streams[i] advances by its own counts[i] >= 1 frames in one
 * launch sequence per internal pass, whatever n and however the counts differ.
 * codes is [n][ld_frames][16] (stream i's first counts[i] rows are read);
 * out[i] receives counts[i] * 1920 samples, nothing is written beyond them.
 * Returns the LARGEST count times 1920, or -1 with a message, nothing decoded
 * and no stream changed, for qwen_tts_codec_mstream_push_any's refusals and for
 * counts NULL, a count < 1, a count > ld_frames, or a stream that would pass
 * max_frames with its own count (named).  Equal counts decode bit for bit what
 * qwen_tts_codec_mstream_push_any decodes. */
int qwen_tts_codec_mstream_push_ragged(qwen_tts_ctx_t *ctx, int n, const int *streams, const int *codes,
                                       const int *counts, int ld_frames, float *const *out);
/* qwen_tts_generate_queue with every utterance streamed.  Prompts, admission
 * (`next`), refill, retire, tail compaction, the ctx->queue_* results,
 * per-utterance sampling and the refusal (and disarming) of armed forcing are
 * the queue's; the codes are the queue's bit for bit.  Each slot's frames go
 * through a multi-stream codec stream of its own as they are decoded, all due
 * slots in one push whatever their positions: cb(u, pcm, n, cb_userdata), u
 * the utterance's index in input order, after its frame 0 (1920 samples),
 * then one short chunk up to the call's cadence (every chunk_frames frames of
 * the loop, for all slots at once), then chunk_frames frames each, then its
 * tail.  A slot that stops is flushed before its slot is refilled and its
 * stream reset; an utterance gets no callback after its last frame.
 * out_audio[u] (malloc'd, caller frees) is the concatenation of u's chunks; no
 * codec pass runs at the end.  perf_first_packet_ms: entry -> the first
 * callback of the call; perf_codec_ms: time in the pushes (perf_talker_ms
 * excludes it).  A caller that wants the first-packet latency per utterance
 * stamps the admission in `next` and the first chunk in `cb`.  A failed push
 * fails the call with -1 (nothing returned). */
int qwen_tts_generate_queue_stream(qwen_tts_ctx_t *ctx, int nq, const char *const *texts, const char *const *speakers,
                                   const char *const *languages, int nb, qwen_tts_queue_next_cb next, void *userdata,
                                   int chunk_frames, qwen_tts_batch_audio_cb cb, void *cb_userdata, float **out_audio,
                                   int *out_samples);

/* One multi-stream codec stream's carried state saved and restored
 * (qtts_hip.h qtts_dev_codec_mstream_save / _restore; DESIGN.md 7,
 * "Snapshots").  save: a snapshot of `stream` (the stream untouched), NULL on
 * refusal; restore: `stream` continues from the snapshot's position, whatever
 * it held before and whatever begin (stream count, max_frames) is active; both
 * one launch, stream-ordered, no host wait.  -1 / NULL with a message, nothing
 * launched and nothing changed for: no begin, a bad stream, a NULL or freed
 * snapshot, a snapshot of another context, a position beyond max_frames.
 * snapshot_free releases one (NULL / already freed: nothing happens);
 * qwen_tts_free releases the device memory of its context's live snapshots
 * (they are then refused and may still be freed).  snapshot_pos: the frames
 * it stands at, -1 for a NULL, freed or orphaned one. */
typedef struct qtts_codec_snapshot qwen_tts_codec_snapshot_t;
qwen_tts_codec_snapshot_t *qwen_tts_codec_mstream_save(qwen_tts_ctx_t *ctx, int stream);
int qwen_tts_codec_mstream_restore(qwen_tts_ctx_t *ctx, int stream, const qwen_tts_codec_snapshot_t *snap);
void qwen_tts_codec_snapshot_free(qwen_tts_codec_snapshot_t *snap);
int qwen_tts_codec_snapshot_pos(const qwen_tts_codec_snapshot_t *snap);

/* Voice handles: a cloned voice made once and used by any number of later
 * calls on the same context.  A handle owns copies of the reference text ids,
 * the reference codes and the speaker x-vector, and -- for an ICL voice, made
 * by the first streamed call that uses it -- one codec snapshot of its
 * reference frames, which every later streamed call restores instead of
 * pushing the reference frames through the codec again.
 * qwen_tts_voice_create: ref_text / ref_codes [n_ref_frames][16] / spk_embed
 *   [hidden] as qwen_tts_generate_voice_clone takes them, with its checks and
 *   messages (codes or an embedding; ICL needs >= 5 reference ids, in range).
 *   No device work.  NULL on error.
 * qwen_tts_voice_create_audio: runs the 12 Hz encoder and the speaker encoder
 *   once on ref_wav (24 kHz mono), then the same; x_vector_only drops the codes.
 * qwen_tts_voice_info: the reference frames (0: x-vector only) and whether the
 *   primed snapshot exists (each may be NULL); 0, or -1 for a NULL handle.
 * qwen_tts_voice_free: releases the handle and its snapshot (also after its
 *   context was freed).
 * A handle is refused by a context other than the one that made it. */
typedef struct qwen_tts_voice qwen_tts_voice_t;
qwen_tts_voice_t *qwen_tts_voice_create(qwen_tts_ctx_t *ctx, const char *ref_text, const int *ref_codes,
                                        int n_ref_frames, const float *spk_embed);
qwen_tts_voice_t *qwen_tts_voice_create_audio(qwen_tts_ctx_t *ctx, const char *ref_text, const float *ref_wav,
                                              int n_ref_samples, int x_vector_only);
int qwen_tts_voice_info(const qwen_tts_voice_t *v, int *n_ref_frames, int *primed);
void qwen_tts_voice_free(qwen_tts_voice_t *v);
/* The voice-clone work queue: qwen_tts_generate_queue / _queue_stream with
 * utterance i spoken in voices[i] (one handle per utterance, repeats allowed)
 * through the ICL prompt of qwen_tts_generate_voice_clone.  Admission (`next`),
 * refill, retire, tail compaction, the ctx->queue_* results,
 * qwen_tts_queue_codes (generated frames only), per-utterance sampling by
 * input index and the refusal of armed forcing are the queue's; every
 * utterance's codes are those of qwen_tts_generate_voice_clone run alone.  A
 * NULL entry of voices or a handle of another context fails the call before
 * the device is touched.
 * Plain form: each utterance's codec pass at the end decodes reference ++
 *   generated codes and cuts at the float position of
 *   qwen_tts_generate_voice_clone_batch.
 * Streamed form: the call's ICL voices that have no snapshot yet are primed
 *   first (at most `nb` at a time in one ragged push, audio dropped) and saved;
 *   an admission, initial or refill, resets the slot's stream and restores its
 *   voice's snapshot (an x-vector-only voice: the reset alone).  Delivery is
 *   qwen_tts_generate_queue_stream's; out_audio[u] starts at the reference
 *   boundary (the frame-boundary cut of qwen_tts_generate_voice_clone_stream). */
int qwen_tts_generate_voice_queue(qwen_tts_ctx_t *ctx, int nq, const char *const *texts,
                                  const qwen_tts_voice_t *const *voices, const char *const *languages,
                                  int non_streaming, int nb, qwen_tts_queue_next_cb next, void *userdata,
                                  float **out_audio, int *out_samples);
int qwen_tts_generate_voice_queue_stream(qwen_tts_ctx_t *ctx, int nq, const char *const *texts,
                                         const qwen_tts_voice_t *const *voices, const char *const *languages,
                                         int non_streaming, int nb, qwen_tts_queue_next_cb next, void *userdata,
                                         int chunk_frames, qwen_tts_batch_audio_cb cb, void *cb_userdata,
                                         float **out_audio, int *out_samples);

/* Text input (the reference's TODO at c/qwen_tts.c:1071-1077,
 * its browser front end tokenizes with @huggingface/transformers,
 * web/wasm/app.js:241-267): Qwen2 byte-level BPE over the model directory's
 * vocab.json / merges.txt / tokenizer_config.json.
 * qwen_tts_tokenize: UTF-8 text (NFC) -> malloc'd ids (caller frees), NULL on
 * error with *n_ids = 0; needs no GPU.
 * qwen_tts_text_prompt: the comma-separated ids of the chat template
 * "<|im_start|>assistant\n{text}<|im_end|>\n<|im_start|>assistant\n" -- the
 * `text` argument of qwen_tts_generate* -- malloc'd, NULL on error. */
int *qwen_tts_tokenize(const char *model_dir, const char *text, int *n_ids);
char *qwen_tts_text_prompt(qwen_tts_ctx_t *ctx, const char *text);
/* the same for an instruct: the ids of "<|im_start|>user\n{instruct}<|im_end|>\n",
 * an entry of qwen_tts_set_utterance_instruct */
char *qwen_tts_instruct_prompt(qwen_tts_ctx_t *ctx, const char *instruct);

/* sizeof(qwen_tts_ctx_t) as compiled into the library (FFI layout check) */
size_t qwen_tts_abi_sizeof_ctx(void);

extern int qwen_tts_verbose;

#endif /* QWEN_TTS_H */
