/*
 * driver.c - the host trace program: qwen_tts.c against the recording fake
 * device (fake_dev.c), on a CPU.
 *
 *   driver MODEL_DIR --list            scenario names
 *   driver MODEL_DIR --trace NAME      the scenario's trace on stdout (the host's
 *                                      own stderr lines in place)
 *   driver MODEL_DIR --sweep NAME      the fault sweep: for K = 1 .. the clean
 *                                      run's device calls, the scenario with the
 *                                      K-th call failing, then a clean generate
 *
 * A trace is the fake's call lines, then per public call: its return value,
 * every output's sample count and hash, the callbacks in order, and the ctx's
 * last_* / queue_* results.
 */
#define _GNU_SOURCE
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/qwen_tts.h"
#include "fake_dev.h"

#define G 16
#define SPF 1920

static qwen_tts_ctx_t *ctx;
static FILE *tr;             /* NULL during the sweep */
static int errors;
static const char *cur_name = "";
static int cur_k;

static void out(const char *fmt, ...) {
    if (!tr) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(tr, fmt, ap);
    va_end(ap);
}

static void bad(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "FAIL %s (fail_at %d): ", cur_name, cur_k);
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    errors++;
}

/* ------------------------------------------------------------------ inputs */
#define HEAD "151644,77091,198,"
#define TAIL ",151645,198,151644,77091,198"
static const char *const TEXTS[7] = {
    HEAD "2354,2244,2355,4041" TAIL,
    HEAD "1111,2222,3333,4444,5555,6666" TAIL,
    HEAD "901,902,903" TAIL,
    HEAD "7001,7002,7003,7004,7005,7006,7007,7008" TAIL,
    HEAD "314,159,265,358,979" TAIL,
    HEAD "27,18,28,18,28,45,90,45,23,53" TAIL,
    HEAD "4242,4243" TAIL,
};
static const char *const SPK[7] = {"aiden", "aiden", NULL, "aiden", "nobody", "aiden", NULL};
static const char *const LANG[7] = {"english", NULL, "english", "auto", "english", "english", "klingon"};
static const char REF_TEXT_A[] = HEAD "1001,1002,1003,1004,151645,198";
static const char REF_TEXT_B[] = HEAD "2001,2002,151645,198";
static int ref_a[3 * G], ref_b[5 * G];
static float spk_a[1024], spk_b[1024], wav_a[2 * SPF + 100], wav_b[4 * SPF];

static void inputs_init(void) {
    for (int i = 0; i < 3 * G; i++) ref_a[i] = (i * 37 + 11) % 2048;
    for (int i = 0; i < 5 * G; i++) ref_b[i] = (i * 53 + 7) % 2048;
    for (int i = 0; i < 1024; i++) { spk_a[i] = (float)(i % 17) * 0.01f; spk_b[i] = (float)(i % 13) * -0.02f; }
    for (int i = 0; i < 2 * SPF + 100; i++) wav_a[i] = (float)((i * 7) % 200 - 100) / 256.0f;
    for (int i = 0; i < 4 * SPF; i++) wav_b[i] = (float)((i * 13) % 300 - 150) / 512.0f;
}

static void setup(int fixed, int max_new) {
    ctx->fixed_codec_tokens = fixed;
    ctx->max_new_tokens = max_new;
    ctx->temperature = 0.9f; ctx->top_p = 1.0f; ctx->top_k = 50; ctx->repetition_penalty = 1.05f;
    ctx->subtalker_temperature = 0.9f; ctx->subtalker_top_p = 1.0f; ctx->subtalker_top_k = 50;
    ctx->sample_seed = 42;
}

/* ---------------------------------------------------------------- reporting */
static void cb_single(const float *pcm, int n, void *user) {
    (void)user;
    out("cb frames=%d rem=%d hash=%08x\n", n / SPF, n % SPF, fake_fnv(pcm, (size_t)n * sizeof(float)));
}

static void cb_batch(int u, const float *pcm, int n, void *user) {
    (void)user;
    out("cb u=%d frames=%d rem=%d hash=%08x\n", u, n / SPF, n % SPF, fake_fnv(pcm, (size_t)n * sizeof(float)));
}

/* one output: NULL with 0 samples, or a live buffer of samples > 0 (read in full, then freed) */
static void report_out(int i, float *a, int n) {
    if (!a && n != 0) bad("output %d is NULL with %d samples", i, n);
    if (a && n <= 0) bad("output %d is set with %d samples", i, n);
    out("out %d samples=%d hash=%08x\n", i, n, a && n > 0 ? fake_fnv(a, (size_t)n * sizeof(float)) : 0);
    free(a);
}

static void report_last(void) {
    int codes[13 * G];   /* (no scenario allows more than 12 frames) */
    const int n = qwen_tts_last_codes(ctx, codes, 13);
    if (n != (ctx->last_frames > 0 ? ctx->last_frames : 0)) bad("last_codes gives %d of %d frames", n, ctx->last_frames);
    out("last stop_reason=%d stop_step=%d frames=%d codes=%08x\n", ctx->last_stop_reason, ctx->last_stop_step,
        ctx->last_frames, n > 0 ? fake_fnv(codes, (size_t)n * G * sizeof(int)) : 0);
}

static void report_queue(void) {
    out("queue n=%d slots=%d frames_launched=%d refills=%d slot_frames_used=%lld rows_launched=%lld\n", ctx->queue_n,
        ctx->queue_slots, ctx->queue_frames_launched, ctx->queue_refills, ctx->queue_slot_frames_used,
        ctx->queue_rows_launched);
    for (int i = 0; i < ctx->queue_n; i++) {
        const int n = ctx->queue_frames[i];
        out("queue %d frames=%d stop_reason=%d slot=%d codes=%08x\n", i, n, ctx->queue_stop_reason[i],
            ctx->queue_slot[i],
            n > 0 && ctx->queue_codes[i] ? fake_fnv(ctx->queue_codes[i], (size_t)n * G * sizeof(int)) : 0);
    }
}

static int n_failed;   /* generate calls of the run that returned NULL / -1 */

static void report_single(const char *call, float *a, int n) {
    out("%s -> %s\n", call, a ? "audio" : "NULL");
    n_failed += !a;
    report_out(0, a, n);
    report_last();
}

static void report_multi(const char *call, int rc, int n, float **a, int *ns, int queue) {
    out("%s -> %d\n", call, rc);
    n_failed += rc != 0;
    for (int i = 0; i < n; i++) report_out(i, a[i], ns[i]);
    if (queue) report_queue();
    else report_last();
}

/* --------------------------------------------------------------- scenarios */
static void sc_generate_fixed(void) {
    setup(6, 12);
    int n = 0;
    float *a = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate", a, n);
}

static void sc_generate_eos(void) {
    setup(0, 12);
    int n = 0;
    float *a = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate", a, n);
}

static void stream_one(int chunk, int fixed) {
    setup(fixed, 12);
    int n = 0;
    float *a = qwen_tts_generate_stream(ctx, TEXTS[1], "aiden", NULL, chunk, cb_single, NULL, &n);
    report_single("generate_stream", a, n);
}
static void sc_stream_c1(void) { stream_one(1, 0); }
static void sc_stream_c4(void) { stream_one(4, 0); }
static void sc_stream_c4_fixed(void) { stream_one(4, 11); }

static void sc_batch_eos(void) {
    setup(0, 12);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_batch(ctx, 3, TEXTS, SPK, LANG, a, ns);
    report_multi("generate_batch", rc, 3, a, ns, 0);
}

static void batch_stream(int fixed) {
    setup(fixed, 12);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_batch_stream(ctx, 3, TEXTS, SPK, LANG, 3, cb_batch, NULL, a, ns);
    report_multi("generate_batch_stream", rc, 3, a, ns, 0);
}
static void sc_batch_stream_eos(void) { batch_stream(0); }
static void sc_batch_stream_fixed(void) { batch_stream(7); }

/* voice clone from codes: two ICL slots of different reference lengths and one x-vector-only slot */
static const char *const VC_RT[3] = {REF_TEXT_A, NULL, REF_TEXT_B};
static const int *const VC_CODES[3] = {ref_a, NULL, ref_b};
static const int VC_NREF[3] = {3, 0, 5};
static const float *const VC_SPK[3] = {spk_a, spk_b, NULL};

static void sc_vc_single(void) {
    setup(0, 12);
    int n = 0;
    float *a = qwen_tts_generate_voice_clone(ctx, TEXTS[2], REF_TEXT_A, ref_a, 3, spk_a, "english", 0, &n);
    report_single("generate_voice_clone", a, n);
    a = qwen_tts_generate_voice_clone(ctx, TEXTS[2], NULL, NULL, 0, spk_b, NULL, 1, &n);
    report_single("generate_voice_clone x-vector non_streaming", a, n);
}

static void sc_vc_single_stream(void) {
    setup(0, 12);
    int n = 0;
    float *a = qwen_tts_generate_voice_clone_stream(ctx, TEXTS[2], REF_TEXT_B, ref_b, 5, NULL, "english", 0, 2,
                                                    cb_single, NULL, &n);
    report_single("generate_voice_clone_stream", a, n);
}

static void sc_vc_batch(void) {
    setup(0, 12);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_voice_clone_batch(ctx, 3, TEXTS + 2, VC_RT, VC_CODES, VC_NREF, VC_SPK, LANG, 0, a, ns);
    report_multi("generate_voice_clone_batch", rc, 3, a, ns, 0);
}

static void sc_vc_batch_stream(void) {
    setup(0, 12);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_voice_clone_batch_stream(ctx, 3, TEXTS + 2, VC_RT, VC_CODES, VC_NREF, VC_SPK, LANG,
                                                              0, 3, cb_batch, NULL, a, ns);
    report_multi("generate_voice_clone_batch_stream", rc, 3, a, ns, 0);
}

/* voice clone from audio */
static const float *const VCA_WAV[3] = {wav_a, wav_b, wav_a};
static const int VCA_N[3] = {2 * SPF + 100, 4 * SPF, 2 * SPF + 100};
static const char *const VCA_RT[3] = {REF_TEXT_A, REF_TEXT_B, NULL};
static const int VCA_XO[3] = {0, 0, 1};

static void sc_vca_single(void) {
    setup(0, 12);
    int n = 0;
    float *a = qwen_tts_generate_voice_clone_audio(ctx, TEXTS[3], REF_TEXT_A, wav_a, VCA_N[0], "english", 0, 0, &n);
    report_single("generate_voice_clone_audio", a, n);
}

static void sc_vca_stream(void) {
    setup(0, 12);
    int n = 0;
    float *a = qwen_tts_generate_voice_clone_audio_stream(ctx, TEXTS[3], REF_TEXT_B, wav_b, VCA_N[1], NULL, 0, 0, 4,
                                                          cb_single, NULL, &n);
    report_single("generate_voice_clone_audio_stream", a, n);
    a = qwen_tts_generate_voice_clone_audio_stream(ctx, TEXTS[3], NULL, wav_a, VCA_N[0], NULL, 1, 0, 4, cb_single, NULL, &n);
    report_single("generate_voice_clone_audio_stream x-vector", a, n);
}

static void sc_vca_batch(void) {
    setup(0, 12);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_voice_clone_audio_batch(ctx, 3, TEXTS + 3, VCA_RT, VCA_WAV, VCA_N, LANG, VCA_XO, 0, a, ns);
    report_multi("generate_voice_clone_audio_batch", rc, 3, a, ns, 0);
}

static void sc_vca_batch_stream(void) {
    setup(0, 12);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_voice_clone_audio_batch_stream(ctx, 3, TEXTS + 3, VCA_RT, VCA_WAV, VCA_N, LANG,
                                                                    VCA_XO, 0, 3, cb_batch, NULL, a, ns);
    report_multi("generate_voice_clone_audio_batch_stream", rc, 3, a, ns, 0);
}

/* the work queue: 7 utterances on 3 slots */
typedef struct { const int *seq; int n, i; } some_t;
static int next_some(void *user) {
    some_t *s = (some_t *)user;
    return s->i < s->n ? s->seq[s->i++] : -1;
}
static const int SOME_SEQ[4] = {4, 1, 6, 0};

static void queue_case(int fixed, int max_new, const char *compact, int some, int chunk) {
    setup(fixed, max_new);
    if (compact) setenv("QTTS_QUEUE_COMPACT", compact, 1);
    else unsetenv("QTTS_QUEUE_COMPACT");
    some_t s = {SOME_SEQ, 4, 0};
    float *a[7] = {0};
    int ns[7] = {0};
    int rc;
    if (chunk)
        rc = qwen_tts_generate_queue_stream(ctx, 7, TEXTS, SPK, LANG, 3, some ? next_some : NULL, &s, chunk, cb_batch,
                                            NULL, a, ns);
    else
        rc = qwen_tts_generate_queue(ctx, 7, TEXTS, SPK, LANG, 3, some ? next_some : NULL, &s, a, ns);
    unsetenv("QTTS_QUEUE_COMPACT");
    report_multi(chunk ? "generate_queue_stream" : "generate_queue", rc, 7, a, ns, 1);
}
static void sc_queue_eos(void) { queue_case(0, 12, NULL, 0, 0); }
static void sc_queue_nocompact(void) { queue_case(0, 12, "0", 0, 0); }
static void sc_queue_fixed(void) { queue_case(4, 12, NULL, 0, 0); }
static void sc_queue_capped(void) { queue_case(0, 5, NULL, 0, 0); }
static void sc_queue_some(void) { queue_case(0, 12, NULL, 1, 0); }
static void sc_queue_stream_eos(void) { queue_case(0, 12, NULL, 0, 2); }
static void sc_queue_stream_nocompact(void) { queue_case(0, 12, "0", 0, 2); }
static void sc_queue_stream_fixed(void) { queue_case(4, 12, NULL, 0, 2); }
static void sc_queue_stream_capped(void) { queue_case(0, 5, NULL, 0, 2); }
static void sc_queue_stream_some(void) { queue_case(0, 12, NULL, 1, 2); }

/* the voice queue: handle A used twice, B once, an x-vector-only handle; a
 * second call reuses the handles the first one primed */
static void voice_queue(int chunk) {
    setup(0, 12);
    qwen_tts_voice_t *va = qwen_tts_voice_create(ctx, REF_TEXT_A, ref_a, 3, spk_a);
    qwen_tts_voice_t *vb = qwen_tts_voice_create(ctx, REF_TEXT_B, ref_b, 5, NULL);
    qwen_tts_voice_t *vx = qwen_tts_voice_create(ctx, NULL, NULL, 0, spk_b);
    out("voice_create -> %d %d %d\n", va != NULL, vb != NULL, vx != NULL);
    if (!va || !vb || !vx) bad("voice_create failed (no device call in it)");
    const qwen_tts_voice_t *vs[5] = {va, vx, va, vb, vx};
    for (int call = 0; call < 2 && va && vb && vx; call++) {
        float *a[5] = {0};
        int ns[5] = {0};
        const int nq = call ? 3 : 5, nb = 2;
        int rc;
        if (chunk)
            rc = qwen_tts_generate_voice_queue_stream(ctx, nq, TEXTS + call, vs + call, LANG, 0, nb, NULL, NULL, chunk,
                                                      cb_batch, NULL, a, ns);
        else
            rc = qwen_tts_generate_voice_queue(ctx, nq, TEXTS + call, vs + call, LANG, 0, nb, NULL, NULL, a, ns);
        report_multi(chunk ? "generate_voice_queue_stream" : "generate_voice_queue", rc, nq, a, ns, 1);
        int nr = -1, primed = -1;
        qwen_tts_voice_info(va, &nr, &primed);
        out("voice A n_ref=%d primed=%d\n", nr, primed);
    }
    qwen_tts_voice_free(va);
    qwen_tts_voice_free(vb);
    qwen_tts_voice_free(vx);
}
static void sc_voice_queue(void) { voice_queue(0); }
static void sc_voice_queue_stream(void) { voice_queue(2); }

static void sc_voice_audio_queue_stream(void) {
    setup(0, 12);
    qwen_tts_voice_t *va = qwen_tts_voice_create_audio(ctx, REF_TEXT_A, wav_a, VCA_N[0], 0);
    qwen_tts_voice_t *vx = qwen_tts_voice_create_audio(ctx, NULL, wav_b, VCA_N[1], 1);
    out("voice_create_audio -> %d %d\n", va != NULL, vx != NULL);
    n_failed += !va || !vx;
    if (va && vx) {
        const qwen_tts_voice_t *vs[3] = {vx, va, va};
        float *a[3] = {0};
        int ns[3] = {0};
        const int rc = qwen_tts_generate_voice_queue_stream(ctx, 3, TEXTS, vs, LANG, 1, 3, NULL, NULL, 3, cb_batch,
                                                            NULL, a, ns);
        report_multi("generate_voice_queue_stream", rc, 3, a, ns, 1);
    }
    qwen_tts_voice_free(va);
    qwen_tts_voice_free(vx);
}

/* forcing and taps */
static void report_armed(int slots) {
    int drawn[13 * G];
    for (int b = 0; b < slots; b++) {
        const int n = qwen_tts_last_drawn(ctx, b, drawn, 13);
        out("last_drawn %d -> %d hash=%08x\n", b, n, n > 0 ? fake_fnv(drawn, (size_t)n * G * sizeof(int)) : 0);
    }
    float lg[4] = {0};
    unsigned bits = 0;
    int id = -1;
    const int n = qwen_tts_tap_result(ctx, 0, lg, 4, &bits, &id);
    out("tap_result 0 -> %d bits=%08x drawn=%d logits=%08x\n", n, n >= 0 ? bits : 0, n >= 0 ? id : -1,
        n >= 0 ? fake_fnv(lg, sizeof lg) : 0);
}

static void force_arm(int slot, int eos_frame) {
    int codes[5 * G];
    for (int i = 0; i < 5 * G; i++) codes[i] = i % 3 == 0 ? -1 : (i * 29 + 5) % 2000;
    if (eos_frame >= 0) codes[eos_frame * G] = ctx->config.codec_eos_id;
    out("force_codes -> %d\n", qwen_tts_force_codes(ctx, slot, codes, eos_frame >= 0 ? eos_frame + 1 : 5));
    out("tap_draw -> %d\n", qwen_tts_tap_draw(ctx, slot, 1, slot == 0 ? 0 : 3));
}

static void sc_force_generate(void) {
    setup(0, 12);
    force_arm(0, 2);   /* a forced EOS at frame 2 */
    int n = 0;
    float *a = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate (forced)", a, n);
    report_armed(1);
}

static void sc_force_batch_stream(void) {
    setup(8, 12);
    force_arm(1, -1);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_batch_stream(ctx, 3, TEXTS, SPK, LANG, 3, cb_batch, NULL, a, ns);
    report_multi("generate_batch_stream (forced)", rc, 3, a, ns, 0);
    report_armed(3);
}

static void sc_force_misfit(void) {   /* a forced slot the run does not have: refused after begin */
    setup(0, 12);
    force_arm(2, -1);
    int n = 0;
    float *a = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate (forced slot 2)", a, n);
}

/* per-utterance sampling */
static void sampling_arm(int n) {
    qwen_tts_sampling_t s[7];
    for (int i = 0; i < n; i++) {
        qwen_tts_sampling_defaults(ctx, &s[i]);
        s[i].temperature = 0.5f + 0.125f * (float)i;
        s[i].top_k = 10 + i;
        s[i].sample_seed = 100 + i;
    }
    out("set_utterance_sampling -> %d\n", qwen_tts_set_utterance_sampling(ctx, n, s));
}

static void sc_sampling_batch(void) {
    setup(0, 12);
    sampling_arm(3);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_batch(ctx, 3, TEXTS, SPK, LANG, a, ns);
    report_multi("generate_batch (sampling)", rc, 3, a, ns, 0);
}

static void sc_sampling_queue(void) {
    setup(0, 12);
    sampling_arm(7);
    float *a[7] = {0};
    int ns[7] = {0};
    const int rc = qwen_tts_generate_queue(ctx, 7, TEXTS, SPK, LANG, 3, NULL, NULL, a, ns);
    report_multi("generate_queue (sampling)", rc, 7, a, ns, 1);
}

static void sc_sampling_count(void) {   /* 2 sets armed for 3 utterances */
    setup(0, 12);
    sampling_arm(2);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_batch_stream(ctx, 3, TEXTS, SPK, LANG, 3, cb_batch, NULL, a, ns);
    report_multi("generate_batch_stream (2 sampling sets)", rc, 3, a, ns, 0);
}

static void sc_both_armed(void) {
    setup(0, 12);
    force_arm(0, -1);
    sampling_arm(1);
    int n = 0;
    float *a = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate (both armed)", a, n);
    out("armed after: force=%d sampling=%d\n", ctx->force != NULL, ctx->sampling != NULL);
}

static void sc_force_before_queue(void) {
    setup(0, 12);
    force_arm(0, -1);
    float *a[7] = {0};
    int ns[7] = {0};
    int rc = qwen_tts_generate_queue(ctx, 7, TEXTS, SPK, LANG, 3, NULL, NULL, a, ns);
    report_multi("generate_queue (forcing armed)", rc, 7, a, ns, 1);
    force_arm(0, -1);
    rc = qwen_tts_generate_queue_stream(ctx, 7, TEXTS, SPK, LANG, 3, NULL, NULL, 2, cb_batch, NULL, a, ns);
    report_multi("generate_queue_stream (forcing armed)", rc, 7, a, ns, 1);
    out("armed after: force=%d sampling=%d\n", ctx->force != NULL, ctx->sampling != NULL);
}

/* what the *_abi.py tests pin as refused before the device, and the prompt refusals */
static void sc_refusals(void) {
    setup(0, 12);
    static qwen_tts_ctx_t blank;   /* a context with no device model behind it */
    static const char *tx[65];
    static const float *wv[65];
    static int nw[65];
    static float *a[65];
    static int ns[65];
    for (int i = 0; i < 65; i++) { tx[i] = "1,2,3"; wv[i] = wav_a; nw[i] = SPF; }
#define R(call) out(#call " -> %d\n", (int)(call))
    R(qwen_tts_generate_batch(&blank, 65, tx, NULL, NULL, a, ns));
    R(qwen_tts_generate_batch(ctx, 0, tx, NULL, NULL, a, ns));
    R(qwen_tts_generate_batch_stream(&blank, 65, tx, NULL, NULL, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_batch_stream(&blank, 0, tx, NULL, NULL, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_clone_batch(&blank, 65, tx, NULL, NULL, NULL, NULL, NULL, 0, a, ns));
    R(qwen_tts_generate_voice_clone_batch_stream(&blank, 65, tx, NULL, NULL, NULL, NULL, NULL, 0, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_clone_batch_stream(&blank, 0, tx, NULL, NULL, NULL, NULL, NULL, 0, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_clone_audio_batch_stream(&blank, 0, tx, NULL, wv, nw, NULL, NULL, 0, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_clone_audio_batch_stream(&blank, 17, tx, NULL, wv, nw, NULL, NULL, 0, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_clone_audio_batch(ctx, 17, tx, NULL, wv, nw, NULL, NULL, 0, a, ns));
    R(qwen_tts_generate_queue(&blank, 2, tx, NULL, NULL, 65, NULL, NULL, a, ns));
    R(qwen_tts_generate_queue_stream(&blank, 2, tx, NULL, NULL, 65, NULL, NULL, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_queue_stream(&blank, 2, tx, NULL, NULL, 0, NULL, NULL, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_queue_stream(NULL, 2, tx, NULL, NULL, 2, NULL, NULL, 4, NULL, NULL, a, ns));
    const qwen_tts_voice_t *vs[2] = {NULL, NULL};
    R(qwen_tts_generate_voice_queue(NULL, 2, tx, vs, NULL, 0, 2, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_queue(&blank, 2, tx, vs, NULL, 0, 2, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_queue(&blank, 2, tx, NULL, NULL, 0, 2, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_queue_stream(&blank, 2, tx, vs, NULL, 0, 2, NULL, NULL, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_queue_stream(&blank, 2, tx, NULL, NULL, 0, 2, NULL, NULL, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_queue_stream(&blank, 2, tx, vs, NULL, 0, 65, NULL, NULL, 4, NULL, NULL, a, ns));
    R(qwen_tts_generate_voice_queue(ctx, 2, TEXTS, vs, NULL, 0, 2, NULL, NULL, a, ns));   /* NULL handles */
    R(qwen_tts_voice_create(NULL, "1,2,3,4,5", ref_a, 1, spk_a) != NULL);
    R(qwen_tts_voice_create(&blank, "1,2,3,4,5", ref_a, 1, spk_a) != NULL);
    R(qwen_tts_voice_create_audio(&blank, "1,2,3,4,5", wav_a, SPF, 0) != NULL);
    R(qwen_tts_voice_create_audio(ctx, NULL, wav_a, SPF, 0) != NULL);           /* ICL without ref_text */
    R(qwen_tts_voice_create(ctx, NULL, NULL, 0, NULL) != NULL);                  /* neither codes nor x-vector */
    R(qwen_tts_voice_create(ctx, "1,2,3", ref_a, 3, NULL) != NULL);              /* < 5 reference ids */
    R(qwen_tts_voice_create(ctx, "1,2,3,4,999999", ref_a, 3, NULL) != NULL);     /* reference id out of range */
    R(qwen_tts_voice_info(NULL, NULL, NULL));
    R(qwen_tts_codec_mstream_save(&blank, 0) != NULL);
    R(qwen_tts_codec_mstream_restore(&blank, 0, NULL));
    R(qwen_tts_codec_snapshot_pos(NULL));
    R(qwen_tts_codec_mstream_push_ragged(&blank, 1, nw, nw, nw, 1, a));
    R(qwen_tts_force_codes(&blank, 0, nw, 1));
    R(qwen_tts_tap_draw(&blank, 0, 0, 0));
    R(qwen_tts_set_utterance_sampling(&blank, 1, NULL));
    R(qwen_tts_set_utterance_sampling(ctx, 0, NULL));
    /* prompt refusals on a live context */
    int n = 7;
    R(qwen_tts_generate(ctx, "1,2,3", NULL, NULL, &n) != NULL);                  /* < 8 ids */
    R(qwen_tts_generate(ctx, "1,2,x", NULL, NULL, &n) != NULL);                  /* not a number */
    R(qwen_tts_generate(ctx, HEAD "999999,5" TAIL, NULL, NULL, &n) != NULL);     /* id out of range */
    const char *t2[2] = {TEXTS[0], "1,2,3"};
    R(qwen_tts_generate_queue(ctx, 2, t2, NULL, NULL, 2, NULL, NULL, a, ns));
    R(qwen_tts_generate_queue(ctx, 2, TEXTS, NULL, NULL, 0, NULL, NULL, a, ns));
    ctx->max_new_tokens = 0;
    R(qwen_tts_generate(ctx, TEXTS[0], NULL, NULL, &n) != NULL);                 /* no frames allowed */
    ctx->max_new_tokens = 12;
    const char *rt[2] = {"1,2,3", NULL};
    const int *rc2[2] = {ref_a, NULL};
    const int nr2[2] = {3, 0};
    R(qwen_tts_generate_voice_clone_batch(ctx, 2, TEXTS, rt, rc2, nr2, NULL, NULL, 0, a, ns));   /* short ref text */
    const char *rt3[2] = {REF_TEXT_A, NULL};
    R(qwen_tts_generate_voice_clone_batch(ctx, 2, TEXTS, rt3, rc2, nr2, NULL, NULL, 0, a, ns));  /* slot 1 has neither */
    const char *rt4[2] = {"1,2,3,4,-5", NULL};
    R(qwen_tts_generate_voice_clone_batch(ctx, 1, TEXTS, rt4, rc2, nr2, NULL, NULL, 0, a, ns));  /* ref id out of range */
    R(qwen_tts_generate_voice_clone_audio(ctx, TEXTS[0], NULL, wav_a, SPF, NULL, 0, 0, &n) != NULL);
    R(qwen_tts_generate_voice_clone_audio_stream(ctx, TEXTS[0], "", wav_a, SPF, NULL, 0, 0, 2, NULL, NULL, &n) != NULL);
    R(qwen_tts_generate_voice_clone_audio_stream(ctx, TEXTS[0], NULL, NULL, SPF, NULL, 0, 0, 2, NULL, NULL, &n) != NULL);
#undef R
    for (int i = 0; i < 65; i++)
        if (a[i] || ns[i]) bad("a refused call left output %d set", i);
}

static const struct { const char *name; void (*run)(void); } SCENARIOS[] = {
    {"generate_fixed", sc_generate_fixed}, {"generate_eos", sc_generate_eos},
    {"stream_c1", sc_stream_c1}, {"stream_c4", sc_stream_c4}, {"stream_c4_fixed", sc_stream_c4_fixed},
    {"batch_eos", sc_batch_eos}, {"batch_stream_eos", sc_batch_stream_eos},
    {"batch_stream_fixed", sc_batch_stream_fixed},
    {"vc_single", sc_vc_single}, {"vc_single_stream", sc_vc_single_stream}, {"vc_batch", sc_vc_batch},
    {"vc_batch_stream", sc_vc_batch_stream},
    {"vca_single", sc_vca_single}, {"vca_stream", sc_vca_stream}, {"vca_batch", sc_vca_batch},
    {"vca_batch_stream", sc_vca_batch_stream},
    {"queue_eos", sc_queue_eos}, {"queue_nocompact", sc_queue_nocompact}, {"queue_fixed", sc_queue_fixed},
    {"queue_capped", sc_queue_capped}, {"queue_some", sc_queue_some},
    {"queue_stream_eos", sc_queue_stream_eos}, {"queue_stream_nocompact", sc_queue_stream_nocompact},
    {"queue_stream_fixed", sc_queue_stream_fixed}, {"queue_stream_capped", sc_queue_stream_capped},
    {"queue_stream_some", sc_queue_stream_some},
    {"voice_queue", sc_voice_queue}, {"voice_queue_stream", sc_voice_queue_stream},
    {"voice_audio_queue_stream", sc_voice_audio_queue_stream},
    {"force_generate", sc_force_generate}, {"force_batch_stream", sc_force_batch_stream},
    {"force_misfit", sc_force_misfit},
    {"sampling_batch", sc_sampling_batch}, {"sampling_queue", sc_sampling_queue},
    {"sampling_count", sc_sampling_count}, {"both_armed", sc_both_armed},
    {"force_before_queue", sc_force_before_queue}, {"refusals", sc_refusals},
};
#define N_SCENARIOS ((int)(sizeof SCENARIOS / sizeof SCENARIOS[0]))

/* one run of a scenario into a malloc'd text (NULL sink: no text) */
static char *run_to_text(void (*run)(void), int fail_at, int want_text) {
    char *text = NULL;
    size_t len = 0;
    FILE *f = want_text ? open_memstream(&text, &len) : NULL;
    tr = f;
    fake_trace_to(f);
    fake_reset(fail_at);
    n_failed = 0;
    run();
    fake_trace_to(NULL);
    tr = NULL;
    if (f) fclose(f);
    return text;
}

/* The failures a generate call may survive.  Anywhere: codec_timing (-v -v
 * only), a snapshot whose position cannot be read (taken as "not primed": the
 * voice is primed again), enc_available (its result is a bit mask), and
 * get_drawn / get_tap, this program's own calls after the run.
 * poll: a lock-step run does not look at any poll's result (a failed one leaves
 * the counts of the poll before); the queue only ignores its step-0 poll, a
 * wait: the first since qtts_dev_begin.
 * get_codes: only a lock-step run's first since qtts_dev_begin, which fills
 * last_codes after the loop (last_frames is then 0; the audio does not depend
 * on it).  Every other one -- an ICL voice's codes for the codec pass, the
 * queue's collection of a finished utterance -- must fail its call. */
static int fault_tolerated(const char *scenario, const char *entry, int nth) {
    static const char *const ok[] = {"codec_timing", "codec_snapshot_pos", "enc_available", "get_drawn", "get_tap"};
    const int lock_step = strstr(scenario, "queue") == NULL;   /* (the queue scenarios carry it in their names) */
    for (size_t i = 0; i < sizeof ok / sizeof ok[0]; i++)
        if (!strcmp(entry, ok[i])) return 1;
    if (!strcmp(entry, "poll")) return lock_step || nth == 1;
    if (!strcmp(entry, "get_codes")) return lock_step && nth == 1;
    return 0;
}

static int sweep(const char *name, void (*run)(void)) {
    cur_name = name;
    cur_k = 0;
    char *base = run_to_text(sc_generate_eos, 0, 1);
    run_to_text(run, 0, 0);
    const int calls = fake_calls(), clean_failed = n_failed;
    for (int k = 1; k <= calls; k++) {
        cur_k = k;
        run_to_text(run, k, 0);
        if (!fake_fault_hit()) bad("the run made fewer device calls than the clean one");
        else if (!clean_failed && !n_failed && !fault_tolerated(name, fake_fault_name(), fake_fault_nth()))
            bad("every call succeeded although %s (%d since begin) failed", fake_fault_name(), fake_fault_nth());
        if (ctx->force || ctx->sampling) bad("an arming survived the call (force %d, sampling %d)", ctx->force != NULL, ctx->sampling != NULL);
        char *again = run_to_text(sc_generate_eos, 0, 1);
        if (!again || strcmp(again, base)) bad("the clean generate after it differs from the first one");
        free(again);
    }
    free(base);
    printf("sweep %s: %d device calls, %d failures\n", name, calls, errors);
    return errors ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s MODEL_DIR --list | --trace NAME | --sweep NAME\n", argv[0]);
        return 2;
    }
    if (!strcmp(argv[2], "--list")) {
        for (int i = 0; i < N_SCENARIOS; i++) printf("%s\n", SCENARIOS[i].name);
        return 0;
    }
    if (argc < 4) return 2;
    int si = -1;
    for (int i = 0; i < N_SCENARIOS; i++)
        if (!strcmp(SCENARIOS[i].name, argv[3])) si = i;
    if (si < 0) { fprintf(stderr, "no scenario %s\n", argv[3]); return 2; }
    inputs_init();
    qwen_tts_verbose = 0;
    ctx = qwen_tts_load(argv[1]);
    if (!ctx) { fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    int rc = 0;
    if (!strcmp(argv[2], "--sweep")) {
        rc = sweep(SCENARIOS[si].name, SCENARIOS[si].run);
    } else {
        /* the host's stderr lines take their place in the trace */
        setvbuf(stdout, NULL, _IOLBF, 0);
        dup2(STDOUT_FILENO, STDERR_FILENO);
        cur_name = SCENARIOS[si].name;
        tr = stdout;
        fake_trace_to(stdout);
        fake_reset(0);
        SCENARIOS[si].run();
        fake_trace_to(NULL);
        tr = NULL;
        fflush(stdout);
        rc = errors ? 1 : 0;
    }
    qwen_tts_free(ctx);
    return rc;
}
