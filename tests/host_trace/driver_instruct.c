/*
 * driver_instruct.c - the host trace program for the instruct arming
 * (qwen_tts_set_utterance_instruct): qwen_tts.c against the recording fake
 * device (fake_dev.c, unchanged), on a CPU.
 *
 *   driver_instruct MODEL_DIR --list          scenario names
 *   driver_instruct MODEL_DIR --trace NAME    the scenario's trace on stdout
 *   driver_instruct MODEL_DIR --sweep NAME    the fault sweep: for K = 1 .. the
 *                                             clean run's device calls, the
 *                                             scenario with the K-th call failing,
 *                                             then a clean plain generate
 *
 * Every scenario NAME has a twin NAME_plain: the same calls without the
 * instruct arming, for the test to compare the logged prompts against.
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

static qwen_tts_ctx_t *ctx;
static FILE *tr;             /* NULL during the sweep */
static int errors, n_failed, armed;
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
/* (utterances 2 and 6: no speaker -- the voice-design layout) */
static const char *const SPK[7] = {"aiden", "aiden", NULL, "aiden", "aiden", "aiden", ""};
static const char *const LANG[7] = {"english", NULL, "english", "auto", "english", "english", "english"};
#define IHEAD "151644,872,198,"
#define ITAIL ",151645,198"
static const char INS_A[] = IHEAD "501,502,503" ITAIL;                                   /* 8 ids */
static const char INS_B[] = IHEAD "61,62,63,64,65,66,67,68,69,70,71,72,73,74,75" ITAIL;  /* 20 ids */
static const char INS_ONE[] = "777";                                                     /* 1 id */
static const char *const INS7[7] = {INS_A, NULL, INS_B, INS_A, "", INS_ONE, INS_B};
static int ref_a[3 * G];
static float spk_a[1024];

static void setup(int fixed, int max_new) {
    ctx->fixed_codec_tokens = fixed;
    ctx->max_new_tokens = max_new;
    ctx->temperature = 0.9f; ctx->top_p = 1.0f; ctx->top_k = 50; ctx->repetition_penalty = 1.05f;
    ctx->subtalker_temperature = 0.9f; ctx->subtalker_top_p = 1.0f; ctx->subtalker_top_k = 50;
    ctx->sample_seed = 42;
}

static void arm_instruct(int n, const char *const *lst) {
    if (!armed) return;
    out("set_utterance_instruct -> %d\n", qwen_tts_set_utterance_instruct(ctx, n, lst));
}

static void arm_sampling(int n) {
    qwen_tts_sampling_t s[7];
    for (int i = 0; i < n; i++) {
        qwen_tts_sampling_defaults(ctx, &s[i]);
        s[i].sample_seed = 100 + i;
    }
    out("set_utterance_sampling -> %d\n", qwen_tts_set_utterance_sampling(ctx, n, s));
}

static void arm_force(void) {
    int codes[2 * G];
    for (int i = 0; i < 2 * G; i++) codes[i] = i % 3 == 0 ? -1 : (i * 29 + 5) % 2000;
    out("force_codes -> %d\n", qwen_tts_force_codes(ctx, 0, codes, 2));
}

static void report_armed_after(void) {
    out("armed after: force=%d sampling=%d instruct=%d\n", ctx->force != NULL, ctx->sampling != NULL,
        ctx->instruct != NULL);
}

static void report_out(int i, float *a, int n) {
    if (!a && n != 0) bad("output %d is NULL with %d samples", i, n);
    if (a && n <= 0) bad("output %d is set with %d samples", i, n);
    out("out %d samples=%d hash=%08x\n", i, n, a && n > 0 ? fake_fnv(a, (size_t)n * sizeof(float)) : 0);
    free(a);
}

static void report_single(const char *call, float *a, int n) {
    out("%s -> %s\n", call, a ? "audio" : "NULL");
    n_failed += !a;
    report_out(0, a, n);
    report_armed_after();
}

static void report_multi(const char *call, int rc, int n, float **a, int *ns) {
    out("%s -> %d\n", call, rc);
    n_failed += rc != 0;
    for (int i = 0; i < n; i++) report_out(i, a[i], ns[i]);
    report_armed_after();
}

/* --------------------------------------------------------------- scenarios */
/* one utterance, instruct + forced codes armed; then the call after it, which is plain */
static void sc_single(void) {
    setup(0, 12);
    const char *lst[1] = {INS_A};
    arm_instruct(1, lst);
    arm_force();
    int n = 0;
    float *a = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate", a, n);
    a = qwen_tts_generate_stream(ctx, TEXTS[0], "aiden", "english", 4, NULL, NULL, &n);
    report_single("generate_stream (after)", a, n);
}

/* a batch of 3, entry 1 NULL, per-utterance sampling armed as well */
static void sc_batch(void) {
    setup(0, 12);
    const char *lst[3] = {INS_B, NULL, INS_ONE};
    arm_instruct(3, lst);
    arm_sampling(3);
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_batch_stream(ctx, 3, TEXTS, SPK, LANG, 3, NULL, NULL, a, ns);
    report_multi("generate_batch_stream", rc, 3, a, ns);
}

/* the queue: 7 utterances on 3 slots (4 refills), indexed by input order */
static void sc_queue(void) {
    setup(0, 12);
    arm_instruct(7, INS7);
    arm_sampling(7);
    float *a[7] = {0};
    int ns[7] = {0};
    const int rc = qwen_tts_generate_queue(ctx, 7, TEXTS, SPK, LANG, 3, NULL, NULL, a, ns);
    report_multi("generate_queue", rc, 7, a, ns);
}

/* 2 instructs armed for 3 utterances and for a queue of 7: -1 before the device is touched */
static void sc_count(void) {
    setup(0, 12);
    const char *lst[2] = {INS_A, INS_B};
    float *a[7] = {0};
    int ns[7] = {0};
    arm_instruct(2, lst);
    int rc = qwen_tts_generate_batch(ctx, 3, TEXTS, SPK, LANG, a, ns);
    report_multi("generate_batch (2 instructs)", rc, 3, a, ns);
    arm_instruct(2, lst);
    rc = qwen_tts_generate_queue_stream(ctx, 7, TEXTS, SPK, LANG, 3, NULL, NULL, 2, NULL, NULL, a, ns);
    report_multi("generate_queue_stream (2 instructs)", rc, 7, a, ns);
    int n = 0;
    float *one = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate (after)", one, n);
}

/* every voice-clone entry and the voice queue refuse an armed instruct */
static void sc_clone(void) {
    setup(0, 12);
    const char *lst[1] = {INS_A};
    int n = 0;
    arm_instruct(1, lst);
    float *one = qwen_tts_generate_voice_clone(ctx, TEXTS[2], NULL, NULL, 0, spk_a, "english", 0, &n);
    report_single("generate_voice_clone", one, n);
    arm_instruct(1, lst);
    one = qwen_tts_generate_voice_clone_stream(ctx, TEXTS[2], NULL, NULL, 0, spk_a, "english", 0, 2, NULL, NULL, &n);
    report_single("generate_voice_clone_stream", one, n);
    arm_instruct(1, lst);
    static float wav[1920];
    one = qwen_tts_generate_voice_clone_audio(ctx, TEXTS[2], NULL, wav, 1920, "english", 1, 0, &n);
    report_single("generate_voice_clone_audio", one, n);
    arm_instruct(1, lst);
    one = qwen_tts_generate_voice_clone_audio_stream(ctx, TEXTS[2], NULL, wav, 1920, "english", 1, 0, 2, NULL, NULL, &n);
    report_single("generate_voice_clone_audio_stream", one, n);
    qwen_tts_voice_t *v = qwen_tts_voice_create(ctx, NULL, NULL, 0, spk_a);
    if (!v) bad("voice_create failed (no device call in it)");
    const qwen_tts_voice_t *vs[1] = {v};
    float *a[1] = {0};
    int ns[1] = {0};
    arm_instruct(1, lst);
    int rc = v ? qwen_tts_generate_voice_queue(ctx, 1, TEXTS, vs, LANG, 0, 1, NULL, NULL, a, ns) : -1;
    report_multi("generate_voice_queue", rc, 1, a, ns);
    arm_instruct(1, lst);
    rc = v ? qwen_tts_generate_voice_queue_stream(ctx, 1, TEXTS, vs, LANG, 0, 1, NULL, NULL, 2, NULL, NULL, a, ns) : -1;
    report_multi("generate_voice_queue_stream", rc, 1, a, ns);
    qwen_tts_voice_free(v);
    one = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate (after)", one, n);
}

static void sc_plain_generate(void) {
    setup(0, 12);
    int n = 0;
    float *a = qwen_tts_generate(ctx, TEXTS[0], "aiden", "english", &n);
    report_single("generate", a, n);
}

static const struct { const char *name; void (*run)(void); int armed; } SCENARIOS[] = {
    {"single", sc_single, 1}, {"single_plain", sc_single, 0},
    {"batch", sc_batch, 1}, {"batch_plain", sc_batch, 0},
    {"queue", sc_queue, 1}, {"queue_plain", sc_queue, 0},
    {"count", sc_count, 1}, {"clone", sc_clone, 1},
};
#define N_SCENARIOS ((int)(sizeof SCENARIOS / sizeof SCENARIOS[0]))

static char *run_to_text(void (*run)(void), int arm, int fail_at, int want_text) {
    char *text = NULL;
    size_t len = 0;
    FILE *f = want_text ? open_memstream(&text, &len) : NULL;
    tr = f;
    fake_trace_to(f);
    fake_reset(fail_at);
    n_failed = 0;
    armed = arm;
    run();
    fake_trace_to(NULL);
    tr = NULL;
    if (f) fclose(f);
    return text;
}

/* (what driver.c's sweep tolerates, for the calls these scenarios make) */
static int fault_tolerated(const char *scenario, const char *entry, int nth) {
    static const char *const ok[] = {"codec_timing", "codec_snapshot_pos", "enc_available", "get_drawn", "get_tap"};
    const int lock_step = strstr(scenario, "queue") == NULL;
    for (size_t i = 0; i < sizeof ok / sizeof ok[0]; i++)
        if (!strcmp(entry, ok[i])) return 1;
    if (!strcmp(entry, "poll")) return lock_step || nth == 1;
    if (!strcmp(entry, "get_codes")) return lock_step && nth == 1;
    return 0;
}

static int sweep(const char *name, void (*run)(void), int arm) {
    cur_name = name;
    cur_k = 0;
    char *base = run_to_text(sc_plain_generate, 0, 0, 1);
    run_to_text(run, arm, 0, 0);
    const int calls = fake_calls(), clean_failed = n_failed;
    for (int k = 1; k <= calls; k++) {
        cur_k = k;
        run_to_text(run, arm, k, 0);
        if (!fake_fault_hit()) bad("the run made fewer device calls than the clean one");
        else if (!clean_failed && !n_failed && !fault_tolerated(name, fake_fault_name(), fake_fault_nth()))
            bad("every call succeeded although %s (%d since begin) failed", fake_fault_name(), fake_fault_nth());
        if (ctx->force || ctx->sampling || ctx->instruct)
            bad("an arming survived the call (force %d, sampling %d, instruct %d)", ctx->force != NULL,
                ctx->sampling != NULL, ctx->instruct != NULL);
        char *again = run_to_text(sc_plain_generate, 0, 0, 1);
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
    for (int i = 0; i < 3 * G; i++) ref_a[i] = (i * 37 + 11) % 2048;
    for (int i = 0; i < 1024; i++) spk_a[i] = (float)(i % 17) * 0.01f;
    qwen_tts_verbose = 0;
    ctx = qwen_tts_load(argv[1]);
    if (!ctx) { fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    int rc = 0;
    if (!strcmp(argv[2], "--sweep")) {
        rc = sweep(SCENARIOS[si].name, SCENARIOS[si].run, SCENARIOS[si].armed);
    } else {
        /* the host's stderr lines take their place in the trace */
        setvbuf(stdout, NULL, _IOLBF, 0);
        dup2(STDOUT_FILENO, STDERR_FILENO);
        cur_name = SCENARIOS[si].name;
        tr = stdout;
        fake_trace_to(stdout);
        fake_reset(0);
        armed = SCENARIOS[si].armed;
        SCENARIOS[si].run();
        fake_trace_to(NULL);
        tr = NULL;
        fflush(stdout);
        rc = errors ? 1 : 0;
    }
    qwen_tts_free(ctx);
    return rc;
}
