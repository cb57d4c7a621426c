/*
 * driver_text_feed.c - the host trace program for incremental text input
 * (qwen_tts_generate_fed_stream / _fed_batch_stream): qwen_tts.c against the
 * recording fake device (fake_dev.c, unchanged) and the fake of the added
 * entries (fake_textfeed.c), on a CPU.
 *
 *   driver_text_feed MODEL_DIR --list          scenario names
 *   driver_text_feed MODEL_DIR --trace NAME    the scenario's trace on stdout
 *   driver_text_feed MODEL_DIR --sweep NAME    the fault sweep: the scenario with
 *                                              the K-th device call failing, for
 *                                              every K of fake_dev.c's calls and
 *                                              then of the text entries', each
 *                                              followed by a clean plain generate
 *
 * The trace holds, in order: the feed callbacks ("feed wait=W" with every
 * utterance's state, then the pushes made in it), the device calls, the gate
 * lines and the audio callbacks.
 */
#define _GNU_SOURCE
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/qwen_tts.h"
#include "fake_dev.h"
#include "fake_textfeed.h"

#define G 16

static qwen_tts_ctx_t *ctx;
static FILE *tr;             /* NULL during the sweep */
static int errors, n_failed;
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
static const int C0[9] = {2354, 2244, 2355, 4041, 2244, 11752, 13, 77, 78};
static const int C1[6] = {1111, 2222, 3333, 4444, 5555, 6666};
static const int C2[5] = {901, 902, 903, 904, 905};
static const char *const SPK[3] = {"aiden", "aiden", NULL};
static const char *const LANG[3] = {"english", NULL, "english"};
#define PLAIN "151644,77091,198,2354,2244,2355,4041,151645,198,151644,77091,198"

static void setup(int fixed, int max_new) {
    ctx->fixed_codec_tokens = fixed;
    ctx->max_new_tokens = max_new;
    ctx->temperature = 0.9f; ctx->top_p = 1.0f; ctx->top_k = 50; ctx->repetition_penalty = 1.05f;
    ctx->subtalker_temperature = 0.9f; ctx->subtalker_top_p = 1.0f; ctx->subtalker_top_k = 50;
    ctx->sample_seed = 42;
    tf_run(fixed, fixed > 0 ? fixed : max_new);
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

static void report_multi(const char *call, int rc, int n, float **a, int *ns) {
    out("%s -> %d\n", call, rc);
    n_failed += rc != 0;
    for (int i = 0; i < n; i++) report_out(i, a[i], ns[i]);
    report_armed_after();
}

static void audio_cb(int u, const float *pcm, int n, void *user) {
    (void)pcm; (void)user;
    out("audio u=%d samples=%d\n", u, n);
}

/* ------------------------------------------------------------- scripted feeds */
typedef struct {
    int nb, calls, pos[3], step;
} script_t;

static void log_cb(qwen_tts_feed_t *f, const script_t *s, int wait) {
    out("feed wait=%d", wait);
    for (int u = 0; u < s->nb; u++) {
        int t = -1, fr = -1, st = -1;
        qwen_tts_feed_state(f, u, &t, &fr, &st);
        out(" u%d=%d/%d/%d", u, t, fr, st);
    }
    out("\n");
}

static void push(qwen_tts_feed_t *f, int u, const int *ids, int n) {
    const int rc = qwen_tts_feed_ids(f, u, ids, n);
    out(" feed_ids u=%d n=%d -> %d\n", u, n, rc);
}

static void close_(qwen_tts_feed_t *f, int u) {
    const int rc = qwen_tts_feed_close(f, u);
    out(" feed_close u=%d -> %d\n", u, rc);
}

/* from position *pos of ids[0..m): the next k ids, and the close behind the last */
static void take(qwen_tts_feed_t *f, int u, const int *ids, int m, int *pos, int k) {
    if (*pos >= m) return;
    if (k > m - *pos) k = m - *pos;
    push(f, u, ids + *pos, k);
    *pos += k;
    if (*pos == m) close_(f, u);
}

/* one utterance: two ids, then three more at every wait = 1, nothing at wait = 0 */
static int feed_starve(qwen_tts_feed_t *f, int wait, void *user) {
    script_t *s = (script_t *)user;
    log_cb(f, s, wait);
    if (wait) take(f, 0, C0, 9, &s->pos[0], s->calls++ ? 3 : 2);
    return 0;
}

/* three utterances: 0 everything at once; 2 one id per callback; 1 two ids, the rest once 0 has 4 frames */
static int feed_batch(qwen_tts_feed_t *f, int wait, void *user) {
    script_t *s = (script_t *)user;
    log_cb(f, s, wait);
    int fr0 = 0;
    qwen_tts_feed_state(f, 0, NULL, &fr0, NULL);
    take(f, 0, C0, 9, &s->pos[0], 9);
    take(f, 2, C2, 5, &s->pos[2], 1);
    if (s->pos[1] == 0) take(f, 1, C1, 6, &s->pos[1], 2);
    else if (fr0 >= 4 || wait) take(f, 1, C1, 6, &s->pos[1], 6);
    return 0;
}

/* EOS mode, two utterances: everything at once, utterance 1's close withheld until a wait = 1 */
static int feed_eos(qwen_tts_feed_t *f, int wait, void *user) {
    script_t *s = (script_t *)user;
    log_cb(f, s, wait);
    if (!s->calls++) {
        take(f, 0, C0, 9, &s->pos[0], 9);
        push(f, 1, C2, 5);
        s->pos[1] = 5;
    } else if (wait) {
        close_(f, 1);
        push(f, 0, C0, 1);   /* utterance 0 has stopped by now: 0, nothing happens */
    }
    return 0;
}

/* two ids, then a wait = 1 callback that does nothing */
static int feed_idle(qwen_tts_feed_t *f, int wait, void *user) {
    script_t *s = (script_t *)user;
    log_cb(f, s, wait);
    if (!s->calls++) push(f, 0, C0, 2);
    return 0;
}

/* everything at once, then < 0 once utterance 0 has 3 frames */
static int feed_abort(qwen_tts_feed_t *f, int wait, void *user) {
    script_t *s = (script_t *)user;
    log_cb(f, s, wait);
    int fr0 = 0;
    qwen_tts_feed_state(f, 0, NULL, &fr0, NULL);
    take(f, 0, C0, 9, &s->pos[0], 9);
    take(f, 1, C1, 6, &s->pos[1], 6);
    return fr0 >= 3 ? -7 : 0;
}

/* utterance 1 closed with nothing; the bad pushes */
static int feed_empty(qwen_tts_feed_t *f, int wait, void *user) {
    script_t *s = (script_t *)user;
    log_cb(f, s, wait);
    const int oob[1] = {1 << 30};
    push(f, 5, C0, 1);
    push(f, 0, oob, 1);
    push(f, 0, C0, 2);
    close_(f, 1);
    push(f, 1, C1, 1);
    return 0;
}

/* --------------------------------------------------------------- scenarios */
static void fed(const char *call, int nb, int fixed, int max_new, int chunk, qwen_tts_text_feed_cb cb) {
    setup(fixed, max_new);
    script_t s;
    memset(&s, 0, sizeof s);
    s.nb = nb;
    float *a[3] = {0};
    int ns[3] = {0};
    const int rc = qwen_tts_generate_fed_batch_stream(ctx, nb, SPK, LANG, chunk, cb, &s, audio_cb, NULL, a, ns);
    report_multi(call, rc, nb, a, ns);
    for (int b = 0; b < nb; b++) out("held %d=%d\n", b, tf_held(b));
}

static void plain(const char *call) {
    setup(0, 12);
    int n = 0;
    float *a = qwen_tts_generate(ctx, PLAIN, "aiden", "english", &n);
    out("%s -> %s\n", call, a ? "audio" : "NULL");
    n_failed += !a;
    report_out(0, a, n);
    report_armed_after();
}

static void sc_starve(void) { fed("fed starve", 1, 8, 64, 4, feed_starve); }
static void sc_batch(void) { fed("fed batch", 3, 6, 64, 2, feed_batch); }
static void sc_eos(void) { fed("fed eos", 2, 0, 12, 4, feed_eos); }
static void sc_idle(void) { fed("fed idle", 1, 8, 64, 4, feed_idle); plain("generate (after)"); }
static void sc_abort(void) { fed("fed abort", 2, 8, 64, 4, feed_abort); plain("generate (after)"); }

static void sc_refusals(void) {
    fed("fed empty", 2, 8, 64, 4, feed_empty);
    setup(8, 64);
    int codes[2 * G];
    for (int i = 0; i < 2 * G; i++) codes[i] = (i * 29 + 5) % 2000;
    out("force_codes -> %d\n", qwen_tts_force_codes(ctx, 0, codes, 2));
    fed("fed forced", 1, 8, 64, 4, feed_starve);
    float *a[1] = {0};
    int ns[1] = {0};
    int rc = qwen_tts_generate_fed_batch_stream(ctx, 1, SPK, LANG, 4, NULL, NULL, audio_cb, NULL, a, ns);
    report_multi("fed no callback", rc, 1, a, ns);
    static float *many[65];
    static int nmany[65];
    script_t s;
    memset(&s, 0, sizeof s);
    rc = qwen_tts_generate_fed_batch_stream(ctx, 65, NULL, NULL, 4, feed_starve, &s, audio_cb, NULL, many, nmany);
    report_multi("fed 65", rc, 0, many, nmany);
    plain("generate (after)");
}

static void sc_plain_generate(void) { plain("generate"); }

static const struct { const char *name; void (*run)(void); } SCENARIOS[] = {
    {"starve", sc_starve}, {"batch", sc_batch}, {"eos", sc_eos},
    {"idle", sc_idle}, {"abort", sc_abort}, {"refusals", sc_refusals},
};
#define N_SCENARIOS ((int)(sizeof SCENARIOS / sizeof SCENARIOS[0]))

static char *run_to_text(void (*run)(void), int fail_at, int tf_fail_at, int want_text) {
    char *text = NULL;
    size_t len = 0;
    FILE *f = want_text ? open_memstream(&text, &len) : NULL;
    tr = f;
    fake_trace_to(f);
    tf_trace_to(f);
    fake_reset(fail_at);
    tf_reset(tf_fail_at);
    n_failed = 0;
    run();
    fake_trace_to(NULL);
    tf_trace_to(NULL);
    tr = NULL;
    if (f) fclose(f);
    return text;
}

/* calls whose result the host does not depend on: the wait for frame 0 (the
 * first poll of a run) and the read of the last codes after the run */
static int fault_tolerated(const char *entry, int nth) {
    return (!strcmp(entry, "poll") && nth == 1) || (!strcmp(entry, "get_codes") && nth == 1);
}

static void after_fault(const char *base, int clean_failed, int text_layer) {
    const int hit = text_layer ? tf_fault_hit() : fake_fault_hit();
    if (!hit) bad("the run made fewer device calls than the clean one");
    else if (!clean_failed && !n_failed && (text_layer || !fault_tolerated(fake_fault_name(), fake_fault_nth())))
        bad("every call succeeded although %s failed", text_layer ? "a text entry" : fake_fault_name());
    if (ctx->force || ctx->sampling || ctx->instruct) bad("an arming survived the call");
    char *again = run_to_text(sc_plain_generate, 0, 0, 1);
    if (!again || strcmp(again, base)) bad("the clean generate after it differs from the first one");
    free(again);
}

static int sweep(const char *name, void (*run)(void)) {
    cur_name = name;
    cur_k = 0;
    char *base = run_to_text(sc_plain_generate, 0, 0, 1);
    run_to_text(run, 0, 0, 0);
    const int calls = fake_calls(), tcalls = tf_calls(), clean_failed = n_failed;
    for (int k = 1; k <= calls; k++) {
        cur_k = k;
        run_to_text(run, k, 0, 0);
        after_fault(base, clean_failed, 0);
    }
    for (int k = 1; k <= tcalls; k++) {
        cur_k = -k;
        run_to_text(run, 0, k, 0);
        after_fault(base, clean_failed, 1);
    }
    free(base);
    printf("sweep %s: %d + %d device calls, %d failures\n", name, calls, tcalls, errors);
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
        tf_trace_to(stdout);
        fake_reset(0);
        tf_reset(0);
        SCENARIOS[si].run();
        fake_trace_to(NULL);
        tf_trace_to(NULL);
        tr = NULL;
        fflush(stdout);
        rc = errors ? 1 : 0;
    }
    qwen_tts_free(ctx);
    return rc;
}
